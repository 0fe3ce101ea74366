// gsd_augment.hip -- batch assembly with on-device data augmentation (include/gsd.h: gsd_gather_augment): the two
// gsd_gather_affine launches of a train step as ONE pass over the pixels, with the sample's flips / shift (image and depth,
// the same draw) and the image's gain / offset / noise applied on the way.  The random stream is gsd_augment.h's, shared
// with the host queries below.
//
// HBM-bound, no LDS traffic beyond one broadcast of the block's draws.  grid (ceil(HW/2048), Ci+Cd, B): a block is 2048
// consecutive OUTPUT elements of one plane of one sample.  A shifted or mirrored row is still a contiguous (ascending or
// descending) span of the source row, so the 64 lanes of a wave read at most two rows' worth of consecutive dwords per load
// and write consecutive dwords; rows of 427 floats are not 16-byte aligned, so only a sample whose geometry came out as the
// identity moves float4s.  The draws are derived once per block by thread 0; identity and geometry-only launches never
// evaluate the noise hash (MODE < 2), and a launch with no geometry knob and no photometry draws nothing at all.
#include "gsd_common.h"
#include "gsd_augment.h"

namespace {

struct AugDraw {
  gsd_aug_geom g;
  gsd_aug_chan p;
  unsigned long long noise_key;
};

constexpr int EPT = 8;                    // output elements per thread
constexpr int BLOCK_ELEMS = 256 * EPT;    // ... and per block

// MODE 0: y = fmaf(x, A, B);  1: gain / offset;  2: gain / offset / noise
template <int MODE>
__global__ __launch_bounds__(256) void gather_augment_kernel(const float* __restrict__ img, const float* __restrict__ dep,
                                                             const long long* __restrict__ idx, long long M, int Ci, int Cd, int H,
                                                             int W, const float* __restrict__ Ai, const float* __restrict__ Bi,
                                                             int nabi, const float* __restrict__ Ad, const float* __restrict__ Bd,
                                                             int nabd, gsd_augment aug, float* __restrict__ out_img,
                                                             float* __restrict__ out_dep, int vec_ok) {
  const int b = blockIdx.z;
  const bool is_img = (int)blockIdx.y < Ci;
  const int c = is_img ? (int)blockIdx.y : (int)blockIdx.y - Ci;
  const int C = is_img ? Ci : Cd;
  const int HW = H * W;
  const long long row = idx[b];
  float* o = (is_img ? out_img : out_dep) + ((size_t)b * C + c) * HW;
  const int e0 = blockIdx.x * BLOCK_ELEMS;
  if (row < 0 || row >= M) {   // an out-of-range index is the caller's bug: make it loud (NaN), never read OOB
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
      const int e = e0 + k * 256 + threadIdx.x;
      if (e < HW) o[e] = __builtin_nanf("");
    }
    return;
  }
  const float* s = (is_img ? img : dep) + ((size_t)row * C + c) * HW;
  const int cc = c < (is_img ? nabi : nabd) ? c : (is_img ? nabi : nabd) - 1;
  const float a = is_img ? Ai[cc] : Ad[cc], bb = is_img ? Bi[cc] : Bd[cc];
  const bool photo = MODE > 0 && is_img;
  const bool geom = aug.p_hflip > 0.f || aug.p_vflip > 0.f || aug.max_dy > 0 || aug.max_dx > 0;

  __shared__ AugDraw sd;
  int hflip = 0, vflip = 0, dy = 0, dx = 0;
  float gain = 1.f, offset = 0.f;
  uint64_t noise_key = 0;
  if (geom || photo) {   // block-uniform
    if (threadIdx.x == 0) {
      const uint64_t key = gsd_aug_key(aug.seed, aug.epoch, row);
      if (geom) sd.g = gsd_aug_geometry(aug, key);
      if (photo) sd.p = gsd_aug_channel(aug, key, c);
      if (MODE == 2 && photo) sd.noise_key = gsd_aug_noise_key(key);
    }
    __syncthreads();
    if (geom) hflip = sd.g.hflip, vflip = sd.g.vflip, dy = sd.g.dy, dx = sd.g.dx;
    if (photo) gain = sd.p.gain, offset = sd.p.offset;
    if (MODE == 2 && photo) noise_key = sd.noise_key;
  }
  const uint64_t ebase = (uint64_t)c * (uint64_t)HW;   // element index of the plane's first pixel in the OUTPUT image

  auto finish = [&](float x, int e) -> float {
    if (photo) {
      const float t = x - aug.pivot;
      x = __fadd_rn(fmaf(gain, t, aug.pivot), offset);
      if (MODE == 2) x = fmaf(aug.noise_std, gsd_aug_noise(noise_key, ebase + (uint64_t)e), x);
    }
    return fmaf(x, a, bb);
  };

  if (vec_ok && !(hflip | vflip | dy | dx)) {   // identity geometry: aligned float4s (HW % 4 == 0)
    // loads are unconditional (a chunk beyond the plane re-reads the plane's last one) and all issued before the first use
    f32x4 v[EPT / 4];
#pragma unroll
    for (int k = 0; k < EPT / 4; ++k) {
      const int e = e0 + k * 1024 + threadIdx.x * 4;
      v[k] = *reinterpret_cast<const f32x4*>(s + (e < HW ? e : HW - 4));
    }
#pragma unroll
    for (int k = 0; k < EPT / 4; ++k) {
      const int e = e0 + k * 1024 + threadIdx.x * 4;
      if (e < HW) {
        f32x4 y;
        y.x = finish(v[k].x, e);
        y.y = finish(v[k].y, e + 1);
        y.z = finish(v[k].z, e + 2);
        y.w = finish(v[k].w, e + 3);
        *reinterpret_cast<f32x4*>(o + e) = y;
      }
    }
    return;
  }
  // Output element e0 + k*256 + tid, k = 0..EPT-1.  ONE division per thread: (h, w) of the next element follow by adding
  // 256 = qW + r with a single carry (r < W).  The loads sit in no branch, so all EPT are in flight before the first use.
  const int q = 256 / W, r = 256 - q * W;   // uniform
  const int e = e0 + threadIdx.x;
  int h = (int)((unsigned)e / (unsigned)W), w = e - h * W;
  float x[EPT];
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    int hs = h - dy, ws = w - dx;
    hs = hs < 0 ? 0 : (hs > H - 1 ? H - 1 : hs);
    ws = ws < 0 ? 0 : (ws > W - 1 ? W - 1 : ws);
    if (vflip) hs = H - 1 - hs;
    if (hflip) ws = W - 1 - ws;
    x[k] = s[hs * W + ws];   // unconditional: (hs, ws) is clamped into the plane for an element beyond it, too
    w += r;
    h += q;
    if (w >= W) w -= W, ++h;
  }
#pragma unroll
  for (int k = 0; k < EPT; ++k)
    if (e + k * 256 < HW) o[e + k * 256] = finish(x[k], e + k * 256);
}

bool unit_prob(float p) { return p >= 0.f && p <= 1.f; }   // false for NaN

int check_augment(const gsd_augment* a, const char* what) {
  GSD_REQUIRE(a != nullptr, GSD_ERR_BAD_ARG, "%s: null augment", what);
  GSD_REQUIRE(unit_prob(a->p_hflip) && unit_prob(a->p_vflip), GSD_ERR_BAD_ARG, "%s: p_hflip / p_vflip must lie in [0, 1]", what);
  GSD_REQUIRE(a->max_dy >= 0 && a->max_dx >= 0 && a->max_dy <= (1 << 20) && a->max_dx <= (1 << 20), GSD_ERR_BAD_ARG,
              "%s: max_dy / max_dx must lie in [0, 2^20]", what);
  GSD_REQUIRE(a->gain >= 0.f && a->gain < 1.f, GSD_ERR_BAD_ARG, "%s: gain must lie in [0, 1)", what);
  GSD_REQUIRE(a->offset >= 0.f && isfinite(a->offset) && a->noise_std >= 0.f && isfinite(a->noise_std) && isfinite(a->pivot),
              GSD_ERR_BAD_ARG, "%s: offset / noise_std must be finite and non-negative, pivot finite", what);
  return GSD_OK;
}

}  // namespace

extern "C" int gsd_gather_augment(const float* img, const float* dep, const int64_t* idx, int64_t M, int B, int Ci, int Cd, int H,
                                  int W, const float* Ai, const float* Bi, int nabi, const float* Ad, const float* Bd, int nabd,
                                  const gsd_augment* aug, float* out_img, float* out_dep, void* stream) {
  GSD_REQUIRE(img && dep && idx && Ai && Bi && Ad && Bd && out_img && out_dep, GSD_ERR_BAD_ARG, "gsd_gather_augment: null pointer");
  GSD_REQUIRE(M > 0 && B > 0 && Ci > 0 && Cd > 0 && H > 0 && W > 0 && nabi > 0 && nabd > 0, GSD_ERR_BAD_ARG,
              "gsd_gather_augment: non-positive size");
  if (int rc = check_augment(aug, "gsd_gather_augment"); rc != GSD_OK) return rc;
  GSD_REQUIRE(Ci <= 8, GSD_ERR_UNSUPPORTED, "gsd_gather_augment: Ci %d > 8 image channels", Ci);
  GSD_REQUIRE(B <= 65535 && Ci + (int64_t)Cd <= 65535 && (int64_t)H * W < (1 << 30), GSD_ERR_UNSUPPORTED,
              "gsd_gather_augment: B, Ci + Cd must be <= 65535 and H*W < 2^30");
  const int HW = H * W;
  const dim3 grid((unsigned)ceil_div(HW, BLOCK_ELEMS), Ci + Cd, B);
  const int vec_ok = (HW % 4 == 0) && (((uintptr_t)img | (uintptr_t)dep | (uintptr_t)out_img | (uintptr_t)out_dep) & 15) == 0;
  const int mode = aug->noise_std != 0.f ? 2 : ((aug->gain != 0.f || aug->offset != 0.f) ? 1 : 0);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, img, dep, (const long long*)idx, (long long)M, Ci, Cd, H,
                       W, Ai, Bi, nabi, Ad, Bd, nabd, *aug, out_img, out_dep, vec_ok);
  };
  if (mode == 2) launch(gather_augment_kernel<2>);
  else if (mode == 1) launch(gather_augment_kernel<1>);
  else launch(gather_augment_kernel<0>);
  GSD_LAUNCH_CHECK("gsd_gather_augment");
  return GSD_OK;
}

extern "C" int gsd_augment_sample(const gsd_augment* aug, int64_t index, int Ci, gsd_augment_draw* out) {
  if (int rc = check_augment(aug, "gsd_augment_sample"); rc != GSD_OK) return rc;
  GSD_REQUIRE(out != nullptr && Ci > 0, GSD_ERR_BAD_ARG, "gsd_augment_sample: bad argument");
  GSD_REQUIRE(Ci <= 8, GSD_ERR_UNSUPPORTED, "gsd_augment_sample: Ci %d > 8 image channels", Ci);
  const uint64_t key = gsd_aug_key(aug->seed, aug->epoch, index);
  const gsd_aug_geom g = gsd_aug_geometry(*aug, key);
  out->hflip = g.hflip;
  out->vflip = g.vflip;
  out->dy = g.dy;
  out->dx = g.dx;
  for (int c = 0; c < 8; ++c) {
    out->gain[c] = 1.f;
    out->offset[c] = 0.f;
    if (c < Ci) {
      const gsd_aug_chan p = gsd_aug_channel(*aug, key, c);
      out->gain[c] = p.gain;
      out->offset[c] = p.offset;
    }
  }
  return GSD_OK;
}

extern "C" int gsd_augment_noise(const gsd_augment* aug, int64_t index, int64_t first, int64_t n, float* out) {
  if (int rc = check_augment(aug, "gsd_augment_noise"); rc != GSD_OK) return rc;
  GSD_REQUIRE(out != nullptr && first >= 0 && n >= 0, GSD_ERR_BAD_ARG, "gsd_augment_noise: bad argument");
  const uint64_t nk = gsd_aug_noise_key(gsd_aug_key(aug->seed, aug->epoch, index));
  for (int64_t i = 0; i < n; ++i) out[i] = gsd_aug_noise(nk, (uint64_t)(first + i));
  return GSD_OK;
}
