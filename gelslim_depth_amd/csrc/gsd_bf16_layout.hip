// gsd_bf16_layout.hip -- everything that builds a bf16 GEMM operand from fp32: the weight images of the convolutions and the
// first layer's im2col.
#include "gsd_bf16_pointwise.h"

namespace {

// ---- weight images ----------------------------------------------------------------------------------------------
struct WImg {
  int T, M, K, Mp, Kp;
};
WImg wimg_dims(int mode, int Cout, int Cin) {
  WImg d;
  switch (mode) {
    case 0: d.T = 9; d.M = Cout; d.K = Cin; break;           // conv3x3 forward      [t][co][ci]
    case 1: d.T = 9; d.M = Cin; d.K = Cout; break;           // conv3x3 dX           [8-t][ci][co]
    case 2: d.T = 1; d.M = Cout; d.K = Cin * 9; break;       // im2col'd first layer [co][ci*9+t]
    case 3: d.T = 1; d.M = 4 * Cout; d.K = Cin; break;       // convT forward        [(kh,kw,co)][ci]
    default: d.T = 4; d.M = Cin; d.K = Cout; break;          // convT dX             [(kh,kw)][ci][co]
  }
  d.Mp = round_up(d.M, 128);
  d.Kp = round_up(d.K, 32);
  return d;
}

__device__ __forceinline__ void weight_image_elements(int mode, const float* __restrict__ w, int Cout, int Cin, u16* __restrict__ out,
                                                      const WImg& d, long long first, long long stride) {
  const long long total = (long long)d.T * d.Mp * d.Kp;
  for (long long e = first; e < total; e += stride) {
    const int k = (int)(e % d.Kp);
    const int m = (int)((e / d.Kp) % d.Mp);
    const int t = (int)(e / ((long long)d.Kp * d.Mp));
    float v = 0.f;
    if (m < d.M && k < d.K) {
      switch (mode) {
        case 0: v = w[((size_t)m * Cin + k) * 9 + t]; break;
        case 1: v = w[((size_t)k * Cin + m) * 9 + (8 - t)]; break;
        case 2: v = w[(size_t)m * Cin * 9 + k]; break;
        case 3: { const int q = m / Cout, co = m - q * Cout; v = w[((size_t)k * Cout + co) * 4 + q]; break; }
        default: v = w[((size_t)m * Cout + k) * 4 + t]; break;
      }
    }
    out[e] = f32_to_bf16(v);
  }
}
__global__ void weight_image_kernel(int mode, const float* __restrict__ w, int Cout, int Cin, u16* __restrict__ out, WImg d) {
  weight_image_elements(mode, w, Cout, Cin, out, d, (long long)blockIdx.x * blockDim.x + threadIdx.x, (long long)gridDim.x * blockDim.x);
}
// every image of a step in one launch (blockIdx.y = job): as 43 separate launches between the convolutions they are latency,
// 10 us each
constexpr int WJOBS = 32;
constexpr int WPAIRS = 2048;   // (row, k) pairs per block: a job gets blocks in proportion to its size
struct WJob { const float* w; u16* out; int mode, Cout, Cin, first_block; WImg d; };
struct WJobs { WJob j[WJOBS]; int n; };
// A thread owns one (row m, column k) of an image, k fastest, and walks its taps: the fp32 source of a pair's taps is ONE contiguous
// run (9 floats of a 3x3 kernel, 4 of a 2x2 one) and every tap's store is coalesced over k -- an element-major walk reads
// 4 bytes at a stride of 36 and pays three 64-bit divisions per element.  ConvT forward (mode 3, m = (q, co)): the pair is
// (co, k) and its four q rows, when the image has no padded rows.
static inline __host__ __device__ int wimg_pairs(int mode, int Cout, const WImg& d) {
  return (mode == 3 && d.Mp == 4 * Cout) ? Cout * d.Kp : d.Mp * d.Kp;
}
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));   // the flat parameter arena aligns tensors to 4 bytes only
// A thread owns EIGHT consecutive k of one row: every tap's store is then 16 bytes (2-byte stores move 128 B per wave-instruction),
// and the fp32 source of a (row, k) pair's taps is still one contiguous run.
__global__ __launch_bounds__(256) void weight_images_kernel(WJobs jobs) {
  int q = 0;
  while (q + 1 < jobs.n && (int)blockIdx.x >= jobs.j[q + 1].first_block) ++q;   // (<= 32 jobs: a linear search)
  const WJob& J = jobs.j[q];
  const WImg d = J.d;
  const bool quad = J.mode == 3 && d.Mp == 4 * J.Cout;
  const int k8n = d.Kp >> 3;                                  // Kp % 32 == 0
  const int units = (quad ? J.Cout : d.Mp) * k8n;             // (row, 8 k) units of the job
  const int base = ((int)blockIdx.x - J.first_block) * (WPAIRS / 8);
  const int end = base + WPAIRS / 8 < units ? base + WPAIRS / 8 : units;
  const size_t plane = (size_t)d.Mp * d.Kp;
  for (int ue = base + threadIdx.x; ue < end; ue += 256) {
    const int m = ue / k8n, k0 = (ue - m * k8n) * 8;
    const size_t o = (size_t)m * d.Kp + k0;
    if (quad) {   // m = co; rows q * Cout + co
      float v[4][8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        f4u t4 = f4u{0.f, 0.f, 0.f, 0.f};
        if (k0 + j < d.K) t4 = *reinterpret_cast<const f4u*>(J.w + ((size_t)(k0 + j) * J.Cout + m) * 4);
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) v[qq][j] = t4[qq];
      }
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) st16(J.out + (size_t)(qq * J.Cout + m) * d.Kp + k0, pack8(v[qq]));
      continue;
    }
    switch (J.mode) {
      case 0:
      case 1: {
        float v[9][8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool in = m < d.M && k0 + j < d.K;
          const float* src = J.mode == 0 ? J.w + ((size_t)m * J.Cin + k0 + j) * 9 : J.w + ((size_t)(k0 + j) * J.Cin + m) * 9;
#pragma unroll
          for (int t = 0; t < 9; ++t) v[t][j] = in ? src[J.mode == 0 ? t : 8 - t] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) st16(J.out + t * plane + o, pack8(v[t]));
        break;
      }
      case 2: {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (m < d.M && k0 + j < d.K) ? J.w[(size_t)m * J.Cin * 9 + k0 + j] : 0.f;
        st16(J.out + o, pack8(v));
        break;
      }
      case 3: {
        float v[8];
        const int qq = m / J.Cout, co = m - qq * J.Cout;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (m < d.M && k0 + j < d.K) ? J.w[((size_t)(k0 + j) * J.Cout + co) * 4 + qq] : 0.f;
        st16(J.out + o, pack8(v));
        break;
      }
      default: {
        float v[4][8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          f4u t4 = f4u{0.f, 0.f, 0.f, 0.f};
          if (m < d.M && k0 + j < d.K) t4 = *reinterpret_cast<const f4u*>(J.w + ((size_t)m * J.Cout + k0 + j) * 4);
#pragma unroll
          for (int t = 0; t < 4; ++t) v[t][j] = t4[t];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) st16(J.out + t * plane + o, pack8(v[t]));
        break;
      }
    }
  }
}

// ---- first-layer im2col: x (N,C,H,W) fp32 -> col (N,H,W,Kp) bf16, k = c*9 + tap ---------------------------------------
__global__ __launch_bounds__(256) void im2col3x3_kernel(const float* __restrict__ x, int C, int H, int W, NhwcD col) {
  const int n = blockIdx.y;
  const int groups = col.C >> 3;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)H * W * groups) return;
  const int gk = (int)(e % groups);
  const int p = (int)(e / groups);
  const int h = p / W, wq = p - h * W;
  float f[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int k = gk * 8 + i;
    float v = 0.f;
    if (k < C * 9) {
      const int c = k / 9, t = k - c * 9;
      const int hi = h + t / 3 - 1, wi = wq + t % 3 - 1;
      if ((unsigned)hi < (unsigned)H && (unsigned)wi < (unsigned)W) v = x[(((size_t)n * C + c) * H + hi) * W + wi];
    }
    f[i] = v;
  }
  st16(col.p + ((long long)n * H * W + p) * col.pitch + gk * 8, pack8(f));
}

}  // namespace

extern "C" int64_t gsd_bf16_weight_image_size(int mode, int Cout, int Cin) {
  if (mode < 0 || mode > 4 || Cout <= 0 || Cin <= 0) return 0;
  const WImg d = wimg_dims(mode, Cout, Cin);
  return (int64_t)d.T * d.Mp * d.Kp;
}

extern "C" int gsd_bf16_weight_image(int mode, const float* w, int Cout, int Cin, void* out, void* stream) {
  GSD_REQUIRE(w && out && mode >= 0 && mode <= 4 && Cout > 0 && Cin > 0, GSD_ERR_BAD_ARG, "gsd_bf16_weight_image: bad argument");
  const WImg d = wimg_dims(mode, Cout, Cin);
  const long long total = (long long)d.T * d.Mp * d.Kp;
  const int grid = (int)(ceil_div64(total, 256) < 8192 ? ceil_div64(total, 256) : 8192);
  hipLaunchKernelGGL(weight_image_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, mode, w, Cout, Cin, (u16*)out, d);
  GSD_LAUNCH_CHECK("gsd_bf16_weight_image");
  return GSD_OK;
}

extern "C" int gsd_bf16_weight_images(const gsd_bf16_wimg_job* jobs, int n, void* stream) {
  GSD_REQUIRE(jobs && n > 0, GSD_ERR_BAD_ARG, "gsd_bf16_weight_images: bad argument");
  for (int i = 0; i < n; ++i)
    GSD_REQUIRE(jobs[i].w && jobs[i].out && jobs[i].mode >= 0 && jobs[i].mode <= 4 && jobs[i].Cout > 0 && jobs[i].Cin > 0, GSD_ERR_BAD_ARG,
                "gsd_bf16_weight_images: bad job %d", i);
  for (int base = 0; base < n; base += WJOBS) {
    WJobs a;
    a.n = n - base < WJOBS ? n - base : WJOBS;
    long long blocks = 0;
    for (int i = 0; i < a.n; ++i) {
      const gsd_bf16_wimg_job& q = jobs[base + i];
      const WImg d = wimg_dims(q.mode, q.Cout, q.Cin);
      a.j[i] = WJob{q.w, (u16*)q.out, q.mode, q.Cout, q.Cin, (int)blocks, d};
      GSD_REQUIRE((long long)d.Mp * d.Kp < 2147483647LL, GSD_ERR_UNSUPPORTED, "gsd_bf16_weight_images: image %d too large", base + i);
      blocks += ceil_div(wimg_pairs(q.mode, q.Cout, d), WPAIRS);
    }
    GSD_REQUIRE(blocks < 2147483647LL, GSD_ERR_UNSUPPORTED, "gsd_bf16_weight_images: images too large");
    hipLaunchKernelGGL(weight_images_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    GSD_LAUNCH_CHECK("gsd_bf16_weight_images");
  }
  return GSD_OK;
}

extern "C" int gsd_bf16_im2col3x3(const float* x, int N, int C, int H, int W, const gsd_nhwc* col, void* stream) {
  GSD_REQUIRE(x && N > 0 && C > 0 && H > 0 && W > 0, GSD_ERR_BAD_ARG, "gsd_bf16_im2col3x3: bad argument");
  if (int e = check_c8(col, "gsd_bf16_im2col3x3 col")) return e;
  GSD_REQUIRE(col->N == N && col->H == H && col->W == W && col->C == round_up(9 * C, 32), GSD_ERR_BAD_ARG,
              "gsd_bf16_im2col3x3: col must be (N,H,W,round_up(9*C,32))");
  GSD_REQUIRE(N <= 65535, GSD_ERR_UNSUPPORTED, "gsd_bf16_im2col3x3: N must be <= 65535");
  const long long per = (long long)H * W * (col->C / 8);
  hipLaunchKernelGGL(im2col3x3_kernel, dim3((unsigned)ceil_div64(per, 256), N), dim3(256), 0, (hipStream_t)stream, x, C, H, W,
                     to_nhwc(*col));
  GSD_LAUNCH_CHECK("gsd_bf16_im2col3x3");
  return GSD_OK;
}
