// gsd_head.hip -- the fp32 network's layers that are neither a 3x3 conv nor a ConvT (gfx950): MaxPool2d(2) of an encoder level
// and the 1x1 output conv with its weight gradient, both reading relu(bn(raw)) through the deferred affine of their source.
#include "gsd_common.h"
#include "gsd_colsum_internal.h"

// ---------------------------------------------------------------------------------------------
// MaxPool2d(2), floor mode, of relu(bn(raw))
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void maxpool2_kernel(const SrcD S, float* __restrict__ y, int C, int Hp, int Wp) {
  // grid: (ceil(Hp*Wp/256), C, N)
  const int c = blockIdx.y, n = blockIdx.z;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= Hp * Wp) return;
  const int hp = e / Wp, wp = e - hp * Wp;
  const float* b = S.p + (size_t)n * S.ns + (size_t)c * S.cs + (size_t)(2 * hp) * S.W + 2 * wp;
  float sc = 1.f, sh = 0.f;
  if (S.scale != nullptr) { sc = S.scale[c]; sh = S.shift[c]; }
  float v0 = fmaf(b[0], sc, sh), v1 = fmaf(b[1], sc, sh), v2 = fmaf(b[S.W], sc, sh), v3 = fmaf(b[S.W + 1], sc, sh);
  float m = fmaxf(fmaxf(v0, v1), fmaxf(v2, v3));
  if (S.relu) m = fmaxf(m, 0.f);
  y[(((size_t)n * C + c) * Hp + hp) * Wp + wp] = m;
}
extern "C" int gsd_maxpool2(const gsd_src* src, float* y, int N, int C, int H, int W, void* stream) {
  GSD_REQUIRE(src && src->ptr && y && N > 0 && C > 0 && H > 1 && W > 1, GSD_ERR_BAD_ARG, "gsd_maxpool2: bad argument");
  GSD_REQUIRE(src->C == C && src->H == H && src->W == W && src->off_h == 0 && src->off_w == 0, GSD_ERR_BAD_ARG,
              "gsd_maxpool2: src must be the full (C,H,W) tensor");
  if (int e = gsd_require_rows_contiguous(*src, "gsd_maxpool2 src")) return e;
  GSD_REQUIRE(N <= 65535 && C <= 65535, GSD_ERR_UNSUPPORTED, "gsd_maxpool2: N, C must be <= 65535");
  const int Hp = H / 2, Wp = W / 2;
  hipLaunchKernelGGL(maxpool2_kernel, dim3(ceil_div(Hp * Wp, 256), C, N), dim3(256), 0, (hipStream_t)stream,
                     to_srcd(*src), y, C, Hp, Wp);
  GSD_LAUNCH_CHECK("gsd_maxpool2");
  return GSD_OK;
}

// The same pool with PITCHED outputs (gsd_maxpool2_pitched): `pooled` goes to rows of pooled->w_stride floats (16-byte aligned,
// columns W/2 .. pitch-1 written 0), and with `act` the activated full-resolution tensor relu(bn(raw)) -- the skip tensor of the
// decoder -- goes to a second pitched destination on the way: one extra write, no extra read.  A thread owns columns 4k .. 4k+3
// of the source rows 2hp and 2hp+1: two unaligned 16-byte loads, two aligned 16-byte stores (act) and one 8-byte store (pooled
// columns 2k, 2k+1).  The pooled value is maxpool2_kernel's expression on the same fmaf results, act is apply_affine's.
__global__ __launch_bounds__(256) void maxpool2_pitched_kernel(const SrcD S, const DstD Pd, const DstD A, int Hp, int Wp, int rows, int K) {
  const int c = blockIdx.y, n = blockIdx.z;
  const float* const in = S.p + (size_t)n * S.ns + (size_t)c * S.cs;
  float* const po = Pd.p + (size_t)n * Pd.ns + (size_t)c * Pd.cs;
  float* const ao = A.p != nullptr ? A.p + (size_t)n * A.ns + (size_t)c * A.cs : nullptr;
  float sc = 1.f, sh = 0.f;
  if (S.scale != nullptr) { sc = S.scale[c]; sh = S.shift[c]; }
  typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
  const int total = rows * K;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
    const int hp = e / K, k = e - hp * K;
    const int w = 4 * k;
    float v[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int h = 2 * hp + r;
      const float* const b = in + (size_t)h * S.W + w;
      if (h < S.H && w + 4 <= S.W) {
        const f32x4 t = *reinterpret_cast<const f32x4u*>(b);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[r][i] = fmaf(t[i], sc, sh);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[r][i] = (h < S.H && w + i < S.W) ? fmaf(b[i], sc, sh) : 0.f;
      }
    }
    if (ao != nullptr && w < A.ws) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int h = 2 * hp + r;
        if (h >= S.H) continue;
        f32x4 d;
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = w + i < S.W ? (S.relu ? fmaxf(v[r][i], 0.f) : v[r][i]) : 0.f;
        *reinterpret_cast<f32x4*>(ao + (size_t)h * A.ws + w) = d;
      }
    }
    if (hp < Hp && 2 * k < Pd.ws) {
      float m[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        m[i] = fmaxf(fmaxf(v[0][2 * i], v[0][2 * i + 1]), fmaxf(v[1][2 * i], v[1][2 * i + 1]));
        if (S.relu) m[i] = fmaxf(m[i], 0.f);
        if (2 * k + i >= Wp) m[i] = 0.f;
      }
      *reinterpret_cast<float2*>(po + (size_t)hp * Pd.ws + 2 * k) = make_float2(m[0], m[1]);
    }
  }
}
extern "C" int gsd_maxpool2_pitched(const gsd_src* src, const gsd_dst* pooled, const gsd_dst* act, int N, void* stream) {
  GSD_REQUIRE(src && src->ptr && pooled && pooled->ptr && N > 0 && src->C > 0 && src->H > 1 && src->W > 1 && src->off_h == 0 &&
                  src->off_w == 0, GSD_ERR_BAD_ARG, "gsd_maxpool2_pitched: bad argument");
  if (int e = gsd_check_src(*src, "gsd_maxpool2_pitched src")) return e;
  if (int e = gsd_check_dst(*pooled, "gsd_maxpool2_pitched pooled", true)) return e;
  const int Hp = src->H / 2, Wp = src->W / 2;
  GSD_REQUIRE(pooled->C == src->C && pooled->H == Hp && pooled->W == Wp && pooled->off_h == 0 && pooled->off_w == 0, GSD_ERR_BAD_ARG,
              "gsd_maxpool2_pitched: pooled must be (C,H/2,W/2)");
  GSD_REQUIRE(pooled->w_stride % 4 == 0 && ((uintptr_t)pooled->ptr & 15) == 0 && pooled->c_stride % 4 == 0 && pooled->n_stride % 4 == 0,
              GSD_ERR_BAD_ARG, "gsd_maxpool2_pitched: pooled needs a 16-byte aligned base and pitch, plane and image strides %% 4 == 0");
  if (act != nullptr) {
    if (int e = gsd_check_dst(*act, "gsd_maxpool2_pitched act", true)) return e;
    GSD_REQUIRE(act->ptr && act->C == src->C && act->H == src->H && act->W == src->W && act->off_h == 0 && act->off_w == 0, GSD_ERR_BAD_ARG,
                "gsd_maxpool2_pitched: act must be the source's (C,H,W)");
    GSD_REQUIRE(act->w_stride % 4 == 0 && ((uintptr_t)act->ptr & 15) == 0 && act->c_stride % 4 == 0 && act->n_stride % 4 == 0,
                GSD_ERR_BAD_ARG, "gsd_maxpool2_pitched: act needs a 16-byte aligned base and pitch, plane and image strides %% 4 == 0");
  }
  GSD_REQUIRE(N <= 65535 && src->C <= 65535, GSD_ERR_UNSUPPORTED, "gsd_maxpool2_pitched: N, C must be <= 65535");
  // source-row pairs: with `act` also the unpaired last row of an odd H; pieces per pair: whatever covers both destinations' pitches
  const int rows = act != nullptr ? (src->H + 1) / 2 : Hp;
  const int ka = act != nullptr ? act->w_stride / 4 : 0, kp = pooled->w_stride / 2;
  const int K = ka > kp ? ka : kp;
  const int bx = ceil_div(rows * K, 256) < 64 ? ceil_div(rows * K, 256) : 64;
  hipLaunchKernelGGL(maxpool2_pitched_kernel, dim3(bx, src->C, N), dim3(256), 0, (hipStream_t)stream, to_srcd(*src), to_dstd(*pooled),
                     act != nullptr ? to_dstd(*act) : null_dstd(), Hp, Wp, rows, K);
  GSD_LAUNCH_CHECK("gsd_maxpool2_pitched");
  return GSD_OK;
}

// ---------------------------------------------------------------------------------------------
// 1x1 output conv (+bias) of relu(bn(raw))
// ---------------------------------------------------------------------------------------------
constexpr int OUTC_MAXK = 8;
__global__ __launch_bounds__(256) void conv1x1_out_kernel(const SrcD S, const float* __restrict__ w,
                                                          const float* __restrict__ b, int C, int K,
                                                          float* __restrict__ out, int HW) {
  const int n = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  float acc[OUTC_MAXK];
#pragma unroll
  for (int k = 0; k < OUTC_MAXK; ++k) acc[k] = 0.f;
  const float* base = S.p + (size_t)n * S.ns + p;
  for (int c = 0; c < C; ++c) {
    float v = base[(size_t)c * S.cs];
    if (S.scale != nullptr) v = fmaf(v, S.scale[c], S.shift[c]);
    if (S.relu) v = fmaxf(v, 0.f);
#pragma unroll
    for (int k = 0; k < OUTC_MAXK; ++k)
      if (k < K) acc[k] = fmaf(w[k * C + c], v, acc[k]);
  }
#pragma unroll
  for (int k = 0; k < OUTC_MAXK; ++k)
    if (k < K) out[((size_t)n * K + k) * HW + p] = acc[k] + (b != nullptr ? b[k] : 0.f);
}
// four consecutive pixels per thread (16-byte loads and stores): H * W % 4 == 0 and 16-byte aligned operands
__global__ __launch_bounds__(256) void conv1x1_out_vec_kernel(const SrcD S, const float* __restrict__ w,
                                                              const float* __restrict__ b, int C, int K,
                                                              float* __restrict__ out, int HW) {
  const int n = blockIdx.y;
  const int p = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (p >= HW) return;
  f32x4 acc[OUTC_MAXK];
#pragma unroll
  for (int k = 0; k < OUTC_MAXK; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* base = S.p + (size_t)n * S.ns + p;
  for (int c = 0; c < C; ++c) {
    f32x4 v = *reinterpret_cast<const f32x4*>(base + (size_t)c * S.cs);
    if (S.scale != nullptr) {
      const float sc = S.scale[c], sh = S.shift[c];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = fmaf(v[i], sc, sh);
    }
    if (S.relu) {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], 0.f);
    }
#pragma unroll
    for (int k = 0; k < OUTC_MAXK; ++k)
      if (k < K) {
        const float wk = w[k * C + c];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[k][i] = fmaf(wk, v[i], acc[k][i]);
      }
  }
#pragma unroll
  for (int k = 0; k < OUTC_MAXK; ++k)
    if (k < K) {
      const float bk = b != nullptr ? b[k] : 0.f;
      *reinterpret_cast<f32x4*>(out + ((size_t)n * K + k) * HW + p) = f32x4{acc[k][0] + bk, acc[k][1] + bk, acc[k][2] + bk, acc[k][3] + bk};
    }
}
extern "C" int gsd_conv1x1_out(const gsd_src* src, const float* w, const float* b, int C, int K, float* out, int N, int H,
                               int W, void* stream) {
  GSD_REQUIRE(src && src->ptr && w && out && N > 0 && C > 0 && K > 0 && H > 0 && W > 0, GSD_ERR_BAD_ARG,
              "gsd_conv1x1_out: bad argument");
  GSD_REQUIRE(K <= OUTC_MAXK, GSD_ERR_UNSUPPORTED, "gsd_conv1x1_out: n_classes %d > %d", K, OUTC_MAXK);
  GSD_REQUIRE(src->C == C && src->H == H && src->W == W && src->off_h == 0 && src->off_w == 0 &&
                  src->c_stride == (int64_t)H * W && src->w_stride == W,
              GSD_ERR_BAD_ARG, "gsd_conv1x1_out: src must be the full contiguous (C,H,W) tensor");
  GSD_REQUIRE(N <= 65535, GSD_ERR_UNSUPPORTED, "gsd_conv1x1_out: N must be <= 65535");
  const bool vec = (H * W) % 4 == 0 && (((uintptr_t)src->ptr | (uintptr_t)out) & 15) == 0 && src->n_stride % 4 == 0;
  if (vec)
    hipLaunchKernelGGL(conv1x1_out_vec_kernel, dim3(ceil_div(H * W, 1024), N), dim3(256), 0, (hipStream_t)stream,
                       to_srcd(*src), w, b, C, K, out, H * W);
  else
    hipLaunchKernelGGL(conv1x1_out_kernel, dim3(ceil_div(H * W, 256), N), dim3(256), 0, (hipStream_t)stream, to_srcd(*src),
                       w, b, C, K, out, H * W);
  GSD_LAUNCH_CHECK("gsd_conv1x1_out");
  return GSD_OK;
}

// dW of the output conv for n_classes > 1 (the K == 1 case comes out of gsd_bn_bwd_reduce mode 2 as its third sum):
//   dw[k][c] = sum_{n,p} dout[n,k,p] * max(0, raw[n,c,p]*scale[c] + shift[c])
// One block per (pixel chunk, channel, image) leaves K partial sums; the column sums (fp64, then fp32) finish it.
constexpr int OUTW_CHUNK = 8192;
__global__ __launch_bounds__(256) void conv1x1_out_wgrad_kernel(const float* __restrict__ raw, const float* __restrict__ scale,
                                                                const float* __restrict__ shift, const float* __restrict__ dout,
                                                                int K, int C, int HW, int chunks, float* __restrict__ partials) {
  const int chunk = blockIdx.x, c = blockIdx.y, n = blockIdx.z;
  const float sc = scale[c], sh = shift[c];
  const float* x = raw + ((size_t)n * C + c) * HW;
  const float* d = dout + (size_t)n * K * HW;
  float s[OUTC_MAXK];
#pragma unroll
  for (int k = 0; k < OUTC_MAXK; ++k) s[k] = 0.f;
  const int e_end = min((chunk + 1) * OUTW_CHUNK, HW);
  for (int e = chunk * OUTW_CHUNK + threadIdx.x; e < e_end; e += 256) {
    const float a = fmaxf(fmaf(x[e], sc, sh), 0.f);
#pragma unroll
    for (int k = 0; k < OUTC_MAXK; ++k)
      if (k < K) s[k] = fmaf(d[(size_t)k * HW + e], a, s[k]);
  }
  __shared__ float red[OUTC_MAXK][4];
#pragma unroll
  for (int k = 0; k < OUTC_MAXK; ++k) {
    const float v = wave_sum_f(s[k]);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    const int row = n * chunks + chunk;
    partials[(size_t)row * K * C + (size_t)threadIdx.x * C + c] =
        red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
  }
}
extern "C" int gsd_conv1x1_out_wgrad_rows(int N, int H, int W) {
  return (N > 0 && H > 0 && W > 0) ? N * ceil_div(H * W, OUTW_CHUNK) : 0;
}
extern "C" int gsd_conv1x1_out_wgrad(const float* raw, const float* scale, const float* shift, const float* dout, int C, int K,
                                     float* dw, float* partials, double* sums, int N, int H, int W, void* stream) {
  GSD_REQUIRE(raw && scale && shift && dout && dw && partials && sums && N > 0 && C > 0 && K > 0 && H > 0 && W > 0, GSD_ERR_BAD_ARG,
              "gsd_conv1x1_out_wgrad: bad argument");
  GSD_REQUIRE(K <= OUTC_MAXK, GSD_ERR_UNSUPPORTED, "gsd_conv1x1_out_wgrad: n_classes %d > %d", K, OUTC_MAXK);
  GSD_REQUIRE(N <= 65535 && C <= 65535, GSD_ERR_UNSUPPORTED, "gsd_conv1x1_out_wgrad: N, C must be <= 65535");
  const int chunks = ceil_div(H * W, OUTW_CHUNK), rows = N * chunks, cols = K * C;
  hipLaunchKernelGGL(conv1x1_out_wgrad_kernel, dim3(chunks, C, N), dim3(256), 0, (hipStream_t)stream, raw, scale, shift, dout, K, C,
                     H * W, chunks, partials);
  GSD_LAUNCH_CHECK("gsd_conv1x1_out_wgrad");
  return gsd_colsum_run("gsd_conv1x1_out_wgrad", partials, rows, cols, cols, 0, 1, sums, sums + cols, dw, 0, cols, stream);
}
