// dX of the network's FIRST conv3x3 (64 output channels back to the 3 input channels at 320x427), with the BatchNorm backward
// of its output applied on the fly.  Replaces, for that one layer, the dX half of aten::convolution_backward at unet.py:11
// (DoubleConv's first Conv2d in `inc`) and the apply half of aten::native_batch_norm_backward behind it: only a caller that
// wants the gradient with respect to the network's input launches it.
//
// Why its own kernel: the general dX kernels tile M (here the 3 input channels) in blocks of 16..64 rows, so at M = 3 the direct
// form would spend ~95 % of its MFMA work on padding, and it would need d_raw = scale * (dz - c1 - (raw - mean) * invstd * c2)
// materialised first (gsd_bn_bwd_apply: read 2, write 1 tensors of 1.12 GB at batch 32).  The arithmetic is small -- 27 (ci, tap)
// products per output channel and pixel, ~15 GFLOP at batch 32 -- against 2.24 GB of dz and raw to stream: HBM-bound.
//
// Form: a block owns a strip of SR output rows of one image and a column tile of up to 2 * blockDim - 2 columns; each thread
// owns two adjacent columns.  The block walks the d_raw rows r = y0-1 .. y1 (one halo row each side, mostly L2 hits: the strips
// of an image sit on one XCD) and per row
//   1. T[(ci, kh, kw)][px] = sum_co w[co][ci][kh][kw] * d_raw[co][r][px]   for its two columns (27 packed FMAs per co on
//      VGPR pairs; weights are uniform scalar loads; d_raw is formed from dz and raw as the pieces arrive);
//   2. the horizontal part of the 3x3 shift-add: column x needs T[kw = 0] of x+1 and T[kw = 2] of x-1 -- one column of each
//      neighbour, exchanged through 2 x 9 floats of LDS per thread (one barrier per row, double-buffered);
//   3. the vertical part in registers: row r adds its kh = 0 / 1 / 2 terms to output rows r-1 / r / r+1, and row r-1 is
//      complete and stored.
// Every dx element is written by exactly one thread, in a fixed summation order; no atomics, no scratch.
#include "gsd_common.h"

#include <type_traits>

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));

// The pointers are separate __restrict__ kernel arguments: the compiler then proves the per-channel loads (weights, BatchNorm
// coefficients) unclobbered by the dx stores and issues them as scalar loads instead of spending VGPRs and vector memory on them.
struct DgFirstParams {
  int N, H, W, Cout;
  int SR;       // output rows per block
  int strips;   // ceil(H / SR)
  int tiles;    // column tiles per row
  int TW;       // output columns per tile: 2 * blockDim.x - 2
};

constexpr int DF_THREADS = 256;

// columns p and p + 1 of one row, zero outside 0 .. W-1.  Branch-free (clamped addresses, then a select): the loads of a whole
// chunk of output channels stay in one basic block and fly together -- with a guarded 8-byte load per piece each channel's
// load sat in its own block and was waited for before the next one was issued (2.04 ms at batch 32 against 1.06 ms now).
__device__ __forceinline__ f32x2 df_load2(const float* row, int p, int W) {
  const float a = row[min(max(p, 0), W - 1)], b = row[min(max(p + 1, 0), W - 1)];
  f32x2 v;
  v[0] = (p >= 0 && p < W) ? a : 0.f;
  v[1] = (p + 1 >= 0 && p + 1 < W) ? b : 0.f;
  return v;
}

constexpr int DF_CH = 8;   // output channels whose pieces are loaded together

template <int CIN, bool BN>
__global__ __launch_bounds__(DF_THREADS) void dgrad3x3_first_kernel(
    const DgFirstParams P,
    const float* __restrict__ dz,    // gradient w.r.t. the BatchNorm output, ReLU mask applied (N, Cout, H, W contiguous)
    const float* __restrict__ raw,   // the conv output the BatchNorm normalised (same shape); unused without BN
    const float* __restrict__ scale, const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ c1, const float* __restrict__ c2,
    const float* __restrict__ w,     // (Cout, Cin, 3, 3)
    float* __restrict__ dx) {        // (N, Cin, H, W) contiguous
  constexpr int K3 = CIN * 3, K9 = CIN * 9;
  // [row parity][0: T[kw = 0] of the thread's first column, 1: T[kw = 2] of its second][ci * 3 + kh][thread]
  __shared__ float edge[2][2][K3][DF_THREADS];
  const int t = threadIdx.x, nt = blockDim.x;
  const int nblocks = P.N * P.strips * P.tiles;
  const int bid = xcd_swizzle(blockIdx.x, nblocks);   // the strips of an image on one XCD: halo rows from its L2
  const int tile = bid % P.tiles, rest = bid / P.tiles;
  const int strip = rest % P.strips, n = rest / P.strips;
  const int y0 = strip * P.SR, y1 = min(y0 + P.SR, P.H);
  const int p0 = tile * P.TW - 1 + 2 * t;   // the thread's two columns p0, p0 + 1 (tile column j = p - tile*TW + 1)
  const bool out0 = t > 0 && p0 < P.W;             // j = 2t is an output column for t >= 1
  const bool out1 = t + 1 < nt && p0 + 1 < P.W;    // j = 2t + 1 is one for t <= nt - 2
  const size_t plane = (size_t)P.H * P.W;
  const float* dzn = dz + (size_t)n * P.Cout * plane;
  const float* rawn = BN ? raw + (size_t)n * P.Cout * plane : nullptr;

  f32x2 acc[3][CIN];   // output rows r-1, r, r+1 of the row being read
#pragma unroll
  for (int s = 0; s < 3; ++s)
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci) acc[s][ci] = f32x2{0.f, 0.f};

  for (int r = y0 - 1; r <= y1; ++r) {
    if (r >= 0 && r < P.H) {   // (uniform) rows outside the image contribute nothing
      f32x2 T[K9];
#pragma unroll
      for (int k = 0; k < K9; ++k) T[k] = f32x2{0.f, 0.f};
      const size_t roff = (size_t)r * P.W;
      // chunks of DF_CH output channels: every load of a chunk first, then its formation and FMAs
      auto chunk = [&](int co0, auto nch) {
        constexpr int NC = decltype(nch)::value;
        f32x2 d[NC], rw[NC];
#pragma unroll
        for (int i = 0; i < NC; ++i) {
          d[i] = df_load2(dzn + (co0 + i) * plane + roff, p0, P.W);
          if (BN) rw[i] = df_load2(rawn + (co0 + i) * plane + roff, p0, P.W);
        }
#pragma unroll
        for (int i = 0; i < NC; ++i) {
          const int co = co0 + i;
          if (BN) {
            const float sc = scale[co], mu = mean[co], is = invstd[co], k1 = c1[co], k2 = c2[co];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
              const float v = sc * (d[i][e] - k1 - (rw[i][e] - mu) * is * k2);   // gsd_bn_bwd_apply's expression
              d[i][e] = (p0 + e >= 0 && p0 + e < P.W) ? v : 0.f;                   // zero padding stays zero
            }
          }
          const float* wc = w + co * K9;
#pragma unroll
          for (int k = 0; k < K9; ++k) {
            const float wk = wc[k];
            T[k] = __builtin_elementwise_fma(d[i], f32x2{wk, wk}, T[k]);
          }
        }
      };
      int co = 0;
      for (; co + DF_CH <= P.Cout; co += DF_CH) chunk(co, std::integral_constant<int, DF_CH>{});
      for (; co < P.Cout; ++co) chunk(co, std::integral_constant<int, 1>{});
      const int par = r & 1;
#pragma unroll
      for (int k3 = 0; k3 < K3; ++k3) {
        edge[par][0][k3][t] = T[k3 * 3 + 0][0];
        edge[par][1][k3][t] = T[k3 * 3 + 2][1];
      }
      __syncthreads();   // (double-buffered by row parity: the next row's writes go to the other half)
#pragma unroll
      for (int k3 = 0; k3 < K3; ++k3) {
        const float left2 = t > 0 ? edge[par][1][k3][t - 1] : 0.f;          // T[kw = 2] of column p0 - 1
        const float right0 = t + 1 < nt ? edge[par][0][k3][t + 1] : 0.f;    // T[kw = 0] of column p0 + 2
        f32x2 h;
        h[0] = (T[k3 * 3 + 0][1] + T[k3 * 3 + 1][0]) + left2;
        h[1] = (right0 + T[k3 * 3 + 1][1]) + T[k3 * 3 + 2][0];
        const int ci = k3 / 3, kh = k3 - 3 * ci;   // row r's kh term belongs to output row r + kh - 1
        acc[kh][ci] += h;
      }
    }
    const int y = r - 1;
    if (y >= y0) {
#pragma unroll
      for (int ci = 0; ci < CIN; ++ci) {
        float* o = dx + (((size_t)n * CIN + ci) * P.H + y) * P.W;
        if (out0) o[p0] = acc[0][ci][0];
        if (out1) o[p0 + 1] = acc[0][ci][1];
      }
    }
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci) {
      acc[0][ci] = acc[1][ci];
      acc[1][ci] = acc[2][ci];
      acc[2][ci] = f32x2{0.f, 0.f};
    }
  }
}

struct DfPlan {
  int threads, TW, tiles, SR, strips;
  long long blocks;
};

DfPlan plan_dgrad_first(int N, int H, int W) {
  DfPlan pl;
  const int pairs = ceil_div(W + 2, 2);   // the tile's columns plus one halo column each side, two per thread
  pl.threads = pairs >= DF_THREADS ? DF_THREADS : ceil_div(pairs, 64) * 64;
  pl.TW = 2 * pl.threads - 2;
  pl.tiles = ceil_div(W, pl.TW);
  // strips of 32 rows, halved (down to 4) until the grid fills ~4 blocks per CU: each strip re-reads 2 halo rows
  pl.SR = 32;
  while (pl.SR > 4 && (long long)N * ceil_div(H, pl.SR) * pl.tiles < 1024) pl.SR /= 2;
  pl.strips = ceil_div(H, pl.SR);
  pl.blocks = (long long)N * pl.strips * pl.tiles;
  return pl;
}

template <int CIN>
void launch_df(const DgFirstParams& P, const float* dz, const float* raw, const float* scale, const float* mean,
               const float* invstd, const float* c1, const float* c2, const float* w, float* dx, const DfPlan& pl,
               hipStream_t st) {
  if (scale != nullptr)
    hipLaunchKernelGGL((dgrad3x3_first_kernel<CIN, true>), dim3((unsigned)pl.blocks), dim3(pl.threads), 0, st, P, dz, raw,
                       scale, mean, invstd, c1, c2, w, dx);
  else
    hipLaunchKernelGGL((dgrad3x3_first_kernel<CIN, false>), dim3((unsigned)pl.blocks), dim3(pl.threads), 0, st, P, dz, raw,
                       scale, mean, invstd, c1, c2, w, dx);
}

}  // namespace

extern "C" int gsd_conv3x3_dgrad_bn_supported(int N, int H, int W, int Cin, int Cout) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
  if (Cin * 9 > 32 || Cout > 65535) return 0;
  return plan_dgrad_first(N, H, W).blocks < 2147483647LL ? 1 : 0;
}

extern "C" int gsd_conv3x3_dgrad_bn(const float* dz, const float* raw, const float* scale, const float* mean,
                                    const float* invstd, const float* c1, const float* c2, const float* w, int Cin,
                                    int Cout, float* dx, int N, int H, int W, void* stream) {
  GSD_REQUIRE(dz && w && dx, GSD_ERR_BAD_ARG, "gsd_conv3x3_dgrad_bn: null argument");
  GSD_REQUIRE(gsd_conv3x3_dgrad_bn_supported(N, H, W, Cin, Cout), GSD_ERR_UNSUPPORTED,
              "gsd_conv3x3_dgrad_bn: serves Cin * 9 <= 32 and Cout <= 65535 only (got N %d H %d W %d Cin %d Cout %d)", N, H, W,
              Cin, Cout);
  GSD_REQUIRE((scale == nullptr) == (raw == nullptr), GSD_ERR_BAD_ARG, "gsd_conv3x3_dgrad_bn: raw and scale come together");
  GSD_REQUIRE(scale == nullptr || (mean && invstd && c1 && c2), GSD_ERR_BAD_ARG,
              "gsd_conv3x3_dgrad_bn: mean, invstd, c1, c2 are required with scale");
  const DfPlan pl = plan_dgrad_first(N, H, W);
  DgFirstParams P;
  P.N = N; P.H = H; P.W = W; P.Cout = Cout;
  P.SR = pl.SR; P.strips = pl.strips; P.tiles = pl.tiles; P.TW = pl.TW;
  const hipStream_t st = (hipStream_t)stream;
  if (Cin == 1) launch_df<1>(P, dz, raw, scale, mean, invstd, c1, c2, w, dx, pl, st);
  else if (Cin == 2) launch_df<2>(P, dz, raw, scale, mean, invstd, c1, c2, w, dx, pl, st);
  else launch_df<3>(P, dz, raw, scale, mean, invstd, c1, c2, w, dx, pl, st);
  GSD_LAUNCH_CHECK("gsd_conv3x3_dgrad_bn");
  return GSD_OK;
}
