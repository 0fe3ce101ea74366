// gsd_depth_metrics.hip -- per-image depth metrics of a batch of predictions (gfx950), include/gsd.h: gsd_depth_metrics.
//
//   e = o - t (fp32).  Row n of the table describes image n alone, over its m = K*H*W elements:
//     0 sum e   1 sum |e|   2 sum e^2   3 max |e|   4 n_t   5 n_p   6 n_tp   7 sum |e| [t contact]   8 sum e^2 [t contact]
//     9 max |t - background|   10 max |o - background|   11 sum |e[h,w+1] - e[h,w]| + |e[h+1,w] - e[h,w]|   12 non-finite e
//   "contact" is gsd_depth_loss's test, |v - background| > contact_eps in fp32, on t (n_t), on o (n_p), on both (n_tp).
//
// Stage 1: a grid of (blocks per image) x N.  A block owns a run of consecutive elements of ONE image, a thread element j of it;
// it reads o and t there and at the right and the lower neighbour, exactly as depth_loss_stage1 does at scale 0: the address
// of a pair that does not exist is clamped to the element's own and the value selected afterwards, so the six loads of an
// element fly together and nothing is guarded.  The neighbours hit the cache (the tensors are read from HBM once); there is no
// LDS tile.  Stage 2: one wave per image adds that image's at most 64 partial rows, one per lane, with the xor butterfly -- a
// fixed order.  No floating-point atomics.
//
// The number of blocks per image depends on m alone, so a row is bitwise reproducible and does not depend on N or on where
// the image stands in the batch: a data-parallel pass may score the images on any rank, in any batch.
//
// Precision: every sum is fp64; |e| and e^2 are formed in fp64 from the fp32 e (both exact), the two slope summands are
// widened before they are added (exact); counts are integers per thread, doubles (exact) from the block reduction on; maxima
// are fp32 comparisons, `v > m ? v : m`, which a NaN never wins.  Contraction is off inside the kernels.
#include "gsd_common.h"

#include <math.h>

namespace {

constexpr int DM_COLS = GSD_DM_COLS;      // doubles per row, of the table and of a block's partial row
constexpr int DM_USED = 13;               // columns that carry something; the rest are written as 0
constexpr int DM_BLOCK_ELEMS = 2048;      // a block is created per this many elements of an image ...
constexpr int DM_MAX_BLOCKS = 64;         // ... up to one per lane of the second stage's wave (64 x 32 images: 8 blocks per CU)
constexpr int DM_MAX_GRID = 1 << 23;      // blocks of 256 threads a launch may hold

struct DmParams {
  long long m;       // elements per image
  long long chunk;   // ceil(m / blocks per image): consecutive elements per block
  int bpi;           // blocks per image
  int dr;            // 256 % W: columns a thread advances per iteration
  int dqh;           // (256 / W) % H: rows, modulo the image height
  int H, W;
  float background, contact_eps;
};

__device__ __forceinline__ bool dm_is_max(int q) { return q == 3 || q == 9 || q == 10; }
__device__ __forceinline__ float dm_max(float v, float m) { return v > m ? v : m; }   // a NaN v loses
__device__ __forceinline__ float dm_e_at(const char* po, const char* pt, long long off) {
  return *reinterpret_cast<const float*>(po + off) - *reinterpret_cast<const float*>(pt + off);
}

__global__ __launch_bounds__(256) void depth_metrics_stage1(const DmParams P, const float* __restrict__ o,
                                                            const float* __restrict__ t, double* __restrict__ ws) {
#pragma clang fp contract(off)
  const int H = P.H, W = P.W;
  const int n = blockIdx.x / P.bpi, b = blockIdx.x - n * P.bpi;
  long long j = (long long)b * P.chunk + threadIdx.x;
  const long long end = min((long long)(b + 1) * P.chunk, P.m);
  const float* oi = o + (long long)n * P.m;
  const float* ti = t + (long long)n * P.m;
  const long long row0 = j / W;
  int w = (int)(j - row0 * W);
  int h = (int)(row0 % H);
  const long long down = 4ll * W;
  double s_e = 0.0, s_abs = 0.0, s_sq = 0.0, s_cabs = 0.0, s_csq = 0.0, s_slope = 0.0;
  int n_t = 0, n_p = 0, n_tp = 0, n_bad = 0;
  float m_e = 0.f, m_t = 0.f, m_p = 0.f;
  for (; j < end; j += 256) {
    const float tv = ti[j], ov = oi[j];
    const float e = ov - tv;
    const float ae = fabsf(e);
    const double ed = (double)e, sq = ed * ed;
    const float dt = fabsf(tv - P.background), dp = fabsf(ov - P.background);
    const bool ct = dt > P.contact_eps, cp = dp > P.contact_eps;
    const char* po = reinterpret_cast<const char*>(oi + j);
    const char* pt = reinterpret_cast<const char*>(ti + j);
    const bool vr = w + 1 < W, vd = h + 1 < H;
    const float er = dm_e_at(po, pt, vr ? 4 : 0), edn = dm_e_at(po, pt, vd ? down : 0);
    const float gr = vr ? er - e : 0.f, gd = vd ? edn - e : 0.f;
    s_e += ed;
    s_abs += (double)ae;
    s_sq += sq;
    s_cabs += ct ? (double)ae : 0.0;
    s_csq += ct ? sq : 0.0;
    s_slope += (double)fabsf(gr) + (double)fabsf(gd);
    n_t += ct ? 1 : 0;
    n_p += cp ? 1 : 0;
    n_tp += (ct && cp) ? 1 : 0;
    n_bad += isfinite(e) ? 0 : 1;
    m_e = dm_max(ae, m_e);
    m_t = dm_max(dt, m_t);
    m_p = dm_max(dp, m_p);
    w += P.dr;
    int dh = P.dqh;
    if (w >= W) w -= W, ++dh;
    h += dh;
    if (h >= H) h -= H;
  }
  __shared__ double red[DM_USED][4];
  const double vals[DM_USED] = {s_e, s_abs, s_sq, (double)m_e, (double)n_t, (double)n_p, (double)n_tp, s_cabs, s_csq,
                                (double)m_t, (double)m_p, s_slope, (double)n_bad};
#pragma unroll
  for (int q = 0; q < DM_USED; ++q) {
    const double v = dm_is_max(q) ? gsd_wave_max(vals[q]) : wave_sum_d(vals[q]);
    if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < DM_COLS) {
    const int q = threadIdx.x;
    double v = 0.0;
    if (q < DM_USED) {
      const double r0 = red[q][0], r1 = red[q][1], r2 = red[q][2], r3 = red[q][3];
      const double a = r1 > r0 ? r1 : r0, c = r3 > r2 ? r3 : r2;
      v = dm_is_max(q) ? (c > a ? c : a) : (r0 + r1) + (r2 + r3);
    }
    ws[(size_t)blockIdx.x * DM_COLS + q] = v;
  }
}

// one wave per image: lane b holds the partial row of the image's block b (zeros beyond the last block)
__global__ __launch_bounds__(64) void depth_metrics_stage2(const double* __restrict__ ws, int bpi, double* __restrict__ table) {
#pragma clang fp contract(off)
  const int n = blockIdx.x, b = threadIdx.x;
  const double* row = ws + ((size_t)n * bpi + (b < bpi ? b : 0)) * DM_COLS;
  double tot[DM_USED];
#pragma unroll
  for (int q = 0; q < DM_USED; ++q) tot[q] = b < bpi ? row[q] : 0.0;   // sums and counts add 0; the maxima are never negative
#pragma unroll
  for (int q = 0; q < DM_USED; ++q) tot[q] = dm_is_max(q) ? gsd_wave_max(tot[q]) : wave_sum_d(tot[q]);
  if (threadIdx.x == 0) {
    double* out = table + (size_t)n * DM_COLS;
#pragma unroll
    for (int q = 0; q < DM_USED; ++q) out[q] = tot[q];
#pragma unroll
    for (int q = DM_USED; q < DM_COLS; ++q) out[q] = 0.0;
  }
}

// elements of one (K, H, W) image, or 0 when a dimension is not positive or N images of it leave int64
int64_t dm_image_elems(int N, int K, int H, int W) {
  if (N <= 0 || K <= 0 || H <= 0 || W <= 0) return 0;
  const int64_t hw = (int64_t)H * W;
  return (int64_t)N * K > INT64_MAX / hw ? 0 : (int64_t)K * hw;
}

// blocks per image: a function of the image's element count alone
int dm_blocks_per_image(int64_t m) {
  const int64_t b = ceil_div64(m, DM_BLOCK_ELEMS);
  return (int)(b < DM_MAX_BLOCKS ? b : DM_MAX_BLOCKS);
}

}   // namespace

extern "C" int64_t gsd_depth_metrics_workspace(int N, int K, int H, int W) {
  const int64_t m = dm_image_elems(N, K, H, W);
  return m > 0 ? (int64_t)N * dm_blocks_per_image(m) * DM_COLS : 0;
}

extern "C" int gsd_depth_metrics(const struct gsd_depth_metrics* spec, const float* o, const float* t, int N, int K, int H, int W,
                                 double* table, double* workspace, int64_t workspace_elems, void* stream) {
  GSD_REQUIRE(spec && o && t && table && workspace, GSD_ERR_BAD_ARG, "gsd_depth_metrics: null pointer");
  const int64_t m = dm_image_elems(N, K, H, W);
  GSD_REQUIRE(m > 0, GSD_ERR_BAD_ARG, "gsd_depth_metrics: bad dims N=%d K=%d H=%d W=%d", N, K, H, W);
  GSD_REQUIRE(spec->reserved[0] == 0 && spec->reserved[1] == 0, GSD_ERR_BAD_ARG, "gsd_depth_metrics: the reserved words must be 0");
  GSD_REQUIRE(isfinite(spec->contact_eps) && spec->contact_eps >= 0.f, GSD_ERR_BAD_ARG,
              "gsd_depth_metrics: contact_eps %g must be finite and >= 0", (double)spec->contact_eps);
  GSD_REQUIRE(isfinite(spec->background), GSD_ERR_BAD_ARG, "gsd_depth_metrics: background must be finite");
  GSD_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)table & 7) == 0, GSD_ERR_BAD_ARG,
              "gsd_depth_metrics: table and workspace must be 8-byte aligned");
  const int bpi = dm_blocks_per_image(m);
  const int64_t blocks = (int64_t)N * bpi;
  GSD_REQUIRE(blocks <= DM_MAX_GRID, GSD_ERR_UNSUPPORTED, "gsd_depth_metrics: %lld blocks (N=%d x %d per image), at most %d per launch",
              (long long)blocks, N, bpi, DM_MAX_GRID);
  GSD_REQUIRE(workspace_elems >= blocks * DM_COLS, GSD_ERR_WORKSPACE, "gsd_depth_metrics: workspace of %lld doubles, need %lld",
              (long long)workspace_elems, (long long)(blocks * DM_COLS));

  DmParams P;
  P.m = m;
  P.chunk = ceil_div64(m, bpi);
  P.bpi = bpi;
  P.dr = 256 % W;
  P.dqh = (256 / W) % H;
  P.H = H, P.W = W;
  P.background = spec->background, P.contact_eps = spec->contact_eps;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(depth_metrics_stage1, dim3((unsigned)blocks), dim3(256), 0, st, P, o, t, workspace);
  GSD_LAUNCH_CHECK("gsd_depth_metrics stage1");
  hipLaunchKernelGGL(depth_metrics_stage2, dim3(N), dim3(64), 0, st, (const double*)workspace, bpi, table);
  GSD_LAUNCH_CHECK("gsd_depth_metrics stage2");
  return GSD_OK;
}
