// gsd_bn.hip -- BatchNorm of the fp32 train step (gfx950): the ordered two-stage column sums that finish every statistic,
// forward statistics -> (mean, invstd, scale, shift) and the running statistics, the eval-mode coefficients, and the
// BatchNorm + ReLU (+ max-pool / 1x1 output conv) backward (reduce, finalize, apply).  Streaming passes along W (NCHW rows);
// reductions are two-stage and ordered (bitwise reproducible), never float atomics.
#include "gsd_common.h"
#include "gsd_colsum_internal.h"

// ---------------------------------------------------------------------------------------------
// column sums of a [rows][ncols] fp32 matrix into fp64 (two ordered stages)
// ---------------------------------------------------------------------------------------------
constexpr int RG = 64;  // row groups of stage 1 (part of the workspace contract: callers allocate (1+RG) x columns doubles)
constexpr int CS_LANES = 16;   // row lanes per block: 64 columns x 16 rows in flight, four independent partial sums each
// blockIdx.z = column range `half` (the sum | sum-of-squares halves of a conv partial row are `half_off` apart); a few
// ten thousand partial rows of 64..1024 columns: the grid is (columns/64, 64, halves) blocks of 1024 threads.
__global__ __launch_bounds__(64 * CS_LANES) void colsum_stage1(const float* __restrict__ part, int rows, int ld, int ncols,
                                                               int half_off, double* __restrict__ tmp) {
  const int col = blockIdx.x * 64 + (threadIdx.x & 63);
  const int rl = threadIdx.x >> 6;
  const int g = blockIdx.y;
  part += (size_t)blockIdx.z * half_off;
  tmp += (size_t)blockIdx.z * RG * ncols;
  const int per = (rows + RG - 1) / RG;
  const int rb = g * per, re = min(rb + per, rows);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (col < ncols) {
    int r = rb + rl;
    for (; r + 3 * CS_LANES < re; r += 4 * CS_LANES) {   // four loads in flight per thread
      const float a = part[(size_t)r * ld + col], b = part[(size_t)(r + CS_LANES) * ld + col];
      const float c = part[(size_t)(r + 2 * CS_LANES) * ld + col], d = part[(size_t)(r + 3 * CS_LANES) * ld + col];
      s0 += (double)a; s1 += (double)b; s2 += (double)c; s3 += (double)d;
    }
    for (; r < re; r += CS_LANES) s0 += (double)part[(size_t)r * ld + col];
  }
  __shared__ double red[CS_LANES][64];
  red[rl][threadIdx.x & 63] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (rl == 0 && col < ncols) {
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < CS_LANES; ++i) t += red[i][threadIdx.x];
    tmp[(size_t)g * ncols + col] = t;
  }
}
// out32 (optional): columns [c_begin, c_begin + c_count) of the FIRST half (blockIdx.y == 0) also leave as fp32
__global__ void colsum_stage2(const double* __restrict__ tmp, int ncols, double* __restrict__ sums, float* __restrict__ out32,
                              int c_begin, int c_count) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  tmp += (size_t)blockIdx.y * RG * ncols;
  sums += (size_t)blockIdx.y * ncols;
  if (col < ncols) {
    double s = 0.0;
    for (int g = 0; g < RG; ++g) s += tmp[(size_t)g * ncols + col];
    sums[col] = s;
    if (out32 != nullptr && blockIdx.y == 0 && col >= c_begin && col < c_begin + c_count) out32[col - c_begin] = (float)s;
  }
}
int gsd_colsum_run(const char* what, const float* part, int rows, int ld, int ncols, int half_off, int halves, double* sums,
                   double* tmp, float* out32, int c_begin, int c_count, void* stream) {
  auto launched = [what](int stage) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return GSD_OK;
    gsd_set_error("%s stage%d: launch failed: %s", what, stage, hipGetErrorString(e));
    return GSD_ERR_HIP;
  };
  hipLaunchKernelGGL(colsum_stage1, dim3(ceil_div(ncols, 64), RG, halves), dim3(64 * CS_LANES), 0, (hipStream_t)stream, part, rows,
                     ld, ncols, half_off, tmp);
  if (int e = launched(1)) return e;
  hipLaunchKernelGGL(colsum_stage2, dim3(ceil_div(ncols, 256), halves), dim3(256), 0, (hipStream_t)stream, tmp, ncols, sums, out32,
                     c_begin, c_count);
  return launched(2);
}

// sums layout: [0..C) sum, [C..2C) sum of squares.  tmp space lives right behind `sums`
// (caller allocates (1+RG)*2*C doubles for `sums`).
extern "C" int gsd_bn_reduce_partials(const float* partials, int rows, int Mpad, int C, double* sums, void* stream) {
  GSD_REQUIRE(partials && sums && rows > 0 && C > 0 && Mpad >= C, GSD_ERR_BAD_ARG, "gsd_bn_reduce_partials: bad argument");
  // the two halves (sum | sumsq) are Mpad apart in a partial row: two column ranges of one launch
  return gsd_colsum_run("gsd_bn_reduce_partials", partials, rows, 2 * Mpad, C, Mpad, 2, sums, sums + 2 * C, nullptr, 0, 0, stream);
}

// Per-channel sums of what a conv launch stored (the first halves of its partial rows), channels [c_begin, c_begin + c_count),
// as fp32 -- the ConvT bias gradient from the statistics epilogue of the dX launch that writes the up-sampled tensor's gradient.
extern "C" int gsd_partials_channel_sums(const float* partials, int rows, int Mpad, int C, int c_begin, int c_count, float* out,
                                         double* sums, void* stream) {
  GSD_REQUIRE(partials && sums && out && rows > 0 && C > 0 && Mpad >= C && c_begin >= 0 && c_count > 0 && c_begin + c_count <= C,
              GSD_ERR_BAD_ARG, "gsd_partials_channel_sums: bad argument");
  return gsd_colsum_run("gsd_partials_channel_sums", partials, rows, 2 * Mpad, C, Mpad, 1, sums, sums + 2 * C, out, c_begin, c_count,
                        stream);
}

// BatchNorm2d.num_batches_tracked += 1 for every layer of a train-mode forward: one launch for up to 64 int64 counters
struct counter_ptrs { long long* p[64]; };
__global__ void add_counters_kernel(counter_ptrs c, int n, long long delta) {
  const int i = threadIdx.x;
  if (i < n) *c.p[i] += delta;
}
extern "C" int gsd_add_counters(int64_t* const* counters, int n, int64_t delta, void* stream) {
  GSD_REQUIRE(counters && n > 0, GSD_ERR_BAD_ARG, "gsd_add_counters: bad argument");
  for (int base = 0; base < n; base += 64) {
    counter_ptrs c;
    const int m = n - base < 64 ? n - base : 64;
    for (int i = 0; i < m; ++i) {
      GSD_REQUIRE(counters[base + i] != nullptr, GSD_ERR_BAD_ARG, "gsd_add_counters: null counter");
      c.p[i] = (long long*)counters[base + i];
    }
    hipLaunchKernelGGL(add_counters_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, c, m, (long long)delta);
    GSD_LAUNCH_CHECK("gsd_add_counters");
  }
  return GSD_OK;
}

// ---------------------------------------------------------------------------------------------
// BatchNorm forward: statistics -> (mean, invstd, scale, shift), running statistics, eval coefficients
// ---------------------------------------------------------------------------------------------
// Non-finite guard (gsd_guard, include/gsd.h): a batch statistic that is NaN/Inf never reaches the running statistics (a
// diverged or NaN-fed step would otherwise poison eval mode for good: every consumer turns a NaN activation into 0 through
// max(., 0), so the loss can stay finite), and the step is marked so that gsd_adam_ema can skip it.
// Returns whether the running statistics may be updated: not with non-finite values, and not once an EARLIER layer of this
// step has raised the guard (behind a NaN layer the activations are all 0 -- finite, but not statistics worth keeping).
__device__ __forceinline__ bool bn_stats_finite(double mu, double var, int* guard_words, int tick) {
  const bool finite = isfinite(mu) && isfinite(var);
  if (guard_words == nullptr) return finite;
  if (!finite) guard_words[0] = tick;   // benign race: every writer stores the same tick
  return finite && guard_words[0] != tick;
}
// Channel c from its (sum, sum of squares, count): mean, invstd, the deferred affine (scale, shift), and the guarded
// running-statistics update.  The one copy of this arithmetic: the three-launch and the one-launch form are held bit-equal.
__device__ __forceinline__ void bn_finalize_channel(int c, double sum, double sumsq, double count, const float* gamma,
                                                    const float* beta, float eps, float momentum, float* running_mean,
                                                    float* running_var, float* mean, float* invstd, float* scale, float* shift,
                                                    int* guard_words, int tick) {
  const double mu = sum / count;
  double var = sumsq / count - mu * mu;  // biased (normalisation) variance
  const bool finite = bn_stats_finite(mu, var, guard_words, tick);
  if (var < 0.0) var = 0.0;
  const double is = 1.0 / sqrt(var + (double)eps);
  mean[c] = (float)mu;
  invstd[c] = (float)is;
  scale[c] = (float)((double)gamma[c] * is);
  shift[c] = (float)((double)beta[c] - mu * (double)gamma[c] * is);
  if (running_mean != nullptr && finite) {
    const double unb = count > 1.0 ? var * count / (count - 1.0) : var;
    running_mean[c] = (float)((1.0 - (double)momentum) * (double)running_mean[c] + (double)momentum * mu);
    running_var[c] = (float)((1.0 - (double)momentum) * (double)running_var[c] + (double)momentum * unb);
  }
}
__global__ void bn_finalize_kernel(const double* __restrict__ sums, int C, double count, const float* __restrict__ gamma,
                                   const float* __restrict__ beta, float eps, float momentum, float* running_mean,
                                   float* running_var, float* mean, float* invstd, float* scale, float* shift,
                                   int* guard_words, int tick) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  bn_finalize_channel(c, sums[c], sums[C + c], count, gamma, beta, eps, momentum, running_mean, running_var, mean, invstd, scale,
                      shift, guard_words, tick);
}
// One-launch forms: a block owns 16 channels; its 64 row lanes (4 per wave x 16 waves) sum the partial rows in fp64 in a
// fixed order (strided rows -> xor-shuffle inside the wave -> wave order in LDS), then 16 threads finalise.
// `sums` still receives the per-channel totals (SyncBN and the tests read them).
constexpr int RF_CH = 16, RF_LANES = 64;
template <int NV>
__device__ __forceinline__ bool rf_block_sums(const float* __restrict__ part, int rows, int ld, const int (&off)[NV], int C,
                                              double (&v)[NV]) {
  const int c = blockIdx.x * RF_CH + (threadIdx.x & (RF_CH - 1)), rl = threadIdx.x / RF_CH;
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = 0.0;
  if (c < C) {
    int r = rl;
    for (; r + 3 * RF_LANES < rows; r += 4 * RF_LANES) {   // four rows' loads in flight (thousands of rows from the stand-alone reduce kernels); same order of additions
      float f[4][NV];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int i = 0; i < NV; ++i) f[u][i] = off[i] >= 0 ? part[(size_t)(r + u * RF_LANES) * ld + off[i] + c] : 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int i = 0; i < NV; ++i)
          if (off[i] >= 0) v[i] += (double)f[u][i];
    }
    for (; r < rows; r += RF_LANES) {
#pragma unroll
      for (int i = 0; i < NV; ++i)
        if (off[i] >= 0) v[i] += (double)part[(size_t)r * ld + off[i] + c];
    }
  }
  __shared__ double red[NV][RF_LANES / 4][RF_CH];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    v[i] += __shfl_xor(v[i], 16);
    v[i] += __shfl_xor(v[i], 32);
    if ((threadIdx.x & 63) < RF_CH) red[i][threadIdx.x >> 6][threadIdx.x & 63] = v[i];
  }
  __syncthreads();
  if (threadIdx.x >= RF_CH || c >= C) return false;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    double t = 0.0;
    for (int w = 0; w < RF_LANES / 4; ++w) t += red[i][w][threadIdx.x];
    v[i] = t;
  }
  return true;
}

__global__ __launch_bounds__(1024) void bn_reduce_finalize_kernel(const float* __restrict__ part, int rows, int ld, int off2, int C,
                                                                 double* __restrict__ sums, double count, const float* gamma,
                                                                 const float* beta, float eps, float momentum, float* running_mean,
                                                                 float* running_var, float* mean, float* invstd, float* scale,
                                                                 float* shift, int* guard_words, int tick) {
  const int off[2] = {0, off2};
  double v[2];
  if (!rf_block_sums<2>(part, rows, ld, off, C, v)) return;
  const int c = blockIdx.x * RF_CH + threadIdx.x;
  sums[c] = v[0];
  sums[C + c] = v[1];
  bn_finalize_channel(c, v[0], v[1], count, gamma, beta, eps, momentum, running_mean, running_var, mean, invstd, scale, shift,
                      guard_words, tick);
}

extern "C" int gsd_bn_reduce_finalize(const float* partials, int rows, int Mpad, int C, double* sums, double count,
                                      const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                                      float* running_var, float* mean, float* invstd, float* scale, float* shift,
                                      const gsd_guard* guard, void* stream) {
  GSD_REQUIRE(partials && sums && gamma && beta && mean && invstd && scale && shift && rows > 0 && C > 0 && Mpad >= C && count > 0,
              GSD_ERR_BAD_ARG, "gsd_bn_reduce_finalize: bad argument");
  GSD_REQUIRE((running_mean == nullptr) == (running_var == nullptr), GSD_ERR_BAD_ARG,
              "gsd_bn_reduce_finalize: running stats must come together");
  hipLaunchKernelGGL(bn_reduce_finalize_kernel, dim3(ceil_div(C, RF_CH)), dim3(RF_CH * RF_LANES), 0, (hipStream_t)stream, partials, rows, 2 * Mpad,
                     Mpad, C, sums, count, gamma, beta, eps, momentum, running_mean, running_var, mean, invstd, scale, shift,
                     gsd_guard_words(guard), gsd_guard_tick(guard));
  GSD_LAUNCH_CHECK("gsd_bn_reduce_finalize");
  return GSD_OK;
}

extern "C" int gsd_bn_finalize(const double* sums, int C, double count, const float* gamma, const float* beta, float eps,
                               float momentum, float* running_mean, float* running_var, float* mean, float* invstd,
                               float* scale, float* shift, const gsd_guard* guard, void* stream) {
  GSD_REQUIRE(sums && gamma && beta && mean && invstd && scale && shift && C > 0 && count > 0, GSD_ERR_BAD_ARG,
              "gsd_bn_finalize: bad argument");
  GSD_REQUIRE((running_mean == nullptr) == (running_var == nullptr), GSD_ERR_BAD_ARG,
              "gsd_bn_finalize: running stats must come together");
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, (hipStream_t)stream, sums, C, count, gamma,
                     beta, eps, momentum, running_mean, running_var, mean, invstd, scale, shift,
                     gsd_guard_words(guard), gsd_guard_tick(guard));
  GSD_LAUNCH_CHECK("gsd_bn_finalize");
  return GSD_OK;
}

// STATS: also mean / invstd, which the backward of an eval-mode layer reads.  <false> ignores the two pointers on purpose
// (gsd_bn_eval_coeffs passes NULL): a compile-time switch, not a run-time null check, keeps the code of both forms what
// it was as two kernels.
template <bool STATS>
__global__ void bn_eval_coeffs_kernel(const float* gamma, const float* beta, const float* rm, const float* rv, float eps,
                                      int C, float* scale, float* shift, float* mean, float* invstd) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float sc = gamma[c] / sqrtf(rv[c] + eps);
  scale[c] = sc;
  shift[c] = beta[c] - rm[c] * sc;
  if (STATS) {
    mean[c] = rm[c];
    invstd[c] = 1.f / sqrtf(rv[c] + eps);
  }
}
extern "C" int gsd_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                                  const float* running_var, float eps, int C, float* scale, float* shift, void* stream) {
  GSD_REQUIRE(gamma && beta && running_mean && running_var && scale && shift && C > 0, GSD_ERR_BAD_ARG,
              "gsd_bn_eval_coeffs: bad argument");
  hipLaunchKernelGGL(bn_eval_coeffs_kernel<false>, dim3(ceil_div(C, 256)), dim3(256), 0, (hipStream_t)stream, gamma, beta,
                     running_mean, running_var, eps, C, scale, shift, (float*)nullptr, (float*)nullptr);
  GSD_LAUNCH_CHECK("gsd_bn_eval_coeffs");
  return GSD_OK;
}

extern "C" int gsd_bn_eval_coeffs_bwd(const float* gamma, const float* beta, const float* running_mean,
                                      const float* running_var, float eps, int C, float* scale, float* shift, float* mean,
                                      float* invstd, void* stream) {
  GSD_REQUIRE(gamma && beta && running_mean && running_var && scale && shift && mean && invstd && C > 0, GSD_ERR_BAD_ARG,
              "gsd_bn_eval_coeffs_bwd: bad argument");
  hipLaunchKernelGGL(bn_eval_coeffs_kernel<true>, dim3(ceil_div(C, 256)), dim3(256), 0, (hipStream_t)stream, gamma, beta,
                     running_mean, running_var, eps, C, scale, shift, mean, invstd);
  GSD_LAUNCH_CHECK("gsd_bn_eval_coeffs_bwd");
  return GSD_OK;
}

// ---------------------------------------------------------------------------------------------
// BatchNorm + ReLU (+ max-pool / 1x1 output conv) backward, pass 1
// ---------------------------------------------------------------------------------------------
constexpr int BWD_CHUNK = 8192;  // elements of one (n, c) plane handled by one block

struct BnBwdParams {
  const float* raw;
  const float* scale;
  const float* shift;
  const float* mean;
  const float* invstd;
  SrcD da;
  const float* dpool;
  const float* dout;
  const float* wout;
  int K;
  float* dz;
  float* partials;
  int N, C, H, W, chunks;
};

// The three sums of block (chunk, c, n), 256 threads, into its partial row: wave sums, the four waves through LDS in wave order,
// threads 0..2 store [sum dz | sum dz*xhat | third] of channel c.  Shared by the element-per-thread kernels; the pooling
// kernel has two sums and its own epilogue.
__device__ __forceinline__ void bn_bwd_store_sums(const BnBwdParams& P, int n, int chunk, int c, float s1, float s2, float s3) {
  __shared__ float red[3][4];
  s1 = wave_sum_f(s1);
  s2 = wave_sum_f(s2);
  s3 = wave_sum_f(s3);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = s1;
    red[1][threadIdx.x >> 6] = s2;
    red[2][threadIdx.x >> 6] = s3;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int row = n * P.chunks + chunk;
    P.partials[(size_t)row * 3 * P.C + threadIdx.x * P.C + c] =
        red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
  }
}

// Modes 0 and 2, one thread per element: the form for planes the 16-byte kernel below does not take (unaligned operands, H * W
// not a multiple of 4, mode 2 with K > 1)
template <int MODE>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const BnBwdParams P) {
  // grid: (chunks, C, N)
  const int chunk = blockIdx.x, c = blockIdx.y, n = blockIdx.z;
  const int HW = P.H * P.W;
  const size_t plane = ((size_t)n * P.C + c) * HW;
  const float sc = P.scale[c], sh = P.shift[c], mu = P.mean[c], is = P.invstd[c];
  float s1 = 0.f, s2 = 0.f, s3 = 0.f;
  const int e_end = min((chunk + 1) * BWD_CHUNK, HW);
  for (int e = chunk * BWD_CHUNK + threadIdx.x; e < e_end; e += 256) {
    const float x = P.raw[plane + e];
    const float y = fmaf(x, sc, sh);
    float g;
    if constexpr (MODE == 2) {
      g = 0.f;
      for (int k = 0; k < P.K; ++k) {
        const float d = P.dout[((size_t)n * P.K + k) * HW + e];
        g = fmaf(d, P.wout[(size_t)k * P.C + c], g);
        if (k == 0) s3 = fmaf(d, fmaxf(y, 0.f), s3);  // dW_out[0][c] (all of dW_out when K == 1; K > 1: gsd_conv1x1_out_wgrad)
      }
    } else {
      g = 0.f;
      if (P.da.p != nullptr) {
        const int h = e / P.W, w = e - h * P.W;
        g = P.da.p[(size_t)n * P.da.ns + (size_t)c * P.da.cs + (size_t)h * P.da.W + w];
      }
    }
    const float dzv = y > 0.f ? g : 0.f;
    P.dz[plane + e] = dzv;
    s1 += dzv;
    s2 = fmaf(dzv, (x - mu) * is, s2);
  }
  bn_bwd_store_sums(P, n, chunk, c, s1, s2, s3);
}

// Modes 0 and 2 with 16-byte accesses (planes of a multiple of 4 elements, 16-byte aligned operands): a thread owns four
// consecutive elements.  Same sums as the scalar kernel up to the order of addition.
template <int MODE>
__global__ __launch_bounds__(256) void bn_bwd_reduce_vec_kernel(const BnBwdParams P) {
  const int chunk = blockIdx.x, c = blockIdx.y, n = blockIdx.z;
  const int HW = P.H * P.W;
  const size_t plane = ((size_t)n * P.C + c) * HW;
  const float sc = P.scale[c], sh = P.shift[c], mu = P.mean[c], is = P.invstd[c];
  const float wo = MODE == 2 ? P.wout[c] : 0.f;
  const float* gsrc = MODE == 2 ? P.dout + (size_t)n * HW : P.da.p + (size_t)n * P.da.ns + (size_t)c * P.da.cs;
  float s1 = 0.f, s2 = 0.f, s3 = 0.f;
  const int e_end = min((chunk + 1) * BWD_CHUNK, HW);
  for (int e = chunk * BWD_CHUNK + threadIdx.x * 4; e < e_end; e += 1024) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(P.raw + plane + e);
    const f32x4 d = *reinterpret_cast<const f32x4*>(gsrc + e);
    f32x4 dz;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float y = fmaf(x[i], sc, sh);
      float g = d[i];
      if (MODE == 2) {
        s3 = fmaf(d[i], fmaxf(y, 0.f), s3);   // dW_out[0][c]
        g = d[i] * wo;
      }
      dz[i] = y > 0.f ? g : 0.f;
      s1 += dz[i];
      s2 = fmaf(dz[i], (x[i] - mu) * is, s2);
    }
    *reinterpret_cast<f32x4*>(P.dz + plane + e) = dz;
  }
  bn_bwd_store_sums(P, n, chunk, c, s1, s2, s3);
}

// Mode 1 (gradient = da + the max-pool backward of dpool), one thread per 2x2 POOLING WINDOW: its four raw values are read once
// (two 8-byte loads) and serve both the arg-max and the four dz -- an element-per-thread form re-reads the window for every
// element (measured 3.7 TB/s).  Windows cut by an odd H / W keep the elements that exist and get no pooled gradient (floor mode).
constexpr int BWD_WCHUNK = BWD_CHUNK / 4;   // windows per block
__global__ __launch_bounds__(256) void bn_bwd_reduce_pool_kernel(const BnBwdParams P) {
  typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));
  const int chunk = blockIdx.x, c = blockIdx.y, n = blockIdx.z;
  const int HW = P.H * P.W;
  const size_t plane = ((size_t)n * P.C + c) * HW;
  const float sc = P.scale[c], sh = P.shift[c], mu = P.mean[c], is = P.invstd[c];
  const int Hp = P.H >> 1, Wp = P.W >> 1, Hc = (P.H + 1) >> 1, Wc = (P.W + 1) >> 1;
  const float* xr = P.raw + plane;
  const float* ga = P.da.p != nullptr ? P.da.p + (size_t)n * P.da.ns + (size_t)c * P.da.cs : nullptr;
  const float* dp = P.dpool + ((size_t)n * P.C + c) * Hp * Wp;
  float* dzp = P.dz + plane;
  float s1 = 0.f, s2 = 0.f;
  const int q_end = min((chunk + 1) * BWD_WCHUNK, Hc * Wc);
  for (int q = chunk * BWD_WCHUNK + threadIdx.x; q < q_end; q += 256) {
    const int hp = q / Wc, wp = q - hp * Wc;
    const int o0 = 2 * hp * P.W + 2 * wp, o1 = o0 + P.W;
    const bool col1 = 2 * wp + 1 < P.W, row1 = 2 * hp + 1 < P.H;
    float x[4] = {0.f, 0.f, 0.f, 0.f}, g[4] = {0.f, 0.f, 0.f, 0.f};
    if (col1) {
      const f32x2u t = *reinterpret_cast<const f32x2u*>(xr + o0);
      x[0] = t[0], x[1] = t[1];
      if (ga != nullptr) { const f32x2u u = *reinterpret_cast<const f32x2u*>(ga + o0); g[0] = u[0], g[1] = u[1]; }
      if (row1) {
        const f32x2u t1 = *reinterpret_cast<const f32x2u*>(xr + o1);
        x[2] = t1[0], x[3] = t1[1];
        if (ga != nullptr) { const f32x2u u = *reinterpret_cast<const f32x2u*>(ga + o1); g[2] = u[0], g[3] = u[1]; }
      }
    } else {
      x[0] = xr[o0];
      if (ga != nullptr) g[0] = ga[o0];
      if (row1) {
        x[2] = xr[o1];
        if (ga != nullptr) g[2] = ga[o1];
      }
    }
    float y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = fmaf(x[i], sc, sh);
    if (col1 && row1) {   // a whole window: the first maximum of relu(bn(raw)) in (0,0),(0,1),(1,0),(1,1) order takes dpool
      float best = fmaxf(y[0], 0.f);
      int bi = 0;
#pragma unroll
      for (int i = 1; i < 4; ++i) {
        const float v = fmaxf(y[i], 0.f);
        if (v > best) { best = v; bi = i; }
      }
      const float dpv = dp[hp * Wp + wp];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (bi == i) g[i] += dpv;
    }
    float dz[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ex = (i & 1 ? col1 : true) && (i & 2 ? row1 : true);
      dz[i] = (ex && y[i] > 0.f) ? g[i] : 0.f;
      s1 += dz[i];
      s2 = fmaf(dz[i], (x[i] - mu) * is, s2);
    }
    if (col1) {
      *reinterpret_cast<f32x2u*>(dzp + o0) = f32x2u{dz[0], dz[1]};
      if (row1) *reinterpret_cast<f32x2u*>(dzp + o1) = f32x2u{dz[2], dz[3]};
    } else {
      dzp[o0] = dz[0];
      if (row1) dzp[o1] = dz[2];
    }
  }
  // two sums only (no third in this mode, its column is written 0): the epilogue stays this kernel's own, bn_bwd_store_sums
  // with a zero third sum costs it an LDS word per wave and a read in thread 2
  __shared__ float red[2][4];
  s1 = wave_sum_f(s1);
  s2 = wave_sum_f(s2);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = s1;
    red[1][threadIdx.x >> 6] = s2;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int row = n * P.chunks + chunk;
    P.partials[(size_t)row * 3 * P.C + threadIdx.x * P.C + c] =
        threadIdx.x < 2 ? red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3] : 0.f;
  }
}

// partial rows of one launch: per image, the blocks of the window-per-thread form (>= those of the element forms, whose
// surplus blocks write zeros)
static int bwd_chunks(int H, int W) { return ceil_div(((H + 1) / 2) * ((W + 1) / 2), BWD_WCHUNK); }
extern "C" int gsd_bn_bwd_partial_rows(int N, int C, int H, int W) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  return N * bwd_chunks(H, W);
}

extern "C" int gsd_bn_bwd_reduce(int mode, const float* raw, const float* scale, const float* shift, const float* mean,
                                 const float* invstd, const gsd_src* da, const float* dpool, const float* dout,
                                 const float* wout, int K, float* dz, float* partials, int N, int C, int H, int W,
                                 void* stream) {
  GSD_REQUIRE(raw && scale && shift && mean && invstd && dz && partials, GSD_ERR_BAD_ARG, "gsd_bn_bwd_reduce: null argument");
  GSD_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && mode >= 0 && mode <= 2, GSD_ERR_BAD_ARG, "gsd_bn_bwd_reduce: bad sizes");
  GSD_REQUIRE(N <= 65535 && C <= 65535, GSD_ERR_UNSUPPORTED, "gsd_bn_bwd_reduce: N, C must be <= 65535");
  BnBwdParams P;
  P.raw = raw; P.scale = scale; P.shift = shift; P.mean = mean; P.invstd = invstd;
  P.da = null_srcd();
  if (mode != 2 && da != nullptr && da->ptr != nullptr) {
    GSD_REQUIRE(da->scale == nullptr && da->relu == 0 && da->off_h == 0 && da->off_w == 0 && da->H == H && da->W == W &&
                    da->C >= C,
                GSD_ERR_BAD_ARG, "gsd_bn_bwd_reduce: da must be a plain (>=C,H,W) tensor");
    if (int e = gsd_require_rows_contiguous(*da, "gsd_bn_bwd_reduce da")) return e;
    P.da = to_srcd(*da);
  }
  if (mode == 0) GSD_REQUIRE(P.da.p != nullptr, GSD_ERR_BAD_ARG, "gsd_bn_bwd_reduce: mode PLAIN needs da");
  if (mode == 1) GSD_REQUIRE(dpool != nullptr, GSD_ERR_BAD_ARG, "gsd_bn_bwd_reduce: mode POOL needs dpool");
  if (mode == 2) {
    GSD_REQUIRE(dout != nullptr && wout != nullptr, GSD_ERR_BAD_ARG, "gsd_bn_bwd_reduce: mode OUTC needs dout, wout");
    GSD_REQUIRE(K >= 1 && K <= 8, GSD_ERR_UNSUPPORTED, "gsd_bn_bwd_reduce: backward of the output conv supports 1 <= n_classes <= 8 (got %d)", K);
  }
  P.dpool = dpool; P.dout = dout; P.wout = wout; P.K = K;
  P.dz = dz; P.partials = partials;
  P.N = N; P.C = C; P.H = H; P.W = W;
  P.chunks = bwd_chunks(H, W);
  dim3 grid(P.chunks, C, N);
  const float* gsrc = mode == 2 ? dout : P.da.p;
  const bool vec = (H * W) % 4 == 0 && (((uintptr_t)raw | (uintptr_t)dz | (uintptr_t)gsrc) & 15) == 0 &&
                   (mode == 2 || (P.da.ns % 4 == 0 && P.da.cs % 4 == 0));
  if (mode == 1) hipLaunchKernelGGL(bn_bwd_reduce_pool_kernel, grid, dim3(256), 0, (hipStream_t)stream, P);
  else if (mode == 0 && vec) hipLaunchKernelGGL((bn_bwd_reduce_vec_kernel<0>), grid, dim3(256), 0, (hipStream_t)stream, P);
  else if (mode == 2 && vec && K == 1) hipLaunchKernelGGL((bn_bwd_reduce_vec_kernel<2>), grid, dim3(256), 0, (hipStream_t)stream, P);
  else if (mode == 0) hipLaunchKernelGGL((bn_bwd_reduce_kernel<0>), grid, dim3(256), 0, (hipStream_t)stream, P);
  else hipLaunchKernelGGL((bn_bwd_reduce_kernel<2>), grid, dim3(256), 0, (hipStream_t)stream, P);
  GSD_LAUNCH_CHECK("gsd_bn_bwd_reduce");
  return GSD_OK;
}

// sums: 3*C doubles followed by RG*3*C doubles of scratch
extern "C" int gsd_bn_bwd_reduce_partials(const float* partials, int rows, int C, double* sums, void* stream) {
  GSD_REQUIRE(partials && sums && rows > 0 && C > 0, GSD_ERR_BAD_ARG, "gsd_bn_bwd_reduce_partials: bad argument");
  return gsd_colsum_run("gsd_bn_bwd_reduce_partials", partials, rows, 3 * C, 3 * C, 0, 1, sums, sums + 3 * C, nullptr, 0, 0, stream);
}

// Channel c from its sums (sum dz, sum dz*xhat, third: elements first, first + stride, first + 2 * stride): the parameter
// gradients are this rank's LOCAL sums, the coefficients of the apply pass the GLOBAL sums over the count (one rank: the same
// sums).  The sums come as pointer, first index and stride, not as values, because the third one is READ only for a layer
// that has dwout: the three-launch form (sl, sg, c, C) must not touch sl[2C + c] otherwise; the one-launch form passes its
// registers (v, v, 0, 1).
__device__ __forceinline__ void bn_bwd_finalize_channel(int c, const double* local, const double* global, int first, int stride,
                                                        double count, float* dgamma, float* dbeta, float* dwout, float* c1,
                                                        float* c2) {
  dbeta[c] = (float)local[first];
  dgamma[c] = (float)local[stride + first];
  if (dwout != nullptr) dwout[c] = (float)local[2 * stride + first];
  c1[c] = (float)(global[first] / count);
  c2[c] = (float)(global[stride + first] / count);
}
__global__ void bn_bwd_finalize_kernel(const double* sl, const double* sg, int C, double count, float* dgamma,
                                       float* dbeta, float* dwout, float* c1, float* c2) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  bn_bwd_finalize_channel(c, sl, sg, c, C, count, dgamma, dbeta, dwout, c1, c2);
}
extern "C" int gsd_bn_bwd_finalize(const double* sums_local, const double* sums_global, int C, double count,
                                   float* dgamma, float* dbeta, float* dwout, float* c1, float* c2, void* stream) {
  GSD_REQUIRE(sums_local && dgamma && dbeta && c1 && c2 && C > 0 && count > 0, GSD_ERR_BAD_ARG,
              "gsd_bn_bwd_finalize: bad argument");
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, (hipStream_t)stream, sums_local,
                     sums_global != nullptr ? sums_global : sums_local, C, count, dgamma, dbeta, dwout, c1, c2);
  GSD_LAUNCH_CHECK("gsd_bn_bwd_finalize");
  return GSD_OK;
}

__global__ __launch_bounds__(1024) void bn_bwd_reduce_finalize_kernel(const float* __restrict__ part, int rows, int ld, int off2,
                                                                     int off3, int C, double* __restrict__ sums, double count,
                                                                     float* dgamma, float* dbeta, float* dwout, float* c1,
                                                                     float* c2) {
  const int off[3] = {0, off2, off3};
  double v[3];
  if (!rf_block_sums<3>(part, rows, ld, off, C, v)) return;
  const int c = blockIdx.x * RF_CH + threadIdx.x;
  sums[c] = v[0];
  sums[C + c] = v[1];
  sums[2 * C + c] = v[2];
  bn_bwd_finalize_channel(c, v, v, 0, 1, count, dgamma, dbeta, dwout, c1, c2);
}

extern "C" int gsd_bn_bwd_reduce_finalize(const float* partials, int rows, int layout_mpad, int C, double* sums, double count,
                                          float* dgamma, float* dbeta, float* dwout, float* c1, float* c2, void* stream) {
  GSD_REQUIRE(partials && sums && dgamma && dbeta && c1 && c2 && rows > 0 && C > 0 && count > 0, GSD_ERR_BAD_ARG,
              "gsd_bn_bwd_reduce_finalize: bad argument");
  GSD_REQUIRE(layout_mpad == 0 || (layout_mpad >= C && dwout == nullptr), GSD_ERR_BAD_ARG,
              "gsd_bn_bwd_reduce_finalize: the conv-epilogue layout has no third column block");
  // layout_mpad == 0: rows of [sum dz | sum dz*xhat | third] (3*C) from the stand-alone reduce kernels;
  // layout_mpad  > 0: rows of 2*mpad from a dX epilogue (gsd_conv3x3_dgrad_bnrelu / gsd_bf16_bnbwd)
  const int ld = layout_mpad > 0 ? 2 * layout_mpad : 3 * C, off2 = layout_mpad > 0 ? layout_mpad : C;
  hipLaunchKernelGGL(bn_bwd_reduce_finalize_kernel, dim3(ceil_div(C, RF_CH)), dim3(RF_CH * RF_LANES), 0, (hipStream_t)stream, partials, rows, ld,
                     off2, layout_mpad > 0 ? -1 : 2 * C, C, sums, count, dgamma, dbeta, dwout, c1, c2);
  GSD_LAUNCH_CHECK("gsd_bn_bwd_reduce_finalize");
  return GSD_OK;
}

template <bool VEC4>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(float* __restrict__ dz, const float* __restrict__ raw,
                                                           const float* scale, const float* mean, const float* invstd,
                                                           const float* c1, const float* c2, int C, int HW, int chunks) {
  const int chunk = blockIdx.x, c = blockIdx.y, n = blockIdx.z;
  const size_t plane = ((size_t)n * C + c) * HW;
  const float sc = scale[c], mu = mean[c], is = invstd[c], k1 = c1[c], k2 = c2[c];
  const int e_end = min((chunk + 1) * BWD_CHUNK, HW);
  if (VEC4) {   // HW % 4 == 0 and 16-byte aligned tensors: one 16-byte load / store per lane
    for (int e = chunk * BWD_CHUNK + threadIdx.x * 4; e < e_end; e += 1024) {
      const f32x4 r = *reinterpret_cast<const f32x4*>(raw + plane + e);
      f32x4 d = *reinterpret_cast<const f32x4*>(dz + plane + e);
#pragma unroll
      for (int i = 0; i < 4; ++i) d[i] = sc * (d[i] - k1 - (r[i] - mu) * is * k2);
      *reinterpret_cast<f32x4*>(dz + plane + e) = d;
    }
  } else {
    for (int e = chunk * BWD_CHUNK + threadIdx.x; e < e_end; e += 256) {
      const float xh = (raw[plane + e] - mu) * is;
      dz[plane + e] = sc * (dz[plane + e] - k1 - xh * k2);
    }
  }
}
// Out-of-place form into a PITCHED buffer (rows of `pitch` floats, pitch % 4 == 0, 16-byte aligned): the result is what the
// dW and dX kernels read next, and rows that start 16-byte aligned let them move it as aligned 16-byte LDS-DMA pieces (a
// quarter of the gather instructions).  Same traffic as the in-place pass.  A thread owns 4 consecutive columns of one row:
// four coalesced dword loads per input (the contiguous W = 427 rows are not 16-byte aligned), one 16-byte store; columns
// W .. pitch-1 are written 0 -- the padding value of a plain gradient operand.
__global__ __launch_bounds__(256) void bn_bwd_apply_pitched_kernel(const float* __restrict__ dz, const float* __restrict__ raw,
                                                                   const float* scale, const float* mean, const float* invstd,
                                                                   const float* c1, const float* c2, float* __restrict__ out,
                                                                   int C, int H, int W, int pitch) {
  const int c = blockIdx.y, n = blockIdx.z;
  const int q4 = pitch >> 2;                       // 16-byte pieces per output row
  const int total = H * q4;
  const size_t plane = ((size_t)n * C + c) * (size_t)H * W;
  float* const o = out + ((size_t)n * C + c) * (size_t)H * pitch;
  const float sc = scale[c], mu = mean[c], is = invstd[c], k1 = c1[c], k2 = c2[c];
  typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
  for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
    const int h = e / q4, w = (e - h * q4) * 4;
    const size_t src = plane + (size_t)h * W + w;
    f32x4 d;
    if (w + 4 <= W) {   // one (unaligned) 16-byte load per input: the contiguous rows of W = 427 floats are not 16-byte aligned
      const f32x4 g = *reinterpret_cast<const f32x4u*>(dz + src), r = *reinterpret_cast<const f32x4u*>(raw + src);
#pragma unroll
      for (int i = 0; i < 4; ++i) d[i] = sc * (g[i] - k1 - (r[i] - mu) * is * k2);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool ok = w + i < W;
        const float g = ok ? dz[src + i] : 0.f, r = ok ? raw[src + i] : mu;
        d[i] = ok ? sc * (g - k1 - (r - mu) * is * k2) : 0.f;
      }
    }
    *reinterpret_cast<f32x4*>(o + (size_t)h * pitch + w) = d;
  }
}
extern "C" int gsd_bn_bwd_apply(float* dz, const float* raw, const float* scale, const float* mean, const float* invstd,
                                const float* c1, const float* c2, int N, int C, int H, int W, float* out, int out_w_stride,
                                void* stream) {
  GSD_REQUIRE(dz && raw && scale && mean && invstd && c1 && c2 && N > 0 && C > 0 && H > 0 && W > 0, GSD_ERR_BAD_ARG,
              "gsd_bn_bwd_apply: bad argument");
  GSD_REQUIRE(N <= 65535 && C <= 65535, GSD_ERR_UNSUPPORTED, "gsd_bn_bwd_apply: N, C must be <= 65535");
  if (out != nullptr) {
    GSD_REQUIRE(out_w_stride >= W && out_w_stride % 4 == 0 && ((uintptr_t)out & 15) == 0, GSD_ERR_BAD_ARG,
                "gsd_bn_bwd_apply: the pitched destination needs a 16-byte aligned base and a row pitch %% 4 == 0 (got %d for W %d)",
                out_w_stride, W);
    const int total = H * (out_w_stride / 4);
    const int bx = ceil_div(total, 256) < 64 ? ceil_div(total, 256) : 64;
    hipLaunchKernelGGL(bn_bwd_apply_pitched_kernel, dim3(bx, C, N), dim3(256), 0, (hipStream_t)stream, dz, raw, scale, mean,
                       invstd, c1, c2, out, C, H, W, out_w_stride);
    GSD_LAUNCH_CHECK("gsd_bn_bwd_apply (pitched)");
    return GSD_OK;
  }
  const int chunks = ceil_div(H * W, BWD_CHUNK);
  const bool vec4 = (H * W) % 4 == 0 && (((uintptr_t)dz | (uintptr_t)raw) & 15) == 0;
  if (vec4)
    hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, dim3(chunks, C, N), dim3(256), 0, (hipStream_t)stream, dz, raw, scale, mean,
                       invstd, c1, c2, C, H * W, chunks);
  else
    hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, dim3(chunks, C, N), dim3(256), 0, (hipStream_t)stream, dz, raw, scale, mean,
                       invstd, c1, c2, C, H * W, chunks);
  GSD_LAUNCH_CHECK("gsd_bn_bwd_apply");
  return GSD_OK;
}

// relu(bn(raw)) written ONCE into a PITCHED buffer (gsd_bnrelu_pitched): what every m-block of a conv3x3 consumer would otherwise
// recompute on its halo window.  Rows of `pitch` floats start 16-byte aligned, so the consumer moves them as aligned 16-byte
// LDS-DMA pieces -- the launch class of the dX convs.  As bn_bwd_apply_pitched_kernel: a thread owns 4 consecutive columns of one
// row, one unaligned 16-byte load, one aligned 16-byte store; columns W .. pitch-1 are written 0 on every call.  The value is
// apply_affine's (one fmaf, one fmaxf): the bits the deferred consumers compute.
__global__ __launch_bounds__(256) void bnrelu_pitched_kernel(const SrcD S, const DstD D) {
  const int c = blockIdx.y, n = blockIdx.z;
  const int q4 = D.ws >> 2;
  const int total = S.H * q4;
  const float* const in = S.p + (size_t)n * S.ns + (size_t)c * S.cs;
  float* const o = D.p + (size_t)n * D.ns + (size_t)c * D.cs;
  const float sc = S.scale[c], sh = S.shift[c];
  typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
  for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
    const int h = e / q4, w = (e - h * q4) * 4;
    const float* const r = in + (size_t)h * S.W + w;
    f32x4 d;
    if (w + 4 <= S.W) {
      const f32x4 v = *reinterpret_cast<const f32x4u*>(r);
#pragma unroll
      for (int i = 0; i < 4; ++i) d[i] = apply_affine(v[i], sc, sh, 1);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) d[i] = w + i < S.W ? apply_affine(r[i], sc, sh, 1) : 0.f;
    }
    *reinterpret_cast<f32x4*>(o + (size_t)h * D.ws + w) = d;
  }
}
extern "C" int gsd_bnrelu_pitched(const gsd_src* src, const gsd_dst* dst, int N, void* stream) {
  GSD_REQUIRE(src && dst && src->ptr && dst->ptr && N > 0, GSD_ERR_BAD_ARG, "gsd_bnrelu_pitched: bad argument");
  GSD_REQUIRE(src->scale && src->shift && src->relu != 0 && src->off_h == 0 && src->off_w == 0, GSD_ERR_BAD_ARG,
              "gsd_bnrelu_pitched: the source must carry a deferred BatchNorm + ReLU");
  if (int e = gsd_check_src(*src, "gsd_bnrelu_pitched src")) return e;
  if (int e = gsd_check_dst(*dst, "gsd_bnrelu_pitched dst", true)) return e;
  GSD_REQUIRE(dst->C == src->C && dst->H == src->H && dst->W == src->W && dst->off_h == 0 && dst->off_w == 0, GSD_ERR_BAD_ARG,
              "gsd_bnrelu_pitched: dst must be the source's (C,H,W)");
  GSD_REQUIRE(dst->w_stride % 4 == 0 && ((uintptr_t)dst->ptr & 15) == 0 && dst->c_stride % 4 == 0 && dst->n_stride % 4 == 0,
              GSD_ERR_BAD_ARG, "gsd_bnrelu_pitched: the destination needs a 16-byte aligned base and pitch, plane and image strides "
              "%% 4 == 0 (pitch %d for W %d)", dst->w_stride, dst->W);
  GSD_REQUIRE(N <= 65535 && src->C <= 65535, GSD_ERR_UNSUPPORTED, "gsd_bnrelu_pitched: N, C must be <= 65535");
  const int total = src->H * (dst->w_stride / 4);
  const int bx = ceil_div(total, 256) < 64 ? ceil_div(total, 256) : 64;
  hipLaunchKernelGGL(bnrelu_pitched_kernel, dim3(bx, src->C, N), dim3(256), 0, (hipStream_t)stream, to_srcd(*src), to_dstd(*dst));
  GSD_LAUNCH_CHECK("gsd_bnrelu_pitched");
  return GSD_OK;
}
