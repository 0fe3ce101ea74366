// gsd_optim.hip -- what follows the backward pass of an fp32 train step (gfx950): the loss and its gradient, gradient clipping
// by global norm, fused Adam + EMA over the flat parameter arena, and the snapshot / restore that lets a step skipped by the
// non-finite guard leave no trace.  Reductions are two-stage and ordered (bitwise reproducible), never float atomics.
#include "gsd_common.h"

// ---------------------------------------------------------------------------------------------
// loss (MSE / L1) forward + gradient
// ---------------------------------------------------------------------------------------------
constexpr int LOSS_BLOCKS = 1024;
template <int KIND>
__global__ __launch_bounds__(256) void loss_stage1(const float* __restrict__ o, const float* __restrict__ t,
                                                   long long numel, float gscale, float* __restrict__ grad,
                                                   float* __restrict__ ws) {
  double s = 0.0;
  const float inv = 1.0f / (float)numel;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < numel; i += (long long)gridDim.x * 256) {
    const float d = o[i] - t[i];
    if (KIND == 0) {
      s += (double)d * (double)d;
      if (grad != nullptr) grad[i] = 2.f * d * inv * gscale;
    } else {
      s += (double)fabsf(d);
      if (grad != nullptr) grad[i] = (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) * inv * gscale;
    }
  }
  __shared__ double red[4];
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) reinterpret_cast<double*>(ws)[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ void loss_stage2(const float* ws, int nblocks, long long numel, float* loss_out, int* guard_words, int tick) {
  // single wave
  double s = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 64) s += reinterpret_cast<const double*>(ws)[i];
  s = wave_sum_d(s);
  if (threadIdx.x == 0) {
    const float loss = (float)(s / (double)numel);
    loss_out[0] = loss;
    if (guard_words != nullptr && !isfinite(loss)) guard_words[0] = tick;   // the reference's `pred_loss.isnan()` test, on the device
  }
}
extern "C" int gsd_loss_fwd_bwd(int kind, const float* o, const float* t, int64_t numel, float grad_scale, float* loss_out,
                                float* grad, float* workspace, const gsd_guard* guard, void* stream) {
  GSD_REQUIRE(o && t && loss_out && workspace && numel > 0 && (kind == 0 || kind == 1), GSD_ERR_BAD_ARG,
              "gsd_loss_fwd_bwd: bad argument");
  GSD_REQUIRE(((uintptr_t)workspace & 7) == 0, GSD_ERR_BAD_ARG, "gsd_loss_fwd_bwd: workspace must be 8-byte aligned");
  const int blocks = gsd_grid_256(numel, LOSS_BLOCKS);
  if (kind == 0)
    hipLaunchKernelGGL((loss_stage1<0>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, o, t, (long long)numel,
                       grad_scale, grad, workspace);
  else
    hipLaunchKernelGGL((loss_stage1<1>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, o, t, (long long)numel,
                       grad_scale, grad, workspace);
  GSD_LAUNCH_CHECK("gsd_loss_fwd_bwd stage1");
  hipLaunchKernelGGL(loss_stage2, dim3(1), dim3(64), 0, (hipStream_t)stream, workspace, blocks, (long long)numel, loss_out,
                     gsd_guard_words(guard), gsd_guard_tick(guard));
  GSD_LAUNCH_CHECK("gsd_loss_fwd_bwd stage2");
  return GSD_OK;
}

// ---------------------------------------------------------------------------------------------
// fused Adam (coupled L2) + EMA over a flat arena
// ---------------------------------------------------------------------------------------------
// CLIP: the gradient scale is grad_scale * clip[1], the product formed on the device from gsd_grad_norm's coefficient; the update
// is the same statements either way, so clip[1] == 1 gives the bits of the form without it.
template <bool CLIP>
__global__ __launch_bounds__(256) void adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v,
                                                       float* __restrict__ ema, long long numel, float lr_over_bc1,
                                                       float sqrt_bc2, float b1, float b2, float eps, float wd,
                                                       float one_minus_d, float grad_scale, const float* __restrict__ clip,
                                                       int* guard_words, int tick) {
  if (guard_words != nullptr && guard_words[0] == tick) {   // a non-finite statistic, loss or gradient norm: skip the step, count it
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&guard_words[1], 1);
    return;
  }
  const float gscale = CLIP ? grad_scale * clip[1] : grad_scale;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < numel; i += (long long)gridDim.x * 256) {
    float pv = p[i];
    const float gv = fmaf(wd, pv, g[i] * gscale);   // g += wd*p            (torch _single_tensor_adam)
    float mv = m[i];
    mv = mv + (gv - mv) * (1.f - b1);               // exp_avg.lerp_(g, 1-b1)
    const float vv = fmaf(1.f - b2, gv * gv, v[i] * b2);   // exp_avg_sq.mul_(b2).addcmul_(g,g,1-b2)
    const float denom = sqrtf(vv) / sqrt_bc2 + eps;    // sqrt(v)/sqrt(bc2) + eps
    pv = pv - lr_over_bc1 * (mv / denom);                  // p.addcdiv_(m, denom, -lr/bc1)
    p[i] = pv;
    m[i] = mv;
    v[i] = vv;
    if (ema != nullptr) {
      const float s = ema[i];
      ema[i] = s - one_minus_d * (s - pv);          // torch_ema: shadow.sub_((1-d)*(shadow-param))
    }
  }
}
// bias corrections of step `step`, grid, launch.  clip == nullptr: the form without the device-side coefficient.
static int adam_ema_run(const char* what, float* p, const float* g, float* m, float* v, float* ema, int64_t numel, int step, float lr,
                        float beta1, float beta2, float eps, float weight_decay, float ema_decay, float grad_scale,
                        const float* clip, const gsd_guard* guard, void* stream) {
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const float lr_over_bc1 = (float)((double)lr / bc1);
  const float sqrt_bc2 = (float)sqrt(bc2);
  hipLaunchKernelGGL(clip != nullptr ? adam_ema_kernel<true> : adam_ema_kernel<false>, dim3(gsd_grid_256(numel, 4096)), dim3(256), 0,
                     (hipStream_t)stream, p, g, m, v, ema, (long long)numel, lr_over_bc1, sqrt_bc2, beta1, beta2, eps, weight_decay,
                     1.0f - ema_decay, grad_scale, clip, gsd_guard_words(guard), gsd_guard_tick(guard));
  GSD_LAUNCH_CHECK(what);
  return GSD_OK;
}
extern "C" int gsd_adam_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t numel, int step, float lr,
                            float beta1, float beta2, float eps, float weight_decay, float ema_decay, float grad_scale,
                            const gsd_guard* guard, void* stream) {
  GSD_REQUIRE(p && g && m && v && numel > 0 && step >= 1, GSD_ERR_BAD_ARG, "gsd_adam_ema: bad argument");
  if (int e = gsd_check_guard(guard, "gsd_adam_ema")) return e;
  return adam_ema_run("gsd_adam_ema", p, g, m, v, ema, numel, step, lr, beta1, beta2, eps, weight_decay, ema_decay, grad_scale,
                      nullptr, guard, stream);
}
// gsd_adam_ema behind gsd_grad_norm: `clip` is its two floats
extern "C" int gsd_adam_ema_clip(float* p, const float* g, float* m, float* v, float* ema, int64_t numel, int step, float lr,
                                 float beta1, float beta2, float eps, float weight_decay, float ema_decay, float grad_scale,
                                 const float* clip, const gsd_guard* guard, void* stream) {
  GSD_REQUIRE(p && g && m && v && clip && numel > 0 && step >= 1, GSD_ERR_BAD_ARG, "gsd_adam_ema_clip: bad argument");
  if (int e = gsd_check_guard(guard, "gsd_adam_ema_clip")) return e;
  return adam_ema_run("gsd_adam_ema_clip", p, g, m, v, ema, numel, step, lr, beta1, beta2, eps, weight_decay, ema_decay, grad_scale,
                      clip, guard, stream);
}

// A skipped step leaves no trace in the BatchNorm running statistics: snapshot before the step, conditional restore behind it
__global__ void guard_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, long long n, const int* guard_words,
                                  int tick) {
  if (guard_words != nullptr && guard_words[0] != tick) return;   // restore form: only when this step was marked bad
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) dst[i] = src[i];
}
extern "C" int gsd_guard_snapshot(const float* live, float* snapshot, int64_t n, void* stream) {
  GSD_REQUIRE(live && snapshot && n > 0, GSD_ERR_BAD_ARG, "gsd_guard_snapshot: bad argument");
  const int blocks = gsd_grid_256(n, 1024);
  hipLaunchKernelGGL(guard_copy_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, live, snapshot, (long long)n,
                     (const int*)nullptr, 0);
  GSD_LAUNCH_CHECK("gsd_guard_snapshot");
  return GSD_OK;
}
extern "C" int gsd_guard_restore(const gsd_guard* guard, float* live, const float* snapshot, int64_t n, void* stream) {
  GSD_REQUIRE(guard && guard->words && guard->tick != 0 && live && snapshot && n > 0, GSD_ERR_BAD_ARG,
              "gsd_guard_restore: bad argument");
  const int blocks = gsd_grid_256(n, 1024);
  hipLaunchKernelGGL(guard_copy_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, snapshot, live, (long long)n,
                     (const int*)guard->words, guard->tick);
  GSD_LAUNCH_CHECK("gsd_guard_restore");
  return GSD_OK;
}

// ---------------------------------------------------------------------------------------------
// gradient clipping by global norm (torch.nn.utils.clip_grad_norm_) over the flat gradient arena
// ---------------------------------------------------------------------------------------------
// The arena is cut into groups of four consecutive floats; group k belongs to thread k mod (blocks * 256), which adds its
// groups in rising order, element by element.  The number of blocks is a function of numel alone, so which thread adds
// what, and in which order, does not depend on where g starts: a 16-byte aligned arena is read with one 16-byte load per
// group, any other with four 4-byte loads, and both give the same bits.  The last, short group is read element by element.
constexpr int GNORM_MAX_BLOCKS = 2048;
static inline int grad_norm_blocks(int64_t numel) {
  return gsd_grid_256(ceil_div64(numel, 4), GNORM_MAX_BLOCKS);   // a thread per group of four
}
template <bool ALIGNED>
__global__ __launch_bounds__(256) void grad_norm_stage1(const float* __restrict__ g, long long numel, double* __restrict__ ws) {
  const long long groups = numel >> 2;   // full groups
  const long long stride = (long long)gridDim.x * 256;
  double s = 0.0;
  long long k = (long long)blockIdx.x * 256 + threadIdx.x;
#pragma unroll 4
  for (; k < groups; k += stride) {
    float x0, x1, x2, x3;
    if (ALIGNED) {
      const float4 q = reinterpret_cast<const float4*>(g)[k];
      x0 = q.x, x1 = q.y, x2 = q.z, x3 = q.w;
    } else {
      x0 = g[4 * k], x1 = g[4 * k + 1], x2 = g[4 * k + 2], x3 = g[4 * k + 3];
    }
    s = fma((double)x0, (double)x0, s);   // the square of an fp32 value is exact in fp64: one rounding per addition
    s = fma((double)x1, (double)x1, s);
    s = fma((double)x2, (double)x2, s);
    s = fma((double)x3, (double)x3, s);
  }
  if (k == groups)   // the owner of the short group, if there is one
    for (long long i = 4 * groups; i < numel; ++i) s = fma((double)g[i], (double)g[i], s);
  __shared__ double red[4];
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) ws[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void grad_norm_stage2(const double* __restrict__ ws, int nblocks, float grad_scale, float max_norm,
                                                        float* __restrict__ clip, int* guard_words, int tick) {
  double s = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 256) s += ws[i];
  __shared__ double red[4];
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double S = (red[0] + red[1]) + (red[2] + red[3]);
    const float total = (float)(sqrt(S) * (double)grad_scale);   // L2 norm of the averaged gradient, rounded once
    float coef = fminf(1.f, max_norm / (total + 1e-6f));         // clip_grad_norm_: clamp(max_norm / (total + 1e-6), max=1)
    if (!isfinite(total)) {                                      // fminf(1, NaN) is 1: a non-finite norm must not pass as "no clip"
      coef = __builtin_nanf("");
      if (guard_words != nullptr) guard_words[0] = tick;
    }
    clip[0] = total;
    clip[1] = coef;
  }
}
extern "C" int64_t gsd_grad_norm_workspace(int64_t numel) { return numel > 0 ? grad_norm_blocks(numel) : 0; }
extern "C" int gsd_grad_norm(const float* g, int64_t numel, float grad_scale, float max_norm, float* clip, double* workspace,
                             int64_t workspace_elems, const gsd_guard* guard, void* stream) {
  GSD_REQUIRE(g && clip && workspace && numel > 0, GSD_ERR_BAD_ARG, "gsd_grad_norm: null pointer or numel <= 0");
  GSD_REQUIRE(max_norm > 0.f, GSD_ERR_BAD_ARG, "gsd_grad_norm: max_norm must be > 0 (+inf: measure only), got %g", (double)max_norm);
  GSD_REQUIRE(((uintptr_t)g & 3) == 0 && ((uintptr_t)clip & 3) == 0 && ((uintptr_t)workspace & 7) == 0, GSD_ERR_BAD_ARG,
              "gsd_grad_norm: g and clip must be 4-byte aligned, workspace 8-byte aligned");
  if (int e = gsd_check_guard(guard, "gsd_grad_norm")) return e;
  const int blocks = grad_norm_blocks(numel);
  GSD_REQUIRE(workspace_elems >= blocks, GSD_ERR_WORKSPACE, "gsd_grad_norm: workspace of %lld doubles, need %d",
              (long long)workspace_elems, blocks);
  if (((uintptr_t)g & 15) == 0)
    hipLaunchKernelGGL((grad_norm_stage1<true>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, g, (long long)numel, workspace);
  else
    hipLaunchKernelGGL((grad_norm_stage1<false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, g, (long long)numel, workspace);
  GSD_LAUNCH_CHECK("gsd_grad_norm stage1");
  hipLaunchKernelGGL(grad_norm_stage2, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, blocks, grad_scale,
                     max_norm, clip, gsd_guard_words(guard), gsd_guard_tick(guard));
  GSD_LAUNCH_CHECK("gsd_grad_norm stage2");
  return GSD_OK;
}
