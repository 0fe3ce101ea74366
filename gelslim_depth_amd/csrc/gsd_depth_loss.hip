// gsd_depth_loss.hip -- the depth-aware training loss and its gradient (gfx950), include/gsd.h: gsd_depth_loss.
//
//   e      = o - t                                    (fp32, as everything that decides a branch)
//   L_data = (1/M) sum w * rho(e),  w = 1 + contact_weight * [|t - background| > contact_eps],  rho = e^2 | |e| | huber(delta)
//   L_grad = sum_k (1/M_k) sum over the grid h mod s = 0, w mod s = 0 (s = 2^k) of phi(e[h,w+s] - e[h,w]) + phi(e[h+s,w] - e[h,w])
//   L      = L_data + grad_weight * L_grad
//
// One fused pass: a block owns a run of consecutive elements, a thread element i of it (64-bit index); it reads o and t there
// and at up to four neighbours per scale, adds its five summands in fp64 and -- when a gradient is asked for -- writes
// d L / d o[i] in GATHER form: the pixel collects the derivative of every pair it is an end of (left, right, upper, lower), so
// nothing is scattered and no atomics are needed.  The second stage, one wave, adds the per-block partial sums in a fixed
// order.  The block count is a function of the shape alone, so the results are bitwise reproducible and do not depend on
// whether a gradient is written.
//
// Neighbour reads are branch-free (the lesson of gsd_dgrad_first.hip): the address of a pair that does not exist is clamped
// to the pixel's own, the value is selected afterwards, and the up to eight loads of a scale fly together.  They hit the
// cache (the tensors are read from HBM once); there is no LDS tile.  The only branch is wave-uniform: a wave none of whose
// elements lies on the grid of a scale -- every other row at s = 2, three rows in four at s = 4, seven in eight at s = 8 --
// skips that scale.
//
// Precision: the data term's summands are formed in fp64 (the square of an fp32 value is exact there); a scale's two slope
// summands are added in fp32 (|g| + |g|: one rounding; g^2 + g^2: two) and join an fp64 accumulator per scale; every sum is
// fp64.  The gradient is fp32 throughout: at most 17 summands, each with at most four roundings (its fp32 coefficient, the
// product, the addition), well inside 2^-19 of the sum of their magnitudes.  Contraction is off inside the kernels: the two
// instantiations of a shape (with and without a gradient) must add the same bits.
#include "gsd_common.h"

#include <math.h>

namespace {

constexpr int DL_BLOCKS = 1024;   // block cap, as gsd_loss_fwd_bwd's: four blocks of four waves for each of the MI355X's 256 CUs
constexpr int DL_SUMS = 5;        // per-block partial sums: w*rho, slope term (normalised per scale), e^2, |e|, contact count

struct DlParams {
  long long numel;
  long long chunk;   // ceil(numel / blocks): consecutive elements per block
  int dr;            // 256 % W: columns a thread advances per iteration
  int dqh;           // (256 / W) % H: rows, modulo the image height
  int H, W;
  int data_kind, grad_kind;
  float delta, contact_eps, background, grad_scale;
  float w_contact_f, inv_M_f;   // the gradient's fp32 copies of the two below
  float g_Mk[4];                // grad_weight / M_k
  double w_contact;             // 1 + contact_weight
  double inv_M;                 // 1 / M
  double inv_Mk[4];             // 1 / M_k
};

__device__ __forceinline__ float dl_signf(float g) { return g > 0.f ? 1.f : (g < 0.f ? -1.f : 0.f); }
// e at byte offset `off` from the element's own address (0: the element itself, when the pair does not exist)
__device__ __forceinline__ float dl_e_at(const char* po, const char* pt, long long off) {
  return *reinterpret_cast<const float*>(po + off) - *reinterpret_cast<const float*>(pt + off);
}

template <int S, bool GRAD>
__global__ __launch_bounds__(256) void depth_loss_stage1(const DlParams P, const float* __restrict__ o,
                                                         const float* __restrict__ t, float* __restrict__ grad,
                                                         double* __restrict__ ws) {
#pragma clang fp contract(off)
  double a_data = 0.0, a_sq = 0.0, a_abs = 0.0, a_contact = 0.0;
  double a_scale[S > 0 ? S : 1] = {};   // sum of phi per scale, divided by M_k behind the loop
  const int H = P.H, W = P.W;
  // A block owns `chunk` consecutive elements (ten rows at batch 32) and walks them 256 at a time: the neighbours of its
  // elements are mostly its own, so their loads hit the CU's cache.  (h, w) of element i are carried along instead of divided
  // out again: i advances by 256, that is dr columns and dqh rows.
  long long i = (long long)blockIdx.x * P.chunk + threadIdx.x;
  const long long end = min((long long)(blockIdx.x + 1) * P.chunk, P.numel);
  const long long row0 = i / W;
  int w = (int)(i - row0 * W);
  int h = (int)(row0 % H);
  const double delta = (double)P.delta;
  for (; i < end; i += 256) {
    const float ti = t[i];
    const float e = o[i] - ti;
    const float ae = fabsf(e);
    const double ed = (double)e, sq = ed * ed;
    const bool contact = fabsf(ti - P.background) > P.contact_eps;
    const double wgt = contact ? P.w_contact : 1.0;
    const bool small = ae <= P.delta;
    double rho;
    float drho;
    if (P.data_kind == 0) {
      rho = sq, drho = 2.f * e;
    } else if (P.data_kind == 1) {
      rho = (double)ae, drho = dl_signf(e);
    } else {
      rho = small ? 0.5 * sq : delta * ((double)ae - 0.5 * delta);
      drho = small ? e : (e > 0.f ? P.delta : -P.delta);   // clamp(e, -delta, delta); a NaN e has made rho NaN already
    }
    a_data += wgt * rho;
    a_sq += sq;
    a_abs += (double)ae;
    a_contact += contact ? 1.0 : 0.0;
    float d = (contact ? P.w_contact_f : 1.f) * drho * P.inv_M_f;
    const char* po = reinterpret_cast<const char*>(o + i);
    const char* pt = reinterpret_cast<const char*>(t + i);
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const int s = 1 << k;
      const bool on = ((h | w) & (s - 1)) == 0;   // on the grid of this scale
      // Scale k concerns one pixel in 4^k.  A wave's 64 elements lie in one row or two, so for k >= 1 most waves hold no grid
      // point at all and skip the scale as a whole -- a wave-uniform branch; inside it nothing is guarded.
      if (k > 0 && !__any(on)) continue;
      const long long sw = 4ll * s * W;
      const bool vr = on && w + s < W, vd = on && h + s < H;
      const float er = dl_e_at(po, pt, vr ? 4 * s : 0), edn = dl_e_at(po, pt, vd ? sw : 0);
      const float gr = vr ? er - e : 0.f, gd = vd ? edn - e : 0.f;
      float gl = 0.f, gu = 0.f;
      if (GRAD) {
        const bool vl = on && w - s >= 0, vu = on && h - s >= 0;
        const float el = dl_e_at(po, pt, vl ? -4 * s : 0), eu = dl_e_at(po, pt, vu ? -sw : 0);
        gl = vl ? e - el : 0.f, gu = vu ? e - eu : 0.f;
      }
      if (P.grad_kind == 0) {   // phi = |g|, phi' = sign(g): the four signs add exactly
        a_scale[k] += (double)(fabsf(gr) + fabsf(gd));
        if (GRAD) d = fmaf(P.g_Mk[k], dl_signf(gl) - dl_signf(gr) + dl_signf(gu) - dl_signf(gd), d);
      } else {                  // phi = g^2, phi' = 2 g
        a_scale[k] += (double)fmaf(gr, gr, gd * gd);
        if (GRAD) d = fmaf(P.g_Mk[k], 2.f * (gl - gr + gu - gd), d);
      }
    }
    if (GRAD) grad[i] = d * P.grad_scale;
    w += P.dr;
    int dh = P.dqh;
    if (w >= W) w -= W, ++dh;
    h += dh;
    if (h >= H) h -= H;
  }
  double a_slope = 0.0;
#pragma unroll
  for (int k = 0; k < S; ++k) a_slope += a_scale[k] * P.inv_Mk[k];
  __shared__ double red[DL_SUMS][4];
  const double sums[DL_SUMS] = {a_data, a_slope, a_sq, a_abs, a_contact};
#pragma unroll
  for (int q = 0; q < DL_SUMS; ++q) {
    const double v = wave_sum_d(sums[q]);
    if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < DL_SUMS) {
    const int q = threadIdx.x;
    ws[(size_t)q * gridDim.x + blockIdx.x] = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
  }
}

// single wave: ws holds DL_SUMS runs of nblocks partial sums
__global__ __launch_bounds__(64) void depth_loss_stage2(const double* __restrict__ ws, int nblocks, double inv_M, double grad_weight,
                                                        float* __restrict__ terms, int* guard_words, int tick) {
#pragma clang fp contract(off)
  // the five runs side by side, four blocks ahead: 20 loads in flight instead of one (each lane still adds its blocks in rising order)
  double tot[DL_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int b = threadIdx.x; b < nblocks; b += 64) {
#pragma unroll
    for (int q = 0; q < DL_SUMS; ++q) tot[q] += ws[(size_t)q * nblocks + b];
  }
#pragma unroll
  for (int q = 0; q < DL_SUMS; ++q) tot[q] = wave_sum_d(tot[q]);
  if (threadIdx.x == 0) {
    const double l_data = tot[0] * inv_M, l_grad = tot[1];
    const float loss = (float)(l_data + grad_weight * l_grad);
    terms[0] = loss;
    terms[1] = (float)l_data;
    terms[2] = (float)l_grad;
    terms[3] = (float)(tot[2] * inv_M);
    terms[4] = (float)(tot[3] * inv_M);
    terms[5] = (float)(tot[4] * inv_M);
    if (guard_words != nullptr && !isfinite(loss)) guard_words[0] = tick;   // as gsd_loss_fwd_bwd
  }
}

// elements of the (N, K, H, W) tensor, or 0 when a dimension is not positive or the product leaves int64
int64_t dl_numel(int N, int K, int H, int W) {
  if (N <= 0 || K <= 0 || H <= 0 || W <= 0) return 0;
  const int64_t nk = (int64_t)N * K, hw = (int64_t)H * W;
  return nk > INT64_MAX / hw ? 0 : nk * hw;
}

bool dl_weight_ok(float v) { return isfinite(v) && v >= 0.f; }

template <int S>
void dl_launch(bool with_grad, int blocks, hipStream_t st, const DlParams& P, const float* o, const float* t, float* grad,
               double* ws) {
  if (with_grad)
    hipLaunchKernelGGL((depth_loss_stage1<S, true>), dim3(blocks), dim3(256), 0, st, P, o, t, grad, ws);
  else
    hipLaunchKernelGGL((depth_loss_stage1<S, false>), dim3(blocks), dim3(256), 0, st, P, o, t, grad, ws);
}

}   // namespace

extern "C" int64_t gsd_depth_loss_workspace(int N, int K, int H, int W) {
  const int64_t numel = dl_numel(N, K, H, W);
  return numel > 0 ? (int64_t)DL_SUMS * gsd_grid_256(numel, DL_BLOCKS) : 0;
}

extern "C" int gsd_depth_loss_fwd_bwd(const gsd_depth_loss* spec, const float* o, const float* t, int N, int K, int H, int W,
                                      float grad_scale, float* terms, float* grad, double* workspace, int64_t workspace_elems,
                                      const gsd_guard* guard, void* stream) {
  GSD_REQUIRE(spec && o && t && terms && workspace, GSD_ERR_BAD_ARG, "gsd_depth_loss_fwd_bwd: null pointer");
  const int64_t numel = dl_numel(N, K, H, W);
  GSD_REQUIRE(numel > 0, GSD_ERR_BAD_ARG, "gsd_depth_loss_fwd_bwd: bad dims N=%d K=%d H=%d W=%d", N, K, H, W);
  GSD_REQUIRE(spec->data_kind >= 0 && spec->data_kind <= 2, GSD_ERR_BAD_ARG,
              "gsd_depth_loss_fwd_bwd: data_kind %d (0 mse, 1 l1, 2 huber)", spec->data_kind);
  GSD_REQUIRE(spec->grad_kind == 0 || spec->grad_kind == 1, GSD_ERR_BAD_ARG, "gsd_depth_loss_fwd_bwd: grad_kind %d (0 l1, 1 l2)",
              spec->grad_kind);
  GSD_REQUIRE(spec->grad_scales >= 0 && spec->grad_scales <= 4, GSD_ERR_BAD_ARG, "gsd_depth_loss_fwd_bwd: grad_scales %d not in 0..4",
              spec->grad_scales);
  GSD_REQUIRE(spec->reserved == 0, GSD_ERR_BAD_ARG, "gsd_depth_loss_fwd_bwd: the reserved word must be 0");
  GSD_REQUIRE(dl_weight_ok(spec->huber_delta) && (spec->data_kind != 2 || spec->huber_delta > 0.f), GSD_ERR_BAD_ARG,
              "gsd_depth_loss_fwd_bwd: huber_delta %g (finite, not negative; positive for huber)", (double)spec->huber_delta);
  GSD_REQUIRE(dl_weight_ok(spec->contact_weight), GSD_ERR_BAD_ARG, "gsd_depth_loss_fwd_bwd: contact_weight %g must be finite and >= 0",
              (double)spec->contact_weight);
  GSD_REQUIRE(dl_weight_ok(spec->contact_eps), GSD_ERR_BAD_ARG, "gsd_depth_loss_fwd_bwd: contact_eps %g must be finite and >= 0",
              (double)spec->contact_eps);
  GSD_REQUIRE(isfinite(spec->background), GSD_ERR_BAD_ARG, "gsd_depth_loss_fwd_bwd: background must be finite");
  GSD_REQUIRE(dl_weight_ok(spec->grad_weight), GSD_ERR_BAD_ARG, "gsd_depth_loss_fwd_bwd: grad_weight %g must be finite and >= 0",
              (double)spec->grad_weight);
  GSD_REQUIRE(((uintptr_t)workspace & 7) == 0, GSD_ERR_BAD_ARG, "gsd_depth_loss_fwd_bwd: workspace must be 8-byte aligned");
  if (int e = gsd_check_guard(guard, "gsd_depth_loss_fwd_bwd")) return e;
  const int blocks = gsd_grid_256(numel, DL_BLOCKS);
  GSD_REQUIRE(workspace_elems >= (int64_t)DL_SUMS * blocks, GSD_ERR_WORKSPACE, "gsd_depth_loss_fwd_bwd: workspace of %lld doubles, need %d",
              (long long)workspace_elems, DL_SUMS * blocks);

  DlParams P;
  P.numel = numel;
  P.chunk = ceil_div64(numel, blocks);
  P.dr = 256 % W;
  P.dqh = (256 / W) % H;
  P.H = H, P.W = W;
  P.data_kind = spec->data_kind, P.grad_kind = spec->grad_kind;
  P.delta = spec->huber_delta, P.contact_eps = spec->contact_eps, P.background = spec->background, P.grad_scale = grad_scale;
  P.w_contact = 1.0 + (double)spec->contact_weight;
  P.inv_M = 1.0 / (double)numel;
  P.w_contact_f = (float)P.w_contact, P.inv_M_f = (float)P.inv_M;
  for (int k = 0; k < 4; ++k) {
    const int64_t s = (int64_t)1 << k;
    const double Mk = (double)N * (double)K * (double)ceil_div64(H, s) * (double)ceil_div64(W, s);
    P.inv_Mk[k] = 1.0 / Mk;
    P.g_Mk[k] = (float)((double)spec->grad_weight / Mk);
  }
  const hipStream_t st = (hipStream_t)stream;
  const bool g = grad != nullptr;
  switch (spec->grad_scales) {
    case 0: dl_launch<0>(g, blocks, st, P, o, t, grad, workspace); break;
    case 1: dl_launch<1>(g, blocks, st, P, o, t, grad, workspace); break;
    case 2: dl_launch<2>(g, blocks, st, P, o, t, grad, workspace); break;
    case 3: dl_launch<3>(g, blocks, st, P, o, t, grad, workspace); break;
    default: dl_launch<4>(g, blocks, st, P, o, t, grad, workspace); break;
  }
  GSD_LAUNCH_CHECK("gsd_depth_loss_fwd_bwd stage1");
  hipLaunchKernelGGL(depth_loss_stage2, dim3(1), dim3(64), 0, st, (const double*)workspace, blocks, P.inv_M,
                     (double)spec->grad_weight, terms, gsd_guard_words(guard), gsd_guard_tick(guard));
  GSD_LAUNCH_CHECK("gsd_depth_loss_fwd_bwd stage2");
  return GSD_OK;
}
