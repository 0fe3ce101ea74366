// gsd_lm_step.h -- one Levenberg-Marquardt step's bookkeeping and solve, shared by mesh_pose_lm_update (N = 4, a mask of free
// parameters) and mesh_icp_lm_update (N = 6, all free); DESIGN.md section 25.  One thread per problem, fp64, contraction off, the
// operations in the order that tests/mesh_pose_refine_ref.py::lm_update_ref and tests/mesh_closest_ref.py::lm_update repeat.
// Every loop unrolls and every index is a constant: the matrices live in registers.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// Whether the trial is taken (the first call takes it; afterwards a strictly smaller cost, so a NaN never wins), the damping's
// move (down on success, up otherwise, within its bounds) and the count of accepted trials.  Lm: down, up, lambda_min, lambda_max,
// first.
template <typename Lm>
__device__ __forceinline__ bool gsd_lm_accept(const Lm& lm, double trial_cost, double cost, double& lam, int& accepted) {
#pragma clang fp contract(off)
  const bool take = lm.first || trial_cost < cost;
  if (!lm.first) {
    lam = take ? fmax(lam * lm.down, lm.lambda_min) : fmin(lam * lm.up, lm.lambda_max);
    accepted += take ? 1 : 0;
  }
  return take;
}

// (A + lam diag A) d = -b by Cholesky in the parameters' order, A_upper the upper triangle of A row by row.  A parameter whose bit
// of free_mask is clear has the identity's row and column and a zero right-hand side: its step is exactly 0 and the others'
// factorisation meets only exact zeros from it.  d = 0 unless every pivot is positive and finite and every component finite;
// component k is clipped to +- max_step[k].
template <int N>
__device__ __forceinline__ void gsd_lm_solve(const double* A_upper, const double* b, double lam, unsigned free_mask,
                                             const double* max_step, double (&d)[N]) {
#pragma clang fp contract(off)
  double M[N][N], rhs[N], Lc[N][N], z[N];
  {
    int s = 0;
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
      for (int k = j; k < N; ++k, ++s) {
        const bool both = ((free_mask >> j) & 1) && ((free_mask >> k) & 1);
        const double a = j == k ? A_upper[s] + lam * A_upper[s] : A_upper[s];
        M[j][k] = M[k][j] = both ? a : (j == k ? 1.0 : 0.0);
      }
  }
#pragma unroll
  for (int j = 0; j < N; ++j) rhs[j] = ((free_mask >> j) & 1) ? -b[j] : 0.0;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double piv = M[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) piv = piv - Lc[j][k] * Lc[j][k];
    ok = ok && piv > 0.0 && isfinite(piv);
    Lc[j][j] = sqrt(piv);
#pragma unroll
    for (int r = j + 1; r < N; ++r) {
      double s = M[r][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s = s - Lc[r][k] * Lc[j][k];
      Lc[r][j] = s / Lc[j][j];
    }
  }
#pragma unroll
  for (int r = 0; r < N; ++r) {
    double s = rhs[r];
#pragma unroll
    for (int k = 0; k < r; ++k) s = s - Lc[r][k] * z[k];
    z[r] = s / Lc[r][r];
  }
#pragma unroll
  for (int r = N - 1; r >= 0; --r) {
    double s = z[r];
#pragma unroll
    for (int k = r + 1; k < N; ++k) s = s - Lc[k][r] * d[k];
    d[r] = s / Lc[r][r];
  }
#pragma unroll
  for (int k = 0; k < N; ++k) ok = ok && isfinite(d[k]);
#pragma unroll
  for (int k = 0; k < N; ++k) d[k] = ok ? fmin(fmax(d[k], -max_step[k]), max_step[k]) : 0.0;
}
