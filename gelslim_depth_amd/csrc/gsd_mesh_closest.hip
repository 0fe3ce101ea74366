// Closest points on a triangle mesh and the normal-equation rows of a rigid registration (include/gsd.h).
//
//   mesh_volume_count / mesh_volume_fill   a 3-D grid of cubic cells over the mesh: count, scan, fill (gsd_cell_lists.h).
//     A triangle is listed in every cell its axis-aligned box touches, widened by MC_CELL_EPS of a cell on either side so that
//     rounding in the index can only add a cell.  A triangle whose fp64 cross product is exactly (0, 0, 0) is listed nowhere.
//   mesh_closest          one lane per point: the lane walks shells of cells of growing Chebyshev radius around the cell of q, the
//     point clamped into the grid's box, and stops once its best d^2 is strictly below a lower bound of every unseen triangle's.
//   mesh_icp_rows         the same walk on p' = R p + t (kept in fp64) and the 30 sums of one start over one block of 256 points:
//     a butterfly per wave, (w0 + w1) + (w2 + w3) through LDS; mesh_icp_rows_sum adds a start's blocks in ascending order.
//   mesh_icp_lm_update    one thread per start: the shared LM step (gsd_lm_step.h) on six parameters, then exp(xi) T.
//
// The distance arithmetic (mc_triangle) is the definition: fp64 from the fp32 loads on, contraction off, + - * / and comparisons
// only, so that a numpy twin repeats it bit for bit.  No per-lane array is indexed with a run-time value.
#include "gsd_common.h"
#include "gsd_cell_lists.h"
#include "gsd_lm_step.h"

#include <math.h>

namespace {

constexpr int MC_MAX_T = 1 << 24;        // triangles per mesh
constexpr int MC_MAX_AXIS = 1024;        // cells per grid axis
constexpr int64_t MC_MAX_CELLS = 1 << 24;
constexpr int MC_ROW = GSD_ICP_ROW;
constexpr int MC_BLOCK = 256;            // points per block of the query and of the row sums
constexpr double MC_CELL_EPS = 1e-6;     // of a cell: how far a triangle's index range is widened
constexpr double MC_SHRINK = 1.0 - 1.0 / 1073741824.0;   // 1 - 2^-30: the stop bound is rounded down by far more than any rounding error

struct McVol {          // gsd_mesh_volume by value
  double x0, y0, z0, x1, y1, z1, cell, inv_cell;
  int nx, ny, nz;
};

__device__ __forceinline__ int mc_cell(double v, double g0, double inv_cell, double eps, int n) {
#pragma clang fp contract(off)
  const double f = floor((v - g0) * inv_cell + eps);
  int i = f < 0.0 ? 0 : (f > (double)(n - 1) ? n - 1 : (int)f);
  return i;
}

struct McTri {
  double ax, ay, az, bx, by, bz, cx, cy, cz;
};
__device__ __forceinline__ McTri mc_load(const float* __restrict__ tri, int id) {
  const float* v = tri + (size_t)id * 9;
  McTri t;
  t.ax = v[0], t.ay = v[1], t.az = v[2], t.bx = v[3], t.by = v[4], t.bz = v[5], t.cx = v[6], t.cy = v[7], t.cz = v[8];
  return t;
}
__device__ __forceinline__ double mc_dot(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
  return (ax * bx + ay * by) + az * bz;
}
// (b - a) x (c - a), each component two rounded products and one subtraction
__device__ __forceinline__ void mc_cross(const McTri& t, double& nx, double& ny, double& nz) {
#pragma clang fp contract(off)
  const double ux = t.bx - t.ax, uy = t.by - t.ay, uz = t.bz - t.az;
  const double vx = t.cx - t.ax, vy = t.cy - t.ay, vz = t.cz - t.az;
  nx = uy * vz - uz * vy;
  ny = uz * vx - ux * vz;
  nz = ux * vy - uy * vx;
}
__device__ __forceinline__ bool mc_degenerate(const McTri& t) {
  double nx, ny, nz;
  mc_cross(t, nx, ny, nz);
  return nx == 0.0 && ny == 0.0 && nz == 0.0;
}

// cells [i0, i1] per axis that the triangle's box touches, widened
__device__ __forceinline__ void mc_cell_range(const McTri& t, const McVol& G, int (&lo)[3], int (&hi)[3]) {
  lo[0] = mc_cell(fmin(t.ax, fmin(t.bx, t.cx)), G.x0, G.inv_cell, -MC_CELL_EPS, G.nx);
  hi[0] = mc_cell(fmax(t.ax, fmax(t.bx, t.cx)), G.x0, G.inv_cell, MC_CELL_EPS, G.nx);
  lo[1] = mc_cell(fmin(t.ay, fmin(t.by, t.cy)), G.y0, G.inv_cell, -MC_CELL_EPS, G.ny);
  hi[1] = mc_cell(fmax(t.ay, fmax(t.by, t.cy)), G.y0, G.inv_cell, MC_CELL_EPS, G.ny);
  lo[2] = mc_cell(fmin(t.az, fmin(t.bz, t.cz)), G.z0, G.inv_cell, -MC_CELL_EPS, G.nz);
  hi[2] = mc_cell(fmax(t.az, fmax(t.bz, t.cz)), G.z0, G.inv_cell, MC_CELL_EPS, G.nz);
}

// one thread per triangle: +1 on every cell of its range
__global__ __launch_bounds__(256) void mesh_volume_count(const McVol G, const float* __restrict__ tri, int T, int* __restrict__ count) {
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= T) return;
  const McTri t = mc_load(tri, id);
  if (mc_degenerate(t)) return;
  int lo[3], hi[3];
  mc_cell_range(t, G, lo, hi);
  for (int iz = lo[2]; iz <= hi[2]; ++iz)
    for (int iy = lo[1]; iy <= hi[1]; ++iy)
      for (int ix = lo[0]; ix <= hi[0]; ++ix) atomicAdd(count + ((size_t)iz * G.ny + iy) * G.nx + ix, 1);
}

// one block: start becomes the exclusive sums of the cell counts, cursor a copy, *total the int64 total (gsd_cell_lists.h)
__global__ __launch_bounds__(GSD_CELL_SCAN_THREADS) void mesh_volume_scan(int ncells, int* __restrict__ start, int* __restrict__ cursor,
                                                                          long long* __restrict__ total) {
  gsd_cell_scan(ncells, start, cursor, total);
}

// one thread per triangle: its id into every cell of the range the count pass walked
__global__ __launch_bounds__(256) void mesh_volume_fill(const McVol G, const float* __restrict__ tri, int T, int* __restrict__ cursor,
                                                        int* __restrict__ list, long long list_elems) {
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= T) return;
  const McTri t = mc_load(tri, id);
  if (mc_degenerate(t)) return;
  int lo[3], hi[3];
  mc_cell_range(t, G, lo, hi);
  for (int iz = lo[2]; iz <= hi[2]; ++iz)
    for (int iy = lo[1]; iy <= hi[1]; ++iy)
      for (int ix = lo[0]; ix <= hi[0]; ++ix) {
        const int pos = atomicAdd(cursor + ((size_t)iz * G.ny + iy) * G.nx + ix, 1);
        if (pos >= 0 && pos < list_elems) list[pos] = id;   // a list shorter than the counted total is never overrun
      }
}

// The closest point x of triangle t to p and d^2 = |p - x|^2: the region method on d1..d6, va, vb, vc (DESIGN.md section 23 has
// the order of operations; tests/mesh_closest_ref.py repeats it).
__device__ __forceinline__ double mc_triangle(const McTri& t, double px, double py, double pz, double& x, double& y, double& z) {
#pragma clang fp contract(off)
  const double abx = t.bx - t.ax, aby = t.by - t.ay, abz = t.bz - t.az;
  const double acx = t.cx - t.ax, acy = t.cy - t.ay, acz = t.cz - t.az;
  const double d1 = mc_dot(abx, aby, abz, px - t.ax, py - t.ay, pz - t.az);
  const double d2 = mc_dot(acx, acy, acz, px - t.ax, py - t.ay, pz - t.az);
  const double d3 = mc_dot(abx, aby, abz, px - t.bx, py - t.by, pz - t.bz);
  const double d4 = mc_dot(acx, acy, acz, px - t.bx, py - t.by, pz - t.bz);
  const double d5 = mc_dot(abx, aby, abz, px - t.cx, py - t.cy, pz - t.cz);
  const double d6 = mc_dot(acx, acy, acz, px - t.cx, py - t.cy, pz - t.cz);
  const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const double e1 = d4 - d3, e2 = d5 - d6;
  if (d1 <= 0.0 && d2 <= 0.0) {                            // vertex a
    x = t.ax, y = t.ay, z = t.az;
  } else if (d3 >= 0.0 && d4 <= d3) {                      // vertex b
    x = t.bx, y = t.by, z = t.bz;
  } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {        // edge ab
    const double v = d1 / (d1 - d3);
    x = t.ax + v * abx, y = t.ay + v * aby, z = t.az + v * abz;
  } else if (d6 >= 0.0 && d5 <= d6) {                      // vertex c
    x = t.cx, y = t.cy, z = t.cz;
  } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {        // edge ac
    const double w = d2 / (d2 - d6);
    x = t.ax + w * acx, y = t.ay + w * acy, z = t.az + w * acz;
  } else if (va <= 0.0 && e1 >= 0.0 && e2 >= 0.0) {        // edge bc
    const double w = e1 / (e1 + e2);
    x = t.bx + w * (t.cx - t.bx), y = t.by + w * (t.cy - t.by), z = t.bz + w * (t.cz - t.bz);
  } else {                                                 // face
    const double s = (va + vb) + vc;
    const double v = vb / s, w = vc / s;
    x = (t.ax + v * abx) + w * acx, y = (t.ay + v * aby) + w * acy, z = (t.az + v * abz) + w * acz;
  }
  const double rx = px - x, ry = py - y, rz = pz - z;
  return (rx * rx + ry * ry) + rz * rz;
}

struct McBest {
  double d2, x, y, z;
  int id;
};

// every triangle of cell (ix, iy, iz) against the lane's best: a smaller d^2 wins, among bit-equal ones the lower id
__device__ __forceinline__ void mc_visit(const McVol& G, const float* __restrict__ tri, const int* __restrict__ start,
                                         const int* __restrict__ list, int ix, int iy, int iz, double px, double py, double pz,
                                         McBest& b) {
  const size_t c = ((size_t)iz * G.ny + iy) * G.nx + ix;
  const int lo = start[c], hi = start[c + 1];
  for (int k = lo; k < hi; ++k) {
    const int id = list[k];
    double x, y, z;
    const double d2 = mc_triangle(mc_load(tri, id), px, py, pz, x, y, z);
    if (d2 < b.d2 || (d2 == b.d2 && id < b.id)) b.d2 = d2, b.x = x, b.y = y, b.z = z, b.id = id;
  }
}

// gap from q to the faces of the walked block [c - r, c + r] along one axis that lie inside the grid (+inf where neither does).
// Formed from q - g0, as mc_cell forms its index: the rounding error is relative to the grid's extent, not to the coordinates
// (q - g0 itself is exact or nearly so, q lies within the grid), so the margins in units of a cell cover it wherever the mesh lies.
__device__ __forceinline__ double mc_gap(double q, double g0, double cell, int c, int r, int n) {
#pragma clang fp contract(off)
  const double u = q - g0;
  double m = INFINITY;
  if (c - r > 0) m = fmin(m, u - (double)(c - r) * cell);
  if (c + r + 1 < n) m = fmin(m, (double)(c + r + 1) * cell - u);
  return m;
}

// The winner of the finite point p within sqrt(D2): b.id = -1 when there is none.
// A triangle that no walked cell lists lies wholly beyond an interior face of the walked block (its index range misses the block's
// on some axis), so for each of its points x: |p - x|^2 >= |p - q|^2 + |q - x|^2 >= |p - q|^2 + m^2, m the smallest gap.  The walk
// stops when the best d^2 is STRICTLY below that bound (an unseen tie could have the lower id), or the bound is above D2.  The
// bound is rounded down (MC_SHRINK on both terms and 2^-30 of a cell off m), so that rounding can only delay the stop.
__device__ __forceinline__ McBest mc_query(const McVol& G, const float* __restrict__ tri, const int* __restrict__ start,
                                           const int* __restrict__ list, double px, double py, double pz, double D2) {
#pragma clang fp contract(off)
  const double qx = fmin(fmax(px, G.x0), G.x1), qy = fmin(fmax(py, G.y0), G.y1), qz = fmin(fmax(pz, G.z0), G.z1);
  const double ex = px - qx, ey = py - qy, ez = pz - qz;
  const double pq2 = ((ex * ex + ey * ey) + ez * ez) * MC_SHRINK;
  const int cx = mc_cell(qx, G.x0, G.inv_cell, 0.0, G.nx), cy = mc_cell(qy, G.y0, G.inv_cell, 0.0, G.ny),
            cz = mc_cell(qz, G.z0, G.inv_cell, 0.0, G.nz);
  const int rmax = max(max(max(cx, G.nx - 1 - cx), max(cy, G.ny - 1 - cy)), max(cz, G.nz - 1 - cz));
  McBest b;
  b.d2 = INFINITY, b.x = b.y = b.z = 0.0, b.id = -1;
  for (int r = 0;; ++r) {
    const int x0 = max(cx - r, 0), x1 = min(cx + r, G.nx - 1);
    const int y0 = max(cy - r, 0), y1 = min(cy + r, G.ny - 1);
    const int z0 = max(cz - r, 0), z1 = min(cz + r, G.nz - 1);
    for (int iz = z0; iz <= z1; ++iz)
      for (int iy = y0; iy <= y1; ++iy) {
        if (abs(iz - cz) == r || abs(iy - cy) == r) {
          for (int ix = x0; ix <= x1; ++ix) mc_visit(G, tri, start, list, ix, iy, iz, px, py, pz, b);
        } else {      // r > 0 here: only the two cells of the shell on this line
          if (cx - r >= 0) mc_visit(G, tri, start, list, cx - r, iy, iz, px, py, pz, b);
          if (cx + r <= G.nx - 1) mc_visit(G, tri, start, list, cx + r, iy, iz, px, py, pz, b);
        }
      }
    if (r >= rmax) break;      // the whole grid is walked
    double m = fmin(fmin(mc_gap(qx, G.x0, G.cell, cx, r, G.nx), mc_gap(qy, G.y0, G.cell, cy, r, G.ny)),
                    mc_gap(qz, G.z0, G.cell, cz, r, G.nz));
    m = fmax(m * MC_SHRINK - G.cell * (1.0 - MC_SHRINK), 0.0);
    const double bound = pq2 + m * m;
    if (b.d2 < bound || bound > D2) break;
  }
  if (!(b.d2 <= D2)) b.id = -1;
  return b;
}

__global__ __launch_bounds__(MC_BLOCK) void mesh_closest(const McVol G, const float* __restrict__ tri, const int* __restrict__ start,
                                                         const int* __restrict__ list, const float* __restrict__ points, long long N,
                                                         double D2, int* __restrict__ triangle, float* __restrict__ closest,
                                                         float* __restrict__ distance, double* __restrict__ sq_distance) {
  const long long i = (long long)blockIdx.x * MC_BLOCK + threadIdx.x;
  if (i >= N) return;
  const float fx = points[3 * i], fy = points[3 * i + 1], fz = points[3 * i + 2];
  McBest b;
  b.d2 = INFINITY, b.x = b.y = b.z = 0.0, b.id = -1;
  if (isfinite(fx) && isfinite(fy) && isfinite(fz)) b = mc_query(G, tri, start, list, (double)fx, (double)fy, (double)fz, D2);
  const bool hit = b.id >= 0;
  triangle[i] = b.id;
  closest[3 * i] = hit ? (float)b.x : NAN, closest[3 * i + 1] = hit ? (float)b.y : NAN, closest[3 * i + 2] = hit ? (float)b.z : NAN;
  distance[i] = hit ? (float)sqrt(b.d2) : INFINITY;
  sq_distance[i] = hit ? b.d2 : (double)INFINITY;
}

// One block: 256 points of one start.  v[0..29] of a lane are its terms of the row; a point off the end, a non-finite one and
// (but for the cost) an inactive one add zeros.  KIND 0: point to plane, 1: point to point.
template <int KIND>
__global__ __launch_bounds__(MC_BLOCK) void mesh_icp_rows(const McVol G, const float* __restrict__ tri, const int* __restrict__ start,
                                                          const int* __restrict__ list, const float* __restrict__ points,
                                                          const float* __restrict__ weights, int N, int nblk,
                                                          const double* __restrict__ transforms, double D2,
                                                          double* __restrict__ partial) {
#pragma clang fp contract(off)
  const int s = blockIdx.x / nblk, blk = blockIdx.x - s * nblk;
  const int i = blk * MC_BLOCK + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double v[MC_ROW];
#pragma unroll
  for (int q = 0; q < MC_ROW; ++q) v[q] = 0.0;
  if (i < N) {
    const double* M = transforms + (size_t)s * 12;
    const double fx = points[3 * (size_t)i], fy = points[3 * (size_t)i + 1], fz = points[3 * (size_t)i + 2];
    const double w = weights ? (double)weights[i] : 1.0;
    const double px = ((M[0] * fx + M[1] * fy) + M[2] * fz) + M[3];
    const double py = ((M[4] * fx + M[5] * fy) + M[6] * fz) + M[7];
    const double pz = ((M[8] * fx + M[9] * fy) + M[10] * fz) + M[11];
    if (isfinite(px) && isfinite(py) && isfinite(pz)) {
      const McBest b = mc_query(G, tri, start, list, px, py, pz, D2);
      if (b.id < 0) {
        v[0] = isfinite(D2) ? w * D2 : 0.0;
      } else {
        const double rx = px - b.x, ry = py - b.y, rz = pz - b.z;
        v[0] = w * b.d2, v[1] = 1.0;
        if (KIND == 0) {
          double nx, ny, nz;
          mc_cross(mc_load(tri, b.id), nx, ny, nz);
          const double len = sqrt((nx * nx + ny * ny) + nz * nz);
          nx = nx / len, ny = ny / len, nz = nz / len;
          const double r = (nx * rx + ny * ry) + nz * rz;
          const double J[6] = {nx, ny, nz, py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx};
          v[2] = w * (r * r);
#pragma unroll
          for (int j = 0; j < 6; ++j) v[3 + j] = w * (J[j] * r);
          int q = 9;
#pragma unroll
          for (int j = 0; j < 6; ++j)
#pragma unroll
            for (int k = j; k < 6; ++k, ++q) v[q] = w * (J[j] * J[k]);
        } else {
          // rows of J = [I, -[p']x]
          const double J[3][6] = {{1.0, 0.0, 0.0, 0.0, pz, -py}, {0.0, 1.0, 0.0, -pz, 0.0, px}, {0.0, 0.0, 1.0, py, -px, 0.0}};
          v[2] = w * b.d2;
#pragma unroll
          for (int j = 0; j < 6; ++j) v[3 + j] = w * ((J[0][j] * rx + J[1][j] * ry) + J[2][j] * rz);
          int q = 9;
#pragma unroll
          for (int j = 0; j < 6; ++j)
#pragma unroll
            for (int k = j; k < 6; ++k, ++q) v[q] = w * ((J[0][j] * J[0][k] + J[1][j] * J[1][k]) + J[2][j] * J[2][k]);
        }
      }
    }
  }
  __shared__ double red[MC_BLOCK / 64][MC_ROW];
#pragma unroll
  for (int q = 0; q < MC_ROW; ++q) {
    const double t = wave_sum_d(v[q]);
    if (lane == 0) red[wave][q] = t;
  }
  __syncthreads();
  if (threadIdx.x < MC_ROW) {
    const int q = threadIdx.x;
    partial[(size_t)blockIdx.x * MC_ROW + q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
  }
}

// one wave per start: lane l adds the partial rows l, l + 64, ... of the start's blocks in ascending order, the lanes meet in the
// xor butterfly (gsd_mesh_pose_normal's second launch).  The order is a function of nblk alone.
__global__ __launch_bounds__(64) void mesh_icp_rows_sum(const double* __restrict__ partial, int nblk, double* __restrict__ rows) {
#pragma clang fp contract(off)
  const int s = blockIdx.x, lane = threadIdx.x;
  double tot[MC_ROW];
#pragma unroll
  for (int q = 0; q < MC_ROW; ++q) tot[q] = 0.0;
  for (int t = lane; t < nblk; t += 64) {
    const double* p = partial + ((size_t)s * nblk + t) * MC_ROW;
#pragma unroll
    for (int q = 0; q < MC_ROW; ++q) tot[q] += p[q];
  }
#pragma unroll
  for (int q = 0; q < MC_ROW; ++q) {
    const double t = wave_sum_d(tot[q]);
    if (lane == 0) rows[(size_t)s * MC_ROW + q] = t;
  }
}

struct McLm {           // gsd_icp_lm by value
  double down, up, lambda_min, lambda_max, max_step[6];
  int first;
};

// One thread per start, fp64 (the definition is include/gsd.h's); every index is a constant, the matrices live in registers.
__global__ __launch_bounds__(64) void mesh_icp_lm_update(const McLm lm, int S, double* __restrict__ transforms, double* __restrict__ lambda,
                                                         double* __restrict__ row, double* __restrict__ trial_transforms,
                                                         const double* __restrict__ trial_row, double* __restrict__ trace,
                                                         int* __restrict__ accepted, double* __restrict__ last_step) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= S) return;
  double cur[MC_ROW], T[12];
#pragma unroll
  for (int q = 0; q < MC_ROW; ++q) cur[q] = row[(size_t)i * MC_ROW + q];
#pragma unroll
  for (int q = 0; q < 12; ++q) T[q] = transforms[(size_t)i * 12 + q];
  double lam = lambda[i];
  int count = lm.first ? 0 : accepted[i];
  const bool take = gsd_lm_accept(lm, trial_row[(size_t)i * MC_ROW], cur[0], lam, count);
  if (take) {
#pragma unroll
    for (int q = 0; q < MC_ROW; ++q) cur[q] = trial_row[(size_t)i * MC_ROW + q];
#pragma unroll
    for (int q = 0; q < 12; ++q) T[q] = trial_transforms[(size_t)i * 12 + q];
  }
  double d[6];      // the step in the order v1, v2, v3, w1, w2, w3
  gsd_lm_solve<6>(cur + 9, cur + 3, lam, 0x3fu, lm.max_step, d);
  // exp(xi): E = I + A K + B K^2, u = (I + B K + C K^2) v, K = [w]x, K^2 = w w^T - th2 I
  const double wx = d[3], wy = d[4], wz = d[5];
  const double th2 = (wx * wx + wy * wy) + wz * wz, th = sqrt(th2);
  double A, Bc, Cc;
  if (th < 1e-8) {
    A = 1.0 - th2 / 6.0, Bc = 0.5 - th2 / 24.0, Cc = 1.0 / 6.0 - th2 / 120.0;
  } else {
    const double sn = sin(th), cs = cos(th);
    A = sn / th, Bc = (1.0 - cs) / th2, Cc = (th - sn) / (th2 * th);
  }
  const double K[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
  const double W[3] = {wx, wy, wz};
  double E[3][3], V[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double k2 = W[r] * W[c] - (r == c ? th2 : 0.0), id = r == c ? 1.0 : 0.0;
      E[r][c] = (id + A * K[r][c]) + Bc * k2;
      V[r][c] = (id + Bc * K[r][c]) + Cc * k2;
    }
  double Tn[12];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) Tn[4 * r + c] = (E[r][0] * T[c] + E[r][1] * T[4 + c]) + E[r][2] * T[8 + c];
    Tn[4 * r + 3] = Tn[4 * r + 3] + ((V[r][0] * d[0] + V[r][1] * d[1]) + V[r][2] * d[2]);
  }
  if (take) {
#pragma unroll
    for (int q = 0; q < MC_ROW; ++q) row[(size_t)i * MC_ROW + q] = cur[q];
#pragma unroll
    for (int q = 0; q < 12; ++q) transforms[(size_t)i * 12 + q] = T[q];
  }
  lambda[i] = lam, accepted[i] = count, trace[i] = cur[0];
#pragma unroll
  for (int q = 0; q < 12; ++q) trial_transforms[(size_t)i * 12 + q] = Tn[q];
#pragma unroll
  for (int k = 0; k < 6; ++k) last_step[6 * (size_t)i + k] = fabs(d[k]);
}

McVol mc_vol(const gsd_mesh_volume* g) {
  McVol G;
  G.x0 = g->x0, G.y0 = g->y0, G.z0 = g->z0, G.x1 = g->x1, G.y1 = g->y1, G.z1 = g->z1, G.cell = g->cell, G.inv_cell = g->inv_cell;
  G.nx = g->nx, G.ny = g->ny, G.nz = g->nz;
  return G;
}
int64_t mc_cells(const gsd_mesh_volume* g) { return (int64_t)g->nx * g->ny * g->nz; }

// non-zero (and the message set) for a volume that no call accepts
int mc_check_volume(const gsd_mesh_volume* g, const char* what) {
  GSD_REQUIRE(g != nullptr, 1, "%s: null volume", what);
  GSD_REQUIRE(g->nx >= 1 && g->ny >= 1 && g->nz >= 1 && g->nx <= MC_MAX_AXIS && g->ny <= MC_MAX_AXIS && g->nz <= MC_MAX_AXIS &&
                  mc_cells(g) <= MC_MAX_CELLS,
              1, "%s: %d x %d x %d cells, 1..%d per axis and at most 2^24 in all", what, g->nx, g->ny, g->nz, MC_MAX_AXIS);
  GSD_REQUIRE(isfinite(g->x0) && isfinite(g->y0) && isfinite(g->z0) && isfinite(g->x1) && isfinite(g->y1) && isfinite(g->z1) &&
                  isfinite(g->cell) && isfinite(g->inv_cell) && g->cell > 0.0 && g->inv_cell > 0.0 && g->x1 >= g->x0 && g->y1 >= g->y0 &&
                  g->z1 >= g->z0,
              1, "%s: the volume's box and cell must be finite, ordered and positive", what);
  GSD_REQUIRE(g->reserved == 0, 1, "%s: the reserved word must be 0", what);
  return 0;
}

struct McMesh {
  const gsd_mesh_volume* vol;
  const float* tri;
  int T;
  const int32_t* cells;
  const int32_t* list;
  int64_t list_elems;
};
int mc_check_mesh(const McMesh& M, const char* what) {
  if (mc_check_volume(M.vol, what)) return 1;
  GSD_REQUIRE(M.tri && M.cells && M.list, 1, "%s: null pointer", what);
  GSD_REQUIRE(M.T >= 1 && M.T <= MC_MAX_T, 1, "%s: %d triangles, 1..%d", what, M.T, MC_MAX_T);
  GSD_REQUIRE(M.list_elems >= 1 && M.list_elems <= INT32_MAX, 1, "%s: list of %lld entries, 1..2^31-1", what, (long long)M.list_elems);
  GSD_REQUIRE(((uintptr_t)M.cells & 7) == 0, 1, "%s: cells must be 8-byte aligned", what);
  return 0;
}

}   // namespace

extern "C" int gsd_mesh_volume_plan(const double* bbox, double cell_mm, gsd_mesh_volume* volume) {
  const char* what = "gsd_mesh_volume_plan";
  GSD_REQUIRE(bbox && volume, GSD_ERR_BAD_ARG, "%s: null pointer", what);
  bool ok = true;
  for (int k = 0; k < 3; ++k) ok = ok && isfinite(bbox[k]) && isfinite(bbox[3 + k]) && bbox[3 + k] >= bbox[k];
  GSD_REQUIRE(ok, GSD_ERR_BAD_ARG, "%s: the bounding box must be finite and ordered", what);
  GSD_REQUIRE(isfinite(cell_mm) && cell_mm > 0.0, GSD_ERR_BAD_ARG, "%s: cell size %g must be finite and positive", what, cell_mm);
  const double ex = bbox[3] - bbox[0], ey = bbox[4] - bbox[1], ez = bbox[5] - bbox[2];
  const double ext = fmax(fmax(fmax(ex, ey), ez), 1e-30);
  double cell = fmax(cell_mm, ext / (MC_MAX_AXIS - 2));
  int n[3];
  for (;;) {      // enlarge the side until the grid has at most 2^24 cells
    const double pad = 1e-3 * cell;
    n[0] = (int)fmax(1.0, ceil((ex + 2 * pad) / cell)), n[1] = (int)fmax(1.0, ceil((ey + 2 * pad) / cell));
    n[2] = (int)fmax(1.0, ceil((ez + 2 * pad) / cell));
    if (n[0] <= MC_MAX_AXIS && n[1] <= MC_MAX_AXIS && n[2] <= MC_MAX_AXIS && (int64_t)n[0] * n[1] * n[2] <= MC_MAX_CELLS) break;
    cell *= 1.0625;
  }
  const double pad = 1e-3 * cell;
  volume->x0 = bbox[0] - pad, volume->y0 = bbox[1] - pad, volume->z0 = bbox[2] - pad;
  volume->cell = cell, volume->inv_cell = 1.0 / cell;
  volume->nx = n[0], volume->ny = n[1], volume->nz = n[2];
  // the box that query points are clamped into: it holds every vertex (n * cell covers the extent and both pads)
  volume->x1 = volume->x0 + n[0] * cell, volume->y1 = volume->y0 + n[1] * cell, volume->z1 = volume->z0 + n[2] * cell;
  volume->reserved = 0;
  return mc_check_volume(volume, what) ? GSD_ERR_BAD_ARG : GSD_OK;
}

extern "C" int64_t gsd_mesh_volume_workspace(const gsd_mesh_volume* volume) {
  if (volume == nullptr || volume->nx < 1 || volume->ny < 1 || volume->nz < 1 || volume->nx > MC_MAX_AXIS || volume->ny > MC_MAX_AXIS ||
      volume->nz > MC_MAX_AXIS || mc_cells(volume) > MC_MAX_CELLS)
    return 0;
  return gsd_cell_words(mc_cells(volume));
}

extern "C" int gsd_mesh_volume_count(const gsd_mesh_volume* volume, const float* tri, int T, int32_t* cells, int64_t cells_elems,
                                     void* stream) {
  const char* what = "gsd_mesh_volume_count";
  if (mc_check_volume(volume, what)) return GSD_ERR_BAD_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const auto count = [&](int* start) {
    hipLaunchKernelGGL(mesh_volume_count, dim3((unsigned)ceil_div(T, 256)), dim3(256), 0, st, mc_vol(volume), tri, T, start);
  };
  return gsd_cell_count(GsdCellCall{what, tri, T, MC_MAX_T, mc_cells(volume), cells, cells_elems, nullptr, 0}, count, mesh_volume_scan, st);
}

extern "C" int gsd_mesh_volume_fill(const gsd_mesh_volume* volume, const float* tri, int T, int32_t* cells, int64_t cells_elems,
                                    int32_t* list, int64_t list_elems, void* stream) {
  const char* what = "gsd_mesh_volume_fill";
  if (mc_check_volume(volume, what)) return GSD_ERR_BAD_ARG;
  return gsd_cell_fill(GsdCellCall{what, tri, T, MC_MAX_T, mc_cells(volume), cells, cells_elems, list, list_elems}, mesh_volume_fill,
                       mc_vol(volume), (hipStream_t)stream);
}

extern "C" int gsd_mesh_closest_points(const gsd_mesh_volume* volume, const float* tri, int T, const int32_t* cells, const int32_t* list,
                                       int64_t list_elems, const float* points, int64_t N, double max_distance, int32_t* triangle,
                                       float* closest, float* distance, double* sq_distance, void* stream) {
  const char* what = "gsd_mesh_closest_points";
  if (mc_check_mesh(McMesh{volume, tri, T, cells, list, list_elems}, what)) return GSD_ERR_BAD_ARG;
  GSD_REQUIRE(points && triangle && closest && distance && sq_distance, GSD_ERR_BAD_ARG, "%s: null pointer", what);
  GSD_REQUIRE(N >= 1 && ceil_div64(N, MC_BLOCK) <= INT32_MAX, GSD_ERR_BAD_ARG, "%s: %lld points, at least 1 and at most 2^31-1 blocks", what,
              (long long)N);
  GSD_REQUIRE(max_distance >= 0.0, GSD_ERR_BAD_ARG, "%s: max_distance %g must be >= 0 (+inf: unlimited)", what, max_distance);
  GSD_REQUIRE(((uintptr_t)sq_distance & 7) == 0, GSD_ERR_BAD_ARG, "%s: sq_distance must be 8-byte aligned", what);
  hipLaunchKernelGGL(mesh_closest, dim3((unsigned)ceil_div64(N, MC_BLOCK)), dim3(MC_BLOCK), 0, (hipStream_t)stream, mc_vol(volume), tri,
                     cells + 2, list, points, (long long)N, max_distance * max_distance, triangle, closest, distance, sq_distance);
  GSD_LAUNCH_CHECK(what);
  return GSD_OK;
}

// doubles: one partial row per (start, block of 256 points)
extern "C" int64_t gsd_mesh_icp_rows_workspace(int N, int S) {
  if (N < 1 || S < 1) return 0;
  const int64_t blocks = (int64_t)S * ceil_div64(N, MC_BLOCK);
  return blocks <= INT32_MAX ? blocks * MC_ROW : 0;
}

extern "C" int gsd_mesh_icp_rows(const gsd_mesh_volume* volume, const float* tri, int T, const int32_t* cells, const int32_t* list,
                                 int64_t list_elems, const float* points, const float* weights, int N, const double* transforms, int S,
                                 double max_distance, int kind, double* rows, double* workspace, int64_t workspace_elems, void* stream) {
  const char* what = "gsd_mesh_icp_rows";
  if (mc_check_mesh(McMesh{volume, tri, T, cells, list, list_elems}, what)) return GSD_ERR_BAD_ARG;
  GSD_REQUIRE(points && transforms && rows && workspace, GSD_ERR_BAD_ARG, "%s: null pointer", what);
  const int64_t need = gsd_mesh_icp_rows_workspace(N, S);
  GSD_REQUIRE(need > 0, GSD_ERR_BAD_ARG, "%s: N=%d points and S=%d starts: both at least 1, at most 2^31-1 blocks", what, N, S);
  GSD_REQUIRE(max_distance >= 0.0, GSD_ERR_BAD_ARG, "%s: max_distance %g must be >= 0 (+inf: unlimited)", what, max_distance);
  GSD_REQUIRE(kind == 0 || kind == 1, GSD_ERR_BAD_ARG, "%s: kind %d: 0 (point to plane) or 1 (point to point)", what, kind);
  GSD_REQUIRE((((uintptr_t)transforms | (uintptr_t)rows | (uintptr_t)workspace) & 7) == 0, GSD_ERR_BAD_ARG,
              "%s: the fp64 arrays must be 8-byte aligned", what);
  GSD_REQUIRE(workspace_elems >= need, GSD_ERR_WORKSPACE, "%s: workspace of %lld doubles, need %lld", what, (long long)workspace_elems,
              (long long)need);
  const hipStream_t st = (hipStream_t)stream;
  const int nblk = (int)ceil_div64(N, MC_BLOCK);
  const auto kernel = kind == 0 ? mesh_icp_rows<0> : mesh_icp_rows<1>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(S * nblk)), dim3(MC_BLOCK), 0, st, mc_vol(volume), tri, cells + 2, list, points, weights, N,
                     nblk, transforms, max_distance * max_distance, workspace);
  GSD_LAUNCH_CHECK(what);
  hipLaunchKernelGGL(mesh_icp_rows_sum, dim3((unsigned)S), dim3(64), 0, st, (const double*)workspace, nblk, rows);
  GSD_LAUNCH_CHECK(what);
  return GSD_OK;
}

extern "C" int gsd_mesh_icp_lm_update(const gsd_icp_lm* lm, int S, double* transforms, double* lambda, double* row,
                                      double* trial_transforms, const double* trial_row, double* trace, int32_t* accepted,
                                      double* last_step, void* stream) {
  const char* what = "gsd_mesh_icp_lm_update";
  GSD_REQUIRE(lm && transforms && lambda && row && trial_transforms && trial_row && trace && accepted && last_step, GSD_ERR_BAD_ARG,
              "%s: null pointer", what);
  GSD_REQUIRE(S >= 1, GSD_ERR_BAD_ARG, "%s: %d starts, at least 1", what, S);
  GSD_REQUIRE(lm->down > 0.0 && lm->down <= 1.0 && lm->up >= 1.0 && isfinite(lm->up) && lm->lambda_min >= 0.0 &&
                  lm->lambda_max >= lm->lambda_min && isfinite(lm->lambda_max),
              GSD_ERR_BAD_ARG, "%s: need 0 < down <= 1 <= up and 0 <= lambda_min <= lambda_max, all finite", what);
  for (int k = 0; k < 6; ++k)
    GSD_REQUIRE(lm->max_step[k] >= 0.0 && isfinite(lm->max_step[k]), GSD_ERR_BAD_ARG, "%s: max_step[%d] = %g must be finite and >= 0",
                what, k, lm->max_step[k]);
  GSD_REQUIRE(lm->reserved == 0, GSD_ERR_BAD_ARG, "%s: the reserved word must be 0", what);
  GSD_REQUIRE((((uintptr_t)transforms | (uintptr_t)lambda | (uintptr_t)row | (uintptr_t)trial_transforms | (uintptr_t)trial_row |
                (uintptr_t)trace | (uintptr_t)last_step) & 7) == 0,
              GSD_ERR_BAD_ARG, "%s: the fp64 arrays must be 8-byte aligned", what);
  McLm p;
  p.down = lm->down, p.up = lm->up, p.lambda_min = lm->lambda_min, p.lambda_max = lm->lambda_max;
  for (int k = 0; k < 6; ++k) p.max_step[k] = lm->max_step[k];
  p.first = lm->first != 0;
  hipLaunchKernelGGL(mesh_icp_lm_update, dim3((unsigned)ceil_div(S, 64)), dim3(64), 0, (hipStream_t)stream, p, S, transforms, lambda, row,
                     trial_transforms, trial_row, trace, accepted, last_step);
  GSD_LAUNCH_CHECK(what);
  return GSD_OK;
}
