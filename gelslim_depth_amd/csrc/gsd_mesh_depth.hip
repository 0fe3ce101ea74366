// gsd_mesh_depth.hip -- ground-truth depth images of a rigid triangle mesh under a batch of in-hand poses (gfx950),
// include/gsd.h: gsd_mesh_depth_*.  The definition is DESIGN.md section 16; in short, for every pixel of either finger
//   right = -max(0, Qmax - g/2),   left = min(0, Qmin + g/2),
// Qmax / Qmin the largest / smallest signed perpendicular coordinate q over all triangles whose in-plane projection covers
// the pixel (edges inclusive, zero-area projections skipped, q interpolated linearly and clamped to the triangle's own range),
// 0 where nothing covers it.
//
// The mesh is rigid: everything that depends on it is built once (count -> scan -> fill) and serves any number of poses.
//
//   record (12 floats, 48 B, three 16-byte loads): the triangle's in-plane vertices SORTED lexicographically by (x, y),
//   V0 < V1 < V2, their q, and 1 / (signed doubled area), 0 for a triangle that is skipped.  Coverage is decided by the three
//   edge functions  F_ij(p) = (Vj - Vi) x (p - Vi)  of the sorted pairs (0,1), (1,2), (0,2).  Two triangles that share an edge
//   hold the same two vertex bit patterns in the same order, so both evaluate the SAME floating-point expression for that edge
//   and take it with opposite signs: a point is never rejected by both (no cracks along shared edges), and with inclusive edges
//   it may be accepted by both, which max / min do not notice.  (Vertex + two edge vectors, the textbook record, cannot give
//   that: the third edge would be a difference of differences.)
//
//   grid: nx x ny square cells over the mesh's in-plane bounding box.  A triangle is listed in every cell its vertex bounding
//   box overlaps; the render tests that same bounding box (the same fp32 values, compared exactly) before the edge functions,
//   and both sides map a coordinate to a cell with one monotone expression, so a pixel a triangle covers always finds the
//   triangle in its cell's list -- for ANY cell size.  The image therefore does not depend on the grid (tests render the same
//   batch on a one-cell grid, the default and a four times finer one and compare bits).  The order inside a list depends on
//   the atomic cursor and changes from build to build; the image does not, max and min are order-free.
//
//   render: a block of 256 threads owns a 16 x 16 pixel tile of one (pose, channel) image, a wave an 8 x 8 patch of it, so
//   the 64 mesh points of a wave fall into few cells.  A thread maps its pixel into the mesh frame (pose table: cos, sin from
//   the double-precision functions, rounded once), walks its cell's list, MD_WALK entries per trip, keeping one extreme in a
//   register (the right finger only needs Qmax, the left only Qmin = -max(-q)), and stores one float.  No atomics on the
//   image, no LDS.
//
//   pose score (gsd_mesh_pose_score): the same per-pixel function (md_pixel) on a lattice of pixels,
//   compared with an observed image in registers and reduced to five doubles per candidate pose: tile partials are stored and
//   summed by a second kernel in a fixed order, so a row is reproducible and does not depend on its batch.
//
//   pose score over G widths (gsd_mesh_pose_score_widths): md_pixel = md_depth(md_surface(pose), g/2), and
//   only md_surface is expensive.  A thread finds its point's surface value once and forms the G depths, errors and contact
//   predicates from it; the G rows are reduced in the same order as the single one, so row (b, p, k) has the bits of
//   gsd_mesh_pose_score at the width widths[b][k].
//
//   refinement past the lattice (gsd_mesh_pose_normal, gsd_mesh_depth_render_jacobian, gsd_mesh_pose_lm_update, DESIGN.md section
//   19): the walk can also say WHICH triangle gave m (md_walk<true>; the lowest id among equal values), and from that triangle's
//   slope and the derivatives of the pixel -> mesh map a thread forms dR/d(t1, t2, theta, g) in fp64.  mesh_pose_normal sums e^2,
//   J^T e and J^T J per candidate in mesh_pose_score's shape and order (entry 0 is that kernel's sum_sq to the bit),
//   mesh_render_jacobian writes the per-pixel derivatives out, mesh_pose_lm_update does a damped Gauss-Newton step's bookkeeping
//   for a batch of problems without a host read.
//
//   host layer: the render and the two score entry points share one validator (md_check: grid, view, T, list, alignment), one
//   MdView and one MdLattice builder, and one thread -> point decode on the device (md_point).  Both score entry points check
//   through md_check_score, carve their own workspace layout and hand it to one launcher, md_score: the pose table, for G > 1
//   the half-widths, the score kernel (mesh_pose_score for G = 1, mesh_pose_score_widths<CH> otherwise) and ONE rows kernel,
//   mesh_pose_rows, for every G.  gsd_mesh_pose_score_widths with G = 1 therefore makes gsd_mesh_pose_score's launches by
//   construction: it is the same call of md_score on another workspace layout.
#include "gsd_common.h"
#include "gsd_cell_lists.h"      // the count / scan / fill sequence of the cell lists
#include "gsd_lm_step.h"         // the LM accept rule and solve of mesh_pose_lm_update

#include <math.h>

namespace {

constexpr int MD_REC = GSD_MESH_RECORD_FLOATS;   // floats per triangle record
constexpr int MD_MAX_T = 1 << 24;                // triangles per mesh
constexpr int MD_MAX_N = 2048;                   // cells per grid axis
constexpr int MD_POSE = 8;                       // floats per row of the pose table
constexpr int MD_WALK = 4;                       // list entries a render thread handles per trip

struct MdGrid {
  float x0, y0, inv_cell;
  int nx, ny;
};

__device__ __forceinline__ int md_cell(float v, float g0, float inv_cell, int n) {
#pragma clang fp contract(off)
  const float f = (v - g0) * inv_cell;
  int i = (int)floorf(f);
  i = i < 0 ? 0 : i;
  return i > n - 1 ? n - 1 : i;
}

struct MdTri {
  float x0, y0, x1, y1, x2, y2, q0, q1, q2, inv;
};
__device__ __forceinline__ MdTri md_load(const float* __restrict__ rec, int id) {
  const f32x4* p = reinterpret_cast<const f32x4*>(rec + (size_t)id * MD_REC);
  const f32x4 a = p[0], b = p[1], c = p[2];
  MdTri t;
  t.x0 = a[0], t.y0 = a[1], t.x1 = a[2], t.y1 = a[3];
  t.x2 = b[0], t.y2 = b[1], t.q0 = b[2], t.q1 = b[3];
  t.q2 = c[0], t.inv = c[1];
  return t;
}

// cells [ix0, ix1] x [iy0, iy1] that the vertex bounding box of a record overlaps: the x are sorted, the y are not
__device__ __forceinline__ void md_cell_range(const MdTri& t, const MdGrid& G, int& ix0, int& ix1, int& iy0, int& iy1) {
  ix0 = md_cell(t.x0, G.x0, G.inv_cell, G.nx);
  ix1 = md_cell(t.x2, G.x0, G.inv_cell, G.nx);
  iy0 = md_cell(fminf(t.y0, fminf(t.y1, t.y2)), G.y0, G.inv_cell, G.ny);
  iy1 = md_cell(fmaxf(t.y0, fmaxf(t.y1, t.y2)), G.y0, G.inv_cell, G.ny);
}

__device__ __forceinline__ bool md_less(float ax, float ay, float bx, float by) { return ax < bx || (ax == bx && ay < by); }

// one thread per triangle: the record, and +1 on every cell its bounding box overlaps
__global__ __launch_bounds__(256) void mesh_records_count(const MdGrid G, const float* __restrict__ tri, int T,
                                                          float* __restrict__ rec, int* __restrict__ count) {
#pragma clang fp contract(off)
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= T) return;
  const float* v = tri + (size_t)id * 9;
  float ax = v[0], ay = v[1], aq = v[2], bx = v[3], by = v[4], bq = v[5], cx = v[6], cy = v[7], cq = v[8];
#define MD_SWAP(px, py, pq, rx, ry, rq)                                   \
  if (md_less(rx, ry, px, py)) {                                          \
    float s_;                                                             \
    s_ = px, px = rx, rx = s_, s_ = py, py = ry, ry = s_, s_ = pq, pq = rq, rq = s_; \
  }
  MD_SWAP(ax, ay, aq, bx, by, bq)
  MD_SWAP(bx, by, bq, cx, cy, cq)
  MD_SWAP(ax, ay, aq, bx, by, bq)
#undef MD_SWAP
  // doubled signed area from two rounded products: exactly 0 for coincident or proportional edge vectors (a vertical wall)
  const float p1 = (bx - ax) * (cy - ay), p2 = (by - ay) * (cx - ax);
  const float area = p1 - p2;
  const float inv = 1.0f / area;
  const bool ok = area != 0.f && isfinite(area) && isfinite(inv) && inv != 0.f && isfinite(aq) && isfinite(bq) && isfinite(cq);
  MdTri t;
  t.x0 = ax, t.y0 = ay, t.x1 = bx, t.y1 = by, t.x2 = cx, t.y2 = cy, t.q0 = aq, t.q1 = bq, t.q2 = cq, t.inv = ok ? inv : 0.f;
  f32x4* out = reinterpret_cast<f32x4*>(rec + (size_t)id * MD_REC);
  out[0] = f32x4{ax, ay, bx, by};
  out[1] = f32x4{cx, cy, aq, bq};
  out[2] = f32x4{cq, t.inv, 0.f, 0.f};
  if (!ok) return;
  int ix0, ix1, iy0, iy1;
  md_cell_range(t, G, ix0, ix1, iy0, iy1);
  for (int iy = iy0; iy <= iy1; ++iy)
    for (int ix = ix0; ix <= ix1; ++ix) atomicAdd(count + (size_t)iy * G.nx + ix, 1);
}

// one block: start becomes the exclusive sums of the cell counts, cursor a copy, *total the int64 total (gsd_cell_lists.h)
__global__ __launch_bounds__(GSD_CELL_SCAN_THREADS) void mesh_scan(int ncells, int* __restrict__ start, int* __restrict__ cursor,
                                                                   long long* __restrict__ total) {
  gsd_cell_scan(ncells, start, cursor, total);
}

// one thread per triangle: its id into every cell of the same range the count pass walked
__global__ __launch_bounds__(256) void mesh_fill(const MdGrid G, const float* __restrict__ rec, int T, int* __restrict__ cursor,
                                                 int* __restrict__ list, long long list_elems) {
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= T) return;
  const MdTri t = md_load(rec, id);
  if (t.inv == 0.f) return;
  int ix0, ix1, iy0, iy1;
  md_cell_range(t, G, ix0, ix1, iy0, iy1);
  for (int iy = iy0; iy <= iy1; ++iy)
    for (int ix = ix0; ix <= ix1; ++ix) {
      const int pos = atomicAdd(cursor + (size_t)iy * G.nx + ix, 1);
      if (pos >= 0 && pos < list_elems) list[pos] = id;   // a list shorter than the counted total is never overrun
    }
}

// row n of the pose table: cos, sin, 1000 t1, 1000 t2, g/2 (NaN when g is negative or not finite: the sample's images are NaN).
// `per` consecutive poses share a width: 1 for the render, the P candidates of an observation for the pose score.  A score over
// several widths keeps them in an array of its own (mesh_pose_half_widths) and passes no `widths`: the column is 0, nobody reads it.
__global__ __launch_bounds__(256) void mesh_pose_table(const float* __restrict__ poses, const float* __restrict__ widths, int N, int per,
                                                       float width_offset, float* __restrict__ table) {
#pragma clang fp contract(off)
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const float t1 = poses[3 * (size_t)n], t2 = poses[3 * (size_t)n + 1], th = poses[3 * (size_t)n + 2];
  const float g = widths != nullptr ? widths[n / per] + width_offset : 0.f;
  float* row = table + (size_t)n * MD_POSE;
  row[0] = (float)cos((double)th);
  row[1] = (float)sin((double)th);
  row[2] = 1000.f * t1;
  row[3] = 1000.f * t2;
  row[4] = (g >= 0.f && isfinite(g)) ? 0.5f * g : __builtin_nanf("");
  row[5] = row[6] = row[7] = 0.f;
}

// sg * q of triangle t at the point (x, y), -inf where t does not cover it
__device__ __forceinline__ float md_cover(const MdTri& t, float x, float y, float sg) {
#pragma clang fp contract(off)
  const float ylo = fminf(t.y0, fminf(t.y1, t.y2)), yhi = fmaxf(t.y0, fmaxf(t.y1, t.y2));
  const float d0x = x - t.x0, d0y = y - t.y0, d1x = x - t.x1, d1y = y - t.y1;
  const float e01x = t.x1 - t.x0, e01y = t.y1 - t.y0, e02x = t.x2 - t.x0, e02y = t.y2 - t.y0;
  const float e12x = t.x2 - t.x1, e12y = t.y2 - t.y1;
  const float f01 = fmaf(e01x, d0y, -(e01y * d0x));
  const float f02 = fmaf(e02x, d0y, -(e02y * d0x));
  const float f12 = fmaf(e12x, d1y, -(e12y * d1x));
  const float l2 = f01 * t.inv, l1 = -(f02 * t.inv), l0 = f12 * t.inv;   // barycentric weights of V2, V1, V0
  // the vertex bounding box first (what the binning used), then the three inclusive edges; a skipped triangle has inv = 0
  const bool in = x >= t.x0 && x <= t.x2 && y >= ylo && y <= yhi && l0 >= 0.f && l1 >= 0.f && l2 >= 0.f && t.inv != 0.f;
  float q = fmaf(l2, t.q2 - t.q0, fmaf(l1, t.q1 - t.q0, t.q0));
  const float qlo = fminf(t.q0, fminf(t.q1, t.q2)), qhi = fmaxf(t.q0, fmaxf(t.q1, t.q2));
  q = fminf(fmaxf(q, qlo), qhi);
  return in ? sg * q : -INFINITY;
}

struct MdView {
  float mpp, cx, cy;
  int swap_axes, invert, lr_flip;
  int H, W, tiles_x, tiles_y;
  int T;
  long long list_elems;
};

// What the winner-tracking walk (md_walk<true>) keeps beside m: the triangle that gave it, -1 where none covers the point --
// among equal values THE LOWEST ID, because the order inside a cell's list changes from build to build and the ids do not --
// and the point in the transformed frame, the floats that the derivatives of x and y are made of.
struct MdWin {
  int id;
  float pa, pb;
};

// The surface under pixel (r, c) of one finger under the pose-table row `row`: m = the max of sg * q over the triangles that
// cover the pixel, -inf where none does.  Everything expensive (the pixel -> mesh map, the cell lookup, the walk) is here and
// depends on the pose alone; the width enters in md_depth.  WIN also fills *win; m is the same bits either way.
template <bool WIN>
__device__ __forceinline__ float md_walk(const MdGrid& G, const MdView& V, const float* __restrict__ rec, const int* __restrict__ start,
                                         const int* __restrict__ list, const float* __restrict__ row, int r, int c, bool right,
                                         MdWin* win) {
#pragma clang fp contract(off)
  const float cs = row[0], sn = row[1], t1 = row[2], t2 = row[3];
  // pixel -> transformed in-plane point: u along the unaligned axis (mirrored for the left finger), v along the aligned one
  const float u = V.mpp * ((float)r - 0.5f * (float)V.H), v = V.mpp * ((float)c - 0.5f * (float)V.W);
  const float uu = right ? u : -u;
  const float pa = V.swap_axes ? v : uu, pb = V.swap_axes ? uu : v;   // ascending axis order
  // back into the mesh frame, relative to the mesh's in-plane centre
  float x, y;
  if (V.invert) {      // the transformed cloud was R^T (P - t): P = R P' + t
    x = fmaf(cs, pa, -(sn * pb)) + (t1 - V.cx);
    y = fmaf(sn, pa, cs * pb) + (t2 - V.cy);
  } else {             // the transformed cloud was R P + t: P = R^T (P' - t)
    const float da = pa - t1, db = pb - t2;
    x = fmaf(cs, da, sn * db) - V.cx;
    y = fmaf(cs, db, -(sn * da)) - V.cy;
  }
  const float sg = right ? 1.f : -1.f;
  float m = -INFINITY;                       // max of sg * q over the covering triangles
  int best = -1;
  const float fx = (x - G.x0) * G.inv_cell, fy = (y - G.y0) * G.inv_cell;
  // a point more than a cell outside the grid is outside every triangle's bounding box (a NaN fails the test as well)
  if (fx >= -1.f && fx <= (float)G.nx + 1.f && fy >= -1.f && fy <= (float)G.ny + 1.f) {
    const int cell = md_cell(y, G.y0, G.inv_cell, G.ny) * G.nx + md_cell(x, G.x0, G.inv_cell, G.nx);
    // the list positions are clamped into the list and the ids into the mesh before they address anything
    const int i0 = max(start[cell], 0), i1 = (int)min((long long)start[cell + 1], V.list_elems);
    for (int i = i0; i < i1; i += MD_WALK) {
      // MD_WALK entries per trip: their ids, then their records, are loaded together, so a trip costs two memory round trips
      // instead of two per triangle.  Positions past the end repeat the last entry, which max does not notice.
      int id[MD_WALK];
#pragma unroll
      for (int k = 0; k < MD_WALK; ++k) id[k] = list[min(i + k, i1 - 1)];
      MdTri tri[MD_WALK];
#pragma unroll
      for (int k = 0; k < MD_WALK; ++k) tri[k] = md_load(rec, min(max(id[k], 0), V.T - 1));
#pragma unroll
      for (int k = 0; k < MD_WALK; ++k) {
        const float q = md_cover(tri[k], x, y, sg);
        if constexpr (WIN) {     // a repeated position changes nothing: its id is not below itself
          const int t = min(max(id[k], 0), V.T - 1);
          if (q > m || (q == m && q > -INFINITY && t < best)) best = t;
        }
        m = fmaxf(m, q);
      }
    }
  }
  if constexpr (WIN) win->id = best, win->pa = pa, win->pb = pb;
  return m;
}
__device__ __forceinline__ float md_surface(const MdGrid& G, const MdView& V, const float* __restrict__ rec, const int* __restrict__ start,
                                            const int* __restrict__ list, const float* __restrict__ row, int r, int c, bool right) {
  return md_walk<false>(G, V, rec, start, list, row, r, c, right, nullptr);
}

// The depth of a surface value m (md_surface) at the half-width hg:
// right: -max(0, Qmax - g/2); left: min(0, Qmin + g/2) = -max(0, -Qmin - g/2); nothing covering: m = -inf gives 0
__device__ __forceinline__ float md_depth(float m, float hg) {
#pragma clang fp contract(off)
  float d = -fmaxf(0.f, m - hg);
  d = d == 0.f ? 0.f : d;                    // no negative zero
  if (!(hg == hg)) d = hg;                   // refused width: NaN
  return d;
}

// The depth of pixel (r, c) of one finger under the pose-table row `row`: the float mesh_render stores, and the R that
// mesh_pose_score compares -- both call this, so a scored candidate has the bits of its rendered image.
__device__ __forceinline__ float md_pixel(const MdGrid& G, const MdView& V, const float* __restrict__ rec, const int* __restrict__ start,
                                          const int* __restrict__ list, const float* __restrict__ row, int r, int c, bool right) {
  return md_depth(md_surface(G, V, rec, start, list, row, r, c, right), row[4]);
}

// The work of a thread of the render and score launches: a block of 256 threads owns a 16 x 16 tile of points of one image,
// blockIdx.x = (img * tiles_y + ty) * tiles_x + tx, a wave an 8 x 8 patch of it, a thread the point (i, j).
struct MdPoint {
  int img, n, ch;       // image n * 2 + channel: n the pose (the render) or observation * P + candidate (the score)
  int wave, lane, i, j;
};
__device__ __forceinline__ MdPoint md_point(int tiles_x, int tiles_y) {
  int b = blockIdx.x;
  const int tx = b % tiles_x;
  b /= tiles_x;
  const int ty = b % tiles_y;
  MdPoint p;
  p.img = b / tiles_y, p.n = p.img >> 1, p.ch = p.img & 1;
  p.wave = threadIdx.x >> 6, p.lane = threadIdx.x & 63;
  p.i = ty * 16 + (p.wave >> 1) * 8 + (p.lane >> 3);
  p.j = tx * 16 + (p.wave & 1) * 8 + (p.lane & 7);
  return p;
}

__global__ __launch_bounds__(256) void mesh_render(const MdGrid G, const MdView V, const float* __restrict__ rec,
                                                   const int* __restrict__ start, const int* __restrict__ list,
                                                   const float* __restrict__ table, float* __restrict__ out) {
  const MdPoint p = md_point(V.tiles_x, V.tiles_y);
  const int r = p.i, c = p.j;
  if (r >= V.H || c >= V.W) return;
  const bool right = (p.ch == 1) != (V.lr_flip != 0);
  out[((size_t)p.img * V.H + r) * V.W + c] = md_pixel(G, V, rec, start, list, table + (size_t)p.n * MD_POSE, r, c, right);
}

// ---- pose score: render and compare in registers, one row of five doubles per candidate --------------
constexpr int MD_ROW = GSD_POSE_ROW;      // sum e^2, sum |e|, #{R < -c and D < -c}, #{R < -c}, #{D < -c}

struct MdLattice {      // the pixels r = off + i * stride < H, c = off + j * stride < W, cut into 16 x 16 tiles of lattice points
  int stride, off, rows, cols, tiles_x, tiles_y;
  int P;                // candidates per observation
  float contact;
};

// A block owns a 16 x 16 tile of lattice points of one (observation, candidate, channel), a wave an 8 x 8 patch, a thread one
// point: R from md_pixel, D from the observed image, e = R - D in fp64.  The block's five values are reduced in a fixed order
// (xor butterfly inside a wave, counts by ballot, then (w0 + w1) + (w2 + w3) through LDS) and stored as partial row blockIdx.x;
// nothing is added in memory, so a partial depends on its own tile alone.
__global__ __launch_bounds__(256) void mesh_pose_score(const MdGrid G, const MdView V, const MdLattice S, const float* __restrict__ rec,
                                                       const int* __restrict__ start, const int* __restrict__ list,
                                                       const float* __restrict__ table, const float* __restrict__ observed,
                                                       double* __restrict__ partial) {
#pragma clang fp contract(off)
  const MdPoint p = md_point(S.tiles_x, S.tiles_y);
  const int n = p.n, ch = p.ch, wave = p.wave, lane = p.lane;
  double sq = 0.0, ab = 0.0;
  bool cr = false, cd = false;
  if (p.i < S.rows && p.j < S.cols) {       // a point off the lattice adds zeros; every thread reaches the reduction
    const int r = S.off + p.i * S.stride, c = S.off + p.j * S.stride;   // < H, < W: no overflow
    const bool right = (ch == 1) != (V.lr_flip != 0);
    const float R = md_pixel(G, V, rec, start, list, table + (size_t)n * MD_POSE, r, c, right);
    const float D = observed[(((size_t)(n / S.P) * 2 + ch) * V.H + r) * V.W + c];
    const double e = (double)R - (double)D;
    sq = e * e;
    ab = fabs(e);
    cr = R < -S.contact;
    cd = D < -S.contact && isfinite(D);     // a non-finite D is not contact
  }
  __shared__ double red[4][MD_ROW];
  const double s_sq = wave_sum_d(sq), s_ab = wave_sum_d(ab);
  const int n_i = __popcll(__ballot(cr && cd)), n_r = __popcll(__ballot(cr)), n_d = __popcll(__ballot(cd));
  if (lane == 0) {
    red[wave][0] = s_sq, red[wave][1] = s_ab;
    red[wave][2] = (double)n_i, red[wave][3] = (double)n_r, red[wave][4] = (double)n_d;
  }
  __syncthreads();
  if (threadIdx.x < MD_ROW) {
    const int q = threadIdx.x;
    partial[(size_t)blockIdx.x * MD_ROW + q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
  }
}

// ---- G widths per render -----------------------------------------------------------------------------
constexpr int MD_WIDTHS = GSD_POSE_WIDTHS_MAX;

// half-width k of observation b, entry b * G + k: the expression of mesh_pose_table's row[4]
__global__ __launch_bounds__(256) void mesh_pose_half_widths(const float* __restrict__ widths, int n, float width_offset,
                                                             float* __restrict__ half) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float g = widths[i] + width_offset;
  half[i] = (g >= 0.f && isfinite(g)) ? 0.5f * g : __builtin_nanf("");
}

// wave_sum_d for CH values at once (CH = 2, 4): the same tree -- lane l meets l ^ 32, then l ^ 16, ... -- but while more than
// one value is left an exchange halves them: a lane keeps the half that its bit selects and sends the other, so both lanes add the
// pair of terms that wave_sum_d adds (a + b and b + a are the same bits).  Afterwards v[0] of lane l is the wave's sum of value
// l / (64 / CH), bit for bit what wave_sum_d gives, for fewer exchanges: CH = 4 costs 2 + 1 + 4 of them instead of 4 * 6.
template <int CH>
__device__ __forceinline__ void md_wave_sums(double (&v)[CH], int lane) {
#pragma clang fp contract(off)
  int o = 32;
#pragma unroll
  for (int n = CH; n > 1; n >>= 1, o >>= 1) {
    const bool hi = (lane & o) != 0;
#pragma unroll
    for (int j = 0; j < n / 2; ++j) {
      const double keep = hi ? v[j + n / 2] : v[j], send = hi ? v[j] : v[j + n / 2];
      v[j] = keep + __shfl_xor(send, o, 64);
    }
  }
  for (; o > 0; o >>= 1) v[0] += __shfl_xor(v[0], o, 64);
}

// mesh_pose_score for NW widths per candidate: the same block, wave and thread shape, one md_surface and one D per thread, then
// per width the tail md_depth, e, e^2, |e| and the contact predicates exactly as mesh_pose_score forms them.  Widths are taken CH
// at a time (the last group repeats width NW - 1 and drops the repeats); the wave sums come from md_wave_sums, the counts from
// ballots, the four waves meet as (w0 + w1) + (w2 + w3) through LDS.  The block stores NW partial rows, blockIdx.x * NW + k.
template <int CH>
__global__ __launch_bounds__(256) void mesh_pose_score_widths(const MdGrid G, const MdView V, const MdLattice S, int NW,
                                                              const float* __restrict__ rec, const int* __restrict__ start,
                                                              const int* __restrict__ list, const float* __restrict__ table,
                                                              const float* __restrict__ half, const float* __restrict__ observed,
                                                              double* __restrict__ partial) {
#pragma clang fp contract(off)
  const MdPoint p = md_point(S.tiles_x, S.tiles_y);
  const int n = p.n, ch = p.ch, wave = p.wave, lane = p.lane;
  const float* row = table + (size_t)n * MD_POSE;
  const bool on = p.i < S.rows && p.j < S.cols;   // a point off the lattice adds zeros; every thread reaches the reductions
  float m = 0.f, D = 0.f;
  if (on) {
    const int r = S.off + p.i * S.stride, c = S.off + p.j * S.stride;   // < H, < W: no overflow
    const bool right = (ch == 1) != (V.lr_flip != 0);
    m = md_surface(G, V, rec, start, list, row, r, c, right);
    D = observed[(((size_t)(n / S.P) * 2 + ch) * V.H + r) * V.W + c];
  }
  const bool cd = on && D < -S.contact && isfinite(D);     // a non-finite D is not contact
  const int n_d = __popcll(__ballot(cd));
  __shared__ double red[4][MD_WIDTHS][MD_ROW];
  for (int k0 = 0; k0 < NW; k0 += CH) {
    double sq[CH], ab[CH];
    int n_i[CH], n_r[CH];
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const float R = md_depth(m, half[(size_t)(n / S.P) * NW + min(k0 + u, NW - 1)]);
      const double e = (double)R - (double)D;
      sq[u] = on ? e * e : 0.0;
      ab[u] = on ? fabs(e) : 0.0;
      const bool cr = on && R < -S.contact;
      n_i[u] = __popcll(__ballot(cr && cd)), n_r[u] = __popcll(__ballot(cr));
    }
    md_wave_sums<CH>(sq, lane);
    md_wave_sums<CH>(ab, lane);
#pragma unroll
    for (int u = 0; u < CH; ++u)
      if (lane == u * (64 / CH) && k0 + u < NW) {
        double* w = red[wave][k0 + u];
        w[0] = sq[0], w[1] = ab[0], w[2] = (double)n_i[u], w[3] = (double)n_r[u], w[4] = (double)n_d;
      }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < NW * MD_ROW; t += 256) {
    const int k = t / MD_ROW, q = t - k * MD_ROW;
    partial[((size_t)blockIdx.x * NW + k) * MD_ROW + q] = (red[0][k][q] + red[1][k][q]) + (red[2][k][q] + red[3][k][q]);
  }
}

// One wave per (candidate n, width k), block n * NW + k: lane l adds the partial rows l, l + 64, ... of the candidate's `tpc` tiles
// in ascending order, the 64 lane sums meet in the xor butterfly.  The order is a function of tpc alone.  A refused width gives
// five NaN; its mark is the NaN half-width flag[(n / per) * step + k]: {table + 4, 1, MD_POSE} for the one width of a pose-table
// row, {half, P, NW} for the array of several.
// ROW is the row's length: MD_ROW here, MD_NROW for the normal rows of section 19 (mesh_pose_normal_sum), which add in this order.
template <int ROW>
__device__ __forceinline__ void md_sum_rows(const double* __restrict__ partial, int tpc, int NW, const float* __restrict__ flag, int per,
                                            int step, double* __restrict__ rows) {
#pragma clang fp contract(off)
  const int n = blockIdx.x / NW, k = blockIdx.x - n * NW, lane = threadIdx.x;
  double tot[ROW];
#pragma unroll
  for (int q = 0; q < ROW; ++q) tot[q] = 0.0;
  for (int t = lane; t < tpc; t += 64) {
    const double* p = partial + (((size_t)n * tpc + t) * NW + k) * ROW;
#pragma unroll
    for (int q = 0; q < ROW; ++q) tot[q] += p[q];
  }
#pragma unroll
  for (int q = 0; q < ROW; ++q) tot[q] = wave_sum_d(tot[q]);
  const float hg = flag[(size_t)(n / per) * step + k];
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < ROW; ++q) rows[(size_t)blockIdx.x * ROW + q] = hg == hg ? tot[q] : (double)hg;
  }
}
__global__ __launch_bounds__(64) void mesh_pose_rows(const double* __restrict__ partial, int tpc, int NW, const float* __restrict__ flag,
                                                     int per, int step, double* __restrict__ rows) {
  md_sum_rows<MD_ROW>(partial, tpc, NW, flag, per, step, rows);
}

// ---- refinement past the lattice: normal-equation rows, the Jacobian image, the damped step -----------
constexpr int MD_NROW = GSD_POSE_NORMAL_ROW;   // sum e^2, #active, sum J_k e (a1, a2, theta, g), sum J_j J_k (j <= k, row-major)

// dR/d(a1, a2, theta) of a point whose walk ended on `w` and whose depth is R, a1 = 1000 t1 and a2 = 1000 t2 in mm: 0 unless the
// point is active (R < 0, which needs a winner).  In fp64 from floats alone: the winner's record, reloaded once -- its slope
// (qx, qy), the clamp of q to the triangle's range ignored -- and cs, sn, pa, pb, da, db as md_walk formed them.
__device__ __forceinline__ void md_jacobian(const MdView& V, const float* __restrict__ rec, const float* __restrict__ row, const MdWin& w,
                                            bool right, float R, double (&J)[3]) {
#pragma clang fp contract(off)
  J[0] = J[1] = J[2] = 0.0;
  if (!(R < 0.f) || w.id < 0) return;
  const MdTri t = md_load(rec, w.id);
  const double a = (double)t.q1 - (double)t.q0, b = (double)t.q2 - (double)t.q0, inv = (double)t.inv;
  const double qx = (a * ((double)t.y2 - (double)t.y0) - b * ((double)t.y1 - (double)t.y0)) * inv;
  const double qy = (b * ((double)t.x1 - (double)t.x0) - a * ((double)t.x2 - (double)t.x0)) * inv;
  const double cs = row[0], sn = row[1], pa = w.pa, pb = w.pb;
  const double da = (double)(w.pa - row[2]), db = (double)(w.pb - row[3]);   // the fp32 differences of md_walk
  const double sg = right ? 1.0 : -1.0;
  double xk[3], yk[3];
  if (V.invert) {
    xk[0] = 1.0, xk[1] = 0.0, xk[2] = -sn * pa - cs * pb;
    yk[0] = 0.0, yk[1] = 1.0, yk[2] = cs * pa - sn * pb;
  } else {
    xk[0] = -cs, xk[1] = -sn, xk[2] = -sn * da + cs * db;
    yk[0] = sn, yk[1] = -cs, yk[2] = -sn * db - cs * da;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) J[k] = -sg * (qx * xk[k] + qy * yk[k]);
}

// mesh_pose_score's block, wave and thread shape; a thread adds its point's e^2, J_k e and J_j J_k (J_g = 0.5 where the point is
// active).  The 15 sums go through md_wave_sums<4> in four groups (slot 1 of the 16 is the count, a ballot), the four waves meet
// as (w0 + w1) + (w2 + w3) through LDS and the block stores partial row blockIdx.x: entry 0 takes mesh_pose_score's path to the bit.
__global__ __launch_bounds__(256) void mesh_pose_normal(const MdGrid G, const MdView V, const MdLattice S, const float* __restrict__ rec,
                                                        const int* __restrict__ start, const int* __restrict__ list,
                                                        const float* __restrict__ table, const float* __restrict__ observed,
                                                        double* __restrict__ partial) {
#pragma clang fp contract(off)
  const MdPoint p = md_point(S.tiles_x, S.tiles_y);
  const int n = p.n, ch = p.ch, wave = p.wave, lane = p.lane;
  double e = 0.0, J[4] = {0.0, 0.0, 0.0, 0.0};
  bool active = false;
  if (p.i < S.rows && p.j < S.cols) {       // a point off the lattice adds zeros; every thread reaches the reduction
    const int r = S.off + p.i * S.stride, c = S.off + p.j * S.stride;   // < H, < W: no overflow
    const bool right = (ch == 1) != (V.lr_flip != 0);
    const float* row = table + (size_t)n * MD_POSE;
    MdWin w;
    const float R = md_depth(md_walk<true>(G, V, rec, start, list, row, r, c, right, &w), row[4]);
    const float D = observed[(((size_t)(n / S.P) * 2 + ch) * V.H + r) * V.W + c];
    e = (double)R - (double)D;
    active = R < 0.f;
    double J3[3];
    md_jacobian(V, rec, row, w, right, R, J3);
    J[0] = J3[0], J[1] = J3[1], J[2] = J3[2], J[3] = active ? 0.5 : 0.0;
  }
  double v[4][4];                           // slot 4 g + u is row entry 4 g + u
  v[0][0] = e * e, v[0][1] = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) v[(2 + k) >> 2][(2 + k) & 3] = J[k] * e;
  {
    int s = 6;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = j; k < 4; ++k, ++s) v[s >> 2][s & 3] = J[j] * J[k];
  }
  const int n_active = __popcll(__ballot(active));
  __shared__ double red[4][MD_NROW];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    md_wave_sums<4>(v[g], lane);
    if ((lane & 15) == 0) {
      const int slot = 4 * g + (lane >> 4);
      red[wave][slot] = slot == 1 ? (double)n_active : v[g][0];
    }
  }
  __syncthreads();
  if (threadIdx.x < MD_NROW) {
    const int q = threadIdx.x;
    partial[(size_t)blockIdx.x * MD_NROW + q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
  }
}

// mesh_pose_rows for rows of MD_NROW: one wave per candidate, 16 NaN for a refused width (the NaN half-width of its table row)
__global__ __launch_bounds__(64) void mesh_pose_normal_sum(const double* __restrict__ partial, int tpc, const float* __restrict__ table,
                                                           double* __restrict__ rows) {
  md_sum_rows<MD_NROW>(partial, tpc, 1, table + 4, 1, MD_POSE, rows);
}

// mesh_render's launch; writes J_a1, J_a2, J_theta of every pixel as doubles, (N, 2, 3, H, W): what mesh_pose_normal sums, to look at
__global__ __launch_bounds__(256) void mesh_render_jacobian(const MdGrid G, const MdView V, const float* __restrict__ rec,
                                                            const int* __restrict__ start, const int* __restrict__ list,
                                                            const float* __restrict__ table, double* __restrict__ out) {
  const MdPoint p = md_point(V.tiles_x, V.tiles_y);
  const int r = p.i, c = p.j;
  if (r >= V.H || c >= V.W) return;
  const bool right = (p.ch == 1) != (V.lr_flip != 0);
  const float* row = table + (size_t)p.n * MD_POSE;
  MdWin w;
  const float R = md_depth(md_walk<true>(G, V, rec, start, list, row, r, c, right, &w), row[4]);
  double J[3];
  md_jacobian(V, rec, row, w, right, R, J);
#pragma unroll
  for (int k = 0; k < 3; ++k) out[(((size_t)p.img * 3 + k) * V.H + r) * V.W + c] = J[k];
}

struct MdLm {           // gsd_pose_lm by value
  double down, up, lambda_min, lambda_max, max_step[4];
  int free_mask, first;
};

// One thread per problem, fp64 (the definition is include/gsd.h's).  The system is always 4 x 4: a parameter that is not free has
// the identity's row and column and a zero right-hand side, so its step is exactly 0, the others' factorisation meets only exact
// zeros from it, and every index is a constant -- the matrix lives in registers.
__global__ __launch_bounds__(64) void mesh_pose_lm_update(const MdLm lm, int B, float* __restrict__ pose, float* __restrict__ width,
                                                          double* __restrict__ lambda, double* __restrict__ row,
                                                          float* __restrict__ trial_pose, float* __restrict__ trial_width,
                                                          const double* __restrict__ trial_row, double* __restrict__ trace,
                                                          int* __restrict__ accepted, double* __restrict__ last_step) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= B) return;
  double cur[MD_NROW];
#pragma unroll
  for (int q = 0; q < MD_NROW; ++q) cur[q] = row[(size_t)i * MD_NROW + q];
  float t1 = pose[3 * (size_t)i], t2 = pose[3 * (size_t)i + 1], th = pose[3 * (size_t)i + 2], g = width[i];
  double lam = lambda[i];
  int count = lm.first ? 0 : accepted[i];
  const bool take = gsd_lm_accept(lm, trial_row[(size_t)i * MD_NROW], cur[0], lam, count);
  if (take) {
#pragma unroll
    for (int q = 0; q < MD_NROW; ++q) cur[q] = trial_row[(size_t)i * MD_NROW + q];
    t1 = trial_pose[3 * (size_t)i], t2 = trial_pose[3 * (size_t)i + 1], th = trial_pose[3 * (size_t)i + 2], g = trial_width[i];
  }
  double d[4];      // the step in the order a1, a2, theta, g
  gsd_lm_solve<4>(cur + 6, cur + 2, lam, (unsigned)lm.free_mask, lm.max_step, d);
  if (take) {
#pragma unroll
    for (int q = 0; q < MD_NROW; ++q) row[(size_t)i * MD_NROW + q] = cur[q];
    pose[3 * (size_t)i] = t1, pose[3 * (size_t)i + 1] = t2, pose[3 * (size_t)i + 2] = th, width[i] = g;
  }
  lambda[i] = lam, accepted[i] = count, trace[i] = cur[0];
  trial_pose[3 * (size_t)i] = (float)((double)t1 + d[0] / 1000.0);
  trial_pose[3 * (size_t)i + 1] = (float)((double)t2 + d[1] / 1000.0);
  trial_pose[3 * (size_t)i + 2] = (float)((double)th + d[2]);
  trial_width[i] = (float)((double)g + d[3]);
#pragma unroll
  for (int k = 0; k < 4; ++k) last_step[4 * (size_t)i + k] = fabs(d[k]);
}

// lattice points along an axis of `len` pixels
int md_lattice_len(int len, int stride) {
  const int off = stride / 2;
  return off < len ? (len - 1 - off) / stride + 1 : 0;
}
MdLattice md_lattice(int H, int W, int stride, int P, float contact) {
  MdLattice S;
  S.stride = stride, S.off = stride / 2, S.rows = md_lattice_len(H, stride), S.cols = md_lattice_len(W, stride);
  S.tiles_x = ceil_div(S.cols, 16), S.tiles_y = ceil_div(S.rows, 16), S.P = P, S.contact = contact;
  return S;
}
// blocks of the score launch (the tiles that md_point decodes), or -1 when an argument is out of range
int64_t md_score_blocks(int B, int P, int H, int W, int stride) {
  if (B < 1 || P < 1 || H < 1 || W < 1 || stride < 1 || (int64_t)B * P > INT32_MAX) return -1;
  const MdLattice S = md_lattice(H, W, stride, P, 0.f);
  return (int64_t)S.tiles_x * S.tiles_y * 2 * ((int64_t)B * P);
}

int md_check_grid(const gsd_mesh_grid* g, const char* what) {
  GSD_REQUIRE(g != nullptr, GSD_ERR_BAD_ARG, "%s: null grid", what);
  GSD_REQUIRE(g->nx >= 1 && g->ny >= 1 && g->nx <= MD_MAX_N && g->ny <= MD_MAX_N, GSD_ERR_BAD_ARG,
              "%s: grid of %d x %d cells, 1..%d per axis", what, g->nx, g->ny, MD_MAX_N);
  GSD_REQUIRE(isfinite(g->x0) && isfinite(g->y0) && isfinite(g->cx) && isfinite(g->cy) && isfinite(g->cell) && g->cell > 0.f &&
                  isfinite(g->inv_cell) && g->inv_cell > 0.f,
              GSD_ERR_BAD_ARG, "%s: grid origin, centre and cell size must be finite, the cell size positive", what);
  GSD_REQUIRE(g->reserved[0] == 0 && g->reserved[1] == 0, GSD_ERR_BAD_ARG, "%s: the reserved words must be 0", what);
  return 0;
}
MdGrid md_grid(const gsd_mesh_grid* g) {
  MdGrid G;
  G.x0 = g->x0, G.y0 = g->y0, G.inv_cell = g->inv_cell, G.nx = g->nx, G.ny = g->ny;
  return G;
}
int64_t md_cells(const gsd_mesh_grid* g) { return (int64_t)g->nx * g->ny; }

// ---- the host layer of the three launching entry points; `what` is the one that was called and begins every message ----------
struct MdMesh {         // a built mesh and the view of it, as the caller passed them
  const gsd_mesh_grid* grid;
  const gsd_mesh_view* view;
  const float* records;
  int T;
  const int32_t* cells;
  const int32_t* list;
  int64_t list_elems;
};
int md_check(const MdMesh& M, const char* what) {
  if (md_check_grid(M.grid, what)) return GSD_ERR_BAD_ARG;
  GSD_REQUIRE(M.view && M.records && M.cells && M.list, GSD_ERR_BAD_ARG, "%s: null pointer", what);
  GSD_REQUIRE(isfinite(M.view->mpp) && M.view->mpp > 0.f && isfinite(M.view->width_offset), GSD_ERR_BAD_ARG,
              "%s: mm per pixel %g must be finite and positive, the width offset %g finite", what, (double)M.view->mpp,
              (double)M.view->width_offset);
  GSD_REQUIRE(M.view->reserved == 0, GSD_ERR_BAD_ARG, "%s: the reserved word must be 0", what);
  GSD_REQUIRE(M.T >= 1 && M.T <= MD_MAX_T, GSD_ERR_BAD_ARG, "%s: %d triangles, 1..%d", what, M.T, MD_MAX_T);
  GSD_REQUIRE(M.list_elems >= 1 && M.list_elems <= INT32_MAX, GSD_ERR_BAD_ARG, "%s: list of %lld entries, 1..2^31-1", what,
              (long long)M.list_elems);
  GSD_REQUIRE(((uintptr_t)M.records & 15) == 0, GSD_ERR_BAD_ARG, "%s: records must be 16-byte aligned", what);
  return 0;
}
MdView md_view(const MdMesh& M, int H, int W) {
  MdView V;
  V.mpp = M.view->mpp, V.cx = M.grid->cx, V.cy = M.grid->cy;
  V.swap_axes = M.view->swap_axes != 0, V.invert = M.view->invert_affine != 0, V.lr_flip = M.view->lr_flip != 0;
  V.H = H, V.W = W, V.tiles_x = ceil_div(W, 16), V.tiles_y = ceil_div(H, 16), V.T = M.T, V.list_elems = M.list_elems;
  return V;
}

struct MdScore {        // what is scored: G widths per observation, G = 1 for gsd_mesh_pose_score
  const float* observed;
  int B;
  const float* candidates;
  const float* widths;
  int P, G, H, W, stride;
  float contact;
  double* rows;
};
// everything a score entry point refuses (all of it GSD_ERR_BAD_ARG); `need` is its own workspace formula
int md_check_score(const MdMesh& M, const MdScore& Q, const double* workspace, int64_t workspace_elems, int64_t need, const char* what) {
  if (md_check(M, what)) return GSD_ERR_BAD_ARG;
  GSD_REQUIRE(Q.observed && Q.candidates && Q.widths && Q.rows && workspace, GSD_ERR_BAD_ARG, "%s: null pointer", what);
  GSD_REQUIRE(Q.B >= 1 && Q.P >= 1 && Q.H >= 1 && Q.W >= 1, GSD_ERR_BAD_ARG, "%s: bad dims B=%d P=%d H=%d W=%d", what, Q.B, Q.P, Q.H,
              Q.W);
  GSD_REQUIRE(Q.G >= 1 && Q.G <= MD_WIDTHS, GSD_ERR_BAD_ARG, "%s: %d widths per observation, 1..%d", what, Q.G, MD_WIDTHS);
  GSD_REQUIRE(Q.stride >= 1, GSD_ERR_BAD_ARG, "%s: stride %d must be at least 1", what, Q.stride);
  GSD_REQUIRE(isfinite(Q.contact) && Q.contact >= 0.f, GSD_ERR_BAD_ARG, "%s: contact_depth %g must be finite and >= 0", what,
              (double)Q.contact);
  GSD_REQUIRE(((uintptr_t)Q.rows & 7) == 0 && ((uintptr_t)workspace & 7) == 0, GSD_ERR_BAD_ARG,
              "%s: rows and workspace must be 8-byte aligned", what);
  const int64_t blocks = md_score_blocks(Q.B, Q.P, Q.H, Q.W, Q.stride);
  GSD_REQUIRE(blocks >= 0 && blocks <= INT32_MAX && (int64_t)Q.B * Q.P * Q.G <= INT32_MAX, GSD_ERR_BAD_ARG,
              "%s: %lld blocks (B=%d x P=%d of %d x %d, stride %d) and %lld rows, at most 2^31-1 per launch", what, (long long)blocks, Q.B,
              Q.P, Q.H, Q.W, Q.stride, (long long)Q.B * Q.P * Q.G);
  GSD_REQUIRE(workspace_elems >= need, GSD_ERR_BAD_ARG, "%s: workspace of %lld doubles, need %lld", what, (long long)workspace_elems,
              (long long)need);
  return 0;
}
// The launches of both score entry points, on workspace that the caller has carved: the pose table, for G > 1 the half-widths,
// the score kernel (one partial row per block and width) and the rows kernel.  G = 1 keeps its width in the pose table.
int md_score(const MdMesh& M, const MdScore& Q, float* table, float* half, double* partial, hipStream_t st, const char* what) {
  const int N = Q.B * Q.P, G = Q.G;
  const int64_t blocks = md_score_blocks(Q.B, Q.P, Q.H, Q.W, Q.stride);
  hipLaunchKernelGGL(mesh_pose_table, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, st, Q.candidates, G == 1 ? Q.widths : nullptr, N,
                     Q.P, M.view->width_offset, table);
  GSD_LAUNCH_CHECK(what);
  if (G > 1) {
    hipLaunchKernelGGL(mesh_pose_half_widths, dim3((unsigned)ceil_div(Q.B * G, 256)), dim3(256), 0, st, Q.widths, Q.B * G,
                       M.view->width_offset, half);
    GSD_LAUNCH_CHECK(what);
  }
  if (blocks > 0) {      // a stride that leaves no lattice point: every row is five zeros
    const MdGrid grid = md_grid(M.grid);
    const MdView V = md_view(M, Q.H, Q.W);
    const MdLattice S = md_lattice(Q.H, Q.W, Q.stride, Q.P, Q.contact);
    if (G == 1) {
      hipLaunchKernelGGL(mesh_pose_score, dim3((unsigned)blocks), dim3(256), 0, st, grid, V, S, M.records, M.cells + 2, M.list,
                         (const float*)table, Q.observed, partial);
    } else {
      const auto kernel = G == 2 ? mesh_pose_score_widths<2> : mesh_pose_score_widths<4>;
      hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, st, grid, V, S, G, M.records, M.cells + 2, M.list,
                         (const float*)table, (const float*)half, Q.observed, partial);
    }
    GSD_LAUNCH_CHECK(what);
  }
  hipLaunchKernelGGL(mesh_pose_rows, dim3((unsigned)(N * G)), dim3(64), 0, st, (const double*)partial, (int)(blocks / N), G,
                     G == 1 ? (const float*)table + 4 : (const float*)half, G == 1 ? 1 : Q.P, G == 1 ? MD_POSE : G, Q.rows);
  GSD_LAUNCH_CHECK(what);
  return GSD_OK;
}

}   // namespace

extern "C" int gsd_mesh_depth_plan(const double* bbox, double cell_mm, gsd_mesh_grid* grid) {
  GSD_REQUIRE(bbox && grid, GSD_ERR_BAD_ARG, "gsd_mesh_depth_plan: null pointer");
  const double x0 = bbox[0], y0 = bbox[1], x1 = bbox[2], y1 = bbox[3];
  GSD_REQUIRE(isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1) && x1 >= x0 && y1 >= y0, GSD_ERR_BAD_ARG,
              "gsd_mesh_depth_plan: bounding box (%g, %g)-(%g, %g) must be finite and ordered", x0, y0, x1, y1);
  GSD_REQUIRE(isfinite(cell_mm) && cell_mm > 0.0, GSD_ERR_BAD_ARG, "gsd_mesh_depth_plan: cell size %g must be finite and positive",
              cell_mm);
  const double ext = fmax(fmax(x1 - x0, y1 - y0), 1e-30);
  double cell = fmax(cell_mm, ext / (MD_MAX_N - 2));      // at most MD_MAX_N cells per axis
  const double pad = 1e-3 * cell;                          // the fp32 vertices stay strictly inside the grid
  const double cx = 0.5 * (x0 + x1), cy = 0.5 * (y0 + y1);
  const int nx = (int)fmin((double)MD_MAX_N, fmax(1.0, ceil((x1 - x0 + 2 * pad) / cell)));
  const int ny = (int)fmin((double)MD_MAX_N, fmax(1.0, ceil((y1 - y0 + 2 * pad) / cell)));
  grid->cx = (float)cx, grid->cy = (float)cy;
  grid->x0 = (float)(x0 - pad - cx), grid->y0 = (float)(y0 - pad - cy);    // records are relative to (cx, cy)
  grid->cell = (float)cell, grid->inv_cell = (float)(1.0 / cell);
  grid->nx = nx, grid->ny = ny;
  grid->reserved[0] = grid->reserved[1] = 0;
  return md_check_grid(grid, "gsd_mesh_depth_plan") ? GSD_ERR_BAD_ARG : GSD_OK;
}

extern "C" int64_t gsd_mesh_depth_workspace(const gsd_mesh_grid* grid) {
  if (grid == nullptr || grid->nx < 1 || grid->ny < 1 || grid->nx > MD_MAX_N || grid->ny > MD_MAX_N) return 0;
  return gsd_cell_words(md_cells(grid));
}

extern "C" int gsd_mesh_depth_count(const gsd_mesh_grid* grid, const float* tri, int T, float* records, int32_t* cells,
                                    int64_t cells_elems, void* stream) {
  const char* what = "gsd_mesh_depth_count";
  if (md_check_grid(grid, what)) return GSD_ERR_BAD_ARG;
  GSD_REQUIRE(records != nullptr, GSD_ERR_BAD_ARG, "%s: null pointer", what);
  GSD_REQUIRE(((uintptr_t)records & 15) == 0, GSD_ERR_BAD_ARG, "%s: records must be 16-byte aligned", what);
  const hipStream_t st = (hipStream_t)stream;
  const auto count = [&](int* start) {
    hipLaunchKernelGGL(mesh_records_count, dim3((unsigned)ceil_div(T, 256)), dim3(256), 0, st, md_grid(grid), tri, T, records, start);
  };
  return gsd_cell_count(GsdCellCall{what, tri, T, MD_MAX_T, md_cells(grid), cells, cells_elems, nullptr, 0}, count, mesh_scan, st);
}

extern "C" int gsd_mesh_depth_fill(const gsd_mesh_grid* grid, const float* records, int T, int32_t* cells, int64_t cells_elems,
                                   int32_t* list, int64_t list_elems, void* stream) {
  const char* what = "gsd_mesh_depth_fill";
  if (md_check_grid(grid, what)) return GSD_ERR_BAD_ARG;
  GSD_REQUIRE(((uintptr_t)records & 15) == 0, GSD_ERR_BAD_ARG, "%s: records must be 16-byte aligned", what);
  return gsd_cell_fill(GsdCellCall{what, records, T, MD_MAX_T, md_cells(grid), cells, cells_elems, list, list_elems}, mesh_fill,
                       md_grid(grid), (hipStream_t)stream);
}

extern "C" int64_t gsd_mesh_depth_render_workspace(int N) { return N > 0 ? (int64_t)N * MD_POSE : 0; }

namespace {
// gsd_mesh_depth_render and gsd_mesh_depth_render_jacobian: the same checks, pose table and grid of blocks; `kernel` writes `out`
template <typename Out, typename Kernel>
int md_render(Kernel kernel, const char* what, const MdMesh& M, const float* poses, const float* widths, int N, int H, int W, Out* out,
              float* workspace, int64_t workspace_elems, void* stream) {
  if (md_check(M, what)) return GSD_ERR_BAD_ARG;
  GSD_REQUIRE(poses && widths && out && workspace, GSD_ERR_BAD_ARG, "%s: null pointer", what);
  GSD_REQUIRE(N >= 1 && H >= 1 && W >= 1, GSD_ERR_BAD_ARG, "%s: bad dims N=%d H=%d W=%d", what, N, H, W);
  GSD_REQUIRE(workspace_elems >= (int64_t)N * MD_POSE, GSD_ERR_WORKSPACE, "%s: workspace of %lld floats, need %lld", what,
              (long long)workspace_elems, (long long)N * MD_POSE);
  const MdView V = md_view(M, H, W);
  const int64_t blocks = (int64_t)V.tiles_x * V.tiles_y * 2 * N;
  GSD_REQUIRE(blocks <= INT32_MAX, GSD_ERR_UNSUPPORTED, "%s: %lld blocks (N=%d of %d x %d), at most 2^31-1 per launch", what,
              (long long)blocks, N, H, W);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mesh_pose_table, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, st, poses, widths, N, 1, M.view->width_offset,
                     workspace);
  GSD_LAUNCH_CHECK(what);
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, st, md_grid(M.grid), V, M.records, M.cells + 2, M.list,
                     (const float*)workspace, out);
  GSD_LAUNCH_CHECK(what);
  return GSD_OK;
}
}   // namespace

extern "C" int gsd_mesh_depth_render(const gsd_mesh_grid* grid, const gsd_mesh_view* view, const float* records, int T,
                                     const int32_t* cells, const int32_t* list, int64_t list_elems, const float* poses,
                                     const float* widths, int N, int H, int W, float* out, float* workspace,
                                     int64_t workspace_elems, void* stream) {
  return md_render(mesh_render, "gsd_mesh_depth_render", MdMesh{grid, view, records, T, cells, list, list_elems}, poses, widths, N, H, W,
                   out, workspace, workspace_elems, stream);
}

extern "C" int gsd_mesh_depth_render_jacobian(const gsd_mesh_grid* grid, const gsd_mesh_view* view, const float* records, int T,
                                              const int32_t* cells, const int32_t* list, int64_t list_elems, const float* poses,
                                              const float* widths, int N, int H, int W, double* out, float* workspace,
                                              int64_t workspace_elems, void* stream) {
  const char* what = "gsd_mesh_depth_render_jacobian";
  GSD_REQUIRE(((uintptr_t)out & 7) == 0, GSD_ERR_BAD_ARG, "%s: out must be 8-byte aligned", what);
  return md_render(mesh_render_jacobian, what, MdMesh{grid, view, records, T, cells, list, list_elems}, poses, widths, N, H, W, out,
                   workspace, workspace_elems, stream);
}

// doubles: the pose table (8 floats a row) | one partial row per block
extern "C" int64_t gsd_mesh_pose_score_workspace(int B, int P, int H, int W, int stride) {
  const int64_t blocks = md_score_blocks(B, P, H, W, stride);
  if (blocks < 0 || blocks > INT32_MAX) return 0;
  return (int64_t)B * P * (MD_POSE / 2) + blocks * MD_ROW;
}

extern "C" int gsd_mesh_pose_score(const gsd_mesh_grid* grid, const gsd_mesh_view* view, const float* records, int T,
                                   const int32_t* cells, const int32_t* list, int64_t list_elems, const float* observed, int B,
                                   const float* candidates, const float* widths, int P, int H, int W, int stride, float contact_depth,
                                   double* rows, double* workspace, int64_t workspace_elems, void* stream) {
  const char* what = "gsd_mesh_pose_score";
  const MdMesh M{grid, view, records, T, cells, list, list_elems};
  const MdScore Q{observed, B, candidates, widths, P, 1, H, W, stride, contact_depth, rows};
  if (md_check_score(M, Q, workspace, workspace_elems, gsd_mesh_pose_score_workspace(B, P, H, W, stride), what)) return GSD_ERR_BAD_ARG;
  const int64_t table_words = (int64_t)B * P * (MD_POSE / 2);
  return md_score(M, Q, reinterpret_cast<float*>(workspace), nullptr, workspace + table_words, (hipStream_t)stream, what);
}

// doubles: the pose table (8 floats a row) | the half-widths (B x G floats, rounded up to whole doubles) | G partial rows per block
extern "C" int64_t gsd_mesh_pose_score_widths_workspace(int B, int P, int G, int H, int W, int stride) {
  const int64_t blocks = md_score_blocks(B, P, H, W, stride);
  if (blocks < 0 || blocks > INT32_MAX || G < 1 || G > MD_WIDTHS || (int64_t)B * P * G > INT32_MAX) return 0;
  return (int64_t)B * P * (MD_POSE / 2) + ((int64_t)B * G + 1) / 2 + blocks * G * MD_ROW;
}

// G = 1 (widths is gsd_mesh_pose_score's B floats) makes that call's launches, on this layout
extern "C" int gsd_mesh_pose_score_widths(const gsd_mesh_grid* grid, const gsd_mesh_view* view, const float* records, int T,
                                          const int32_t* cells, const int32_t* list, int64_t list_elems, const float* observed, int B,
                                          const float* candidates, const float* widths, int P, int G, int H, int W, int stride,
                                          float contact_depth, double* rows, double* workspace, int64_t workspace_elems, void* stream) {
  const char* what = "gsd_mesh_pose_score_widths";
  const MdMesh M{grid, view, records, T, cells, list, list_elems};
  const MdScore Q{observed, B, candidates, widths, P, G, H, W, stride, contact_depth, rows};
  if (md_check_score(M, Q, workspace, workspace_elems, gsd_mesh_pose_score_widths_workspace(B, P, G, H, W, stride), what))
    return GSD_ERR_BAD_ARG;
  const int64_t table_words = (int64_t)B * P * (MD_POSE / 2), half_words = ((int64_t)B * G + 1) / 2;
  return md_score(M, Q, reinterpret_cast<float*>(workspace), reinterpret_cast<float*>(workspace + table_words),
                  workspace + table_words + half_words, (hipStream_t)stream, what);
}

// doubles: the pose table (8 floats a row) | one partial row of MD_NROW per block
extern "C" int64_t gsd_mesh_pose_normal_workspace(int B, int P, int H, int W, int stride) {
  const int64_t blocks = md_score_blocks(B, P, H, W, stride);
  if (blocks < 0 || blocks > INT32_MAX) return 0;
  return (int64_t)B * P * (MD_POSE / 2) + blocks * MD_NROW;
}

// md_score's launches with the normal kernels: the pose table with one width per candidate (per = 1), one partial row per block,
// one wave per candidate
extern "C" int gsd_mesh_pose_normal(const gsd_mesh_grid* grid, const gsd_mesh_view* view, const float* records, int T,
                                    const int32_t* cells, const int32_t* list, int64_t list_elems, const float* observed, int B,
                                    const float* candidates, const float* widths, int P, int H, int W, int stride, double* rows,
                                    double* workspace, int64_t workspace_elems, void* stream) {
  const char* what = "gsd_mesh_pose_normal";
  const MdMesh M{grid, view, records, T, cells, list, list_elems};
  const MdScore Q{observed, B, candidates, widths, P, 1, H, W, stride, 0.f, rows};
  if (md_check_score(M, Q, workspace, workspace_elems, gsd_mesh_pose_normal_workspace(B, P, H, W, stride), what)) return GSD_ERR_BAD_ARG;
  const int N = B * P;
  const int64_t blocks = md_score_blocks(B, P, H, W, stride);
  float* table = reinterpret_cast<float*>(workspace);
  double* partial = workspace + (int64_t)N * (MD_POSE / 2);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mesh_pose_table, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, st, candidates, widths, N, 1, view->width_offset,
                     table);
  GSD_LAUNCH_CHECK(what);
  if (blocks > 0) {      // a stride that leaves no lattice point: every row is 16 zeros
    hipLaunchKernelGGL(mesh_pose_normal, dim3((unsigned)blocks), dim3(256), 0, st, md_grid(grid), md_view(M, H, W),
                       md_lattice(H, W, stride, P, 0.f), records, cells + 2, list, (const float*)table, observed, partial);
    GSD_LAUNCH_CHECK(what);
  }
  hipLaunchKernelGGL(mesh_pose_normal_sum, dim3((unsigned)N), dim3(64), 0, st, (const double*)partial, (int)(blocks / N),
                     (const float*)table, rows);
  GSD_LAUNCH_CHECK(what);
  return GSD_OK;
}

extern "C" int gsd_mesh_pose_lm_update(const gsd_pose_lm* lm, int B, float* pose, float* width, double* lambda, double* row,
                                       float* trial_pose, float* trial_width, const double* trial_row, double* trace,
                                       int32_t* accepted, double* last_step, void* stream) {
  const char* what = "gsd_mesh_pose_lm_update";
  GSD_REQUIRE(lm && pose && width && lambda && row && trial_pose && trial_width && trial_row && trace && accepted && last_step,
              GSD_ERR_BAD_ARG, "%s: null pointer", what);
  GSD_REQUIRE(B >= 1, GSD_ERR_BAD_ARG, "%s: %d problems, at least 1", what, B);
  GSD_REQUIRE((lm->free_mask & 7) == 7 && (lm->free_mask & ~15) == 0, GSD_ERR_BAD_ARG,
              "%s: free_mask %d: bits 0..2 (the pose) must be set, bit 3 (the width) may be, no other", what, lm->free_mask);
  GSD_REQUIRE(lm->down > 0.0 && lm->down <= 1.0 && lm->up >= 1.0 && isfinite(lm->up) && lm->lambda_min >= 0.0 &&
                  lm->lambda_max >= lm->lambda_min && isfinite(lm->lambda_max),
              GSD_ERR_BAD_ARG, "%s: need 0 < down <= 1 <= up and 0 <= lambda_min <= lambda_max, all finite", what);
  for (int k = 0; k < 4; ++k)
    GSD_REQUIRE(lm->max_step[k] >= 0.0 && isfinite(lm->max_step[k]), GSD_ERR_BAD_ARG, "%s: max_step[%d] = %g must be finite and >= 0",
                what, k, lm->max_step[k]);
  GSD_REQUIRE((((uintptr_t)lambda | (uintptr_t)row | (uintptr_t)trial_row | (uintptr_t)trace | (uintptr_t)last_step) & 7) == 0,
              GSD_ERR_BAD_ARG, "%s: the fp64 arrays must be 8-byte aligned", what);
  MdLm p;
  p.down = lm->down, p.up = lm->up, p.lambda_min = lm->lambda_min, p.lambda_max = lm->lambda_max;
  for (int k = 0; k < 4; ++k) p.max_step[k] = lm->max_step[k];
  p.free_mask = lm->free_mask, p.first = lm->first != 0;
  hipLaunchKernelGGL(mesh_pose_lm_update, dim3((unsigned)ceil_div(B, 64)), dim3(64), 0, (hipStream_t)stream, p, B, pose, width, lambda,
                     row, trial_pose, trial_width, trial_row, trace, accepted, last_step);
  GSD_LAUNCH_CHECK(what);
  return GSD_OK;
}
