// gsd_depth_points.hip -- contact point clouds and normals from depth images (gfx950), include/gsd.h: gsd_depth_points_*.
// The definition is DESIGN.md section 21: the inverse of section 16's pixel -> mesh map.  In short, a pixel (r, k) of the
// lattice r = stride/2 + i stride, k = stride/2 + j stride whose depth d is below -contact_depth (fp32) is a point
//   sensor frame:  (mpp (r - H/2), mpp (k - W/2), d),                 normal (d_x, d_y, -1)
//   grasp frame:   (s x, y, s (g/2 - d)),  s = +1 right, -1 left,     normal (s d_x, d_y, s)
//   object frame:  the mesh file's coordinates times pc_scale: the in-plane pair through the inverse of the pose, the
//                  perpendicular coordinate q / multiplier + mid
// d_x, d_y differences between immediate CONTACT neighbours of the full image (central, one-sided or 0), every normal of unit
// length, everything after the fp32 loads in fp64 with one rounding at the store.
//
// A stream compaction with a fixed order (image, channel as stored, r, k), without atomics:
//
//   depth_points_count: a block of DP_THREADS threads owns DP_BLOCK consecutive lattice points of one (image, channel) -- the
//   blocks per (image, channel) depend on H, W and stride alone.  Thread t takes the points j DP_THREADS + t, j = 0..3, all four
//   loads in flight at once; a wave counts its points by __ballot / __popcll, the block stores one int.
//
//   depth_points_scan: one block turns the block counts into exclusive offsets, in place, DP_SCAN_PASS counts per pass with
//   a carry from pass to pass, so any number of blocks is served; it leaves the total as an int64 and the B x 2 true counts.
//
//   depth_points_write: the same decode and the same predicate (dp_point); a lane's row is its block's offset + the
//   counts of the (round, wave) slots in front of its own in point order + __popcll(mask & lanes below).  Packed: that row.  Padded (capacity M per
//   image): row b M + (row - the image's first row) while that is below M, the rest dropped; the image's blocks then fill the
//   rows from min(n_b, M) to M - 1 with NaN (pixel: -1).  Every store is guarded by the row count the caller passed.
//
// cos and sin of the poses come from a table (depth_points_table, one thread per image) so that the point kernel runs no
// transcendental function.  Axis indices are resolved with selects, not with an indexed array: the kernels use no scratch.
#include "gsd_common.h"

#include <math.h>

#include <algorithm>

namespace {

constexpr int DP_BLOCK = GSD_DEPTH_POINTS_BLOCK;       // lattice points per block of the count and write launches
constexpr int DP_THREADS = 256;                       // its threads: thread t takes the points j * DP_THREADS + t, one per round j
constexpr int DP_ROUNDS = DP_BLOCK / DP_THREADS;
constexpr int DP_SLOTS = DP_BLOCK / 64;               // (round, wave) pairs of a block; slot j * 4 + wave holds 64 consecutive points
constexpr int DP_SCAN_THREADS = 1024;                 // the scan's one block
constexpr int DP_SCAN_PASS = GSD_DEPTH_POINTS_SCAN_PASS;  // block counts per pass of the scan
constexpr int DP_SCAN_PER = 4;                        // block counts a scan thread takes per pass
static_assert(DP_SCAN_PASS == DP_SCAN_THREADS * DP_SCAN_PER && DP_BLOCK == DP_THREADS * DP_ROUNDS, "blocks and passes");
constexpr int DP_TABLE = 4;                           // doubles per image of the pose table: cos, sin, 1000 t1, 1000 t2
constexpr int DP_HEAD = 4;                            // int32 words in front of the table: the total (int64) and two spare

struct DpView {
  double mpp, width_offset, mid, mult;
  float contact;
  int H, W, stride, off, cols, points, nblk;      // points: lattice points per (image, channel); nblk: blocks per (image, channel)
  int frame, lr_flip, swap_axes, invert, perp;
};

// g = widths[b] + width_offset in fp64; NaN marks a refused one (negative or not finite): that image has no points
__device__ __forceinline__ double dp_width(const DpView& V, const float* __restrict__ widths, int b) {
  if (V.frame == 0) return 0.0;
  const double g = (double)widths[b] + V.width_offset;
  return (g >= 0.0 && g < (double)INFINITY) ? g : (double)NAN;
}

// What a thread of the count and write launches works on in round j: lattice point p of (image, channel) img = blockIdx.x / nblk.
struct DpPoint {
  int img, r, k;
  bool is;        // the pixel is a point
  float d;
};
__device__ __forceinline__ DpPoint dp_point(const DpView& V, const float* __restrict__ depth, const float* __restrict__ widths, int j) {
  DpPoint P;
  P.img = blockIdx.x / V.nblk;
  const int p = (blockIdx.x % V.nblk) * DP_BLOCK + j * DP_THREADS + threadIdx.x;
  const int i = p / V.cols;
  P.r = V.off + i * V.stride, P.k = V.off + (p - i * V.cols) * V.stride;
  P.is = false, P.d = 0.f;
  const double g = dp_width(V, widths, P.img >> 1);
  if (p < V.points && g == g) {
    P.d = depth[((size_t)P.img * V.H + P.r) * V.W + P.k];
    P.is = P.d < -V.contact;        // false for a NaN
  }
  return P;
}

// the block's point count: all loads first, then every wave's count by ballot, the sum by thread 0
__global__ __launch_bounds__(DP_THREADS) void depth_points_count(const DpView V, const float* __restrict__ depth,
                                                                 const float* __restrict__ widths, int* __restrict__ block_count) {
  __shared__ int wave_n[DP_THREADS / 64];
  bool is[DP_ROUNDS];
#pragma unroll
  for (int j = 0; j < DP_ROUNDS; ++j) is[j] = dp_point(V, depth, widths, j).is;
  int n = 0;
#pragma unroll
  for (int j = 0; j < DP_ROUNDS; ++j) n += __popcll(__ballot(is[j]));
  n = gsd_block_count<DP_THREADS>(n, wave_n);
  if (threadIdx.x == 0) block_count[blockIdx.x] = n;
}

// One block: block counts -> exclusive offsets in place, pass by pass with a carry; then the total and the count of every
// (image, channel), to the caller's `counts` and to the workspace copy that the write reads.
__global__ __launch_bounds__(DP_SCAN_THREADS) void depth_points_scan(int nblocks, int nblk, int images, int* block_off, int* __restrict__ counts,
                                                              int* __restrict__ counts_ws, long long* __restrict__ total) {
  const int tid = threadIdx.x;
  const int carry = gsd_block_exclusive_scan<int, DP_SCAN_THREADS, DP_SCAN_PER>(      // below 2^31: there are fewer lattice points than that
      nblocks, [&](int i) { return block_off[i]; }, [&](int i, int run) { block_off[i] = run; });
  if (tid == 0) *total = carry;
  for (int img = tid; img < images; img += DP_SCAN_THREADS) {
    const int n = (img + 1 < images ? block_off[(size_t)(img + 1) * nblk] : carry) - block_off[(size_t)img * nblk];
    counts[img] = n;
    counts_ws[img] = n;
  }
}

// row b of the pose table: cos, sin from the double-precision functions, 1000 t in fp64
__global__ __launch_bounds__(256) void depth_points_table(const float* __restrict__ poses, int B, double* __restrict__ table) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const double th = (double)poses[3 * (size_t)b + 2];
  double* row = table + (size_t)b * DP_TABLE;
  row[0] = cos(th);
  row[1] = sin(th);
  row[2] = 1000.0 * (double)poses[3 * (size_t)b];
  row[3] = 1000.0 * (double)poses[3 * (size_t)b + 1];
}

// component `axis` of the vector that has a at the lower in-plane axis, b at the higher one and c at `perp`
__device__ __forceinline__ double dp_axis(int axis, int perp, double a, double b, double c) {
  const int lo = perp == 0 ? 1 : 0;
  return axis == perp ? c : axis == lo ? a : b;
}

// one difference of the gradient: the neighbours below (m) and above (p) along an axis, usable iff inside and contact
__device__ __forceinline__ double dp_diff(float d, bool has_m, float dm, bool has_p, float dp, float thr, double mpp) {
#pragma clang fp contract(off)
  const bool um = has_m && dm < thr, up = has_p && dp < thr;
  if (um && up) return ((double)dp - (double)dm) / (2.0 * mpp);
  if (up) return ((double)dp - (double)d) / mpp;
  if (um) return ((double)d - (double)dm) / mpp;
  return 0.0;
}

// point P of the cloud into row `row` of the outputs: section 21's arithmetic, fp64, one rounding at the store
__device__ __forceinline__ void dp_emit(const DpView& V, const DpPoint& P, long long row, const float* __restrict__ depth,
                                        const float* __restrict__ widths, const double* __restrict__ table, float* __restrict__ points,
                                        float* __restrict__ normals, int* __restrict__ pixel) {
#pragma clang fp contract(off)
  const int r = P.r, k = P.k;
  const size_t at = ((size_t)P.img * V.H + r) * V.W + k;
  const float d = P.d, thr = -V.contact;
  const double x = V.mpp * ((double)r - 0.5 * (double)V.H), y = V.mpp * ((double)k - 0.5 * (double)V.W);
  double dx = 0.0, dy = 0.0;
  if (normals != nullptr) {
    const bool has_u = r > 0, has_d = r + 1 < V.H, has_l = k > 0, has_r = k + 1 < V.W;
    const float du = has_u ? depth[at - V.W] : 0.f, dd = has_d ? depth[at + V.W] : 0.f;
    const float dl = has_l ? depth[at - 1] : 0.f, dr = has_r ? depth[at + 1] : 0.f;
    dx = dp_diff(d, has_u, du, has_d, dd, thr, V.mpp);
    dy = dp_diff(d, has_l, dl, has_r, dr, thr, V.mpp);
  }
  const int b = P.img >> 1, ch = P.img & 1;
  const double norm = sqrt(dx * dx + dy * dy + 1.0);
  double p0, p1, p2, n0, n1, n2;
  if (V.frame == 0) {
    p0 = x, p1 = y, p2 = (double)d;
    n0 = dx, n1 = dy, n2 = -1.0;
  } else {
    const bool right = (ch == 1) != (V.lr_flip != 0);
    const double s = right ? 1.0 : -1.0;
    const double g = dp_width(V, widths, b);
    const double u = s * x, v = y, q = s * (0.5 * g - (double)d);
    const double nu = s * dx, nv = dy, nq = s;
    if (V.frame == 1) {
      p0 = u, p1 = v, p2 = q;
      n0 = nu, n1 = nv, n2 = nq;
    } else {
      const double* tr = table + (size_t)b * DP_TABLE;
      const double cs = tr[0], sn = tr[1], a1 = tr[2], a2 = tr[3];
      const double ta = V.swap_axes ? v : u, tb = V.swap_axes ? u : v;      // ascending axis order
      const double na = V.swap_axes ? nv : nu, nb = V.swap_axes ? nu : nv;
      double pa, pb, ma, mb;
      if (V.invert) {       // the forward map used M^-1: back through M
        pa = cs * ta - sn * tb + a1, pb = sn * ta + cs * tb + a2;
        ma = cs * na - sn * nb, mb = sn * na + cs * nb;
      } else {              // back through M^-1 = R^T (. - t)
        const double da = ta - a1, db = tb - a2;
        pa = cs * da + sn * db, pb = cs * db - sn * da;
        ma = cs * na + sn * nb, mb = cs * nb - sn * na;
      }
      const double pc = q / V.mult + V.mid, mc = nq / V.mult;
      p0 = dp_axis(0, V.perp, pa, pb, pc), p1 = dp_axis(1, V.perp, pa, pb, pc), p2 = dp_axis(2, V.perp, pa, pb, pc);
      n0 = dp_axis(0, V.perp, ma, mb, mc), n1 = dp_axis(1, V.perp, ma, mb, mc), n2 = dp_axis(2, V.perp, ma, mb, mc);
    }
  }
  points[3 * row] = (float)p0, points[3 * row + 1] = (float)p1, points[3 * row + 2] = (float)p2;
  if (normals != nullptr) normals[3 * row] = (float)(n0 / norm), normals[3 * row + 1] = (float)(n1 / norm), normals[3 * row + 2] = (float)(n2 / norm);
  if (pixel != nullptr) pixel[row] = (int)at;
}

__global__ __launch_bounds__(DP_THREADS) void depth_points_write(const DpView V, const float* __restrict__ depth,
                                                                 const float* __restrict__ widths, const double* __restrict__ table,
                                                                 const int* __restrict__ block_off, const int* __restrict__ counts_ws,
                                                                 int capacity, long long rows, float* __restrict__ points,
                                                                 float* __restrict__ normals, int* __restrict__ pixel) {
  __shared__ int slot_n[DP_SLOTS];
  DpPoint P[DP_ROUNDS];
  unsigned long long mask[DP_ROUNDS];
  int rank[DP_ROUNDS];      // the points in front of this one in its block, in point order
#pragma unroll
  for (int j = 0; j < DP_ROUNDS; ++j) P[j] = dp_point(V, depth, widths, j);
#pragma unroll
  for (int j = 0; j < DP_ROUNDS; ++j) mask[j] = __ballot(P[j].is);
  gsd_block_rank<DP_THREADS, DP_ROUNDS>(mask, slot_n, rank);
  const int b = blockIdx.x / (2 * V.nblk);
  const long long first = capacity > 0 ? block_off[(size_t)(2 * b) * V.nblk] : 0;      // the image's first point
  const long long base = block_off[blockIdx.x];      // the row of the block's first point
#pragma unroll
  for (int j = 0; j < DP_ROUNDS; ++j) {
    long long row = base + rank[j];
    bool keep = P[j].is;
    if (capacity > 0) {
      keep = keep && row - first < capacity;
      row = (long long)b * capacity + (row - first);
    }
    if (keep && row >= 0 && row < rows) dp_emit(V, P[j], row, depth, widths, table, points, normals, pixel);
  }
  if (capacity > 0) {
    // the rows of this image that no point fills, shared out over the image's 2 nblk blocks
    const long long n_b = (long long)counts_ws[2 * b] + counts_ws[2 * b + 1];
    const long long step = 2ll * V.nblk * DP_THREADS;
    for (long long m = (long long)(blockIdx.x % (2 * V.nblk)) * DP_THREADS + threadIdx.x; m < capacity; m += step) {
      const long long at = (long long)b * capacity + m;
      if (m < n_b || at >= rows) continue;
      const float nan = NAN;
      points[3 * at] = nan, points[3 * at + 1] = nan, points[3 * at + 2] = nan;
      if (normals != nullptr) normals[3 * at] = nan, normals[3 * at + 1] = nan, normals[3 * at + 2] = nan;
      if (pixel != nullptr) pixel[at] = -1;
    }
  }
}

// ---- host layer ------------------------------------------------------------------------------------------------------------
int dp_lattice_len(int len, int stride) {
  const int off = stride / 2;
  return off < len ? (len - 1 - off) / stride + 1 : 0;
}
// blocks per (image, channel), or -1 for dims the calls refuse
int64_t dp_nblk(int B, int H, int W, int stride) {
  if (B < 1 || H < 1 || W < 1 || stride < 1 || 2 * (int64_t)B * H * W >= ((int64_t)1 << 31)) return -1;
  // at least one, so that an image whose lattice is empty still has blocks to fill its padded rows
  const int64_t n = std::max<int64_t>(1, ceil_div64((int64_t)dp_lattice_len(H, stride) * dp_lattice_len(W, stride), DP_BLOCK));
  return 2 * (int64_t)B * n > INT32_MAX - DP_SCAN_PASS ? -1 : n;      // the scan indexes the blocks with an int
}
struct DpLayout {      // the workspace, in int32 words: total (int64), two spare, the pose table, the counts, the block offsets
  int64_t table, counts, blocks, words;
  int nblk, nblocks;
};
DpLayout dp_layout(int B, int H, int W, int stride) {
  DpLayout Y;
  Y.nblk = (int)dp_nblk(B, H, W, stride), Y.nblocks = 2 * B * Y.nblk;      // below 2 B H W / DP_BLOCK + 2 B
  Y.table = DP_HEAD, Y.counts = Y.table + 2 * (int64_t)DP_TABLE * B, Y.blocks = Y.counts + 2 * (int64_t)B;
  Y.words = (Y.blocks + Y.nblocks + 1) / 2 * 2;
  return Y;
}

struct DpCall {
  const gsd_depth_points_view* view;
  const float* depth;
  const float* widths;
  int B, H, W, stride;
  const int32_t* workspace;
  int64_t workspace_elems;
};
// what both launching entry points refuse, before any launch
int dp_check(const DpCall& Q, const char* what) {
  GSD_REQUIRE(Q.view && Q.depth && Q.workspace, GSD_ERR_BAD_ARG, "%s: null pointer", what);
  GSD_REQUIRE(dp_nblk(Q.B, Q.H, Q.W, Q.stride) >= 0, GSD_ERR_BAD_ARG,
              "%s: bad dims B=%d H=%d W=%d stride=%d (each at least 1, 2 B H W and the block count below 2^31)", what, Q.B, Q.H, Q.W, Q.stride);
  const gsd_depth_points_view& v = *Q.view;
  GSD_REQUIRE(v.reserved[0] == 0 && v.reserved[1] == 0, GSD_ERR_BAD_ARG, "%s: the reserved words must be 0", what);
  GSD_REQUIRE(v.frame >= 0 && v.frame <= 2, GSD_ERR_BAD_ARG, "%s: frame %d, 0 sensor, 1 grasp, 2 object", what, v.frame);
  GSD_REQUIRE(isfinite(v.mpp) && v.mpp > 0.0 && isfinite(v.width_offset) && isfinite(v.mid), GSD_ERR_BAD_ARG,
              "%s: mm per pixel %g must be finite and positive, the width offset %g and mid %g finite", what, v.mpp, v.width_offset, v.mid);
  GSD_REQUIRE(isfinite(v.contact_depth) && v.contact_depth >= 0.0, GSD_ERR_BAD_ARG, "%s: contact_depth %g must be finite and >= 0", what,
              v.contact_depth);
  GSD_REQUIRE(v.perp_ind >= 0 && v.perp_ind <= 2 && (v.multiplier == 1 || v.multiplier == -1), GSD_ERR_BAD_ARG,
              "%s: perp_ind %d must be 0..2 and multiplier %d +1 or -1", what, v.perp_ind, v.multiplier);
  GSD_REQUIRE((v.swap_axes | v.invert_affine | v.lr_flip) >> 1 == 0, GSD_ERR_BAD_ARG,
              "%s: swap_axes, invert_affine and lr_flip must be 0 or 1", what);
  GSD_REQUIRE(v.frame == 0 || Q.widths != nullptr, GSD_ERR_BAD_ARG, "%s: the grasp and object frames need widths", what);
  GSD_REQUIRE(((uintptr_t)Q.workspace & 7) == 0, GSD_ERR_BAD_ARG, "%s: workspace must be 8-byte aligned", what);
  const int64_t need = dp_layout(Q.B, Q.H, Q.W, Q.stride).words;
  GSD_REQUIRE(Q.workspace_elems >= need, GSD_ERR_WORKSPACE, "%s: workspace of %lld int32 words, need %lld", what,
              (long long)Q.workspace_elems, (long long)need);
  return 0;
}
DpView dp_view(const DpCall& Q, const DpLayout& Y) {
  const gsd_depth_points_view& v = *Q.view;
  DpView V;
  V.mpp = v.mpp, V.width_offset = v.width_offset, V.mid = v.mid, V.mult = (double)v.multiplier, V.contact = (float)v.contact_depth;
  V.H = Q.H, V.W = Q.W, V.stride = Q.stride, V.off = Q.stride / 2;
  const int cols = dp_lattice_len(Q.W, Q.stride);
  V.cols = std::max(cols, 1), V.points = dp_lattice_len(Q.H, Q.stride) * cols, V.nblk = Y.nblk;      // cols divides: never 0
  V.frame = v.frame, V.lr_flip = v.lr_flip, V.swap_axes = v.swap_axes, V.invert = v.invert_affine, V.perp = v.perp_ind;
  return V;
}

}  // namespace

extern "C" {

int64_t gsd_depth_points_workspace(int B, int H, int W, int stride) {
  return dp_nblk(B, H, W, stride) < 0 ? 0 : dp_layout(B, H, W, stride).words;
}

int gsd_depth_points_count(const gsd_depth_points_view* view, const float* depth, const float* widths, int B, int H, int W, int stride,
                           int32_t* counts, int32_t* workspace, int64_t workspace_elems, void* stream) {
  const char* what = "gsd_depth_points_count";
  const DpCall Q{view, depth, widths, B, H, W, stride, workspace, workspace_elems};
  if (const int rc = dp_check(Q, what)) return rc;
  GSD_REQUIRE(counts != nullptr, GSD_ERR_BAD_ARG, "%s: null counts", what);
  const DpLayout Y = dp_layout(B, H, W, stride);
  const DpView V = dp_view(Q, Y);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(depth_points_count, dim3((unsigned)Y.nblocks), dim3(DP_THREADS), 0, st, V, depth, widths, workspace + Y.blocks);
  GSD_LAUNCH_CHECK(what);
  hipLaunchKernelGGL(depth_points_scan, dim3(1), dim3(DP_SCAN_THREADS), 0, st, Y.nblocks, Y.nblk, 2 * B, workspace + Y.blocks, counts,
                     workspace + Y.counts, reinterpret_cast<long long*>(workspace));
  GSD_LAUNCH_CHECK(what);
  return GSD_OK;
}

int gsd_depth_points_write(const gsd_depth_points_view* view, const float* depth, const float* widths, const float* poses, int B, int H,
                           int W, int stride, int capacity, int64_t rows, float* points, float* normals, int32_t* pixel,
                           int32_t* workspace, int64_t workspace_elems, void* stream) {
  const char* what = "gsd_depth_points_write";
  const DpCall Q{view, depth, widths, B, H, W, stride, workspace, workspace_elems};
  if (const int rc = dp_check(Q, what)) return rc;
  GSD_REQUIRE(points != nullptr, GSD_ERR_BAD_ARG, "%s: null points", what);
  GSD_REQUIRE(view->frame != 2 || poses != nullptr, GSD_ERR_BAD_ARG, "%s: the object frame needs poses", what);
  GSD_REQUIRE(capacity >= 0 && rows >= 0 && rows <= INT32_MAX && rows >= (int64_t)B * capacity, GSD_ERR_BAD_ARG,
              "%s: capacity %d per image and outputs of %lld rows: both >= 0, rows at least B x capacity and below 2^31", what, capacity,
              (long long)rows);
  const DpLayout Y = dp_layout(B, H, W, stride);
  const DpView V = dp_view(Q, Y);
  hipStream_t st = (hipStream_t)stream;
  // the table sits between the head and the counts; the write leaves the rest of the workspace as the count made it
  double* table = reinterpret_cast<double*>(workspace + Y.table);
  if (view->frame == 2) {
    hipLaunchKernelGGL(depth_points_table, dim3((unsigned)ceil_div(B, 256)), dim3(256), 0, st, poses, B, table);
    GSD_LAUNCH_CHECK(what);
  }
  if (rows > 0) {
    hipLaunchKernelGGL(depth_points_write, dim3((unsigned)Y.nblocks), dim3(DP_THREADS), 0, st, V, depth, widths, (const double*)table,
                       workspace + Y.blocks, workspace + Y.counts, capacity, (long long)rows, points, normals, pixel);
    GSD_LAUNCH_CHECK(what);
  }
  return GSD_OK;
}

}  // extern "C"
