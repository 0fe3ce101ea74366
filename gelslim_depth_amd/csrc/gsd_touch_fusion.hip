// gsd_touch_fusion.hip -- touches fused into a surface: TSDF integration and marching tetrahedra (gfx950), include/gsd.h: gsd_touch_*.
// The definition is DESIGN.md section 24 and the header's comment; tests/touch_fusion_ref.py is its numpy twin, bit for bit.
//
//   touch_integrate: a gather.  One thread per voxel, a block owns a brick of 16 x 4 x 4 voxels: a wave is one z layer, its 16-voxel
//   rows are whole 64-byte lines of acc and weight.  The block walks the K touches in order; a touch's row (twelve doubles, width,
//   weight) is indexed by the loop counter alone, so it arrives by scalar loads.  Per touch the block first asks whether the brick's
//   box can reach the image at all (tf_reaches, a bound: it never changes a bit) and otherwise skips the touch without a vector
//   instruction.  A sample of both channels issues its eight pixel loads before any of them is used.  The state lives in two
//   registers from the first touch to the last: read once, stored once.  No scratch, no atomics, no division, no LDS.
//   Bricks are handed out in plain order, x fastest.  Handing every XCD a consecutive range of bricks (xcd_swizzle), so that an L2
//   sees a compact part of every image, was measured and lost 6 % on 64 touches into 256^3 voxels.
//
//   touch_extract_count / _scan / _write: a stream compaction with a fixed order (cell, tetrahedron, table order), without
//   atomics, as gsd_depth_points.  A block owns 256 consecutive cells, a thread counts its cell's triangles (0..12); one block
//   turns the block totals into exclusive offsets, 4096 per pass with a carry; the write launch recomputes the same device function
//   (te_cell), places its thread by __shfl_up plus LDS and stores.  A vertex reads its two voxels again rather than keeping eight
//   field values in an indexed array: no scratch.
#include "gsd_common.h"

#include <math.h>

namespace {

// ---- integration -----------------------------------------------------------------------------------------------------------
constexpr int TF_BX = 16, TF_BY = 4, TF_BZ = 4;      // voxels of a brick per axis: 256 threads
static_assert(TF_BX * TF_BY * TF_BZ == 256 && TF_BX * sizeof(float) == 64, "a brick row is one 64-byte line");

struct TfView {
  double x0, y0, z0, h, tau, inv_tau, inv_mpp, half_h, half_w, width_offset;
  double lim_u, lim_v;      // (H/2 + 1) mpp, (W/2 + 1) mpp: the image rectangle grown by one pixel, in mm about its centre
  float contact, carve;
  int nx, ny, nz, nbx, nby, nblocks, K, H, W, lr_flip, cull;
};

// Can any voxel of the box centre c, half extents e, be usable in touch row T?  usable needs 0 <= floor(rf), floor(kf) and
// floor(rf) <= H - 2, so |u| inv_mpp <= H/2 and |v| inv_mpp <= W/2 whichever finger.  Over the box |u - u(c)| <= sum |A0i| e_i.
// The last term covers the rounding of every product and sum here and in the voxel's own u (2^-45 of the magnitudes, where the
// arithmetic errs by 2^-50 of them at most).  A NaN or an infinity compares false: the touch is walked.
__device__ __forceinline__ bool tf_reaches(const double* __restrict__ T, double cx, double cy, double cz, double ex, double ey, double ez,
                                           double lim_u, double lim_v) {
#pragma clang fp contract(off)
  const double uc = ((T[0] * cx + T[1] * cy) + T[2] * cz) + T[3];
  const double vc = ((T[4] * cx + T[5] * cy) + T[6] * cz) + T[7];
  const double ru = (fabs(T[0]) * ex + fabs(T[1]) * ey) + fabs(T[2]) * ez;
  const double rv = (fabs(T[4]) * ex + fabs(T[5]) * ey) + fabs(T[6]) * ez;
  const double mu = (((fabs(T[0] * cx) + fabs(T[1] * cy)) + fabs(T[2] * cz)) + fabs(T[3])) + ru;
  const double mv = (((fabs(T[4] * cx) + fabs(T[5] * cy)) + fabs(T[6] * cz)) + fabs(T[7])) + rv;
  const double eps = 0x1p-45;
  const bool miss = (fabs(uc) - ru) - eps * mu > lim_u || (fabs(vc) - rv) - eps * mv > lim_v;
  return !miss;
}

// the quad of one (voxel, touch, channel): where it is, whether it is usable, its four pixels
struct TfQuad {
  double a;       // rf - r0
  bool usable;
  float d00, d01, d10, d11;
};
__device__ __forceinline__ TfQuad tf_quad(const TfView& V, const float* __restrict__ img, double su, double k0, bool k_ok) {
#pragma clang fp contract(off)
  TfQuad Q;
  const double rf = su * V.inv_mpp + V.half_h;
  const double r0 = floor(rf);
  Q.a = rf - r0;
  Q.usable = k_ok && r0 >= 0.0 && r0 <= (double)(V.H - 2);
  Q.d00 = Q.d01 = Q.d10 = Q.d11 = 0.f;
  if (Q.usable) {
    const float* row = img + (size_t)(int)r0 * V.W + (int)k0;
    Q.d00 = row[0], Q.d01 = row[1], Q.d10 = row[V.W], Q.d11 = row[V.W + 1];
  }
  return Q;
}
__device__ __forceinline__ void tf_update(const TfView& V, const TfQuad& Q, double b, double sq_less_half_g, float w, float wc, float& acc,
                                          float& weight) {
#pragma clang fp contract(off)
  const float lim = (float)INFINITY;
  const bool usable = Q.usable && fabsf(Q.d00) < lim && fabsf(Q.d01) < lim && fabsf(Q.d10) < lim && fabsf(Q.d11) < lim;
  const float thr = -V.contact;
  const bool contact = usable && Q.d00 < thr && Q.d01 < thr && Q.d10 < thr && Q.d11 < thr;
  const double d00 = (double)Q.d00, d01 = (double)Q.d01, d10 = (double)Q.d10, d11 = (double)Q.d11;
  const double top = d00 + b * (d01 - d00);
  const double bot = d10 + b * (d11 - d10);
  const double dbar = top + Q.a * (bot - top);
  const double phi = sq_less_half_g + dbar;
  if (contact) {
    if (phi >= -V.tau) {
      const double x = phi * V.inv_tau;
      const float sample = (float)(x < 1.0 ? x : 1.0);
      const float add = w * sample;
      acc = acc + add;
      weight = weight + w;
    }
  } else if (usable && phi > 0.0) {
    acc = acc + wc;
    weight = weight + wc;
  }
}

__global__ __launch_bounds__(256) void touch_integrate(const TfView V, const float* __restrict__ depth, const float* __restrict__ widths,
                                                       const double* __restrict__ transforms, const float* __restrict__ weights,
                                                       float* __restrict__ acc_out, float* __restrict__ weight_out) {
#pragma clang fp contract(off)
  const int bid = (int)blockIdx.x;
  const int bx = bid % V.nbx, by = (bid / V.nbx) % V.nby, bz = bid / (V.nbx * V.nby);
  const int tid = threadIdx.x;
  const int ix = bx * TF_BX + (tid & (TF_BX - 1)), iy = by * TF_BY + ((tid >> 4) & (TF_BY - 1)), iz = bz * TF_BZ + (tid >> 6);
  if (ix >= V.nx || iy >= V.ny || iz >= V.nz) return;      // no barrier below
  const size_t at = ((size_t)iz * V.ny + iy) * V.nx + ix;
  const double px = V.x0 + V.h * (double)ix, py = V.y0 + V.h * (double)iy, pz = V.z0 + V.h * (double)iz;
  // the brick's box: centre and half extents (block-uniform)
  const double ex = V.h * (0.5 * (TF_BX - 1)), ey = V.h * (0.5 * (TF_BY - 1)), ez = V.h * (0.5 * (TF_BZ - 1));
  const double cx = V.x0 + V.h * ((double)(bx * TF_BX) + 0.5 * (TF_BX - 1));
  const double cy = V.y0 + V.h * ((double)(by * TF_BY) + 0.5 * (TF_BY - 1));
  const double cz = V.z0 + V.h * ((double)(bz * TF_BZ) + 0.5 * (TF_BZ - 1));
  const double s0 = V.lr_flip ? 1.0 : -1.0;      // channel 0's finger
  float acc = acc_out[at], weight = weight_out[at];
  for (int k = 0; k < V.K; ++k) {
    const double* __restrict__ T = transforms + 12 * (size_t)k;
    const double g = (double)widths[k] + V.width_offset;
    if (!(g >= 0.0 && g < (double)INFINITY)) continue;
    if (V.cull && !tf_reaches(T, cx, cy, cz, ex, ey, ez, V.lim_u, V.lim_v)) continue;
    const float w = weights != nullptr ? weights[k] : 1.f;
    const float wc = w * V.carve;
    const double u = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
    const double v = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
    const double q = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
    const double half_g = 0.5 * g;
    const double kf = v * V.inv_mpp + V.half_w;
    const double k0 = floor(kf);
    const double b = kf - k0;
    const bool k_ok = k0 >= 0.0 && k0 <= (double)(V.W - 2);
    const float* img = depth + (size_t)(2 * k) * V.H * V.W;
    const TfQuad Q0 = tf_quad(V, img, s0 * u, k0, k_ok);
    const TfQuad Q1 = tf_quad(V, img + (size_t)V.H * V.W, -s0 * u, k0, k_ok);
    tf_update(V, Q0, b, s0 * q - half_g, w, wc, acc, weight);
    tf_update(V, Q1, b, -s0 * q - half_g, w, wc, acc, weight);
  }
  acc_out[at] = acc;
  weight_out[at] = weight;
}

// ---- extraction ------------------------------------------------------------------------------------------------------------
constexpr int TE_BLOCK = GSD_TOUCH_EXTRACT_BLOCK;      // cells per block, one per thread
constexpr int TE_SCAN_THREADS = 1024;                  // the scan's one block
constexpr int TE_SCAN_PASS = GSD_TOUCH_EXTRACT_SCAN_PASS;
constexpr int TE_SCAN_PER = 4;                         // block totals a scan thread takes per pass
static_assert(TE_SCAN_PASS == TE_SCAN_THREADS * TE_SCAN_PER && TE_BLOCK == 256, "blocks and passes");
constexpr int TE_HEAD = 4;                             // int32 words in front of the block offsets: the total (int64) and two spare

// Triangles of tetrahedron t (corners 0, e_p0, e_p0 + e_p1, 7 as cube corner ids, p the t-th permutation of the axes in
// lexicographic order) whose corner set `mask` is inside: six edges lo | hi << 4 of cube corners (c = dx + 2 dy + 4 dz, lo < hi in
// linear index), 0xff where there is no triangle.  Generated by tests/touch_fusion_ref.py (python tests/touch_fusion_ref.py).
__device__ const unsigned char TE_TABLE[6][16][6] = {
  {{0xff, 0xff, 0xff, 0xff, 0xff, 0xff}, {0x10, 0x30, 0x70, 0xff, 0xff, 0xff}, {0x10, 0x71, 0x31, 0xff, 0xff, 0xff}, {0x30, 0x70, 0x71, 0x30, 0x71, 0x31}, {0x30, 0x31, 0x73, 0xff, 0xff, 0xff}, {0x10, 0x73, 0x70, 0x10, 0x31, 0x73}, {0x10, 0x71, 0x73, 0x10, 0x73, 0x30}, {0x70, 0x71, 0x73, 0xff, 0xff, 0xff}, {0x70, 0x73, 0x71, 0xff, 0xff, 0xff}, {0x10, 0x30, 0x73, 0x10, 0x73, 0x71}, {0x10, 0x73, 0x31, 0x10, 0x70, 0x73}, {0x30, 0x73, 0x31, 0xff, 0xff, 0xff}, {0x30, 0x31, 0x71, 0x30, 0x71, 0x70}, {0x10, 0x31, 0x71, 0xff, 0xff, 0xff}, {0x10, 0x70, 0x30, 0xff, 0xff, 0xff}, {0xff, 0xff, 0xff, 0xff, 0xff, 0xff}},
  {{0xff, 0xff, 0xff, 0xff, 0xff, 0xff}, {0x10, 0x70, 0x50, 0xff, 0xff, 0xff}, {0x10, 0x51, 0x71, 0xff, 0xff, 0xff}, {0x50, 0x71, 0x70, 0x50, 0x51, 0x71}, {0x50, 0x75, 0x51, 0xff, 0xff, 0xff}, {0x10, 0x70, 0x75, 0x10, 0x75, 0x51}, {0x10, 0x75, 0x71, 0x10, 0x50, 0x75}, {0x70, 0x75, 0x71, 0xff, 0xff, 0xff}, {0x70, 0x71, 0x75, 0xff, 0xff, 0xff}, {0x10, 0x75, 0x50, 0x10, 0x71, 0x75}, {0x10, 0x51, 0x75, 0x10, 0x75, 0x70}, {0x50, 0x51, 0x75, 0xff, 0xff, 0xff}, {0x50, 0x71, 0x51, 0x50, 0x70, 0x71}, {0x10, 0x71, 0x51, 0xff, 0xff, 0xff}, {0x10, 0x50, 0x70, 0xff, 0xff, 0xff}, {0xff, 0xff, 0xff, 0xff, 0xff, 0xff}},
  {{0xff, 0xff, 0xff, 0xff, 0xff, 0xff}, {0x20, 0x70, 0x30, 0xff, 0xff, 0xff}, {0x20, 0x32, 0x72, 0xff, 0xff, 0xff}, {0x30, 0x72, 0x70, 0x30, 0x32, 0x72}, {0x30, 0x73, 0x32, 0xff, 0xff, 0xff}, {0x20, 0x70, 0x73, 0x20, 0x73, 0x32}, {0x20, 0x73, 0x72, 0x20, 0x30, 0x73}, {0x70, 0x73, 0x72, 0xff, 0xff, 0xff}, {0x70, 0x72, 0x73, 0xff, 0xff, 0xff}, {0x20, 0x73, 0x30, 0x20, 0x72, 0x73}, {0x20, 0x32, 0x73, 0x20, 0x73, 0x70}, {0x30, 0x32, 0x73, 0xff, 0xff, 0xff}, {0x30, 0x72, 0x32, 0x30, 0x70, 0x72}, {0x20, 0x72, 0x32, 0xff, 0xff, 0xff}, {0x20, 0x30, 0x70, 0xff, 0xff, 0xff}, {0xff, 0xff, 0xff, 0xff, 0xff, 0xff}},
  {{0xff, 0xff, 0xff, 0xff, 0xff, 0xff}, {0x20, 0x60, 0x70, 0xff, 0xff, 0xff}, {0x20, 0x72, 0x62, 0xff, 0xff, 0xff}, {0x60, 0x70, 0x72, 0x60, 0x72, 0x62}, {0x60, 0x62, 0x76, 0xff, 0xff, 0xff}, {0x20, 0x76, 0x70, 0x20, 0x62, 0x76}, {0x20, 0x72, 0x76, 0x20, 0x76, 0x60}, {0x70, 0x72, 0x76, 0xff, 0xff, 0xff}, {0x70, 0x76, 0x72, 0xff, 0xff, 0xff}, {0x20, 0x60, 0x76, 0x20, 0x76, 0x72}, {0x20, 0x76, 0x62, 0x20, 0x70, 0x76}, {0x60, 0x76, 0x62, 0xff, 0xff, 0xff}, {0x60, 0x62, 0x72, 0x60, 0x72, 0x70}, {0x20, 0x62, 0x72, 0xff, 0xff, 0xff}, {0x20, 0x70, 0x60, 0xff, 0xff, 0xff}, {0xff, 0xff, 0xff, 0xff, 0xff, 0xff}},
  {{0xff, 0xff, 0xff, 0xff, 0xff, 0xff}, {0x40, 0x50, 0x70, 0xff, 0xff, 0xff}, {0x40, 0x74, 0x54, 0xff, 0xff, 0xff}, {0x50, 0x70, 0x74, 0x50, 0x74, 0x54}, {0x50, 0x54, 0x75, 0xff, 0xff, 0xff}, {0x40, 0x75, 0x70, 0x40, 0x54, 0x75}, {0x40, 0x74, 0x75, 0x40, 0x75, 0x50}, {0x70, 0x74, 0x75, 0xff, 0xff, 0xff}, {0x70, 0x75, 0x74, 0xff, 0xff, 0xff}, {0x40, 0x50, 0x75, 0x40, 0x75, 0x74}, {0x40, 0x75, 0x54, 0x40, 0x70, 0x75}, {0x50, 0x75, 0x54, 0xff, 0xff, 0xff}, {0x50, 0x54, 0x74, 0x50, 0x74, 0x70}, {0x40, 0x54, 0x74, 0xff, 0xff, 0xff}, {0x40, 0x70, 0x50, 0xff, 0xff, 0xff}, {0xff, 0xff, 0xff, 0xff, 0xff, 0xff}},
  {{0xff, 0xff, 0xff, 0xff, 0xff, 0xff}, {0x40, 0x70, 0x60, 0xff, 0xff, 0xff}, {0x40, 0x64, 0x74, 0xff, 0xff, 0xff}, {0x60, 0x74, 0x70, 0x60, 0x64, 0x74}, {0x60, 0x76, 0x64, 0xff, 0xff, 0xff}, {0x40, 0x70, 0x76, 0x40, 0x76, 0x64}, {0x40, 0x76, 0x74, 0x40, 0x60, 0x76}, {0x70, 0x76, 0x74, 0xff, 0xff, 0xff}, {0x70, 0x74, 0x76, 0xff, 0xff, 0xff}, {0x40, 0x76, 0x60, 0x40, 0x74, 0x76}, {0x40, 0x64, 0x76, 0x40, 0x76, 0x70}, {0x60, 0x64, 0x76, 0xff, 0xff, 0xff}, {0x60, 0x74, 0x64, 0x60, 0x70, 0x74}, {0x40, 0x74, 0x64, 0xff, 0xff, 0xff}, {0x40, 0x60, 0x70, 0xff, 0xff, 0xff}, {0xff, 0xff, 0xff, 0xff, 0xff, 0xff}},
};

struct TeView {
  double x0, y0, z0, h;
  float min_weight;
  int nx, ny, nz, cx, cy, cells;      // cx, cy: cells per axis (nx - 1, ny - 1); cells: all of them, below 2^30
};

// the cell of a thread: where it is, and which of its eight corners are inside (-1: not valid, or beyond the last cell)
struct TeCell {
  int ix, iy, iz, corners;
};
__device__ __forceinline__ double te_field(const TeView& V, const float* __restrict__ acc, const float* __restrict__ weight, int ix, int iy,
                                           int iz, bool& observed) {
  const size_t at = ((size_t)iz * V.ny + iy) * V.nx + ix;
  const float w = weight[at];
  observed = w > V.min_weight;
  return (double)acc[at] / (double)w;
}
__device__ __forceinline__ TeCell te_cell(const TeView& V, const float* __restrict__ acc, const float* __restrict__ weight, int cell) {
  TeCell C;
  C.ix = C.iy = C.iz = 0, C.corners = -1;
  if (cell >= V.cells) return C;
  C.ix = cell % V.cx, C.iy = (cell / V.cx) % V.cy, C.iz = cell / (V.cx * V.cy);
  bool valid = true;
  int corners = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    bool observed;
    const double f = te_field(V, acc, weight, C.ix + (c & 1), C.iy + ((c >> 1) & 1), C.iz + (c >> 2), observed);
    valid = valid && observed;
    corners |= (f < 0.0 ? 1 : 0) << c;
  }
  C.corners = valid ? corners : -1;
  return C;
}
// the inside mask of tetrahedron t (a constant where the loop over t is unrolled)
__device__ __forceinline__ int te_mask(int corners, int t) {
  const int c1 = 1 << (t >> 1);                                               // e_p0: permutations 0, 1 start with x, 2, 3 with y, 4, 5 with z
  const int c2 = t == 0 || t == 2 ? 3 : t == 1 || t == 4 ? 5 : 6;              // e_p0 + e_p1
  return (corners & 1) | ((corners >> c1) & 1) << 1 | ((corners >> c2) & 1) << 2 | ((corners >> 7) & 1) << 3;
}
__device__ __forceinline__ int te_count(int corners) {
  if (corners < 0) return 0;
  int n = 0;
#pragma unroll
  for (int t = 0; t < 6; ++t) {
    const int pc = __popc(te_mask(corners, t));
    n += pc == 2 ? 2 : (pc == 1 || pc == 3) ? 1 : 0;
  }
  return n;
}

__global__ __launch_bounds__(TE_BLOCK) void touch_extract_count(const TeView V, const float* __restrict__ acc, const float* __restrict__ weight,
                                                                long long* __restrict__ block_count) {
  __shared__ int wave_n[TE_BLOCK / 64];
  const int cell = (int)blockIdx.x * TE_BLOCK + (int)threadIdx.x;      // below 2^30 + 256
  const int n = gsd_block_count<TE_BLOCK>(gsd_wave_sum(te_count(te_cell(V, acc, weight, cell).corners)), wave_n);
  if (threadIdx.x == 0) block_count[blockIdx.x] = n;
}

// One block: block totals -> exclusive offsets in place, pass by pass with a carry; then the total,
// to the head of the workspace and to the caller's scalar.
__global__ __launch_bounds__(TE_SCAN_THREADS) void touch_extract_scan(int nblocks, long long* block_off, long long* __restrict__ total_ws,
                                                                      long long* __restrict__ total) {
  const long long carry = gsd_block_exclusive_scan<long long, TE_SCAN_THREADS, TE_SCAN_PER>(
      nblocks, [&](int i) { return block_off[i]; }, [&](int i, long long run) { block_off[i] = run; });      // nblocks is below 2^22
  if (threadIdx.x == 0) *total_ws = carry, *total = carry;
}

// vertex on the edge between the cube corners lo < hi of cell C: section 24's arithmetic, fp64, one rounding at the store
__device__ __forceinline__ void te_vertex(const TeView& V, const float* __restrict__ acc, const float* __restrict__ weight, const TeCell& C,
                                          int edge, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int lo = edge & 15, hi = edge >> 4;
  const int lx = C.ix + (lo & 1), ly = C.iy + ((lo >> 1) & 1), lz = C.iz + (lo >> 2);
  const int hx = C.ix + (hi & 1), hy = C.iy + ((hi >> 1) & 1), hz = C.iz + (hi >> 2);
  bool observed;
  const double f_lo = te_field(V, acc, weight, lx, ly, lz, observed), f_hi = te_field(V, acc, weight, hx, hy, hz, observed);
  const double t = f_lo / (f_lo - f_hi);
  const double ax = V.x0 + V.h * (double)lx, ay = V.y0 + V.h * (double)ly, az = V.z0 + V.h * (double)lz;
  const double bx = V.x0 + V.h * (double)hx, by = V.y0 + V.h * (double)hy, bz = V.z0 + V.h * (double)hz;
  out[0] = (float)(ax + (bx - ax) * t);
  out[1] = (float)(ay + (by - ay) * t);
  out[2] = (float)(az + (bz - az) * t);
}

__global__ __launch_bounds__(TE_BLOCK) void touch_extract_write(const TeView V, const float* __restrict__ acc, const float* __restrict__ weight,
                                                                const long long* __restrict__ block_off, const long long* __restrict__ total_ws,
                                                                long long capacity, long long rows, int nblocks, float* __restrict__ triangles,
                                                                int* __restrict__ cell_out) {
  __shared__ int wave_n[TE_BLOCK / 64];
  const int cell = (int)blockIdx.x * TE_BLOCK + (int)threadIdx.x;
  const TeCell C = te_cell(V, acc, weight, cell);
  const int n = te_count(C.corners);
  const int inc = gsd_wave_inclusive_scan(n);
  const int before = gsd_block_waves_before<TE_BLOCK>(inc, wave_n);
  const long long limit = capacity > 0 && capacity < rows ? capacity : rows;      // rows a triangle may go to
  long long row = block_off[blockIdx.x] + before + (inc - n);
  if (n > 0) {
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      const unsigned char* e = TE_TABLE[t][te_mask(C.corners, t)];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (e[3 * j] == 0xff) continue;
        if (row >= 0 && row < limit) {
          float* out = triangles + 9 * row;
          te_vertex(V, acc, weight, C, e[3 * j], out);
          te_vertex(V, acc, weight, C, e[3 * j + 1], out + 3);
          te_vertex(V, acc, weight, C, e[3 * j + 2], out + 6);
          if (cell_out != nullptr) cell_out[row] = cell;
        }
        ++row;
      }
    }
  }
  if (capacity > 0) {
    // the rows that no triangle fills, shared out over all blocks
    const long long total = *total_ws;
    const long long step = (long long)nblocks * TE_BLOCK;
    for (long long m = (long long)blockIdx.x * TE_BLOCK + threadIdx.x; m < limit; m += step) {
      if (m < total) continue;
      const float nan = NAN;
#pragma unroll
      for (int i = 0; i < 9; ++i) triangles[9 * m + i] = nan;
      if (cell_out != nullptr) cell_out[m] = -1;
    }
  }
}

// ---- host layer ------------------------------------------------------------------------------------------------------------
int tf_check_volume(const gsd_touch_volume* v, const char* what) {
  GSD_REQUIRE(v != nullptr, GSD_ERR_BAD_ARG, "%s: null volume", what);
  GSD_REQUIRE(v->reserved == 0, GSD_ERR_BAD_ARG, "%s: the volume's reserved word must be 0", what);
  GSD_REQUIRE(v->nx >= 2 && v->nx <= 1024 && v->ny >= 2 && v->ny <= 1024 && v->nz >= 2 && v->nz <= 1024, GSD_ERR_BAD_ARG,
              "%s: %d x %d x %d voxels, every axis must have 2..1024", what, v->nx, v->ny, v->nz);
  GSD_REQUIRE(isfinite(v->voxel) && v->voxel > 0.0 && isfinite(v->truncation) && v->truncation > 0.0, GSD_ERR_BAD_ARG,
              "%s: voxel %g and truncation %g must be finite and positive", what, v->voxel, v->truncation);
  GSD_REQUIRE(isfinite(v->x0) && isfinite(v->y0) && isfinite(v->z0), GSD_ERR_BAD_ARG, "%s: the origin must be finite", what);
  return 0;
}
int te_nblocks(const gsd_touch_volume* v) {
  const int64_t cells = (int64_t)(v->nx - 1) * (v->ny - 1) * (v->nz - 1);      // below 2^30
  return (int)ceil_div64(cells, TE_BLOCK);
}
TeView te_view(const gsd_touch_volume* v, double min_weight) {
  TeView V;
  V.x0 = v->x0, V.y0 = v->y0, V.z0 = v->z0, V.h = v->voxel, V.min_weight = (float)min_weight;
  V.nx = v->nx, V.ny = v->ny, V.nz = v->nz, V.cx = v->nx - 1, V.cy = v->ny - 1, V.cells = V.cx * V.cy * (v->nz - 1);
  return V;
}
// what both launching extraction entry points refuse, before any launch
int te_check(const gsd_touch_volume* v, const float* acc, const float* weight, double min_weight, const int32_t* workspace,
             int64_t workspace_elems, const char* what) {
  if (const int rc = tf_check_volume(v, what)) return rc;
  GSD_REQUIRE(acc && weight && workspace, GSD_ERR_BAD_ARG, "%s: null pointer", what);
  GSD_REQUIRE(isfinite(min_weight) && min_weight >= 0.0, GSD_ERR_BAD_ARG, "%s: min_weight %g must be finite and >= 0", what, min_weight);
  GSD_REQUIRE(((uintptr_t)workspace & 7) == 0, GSD_ERR_BAD_ARG, "%s: workspace must be 8-byte aligned", what);
  const int64_t need = TE_HEAD + 2 * (int64_t)te_nblocks(v);
  GSD_REQUIRE(workspace_elems >= need, GSD_ERR_WORKSPACE, "%s: workspace of %lld int32 words, need %lld", what, (long long)workspace_elems,
              (long long)need);
  return 0;
}

}  // namespace

extern "C" {

int gsd_touch_integrate(const gsd_touch_volume* volume, const gsd_touch_view* view, const float* depth, const float* widths,
                        const double* transforms, const float* weights, int K, int H, int W, float* acc, float* weight, void* stream) {
  const char* what = "gsd_touch_integrate";
  if (const int rc = tf_check_volume(volume, what)) return rc;
  GSD_REQUIRE(view && depth && widths && transforms && acc && weight, GSD_ERR_BAD_ARG, "%s: null pointer", what);
  GSD_REQUIRE(K >= 1 && H >= 2 && W >= 2 && 2 * (int64_t)K * H * W < ((int64_t)1 << 31), GSD_ERR_BAD_ARG,
              "%s: bad dims K=%d H=%d W=%d (K at least 1, H and W at least 2, 2 K H W below 2^31)", what, K, H, W);
  const gsd_touch_view& v = *view;
  GSD_REQUIRE(v.reserved[0] == 0 && v.reserved[1] == 0, GSD_ERR_BAD_ARG, "%s: the view's reserved words must be 0", what);
  GSD_REQUIRE(isfinite(v.image_height_mm) && v.image_height_mm > 0.0 && isfinite(v.width_offset), GSD_ERR_BAD_ARG,
              "%s: image height %g must be finite and positive, the width offset %g finite", what, v.image_height_mm, v.width_offset);
  GSD_REQUIRE(isfinite(v.contact_depth) && v.contact_depth >= 0.0 && isfinite(v.carve_weight) && v.carve_weight >= 0.0, GSD_ERR_BAD_ARG,
              "%s: contact_depth %g and carve_weight %g must be finite and >= 0", what, v.contact_depth, v.carve_weight);
  GSD_REQUIRE(((uintptr_t)transforms & 7) == 0, GSD_ERR_BAD_ARG, "%s: transforms must be 8-byte aligned", what);
  const double mpp = v.image_height_mm / (double)H;
  TfView V;
  V.x0 = volume->x0, V.y0 = volume->y0, V.z0 = volume->z0, V.h = volume->voxel;
  V.tau = volume->truncation, V.inv_tau = 1.0 / volume->truncation, V.inv_mpp = 1.0 / mpp;
  GSD_REQUIRE(mpp > 0.0 && isfinite(V.inv_mpp) && isfinite(V.inv_tau), GSD_ERR_BAD_ARG, "%s: image height %g over %d rows, or the truncation %g, has no finite reciprocal",
              what, v.image_height_mm, H, volume->truncation);
  V.half_h = 0.5 * (double)H, V.half_w = 0.5 * (double)W, V.width_offset = v.width_offset;
  V.lim_u = (V.half_h + 1.0) * mpp, V.lim_v = (V.half_w + 1.0) * mpp;
  V.contact = (float)v.contact_depth, V.carve = (float)v.carve_weight;
  V.nx = volume->nx, V.ny = volume->ny, V.nz = volume->nz;
  V.nbx = ceil_div(V.nx, TF_BX), V.nby = ceil_div(V.ny, TF_BY);
  V.nblocks = V.nbx * V.nby * ceil_div(V.nz, TF_BZ);      // at most 64 * 256 * 256
  V.K = K, V.H = H, V.W = W, V.lr_flip = v.lr_flip != 0, V.cull = v.cull != 0;
  hipLaunchKernelGGL(touch_integrate, dim3((unsigned)V.nblocks), dim3(256), 0, (hipStream_t)stream, V, depth, widths, transforms, weights, acc,
                     weight);
  GSD_LAUNCH_CHECK(what);
  return GSD_OK;
}

int64_t gsd_touch_extract_workspace(const gsd_touch_volume* volume) {
  if (volume == nullptr || volume->nx < 2 || volume->nx > 1024 || volume->ny < 2 || volume->ny > 1024 || volume->nz < 2 || volume->nz > 1024)
    return 0;
  return TE_HEAD + 2 * (int64_t)te_nblocks(volume);
}

int gsd_touch_extract_count(const gsd_touch_volume* volume, const float* acc, const float* weight, double min_weight, int64_t* total,
                            int32_t* workspace, int64_t workspace_elems, void* stream) {
  const char* what = "gsd_touch_extract_count";
  if (const int rc = te_check(volume, acc, weight, min_weight, workspace, workspace_elems, what)) return rc;
  GSD_REQUIRE(total != nullptr && ((uintptr_t)total & 7) == 0, GSD_ERR_BAD_ARG, "%s: total must be an 8-byte aligned pointer", what);
  const TeView V = te_view(volume, min_weight);
  const int nblocks = te_nblocks(volume);
  long long* block_off = reinterpret_cast<long long*>(workspace + TE_HEAD);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(touch_extract_count, dim3((unsigned)nblocks), dim3(TE_BLOCK), 0, st, V, acc, weight, block_off);
  GSD_LAUNCH_CHECK(what);
  hipLaunchKernelGGL(touch_extract_scan, dim3(1), dim3(TE_SCAN_THREADS), 0, st, nblocks, block_off, reinterpret_cast<long long*>(workspace),
                     reinterpret_cast<long long*>(total));
  GSD_LAUNCH_CHECK(what);
  return GSD_OK;
}

int gsd_touch_extract_write(const gsd_touch_volume* volume, const float* acc, const float* weight, double min_weight, int64_t capacity,
                            int64_t rows, float* triangles, int32_t* cell, int32_t* workspace, int64_t workspace_elems, void* stream) {
  const char* what = "gsd_touch_extract_write";
  if (const int rc = te_check(volume, acc, weight, min_weight, workspace, workspace_elems, what)) return rc;
  GSD_REQUIRE(triangles != nullptr, GSD_ERR_BAD_ARG, "%s: null triangles", what);
  GSD_REQUIRE(capacity >= 0 && rows >= 0 && rows <= INT32_MAX && rows >= capacity, GSD_ERR_BAD_ARG,
              "%s: capacity %lld and outputs of %lld rows: both >= 0, rows at least the capacity and below 2^31", what, (long long)capacity,
              (long long)rows);
  if (rows == 0) return GSD_OK;
  const TeView V = te_view(volume, min_weight);
  const int nblocks = te_nblocks(volume);
  hipLaunchKernelGGL(touch_extract_write, dim3((unsigned)nblocks), dim3(TE_BLOCK), 0, (hipStream_t)stream, V, acc, weight,
                     reinterpret_cast<const long long*>(workspace + TE_HEAD), reinterpret_cast<const long long*>(workspace), (long long)capacity,
                     (long long)rows, nblocks, triangles, cell);
  GSD_LAUNCH_CHECK(what);
  return GSD_OK;
}

}  // extern "C"
