// gsd_contact_patches.hip -- connected contact patches of depth images (gfx950), include/gsd.h: gsd_contact_patches_*.
// The definition is DESIGN.md section 22.  In short: a pixel is contact iff d < -contact_depth (fp32, gsd_depth_points' rule); a
// patch is a maximal 4- or 8-connected set of contact pixels of one (image, channel) plane; patches of at least min_area pixels
// are numbered 1, 2, ... per plane in raster order of their first pixel; every statistic is an integer.
//
// Labelling is a union-find over ROW RUNS.  A wave owns one segment of CP_SEG = 64 consecutive columns of one row (lane =
// column): one __ballot gives the segment's contact mask, and every maximal run of set bits in it is one node, named by the
// linear index g = (plane H + r) W + k of its first pixel.  The parent image is the `labels` output itself.
//
//   patches_init:    parent[g] = the first pixel of g's run (background: -1); area[g] = 0.
//   patches_merge:   unions of a run with the run to its left across the segment edge (W neighbour) and with the runs of the row
//                    above that touch it (N; with connectivity 8 also NW and NE).  Of the pixels of a run that meet the same
//                    upper run only the first one issues the union.  A union walks both nodes to their roots and hangs the
//                    larger root below the smaller one by atomicMin; when the atomic finds that the larger one was no root any
//                    more, it goes on with what it found there.  Parents only ever decrease, so there are no cycles, and the
//                    root of a finished component is its smallest index: its first pixel in raster order.
//   patches_flatten: every run start finds its root (halving its path), the run's pixels take it, and the run start adds
//                    the run's length to area[root] -- one integer atomic per run.
//   patches_count, patches_scan, patches_number: root flags (parent[g] == g and area[g] >= min_area) become patch numbers by
//                    block counts, a scan per plane and ballot ranks, as gsd_depth_points compacts its points; the scan here
//                    is one block PER PLANE because the numbers restart with every plane.  The number replaces area[root].
//   patches_relabel: labels[g] = number[parent[g]], in place.
//
// Every loop that follows parents carries the bound H W: a chain has at most one node per pixel of the plane, and every round
// of a union lowers the larger of its two nodes.  A logic error would end in a wrong label, not in a hang.  A parent that a
// wave reads may be out of date (another wave's atomic is under way); it is then an earlier parent of the same node, which
// is still in the node's component, so the walk stays inside the component and the atomic's return value corrects it.
// Every write replaces a link (y, c) by a link (y, n) with n connected to c by other links or by a union that its writer
// still has to finish: no connection is ever lost.
//
// Statistics: a wave reduces the pixels of eight rows of a segment per distinct label (shuffles, at most 32 labels per row),
// keeps the sums of the label it met last in registers and issues one 64-bit integer atomic per column of the table when the
// label changes and at the end: add for the sums, max for the extremes.
// Minima are kept as the maximum of the complement, so that a zero-filled table is the identity of every column; a last pass
// turns them back in the rows that hold a patch.  Integer sums, extremes and key minima do not depend on the order.
#include "gsd_common.h"

#include <math.h>

namespace {

constexpr int CP_SEG = GSD_CONTACT_PATCHES_SEG;      // columns per wave: the tile edge along a row
constexpr int CP_THREADS = 256;                      // 4 waves = 4 segments per block
constexpr int CP_WAVES = CP_THREADS / 64;
constexpr int CP_BLOCK = 1024;                       // pixels of one plane per block of the count and number launches
constexpr int CP_ROUNDS = CP_BLOCK / CP_THREADS;
constexpr int CP_SLOTS = CP_BLOCK / 64;
constexpr int CP_COLS = GSD_CONTACT_PATCHES_COLS;    // int64 columns per row of the statistics
constexpr int CP_STAT_ROWS = 8;                      // rows of a segment that one wave of the statistics launch sums
static_assert(CP_SEG == 64, "a segment is one wave wide");

struct CpView {
  float contact;      // a pixel is contact iff d < -contact
  int conn8, min_area;
  int H, W, nseg;     // nseg: segments per row
  int planes;         // 2 B
  int bound;          // H W: what every parent walk is limited to
  int nblk;           // count / number blocks per plane
};

// the segment this wave owns
struct CpSeg {
  bool any;           // false: past the last segment (the whole wave)
  int r, c;           // c: this lane's column, may be >= W in the last segment
  bool in;
  int g;              // (plane H + r) W + c, valid where `in`
};
__device__ __forceinline__ CpSeg cp_seg(const CpView& V) {
  CpSeg S;
  const long long total = (long long)V.planes * V.H * V.nseg;
  const long long gw = (long long)blockIdx.x * CP_WAVES + (threadIdx.x >> 6);
  S.any = gw < total;
  const int seg = (int)(gw % V.nseg);
  const long long row = gw / V.nseg;      // plane H + r
  S.r = (int)(row % V.H);
  S.c = seg * CP_SEG + (threadIdx.x & 63);
  S.in = S.any && S.c < V.W;
  S.g = (int)(row * V.W + S.c);           // below 2^31 where `in`: 2 B H W is
  return S;
}

// first lane of the run of set bits of `m` that holds `lane` (bit `lane` is set)
__device__ __forceinline__ int cp_run_start(unsigned long long m, int lane) {
  const unsigned long long below = ~m & ((1ull << lane) - 1ull);
  return below ? 64 - __clzll((long long)below) : 0;
}
// length of the run of set bits of `m` that starts at `start`
__device__ __forceinline__ int cp_run_len(unsigned long long m, int start) {
  const unsigned long long t = ~m >> start;
  return t ? __ffsll((long long)t) - 1 : 64 - start;
}

__device__ __forceinline__ int cp_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Root of node x: follow the parents while they decrease, at most `bound` steps, halving the path on the way: a node whose
// parent p has the parent gp < p is hung below gp.  The three values are read as one chain (x -> p -> gp), so gp is an ancestor of
// x whatever other waves do meanwhile; a second walk from x that hung the nodes it meets below a root found earlier would not
// be safe: x may have been moved to another tree in between, and a node of that tree would lose its only link.
__device__ __forceinline__ int cp_find(int* parent, int x, int bound) {
  for (int it = 0; it < bound; ++it) {
    const int p = cp_load(parent + x);
    if (p >= x || p < 0) break;           // x is a root
    const int gp = cp_load(parent + p);
    if (gp >= p || gp < 0) return p;      // p is
    atomicMin(parent + x, gp);
    x = gp;
  }
  return x;
}

// one component out of those of pixels a and b
__device__ __forceinline__ void cp_union(int* parent, int a, int b, int bound) {
  for (int it = 0; it < bound; ++it) {
    a = cp_find(parent, a, bound), b = cp_find(parent, b, bound);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = atomicMin(parent + a, b);      // a > b
    if (old == a) return;                          // a was a root and hangs below b now
    a = old;                                       // it was not: what hung there has to meet b as well; old < a
  }
}

__global__ __launch_bounds__(CP_THREADS) void patches_init(const CpView V, const float* __restrict__ depth, int* __restrict__ parent,
                                                         int* __restrict__ area) {
  const CpSeg S = cp_seg(V);
  if (!S.any) return;
  const int lane = threadIdx.x & 63;
  const float d = S.in ? depth[S.g] : 0.f;
  const bool is = S.in && d < -V.contact;      // false for a NaN
  const unsigned long long m = __ballot(is);
  if (S.in) {
    parent[S.g] = is ? S.g - lane + cp_run_start(m, lane) : -1;
    area[S.g] = 0;
  }
}

__global__ __launch_bounds__(CP_THREADS) void patches_merge(const CpView V, int* parent) {
  const CpSeg S = cp_seg(V);
  if (!S.any) return;
  const int lane = threadIdx.x & 63, W = V.W;
  const bool is = S.in && cp_load(parent + S.g) >= 0;
  const bool above = S.in && S.r > 0 && cp_load(parent + S.g - W) >= 0;
  const unsigned long long cur = __ballot(is), up = __ballot(above);
  if (!is) return;
  const bool cur_l = lane > 0 && ((cur >> (lane - 1)) & 1), cur_r = lane < 63 && ((cur >> (lane + 1)) & 1);
  // W: the run that ends in the segment to the left
  if (lane == 0 && S.c > 0 && cp_load(parent + S.g - 1) >= 0) cp_union(parent, S.g, S.g - 1, V.bound);
  if (S.r == 0) return;
  const bool up_l = lane > 0 ? ((up >> (lane - 1)) & 1) : (V.conn8 && S.c > 0 && cp_load(parent + S.g - W - 1) >= 0);
  const bool up_r = lane < 63 ? ((up >> (lane + 1)) & 1) : (V.conn8 && S.c + 1 < W && cp_load(parent + S.g - W + 1) >= 0);
  if (above) {
    // N.  The pixel to the left has met the same upper run if it is contact with contact above it.
    if (!(cur_l && up_l)) cp_union(parent, S.g, S.g - W, V.bound);
  } else if (V.conn8) {
    // NW: left to the pixel on the left when that is contact (the upper pixel is straight above it)
    if (up_l && !cur_l) cp_union(parent, S.g, S.g - W - 1, V.bound);
    // NE: left to the pixel on the right likewise
    if (up_r && !cur_r) cp_union(parent, S.g, S.g - W + 1, V.bound);
  }
}

__global__ __launch_bounds__(CP_THREADS) void patches_flatten(const CpView V, int* parent, int* __restrict__ area) {
  const CpSeg S = cp_seg(V);
  if (!S.any) return;
  const int lane = threadIdx.x & 63;
  const bool is = S.in && cp_load(parent + S.g) >= 0;
  const unsigned long long m = __ballot(is);
  const int start = is ? cp_run_start(m, lane) : lane;
  int root = -1;
  if (is && start == lane) root = cp_find(parent, S.g, V.bound);
  root = __shfl(root, start, 64);
  if (!is) return;
  parent[S.g] = root;
  if (start == lane) atomicAdd(area + root, cp_run_len(m, lane));
}

// pixel j * CP_THREADS + threadIdx.x of the block's CP_BLOCK pixels, if it is a root (else -1), and whether its patch is kept
__device__ __forceinline__ int cp_root(const CpView& V, const int* __restrict__ parent, const int* __restrict__ area, int j, bool* kept) {
  const int plane = blockIdx.x / V.nblk;
  const int i = (blockIdx.x % V.nblk) * CP_BLOCK + j * CP_THREADS + threadIdx.x;
  *kept = false;
  if (i >= V.bound) return -1;
  const int g = plane * V.bound + i;
  if (parent[g] != g) return -1;
  *kept = area[g] >= V.min_area;
  return g;
}

__global__ __launch_bounds__(CP_THREADS) void patches_count(const CpView V, const int* __restrict__ parent, const int* __restrict__ area,
                                                          int* __restrict__ block_count) {
  __shared__ int wave_n[CP_WAVES];
  bool is[CP_ROUNDS];
#pragma unroll
  for (int j = 0; j < CP_ROUNDS; ++j) cp_root(V, parent, area, j, &is[j]);
  int n = 0;
#pragma unroll
  for (int j = 0; j < CP_ROUNDS; ++j) n += __popcll(__ballot(is[j]));
  n = gsd_block_count<CP_THREADS>(n, wave_n);
  if (threadIdx.x == 0) block_count[blockIdx.x] = n;
}

// One block per plane: the plane's block counts -> exclusive offsets in place, CP_THREADS counts per pass with a carry; the
// total is the plane's count of kept patches.
__global__ __launch_bounds__(CP_THREADS) void patches_scan(int nblk, int* block_off, int* __restrict__ counts) {
  int* off = block_off + (size_t)blockIdx.x * nblk;
  const int carry = gsd_block_exclusive_scan<int, CP_THREADS, 1>(      // below 2^31: there are fewer pixels than that
      nblk, [&](int i) { return off[i]; }, [&](int i, int run) { off[i] = run; });
  if (threadIdx.x == 0) counts[blockIdx.x] = carry;
}

// area[root] becomes the patch's number, 0 for a root that is dropped
__global__ __launch_bounds__(CP_THREADS) void patches_number(const CpView V, const int* __restrict__ parent, int* __restrict__ area,
                                                           const int* __restrict__ block_off) {
  __shared__ int slot_n[CP_SLOTS];
  bool is[CP_ROUNDS];
  int g[CP_ROUNDS], rank[CP_ROUNDS];
  unsigned long long mask[CP_ROUNDS];
#pragma unroll
  for (int j = 0; j < CP_ROUNDS; ++j) g[j] = cp_root(V, parent, area, j, &is[j]);
#pragma unroll
  for (int j = 0; j < CP_ROUNDS; ++j) mask[j] = __ballot(is[j]);
  gsd_block_rank<CP_THREADS, CP_ROUNDS>(mask, slot_n, rank);
  const int base = block_off[blockIdx.x];
#pragma unroll
  for (int j = 0; j < CP_ROUNDS; ++j)
    if (g[j] >= 0) area[g[j]] = is[j] ? base + rank[j] + 1 : 0;
}

__global__ __launch_bounds__(CP_THREADS) void patches_relabel(long long pixels, int* __restrict__ labels, const int* __restrict__ number) {
  const long long g = (long long)blockIdx.x * CP_THREADS + threadIdx.x;
  if (g >= pixels) return;
  const int p = labels[g];
  labels[g] = p >= 0 ? number[p] : 0;
}

// ---- statistics ------------------------------------------------------------------------------------------------------------
// the order-preserving map of the fp32 bits to uint32
__device__ __forceinline__ unsigned cp_ord(float d) {
  const unsigned u = __float_as_uint(d);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(CP_THREADS) void patches_stats_zero(long long words, unsigned long long* __restrict__ stats) {
  const long long i = (long long)blockIdx.x * CP_THREADS + threadIdx.x;
  if (i < words) stats[i] = 0ull;
}

// What a wave has summed for one label and not yet added to the table; every member holds the same value in all lanes.
struct CpSums {
  int label;      // 0: nothing
  long long n, r_min, r_max, k_min, k_max, sum_r, sum_k, sum_rr, sum_kk, sum_rk, sum_dq;
  unsigned long long peak;
};
__device__ __forceinline__ void cp_flush(const CpSums& A, int plane, int K, unsigned long long* __restrict__ stats) {
  if (A.label == 0 || (threadIdx.x & 63) != 0) return;
  unsigned long long* row = stats + ((size_t)plane * K + (A.label - 1)) * CP_COLS;
  atomicAdd(row + 0, (unsigned long long)A.n);
  atomicMax(row + 1, ~(unsigned long long)A.r_min);
  atomicMax(row + 2, (unsigned long long)A.r_max);
  atomicMax(row + 3, ~(unsigned long long)A.k_min);
  atomicMax(row + 4, (unsigned long long)A.k_max);
  atomicAdd(row + 5, (unsigned long long)A.sum_r);
  atomicAdd(row + 6, (unsigned long long)A.sum_k);
  atomicAdd(row + 7, (unsigned long long)A.sum_rr);
  atomicAdd(row + 8, (unsigned long long)A.sum_kk);
  atomicAdd(row + 9, (unsigned long long)A.sum_rk);
  atomicAdd(row + 10, (unsigned long long)A.sum_dq);      // two's complement: the sum of negative terms wraps to the right bits
  atomicMax(row + 11, ~A.peak);
}

// A wave owns CP_STAT_ROWS consecutive rows of one 64-column segment.  Row by row it reduces the pixels of each distinct label
// (at most 32 per row) and keeps the sums of the label it met last in registers; they go to the table, one 64-bit integer
// atomic per column, when another label turns up and at the end.  Inside a large patch that is one set of atomics per wave.
__global__ __launch_bounds__(CP_THREADS) void patches_stats(const CpView V, const float* __restrict__ depth, const int* __restrict__ labels,
                                                          int K, unsigned long long* __restrict__ stats) {
#pragma clang fp contract(off)
  const int nband = (V.H + CP_STAT_ROWS - 1) / CP_STAT_ROWS;
  const long long gw = (long long)blockIdx.x * CP_WAVES + (threadIdx.x >> 6);
  if (gw >= (long long)V.planes * nband * V.nseg) return;      // the whole wave
  const int lane = threadIdx.x & 63;
  const int seg = (int)(gw % V.nseg), band = (int)((gw / V.nseg) % nband), plane = (int)(gw / ((long long)V.nseg * nband));
  const int c = seg * CP_SEG + lane, r0 = band * CP_STAT_ROWS;
  const bool in = c < V.W;
  int lab[CP_STAT_ROWS];
  float d[CP_STAT_ROWS];
#pragma unroll
  for (int j = 0; j < CP_STAT_ROWS; ++j) {
    const bool here = in && r0 + j < V.H;
    const size_t g = ((size_t)plane * V.H + (here ? r0 + j : 0)) * V.W + (here ? c : 0);
    lab[j] = here ? labels[g] : 0;
    d[j] = here ? depth[g] : 0.f;
  }
  CpSums A;
  A.label = 0;
#pragma unroll
  for (int j = 0; j < CP_STAT_ROWS; ++j) {
    const bool active = lab[j] >= 1 && lab[j] <= K;
    unsigned long long rem = __ballot(active);
    if (rem == 0ull) continue;
    const long long r = r0 + j, k = c;
    const long long dq = active ? (long long)rint((double)fmaxf(d[j], -1024.0f) * 1048576.0) : 0ll;
    const unsigned long long key = ((unsigned long long)cp_ord(d[j]) << 32) | (unsigned)(r * V.W + k);
    for (int it = 0; it < 64 && rem != 0ull; ++it) {      // one round per distinct label of the row
      const int which = __shfl(lab[j], __ffsll((long long)rem) - 1, 64);
      const bool mine = active && lab[j] == which;
      const unsigned long long mm = __ballot(mine);
      const long long sum_k = gsd_wave_sum(mine ? k : 0ll), sum_kk = gsd_wave_sum(mine ? k * k : 0ll), sum_dq = gsd_wave_sum(mine ? dq : 0ll);
      const unsigned long long peak = gsd_wave_min(mine ? key : ~0ull);
      const long long n = __popcll(mm), base = seg * CP_SEG;
      const long long k_min = base + __ffsll((long long)mm) - 1, k_max = base + 63 - __clzll((long long)mm);
      if (which != A.label) {
        cp_flush(A, plane, K, stats);
        A.label = which;
        A.n = 0, A.r_min = r, A.r_max = r, A.k_min = k_min, A.k_max = k_max;
        A.sum_r = A.sum_k = A.sum_rr = A.sum_kk = A.sum_rk = A.sum_dq = 0;
        A.peak = ~0ull;
      }
      A.n += n;
      A.r_min = r < A.r_min ? r : A.r_min, A.r_max = r > A.r_max ? r : A.r_max;
      A.k_min = k_min < A.k_min ? k_min : A.k_min, A.k_max = k_max > A.k_max ? k_max : A.k_max;
      A.sum_r += r * n, A.sum_k += sum_k, A.sum_rr += r * r * n, A.sum_kk += sum_kk, A.sum_rk += r * sum_k, A.sum_dq += sum_dq;
      A.peak = peak < A.peak ? peak : A.peak;
      rem &= ~mm;
    }
  }
  cp_flush(A, plane, K, stats);
}

// the complemented minima back, in the rows that hold a patch (area > 0); the others stay all zero
__global__ __launch_bounds__(CP_THREADS) void patches_stats_finish(long long rows, unsigned long long* __restrict__ stats) {
  const long long i = (long long)blockIdx.x * CP_THREADS + threadIdx.x;
  if (i >= rows) return;
  unsigned long long* row = stats + i * CP_COLS;
  if (row[0] == 0ull) return;
  row[1] = ~row[1], row[3] = ~row[3], row[11] = ~row[11];
}

// ---- filter ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CP_THREADS) void patches_filter(float contact, long long pixels, int plane_pixels, int K,
                                                           const unsigned* __restrict__ depth, const int* __restrict__ labels,
                                                           const unsigned char* __restrict__ keep, unsigned* __restrict__ out) {
  const long long g = (long long)blockIdx.x * CP_THREADS + threadIdx.x;
  if (g >= pixels) return;
  const unsigned bits = depth[g];
  const int lab = labels[g];
  const bool is = __uint_as_float(bits) < -contact;
  bool kept = lab > 0;
  if (kept && keep != nullptr) kept = lab <= K && keep[(size_t)(g / plane_pixels) * (K + 1) + lab] != 0;
  out[g] = (is && !kept) ? 0u : bits;
}

// ---- host layer ------------------------------------------------------------------------------------------------------------
bool cp_dims_ok(int B, int H, int W) { return B >= 1 && H >= 1 && W >= 1 && 2 * (int64_t)B * H * W < ((int64_t)1 << 31); }
struct CpLayout {      // the workspace in int32 words: the areas / numbers (one per pixel), then the block counts / offsets
  int64_t blocks, words;
  int nblk;
};
CpLayout cp_layout(int B, int H, int W) {
  CpLayout Y;
  Y.nblk = (int)ceil_div64((int64_t)H * W, CP_BLOCK);
  Y.blocks = 2 * (int64_t)B * H * W;
  Y.words = (Y.blocks + 2 * (int64_t)B * Y.nblk + 1) / 2 * 2;
  return Y;
}
int cp_check_view(const gsd_contact_patches_view* v, const char* what) {
  GSD_REQUIRE(v != nullptr, GSD_ERR_BAD_ARG, "%s: null view", what);
  GSD_REQUIRE(isfinite(v->contact_depth) && v->contact_depth >= 0.0, GSD_ERR_BAD_ARG, "%s: contact_depth %g must be finite and >= 0", what,
              v->contact_depth);
  GSD_REQUIRE(v->connectivity == 4 || v->connectivity == 8, GSD_ERR_BAD_ARG, "%s: connectivity %d must be 4 or 8", what, v->connectivity);
  GSD_REQUIRE(v->min_area >= 1, GSD_ERR_BAD_ARG, "%s: min_area %d must be at least 1", what, v->min_area);
  return 0;
}
CpView cp_view(const gsd_contact_patches_view& v, int B, int H, int W) {
  CpView V;
  V.contact = (float)v.contact_depth, V.conn8 = v.connectivity == 8, V.min_area = v.min_area;
  V.H = H, V.W = W, V.nseg = ceil_div(W, CP_SEG), V.planes = 2 * B, V.bound = H * W, V.nblk = cp_layout(B, H, W).nblk;
  return V;
}
// blocks of the launches that give every (plane, row, segment) a wave: at most 2 B H W / 4 + 1
unsigned cp_seg_blocks(const CpView& V) { return (unsigned)ceil_div64((int64_t)V.planes * V.H * V.nseg, CP_WAVES); }

}  // namespace

extern "C" {

int64_t gsd_contact_patches_workspace(int B, int H, int W) { return cp_dims_ok(B, H, W) ? cp_layout(B, H, W).words : 0; }

int gsd_contact_patches_label(const gsd_contact_patches_view* view, const float* depth, int B, int H, int W, int32_t* labels,
                              int32_t* counts, int32_t* workspace, int64_t workspace_elems, void* stream) {
  const char* what = "gsd_contact_patches_label";
  if (const int rc = cp_check_view(view, what)) return rc;
  GSD_REQUIRE(depth && labels && counts && workspace, GSD_ERR_BAD_ARG, "%s: null pointer", what);
  GSD_REQUIRE(cp_dims_ok(B, H, W), GSD_ERR_BAD_ARG, "%s: bad dims B=%d H=%d W=%d (each at least 1, 2 B H W below 2^31)", what, B, H, W);
  const CpLayout Y = cp_layout(B, H, W);
  GSD_REQUIRE(workspace_elems >= Y.words, GSD_ERR_WORKSPACE, "%s: workspace of %lld int32 words, need %lld", what,
              (long long)workspace_elems, (long long)Y.words);
  const CpView V = cp_view(*view, B, H, W);
  hipStream_t st = (hipStream_t)stream;
  int* area = workspace;
  int* block_off = workspace + Y.blocks;
  const dim3 threads(CP_THREADS), segs(cp_seg_blocks(V)), blocks((unsigned)(V.planes * V.nblk));
  const long long pixels = (long long)V.planes * V.bound;
  hipLaunchKernelGGL(patches_init, segs, threads, 0, st, V, depth, labels, area);
  GSD_LAUNCH_CHECK(what);
  hipLaunchKernelGGL(patches_merge, segs, threads, 0, st, V, labels);
  GSD_LAUNCH_CHECK(what);
  hipLaunchKernelGGL(patches_flatten, segs, threads, 0, st, V, labels, area);
  GSD_LAUNCH_CHECK(what);
  hipLaunchKernelGGL(patches_count, blocks, threads, 0, st, V, (const int*)labels, (const int*)area, block_off);
  GSD_LAUNCH_CHECK(what);
  hipLaunchKernelGGL(patches_scan, dim3((unsigned)V.planes), threads, 0, st, V.nblk, block_off, counts);
  GSD_LAUNCH_CHECK(what);
  hipLaunchKernelGGL(patches_number, blocks, threads, 0, st, V, (const int*)labels, area, (const int*)block_off);
  GSD_LAUNCH_CHECK(what);
  hipLaunchKernelGGL(patches_relabel, dim3((unsigned)ceil_div64(pixels, CP_THREADS)), threads, 0, st, pixels, labels, (const int*)area);
  GSD_LAUNCH_CHECK(what);
  return GSD_OK;
}

int gsd_contact_patches_stats(const gsd_contact_patches_view* view, const float* depth, const int32_t* labels, int B, int H, int W, int K,
                              int64_t* stats, void* stream) {
  const char* what = "gsd_contact_patches_stats";
  if (const int rc = cp_check_view(view, what)) return rc;
  GSD_REQUIRE(depth && labels && stats, GSD_ERR_BAD_ARG, "%s: null pointer", what);
  GSD_REQUIRE(cp_dims_ok(B, H, W), GSD_ERR_BAD_ARG, "%s: bad dims B=%d H=%d W=%d (each at least 1, 2 B H W below 2^31)", what, B, H, W);
  GSD_REQUIRE(K >= 1 && 2 * (int64_t)B * K * CP_COLS < ((int64_t)1 << 31), GSD_ERR_BAD_ARG,
              "%s: K %d must be at least 1 and the table below 2^31 values", what, K);
  const CpView V = cp_view(*view, B, H, W);
  hipStream_t st = (hipStream_t)stream;
  const long long rows = 2ll * B * K, words = rows * CP_COLS;
  unsigned long long* table = reinterpret_cast<unsigned long long*>(stats);
  hipLaunchKernelGGL(patches_stats_zero, dim3((unsigned)ceil_div64(words, CP_THREADS)), dim3(CP_THREADS), 0, st, words, table);
  GSD_LAUNCH_CHECK(what);
  const int64_t stat_waves = (int64_t)V.planes * ceil_div(H, CP_STAT_ROWS) * V.nseg;
  hipLaunchKernelGGL(patches_stats, dim3((unsigned)ceil_div64(stat_waves, CP_WAVES)), dim3(CP_THREADS), 0, st, V, depth, labels, K, table);
  GSD_LAUNCH_CHECK(what);
  hipLaunchKernelGGL(patches_stats_finish, dim3((unsigned)ceil_div64(rows, CP_THREADS)), dim3(CP_THREADS), 0, st, rows, table);
  GSD_LAUNCH_CHECK(what);
  return GSD_OK;
}

int gsd_contact_patches_filter(const gsd_contact_patches_view* view, const float* depth, const int32_t* labels, const uint8_t* keep, int B,
                               int H, int W, int K, float* out, void* stream) {
  const char* what = "gsd_contact_patches_filter";
  if (const int rc = cp_check_view(view, what)) return rc;
  GSD_REQUIRE(depth && labels && out, GSD_ERR_BAD_ARG, "%s: null pointer", what);
  GSD_REQUIRE(cp_dims_ok(B, H, W), GSD_ERR_BAD_ARG, "%s: bad dims B=%d H=%d W=%d (each at least 1, 2 B H W below 2^31)", what, B, H, W);
  GSD_REQUIRE(K >= 1 && 2 * (int64_t)B * ((int64_t)K + 1) < ((int64_t)1 << 31), GSD_ERR_BAD_ARG,
              "%s: K %d must be at least 1 and the keep table below 2^31 entries", what, K);
  const long long pixels = 2ll * B * H * W;
  hipLaunchKernelGGL(patches_filter, dim3((unsigned)ceil_div64(pixels, CP_THREADS)), dim3(CP_THREADS), 0, (hipStream_t)stream,
                     (float)view->contact_depth, pixels, H * W, K, reinterpret_cast<const unsigned*>(depth), labels, keep,
                     reinterpret_cast<unsigned*>(out));
  GSD_LAUNCH_CHECK(what);
  return GSD_OK;
}

}  // extern "C"
