// gsd_cell_lists.h -- the per-cell triangle lists of MeshGrid (gsd_mesh_depth_*) and MeshVolume (gsd_mesh_volume_*): one
// workspace layout, one set of argument checks and one count / scan / fill sequence.
//
//   cells, int32 words:  total (int64) | start[ncells + 1] | cursor[ncells]
//
// count: memset of all of it, the unit's count kernel (+1 per (cell, triangle) pair on start), the unit's scan kernel (start
// becomes the exclusive sums, cursor a copy, the head the int64 total).  fill: the unit's fill kernel moves the cursors, after
// which cursor[c] == start[c + 1].  The checks need no device: a host-only program can include this file.
#pragma once
#include <stdint.h>

#include "gsd.h"
#include "gsd_error.h"

struct GsdCellCall {
  const char* what;          // the entry point that was called: it begins every message
  const void* geometry;      // the triangles or records that the unit's kernels read
  int T, max_T;
  int64_t ncells;            // of a grid that the unit has checked already
  int32_t* cells;
  int64_t cells_elems;
  int32_t* list;             // fill only
  int64_t list_elems;
};

static inline int64_t gsd_cell_words(int64_t ncells) { return 2 + (ncells + 1) + ncells; }

static inline int gsd_cell_check(const GsdCellCall& Q, bool fill) {
  GSD_REQUIRE(Q.geometry && Q.cells && (!fill || Q.list), GSD_ERR_BAD_ARG, "%s: null pointer", Q.what);
  GSD_REQUIRE(Q.T >= 1 && Q.T <= Q.max_T, GSD_ERR_BAD_ARG, "%s: %d triangles, 1..%d", Q.what, Q.T, Q.max_T);
  // the order of gsd_mesh_volume_fill: a list length out of range is GSD_ERR_BAD_ARG whatever the workspace is
  GSD_REQUIRE(!fill || (Q.list_elems >= 1 && Q.list_elems <= INT32_MAX), GSD_ERR_BAD_ARG, "%s: list of %lld entries, 1..2^31-1", Q.what,
              (long long)Q.list_elems);
  GSD_REQUIRE(((uintptr_t)Q.cells & 7) == 0, GSD_ERR_BAD_ARG, "%s: cells must be 8-byte aligned", Q.what);
  GSD_REQUIRE(Q.cells_elems >= gsd_cell_words(Q.ncells), GSD_ERR_WORKSPACE, "%s: cells of %lld words, need %lld", Q.what,
              (long long)Q.cells_elems, (long long)gsd_cell_words(Q.ncells));
  return GSD_OK;
}

#ifdef __HIPCC__
#include "gsd_common.h"

constexpr int GSD_CELL_SCAN_THREADS = 1024, GSD_CELL_SCAN_PER = 2;      // 2, 4 and 8 counts per thread were timed: DESIGN.md section 25

// The body of a unit's scan kernel (one block of GSD_CELL_SCAN_THREADS): sums in int64, the low 32 bits stored -- the int32 starts
// wrap beyond 2^31 - 1 pairs, and the caller reads the total before it fills.
__device__ __forceinline__ void gsd_cell_scan(int ncells, int* __restrict__ start, int* __restrict__ cursor, long long* __restrict__ total) {
  const long long all = gsd_block_exclusive_scan<long long, GSD_CELL_SCAN_THREADS, GSD_CELL_SCAN_PER>(
      ncells, [&](int c) { return start[c]; }, [&](int c, long long run) { start[c] = cursor[c] = (int)run; });
  if (threadIdx.x == 0) start[ncells] = (int)all, *total = all;
}

// launch_count(start) launches the unit's count kernel; scan is its scan kernel
template <typename Count, typename Scan>
int gsd_cell_count(const GsdCellCall& Q, Count launch_count, Scan scan, hipStream_t st) {
  if (const int rc = gsd_cell_check(Q, false)) return rc;
  if (hipError_t e = hipMemsetAsync(Q.cells, 0, sizeof(int32_t) * (size_t)gsd_cell_words(Q.ncells), st); e != hipSuccess) {
    gsd_set_error("%s: hipMemsetAsync: %s", Q.what, hipGetErrorString(e));
    return GSD_ERR_HIP;
  }
  int* start = Q.cells + 2;
  launch_count(start);
  GSD_LAUNCH_CHECK(Q.what);
  hipLaunchKernelGGL(scan, dim3(1), dim3(GSD_CELL_SCAN_THREADS), 0, st, (int)Q.ncells, start, start + Q.ncells + 1,
                     reinterpret_cast<long long*>(Q.cells));
  GSD_LAUNCH_CHECK(Q.what);
  return GSD_OK;
}

// fill(G, geometry, T, cursor, list, list_elems) is the unit's fill kernel, one thread per triangle
template <typename Fill, typename Grid>
int gsd_cell_fill(const GsdCellCall& Q, Fill fill, const Grid& G, hipStream_t st) {
  if (const int rc = gsd_cell_check(Q, true)) return rc;
  hipLaunchKernelGGL(fill, dim3((unsigned)ceil_div(Q.T, 256)), dim3(256), 0, st, G, static_cast<const float*>(Q.geometry), Q.T,
                     Q.cells + 2 + Q.ncells + 1, Q.list, (long long)Q.list_elems);
  GSD_LAUNCH_CHECK(Q.what);
  return GSD_OK;
}
#endif
