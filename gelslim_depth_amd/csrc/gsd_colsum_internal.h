// gsd_colsum_internal.h -- the ordered two-stage column sums of gsd_bn.hip for the other unit that finishes a reduction with
// them (gsd_conv1x1_out_wgrad in gsd_head.hip).  Library-internal (C++ linkage, not part of include/gsd.h); the kernels
// themselves are compiled into gsd_bn.hip only.
#pragma once

// Column sums of `halves` column ranges ([h * half_off, h * half_off + ncols) of every row) of the fp32 matrix
// part[rows][ld], in fp64: sums[h * ncols + col].
// tmp: RG * halves * ncols doubles of scratch (RG: the row groups of stage 1, gsd_bn.hip; the workspace contracts of the
// entry points put tmp right behind `sums`).
// out32 (may be NULL): columns [c_begin, c_begin + c_count) of the first range also leave as fp32.
// Arguments are the entry point's, already validated by it.  Returns a gsd_status; on a failed launch the error string
// is set, with `what` naming the entry point.
int gsd_colsum_run(const char* what, const float* part, int rows, int ld, int ncols, int half_off, int halves, double* sums,
                   double* tmp, float* out32, int c_begin, int c_count, void* stream);
