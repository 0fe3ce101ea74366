// gsd_wgrad_internal.h -- the Winograd forms of the conv3x3 weight gradient as gsd_conv3x3_wgrad (gsd_wgrad.hip) calls them.
// Library-internal (C++ linkage, not part of include/gsd.h); the arguments are the entry point's, already validated by it.
#pragma once
#include <stdint.h>
#include "gsd.h"

// Winograd F(4,3) along rows (gsd_wgrad_w43.hip): same arguments and result layout as the direct form; chosen per shape
// (GSD_WGRAD_ALGO=0|1 forces one)
int gsd_wgrad_w43_use(int N, int H, int W, int Cin, int Cout);
int64_t gsd_wgrad_w43_workspace(int N, int H, int W, int Cin, int Cout);
int64_t gsd_wgrad_w43_mfma_count(int N, int H, int W, int Cin, int Cout);
int gsd_wgrad_w43_run(const gsd_src* a, int nsrc, const gsd_src* dy, int Cin, int Cout, float* dw, float* workspace,
                      int64_t workspace_elems, int N, int H, int W, void* stream);
// slab[split][9][Cout][Cin] -> dW (Cout,Cin,3,3): the ordered split sum, shared by both Winograd forms
int gsd_wgrad_w43_reduce_run(const float* workspace, float* dw, int splits, int Cout, int Cin, void* stream);

// Two-dimensional Winograd F(2x4,3x3) (gsd_wgrad_w2d.hip): chosen per CALL (it needs the row-pitched dy, slack around the
// activation segments and channel counts that are multiples of its block); same slab layout and reducer as the row form
int gsd_wgrad_w2d_use(const gsd_src* a, int nsrc, const gsd_src* dy, int Cin, int Cout, int N, int H, int W);
int64_t gsd_wgrad_w2d_workspace(int N, int H, int W, int Cin, int Cout);
int64_t gsd_wgrad_w2d_mfma_count(int N, int H, int W, int Cin, int Cout);
int gsd_wgrad_w2d_run(const gsd_src* a, int nsrc, const gsd_src* dy, int Cin, int Cout, float* workspace, int64_t workspace_elems,
                      int N, int H, int W, int* splits_out, void* stream);
