// gsd_wgrad_host.h -- host-side code shared by the three conv3x3 weight-gradient forms: direct taps (gsd_wgrad.hip), Winograd F(4,3)
// along rows (gsd_wgrad_w43.hip) and two-dimensional Winograd F(2x4,3x3) (gsd_wgrad_w2d.hip).  The Winograd forms as
// gsd_conv3x3_wgrad calls them, operand validation, the split-count picker, the kernel-parameter fields the forms have in common and
// the operand predicates of the two Winograd forms.  The ConvT k2s2 weight gradient (gsd_convT_wgrad.hip) takes its gradient-operand
// check, split picker and kernel arguments from here too.  Library-internal (C++ linkage, not part of include/gsd.h).
#pragma once
#include "gsd_common.h"

// ---- the Winograd forms as gsd_conv3x3_wgrad (gsd_wgrad.hip) calls them ------------------------------------------------------------
// The arguments are the entry point's, already validated by it (wgrad_check_operands, a workspace that holds any form's slabs).  A
// form's _run writes its partial slabs [slab][9 = r*3+s][Cout][Cin] into `workspace` and returns how many there are (> 0) or a
// GSD_ERR_* code (< 0); the entry point then sums them (wgrad3x3_reduce_kernel), as it does for its own direct form.
//
// Winograd F(4,3) along rows
int64_t gsd_wgrad_w43_workspace(int N, int H, int W, int Cin, int Cout);
int64_t gsd_wgrad_w43_mfma_count(int N, int H, int W, int Cin, int Cout);
int gsd_wgrad_w43_run(const gsd_src* a, int nsrc, const gsd_src* dy, int Cin, int Cout, float* workspace, int N, int H, int W,
                      void* stream);
// Two-dimensional Winograd F(2x4,3x3): chosen per CALL among the shapes that go to a Winograd form (it needs the row-pitched dy, slack
// around the activation segments and channel counts that are multiples of its block; GSD_WGRAD_W2D=0 switches it off)
int gsd_wgrad_w2d_use(const gsd_src* a, int nsrc, const gsd_src* dy, int Cin, int Cout, int N, int H, int W);
int64_t gsd_wgrad_w2d_workspace(int N, int H, int W, int Cin, int Cout);
int64_t gsd_wgrad_w2d_mfma_count(int N, int H, int W, int Cin, int Cout);
int gsd_wgrad_w2d_run(const gsd_src* a, int nsrc, const gsd_src* dy, int Cin, int Cout, float* workspace, int N, int H, int W,
                      void* stream);

// ---- operand validation ------------------------------------------------------------------------------------------------------------
// A gradient operand of the entry point `what`: a plain tensor with sane strides.
static inline int wgrad_check_plain(const gsd_src& s, const char* what) {
  GSD_REQUIRE(s.ptr != nullptr && s.scale == nullptr && s.shift == nullptr && s.relu == 0 && s.off_h == 0 && s.off_w == 0,
              GSD_ERR_BAD_ARG, "%s: gradient operand must be a plain tensor", what);
  GSD_REQUIRE(s.w_stride >= s.W && s.c_stride >= (int64_t)s.H * s.w_stride && s.n_stride >= s.c_stride, GSD_ERR_BAD_ARG,
              "%s: strides too small", what);
  return 0;
}

// Operands of gsd_conv3x3_wgrad.  pitched: the shape goes to a Winograd form -- both address activation and dy rows through w_stride
// and mask by W (a pitched activation, concat or gradient buffer is read in place); the direct form's rows must be contiguous.
static inline int wgrad_check_operands(const gsd_src* a, int nsrc, const gsd_src* dy, int Cin, int Cout, const float* dw,
                                       const float* workspace, int N, int H, int W, bool pitched) {
  GSD_REQUIRE(a && dy && dw && workspace, GSD_ERR_BAD_ARG, "gsd_conv3x3_wgrad: null argument");
  GSD_REQUIRE(nsrc >= 1 && nsrc <= 2, GSD_ERR_BAD_ARG, "gsd_conv3x3_wgrad: nsrc must be 1 or 2");
  GSD_REQUIRE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, GSD_ERR_BAD_ARG, "gsd_conv3x3_wgrad: bad sizes");
  int csum = 0;
  for (int i = 0; i < nsrc; ++i) {
    GSD_REQUIRE(a[i].ptr != nullptr && a[i].C > 0 && a[i].H > 0 && a[i].W > 0, GSD_ERR_BAD_ARG,
                "gsd_conv3x3_wgrad: bad activation segment %d", i);
    GSD_REQUIRE((a[i].scale == nullptr) == (a[i].shift == nullptr), GSD_ERR_BAD_ARG,
                "gsd_conv3x3_wgrad: scale/shift must come together");
    csum += a[i].C;
  }
  GSD_REQUIRE(csum == Cin, GSD_ERR_BAD_ARG, "gsd_conv3x3_wgrad: activation segments hold %d channels, Cin=%d", csum, Cin);
  for (int i = 0; i < nsrc; ++i) {
    GSD_REQUIRE(a[i].w_stride >= a[i].W && a[i].c_stride >= (int64_t)a[i].H * a[i].w_stride && a[i].n_stride >= a[i].c_stride,
                GSD_ERR_BAD_ARG, "gsd_conv3x3_wgrad: activation segment %d: strides too small", i);
    if (!pitched)
      if (int e = gsd_require_rows_contiguous(a[i], "gsd_conv3x3_wgrad activation (direct form)")) return e;
  }
  if (int e = wgrad_check_plain(*dy, "gsd_conv3x3_wgrad dy")) return e;
  if (!pitched)
    if (int e = gsd_require_rows_contiguous(*dy, "gsd_conv3x3_wgrad dy (direct form)")) return e;
  GSD_REQUIRE(dy->C == Cout && dy->H == H && dy->W == W, GSD_ERR_BAD_ARG, "gsd_conv3x3_wgrad: dy must be (Cout,H,W)");
  for (int i = 0; i < nsrc; ++i)
    GSD_REQUIRE(a[i].scale == nullptr || a[i].relu != 0, GSD_ERR_UNSUPPORTED,
                "gsd_conv3x3_wgrad: an affine activation segment must also have relu (zero padding uses a NaN sentinel)");
  return 0;
}

// ---- planning and kernel parameters ------------------------------------------------------------------------------------------------
// Split-K: `target` resident blocks over `tiles` (m, n) tiles, at most one split per stage (or k-step) and 2048, at least one.
static inline int wgrad_pick_splits(int target, int tiles, int stages) {
  int splits = ceil_div(target, tiles);
  if (splits > stages) splits = stages;
  if (splits > 2048) splits = 2048;
  if (splits < 1) splits = 1;
  return splits;
}

// Kernel arguments of the direct conv3x3 form (gsd_wgrad.hip) and of the ConvT k2s2 kernels (gsd_convT_wgrad.hip).  One struct for
// both, as the kernels were compiled before the ConvT code moved out: a struct of its own with the ConvT fields only (and this one
// without tiles_flat) moves the kernel-argument offsets, hipcc then groups the argument loads differently and renumbers the scalar
// registers of all six kernels (profiles/ab_wgrad_asm.txt holds them to the instruction).  A user leaves the other's fields 0.
struct WgradParams {
  SrcD a0, a1;  // B operand (activation; ConvT: a0 = x, a1 unused)
  SrcD dy;      // A operand (gradient, plain)
  float* slabs;
  int M, Ncols, Cact;  // M rows (Cout; ConvT: Cout * 4), Ncols = Cin, Cact = total channels of a0+a1
  int N, H, W;
  int TH, TW, tiles_y, tiles_x, WR, WC, PS;  // conv3x3: stage of TH x TW pixels, its halo window and LDS plane stride
  int tiles_flat;                            // ConvT: 64-pixel stages per image
  int stages_total, splits, mblocks, nblocks;
};

// The kernel-parameter fields that WgradParams, WgW43Params and WgW2dParams share by name (the structs are kernel arguments and stay
// separate: each form adds its own tile geometry).
template <class Params>
static inline void wgrad_fill_common(Params& P, const gsd_src* a, int nsrc, const gsd_src* dy, int Cin, int Cout, float* slabs, int N,
                                     int H, int W, int splits, int mblocks, int nblocks) {
  P.a0 = to_srcd(a[0]);
  P.a1 = nsrc > 1 ? to_srcd(a[1]) : null_srcd();
  P.dy = to_srcd(*dy);
  P.slabs = slabs;
  P.M = Cout; P.Ncols = Cin;
  P.N = N; P.H = H; P.W = W;
  P.splits = splits; P.mblocks = mblocks; P.nblocks = nblocks;
}

// no activation segment carries a deferred BatchNorm / ReLU: the Winograd kernels' PLAIN instantiations drop the transform's fma/max
static inline bool wgrad_plain(const gsd_src* a, int nsrc) {
  for (int i = 0; i < nsrc; ++i)
    if (a[i].scale != nullptr || a[i].relu != 0) return false;
  return true;
}

// dy moves as aligned 16-byte pieces: rows, planes and images of the gradient buffer start 16-byte aligned
static inline bool wgrad_dy_x4(const gsd_src& dy) {
  return dy.w_stride % 4 == 0 && ((uintptr_t)dy.ptr & 15) == 0 && dy.c_stride % 4 == 0 && dy.n_stride % 4 == 0;
}
