// gsd_bf16_host.h -- host-side code shared by the six bf16 MFMA convolution units: gsd_bf16_conv.hip, gsd_bf16_ctgemm.hip,
// gsd_bf16_wgrad.hip, gsd_bf16_c64.hip, gsd_bf16_inc.hip and gsd_bf16_first.hip.  The rules that size a launch -- and with it the
// BatchNorm partial rows and workspace elements the engine allocates BEFORE the launch, so a query and its launch go through the same
// call here -- the XCD-order flag, the tile picker, and the operands of the fused BatchNorm backward.  Every planner deals its blocks
// over gsd_cu_count() (gsd_common.h).  Library-internal (C++ linkage, not part of include/gsd_bf16.h).
#pragma once
#include <stdio.h>
#include "gsd_bf16_common.h"

// ---- gsd_bf16_ctgemm.hip: the large-tile kernel behind gsd_bf16_conv_dense for the transposed convolutions' forward and dX ---------
bool gsd_ctgemm_shape(int N, int H, int W, int K, int M, int ntaps, int stride, int scatter_cs);
bool gsd_ctgemm_operands(const gsd_nhwc* in, const gsd_nhwc* out, const gsd_bf16_bnbwd* bw, int ntaps, const int* ty, const int* tx, int H,
                         int W);
int gsd_ctgemm_misfit(const gsd_nhwc* in, const gsd_nhwc* out, const gsd_nhwc* y, int ntaps, const int* ty, const int* tx, int H, int W);
int gsd_ctgemm_partial_rows(int N, int H, int W, int M);
int gsd_ctgemm_launch(const gsd_nhwc* in, const void* wt, const gsd_nhwc* out, int K, int M, int ntaps, const int* ty, const int* tx, int H,
                      int W, int scatter_cs, int oy, int ox, const float* bias, float* partials, const gsd_bf16_bnbwd* bw, void* stream);

// ---- persistent grids --------------------------------------------------------------------------------------------------------------
// Blocks that each keep ONE m-block (gconv_bf16_kernel, ctgemm_bf16_kernel): items = (pixel tile, m-block) pairs, one block per CU
// (the LDS image allows one) rounded down to a multiple of mblocks, at least mblocks, at most the items.
static inline long bf16_mblock_grid(long items, int mblocks) {
  long grid = gsd_cu_count() / mblocks * mblocks;
  if (grid < mblocks) grid = mblocks;
  return grid > items ? items : grid;
}

// Blocks that walk the TH x TW pixel tiles of an (N, H, W) image set (c64, inc, first, first dW): min(tiles, cap) of them, one
// partial row or slab each.  false: 2^31 tiles or more, which every launch refuses (ntiles and grid are then those of 2^31 - 1).
struct Bf16Tiles {
  int tiles_y, tiles_x, ntiles, grid;
};
static inline bool bf16_tile_grid(int N, int H, int W, int TH, int TW, int cap, Bf16Tiles* t) {
  t->tiles_y = ceil_div(H, TH);
  t->tiles_x = ceil_div(W, TW);
  const long nt = (long)N * t->tiles_y * t->tiles_x;
  t->ntiles = nt < 2147483647L ? (int)nt : 2147483647;
  t->grid = t->ntiles < cap ? t->ntiles : cap;
  return nt < 2147483647L;
}
// ... as the launch of the entry point `name` takes it: the tile counts of the kernel parameters (which hold N, H, W) and the grid
template <class Params>
static inline int bf16_plan_tiles(const char* name, Params& P, int TH, int TW, int cap, int* grid) {
  Bf16Tiles t;
  GSD_REQUIRE(bf16_tile_grid(P.N, P.H, P.W, TH, TW, cap, &t), GSD_ERR_UNSUPPORTED, "%s: too many tiles", name);
  P.tiles_y = t.tiles_y; P.tiles_x = t.tiles_x; P.ntiles = t.ntiles;
  *grid = t.grid;
  return 0;
}

// ---- XCD-aware block order (GSD_BF16_XCD, default on) --------------------------------------------------------------------------------
// Two conditions that stay apart, because the kernels decode a block index differently.  The weight-gradient kernels renumber any
// grid (xcd_swizzle): the knob alone.  The persistent kernels above give XCD x the pixel tiles [ntile x/8, ntile (x+1)/8) and its
// grid/8 blocks sweep them m-block by m-block: only a grid of 8 x (a multiple of mblocks) blocks can be dealt that way.
static inline bool bf16_xcd_knob() { return gsd_env_int("GSD_BF16_XCD", 1) != 0; }
static inline int bf16_xcd_order(long grid, int mblocks) { return (bf16_xcd_knob() && grid % 8 == 0 && (grid / 8) % mblocks == 0) ? 1 : 0; }

// ---- tile picker ---------------------------------------------------------------------------------------------------------------------
// The TH x TW tile of `npix` pixels, TW a power of two in [tw_min, tw_max], that covers H x W with the fewest tiles, into the plan's
// fields of those names, with the tile counts and the 3 x 3 halo (HC columns, HP pixels).  Ties: the forward kernels take the WIDER tile
// (longer DMA row segments, `<=` over rising TW), the weight gradients the narrower one (`<`).  force_tw != 0: that width only.
template <class Plan>
static inline void bf16_pick_tile(Plan& p, int H, int W, int npix, int tw_min, int tw_max, bool ties_wider, int force_tw) {
  long best = -1;
  for (int tw = tw_min; tw <= tw_max; tw *= 2) {
    if (force_tw && tw != force_tw) continue;
    const int th = npix / tw;
    const long cost = (long)ceil_div(H, th) * ceil_div(W, tw);
    if (best < 0 || cost < best || (ties_wider && cost == best)) {
      best = cost;
      p.TW = tw;
      p.TH = th;
    }
  }
  p.tiles_y = ceil_div(H, p.TH);
  p.tiles_x = ceil_div(W, p.TW);
  p.HC = p.TW + 2;
  p.HP = (p.TH + 2) * (p.TW + 2);
}

// ---- fused BatchNorm + ReLU backward, pass 1 (gsd_bf16_bnbwd) ------------------------------------------------------------------------
// bw of the entry point `name`, whose output is (N, H, W, M): all four coefficient vectors and the partials, and y with out's geometry.
static inline int bf16_check_bnbwd(const char* name, const gsd_bf16_bnbwd* bw, const float* partials, int N, int H, int W, int M) {
  char what[96];
  snprintf(what, sizeof what, "%s bw.y", name);
  if (int e = gsd_check_nhwc(bw->y, what)) return e;
  GSD_REQUIRE(bw->scale && bw->shift && bw->mean && bw->invstd && partials, GSD_ERR_BAD_ARG,
              "%s: fused BatchNorm backward needs coefficients and partials", name);
  GSD_REQUIRE(bw->y->N == N && bw->y->H == H && bw->y->W == W && bw->y->C == M && (bw->y->pitch & 3) == 0, GSD_ERR_BAD_ARG,
              "%s: bw.y must have out's geometry", name);
  return 0;
}
// The bw_* fields that GConvP, CtP and C64P share by name (the structs are kernel arguments and stay separate); bw == nullptr: none.
template <class Params>
static inline void bf16_fill_bnbwd(Params& P, const gsd_bf16_bnbwd* bw) {
  P.bw_y = bw ? (const u16*)bw->y->ptr : nullptr;
  P.bw_pitch = bw ? bw->y->pitch : 0;
  P.bw_scale = bw ? bw->scale : nullptr;
  P.bw_shift = bw ? bw->shift : nullptr;
  P.bw_mean = bw ? bw->mean : nullptr;
  P.bw_invstd = bw ? bw->invstd : nullptr;
}
