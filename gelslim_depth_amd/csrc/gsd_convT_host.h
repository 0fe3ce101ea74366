// gsd_convT_host.h -- host-side code shared by the fp32 ConvTranspose2d(k2,s2) entry points: forward and dX (gsd_convT.hip), dW and db
// (gsd_convT_wgrad.hip).  Operand validation, the rule that admits the LDS-DMA dX kernel, and the plans that fill the kernels'
// geometry fields and size their launches.  Library-internal (C++ linkage, not part of include/gsd.h).
#pragma once
#include <stdio.h>
#include "gsd_common.h"

// Fused backward of relu(bn(raw)) on the destination (gsd_convT2x2_dgrad_bnrelu); all null: a plain dX.
struct ConvTBw {
  const float *raw = nullptr, *scale = nullptr, *shift = nullptr, *mean = nullptr, *invstd = nullptr;
};

// ---- operand validation ------------------------------------------------------------------------------------------------------------
static inline int convT_check_sizes(const char* name, int Cin, int Cout, int N, int H, int W) {
  GSD_REQUIRE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, GSD_ERR_BAD_ARG, "%s: bad sizes", name);
  return 0;
}

// Does the LDS-DMA dX kernel admit these arguments?  Its pixel pairs run over rows of round_up(W, 2) columns: the virtual last
// column of an odd-width plane reads two floats past the end of a dy row -- past the tensor for the very last row, so the caller
// must vouch for them (gsd_src.slack) -- and the batch's dy offsets must fit the kernel's address arithmetic.
static inline bool convT_dgrad_dma_admits(const gsd_src* dy, int Cin, int Cout, int N, int H, int W) {
  if (dy == nullptr || Cin <= 0 || Cout <= 0 || N <= 0 || H <= 0 || W <= 0) return false;
  return !((W & 1) && dy->slack < 2) && (int64_t)N * dy->n_stride < (1LL << 40);
}

// dy of the entry point `name`, which calls the operand `arg`: the plain (Cout, 2H, 2W) gradient, 8-byte aligned with even strides
// (every kernel reads the kw = 0 / 1 pair of a pixel as one 8-byte piece).
static inline int convT_check_dy(const char* name, const char* arg, const gsd_src& dy, int Cout, int H, int W) {
  GSD_REQUIRE(dy.C == Cout && dy.H == 2 * H && dy.W == 2 * W && dy.scale == nullptr && dy.relu == 0 && dy.off_h == 0 && dy.off_w == 0,
              GSD_ERR_BAD_ARG, "%s: %s must be the plain (Cout,2H,2W) gradient", name, arg);
  GSD_REQUIRE(((uintptr_t)dy.ptr & 7) == 0 && (dy.c_stride & 1) == 0 && (dy.n_stride & 1) == 0, GSD_ERR_UNSUPPORTED,
              "%s: %s must be 8-byte aligned with even strides", name, arg);
  return 0;
}

// Source and destination of the forward.  The epilogue addresses output rows through w_stride: a pitched destination -- the
// up-sampled half of a decoder level's concat buffer -- is written in place; only the 8-byte stores ask for an even pitch.
static inline int convT_check_fwd_operands(const char* name, const gsd_src& src, const gsd_dst& dst, int Cin, int Cout, int H, int W) {
  char what[64];
  snprintf(what, sizeof what, "%s src", name);
  if (int e = gsd_check_src(src, what)) return e;
  snprintf(what, sizeof what, "%s dst", name);
  if (int e = gsd_check_dst(dst, what, true)) return e;
  GSD_REQUIRE((dst.w_stride & 1) == 0, GSD_ERR_UNSUPPORTED, "%s: dst needs an even row pitch (got %d)", name, dst.w_stride);
  GSD_REQUIRE(src.C == Cin && src.H == H && src.W == W && src.off_h == 0 && src.off_w == 0, GSD_ERR_BAD_ARG,
              "%s: src must be the full (Cin,H,W) tensor", name);
  GSD_REQUIRE(dst.C == Cout && dst.H == 2 * H && dst.W == 2 * W && dst.off_h == 0 && dst.off_w == 0, GSD_ERR_BAD_ARG,
              "%s: dst must be (Cout,2H,2W)", name);
  GSD_REQUIRE(((uintptr_t)dst.ptr & 7) == 0 && (dst.c_stride & 1) == 0 && (dst.n_stride & 1) == 0, GSD_ERR_UNSUPPORTED,
              "%s: dst must be 8-byte aligned with even strides", name);
  return 0;
}

// Source (dy) and destination of a dX launch, plain or fused (the fused form's raw shares the destination's strides).
static inline int convT_check_dgrad_operands(const char* name, const gsd_src& dy, const gsd_dst& dst, int Cin, int Cout, int H, int W) {
  char what[64];
  snprintf(what, sizeof what, "%s src", name);
  if (int e = gsd_check_src(dy, what)) return e;
  snprintf(what, sizeof what, "%s dst", name);
  if (int e = gsd_check_dst(dst, what)) return e;
  if (int e = convT_check_dy(name, "src", dy, Cout, H, W)) return e;
  GSD_REQUIRE(dst.C == Cin && dst.H == H && dst.W == W && dst.off_h == 0 && dst.off_w == 0, GSD_ERR_BAD_ARG,
              "%s: dst must be the full (Cin,H,W) gradient buffer", name);
  return 0;
}

// ---- planning ----------------------------------------------------------------------------------------------------------------------
// Block tile of the two LDS-DMA kernels (their BM x BN) and the k rows of one chunk (their KC): an operand image of a chunk is
// CT_KC x 128 floats for the weights and for either kernel's activations (the dX kernel's: KC / 2 rows of 2 BN interleaved floats).
constexpr int CT_BM = 128, CT_BN = 128, CT_KC = 32;
constexpr size_t CT_DMA_IMAGES = (size_t)2 * (CT_KC * CT_BM + CT_KC * CT_BN);   // double-buffered: 64 KiB, two blocks per CU

struct ConvTLaunch {
  int grid;
  size_t lds;
  bool wide;   // the register-staged dX kernel only: 64 x 256 blocks (Cin <= 64) instead of 128 x 128
};

static inline int convT_size_launch(const char* name, long grid, size_t lds_floats, ConvTLaunch* L) {
  GSD_REQUIRE(grid < 2147483647L, GSD_ERR_UNSUPPORTED, "%s: grid too large", name);
  L->grid = (int)grid;
  L->lds = lds_floats * sizeof(float);
  return 0;
}

// Forward (ConvTFwdParams): k = ci in chunks of CT_KC channels, m = co*4+kh*2+kw, pixel tiles over the flattened pixels of the whole
// batch; the deferred BatchNorm coefficients of every (padded) input channel ride behind the operand images.
template <class Params>
static inline int convT_plan_fwd(const char* name, Params& P, int Cin, int Cout, int N, int H, int W, ConvTLaunch* L) {
  P.K = Cin;
  P.Kpad = round_up(Cin, CT_KC);
  P.M = Cout * 4;
  P.nchunks = P.Kpad / CT_KC;
  P.mblocks = ceil_div(P.M, CT_BM);
  P.N = N; P.H = H; P.W = W;
  P.tiles_flat = (int)ceil_div64((int64_t)N * H * W, CT_BN);
  if (int e = convT_size_launch(name, (long)P.tiles_flat * P.mblocks, CT_DMA_IMAGES + 2 * P.Kpad, L)) return e;
  GSD_REQUIRE(L->lds <= 80 * 1024, GSD_ERR_UNSUPPORTED, "%s: Cin %d too large for the coefficient table", name, Cin);
  return 0;
}

// dX on the LDS-DMA kernel (ConvTDgParams): k = co*4+kh*2+kw in chunks of CT_KC / 4 output channels, m = ci, pixel tiles over the
// whole batch's virtual grid of round_up(W, 2) columns.  fused: two partial rows per pixel tile, of 2 * Mpad floats each.
static inline int convT_dgrad_tiles(int N, int H, int W) { return (int)ceil_div64((int64_t)N * H * round_up(W, 2), CT_BN); }
template <class Params>
static inline int convT_plan_dgrad(const char* name, Params& P, int Cin, int Cout, int N, int H, int W, bool fused, ConvTLaunch* L) {
  P.K = Cout * 4;
  P.Kpad = round_up(Cout, CT_KC / 4) * 4;
  P.M = Cin;
  P.nchunks = P.Kpad / CT_KC;
  P.mblocks = ceil_div(Cin, CT_BM);
  P.N = N; P.H = H; P.W = W;
  P.Wv = round_up(W, 2);
  P.tiles_flat = convT_dgrad_tiles(N, H, W);
  P.Mpad = fused ? round_up(Cin, 64) : 0;
  return convT_size_launch(name, (long)P.tiles_flat * P.mblocks, CT_DMA_IMAGES, L);
}

// dX on the register-staged kernel (ConvTDgStagedParams): k in chunks of 4 output channels, pixel tiles per image, block tile
// 64 x 256 for Cin <= 64 and 128 x 128 above; LDS rows of 16 k-rows with 16 floats of padding (<= 24 KB).
template <class Params>
static inline int convT_plan_dgrad_staged(const char* name, Params& P, int Cin, int Cout, int N, int H, int W, ConvTLaunch* L) {
  L->wide = Cin <= 64;
  const int BM = L->wide ? 64 : 128, BN = L->wide ? 256 : 128;
  P.K = Cout * 4;
  P.M = Cin;
  P.Mpad = round_up(Cin, 64);
  P.nchunks = ceil_div(Cout, 4);
  P.mblocks = ceil_div(Cin, BM);
  P.N = N; P.H = H; P.W = W;
  P.tiles_flat = ceil_div(H * W, BN);
  return convT_size_launch(name, (long)N * P.tiles_flat * P.mblocks, (size_t)16 * (BM + 16) + 16 * (BN + 16), L);
}
