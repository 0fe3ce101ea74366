// gsd_conv3x3_w2d_strips.hip -- the two-dimensional Winograd conv3x3 (gsd_conv3x3_w2d.hip) over a BAND-MAJOR FLAT TILE LIST, for the
// deep levels of the U-Net.
//
// The rectangular form gives a block a TH x TW rectangle of 32 Winograd tiles of one image, TW a power of two.  At 40 x 53 an image
// is 20 x 14 = 280 tiles and takes 5 x 2 = 10 blocks (320 slots: 12.5 % of the MFMA work is on tiles that hold no pixel), at
// 20 x 26 it is 10 x 7 = 70 tiles in 3 blocks (96 slots: 27 %).  Here the tiles of the whole launch are listed flat (band by band,
// column by column: gsd_conv3x3_w2d_kernel.h) and a block takes the next 32: 280 blocks instead of 320 at 40 x 53 x 32 images, 70
// instead of 96 at 20 x 26.  A tile keeps its anchor, its window, its products and its output transform: outputs are bit-identical
// to the rectangular form's; only which block computes a tile changes.  The BatchNorm partial rows keep their bits as well: the
// epilogue leaves per-tile sums and w2d_strips_rows_kernel adds them in the rectangles' rows and lane order (below).
//
// The price is the window: a group's 16 tiles are 8 columns of a band, 6 window rows of up to 14 pieces where the rectangle has
// 10 rows of 10 for twice as many tiles -- three fill instructions per wave and chunk instead of two (same three MFMA gaps), and
// 10.5 KiB per chunk image instead of 6.3 (two blocks per CU still fit: the form keeps no affine table).  The chunk loop, the
// transforms, the MFMA schedule and the epilogue are the shared code of gsd_conv3x3_w2d_kernel.h.
//
// Which launches: one plain, row-pitched, 16-byte aligned source (the class of every dX launch and of the "activate once"
// forwards), unsplit, where the list has fewer blocks than plan_w2d's grid, no group has more than three strips or 14 pieces a row,
// and the tensor fits the lanes' unsigned 32-bit byte offsets.  GSD_W2D_STRIPS: 0 never, 1 wherever admitted; unset: where the
// launcher's run-time model has the shorter list finish sooner at 3 % more per chunk (w2d_strips_take, gsd_conv3x3_w2d.hip).
#include "gsd_conv3x3_w2d_kernel.h"

__global__ __launch_bounds__(128 * NWP, 2) void conv3x3_w2d_strips_kernel(const W2DParams P, const W2DStrips SP) {
  w2d_block<true, 1, false, true>(P, SP);
}

// The statistics of a strips launch, in the rectangular form's bits.  The conv kernel left the sums of every TILE (one lane's 2 x 4
// pixels, added in the epilogue's order: the same value whichever block computed the tile).  The rectangular form adds the 16
// tiles of a pixel group with reduce16_to_lane15, lane q = tile (q / TWq, q % TWq) of the group's rectangle, empty slots 0.  Here 16
// lanes take the same tiles in the same places and run the same reduction: partial row (rectangle, group) gets the bits
// conv3x3_w2d_kernel writes, so the batch statistics -- and a train step -- do not depend on which form ran.
// Block = 16 channels x 16 lanes of one partial row; grid (Mpad / 16, rows).
__global__ __launch_bounds__(256) void w2d_strips_rows_kernel(const W2DParams P, const W2DStrips SP) {
  const int l16 = threadIdx.x & 15, co = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int r = blockIdx.y, pt = r / NWP, ph = r - pt * NWP;
  const int tpi_r = P.tiles_y * P.tiles_x;
  const int n = pt / tpi_r, rt = pt - n * tpi_r;
  const int by = rt / P.tiles_x, bx = rt - by * P.tiles_x;
  const int q = ph * 16 + l16;
  float s1 = 0.f, s2 = 0.f;
  if (q < (P.TH >> 1) * P.TWq) {
    const int tr2 = q >> P.TWq_sh, tq = q - tr2 * P.TWq;
    const int ty = by * (P.TH >> 1) + tr2, tx = bx * P.TWq + tq;
    if (ty < SP.TY && tx < SP.TX) {
      const int band = ty >> 1, two = 2 * band + 1 < SP.TY ? 1 : 0;
      const size_t t = (size_t)n * SP.TY * SP.TX + (size_t)band * (2 * SP.TX) + (two ? 2 * tx + (ty & 1) : tx);
      const float* tp = P.partials + t * (2 * P.Mpad) + co;
      s1 = tp[0];
      s2 = tp[P.Mpad];
    }
  }
  s1 = reduce16_to_lane15(s1);
  s2 = reduce16_to_lane15(s2);
  if (l16 == 15) {
    SP.rows[(size_t)r * (2 * P.Mpad) + co] = s1;
    SP.rows[(size_t)r * (2 * P.Mpad) + P.Mpad + co] = s2;
  }
}

static int w2d_strips_plane_stride(int N, const W2DStripPlan& pl);

// The list of an (N, H, W) launch: tiles per image, blocks, the most strips / pieces per window row any group has, and (where the
// kernel admits the list) the plane stride.  Walking the groups and searching the stride is a fraction of a millisecond of HOST
// time: done once per shape and remembered -- an idempotent cache like plan_w2d's, key and payload in ONE 64-bit atomic (every
// thread computes the same value; a reader never sees one entry's key with another's payload).
bool w2d_strips_plan(int N, int H, int W, W2DStripPlan* p) {
  p->TY = ceil_div(H, 2);
  p->TX = ceil_div(W, 4);
  const int64_t nt = (int64_t)N * p->TY * p->TX;
  p->max_strips = p->max_pieces = 0;
  p->PS = 0;
  p->nblocks = (int)ceil_div64(nt, 32);
  if (nt >= (1LL << 30)) return false;
  static std::atomic<uint64_t> memo[16];
  const bool keyed = N < (1 << 14) && H < (1 << 14) && W < (1 << 14);
  const uint64_t key = ((uint64_t)N << 28) | ((uint64_t)H << 14) | (uint64_t)W;   // 42 bits; payload: strips 5, pieces 7, PS / 4 10
  std::atomic<uint64_t>& mm = memo[(N * 7 + H * 3 + W) & 15];
  if (keyed) {
    const uint64_t v = mm.load(std::memory_order_acquire);
    if (v != 0 && (v >> 22) == key) {
      p->max_strips = (int)(v >> 17) & 31;
      p->max_pieces = (int)(v >> 10) & 127;
      p->PS = ((int)v & 1023) * 4;
      return p->max_strips <= W2D_STRIPS && p->max_pieces <= W2D_STRIP_NP;
    }
  }
  // a group's shape depends on its offset inside an image: the first TY TX groups show every one (and the list's end only cuts one short)
  const int64_t groups = std::min<int64_t>(ceil_div64(nt, 16), (int64_t)p->TY * p->TX + 1);
  for (int g = 0; g < (int)groups; ++g) {
    W2DStrip st[16];
    const int k = w2d_group_strips(g, N, p->TY, p->TX, st);
    p->max_strips = std::max(p->max_strips, k);
    if (k <= 16) p->max_pieces = std::max(p->max_pieces, st[k - 1].s0 + st[k - 1].c + 2);
  }
  const bool ok = p->max_strips <= W2D_STRIPS && p->max_pieces <= W2D_STRIP_NP;
  if (ok) p->PS = w2d_strips_plane_stride(N, *p);
  if (keyed && p->max_pieces < 128 && p->PS < 4096)
    mm.store((key << 22) | ((uint64_t)p->max_strips << 17) | ((uint64_t)p->max_pieces << 10) | (uint64_t)(p->PS / 4), std::memory_order_release);
  return ok;
}

// Plane stride of the strips windows (row pitch 56 floats, groups 336 apart) with the fewest bank conflicts of the consumers' reads,
// over the groups of the first image
static int w2d_strips_plane_stride(int N, const W2DStripPlan& pl) {
  const int WCp = 4 * W2D_STRIP_NP, GS = 6 * WCp;
  const int nt = N * pl.TY * pl.TX, blocks = std::min(pl.nblocks, std::max(1, ceil_div(pl.TY * pl.TX, 32)));
  int best = -1, ps_best = 2 * GS + 4;
  for (int ps = 2 * GS + 4; ps < 2 * GS + 4 + 68; ps += 4) {
    int cyc = 0;
    for (int b = 0; b < blocks; ++b)
      for (int gg = 0; gg < 2; ++gg) {
        W2DStrip st[W2D_STRIPS];
        w2d_group_strips(2 * b + gg, N, pl.TY, pl.TX, st);
        int addr[64];
        for (int lane = 0; lane < 64; ++lane) {
          const W2DTile t = w2d_tile_of(32 * b + 16 * gg + (lane & 15), N, pl.TY, pl.TX, st);
          addr[lane] = (lane >> 4) * ps + gg * GS + (t.n < 0 || 32 * b + 16 * gg + (lane & 15) >= nt ? 0 : 2 * (t.ty & 1) * WCp + 4 * t.piece);
        }
        cyc += conv3_read_cycles(addr);
      }
    if (best < 0 || cyc < best) {
      best = cyc;
      ps_best = ps;
    }
  }
  return ps_best;
}

// P: the rectangular launch's parameters, complete (w2d_impl)
// scratch: w2d_strips_scratch_elems floats where the launch has partial rows
int w2d_strips_launch(W2DParams P, const W2DStripPlan& pl, const gsd_dst* dst, int ndst, float* scratch, hipStream_t st) {
  W2DStrips SP;
  SP.TY = pl.TY; SP.TX = pl.TX;
  SP.GS = 6 * 4 * W2D_STRIP_NP;
  SP.nblocks = pl.nblocks;
  SP.prows = P.ptiles * NWP;
  SP.rows = P.partials;
  if (P.partials != nullptr) P.partials = scratch;
  P.ptiles = pl.nblocks;
  P.WCp = 4 * W2D_STRIP_NP;
  P.PS = pl.PS;
  P.nslab = 1;
  P.slabs = nullptr;
  // the interior epilogue's lane offsets now span the images as well
  P.dfast = 0;
  for (int i = 0; i < ndst; ++i)
    if (4 * ((int64_t)P.N * dst[i].n_stride + 12 * (int64_t)dst[i].c_stride + (int64_t)dst[i].H * dst[i].w_stride) < (1LL << 32)) P.dfast |= 1 << i;
  const size_t lds = (size_t)(2 * (W2D_WTILE + 4 * P.PS) + 4 * W2D_BM) * sizeof(float);
  const long grid = (long)pl.nblocks * P.mblocks;
  GSD_REQUIRE(grid < 2147483647L, GSD_ERR_UNSUPPORTED, "gsd_conv3x3_w2d: grid too large");
  if (gsd_env_set("GSD_W2D_TRACE"))
    fprintf(stderr, "w2d strips M%d K%d %dx%d N%d blocks %d (rect %d) strips<=%d pieces<=%d PS %d dfast %d\n", P.Cout, P.Cin, P.H, P.W, P.N,
            pl.nblocks, SP.prows / NWP, pl.max_strips, pl.max_pieces, P.PS, P.dfast);
  if (int e = gsd_launch<conv3x3_w2d_strips_kernel>("gsd_conv3x3_w2d (strips)", dim3((unsigned)grid), dim3(128 * NWP), lds, st, P, SP)) return e;
  if (SP.rows != nullptr) {
    GSD_REQUIRE(SP.prows <= 65535, GSD_ERR_UNSUPPORTED, "gsd_conv3x3_w2d (strips): too many partial rows");
    hipLaunchKernelGGL(w2d_strips_rows_kernel, dim3(P.Mpad / 16, SP.prows), dim3(256), 0, st, P, SP);
    GSD_LAUNCH_CHECK("gsd_conv3x3_w2d (strip rows)");
  }
  return GSD_OK;
}

// ---- host mirrors of the listing, for tests: the code the kernel runs (w2d_group_strips / w2d_tile_of) ---------------------------
// Lane (t & 15) of pixel group t >> 4: out[0..4] = image (-1: past the end of the list, an empty lane), tile row, tile column, strip
// of the group, first piece of the tile's window in the group's window rows.
extern "C" int gsd_conv3x3_w2d_strips_tile(int N, int H, int W, int t, int* out) {
  if (N <= 0 || H <= 0 || W <= 0 || t < 0 || out == nullptr) return GSD_ERR_BAD_ARG;
  const int TY = ceil_div(H, 2), TX = ceil_div(W, 4);
  W2DStrip st[16];
  w2d_group_strips(t >> 4, N, TY, TX, st);
  const W2DTile r = w2d_tile_of(t, N, TY, TX, st);
  out[0] = r.n; out[1] = r.ty; out[2] = r.tx; out[3] = r.strip; out[4] = r.piece;
  return 0;
}
