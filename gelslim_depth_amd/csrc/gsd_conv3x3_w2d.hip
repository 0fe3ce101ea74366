// gsd_conv3x3_w2d.hip -- conv3x3 (pad 1, stride 1, no bias) forward and dX with the TWO-dimensional Winograd minimal-filtering
// identity F(2 x 4, 3 x 3) on v_mfma_f32_16x16x4_f32 (gfx950): F(4,3) along the image rows (as gsd_conv3x3_w43.hip) combined
// with F(2,3) down the columns.
//
// Same operator as gsd_conv3x3.hip / gsd_conv3x3_w43.hip (aten::convolution at /root/reference/gelslim_depth/models/unet.py:11,14
// and the dX half of aten::convolution_backward), same fp32 storage and fp32 accumulation.  A tile of 2 x 4 outputs of one
// channel needs a 4 x 6 input window and, per input channel, 4 x 6 = 24 products instead of 2 * 4 * 9 = 72:
//
//   Y (2x4) = A2^T [ (G2 g G4^T) .* (B2^T d B4) ] A4,     d = the 4 x 6 window, g = the 3 x 3 kernel
//
// a third of the direct form's multiplications and two thirds of the row-only form's (36 per 2 x 4 outputs).  The contraction
// over the input channels stays on the MFMA: 24 GEMMs M_f[m][tile] = sum_ci U_f[ci][m] * V_f[ci][tile], f = (fr, fc).
// F(2,3) is the mildest Winograd transform there is (constants 1 and 1/2): the op-level tests bound the combined form at the same
// 1e-5 relative L1 against the fp64 oracle as the row-only form (north-star tolerance: 1e-3).
//
// Block = 4 waves on a 64-channel x 256-pixel tile, as the row-only kernel, but the waves split it 2 (frequency-row halves) x 2 (pixel
// halves): a wave owns all 64 output channels x 16 tiles (128 pixels) x 12 of the 24 frequencies = 4 MFMA m-tiles x 12 = 192
// accumulator registers (all 24 would need 384), two blocks per CU.  Per 4-channel chunk a wave issues 12 frequencies x 4 MFMAs = 48
// MFMAs for 128 pixels where the row-only kernel issues 72 for 64, and transforms only the 18 window values and the two frequency
// rows its MFMAs use (the channel-half split computed all 24 and four rows in both waves of a pixel group, and fed each V value to
// two MFMAs instead of four).  The two halves of a pixel group trade accumulators once, after the chunk loop.  The weight image of a chunk is 96 x 64 floats = 24 KiB (U = G2 g G4^T,
// laid out once per optimiser step by gsd_weight_layout modes 8 / 9); the (TH + 2) x (TW + 2) halo window, the LDS-DMA fills, the
// deferred BatchNorm + ReLU of the sources (NaN-sentinel padding), the two source segments (concat), the two cropped destinations,
// the BatchNorm partial sums and the fused BatchNorm-backward dX epilogue are those of gsd_conv3x3_w43.hip (its straight-fill
// form: every 4-channel chunk lies inside one source segment -- always true in the U-Net).
//
// What sets this kernel's rate is its vector-to-MFMA instruction ratio (an fp32 MFMA stream hides LDS reads and scalar instructions
// but not vector instructions: profiles/r05_mfma_f32_issue_ubench.txt), hence: the operand transform, the deferred-BatchNorm affine
// and the output transform on PAIRS of floats (packed fp32 instructions, bit-identical to the scalar form); the chunk loop unrolled
// by two so that the LDS image offsets are instruction immediates; 16-byte halo pieces wherever the source admits them (HM);
// plane offsets of the epilogue as scalar arithmetic.  K slabs (SPLIT) for the launches that would leave the chip idle.
// The loop's BOOKKEEPING runs on the scalar unit: fills address a wave-uniform base plus an unsigned 32-bit lane offset under an
// exec mask held in a scalar register pair, and wave-uniform conditions are scalar integers, not bools (hipcc carries a uniform
// bool that crosses a block boundary through a vector register).  The kernel lives at 256 registers: state the loop does not need
// waits in LDS or packed in one register, and tests/test_w2d_isa.py holds every instantiation to zero scratch and the loop to its
// vector-instruction count (profiles/r07_w2d_isa_counts.txt).
// WHERE the loop's vector work sits counts for more than how much there is: every MFMA-to-MFMA gap that carries a vector
// instruction or a fill costs cycles of its own, in both waves of a SIMD one after the other.  A chunk has three such gaps under
// its MFMAs (weight fills; a halo fill; a halo fill + the second frequency row's transform) and the barrier's; the plain forms keep their LDS
// addresses of both images in registers, so the loop's vector instructions are the transforms' arithmetic and nothing else;
// the accumulators are zeroed by LDS reads (tests/test_w2d_gaps.py, profiles/w2d_gaps_isa_counts.txt).
#include "gsd_conv3x3_host.h"

#include "gsd_conv3x3_w2d_kernel.h"   // the device code: parameters, epilogue, the block body (shared with the strips form)

// The rectangular form: block = one TH x TW pixel tile of one image (plan_w2d below)
template <bool PLAIN, int HM = 0, bool SPLIT = false>
__global__ __launch_bounds__(128 * NWP, 2) void conv3x3_w2d_kernel(const W2DParams P) {
  w2d_block<PLAIN, HM, SPLIT, false>(P, W2DStrips{});
}

// The second half of a K-slab launch: one block per (pixel tile, m-block) with the conv kernel's thread -> (tile, channel) map adds
// the slabs IN SLAB ORDER (run-to-run bitwise) and runs the conv kernel's epilogue on the sums.
__global__ __launch_bounds__(128 * NWP) void w2d_slab_reduce_kernel(const W2DParams P) {
  constexpr int BM = W2D_BM;
  __shared__ float sBw[4 * BM];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave8 = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ph = wave8 % NWP, mh = wave8 / NWP;
  const int j = lane >> 4, l16 = lane & 15;
  const int lid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int pt = w2d_div(lid, P.d_mblocks);
  const int mbb = lid - pt * P.mblocks;
  const int m0 = mbb * BM;
  const int tpi = P.tiles_y * P.tiles_x;
  const int n = w2d_div(pt, P.d_tpi);
  const int rt = pt - n * tpi;
  const int ty = w2d_div(rt, P.d_tiles_x);
  const int h0 = ty * P.TH, w0 = (rt - ty * P.tiles_x) * P.TW;
  const int q = ph * 16 + l16;
  const bool q_ok = q < (P.TH >> 1) * P.TWq && q < 16 * NWP;
  const int tr2 = q_ok ? q >> P.TWq_sh : 0;
  const int tq = q_ok ? q - tr2 * P.TWq : 0;
  int vmask = 0;
  if (q_ok) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
      if (h0 + 2 * tr2 + a < P.H) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (w0 + 4 * tq + i < P.W) vmask |= 1 << (4 * a + i);
      }
  }
  if (P.bw_raw != nullptr) {
    for (int c = tid; c < BM; c += 128 * NWP) {
      const int co = m0 + c < P.Cout ? m0 + c : 0;
      sBw[c] = P.bw_scale[co];
      sBw[BM + c] = P.bw_shift[co];
      sBw[2 * BM + c] = P.bw_mean[co];
      sBw[3 * BM + c] = P.bw_invstd[co];
    }
    __syncthreads();
  }
  const size_t tile_elems = (size_t)(BM * 128 * NWP);
  const float* const s0 = P.slabs + ((size_t)pt * P.nslab * P.mblocks + mbb) * tile_elems;
  auto get_pair = [&](const int p, float (&y)[2][2][4]) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const float* o = s0 + ((size_t)(mh * 32 + (p >> 1) * 16 + j * 4 + (p & 1) * 2 + e) * (16 * NWP) + q) * 8;
      f32x4 a = *reinterpret_cast<const f32x4*>(o), b = *reinterpret_cast<const f32x4*>(o + 4);
      for (int s = 1; s < P.nslab; ++s) {
        o += (size_t)P.mblocks * tile_elems;
        a += *reinterpret_cast<const f32x4*>(o);
        b += *reinterpret_cast<const f32x4*>(o + 4);
      }
      y[e][0][0] = a[0], y[e][0][1] = a[1], y[e][0][2] = a[2], y[e][0][3] = a[3];
      y[e][1][0] = b[0], y[e][1][1] = b[1], y[e][1][2] = b[2], y[e][1][3] = b[3];
    }
  };
  w2d_epilogue(P, sBw, n, h0, w0, tr2, tq, vmask, m0, mh, ph, j, l16, pt, get_pair);
}

// -------------------------------------------------------------------------------------------------
// host side
// -------------------------------------------------------------------------------------------------
namespace {

struct W2DPlan {
  int TH, TW, TWq, tiles_y, tiles_x, mblocks, WR, WC, WCp, PS;
};

// TH x TW output tile of 16 NWP two-row Winograd tiles (256 pixels) whose padded halo window fits the 128 NW DMA positions:
// fewest blocks; among equals 32-wide rows, then the widest.  The LDS row pitch and plane stride are the ones with the fewest
// bank conflicts.
bool plan_w2d(int N, int H, int W, int M, W2DPlan* best) {
  long best_cost = -1;
  const int force_tw = gsd_env_int("GSD_W2D_TW", 0);   // tuning
  const int maxpos = 256 * NWP;
  static const int tws[4] = {32, 64, 16, 8};
  for (int k = 0; k < 4; ++k) {
    const int tw = tws[k];
    if (force_tw && tw != force_tw) continue;
    const int twq = tw / 4;
    int th = 2 * (16 * NWP / twq);
    const int wcp0 = round_up(tw + 2, 4);
    if ((th + 2) * wcp0 > maxpos) continue;
    const int ty = ceil_div(H, th);
    th = round_up(ceil_div(H, ty), 2);
    const long blocks = (long)ty * ceil_div(W, tw) * N;
    // 8-pixel rows (32 x 8 tiles) save a few blocks on 213-pixel rows (135 against 140 per image) but their halo is 34 rows of 40
    // bytes -- and too many pieces for the 16-byte fills: they have to save GSD_W2D_TW8_PCT percent (default 8) to be taken
    // (measured: step 97.35 -> 96.66 ms; 8 x 32 instead of 16 x 16 tiles at 320 x 427, 560 against 540 per image: +0.2 ms, not taken)
    const long cost = (blocks * 8 + (tw == 32 ? 0 : tw == 64 ? 1 : tw == 16 ? 2 : 3)) * (tw == 8 ? 100 + gsd_env_int("GSD_W2D_TW8_PCT", 8) : 100);
    if (best_cost < 0 || cost < best_cost) {
      best_cost = cost;
      best->TH = th; best->TW = tw; best->TWq = twq;
      best->tiles_y = ty; best->tiles_x = ceil_div(W, tw);
      best->WR = th + 2; best->WC = tw + 2;
    }
  }
  best->mblocks = ceil_div(M, W2D_BM);
  if (best_cost < 0) return false;
  // LDS row pitch and plane stride of the chosen tile: a search over 36 candidates of ~10^5 operations each, i.e. a fraction of a
  // millisecond of HOST time -- per (tile, block form) it is done once and remembered (an idempotent cache like cu_count(): every
  // thread computes the same value, the key is published last)
  // (key, WCp, PS) travel in ONE 64-bit atomic: a reader never sees the key of one entry with the payload of another (with the key
  //  and the payload in separate words two writers of colliding keys could hand a reader a torn pair, and the LDS size would then
  //  be computed from another PS than the kernel's)
  static std::atomic<uint64_t> memo[16];
  const int th = best->TH, tw = best->TW, key = (th << 16) | (tw << 4);
  std::atomic<uint64_t>& mm = memo[(th * 7 + tw) & 15];
  {
    const uint64_t v = mm.load(std::memory_order_acquire);
    if (v != 0 && (int)(v >> 40) == key) {
      best->WCp = (int)(v >> 20) & 0xFFFFF;
      best->PS = (int)v & 0xFFFFF;
      return true;
    }
  }
  const int wcp0 = round_up(tw + 2, 4);
  int bc = -1;
  for (int c = wcp0; c <= wcp0 + 12 && (th + 2) * c <= maxpos; c += 4)
    for (int ps = round_up((th + 2) * c, 4) + 4; ps < round_up((th + 2) * c, 4) + 4 + 36; ps += 4) {
      const int cyc = conv3_halo_read_cycles(NWP, 2, best->TWq, c, ps, 0);
      if (bc < 0 || cyc < bc) {
        bc = cyc;
        best->WCp = c;
        best->PS = ps;
      }
    }
  if (key < (1 << 24) && best->WCp < (1 << 20) && best->PS < (1 << 20))
    mm.store(((uint64_t)key << 40) | ((uint64_t)best->WCp << 20) | (uint64_t)best->PS, std::memory_order_release);
  return true;
}

// X4: plane stride of the shifted planes (row pitch 4 NP floats) with the fewest bank conflicts of the consumers' reads
int w2d_x4_plane_stride(int TWq, int WCp, int WR) {
  static std::atomic<uint64_t> memo[8];   // (key, PS) in one 64-bit atomic, as in plan_w2d
  const int key = (TWq << 20) | (WCp << 8) | WR;
  std::atomic<uint64_t>& mm = memo[(TWq + WR) & 7];
  {
    const uint64_t v = mm.load(std::memory_order_acquire);
    if (v != 0 && (int)(v >> 32) == key) return (int)(v & 0xFFFFFFFFu);
  }
  int best = -1, ps_best = WR * WCp + 4;
  for (int ps = WR * WCp + 4; ps < WR * WCp + 4 + 68; ps += 4) {
    const int c = conv3_halo_read_cycles(NWP, 2, TWq, WCp, ps, 0);
    if (best < 0 || c < best) {
      best = c;
      ps_best = ps;
    }
  }
  mm.store(((uint64_t)(unsigned)key << 32) | (uint64_t)(unsigned)ps_best, std::memory_order_release);
  return ps_best;
}

template <bool PLAIN, int HM = 0, bool SPLIT = false>
int launch_w2d(const W2DParams& P, int grid, size_t lds, hipStream_t st) {
  if (int e = gsd_launch<conv3x3_w2d_kernel<PLAIN, HM, SPLIT>>("gsd_conv3x3_w2d", dim3(grid), dim3(128 * NWP), lds, st, P)) return e;
  if constexpr (SPLIT) {
    hipLaunchKernelGGL(w2d_slab_reduce_kernel, dim3(grid / P.nslab), dim3(128 * NWP), 0, st, P);
    GSD_LAUNCH_CHECK("gsd_conv3x3_w2d (slab sums)");
  }
  return GSD_OK;
}

// The K-slab model (gsd_conv3x3_host.h) at this kernel's own rate: pairs of blocks at 2.07 us per chunk and block (+ 5 us per
// block), an odd last block at 0.66 of that (the per-block cost and the lone-block factor fitted to profiles/r05_w2d_vs_w43.txt:
// the 20 x 26 and 40 x 53 layers at batch 8, where k is 1-3); the slab sums cost what the row form's do.  GSD_W2D_SPLIT: 0 / 1
// never, S >= 2 that many slabs (tuning).
constexpr Conv3SlabModel w2d_slabs = {2.07, 5.0, 0.66, "GSD_W2D_SPLIT"};

// 1: an unsplit <plain, aligned pieces> launch of this shape runs the band-major strip list (gsd_conv3x3_w2d_strips.hip) instead of
// the rect_ptiles rectangles of plan_w2d.  GSD_W2D_STRIPS = 0: never; 1: wherever the kernel admits the list and it has fewer
// blocks.  Unset: where, besides, the run-time model has it finish sooner at W2D_STRIPS_CHUNK_COST times the rectangles' time per
// chunk.  The list's windows are larger (three fill units per wave and chunk instead of two, 10.5 KiB instead of 6.3): where the
// shorter list needs as many rounds of the chip's block slots as the rectangles it measured 4 % SLOWER (40 x 53 512 -> 256 at batch
// 32: 1280 against 1120 blocks, 536 -> 559 us; 512 -> 1024 at batch 8), where it saves a round 4 to 13 % faster
// (profiles/w2d_strips_layers_b32.txt) -- what the model's whole blocks per CU tell apart.  Measured at the two deep levels only
// (280 and 70 tiles an image): images of more than W2D_STRIPS_MAX_TILES tiles keep the rectangles unless the switch is 1.
constexpr double W2D_STRIPS_CHUNK_COST = 1.03;
constexpr int W2D_STRIPS_MAX_TILES = 512;
int w2d_strips_take(int N, int H, int W, long rect_ptiles, int mblocks, int nchunks, W2DStripPlan* p) {
  const int sw = gsd_env_int("GSD_W2D_STRIPS", -1);
  if (sw == 0) return 0;
  const int64_t nb = ceil_div64((int64_t)N * ceil_div(H, 2) * ceil_div(W, 4), 32);
  if (nb >= rect_ptiles) return 0;
  if (sw != 1 && ceil_div(H, 2) * ceil_div(W, 4) > W2D_STRIPS_MAX_TILES) return 0;
  if (sw != 1 && W2D_STRIPS_CHUNK_COST * w2d_slabs.time_us(nb * mblocks, nchunks, 1, false) >= w2d_slabs.time_us(rect_ptiles * mblocks, nchunks, 1, false))
    return 0;
  return w2d_strips_plan(N, H, W, p) ? 1 : 0;
}

// Pixel-tile blocks of an UNSPLIT launch of the class the deep levels run in train mode -- one plain, row-pitched, aligned source
// (every dX launch, the "activate once" forwards): the strip list's where the launcher takes it (w2d_impl), else the rectangles'
long w2d_plain_ptiles(int N, int H, int W, int nchunks, const W2DPlan& p) {
  const long rect = (long)N * p.tiles_y * p.tiles_x;
  if (4 * ceil_div(p.WR * (p.TW / 4 + 2), 64) > 8 || gsd_env_int("GSD_W2D_X4", 1) == 0) return rect;
  W2DStripPlan sp;
  return w2d_strips_take(N, H, W, rect, p.mblocks, nchunks, &sp) ? sp.nblocks : rect;
}

}  // namespace

// 1: the shape and its operands fit the two-dimensional form (every 4-channel chunk inside one source segment)
extern "C" int gsd_conv3x3_w2d_supported(int Cin, int C0) {
  return (Cin > 0 && Cin % 4 == 0 && C0 > 0 && C0 <= Cin && C0 % 4 == 0) ? 1 : 0;
}

extern "C" int gsd_conv3x3_w2d_partial_rows(int N, int H, int W, int Cout) {
  if (N <= 0 || H <= 0 || W <= 0 || Cout <= 0) return 0;
  W2DPlan p;
  if (!plan_w2d(N, H, W, Cout, &p)) return 0;
  return N * p.tiles_y * p.tiles_x * NWP;
}

// MFMA instructions of one launch (all blocks, padding included)
extern "C" int64_t gsd_conv3x3_w2d_mfma_count(int N, int H, int W, int Cin, int Cout) {
  W2DPlan p;
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || !plan_w2d(N, H, W, Cout, &p)) return 0;
  return (int64_t)N * p.tiles_y * p.tiles_x * p.mblocks * ceil_div(Cin, 4) * (2 * NWP * 48);
}

// MFMA instructions the launch ISSUES, given its source class (gsd_conv3x3_w2d_source_class) and whether the caller lends K-slab
// scratch: an unsplit class-1 launch runs the strip list where the launcher takes it, with fewer blocks than the rectangles
extern "C" int64_t gsd_conv3x3_w2d_mfma_count_class(int N, int H, int W, int Cin, int Cout, int source_class, int with_workspace) {
  W2DPlan p;
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || !plan_w2d(N, H, W, Cout, &p)) return 0;
  long pt = (long)N * p.tiles_y * p.tiles_x;
  const bool cut = with_workspace && Cin % 4 == 0 && w2d_slabs.pick(pt * p.mblocks, Cin / 4, false) > 1;
  if (source_class == 1 && !cut) pt = w2d_plain_ptiles(N, H, W, ceil_div(Cin, 4), p);
  return (int64_t)pt * p.mblocks * ceil_div(Cin, 4) * (2 * NWP * 48);
}

// The strip listing of an (N, H, W) launch Cin -> Cout, for tests and tools.  out[0..6] = blocks of the list, most strips of a
// group, most pieces of a window row, pieces of a block's chunk image (2 groups x 6 rows x 4 planes x the row's pieces), blocks of
// the rectangular grid, 1 if the kernel admits the list and it has fewer blocks (GSD_W2D_STRIPS aside), 1 if an unsplit class-1
// launch takes it as the environment stands.  Returns 0, or < 0 on bad sizes.
extern "C" int gsd_conv3x3_w2d_strips_plan(int N, int H, int W, int Cin, int Cout, int* out) {
  W2DPlan r;
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || out == nullptr || !plan_w2d(N, H, W, Cout, &r)) return GSD_ERR_BAD_ARG;
  W2DStripPlan p, q;
  const bool ok = w2d_strips_plan(N, H, W, &p);
  const int rect = N * r.tiles_y * r.tiles_x;
  out[0] = p.nblocks; out[1] = p.max_strips; out[2] = p.max_pieces;
  out[3] = 2 * 6 * 4 * p.max_pieces;
  out[4] = rect;
  out[5] = ok && p.nblocks < rect ? 1 : 0;
  out[6] = w2d_strips_take(N, H, W, rect, r.mblocks, ceil_div(Cin, 4), &q);
  return 0;
}

// Floats of scratch with which a train-mode class-1 launch of the shape runs the strip list AND writes partial rows (0: it keeps
// the rectangles, or is cut into K slabs): the caller's K-slab scratch serves, at least this large
extern "C" int64_t gsd_conv3x3_w2d_strips_scratch(int N, int H, int W, int Cin, int Cout) {
  W2DPlan r;
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || Cin % 4 != 0 || !plan_w2d(N, H, W, Cout, &r)) return 0;
  const long pt = (long)N * r.tiles_y * r.tiles_x;
  if (w2d_slabs.pick(pt * r.mblocks, Cin / 4, false) > 1 || w2d_slabs.pick(pt * r.mblocks, Cin / 4, true) > 1) return 0;
  if (4 * ceil_div(r.WR * (r.TW / 4 + 2), 64) > 8 || gsd_env_int("GSD_W2D_X4", 1) == 0) return 0;
  W2DStripPlan sp;
  return w2d_strips_take(N, H, W, pt, r.mblocks, Cin / 4, &sp) ? w2d_strips_scratch_elems(sp, round_up(Cout, 64)) : 0;
}

// 1: one plain source whose rows start 16-byte aligned on a pitch that is a multiple of 4 floats -- the class that moves its halo as
// aligned 16-byte pieces (and runs the strip list at the deep levels); 0: every other source
extern "C" int gsd_conv3x3_w2d_source_class(const gsd_src* src, int nsrc) {
  if (src == nullptr || nsrc != 1 || src[0].scale != nullptr || src[0].relu != 0) return 0;
  return (((uintptr_t)src[0].ptr & 15) == 0 && src[0].w_stride % 4 == 0 && src[0].c_stride % 4 == 0 && src[0].n_stride % 4 == 0 &&
          src[0].off_h == 0 && src[0].off_w == 0 && src[0].w_stride >= round_up(src[0].W, 4)) ? 1 : 0;
}

// Modelled run time of the launch in microseconds, as gsd_conv3x3_w43_estimate_us (the block count of the path a train-mode
// launch of the shape runs: w2d_plain_ptiles)
extern "C" double gsd_conv3x3_w2d_estimate_us(int N, int H, int W, int Cin, int Cout) {
  W2DPlan p;
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || !plan_w2d(N, H, W, Cout, &p)) return 0.0;
  const long blocks = w2d_plain_ptiles(N, H, W, ceil_div(Cin, 4), p) * p.mblocks;
  return w2d_slabs.time_us(blocks, ceil_div(Cin, 4), 1, false);
}

// ... with the K-slab form where it pays (train mode with a workspace: what the engine's launches run)
extern "C" double gsd_conv3x3_w2d_estimate_slabs_us(int N, int H, int W, int Cin, int Cout) {
  W2DPlan p;
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || !plan_w2d(N, H, W, Cout, &p)) return 0.0;
  const long blocks = (long)N * p.tiles_y * p.tiles_x * p.mblocks;
  const int S = w2d_slabs.pick(blocks, ceil_div(Cin, 4), false);
  if (S == 1) return w2d_slabs.time_us(w2d_plain_ptiles(N, H, W, ceil_div(Cin, 4), p) * p.mblocks, ceil_div(Cin, 4), 1, false);   // (a cut launch keeps the rectangles)
  return w2d_slabs.time_us(blocks, ceil_div(Cin, 4), S, false);
}

// Floats of K-slab scratch a train-mode launch of this shape wants (0: it runs unsplit); the launcher takes the capacity and
// shrinks S to what fits.
extern "C" int64_t gsd_conv3x3_w2d_workspace(int N, int H, int W, int Cin, int Cout) {
  W2DPlan p;
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || Cin % 4 != 0 || !plan_w2d(N, H, W, Cout, &p)) return 0;
  const long blocks = (long)N * p.tiles_y * p.tiles_x * p.mblocks;
  const int S = std::max(w2d_slabs.pick(blocks, Cin / 4, false), w2d_slabs.pick(blocks, Cin / 4, true));
  return S > 1 ? (int64_t)blocks * S * (W2D_BM * 256) : 0;
}

// 1: a caller that has both forms' weight layouts at hand should run this launch through gsd_conv3x3_w2d instead of
// gsd_conv3x3_w43.  train == 0 (eval-mode inference): always -- the two-dimensional form neither folds rows across images nor
// cuts K slabs, so image i of a batch gets the bits the image alone gets, whatever the batch.  train != 0: the modelled times
// decide (the deep levels at small batches stay with the row form's K slabs).  GSD_CONV_W2D = 0 never, 1 always.
extern "C" int gsd_conv3x3_prefers_w2d(int N, int H, int W, int Cin, int Cout, int train) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin < 16 || Cin % 4 != 0 || Cout <= 0) return 0;
  const int forced = gsd_env_int("GSD_CONV_W2D", -1);
  if (forced == 0 || forced == 1) return forced;
  if (!train) return 1;
  const double a = gsd_conv3x3_w2d_estimate_slabs_us(N, H, W, Cin, Cout), b = gsd_conv3x3_w43_estimate_us(N, H, W, Cin, Cout, 1);
  return a > 0.0 && b > 0.0 && a < b ? 1 : 0;
}

// Activate-once query (ActOnceModel, gsd_conv3x3_host.h): 1 when writing relu(bn(.)) of an (N, Cact, H, W) tensor once, row-pitched,
// pays for its train-mode conv3x3 consumer Cin -> Cout (Cact of its Cin input channels are that tensor's).  0 when that consumer is not the two-dimensional form (small batches and
// the row form, channel counts), when it reads the tensor at a pad offset, or when its tile's halo has too many 16-byte pieces for
// the aligned fills (the `x4` condition of w2d_impl).  GSD_ACT_ONCE_FORCE = 0 / 1 overrides the model where the launch admits it.
constexpr ActOnceModel act_once = {0.15, 0.06, 0.33, 0.07, 0.055, 0.28, 6.3e6, 4.0};
extern "C" int gsd_act_once_pays(int N, int H, int W, int Cact, int Cin, int Cout, int off_h, int off_w, int pass_kind) {
  if (N <= 0 || H <= 0 || W <= 0 || Cact <= 0 || Cin < Cact || Cout <= 0 || off_h != 0 || off_w != 0) return 0;
  if (!gsd_conv3x3_w2d_supported(Cin, Cact) || gsd_conv3x3_algo(N, H, W, Cin, Cout) != 1 || !gsd_conv3x3_prefers_w2d(N, H, W, Cin, Cout, 1))
    return 0;
  W2DPlan p;
  if (!plan_w2d(N, H, W, Cout, &p)) return 0;
  if (4 * ceil_div(p.WR * (p.TW / 4 + 2), 64) > 8 || gsd_env_int("GSD_W2D_X4", 1) == 0) return 0;
  const int forced = gsd_env_int("GSD_ACT_ONCE_FORCE", -1);
  if (forced == 0 || forced == 1) return forced;
  const long blocks = (long)N * p.tiles_y * p.tiles_x * p.mblocks;
  // pass_kind 2 (the pooled tensor) is plain today: its chunks save the alignment part only; a concat's other Cin - Cact channels
  // (the up-sampled half) are plain and dense today and aligned then
  const int act = pass_kind >= 2 ? 0 : Cact / 4, plain_chunks = Cin / 4 - act;
  return act_once.saving_us(blocks, act, plain_chunks, p.mblocks) > act_once.cost_us(N, Cact, H, W, pass_kind) ? 1 : 0;
}

static int w2d_impl(const gsd_src* src, int nsrc, const float* wt, int Cin, int Cout, const gsd_dst* dst, int ndst, float* partials,
                    const Conv3Bw& bw, int N, int H, int W, void* stream, float* ws = nullptr, int64_t ws_elems = 0) {
  if (int e = conv3_check_operands("gsd_conv3x3_w2d", true, true, src, nsrc, wt, Cin, Cout, dst, ndst, N, H, W)) return e;
  GSD_REQUIRE(gsd_conv3x3_w2d_supported(Cin, src[0].C), GSD_ERR_UNSUPPORTED,
              "gsd_conv3x3_w2d: Cin=%d and the first segment's %d channels must be multiples of 4 (use gsd_conv3x3_w43)", Cin, src[0].C);

  // (fills address a plane by an unsigned 32-bit BYTE offset from 16 bytes in front of it)
  for (int i = 0; i < nsrc; ++i)
    GSD_REQUIRE((int64_t)src[i].H * src[i].w_stride + 4 < (1LL << 30), GSD_ERR_UNSUPPORTED,
                "gsd_conv3x3_w2d: a source plane must stay below 2^30 floats");
  W2DPlan pl;
  GSD_REQUIRE(plan_w2d(N, H, W, Cout, &pl), GSD_ERR_UNSUPPORTED, "gsd_conv3x3_w2d: no tile shape");
  W2DParams P;
  conv3_fill_common(P, src, nsrc, wt, Cin, Cout, dst, ndst, partials, bw, N, H, W);   // (nchunks = Cin / 4: no remainder)
  P.mblocks = pl.mblocks;
  P.TH = pl.TH; P.TW = pl.TW; P.TWq = pl.TWq; P.tiles_y = pl.tiles_y; P.tiles_x = pl.tiles_x;
  P.WR = pl.WR; P.WC = pl.WC; P.WCp = pl.WCp; P.PS = pl.PS;
  P.NPV = ceil_div(P.WR * P.WCp, 64);
  GSD_REQUIRE(P.NPV <= 4 * NWP, GSD_ERR_UNSUPPORTED, "gsd_conv3x3_w2d: halo window too large");
  // block order: as many m-blocks per pass as have their weight images (24 KiB per chunk) in 3 MiB of the XCD's 4-MiB L2, over
  // groups of as many pixel tiles as make 64 blocks (what an XCD of the four-wave form holds).  GSD_W2D_MGROUP: 0 all m-blocks of a
  // pixel tile together (the order of the shallow levels), n that many; GSD_W2D_PGROUP the pixel tiles per group.  (tuning / A-B runs)
  {
    int g = (gsd_env_int("GSD_W2D_L2KB", 3072) << 10) / (P.nchunks * W2D_WTILE * 4);
    const int forced = gsd_env_int("GSD_W2D_MGROUP", -1);
    if (forced == 0) g = P.mblocks;
    if (forced > 0) g = forced;
    P.mgrp = std::min(std::max(g, 1), P.mblocks);
    P.pgrp = std::max(gsd_env_int("GSD_W2D_PGROUP", 64 / P.mgrp), 1);
    P.ptiles = N * pl.tiles_y * pl.tiles_x;
  }
  const long base = (long)N * pl.tiles_y * pl.tiles_x * P.mblocks;
  // K slabs: only with a workspace (the engine lends one in train mode), only in the four-wave form, and never more than fit
  int S = ws != nullptr ? w2d_slabs.pick(base, P.nchunks, bw.raw != nullptr) : 1;
  while (S > 1 && (int64_t)base * S * (W2D_BM * 256) > ws_elems) --S;
  if (S > 1 && P.nchunks / S < 2) S = 1;
  P.nslab = S;
  P.slabs = S > 1 ? ws : nullptr;
  if (S > 1) GSD_REQUIRE(((uintptr_t)ws & 15) == 0, GSD_ERR_BAD_ARG, "gsd_conv3x3_w2d: the K-slab workspace must be 16-byte aligned");
  const long grid = base * S;
  P.d_mblocks = w2d_div_of(P.mblocks);
  P.d_nslab = w2d_div_of(S);
  P.d_tpi = w2d_div_of(pl.tiles_y * pl.tiles_x);
  P.d_tiles_x = w2d_div_of(pl.tiles_x);
  P.TWq_sh = pl.TWq == 2 ? 1 : pl.TWq == 4 ? 2 : pl.TWq == 8 ? 3 : 4;
  P.dfast = 0;
  for (int i = 0; i < ndst; ++i)
    // (the largest lane offset: 12 planes further, the last tile row, in bytes)
    if (4 * (12 * (int64_t)dst[i].c_stride + (int64_t)dst[i].H * dst[i].w_stride) < (1LL << 32)) P.dfast |= 1 << i;
  GSD_REQUIRE(grid < 2147483647L, GSD_ERR_UNSUPPORTED, "gsd_conv3x3_w2d: grid too large");
  bool plain = true;
  for (int i = 0; i < nsrc; ++i) plain = plain && src[i].scale == nullptr && src[i].relu == 0;
  // 16-byte halo pieces: one plain source whose rows start 16-byte aligned (pitch, plane and image strides multiples of 4 floats);
  // its pad columns must hold zeros -- the engine's row-pitched d_raw buffer does (GSD_W2D_X4=0: dword gathers, A/B runs)
  P.NP = pl.TW / 4 + 2;
  P.NI = ceil_div(P.WR * P.NP, 64);
  const bool x4 = 4 * P.NI <= 8 && gsd_env_int("GSD_W2D_X4", 1) != 0 && gsd_conv3x3_w2d_source_class(src, nsrc) == 1;
  // unaligned 16-byte pieces for every other source: each segment vouches for 4 readable floats around its tensor (slack), lane
  // offsets stay 32-bit.  GSD_W2D_U4=0 keeps the dword gathers.  Default 1 since the loop's other vector work was halved (packed
  // transforms, constant image offsets): forward layer set 21.9 -> 21.2 ms, step -0.4 ms, bit-identical (when first built, against
  // the scalar transforms, it measured neutral: 97.7-97.9 ms either way)
  bool u4 = !x4 && 4 * P.NI <= 8 && gsd_env_int("GSD_W2D_U4", 1) != 0;
  for (int i = 0; i < nsrc && u4; ++i) u4 = src[i].slack >= 4;
  if (x4 || u4) {
    P.WCp = 4 * P.NP;
    P.PS = w2d_x4_plane_stride(pl.TWq, P.WCp, P.WR);
  }
  P.d_NP = w2d_div_of(P.NP);
  P.d_WCp = w2d_div_of(P.WCp);
  // the deep levels' <plain, aligned pieces, unsplit> launches run the band-major flat tile list where it has fewer blocks
  // (gsd_conv3x3_w2d_strips.hip; GSD_W2D_STRIPS); its lanes' source offsets span the images: the whole tensor within 2^30 floats
  if (x4 && S == 1 && (int64_t)N * src[0].n_stride + (int64_t)src[0].H * src[0].w_stride + 8 < (1LL << 30)) {
    W2DStripPlan sp;
    // (a launch with partial rows leaves per-tile sums in the caller's scratch -- unused, as the launch is unsplit -- from which its
    //  rows are added in the rectangles' order: without enough scratch it keeps the rectangles)
    if (w2d_strips_take(N, H, W, P.ptiles, P.mblocks, P.nchunks, &sp) && (long)P.ptiles * NWP <= 65535 &&
        (partials == nullptr || (ws != nullptr && ((uintptr_t)ws & 15) == 0 && ws_elems >= w2d_strips_scratch_elems(sp, P.Mpad))))
      return w2d_strips_launch(P, sp, dst, ndst, ws, (hipStream_t)stream);
  }
  const size_t lds = (size_t)(2 * (W2D_WTILE + 4 * P.PS) + 2 * 4 * P.nchunks + 4 * W2D_BM + 3 * 128 * NWP) * sizeof(float);
  if (gsd_env_set("GSD_W2D_TRACE"))
    fprintf(stderr, "w2d M%d K%d %dx%d N%d nsrc %d ndst %d plain %d x4 %d u4 %d | ptr&15 %d ws %d cs%%4 %d ns%%4 %d NI %d tile %dx%d slabs %d dfast %d\n", Cout, Cin, H, W, N,
            nsrc, ndst, (int)plain, (int)x4, (int)u4, (int)((uintptr_t)src[0].ptr & 15), src[0].w_stride, (int)(src[0].c_stride % 4),
            (int)(src[0].n_stride % 4), P.NI, pl.TH, pl.TW, S, P.dfast);
  if (S > 1) {
    if (x4) return launch_w2d<true, 1, true>(P, (int)grid, lds, (hipStream_t)stream);
    if (u4) return plain ? launch_w2d<true, 2, true>(P, (int)grid, lds, (hipStream_t)stream) : launch_w2d<false, 2, true>(P, (int)grid, lds, (hipStream_t)stream);
    return plain ? launch_w2d<true, 0, true>(P, (int)grid, lds, (hipStream_t)stream) : launch_w2d<false, 0, true>(P, (int)grid, lds, (hipStream_t)stream);
  }
  if (x4) return launch_w2d<true, 1>(P, (int)grid, lds, (hipStream_t)stream);
  if (u4) return plain ? launch_w2d<true, 2>(P, (int)grid, lds, (hipStream_t)stream) : launch_w2d<false, 2>(P, (int)grid, lds, (hipStream_t)stream);
  return plain ? launch_w2d<true>(P, (int)grid, lds, (hipStream_t)stream) : launch_w2d<false>(P, (int)grid, lds, (hipStream_t)stream);
}

extern "C" int gsd_conv3x3_w2d(const gsd_src* src, int nsrc, const float* wt, int Cin, int Cout, const gsd_dst* dst, int ndst,
                               float* partials, int N, int H, int W, void* stream) {
  return w2d_impl(src, nsrc, wt, Cin, Cout, dst, ndst, partials, Conv3Bw{}, N, H, W, stream);
}

extern "C" int gsd_conv3x3_w2d_dgrad_bnrelu(const gsd_src* src, const float* wt, int Cin, int Cout, const gsd_dst* dst,
                                            const float* raw, const float* scale, const float* shift, const float* mean,
                                            const float* invstd, float* partials, int N, int H, int W, void* stream) {
  return gsd_conv3x3_w2d_dgrad_bnrelu_ws(src, wt, Cin, Cout, dst, raw, scale, shift, mean, invstd, partials, nullptr, 0, N, H, W, stream);
}

// The same two with K-slab scratch lent by the caller (gsd_conv3x3_w2d_workspace floats; any capacity is safe: the launcher shrinks
// the slab count to what fits, 0 or a null pointer runs unsplit): what a train-mode schedule calls.  The sum over the input
// channels is then taken slab by slab in a fixed order -- run-to-run bitwise, not bit-equal to the unsplit launch.
extern "C" int gsd_conv3x3_w2d_ws(const gsd_src* src, int nsrc, const float* wt, int Cin, int Cout, const gsd_dst* dst, int ndst,
                                  float* partials, float* workspace, int64_t workspace_elems, int N, int H, int W, void* stream) {
  return w2d_impl(src, nsrc, wt, Cin, Cout, dst, ndst, partials, Conv3Bw{}, N, H, W, stream, workspace, workspace_elems);
}

extern "C" int gsd_conv3x3_w2d_dgrad_bnrelu_ws(const gsd_src* src, const float* wt, int Cin, int Cout, const gsd_dst* dst,
                                               const float* raw, const float* scale, const float* shift, const float* mean,
                                               const float* invstd, float* partials, float* workspace, int64_t workspace_elems, int N,
                                               int H, int W, void* stream) {
  const Conv3Bw bw{raw, scale, shift, mean, invstd};
  if (int e = conv3_check_dgrad_bnrelu("gsd_conv3x3_w2d_dgrad_bnrelu", dst, bw, partials, Cout, H, W)) return e;
  return w2d_impl(src, 1, wt, Cin, Cout, dst, 1, partials, bw, N, H, W, stream, workspace, workspace_elems);
}
