// gsd_wgrad_w2d.hip -- dW of conv3x3 with the transposed TWO-dimensional Winograd identity F(2x4, 3x3) (gfx950).
//
//   dW[co][ci][r][s] = sum_{n,h,w} dy[n,co,h,w] * a[n,ci,h+r-1,w+s-1]
//
// (the dW half of aten::convolution_backward for /root/reference/gelslim_depth/models/unet.py:11,14).  The forward identity of
// gsd_conv3x3_w2d.hip, Y = A2^T[(G2 g G4^T) .* (B2^T d B4)]A4, is linear in g, so for every tile of 2 x 4 outputs
//
//   dg = G2^T [ (A2 dY A4^T) .* (B2^T d B4) ] G4
//
// with the forward's input transform of the 4 x 6 window d, dY (2 x 4) transformed to 4 x 6, and G2^T . G4 applied once at the
// very end: 24 products per (co, ci) and 8 pixels instead of 36 in the row form (gsd_wgrad_w43.hip) and 72 in the direct one.
//
//   D_f[co][ci] = sum_tiles U_f[co][tile] * V_f[tile][ci]      f = (fr, fc), 24 frequencies
//
// GEMM view: M = co, N = ci, K = tiles (4 per v_mfma_f32_16x16x4_f32).  What made this form lose when every wave transformed its
// own operands (7 vector instructions per MFMA at a 16 x 16 wave tile, 264 registers at 32 x 16) is the
// transform work, so here it is done ONCE PER BLOCK and shared through LDS:
//
//   * a block of 8 waves owns BM x BN = 128 co x 32 ci (or 64 x 64 for the 64-channel layers); a k-step is 4 tiles (32 pixels:
//     1 x 4, 2 x 2 or 4 x 1 tiles, chosen per shape); one block per CU, split-K over k-steps;
//   * per k-step every thread takes one or two small transform TASKS -- "U" (one (co, tile): two aligned 16-byte pieces of the
//     row-pitched dy -> A4 along the rows, A2 down the columns -> 24 values) and "V row" (one window row of a (ci, tile): 6 floats ->
//     deferred BatchNorm+ReLU -> B4^T; the B2^T column transform takes the partner row from the lane's quad by DPP) -- in packed
//     fp32 math, and stores the results as [tile][channel][24 frequencies] images;
//   * the raw values of the NEXT k-step wait in LDS, moved by LDS-DMA: dy pieces in per-thread private slots, the activation windows
//     as one image per block and k-step (the halo shared by its tiles, filled as runs of consecutive 16-byte pieces); nothing raw is
//     held in registers across MFMAs (192 accumulators + one piece's values is all that fits);
//   * a wave's 48 MFMAs of k-step i (tile 32 co x 16 ci x 24 frequencies = 192 accumulator registers; operands frequency-major: one
//     ds_read_b128 is four frequencies of (channel l16, tile j), 18 reads per 48 MFMAs, no vector work) run in six groups with the
//     transform of k-step i+1 in PIECES between them -- a software pipeline inside the wave: with separate phases all eight waves of
//     the CU sat in the same phase and the matrix pipes were 0.53 busy (docs/LOG_r06.md);
//   * two transform images and two window images (k-step parity), one barrier per k-step.
//
// On two thirds of the row form's MFMAs; 22.5 ms for the network's 17 layers at batch 32 (row form: 29.5; this kernel before its
// bookkeeping left the vector pipe: 23.8 on the same box, profiles/wg2d_scalar_layers_b32.txt).  The kernel lives at the register
// limit and must compile to ZERO scratch (tests/test_abi.py): with spills hipcc stored two slots on some paths of a branchy
// prologue only and reloaded them on all.
// Split-K over k-steps; the slabs have the row form's layout and gsd_conv3x3_wgrad sums them in a fixed order (wgrad3x3_reduce_kernel,
// gsd_wgrad.hip): bitwise reproducible.
//
// Conventions: U row 3 is +dY row 1 and V row 3 is d3 - d1 (both signs of the textbook F(2,3) flipped: same products).
//
// Record order.  The 24 frequencies (fr, fc) of a (tile, channel) record are six 16-byte groups, one ds_read_b128 operand each, and
// every group is made of the register pairs the packed transforms produce together ((1,2), (3,4) and, in a V row, (0,5)):
//   group 0..3: frequencies fc = 1, 2, 3, 4 of row fr = 0, 3, 1, 2 (in this order: the 64 x 64 form's U lane then reaches its own row
//               and the row it combines with its partner, 0 and 1 or 3 and 2, at one constant distance, 32 bytes);
//   group 4:    [row 0 fc 0, row 3 fc 0, row 0 fc 5, row 3 fc 5];        group 5: the same of rows 1 and 2.
// A U task stores groups as 16-byte pieces; the frequencies 0 and 5 of a row are y[0] and y[3] of a raw dy piece and never a
// register pair, so groups 4 and 5 take 4-byte stores where a lane holds one row (V rows, the 64 x 64 form's U) and one 16-byte
// store assembled by three v_mov where it holds both (the 128 x 32 form's U).  U, V and the epilogue agree on this order and
// nothing else knows it: the accumulator of frequency (fr, fc) is acc[4 group + position].
//
// The loop keeps its bookkeeping off the vector pipe (an fp32 MFMA stream hides scalar instructions and LDS reads, no vector one):
//   * every k-step loads and transforms: a block that has run out of k-steps fetches its last one again (the walk stops, by scalar
//     selects) into the image of a k-step whose MFMAs never run -- no "is there a next k-step" flag in front of every piece;
//   * what is wave-uniform (the border flag, the walk, the fill tests) is an integer in a scalar register;
//   * border k-steps take their masks from two per-lane tables built once in the prologue (row_tab, col_tab below): a lane's masks
//     are separable into a part that depends on the k-step's row position and one that depends on its column position, and only
//     the first, the last and (with a cropped segment) the last-but-one position of a direction mask anything.  The border pieces
//     lie out of line; an interior k-step runs straight through.
// Static counts per instantiation: tests/test_wg2d_isa.py, profiles/wg2d_isa_counts.txt.
#include "gsd_wgrad_host.h"
#include <type_traits>

#include <cstdio>
#include <cstdlib>

typedef float f32x2d __attribute__((ext_vector_type(2)));

// An LDS location from its 32-bit byte address.  The lane's task addresses are formed ONCE, in the prologue, with the base of the
// dynamic LDS block in them: `smem + offset` per access left a `v_add_u32 v, 0, v` in front of every task's LDS instructions (the
// base is resolved to 0 only after instruction selection).
template <class T>
__device__ __forceinline__ __attribute__((address_space(3))) T* wg_lds(unsigned byte_addr) {
  return (__attribute__((address_space(3))) T*)(size_t)byte_addr;
}

struct WgW2dParams {
  SrcD a0, a1;   // activation (B operand), up to two concatenated segments
  SrcD dy;       // gradient w.r.t. the raw conv output (plain, row pitch % 4 == 0, 16-byte aligned)
  float* slabs;  // [split][9 = r*3+s][M][Ncols]: G2^T . G4 applied per split
  int M, Ncols;
  int N, H, W;
  int KY, KX, kx_log2;   // tiles of a k-step: KY x KX == 4
  int tiles_y, tiles_x, sy_n, sx_n;
  int WR, NP, NI;        // window of a k-step: 2 KY + 2 rows x KX + 1 pieces of 4 floats per channel; NI 64-piece fills per block
  int ksteps_total, splits, mblocks, nblocks;
};

// x where bit `bit` of m is set, +0 elsewhere: a sign-extended bit and an AND.  (The mask is opaque: hipcc otherwise turns the AND
// back into a bit test, a compare and a select, hoists the tests of two tasks out of a border block and speculates the block.)
__device__ __forceinline__ int wg_bit_mask(int m, const int bit) {
  int k = (m << (31 - bit)) >> 31;
  asm volatile("" : "+v"(k));
  return k;
}
__device__ __forceinline__ float wg_keep(float x, int m, const int bit) {
  return __builtin_bit_cast(float, __builtin_bit_cast(int, x) & wg_bit_mask(m, bit));
}
__device__ __forceinline__ f32x4 wg_keep4(const f32x4 x, int m, const int bit) {
  typedef int i32x4w __attribute__((ext_vector_type(4)));
  const int k = wg_bit_mask(m, bit);
  return __builtin_bit_cast(f32x4, __builtin_bit_cast(i32x4w, x) & i32x4w{k, k, k, k});
}

__device__ __forceinline__ float w2d_dpp(float v, const int ctrl_is_pair) {
  // quad_perm [2,2,1,1] (0x5A): V column transform partners; quad_perm [1,0,3,2] (0xB1): the other row of a dy pair
  return ctrl_is_pair ? __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true))
                      : __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x5A, 0xf, 0xf, true));
}

// NWM x NWN waves of 32 co x 16 ci.  (4,2): 128 co x 32 ci -- U tasks: one (co, tile) per thread, V row tasks: one per thread.
// (2,4): 64 co x 64 ci -- U tasks split by dy row (the A2 column transform takes the other row by DPP), two V row tasks per thread.
// PLAIN: no activation segment carries a deferred BatchNorm / ReLU.
template <int NWM, int NWN, bool PLAIN>
__global__ __launch_bounds__(512, 1) void wgrad3x3_w2d_kernel(const WgW2dParams P) {
  static_assert(NWM * NWN == 8, "8-wave blocks");
  constexpr int BM = 32 * NWM, BN = 16 * NWN;
  constexpr bool UROW = BM == 64;
  constexpr int NV = BN / 32;
  constexpr int TSU = BM * 24 + 4, TSV = BN * 24 + 4;   // tile strides: an odd number of 16-byte slots (conflict-free b128 reads)
  constexpr int BUF = 4 * TSU + 4 * TSV;
  constexpr int NPD = UROW ? 1 : 2;               // dy pieces per thread and k-step (private slots: [piece][wave][64 lanes x 4 floats])
  constexpr int WINI = BN == 32 ? 10 : 20;        // window image of the block's BN channels: at most BN * 20 pieces = WINI fills of 1 KiB
  constexpr int KB = BN == 32 ? 2 : 3;            // window fills per wave at most
  constexpr int WIN = NPD * 8 * 256;              // first float of the window image
  constexpr int IMG = WIN + 2 * WINI * 256;       // first float of image 0 (two window images: k-step parity, like the images)
  extern __shared__ __attribute__((aligned(16))) float smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / NWN, wn = wave % NWN;
  const int j = lane >> 4, l16 = lane & 15;

  const int lid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int per_split = P.mblocks * P.nblocks;
  const int split = lid / per_split;
  const int rem = lid - split * per_split;
  const int mb = rem % P.mblocks, nb = rem / P.mblocks;
  const int m0 = mb * BM, n0 = nb * BN;
  const int s_begin = (int)((long long)split * P.ksteps_total / P.splits);
  const int s_end = (int)((long long)(split + 1) * P.ksteps_total / P.splits);
  const int nst = s_end - s_begin;

  // ---- the block's activation segment (the host guarantees that its BN channels lie in one) ---------------------------------
  const bool seg1 = P.a1.C > 0 && n0 >= P.a0.C;
  const float* const S_p = seg1 ? P.a1.p : P.a0.p;
  const long long S_ns = seg1 ? P.a1.ns : P.a0.ns, S_cs = seg1 ? P.a1.cs : P.a0.cs;
  const int S_H = seg1 ? P.a1.H : P.a0.H, S_W = seg1 ? P.a1.W : P.a0.W, S_ws = seg1 ? P.a1.ws : P.a0.ws;
  const int S_oh = seg1 ? P.a1.oh : P.a0.oh, S_ow = seg1 ? P.a1.ow : P.a0.ow;
  const int S_c0 = n0 - (seg1 ? P.a0.C : 0);   // first channel of the block inside the segment

  // ---- transform tasks of this thread -----------------------------------------------------------------------------------------
  // (the tile coordinates inside the k-step are needed again for the border masks only: the class tables below, built once)
  const int kxm = P.KX - 1;
  // U: (co, tile[, dy row])
  const int u_t = UROW ? (tid >> 1) & 3 : tid & 3;
  const int u_r = UROW ? tid & 1 : 0;
  const int u_co = UROW ? tid >> 3 : tid >> 2;
  const int u_tyl = u_t >> P.kx_log2, u_txl = u_t & kxm;
  unsigned u_voff = (unsigned)((long long)u_co * P.dy.cs + (long long)(2 * u_tyl + u_r) * P.dy.ws + 4 * u_txl) * 4u;
  const unsigned smem_b = (unsigned)(size_t)(__attribute__((address_space(3))) void*)smem;   // LDS byte address of smem[0]
  // LDS byte addresses of the thread's results in image 0 (record order: see the header).  UROW: u_wr is the lane's own row (fr 0
  // or 3; the combined row fr 1 or 2 lies 32 bytes behind it), u_ws its frequency 0 (frequency 5 at + 8, the combined row's at + 16)
  const unsigned u_rec = smem_b + (unsigned)(IMG + u_t * TSU + u_co * 24) * 4u;
  const unsigned u_wr = u_rec + (UROW ? 16u * u_r : 0u);
  const unsigned u_ws = u_rec + 64u + 4u * u_r;
  // V rows: (ci, tile, window row kr); lane quad = the four rows of one (ci, tile)
  const int v_kr = tid & 3, v_t = (tid >> 2) & 3, v_ci = tid >> 4;
  const int v_tyl = v_t >> P.kx_log2, v_txl = v_t & kxm;
  const unsigned v_rd = smem_b + (unsigned)(WIN + ((v_ci * P.WR + 2 * v_tyl + v_kr) * P.NP + v_txl) * 4) * 4u;   // its 6 floats in the window image
  const int v_slot = (0x1320 >> (4 * v_kr)) & 3;   // frequency row kr -> its 16-byte group: rows are stored in the order 0, 3, 1, 2
  const unsigned v_rec = smem_b + (unsigned)(IMG + 4 * TSU + v_t * TSV + v_ci * 24) * 4u;
  const unsigned v_wr = v_rec + 16u * v_slot;                                  // the row's frequencies 1..4
  const unsigned v_ws = v_rec + 64u + 16u * (v_slot >> 1) + 4u * (v_slot & 1);   // its frequency 0; frequency 5 at + 8
  float v_sgn = (tid & 3) == 1 ? 1.f : -1.f;   // kr0: r0 - r2, kr1: r1 + r2, kr2: r2 - r1, kr3: r3 - r1
  float u_sgn = (UROW && (tid & 1)) ? -1.f : 1.f;    // UROW: row 0 forms r0 + r1, row 1 forms r0 - r1
  // deferred BatchNorm of the block's BN channels: (scale, shift) pairs in LDS behind the images, read per task and k-step (one
  // ds_read_b64 instead of two registers per task held for the whole kernel; the kernel lives at the register limit)
  constexpr int SCS = IMG + 2 * BUF;
  float lo = -__builtin_inff();
  if constexpr (!PLAIN) {
    const SrcD& S = seg1 ? P.a1 : P.a0;
    if (tid < BN) {
      f32x2d v = f32x2d{1.f, 0.f};
      if (S.scale != nullptr) v = f32x2d{S.scale[S_c0 + tid], S.shift[S_c0 + tid]};
      *reinterpret_cast<f32x2d*>(smem + SCS + 2 * tid) = v;
    }
    if (S.relu) lo = 0.f;
    // (published by the first barrier of the pipeline below)
  }

  // ---- coordinates of the next k-step to LOAD, carried incrementally ---------------------------------------------------------
  int st_n, st_sy, st_sx;
  {
    const int per = P.sy_n * P.sx_n;
    st_n = s_begin / per;
    const int rs = s_begin - st_n * per;
    st_sy = rs / P.sx_n;
    st_sx = rs - st_sy * P.sx_n;
  }

  // Raw operands of one k-step wait in LDS (by LDS-DMA), not in registers (14 of them held across the MFMA phase did not fit 256):
  //   * dy: every thread moves ITS OWN pieces (one or two rows of 16 bytes) into a private slot -- piece p of wave w occupies 1 KiB
  //     at (p * 8 + w) * 256 floats, lane l its bytes [16 l, 16 l + 16) -- and reads them back itself a k-step later: the only
  //     ordering needed is the thread's own vmcnt(0) before the read, and program order read -> next fill;
  //   * activation windows: ONE image per block and k-step, [channel][window row][piece of 4 floats], the halo shared by the tiles
  //     of the k-step (80 instead of 128 bytes per row at 1 x 4 tiles) and moved as runs of consecutive pieces by consecutive lanes
  //     (fill i = pieces 64 i .. 64 i + 63 of the image, wave w issues fills w, w + 8, ...).  Another wave's pieces are read, so
  //     there are two window images (k-step parity) and the fills are published by the k-step's barrier (vmcnt(0) in front of it).
  int r_mask = 0;            // edge k-steps: bit 0/1 dy row ok, bits 2..7: window columns of the V tasks ok (bits 8..: the loaded k-step's fills)
  int r_edge = 0;            // wave-uniform, an INTEGER in a scalar register: the masks apply (hipcc parks a uniform bool that crosses
                             // the loop in a vector register and branches on it through v_cndmask / v_cmp / vcc)
  int st_left = nst - 1;     // k-steps the walk below may still advance by
  float* const raw_w = smem + wave * 256;                       // this wave's slot of piece 0 (wave-uniform: the DMA's LDS base)
  const float* const raw_r = smem + wave * 256 + lane * 4;  // this lane's 16 bytes of piece 0
  // window fills of this wave: piece 64 (wave + 8 k) + lane = (channel, window row, piece) -> byte offset from the k-step's window
  // origin in the first channel's plane (0 for a dummy lane behind the image); what a border k-step masks: row_tab / col_tab
  unsigned x_off[KB];
  auto fill_bit = [](const int k) { return k < 2 ? 256 << k : 2; };   // mask bit of window fill k
  int row_tab, col_tab;   // border masks of this lane by k-step class (below)
  // the last-but-one k-step of a direction is a border k-step only where the segment ends inside its window (-1: it does not)
  const int sy_l2 = P.sy_n > 2 && 2 * (P.sy_n - 1) * P.KY + 1 - S_oh > S_H ? P.sy_n - 2 : -1;
  const int sx_l2 = P.sx_n > 2 && 4 * (P.sx_n - 1) * P.KX + 1 - S_ow > S_W ? P.sx_n - 2 : -1;
  {
    int x_wr[KB], x_pp[KB];   // window row and piece of fill k (-1: a dummy lane behind the image)
    const int per_ch = P.WR * P.NP;
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      const int pid = 64 * (wave + 8 * k) + lane;
      const int ch = pid / per_ch, rem = pid - ch * per_ch;
      const int wr = rem / P.NP, pp = rem - wr * P.NP;
      const bool dummy = ch >= BN;
      x_off[k] = dummy ? 0u : (unsigned)((long long)ch * S_cs + (long long)wr * S_ws + 4 * pp) * 4u;
      x_wr[k] = dummy ? -1 : wr;
      x_pp[k] = pp;
    }
    // Border masks.  What a lane must mask in a border k-step is separable: the dy rows and window rows that exist depend on the
    // k-step's ROW position only, the tile columns and window columns on its COLUMN position only, and only the first, the last
    // and -- where a cropped segment ends inside its window -- the last but one k-step of a direction need a mask in that direction
    // (the host admits no other geometry).  So the lane's masks are computed ONCE, here, for these positions -- a 10-bit field each:
    //   bits 0, 1: dy row 0 / 1 of the U task    bits 2..7: the six window columns of the V row task(s)    bits 8, 9: window fills 0, 1
    //   (64 x 64 form: its U task has one dy row, bit 0, and bit 1 is window fill 2)
    // (a row field has its V bits all equal, a column field its U bits) -- and a border k-step ANDs the row field and the column
    // field of its two classes.  A table holds the fields of class 1 (first), 2 (last, not first) and 3 (last but one, where it
    // needs a mask) at bit 10 x (class - 1): a lookup is a shift by a scalar; class 0 (no mask in this direction) is all ones, ORed
    // in from a scalar.  A dummy fill lane has no bit in any field.
    auto row_field = [&](const int ty0) {
      const int hs = 2 * ty0 - 1 - S_oh;
      const int uty = ty0 + u_tyl, h = 2 * uty + u_r;
      int f = (uty < P.tiles_y && h < P.H ? 1 : 0) | (!UROW && uty < P.tiles_y && h + 1 < P.H ? 2 : 0);
      if (ty0 + v_tyl < P.tiles_y && (unsigned)(hs + 2 * v_tyl + v_kr) < (unsigned)S_H) f |= 0xFC;
#pragma unroll
      for (int k = 0; k < KB; ++k)
        if (x_wr[k] >= 0 && (unsigned)(hs + x_wr[k]) < (unsigned)S_H) f |= fill_bit(k);
      return f;
    };
    auto col_field = [&](const int tx0) {
      const int wsx = 4 * tx0 - 1 - S_ow;
      int f = tx0 + u_txl < P.tiles_x ? (UROW ? 1 : 3) : 0;
      // the valid columns of the 6-float row piece are the range [max(0, -c0), min(6, S_W - c0)): a mask from two shifts
      const int c0 = wsx + 4 * v_txl;
      const int lo_ = c0 < 0 ? -c0 : 0, hi_ = S_W - c0;
      const int lo = lo_ < 6 ? lo_ : 6, hi = hi_ < 0 ? 0 : (hi_ < 6 ? hi_ : 6);   // shift counts in [0, 6]
      if (tx0 + v_txl < P.tiles_x && hi > lo) f |= (((1 << hi) - 1) & ~((1 << lo) - 1)) << 2;
#pragma unroll
      for (int k = 0; k < KB; ++k) {
        const int ck = wsx + 4 * x_pp[k];
        if (x_wr[k] >= 0 && ck + 3 >= 0 && ck < S_W) f |= fill_bit(k);
      }
      return f;
    };
    row_tab = row_field(0) | row_field((P.sy_n - 1) * P.KY) << 10 | row_field((P.sy_n > 2 ? P.sy_n - 2 : 0) * P.KY) << 20;
    col_tab = col_field(0) | col_field((P.sx_n - 1) * P.KX) << 10 | col_field((P.sx_n > 2 ? P.sx_n - 2 : 0) * P.KX) << 20;
    asm volatile("" : "+v"(row_tab), "+v"(col_tab));
  }

  // Addresses: a wave-uniform 64-bit base that depends on the IMAGE only (the block's first channel plane) plus an unsigned 32-bit
  // byte offset per lane = (k-step origin, scalar) + (task constant).  A lane whose piece must not be read where it lies takes
  // offset 0 instead.  (The first form of this code selected between 64-bit pointers per lane and held 14 raw registers across
  // the MFMA phase; at 256 registers hipcc then spilled the zero-extended offsets on some paths of the branchy prologue only and
  // reloaded them on all -- wild addresses, a memory fault at the 160x213 level.  No 64-bit vector address selects here, the raw
  // values wait in LDS, and tests/test_abi.py checks that these kernels use no scratch.)
  // the wave issues fill k: all but the last are always on (the host checks NI > 8 (KB - 1)); the last as a scalar integer
  auto fill_on = [&](const int k) __attribute__((always_inline)) {
    if (k < KB - 1) return true;
    int w = wave;
    asm volatile("" : "+s"(w));   // (opaque: the test is two scalar instructions here, not a flag that hipcc parks in a vector register)
    return w + 8 * (KB - 1) < P.NI;
  };
  auto load = [&](auto wb_c) __attribute__((always_inline)) {
    constexpr int wb = decltype(wb_c)::value;   // window image of the k-step (its parity inside the block's range)
    const int n = st_n, ty0 = st_sy * P.KY, tx0 = st_sx * P.KX;
    // the k-step's classes (0: no mask, 1: first, 2: last and not first, 3: last but one where that needs one), scalar integers
    const int cy = st_sy == 0 ? 1 : (st_sy == P.sy_n - 1 ? 2 : (st_sy == sy_l2 ? 3 : 0));
    const int cx = st_sx == 0 ? 1 : (st_sx == P.sx_n - 1 ? 2 : (st_sx == sx_l2 ? 3 : 0));
    {
      // advance the walk -- by scalar selects, and not past the block's last k-step: a load that comes after it fetches that k-step
      // again (addresses a real load has read), into the image and slots of a k-step whose MFMAs never run
      const int adv = st_left > 0 ? 1 : 0;
      st_left -= adv;
      const int sx1 = st_sx + 1, wx = sx1 == P.sx_n ? 1 : 0;
      const int sy1 = st_sy + wx, wy = sy1 == P.sy_n ? 1 : 0;
      st_sx = adv ? (wx ? 0 : sx1) : st_sx;
      st_sy = adv ? (wy ? 0 : sy1) : st_sy;
      st_n += adv & wy;
    }
    const char* const dblk = reinterpret_cast<const char*>(P.dy.p + (long long)n * P.dy.ns + (long long)m0 * P.dy.cs);
    // (the activation base is 4 floats IN FRONT of the plane, inside the slack the caller vouches for: the piece that starts at
    //  column -1 of row 0 of the block's first channel has offset -4 bytes from the plane, and the offsets are UNSIGNED 32-bit --
    //  a zero-extended -4 is 4 GiB away: the memory fault of this kernel's first LDS-DMA builds)
    const char* vblk = reinterpret_cast<const char*>(S_p + (long long)n * S_ns + (long long)S_c0 * S_cs) - 16;
    asm volatile("" : "+s"(vblk));   // (a scalar: otherwise hipcc adds the -16 per lane and fill, a 64-bit vector addition each)
    const int hs = 2 * ty0 - 1 - S_oh, wsx = 4 * tx0 - 1 - S_ow;
    const unsigned d_org = (unsigned)(2 * ty0 * P.dy.ws + 4 * tx0) * 4u;   // k-step origin inside a dy plane, bytes
    const int v_org = (hs * S_ws + wsx) * 4 + 16;                          // ... from vblk (< 0 only where every lane is masked)
    r_edge = __builtin_amdgcn_readfirstlane(cy | cx);
    asm volatile("" : "+v"(u_voff));   // (opaque: hipcc otherwise re-associates the sum in element units, four vector instructions for two)
    unsigned o_y0 = d_org + u_voff, o_y1 = d_org + (unsigned)P.dy.ws * 4u + u_voff;
    unsigned x_o[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) x_o[k] = (unsigned)v_org + x_off[k];
    if (__builtin_expect(r_edge != 0, 0)) {
      const int m = ((row_tab >> (cy ? 10 * cy - 10 : 0)) | (cy ? 0 : 0x3ff)) & ((col_tab >> (cx ? 10 * cx - 10 : 0)) | (cx ? 0 : 0x3ff));   // (bits 10.. are not looked at)
      o_y0 &= (unsigned)wg_bit_mask(m, 0);
      if constexpr (!UROW) o_y1 &= (unsigned)wg_bit_mask(m, 1);
#pragma unroll
      for (int k = 0; k < KB; ++k) x_o[k] &= (unsigned)wg_bit_mask(m, k < 2 ? 8 + k : 1);
      r_mask = m;
    }
    auto fill = [&](const char* base, unsigned off, float* dst) __attribute__((always_inline)) {
      __builtin_amdgcn_global_load_lds(reinterpret_cast<const float*>(base + off), dst, 16, 0, 0);
    };
    // window pieces: one with a column inside the segment lies within 3 floats of its row's ends (slack >= 4) and is read where it
    // lies, partly outside or not (the transform masks by column); one without is not read where it lies (offset 0)
#pragma unroll
    for (int k = 0; k < KB; ++k)
      if (fill_on(k)) {
        fill(vblk, x_o[k], smem + WIN + wb * (WINI * 256) + (wave + 8 * k) * 256);
      }
    // dy pieces go into the slots this thread reads its raw dy rows from: those reads have to have RETURNED before a fill can land
    __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0)
    fill(dblk, o_y0, raw_w);
    if constexpr (!UROW) fill(dblk, o_y1, raw_w + 8 * 256);
  };

  // Stores of a task's 24 (U) or 6 (V row) values at byte offset `ib` (the image) from the task's addresses.  A 16-byte group is
  // two register pairs that the transforms produce together, so hipcc's 16-byte stores need no v_mov -- except the one group of the
  // 128 x 32 form's U task that holds y[0] and y[3] of its two raw pieces.  The 4-byte stores are volatile: left to itself hipcc
  // pairs them into the two-address form, whose 8-bit offsets do not reach image 1 -- a v_add_u32 per pair.
  auto st1 = [&](const unsigned a, const float v) __attribute__((always_inline)) { *wg_lds<volatile float>(a) = v; };
  auto st_u = [&](const unsigned ib, const f32x4& y0, const f32x4& y1, const f32x2d a12, const f32x2d a34, const f32x2d b12,
                  const f32x2d b34) __attribute__((always_inline)) {
    if constexpr (UROW) {
      // this lane holds A4 of ONE dy row; rows fr of U = [r0, r0 + r1, r0 - r1, r1]: lane r = 0 stores (own, own + x) as rows 0, 1,
      // lane r = 1 stores (own, x - own) as rows 3, 2
      asm volatile("" : "+v"(u_sgn));   // (as the V column sign)
      const float sgn = u_sgn;
      const f32x2d sg = {sgn, sgn};
      const f32x2d x12 = {w2d_dpp(a12[0], 1), w2d_dpp(a12[1], 1)}, x34 = {w2d_dpp(a34[0], 1), w2d_dpp(a34[1], 1)};
      const float x0 = w2d_dpp(y0[0], 1), x5 = w2d_dpp(y0[3], 1);
      const f32x2d t12 = __builtin_elementwise_fma(a12, sg, x12), t34 = __builtin_elementwise_fma(a34, sg, x34);
      *wg_lds<f32x4>(u_wr + ib) = f32x4{a12[0], a12[1], a34[0], a34[1]};
      *wg_lds<f32x4>(u_wr + ib + 32) = f32x4{t12[0], t12[1], t34[0], t34[1]};
      st1(u_ws + ib, y0[0]);
      st1(u_ws + ib + 8, y0[3]);
      st1(u_ws + ib + 16, __builtin_fmaf(y0[0], sgn, x0));
      st1(u_ws + ib + 24, __builtin_fmaf(y0[3], sgn, x5));
    } else {
      // rows fr of U = [r0, r0 + r1, r0 - r1, r1]; (s0, d0) and (s5, d5) by one packed fma with (1, -1) each
      const f32x2d pm = {1.f, -1.f};
      const f32x2d sd0 = __builtin_elementwise_fma(f32x2d{y1[0], y1[0]}, pm, f32x2d{y0[0], y0[0]});
      const f32x2d sd5 = __builtin_elementwise_fma(f32x2d{y1[3], y1[3]}, pm, f32x2d{y0[3], y0[3]});
      *wg_lds<f32x2d>(u_wr + ib) = a12;
      *wg_lds<f32x2d>(u_wr + ib + 8) = a34;
      *wg_lds<f32x2d>(u_wr + ib + 16) = b12;
      *wg_lds<f32x2d>(u_wr + ib + 24) = b34;
      *wg_lds<f32x2d>(u_wr + ib + 32) = a12 + b12;
      *wg_lds<f32x2d>(u_wr + ib + 40) = a34 + b34;
      *wg_lds<f32x2d>(u_wr + ib + 48) = a12 - b12;
      *wg_lds<f32x2d>(u_wr + ib + 56) = a34 - b34;
      *wg_lds<f32x4>(u_wr + ib + 64) = f32x4{y0[0], y1[0], y0[3], y1[3]};
      *wg_lds<f32x2d>(u_wr + ib + 80) = sd0;
      *wg_lds<f32x2d>(u_wr + ib + 88) = sd5;
    }
  };
  auto st_v = [&](const unsigned ib, const f32x2d o12, const f32x2d o34, const f32x2d o05) __attribute__((always_inline)) {
    *wg_lds<f32x4>(v_wr + ib) = f32x4{o12[0], o12[1], o34[0], o34[1]};
    st1(v_ws + ib, o05[0]);
    st1(v_ws + ib + 8, o05[1]);
  };

  // transform this thread's raw pieces into LDS image `buf` (compile-time constant)
  auto transform = [&](auto buf_c) __attribute__((always_inline)) {
    constexpr int buf = decltype(buf_c)::value;
    // Packed fp32 math (v_pk_add_f32 / v_pk_fma_f32: two floats for the issue slot of one; an fp32 MFMA stream does not hide vector
    // instructions, profiles/r05_mfma_f32_issue_ubench.txt).  The transforms produce the frequencies (1,2), (3,4) and (0,5) of a row
    // as register pairs; st_u / st_v store them in the record order of the header.
    const f32x2d p1m1 = {1.f, -1.f}, p2m2 = {2.f, -2.f}, c4 = {4.f, 4.f};
    // A4 of one dy row (y0..y3) -> (U1, U2), (U3, U4); U0 = y0, U5 = y3
    auto a4_row = [&](const f32x4& y, f32x2d& u12, f32x2d& u34) __attribute__((always_inline)) {
      const f32x2d lo2 = {y[0], y[1]}, hi2 = {y[2], y[3]};
      const f32x2d pq = lo2 + hi2;                                   // (y0 + y2, y1 + y3)
      const f32x2d ab = __builtin_elementwise_fma(c4, hi2, lo2);     // (y0 + 4 y2, y1 + 4 y3)
      u12 = __builtin_elementwise_fma(f32x2d{pq[1], pq[1]}, p1m1, f32x2d{pq[0], pq[0]});
      u34 = __builtin_elementwise_fma(f32x2d{ab[1], ab[1]}, p2m2, f32x2d{ab[0], ab[0]});
    };
    // ---- U ----
    {
      f32x4 y0 = *reinterpret_cast<const f32x4*>(raw_r), y1 = y0;
      if constexpr (!UROW) y1 = *reinterpret_cast<const f32x4*>(raw_r + 8 * 256);
      if (r_edge) {
        y0 = wg_keep4(y0, r_mask, 0);
        if constexpr (!UROW) y1 = wg_keep4(y1, r_mask, 1);
      }
      f32x2d a12, a34;
      a4_row(y0, a12, a34);
      f32x2d b12 = a12, b34 = a34;
      if constexpr (!UROW) a4_row(y1, b12, b34);
      st_u(buf * BUF * 4u, y0, y1, a12, a34, b12, b34);
    }
    // ---- V rows ----
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const unsigned wp = v_rd + buf * (WINI * 256) * 4u + (i ? (unsigned)(32 * 16 * (P.WR * P.NP)) : 0u);
      const f32x4 ra = *wg_lds<const f32x4>(wp);
      const f32x2d rb = *wg_lds<const f32x2d>(wp + 16);
      f32x2d t0 = {ra[0], ra[1]}, t1 = {ra[2], ra[3]}, t2 = rb;
      if constexpr (!PLAIN) {
        const f32x2d ss = *reinterpret_cast<const f32x2d*>(smem + SCS + 2 * ((tid >> 4) + 32 * i));
        const f32x2d sc2 = {ss[0], ss[0]}, sh2 = {ss[1], ss[1]}, lo2 = {lo, lo};
        t0 = __builtin_elementwise_max(__builtin_elementwise_fma(t0, sc2, sh2), lo2);
        t1 = __builtin_elementwise_max(__builtin_elementwise_fma(t1, sc2, sh2), lo2);
        t2 = __builtin_elementwise_max(__builtin_elementwise_fma(t2, sc2, sh2), lo2);
      }
      if (r_edge) {
        const int m = r_mask;
        t0 = f32x2d{wg_keep(t0[0], m, 2), wg_keep(t0[1], m, 3)};
        t1 = f32x2d{wg_keep(t1[0], m, 4), wg_keep(t1[1], m, 5)};
        t2 = f32x2d{wg_keep(t2[0], m, 6), wg_keep(t2[1], m, 7)};
      }
      // B4^T of the window row d0..d5 = (t0, t1, t2), as gsd_conv3x3_w2d.hip forms it
      const f32x2d m41 = {-4.f, -1.f}, m5 = {-5.f, -5.f};
      const f32x2d ac = __builtin_elementwise_fma(f32x2d{t1[0], t1[0]}, m41, f32x2d{t2[0], t2[0]});   // (d4 - 4 d2, d4 - d2)
      const f32x2d be = __builtin_elementwise_fma(f32x2d{t0[1], t0[1]}, m41, f32x2d{t1[1], t1[1]});   // (d3 - 4 d1, d3 - d1)
      const f32x2d v12 = __builtin_elementwise_fma(f32x2d{be[0], be[0]}, p1m1, f32x2d{ac[0], ac[0]});
      const f32x2d v34 = __builtin_elementwise_fma(f32x2d{be[1], be[1]}, p2m2, f32x2d{ac[1], ac[1]});
      const f32x2d v05 = __builtin_elementwise_fma(t0, c4, __builtin_elementwise_fma(t1, m5, t2));
      // B2^T down the window column: the partner row from the lane's quad
      const f32x2d sg = {v_sgn, v_sgn};
      const f32x2d x12 = {w2d_dpp(v12[0], 0), w2d_dpp(v12[1], 0)}, x34 = {w2d_dpp(v34[0], 0), w2d_dpp(v34[1], 0)};
      const f32x2d x05 = {w2d_dpp(v05[0], 0), w2d_dpp(v05[1], 0)};
      st_v((buf * BUF + i * (32 * 24)) * 4u, __builtin_elementwise_fma(sg, x12, v12), __builtin_elementwise_fma(sg, x34, v34),
           __builtin_elementwise_fma(sg, x05, v05));
    }
  };

  f32x4 acc[2][24];   // (zeroed behind the pipeline's prologue: 192 registers that the prologue's address work does not have to avoid)

  // operand reads: ONE address register per operand, the image's offset (< 64 KiB) in the instruction's immediate
  unsigned a_rd = smem_b + (unsigned)(IMG + j * TSU + (wm * 32 + l16) * 24) * 4u;
  unsigned b_rd = smem_b + (unsigned)(IMG + 4 * TSU + j * TSV + (wn * 16 + l16) * 24) * 4u;
  asm volatile("" : "+v"(a_rd), "+v"(b_rd));
  static_assert((BUF + 16 * 24 + 24) * 4 < 65536, "image 1 within the 16-bit offset of a ds_read");

  // ---- pipeline: image (it & 1) holds the transforms of k-step `it`; the raw registers hold k-step it + 1 ---------------------
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  if (nst > 0) {
    load(I0{});
    gsd_dma_barrier();   // vmcnt(0) + barrier: everyone's fills of the first k-step are in
    transform(I0{});
    load(I1{});          // (the block's only k-step again if nst == 1)
    gsd_dma_barrier();
  }
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int f = 0; f < 24; ++f) acc[m][f] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (nst > 0) {
    // The transform of k-step it + 1 runs in pieces BETWEEN the MFMA groups of k-step it (a software pipeline inside the wave).
    // With separate phases a k-step was a chain of exposed latencies: raw reads -> transform -> stores | fills | operand reads ->
    // MFMAs, every wave of the CU in the same phase (barrier): stamps showed a wave in its MFMA phase for 36 % of a k-step and
    // removing a third of the vector instructions changed nothing.  Here the vector work rides between the MFMA groups: a piece
    // of ~10-16 instructions works on values that were read a group earlier, clustered (the first vector instruction in an MFMA gap
    // costs 12.6 cycles, each further one 4: profiles/r05_mfma_f32_issue_ubench.txt), and its LDS latencies lie behind MFMAs.
    auto step = [&](auto cur_c) __attribute__((always_inline)) {
      constexpr int cur = decltype(cur_c)::value, nxt = cur ^ 1;
      const f32x2d p1m1 = {1.f, -1.f}, p2m2 = {2.f, -2.f}, c4 = {4.f, 4.f};
      // One operand group = four frequencies of (channel l16, tile j) per ds_read_b128: 3 reads feed 8 MFMAs.  The groups are NOT
      // double-buffered in the source: 12 operand registers instead of 24 keep the kernel inside 256 registers without scratch, and
      // the SIMD's other wave multiplies while this one waits for its reads.
      f32x4 a0, a1, b;
      auto rd_ops = [&](const int g) __attribute__((always_inline)) {
        a0 = *wg_lds<const f32x4>(a_rd + (cur * BUF + 4 * g) * 4u);
        a1 = *wg_lds<const f32x4>(a_rd + (cur * BUF + 16 * 24 + 4 * g) * 4u);
        b = *wg_lds<const f32x4>(b_rd + (cur * BUF + 4 * g) * 4u);
      };
      auto mm = [&](const int g) __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[0][4 * g + e] = mfma16(a0[e], b[e], acc[0][4 * g + e]);
          acc[1][4 * g + e] = mfma16(a1[e], b[e], acc[1][4 * g + e]);
        }
      };
      auto a4_row = [&](const f32x4& y, f32x2d& u12, f32x2d& u34) __attribute__((always_inline)) {
        const f32x2d lo2 = {y[0], y[1]}, hi2 = {y[2], y[3]};
        const f32x2d pq = lo2 + hi2;
        const f32x2d ab = __builtin_elementwise_fma(c4, hi2, lo2);
        u12 = __builtin_elementwise_fma(f32x2d{pq[1], pq[1]}, p1m1, f32x2d{pq[0], pq[0]});
        u34 = __builtin_elementwise_fma(f32x2d{ab[1], ab[1]}, p2m2, f32x2d{ab[0], ab[0]});
      };
      // masks of the k-step being transformed (load() below replaces r_mask / r_edge by the next one's)
      const int t_mask = r_mask;
      int t_edge = r_edge;
      asm volatile("" : "+s"(t_edge));
      auto edge = [&]() __attribute__((always_inline)) {   // opaque per use: a scalar compare and branch each
        int e = t_edge;
        asm volatile("" : "+s"(e));
        return e != 0;
      };
      f32x4 y0, y1;
      f32x2d a12, a34, b12, b34;
      f32x4 ra;
      f32x2d rb, v12, v34, v05;
      auto rd_y = [&]() __attribute__((always_inline)) {
        y0 = *reinterpret_cast<const f32x4*>(raw_r);
        y1 = y0;
        if constexpr (!UROW) y1 = *reinterpret_cast<const f32x4*>(raw_r + 8 * 256);
      };
      auto u_rows = [&]() __attribute__((always_inline)) {      // A4 along the dy rows
        if (__builtin_expect(edge(), 0)) {   // (the border pieces lie out of line: the interior path falls through)
          y0 = wg_keep4(y0, t_mask, 0);
          if constexpr (!UROW) y1 = wg_keep4(y1, t_mask, 1);
        }
        a4_row(y0, a12, a34);
        if constexpr (!UROW) a4_row(y1, b12, b34);
      };
      auto u_cols = [&]() __attribute__((always_inline)) {      // A2 down the columns, stores
        st_u(nxt * BUF * 4u, y0, y1, a12, a34, b12, b34);
      };
      auto rd_v = [&](const int i) __attribute__((always_inline)) {
        const unsigned wp = v_rd + nxt * (WINI * 256) * 4u + (i ? (unsigned)(32 * 16 * (P.WR * P.NP)) : 0u);
        ra = *wg_lds<const f32x4>(wp);
        rb = *wg_lds<const f32x2d>(wp + 16);
      };
      auto v_rows = [&](const int i) __attribute__((always_inline)) {   // deferred BatchNorm + ReLU, masks, B4^T along the window row
        f32x2d t0 = {ra[0], ra[1]}, t1 = {ra[2], ra[3]}, t2 = rb;
        if constexpr (!PLAIN) {
          const f32x2d ss = *reinterpret_cast<const f32x2d*>(smem + SCS + 2 * ((tid >> 4) + 32 * i));
          const f32x2d sc2 = {ss[0], ss[0]}, sh2 = {ss[1], ss[1]}, lo2 = {lo, lo};
          t0 = __builtin_elementwise_max(__builtin_elementwise_fma(t0, sc2, sh2), lo2);
          t1 = __builtin_elementwise_max(__builtin_elementwise_fma(t1, sc2, sh2), lo2);
          t2 = __builtin_elementwise_max(__builtin_elementwise_fma(t2, sc2, sh2), lo2);
        }
        if (__builtin_expect(edge(), 0)) {   // (the border pieces lie out of line: the interior path falls through)
          const int m = t_mask;
          t0 = f32x2d{wg_keep(t0[0], m, 2), wg_keep(t0[1], m, 3)};
          t1 = f32x2d{wg_keep(t1[0], m, 4), wg_keep(t1[1], m, 5)};
          t2 = f32x2d{wg_keep(t2[0], m, 6), wg_keep(t2[1], m, 7)};
        }
        const f32x2d m41 = {-4.f, -1.f}, m5 = {-5.f, -5.f};
        const f32x2d ac = __builtin_elementwise_fma(f32x2d{t1[0], t1[0]}, m41, f32x2d{t2[0], t2[0]});
        const f32x2d be = __builtin_elementwise_fma(f32x2d{t0[1], t0[1]}, m41, f32x2d{t1[1], t1[1]});
        v12 = __builtin_elementwise_fma(f32x2d{be[0], be[0]}, p1m1, f32x2d{ac[0], ac[0]});
        v34 = __builtin_elementwise_fma(f32x2d{be[1], be[1]}, p2m2, f32x2d{ac[1], ac[1]});
        v05 = __builtin_elementwise_fma(t0, c4, __builtin_elementwise_fma(t1, m5, t2));
      };
      auto v_cols = [&](const int i) __attribute__((always_inline)) {   // B2^T down the window column (quad partners by DPP), stores
        // ONE register for the whole kernel (re-deriving it cost four vector instructions per task); opaque here, so that the pair
        // is formed by the instruction's operand selects and not held as two registers
        asm volatile("" : "+v"(v_sgn));
        const f32x2d sg = {v_sgn, v_sgn};
        const f32x2d x12 = {w2d_dpp(v12[0], 0), w2d_dpp(v12[1], 0)}, x34 = {w2d_dpp(v34[0], 0), w2d_dpp(v34[1], 0)};
        const f32x2d x05 = {w2d_dpp(v05[0], 0), w2d_dpp(v05[1], 0)};
        st_v((nxt * BUF + i * (32 * 24)) * 4u, __builtin_elementwise_fma(sg, x12, v12), __builtin_elementwise_fma(sg, x34, v34),
             __builtin_elementwise_fma(sg, x05, v05));
      };
      // one MFMA group, the next group's operand reads behind it, and a vector piece
      auto group = [&](const int g, auto piece) __attribute__((always_inline)) {
        mm(g);
        __builtin_amdgcn_sched_barrier(0);
        if (g + 1 < 6) rd_ops(g + 1);
        piece();
        __builtin_amdgcn_sched_barrier(0);
      };
      rd_ops(0);
      rd_y();
      __builtin_amdgcn_sched_barrier(0);
      group(0, [&]() __attribute__((always_inline)) { load(cur_c); });   // fills of k-step it + 2 (this one's parity); waits for rd_y
      group(1, [&]() __attribute__((always_inline)) { u_rows(); if constexpr (UROW) u_cols(); });
      group(2, [&]() __attribute__((always_inline)) { rd_v(0); if constexpr (!UROW) u_cols(); });
      group(3, [&]() __attribute__((always_inline)) { v_rows(0); });
      group(4, [&]() __attribute__((always_inline)) { v_cols(0); if constexpr (NV > 1) rd_v(1); });
      group(5, [&]() __attribute__((always_inline)) {
        if constexpr (NV > 1) {
          v_rows(1);
          v_cols(1);
        }
      });
      // the fills of k-step it + 2 have had the MFMA groups to land; published to the other waves (window pieces) by the barrier
      gsd_dma_barrier();
    };
    for (int it = 0; it < nst; it += 2) {
      step(I0{});
      if (it + 1 < nst) step(I1{});
    }
  }

  // ---- epilogue: G4 along fc, G2^T along fr, per split (linear: the slab reduction only adds) ---------------------------------
  const size_t pl = (size_t)P.M * P.Ncols;
  // (lane coordinates re-derived behind the loop from a laundered thread id: nothing of the epilogue's addressing is held in a
  //  register -- or spilled -- across the loop)
  int tid_e = threadIdx.x;
  asm volatile("" : "+v"(tid_e));
  const int j_e = (tid_e & 63) >> 4, l16_e = tid_e & 15;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int mr = m0 + wm * 32 + m * 16 + j_e * 4 + reg;
      const int col = n0 + wn * 16 + l16_e;
      float E[4][3];
#pragma unroll
      for (int fr = 0; fr < 4; ++fr) {
        // (record order: frequencies 1..4 of row fr in group sl, frequencies 0 and 5 in groups 4 and 5 -- see the header)
        const int sl = (0x1320 >> (4 * fr)) & 3, f0 = 16 + 4 * (sl >> 1) + (sl & 1);
        const float D1 = acc[m][4 * sl + 0][reg], D2 = acc[m][4 * sl + 1][reg], D3 = acc[m][4 * sl + 2][reg];
        const float D4 = acc[m][4 * sl + 3][reg], D0 = acc[m][f0][reg], D5 = acc[m][f0 + 2][reg];
        E[fr][0] = 0.25f * D0 - (1.f / 6.f) * (D1 + D2) + (1.f / 24.f) * (D3 + D4);
        E[fr][1] = (1.f / 6.f) * (D2 - D1) + (1.f / 12.f) * (D3 - D4);
        E[fr][2] = (1.f / 6.f) * (D3 + D4 - D1 - D2) + D5;
      }
      float* const o = P.slabs + ((size_t)split * 9 * P.M + mr) * P.Ncols + col;
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const float h = 0.5f * (E[1][s] + E[2][s]);
        o[(0 * 3 + s) * pl] = E[0][s] + h;
        o[(1 * 3 + s) * pl] = 0.5f * (E[1][s] - E[2][s]);
        o[(2 * 3 + s) * pl] = h + E[3][s];
      }
    }
}

namespace {

struct WgW2dPlan {
  int KY, KX, kx_log2, tiles_y, tiles_x, sy_n, sx_n, BM, BN, mblocks, nblocks, ksteps_total, splits;
  int64_t slab_elems;
  bool ok;
};

WgW2dPlan plan_wg2d(int N, int H, int W, int M, int Ncols) {
  WgW2dPlan p;
  p.tiles_y = ceil_div(H, 2);
  p.tiles_x = ceil_div(W, 4);
  long best = -1;
  int force_kx = gsd_env_int("GSD_WG2D_KX", 0);   // tuning: 1, 2 or 4 tiles across; any other value is ignored
  if (force_kx != 1 && force_kx != 2 && force_kx != 4) force_kx = 0;
  p.KY = 1; p.KX = 4;
  for (int kx = 4; kx >= 1; kx /= 2) {
    if (force_kx && kx != force_kx) continue;
    const int ky = 4 / kx;
    // fewest k-steps, weighted by what a k-step of that shape costs (profiles/r06_wg2d_kstep_shapes.txt, batch 32): 2 x 2 tiles cost
    // what 1 x 4 tiles cost within 2 % either way (a 6 x 12 window instead of 4 x 20) and get the ties, 4 x 1 tiles 7-16 % more
    const long steps = (long)ceil_div(p.tiles_y, ky) * ceil_div(p.tiles_x, kx) * (kx == 4 ? 100 : kx == 2 ? 99 : 112);
    if (best < 0 || steps < best) {
      best = steps;
      p.KY = ky; p.KX = kx;
    }
  }
  p.kx_log2 = p.KX == 4 ? 2 : p.KX == 2 ? 1 : 0;
  p.sy_n = ceil_div(p.tiles_y, p.KY);
  p.sx_n = ceil_div(p.tiles_x, p.KX);
  p.BM = M >= 128 ? 128 : 64;
  p.BN = p.BM == 128 ? 32 : 64;
  p.ok = M % p.BM == 0 && Ncols % p.BN == 0;
  p.mblocks = ceil_div(M, p.BM);
  p.nblocks = ceil_div(Ncols, p.BN);
  p.ksteps_total = N * p.sy_n * p.sx_n;
  const int target = gsd_env_int("GSD_WG2D_BLOCKS", gsd_cu_count());   // one block per CU (256 on MI355X, and where no device is visible)
  p.splits = wgrad_pick_splits(target, p.mblocks * p.nblocks, p.ksteps_total);
  p.slab_elems = (int64_t)p.splits * 9 * M * Ncols;
  return p;
}

}  // namespace

// floats of slab scratch the 2-D form wants for a shape (0: the shape is not served)
int64_t gsd_wgrad_w2d_workspace(int N, int H, int W, int Cin, int Cout) {
  const WgW2dPlan p = plan_wg2d(N, H, W, Cout, Cin);
  return p.ok ? p.slab_elems : 0;
}

// MFMA instructions of one launch: k-steps x 24 frequencies per (16 co x 16 ci) pair
int64_t gsd_wgrad_w2d_mfma_count(int N, int H, int W, int Cin, int Cout) {
  const WgW2dPlan p = plan_wg2d(N, H, W, Cout, Cin);
  return p.ok ? (int64_t)p.ksteps_total * 24 * (Cout / 16) * (Cin / 16) : 0;
}

// 1: the arguments admit the 2-D form (shape, segment geometry, alignment, slack); GSD_WGRAD_W2D=0 switches it off
int gsd_wgrad_w2d_use(const gsd_src* a, int nsrc, const gsd_src* dy, int Cin, int Cout, int N, int H, int W) {
  if (gsd_env_int("GSD_WGRAD_W2D", 1) == 0) return 0;
  const WgW2dPlan p = plan_wg2d(N, H, W, Cout, Cin);
  if (!p.ok) return 0;
  if (!wgrad_dy_x4(*dy)) return 0;
  if (dy->w_stride < 4 * p.tiles_x) return 0;
  if ((int64_t)p.BM * dy->c_stride * 4 >= (1LL << 31)) return 0;   // lane offsets are 32-bit byte offsets inside a block's planes
  if (nsrc == 2 && a[0].C % p.BN != 0) return 0;
  for (int i = 0; i < nsrc; ++i) {
    // the kernel's border masks go by k-step class: a k-step that is not the first, the last or the last but one of a direction
    // must lie inside the segment in that direction (true whenever the pad offsets are smaller than a k-step, as in the U-Net)
    if (p.sy_n > 2 && (a[i].off_h < 0 || a[i].off_h > 2 * p.KY - 1 || 2 * (p.sy_n > 3 ? p.sy_n - 2 : 0) * p.KY + 1 - a[i].off_h > a[i].H)) return 0;
    if (p.sx_n > 2 && (a[i].off_w < 0 || a[i].off_w > 4 * p.KX - 1 || 4 * (p.sx_n > 3 ? p.sx_n - 2 : 0) * p.KX + 1 - a[i].off_w > a[i].W)) return 0;
    if (a[i].slack < 4) return 0;
    if ((int64_t)p.BN * a[i].c_stride * 4 >= (1LL << 31)) return 0;
    if ((int64_t)(a[i].H + 4) * a[i].w_stride * 4 >= (1LL << 31)) return 0;   // (k-step origins inside a plane are 32-bit too)
  }
  return 1;
}

// arguments and workspace already validated by gsd_conv3x3_wgrad, the form's own conditions by gsd_wgrad_w2d_use; returns the slab count
int gsd_wgrad_w2d_run(const gsd_src* a, int nsrc, const gsd_src* dy, int Cin, int Cout, float* workspace, int N, int H, int W,
                      void* stream) {
  const WgW2dPlan pl = plan_wg2d(N, H, W, Cout, Cin);
  WgW2dParams P;
  wgrad_fill_common(P, a, nsrc, dy, Cin, Cout, workspace, N, H, W, pl.splits, pl.mblocks, pl.nblocks);
  P.KY = pl.KY; P.KX = pl.KX; P.kx_log2 = pl.kx_log2;
  P.tiles_y = pl.tiles_y; P.tiles_x = pl.tiles_x; P.sy_n = pl.sy_n; P.sx_n = pl.sx_n;
  P.WR = 2 * pl.KY + 2; P.NP = pl.KX + 1;
  P.NI = (pl.BN * P.WR * P.NP + 63) / 64;
  P.ksteps_total = pl.ksteps_total;
  const bool plain = wgrad_plain(a, nsrc);
  const long grid = (long)pl.splits * pl.mblocks * pl.nblocks;
  // LDS (floats): dy slots [1 or 2 pieces][8 waves][256] | two window images of 10 / 20 KiB | two images of [4 tiles][BM | BN][24] (+4) | (scale, shift)[BN]
  const size_t lds = ((size_t)(pl.BM == 64 ? 1 : 2) * 8 * 256 + (size_t)2 * (pl.BN == 32 ? 10 : 20) * 256 +
                      (size_t)2 * (4 * (pl.BM * 24 + 4) + 4 * (pl.BN * 24 + 4)) + 2 * pl.BN) * sizeof(float);
  GSD_REQUIRE(P.NI <= 8 * (pl.BN == 32 ? 2 : 3) && P.NI <= (pl.BN == 32 ? 10 : 20) && P.NI > 8 * (pl.BN == 32 ? 1 : 2), GSD_ERR_UNSUPPORTED, "gsd_conv3x3_wgrad (w2d): window image too large");
  if (gsd_env_set("GSD_WG43_TRACE"))   // tuning: one line per launch
    fprintf(stderr, "wg2d M%d N%d %dx%d B%d kstep %dx%d ksteps %d splits %d blocks %ld BM %d BN %d plain %d lds %zu\n", Cout, Cin, H, W,
            N, pl.KY, pl.KX, pl.ksteps_total, pl.splits, grid, pl.BM, pl.BN, (int)plain, lds);
  const dim3 g((int)grid);
  const hipStream_t st = (hipStream_t)stream;
  const char* const what = "gsd_conv3x3_wgrad (w2d)";
  if (int e = pl.BM == 128 ? (plain ? gsd_launch<wgrad3x3_w2d_kernel<4, 2, true>>(what, g, dim3(512), lds, st, P)
                                    : gsd_launch<wgrad3x3_w2d_kernel<4, 2, false>>(what, g, dim3(512), lds, st, P))
                           : (plain ? gsd_launch<wgrad3x3_w2d_kernel<2, 4, true>>(what, g, dim3(512), lds, st, P)
                                    : gsd_launch<wgrad3x3_w2d_kernel<2, 4, false>>(what, g, dim3(512), lds, st, P)))
    return e;
  return pl.splits;
}
