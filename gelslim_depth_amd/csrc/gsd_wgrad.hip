// gsd_wgrad.hip -- weight gradients as implicit GEMM over pixels on v_mfma_f32_16x16x4_f32 (gfx950).
//
//   conv3x3:  dW[co][ci][tap] = sum_{n,h,w} dy[n,co,h,w] * a[n,ci,h+kh-1,w+kw-1]      (wgrad3x3_dma_kernel)
//             (the dW half of aten::convolution_backward for /root/reference/gelslim_depth/models/unet.py:11,14)
//   convT2x2: dW[ci][co][kh][kw] = sum_{n,h,w} x[n,ci,h,w] * dy[n,co,2h+kh,2w+kw]      (convT_wgrad_kernel, unet.py:36)
//
// GEMM view: D[m][col] = sum_pixels A[m][pixel] * B[pixel][col] with the pixel index on the MFMA
// k dimension (4 consecutive pixels of one row per instruction).  A = dy rows (convT: space-to-depth
// rows (co,kh,kw)), B = activation with deferred BatchNorm+ReLU, zero padding and the two-segment
// channel concat recomputed on load, so the tensors the reference saves for backward (relu outputs,
// padded/concatenated inputs) are never stored.
//
// Wave tile: 64 m-rows x (16 input channels x 9 taps) [conv3x3] or 64 x 64 [convT].
// Reduction over pixels is split across blocks (split-K); every block writes a partial slab and a
// second kernel sums the slabs in a fixed order => bitwise reproducible.
#include "gsd_common.h"
#include "gsd_wgrad_internal.h"

#include <cstdlib>

struct WgradParams {
  SrcD a0, a1;  // B operand (activation)
  SrcD dy;      // A operand (gradient, plain)
  float* slabs;
  int M, Ncols, Cact;  // M rows (Cout or Cout*4), Ncols = Cin, Cact = total channels of a0+a1
  int N, H, W;
  int TH, TW, tiles_y, tiles_x, WR, WC, PS;  // conv3x3
  int tiles_flat;                            // convT
  int stages_total, splits, mblocks, nblocks;
};

// ConvT2x2 dW: flat 64-pixel stages, register-staged operand tiles (A = space-to-depth dy rows (co,kh,kw),
// B = x with the deferred BatchNorm+ReLU applied on load), wave tile 64 x 64.
template <int WM, int WN>
__global__ __launch_bounds__(256) void convT_wgrad_kernel(const WgradParams P) {
  constexpr int MT = 4, NTB = 4;
  constexpr int BMw = WM * 64, BNw = WN * 64;
  constexpr int DS = 66;  // == 2 (mod 32): 16 rows x 2 k-pixels of a half-wave hit 32 distinct banks

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Al = smem;             // [BMw][DS]
  float* Xl = smem + BMw * DS;  // [BNw][DS]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int j = lane >> 4, l16 = lane & 15;

  const int per_split = P.mblocks * P.nblocks;
  const int split = blockIdx.x / per_split;
  const int rem = blockIdx.x - split * per_split;
  const int mb = rem % P.mblocks, nb = rem / P.mblocks;
  const int m0 = mb * BMw, n0 = nb * BNw;
  const int s_begin = (int)((long long)split * P.stages_total / P.splits);
  const int s_end = (int)((long long)(split + 1) * P.stages_total / P.splits);
  const int HW = P.H * P.W;

  f32x4 acc[MT][NTB];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int t = 0; t < NTB; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int q = tid & 63;     // loader pixel
  const int lrow = tid >> 6;  // loader row phase 0..3

  for (int stage = s_begin; stage < s_end; ++stage) {
    const int n = stage / P.tiles_flat;
    const int p = (stage - n * P.tiles_flat) * 64 + q;
    const bool pix_ok = p < HW;
    const int h = pix_ok ? p / P.W : 0;
    const int w = pix_ok ? p - h * P.W : 0;
    __syncthreads();  // previous stage's MFMAs are done with LDS
#pragma unroll
    for (int i = 0; i < BMw / 8; ++i) {
      const int rr = lrow + 4 * i;  // (co_i, kh)
      const int co = (m0 >> 2) + (rr >> 1);
      const int kh = rr & 1;
      float2 v = make_float2(0.f, 0.f);
      if (pix_ok && co < P.dy.C)
        v = *reinterpret_cast<const float2*>(P.dy.p + (long long)n * P.dy.ns + (long long)co * P.dy.cs +
                                             (long long)(2 * h + kh) * P.dy.W + 2 * w);
      const int mrow = (rr >> 1) * 4 + kh * 2;
      Al[mrow * DS + q] = v.x;
      Al[(mrow + 1) * DS + q] = v.y;
    }
#pragma unroll
    for (int i = 0; i < BNw / 4; ++i) {
      const int ch = lrow + 4 * i;
      const int c = n0 + ch;
      float v = 0.f;
      if (pix_ok && c < P.a0.C) {
        v = P.a0.p[(long long)n * P.a0.ns + (long long)c * P.a0.cs + p];
        if (P.a0.scale != nullptr) v = apply_affine(v, P.a0.scale[c], P.a0.shift[c], P.a0.relu);
        else if (P.a0.relu) v = fmaxf(v, 0.f);
      }
      Xl[ch * DS + q] = v;
    }
    __syncthreads();
    const int a_base = (wm * 64 + l16) * DS + j;
    const int b_base = (wn * 64 + l16) * DS + j;
    for (int s = 0; s < 16; ++s) {
      float a[MT], b[NTB];
#pragma unroll
      for (int m = 0; m < MT; ++m) a[m] = Al[a_base + m * 16 * DS + 4 * s];
#pragma unroll
      for (int t = 0; t < NTB; ++t) b[t] = Xl[b_base + t * 16 * DS + 4 * s];
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NTB; ++t) acc[m][t] = mfma16(a[m], b[t], acc[m][t]);
    }
  }

  // ---- slab store: slab[split][m][ci] ------------------------------------------------------------
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int mr = m0 + wm * 64 + m * 16 + j * 4 + reg;
      if (mr < P.M) {
#pragma unroll
        for (int t = 0; t < NTB; ++t) {
          const int col = n0 + wn * 64 + t * 16 + l16;
          if (col < P.Ncols) P.slabs[((size_t)split * P.M + mr) * P.Ncols + col] = acc[m][t][reg];
        }
      }
    }
}

// -------------------------------------------------------------------------------------------------
// conv3x3 dW, LDS-DMA form.  Both operand tiles go HBM/L2 -> LDS with global_load_lds_dword (no VGPR
// staging).  One LDS image per block and two blocks per CU (<= 256 registers per lane): a block's DMA issue +
// flight is covered by the other block's MFMAs -- measured 16 % faster than one block per CU with a double-buffered
// image, where the 64-80 DMA issues per stage sit on the MFMA critical path.  The
// deferred BatchNorm+ReLU of the activation operand is applied after the ds_read, per lane (a lane's
// input channel is fixed): b = max(fma(raw, scale, shift), lo).  Zero padding / out-of-segment
// positions are DMA'd from a sentinel: quiet NaN for relu'd segments (max(NaN,0) = 0), 0 otherwise.
// -------------------------------------------------------------------------------------------------
__device__ const float gsd_pad[2] = {0.f, __builtin_nanf("")};

// KSP: <= 16 input channels: one 64 x 16ci tile, the 4 waves take every 4th k-step (each writes its own slab).
template <int WM, int WN, bool KSP>
__global__ __launch_bounds__(256, 2) void wgrad3x3_dma_kernel(const WgradParams P) {
  constexpr int MT = 4, NW = WM * WN;
  constexpr int BMw = WM * 64, BNw = KSP ? 16 : WN * 16, DS = 66;
  static_assert(NW == 4, "4 waves per block");
  static_assert(!KSP || WM == 1, "k-split form is for M <= 64 tiles");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int XS = P.PS;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6) & 3;   // MFMA sub-tile and share of the DMA work
  const int wm = KSP ? 0 : wave / WN, wn = KSP ? 0 : wave % WN;
  const int j = lane >> 4, l16 = lane & 15;

  // XCD-aware block order: the blocks of one split (same pixel range, different (m,n) tiles) read the same dy /
  // activation tiles, so they should share an L2.  Hardware deals blocks round-robin over the 8 XCDs (b and b+8
  // share one): give each XCD a contiguous range of logical ids (bijective for any grid size).  Speed only.
  const int lid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int per_split = P.mblocks * P.nblocks;
  const int split = lid / per_split;
  const int rem = lid - split * per_split;
  const int mb = rem % P.mblocks, nb = rem / P.mblocks;
  const int m0 = mb * BMw, n0 = nb * BNw;
  const int s_begin = (int)((long long)split * P.stages_total / P.splits);
  const int s_end = (int)((long long)(split + 1) * P.stages_total / P.splits);

  // lane geometry of the DMA
  const bool a_qin = lane < P.TH * P.TW;
  const int a_r = a_qin ? lane / P.TW : 0;
  const int a_c = a_qin ? lane - a_r * P.TW : 0;
  int b_rr[4], b_cc[4];
  bool b_ok[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int pos = p * 64 + lane;
    b_ok[p] = pos < P.WR * P.WC;
    b_rr[p] = pos / P.WC;
    b_cc[p] = pos - b_rr[p] * P.WC;
  }

  // per-lane transform of the B operand (lane's input channel is fixed)
  float sc = 1.f, sh = 0.f, lo = -__builtin_inff();
  {
    const int c = n0 + wn * 16 + l16;
    const bool first = c < P.a0.C;
    const SrcD& S = first ? P.a0 : P.a1;
    const int cc = first ? c : c - P.a0.C;
    if (c < P.Cact && cc < S.C) {
      if (S.scale != nullptr) {
        sc = S.scale[cc];
        sh = S.shift[cc];
      }
      if (S.relu) lo = 0.f;
    }
  }

  auto issue_dma = [&](int stage) {
    const int tpi = P.tiles_y * P.tiles_x;
    const int n = stage / tpi;
    const int rs = stage - n * tpi;
    const int ty = rs / P.tiles_x;
    const int h0 = ty * P.TH, w0 = (rs - ty * P.tiles_x) * P.TW;
    float* Ab = smem;
    float* Bb = Ab + BMw * DS;
    const bool pix_ok = a_qin && (h0 + a_r) < P.H && (w0 + a_c) < P.W;
    const float* abase = P.dy.p + (long long)n * P.dy.ns + (long long)(h0 + a_r) * P.dy.W + (w0 + a_c);
#pragma unroll 4
    for (int i = 0; i < BMw / 4; ++i) {
      const int row = wave + 4 * i;
      const int co = m0 + row;
      const float* g = (pix_ok && co < P.M) ? abase + (long long)co * P.dy.cs : &gsd_pad[0];
      __builtin_amdgcn_global_load_lds(g, Ab + row * DS, 4, 0, 0);
    }
#pragma unroll 2
    for (int i = 0; i < BNw / 4; ++i) {
      const int ch = wave + 4 * i;
      const int c = n0 + ch;
      const bool first = c < P.a0.C;
      const SrcD& S = first ? P.a0 : P.a1;
      const int cc = first ? c : c - P.a0.C;
      const bool c_ok = c < P.Cact && cc < S.C;
      const float* sentinel = (c_ok && S.relu) ? &gsd_pad[1] : &gsd_pad[0];
      const float* cbase = S.p + (long long)n * S.ns + (long long)cc * S.cs;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        if (b_ok[p]) {
          const int hs = h0 - 1 + b_rr[p] - S.oh, ws = w0 - 1 + b_cc[p] - S.ow;
          const bool ok = c_ok && (unsigned)hs < (unsigned)S.H && (unsigned)ws < (unsigned)S.W;
          const float* g = ok ? cbase + hs * S.W + ws : sentinel;
          __builtin_amdgcn_global_load_lds(g, Bb + ch * XS + p * 64, 4, 0, 0);
        }
      }
    }
  };

  f32x4 acc[MT][9];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (P.TH * P.TW) / 4;
  const int a_off = (wm * 64 + l16) * DS + j;
  const int b_off = BMw * DS + (wn * 16 + l16) * XS + j;

  auto compute = [&]() {
    if constexpr (KSP) {
      const float* Ab = smem + a_off;
      const float* Bb = smem + b_off;
      for (int s = wave; s < nk; s += 4) {
        const int q0 = 4 * s;
        const int r = q0 / P.TW, c = q0 - r * P.TW;
        const int xb = r * P.WC + c;
        float a[MT], b[9];
#pragma unroll
        for (int m = 0; m < MT; ++m) a[m] = Ab[m * 16 * DS + q0];
#pragma unroll
        for (int t = 0; t < 9; ++t) b[t] = fmaxf(fmaf(Bb[xb + (t / 3) * P.WC + (t % 3)], sc, sh), lo);
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int t = 0; t < 9; ++t) acc[m][t] = mfma16(a[m], b[t], acc[m][t]);
      }
      return;
    }
    const float* Ab = smem + a_off;
    const float* Bb = smem + b_off;
    int r = 0, c = 0;
    float an[MT], bn[9];
#pragma unroll
    for (int m = 0; m < MT; ++m) an[m] = Ab[m * 16 * DS];
#pragma unroll
    for (int t = 0; t < 9; ++t) bn[t] = Bb[(t / 3) * P.WC + (t % 3)];
    for (int s = 0; s < nk; ++s) {
      float a[MT], b[9];
#pragma unroll
      for (int m = 0; m < MT; ++m) a[m] = an[m];
#pragma unroll
      for (int t = 0; t < 9; ++t) b[t] = fmaxf(fmaf(bn[t], sc, sh), lo);
      c += 4;
      if (c >= P.TW) {
        c = 0;
        ++r;
      }
      {
        // next k-step's operands: issued before this k-step's MFMAs so their LDS latency hides behind them
        // (one wave per SIMD here: nobody else covers it).  Reading one step past the stage's last is harmless:
        // the addresses stay inside this buffer's LDS image and the values are never used.
        const int xb = r * P.WC + c;
        const int sn = (s + 1 < nk) ? s + 1 : s;
#pragma unroll
        for (int m = 0; m < MT; ++m) an[m] = Ab[m * 16 * DS + 4 * sn];
#pragma unroll
        for (int t = 0; t < 9; ++t) bn[t] = Bb[((s + 1 < nk) ? xb : 0) + (t / 3) * P.WC + (t % 3)];
      }
      // hipcc's own instruction order: faster at 2 waves per SIMD than sched_barrier fences or a sched_group_barrier interleave
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[m][t] = mfma16(a[m], b[t], acc[m][t]);
    }
  };

  const int nst = s_end - s_begin;
  for (int it = 0; it < nst; ++it) {
    gsd_dma_barrier();  // everyone left the image
    issue_dma(s_begin + it);
    gsd_dma_barrier();  // vmcnt(0) + barrier: the image is complete
    compute();
  }

  const int slab = KSP ? split * 4 + wave : split;
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int mr = m0 + wm * 64 + m * 16 + j * 4 + reg;
      if (mr < P.M) {
        const int col = n0 + wn * 16 + l16;
        if (col < P.Ncols) {
#pragma unroll
          for (int t = 0; t < 9; ++t)
            P.slabs[(((size_t)slab * 9 + t) * P.M + mr) * P.Ncols + col] = acc[m][t][reg];
        }
      }
    }
}

// ConvT2x2 dW, LDS-DMA form (default).  Same GEMM as convT_wgrad_kernel; both tiles go HBM/L2 -> LDS with
// global_load_lds_dword (one instruction = one 64-pixel row of the image; the space-to-depth gather of dy and the
// flat pixel -> (h, w) map live in the per-lane source address), one LDS image per block and two blocks per CU, so one
// block's DMA issue + flight is covered by the other's MFMAs.  The deferred BatchNorm+ReLU of x is applied after the
// ds_read (a lane owns four fixed input channels).  Measured against the register-staged kernel: see DESIGN.md.
// BX: the activation operand as aligned 16-byte pieces -- 64 consecutive pixels of a channel plane are 256 contiguous bytes
// (H * W % 4 == 0, 16-byte aligned strides): an instruction fills four channel rows, 8 instead of 32 instructions per wave and
// stage.  The rows are then contiguous in LDS (pitch 64), so piece q of row r is stored at slot q ^ (r & 15) (swizzle on the
// DMA's source piece and on the read) to keep the 16 rows of a read off one bank.
__device__ __attribute__((aligned(16))) const float gsd_zero16_wg[4] = {0.f, 0.f, 0.f, 0.f};
typedef float f32x2 __attribute__((ext_vector_type(2)));
// AX (XM == 2): the gradient operand as 16-byte pieces too.  Rows m = (co, kh, kw = 0 / 1) read the same stretch of dy row
// 2h + kh interleaved, so an LDS row holds a (co, kh) PAIR of m rows: 128 floats = 64 pixels x (kw 0, kw 1), a piece = two
// pixels; an instruction fills two such rows (four m rows): 8 instead of 32 instructions per wave and stage.  Slot q of row R
// holds source piece q ^ (R & 7) (eight rows a read touches -> eight bank groups).  A pixel pair that straddles the end of an
// image row (odd W only) gets its second pixel's two floats from a plain load issued beside the fills and written over the
// piece by the same lane once its fills have landed.
template <int XM>
__global__ __launch_bounds__(256, 2) void convT_wgrad_dma_kernel(const WgradParams P) {
  constexpr bool BX = XM >= 1, AX = XM == 2;
  constexpr int MT = 4, NTB = 4, BMw = 128, BNw = 128, DS = 66, DSB = BX ? 64 : DS;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Al = smem;
  float* Bl = smem + BMw * DS;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int j = lane >> 4, l16 = lane & 15;

  const int lid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int per_split = P.mblocks * P.nblocks;
  const int split = lid / per_split;
  const int rem = lid - split * per_split;
  const int mb = rem % P.mblocks, nb = rem / P.mblocks;
  const int m0 = mb * BMw, n0 = nb * BNw;
  const int s_begin = (int)((long long)split * P.stages_total / P.splits);
  const int s_end = (int)((long long)(split + 1) * P.stages_total / P.splits);
  const int HW = P.H * P.W;

  float sc[NTB], sh[NTB], lo[NTB];
#pragma unroll
  for (int t = 0; t < NTB; ++t) {
    const int c = n0 + wn * 64 + t * 16 + l16;
    sc[t] = 1.f; sh[t] = 0.f; lo[t] = -__builtin_inff();
    if (c < P.a0.C) {
      if (P.a0.scale != nullptr) { sc[t] = P.a0.scale[c]; sh[t] = P.a0.shift[c]; }
      if (P.a0.relu) lo[t] = 0.f;
    }
  }

  f32x4 acc[MT][NTB];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int t = 0; t < NTB; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int a_off = AX ? (wm * 32 + (l16 >> 1)) * 128 + 2 * (j & 1) + (l16 & 1) : (wm * 64 + l16) * DS + j;
  // AX loader role: lane = (row lr of the instruction's two (co, kh) rows, slot q of 32); rows R = 2 * (wave + 4 i) + lr, so
  // (R & 7) == (2 * wave + lr) & 7 for all of the wave's instructions
  const int a_lr = lane >> 5, a_q = lane & 31;
  const int a_sp = a_q ^ ((2 * wave + a_lr) & 7);   // source piece = pixel pair of the stage
  const int b_off = (wn * 64 + l16) * DSB + j;   // BX: rows wn*64 + t*16 + l16: (row & 15) == l16
  // BX loader role: lane = (row lr of the instruction's four, slot q); the wave's instructions cover rows 4*(wave + 4 i) + lr,
  // so (row & 15) == (4 * wave + lr) & 15 for all of them; the lane fetches source piece q ^ (row & 15)
  const int b_lr = lane >> 4;
  const int b_piece = (lane & 15) ^ ((4 * wave + b_lr) & 15);
  for (int stage = s_begin; stage < s_end; ++stage) {
    const int n = stage / P.tiles_flat;
    const int p = (stage - n * P.tiles_flat) * 64 + lane;
    const bool pix_ok = p < HW;
    const int h = pix_ok ? p / P.W : 0;
    const int w = pix_ok ? p - h * P.W : 0;
    __syncthreads();   // every wave has finished reading the previous stage's image
    f32x2 a_fix[AX ? BMw / 16 : 1];
    bool a_str = false;
    if constexpr (AX) {
      const int pa = (stage - n * P.tiles_flat) * 64 + 2 * a_sp;   // first pixel of this lane's pair
      const bool pa_ok = pa < HW;
      const int ha = pa_ok ? pa / P.W : 0, wa = pa_ok ? pa - ha * P.W : 0;
      a_str = pa_ok && wa == P.W - 1;                              // the pair's second pixel starts the next image row
      const bool pb_ok = pa + 1 < HW;
      const float* abase = P.dy.p + (long long)n * P.dy.ns + (long long)(2 * ha) * P.dy.W + 2 * wa;
#pragma unroll
      for (int i = 0; i < BMw / 16; ++i) {
        const int R = 2 * (wave + 4 * i) + a_lr;      // (co, kh) row of the block
        const int m = m0 + 2 * R;
        const float* src = abase + (long long)(m >> 2) * P.dy.cs + ((m >> 1) & 1) * P.dy.W;
        const float* gsrc = (pa_ok && m < P.M) ? src : &gsd_zero16_wg[0];
        float* dstp = Al + (wave + 4 * i) * 256;
        __builtin_amdgcn_global_load_lds(gsrc, dstp, 16, 0, 0);
        a_fix[i] = f32x2{0.f, 0.f};
        if (a_str && pb_ok && m < P.M) a_fix[i] = *reinterpret_cast<const f32x2*>(src + 2 * P.dy.W - 2 * wa);   // row 2(ha+1)+kh, column 0
      }
    } else {
      const float* abase = P.dy.p + (long long)n * P.dy.ns + (long long)(2 * h) * P.dy.W + 2 * w;
#pragma unroll 4
      for (int i = 0; i < BMw / 4; ++i) {
        const int row = wave + 4 * i;           // m = (co, kh, kw)
        const int m = m0 + row;
        const float* gsrc = (pix_ok && m < P.M) ? abase + (long long)(m >> 2) * P.dy.cs + ((m >> 1) & 1) * P.dy.W + (m & 1) : &gsd_pad[0];
        __builtin_amdgcn_global_load_lds(gsrc, Al + row * DS, 4, 0, 0);
      }
    }
    if constexpr (BX) {
      const int p0 = (stage - n * P.tiles_flat) * 64 + 4 * b_piece;   // first pixel of this lane's piece (H * W % 4 == 0)
      const bool pc_ok = p0 < HW;
      const float* bbase = P.a0.p + (long long)n * P.a0.ns + p0;
#pragma unroll 4
      for (int i = 0; i < BNw / 16; ++i) {
        const int ch = 4 * (wave + 4 * i) + b_lr;
        const int c = n0 + ch;
        const float* gsrc = (pc_ok && c < P.a0.C) ? bbase + (long long)c * P.a0.cs : &gsd_zero16_wg[0];
        float* dstp = Bl + (wave + 4 * i) * (4 * DSB);
        __builtin_amdgcn_global_load_lds(gsrc, dstp, 16, 0, 0);
      }
    } else {
      const float* bbase = P.a0.p + (long long)n * P.a0.ns + p;
#pragma unroll 4
      for (int i = 0; i < BNw / 4; ++i) {
        const int ch = wave + 4 * i;
        const int c = n0 + ch;
        const float* gsrc = (pix_ok && c < P.a0.C) ? bbase + (long long)c * P.a0.cs : &gsd_pad[0];
        __builtin_amdgcn_global_load_lds(gsrc, Bl + ch * DS, 4, 0, 0);
      }
    }
    if constexpr (AX) {
      __builtin_amdgcn_s_waitcnt(0x0F70);   // this wave's fills (and the plain loads behind them) have landed
      if (a_str) {
#pragma unroll
        for (int i = 0; i < BMw / 16; ++i)
          *reinterpret_cast<f32x2*>(&Al[(wave + 4 * i) * 256 + lane * 4 + 2]) = a_fix[i];
      }
      __syncthreads();
    } else {
      gsd_dma_barrier();   // vmcnt(0) + barrier: the image is complete
    }
    float an[MT], bn[NTB];
#pragma unroll
    for (int m = 0; m < MT; ++m) an[m] = AX ? Al[a_off + m * 8 * 128 + 4 * ((j >> 1) ^ (l16 >> 1))] : Al[a_off + m * 16 * DS];
#pragma unroll
    for (int t = 0; t < NTB; ++t) bn[t] = Bl[b_off + t * 16 * DSB + (BX ? 4 * l16 : 0)];   // BX: piece 0 sits in slot 0 ^ l16
    for (int s = 0; s < 16; ++s) {
      float a[MT], b[NTB];
#pragma unroll
      for (int m = 0; m < MT; ++m) a[m] = an[m];
#pragma unroll
      for (int t = 0; t < NTB; ++t) b[t] = fmaxf(fmaf(bn[t], sc[t], sh[t]), lo[t]);
      const int sn = s + 1 < 16 ? s + 1 : s;   // next k-step's operands before this k-step's MFMAs
#pragma unroll
      for (int m = 0; m < MT; ++m)
        an[m] = AX ? Al[a_off + m * 8 * 128 + 4 * ((2 * sn + (j >> 1)) ^ (l16 >> 1))] : Al[a_off + m * 16 * DS + 4 * sn];
#pragma unroll
      for (int t = 0; t < NTB; ++t) bn[t] = Bl[b_off + t * 16 * DSB + 4 * (BX ? (sn ^ l16) : sn)];
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NTB; ++t) acc[m][t] = mfma16(a[m], b[t], acc[m][t]);
    }
  }
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int mr = m0 + wm * 64 + m * 16 + j * 4 + reg;
      if (mr < P.M) {
#pragma unroll
        for (int t = 0; t < NTB; ++t) {
          const int col = n0 + wn * 64 + t * 16 + l16;
          if (col < P.Ncols) P.slabs[((size_t)split * P.M + mr) * P.Ncols + col] = acc[m][t][reg];
        }
      }
    }
}

// Sum the slabs in split order and write the reference layout.
//   MODE 0: slab[split][tap][co][ci] -> dW[co][ci][tap]
//   MODE 1: slab[split][m][ci]       -> dW[ci][m]          (m = co*4+kh*2+kw)
// LANES split lanes per element (block = 64 elements x LANES): the launches with few output elements are the ones with
// hundreds of slabs (the 3-channel first layer: 1,728 elements x 2,048 slabs), which one thread per element walks serially.
template <int MODE, int LANES>
__global__ __launch_bounds__(LANES == 1 ? 256 : 64 * LANES) void wgrad_reduce_kernel(const float* __restrict__ slabs,
                                                                                     float* __restrict__ dw, int splits, int M,
                                                                                     int Ncols) {
  constexpr int EL = LANES == 1 ? 256 : 64;
  const long long per = (long long)(MODE == 0 ? 9 : 1) * M * Ncols;
  const int el = threadIdx.x % EL, sl = threadIdx.x / EL;
  __shared__ float red[LANES][EL];
  for (long long e0 = (long long)blockIdx.x * EL; e0 < per; e0 += (long long)gridDim.x * EL) {
    const long long e = e0 + el;
    const bool ok = e < per;
    float s = 0.f;
    if (ok)
      for (int k = sl; k < splits; k += LANES) s += slabs[(size_t)k * per + e];
    if (LANES > 1) {
      red[sl][el] = s;
      __syncthreads();
      if (sl == 0) {
        s = 0.f;
#pragma unroll
        for (int i = 0; i < LANES; ++i) s += red[i][el];
      }
    }
    if (sl == 0 && ok) {
      const int col = (int)(e % Ncols);
      const long long t2 = e / Ncols;
      const int mr = (int)(t2 % M);
      if (MODE == 0) {
        const int tap = (int)(t2 / M);
        dw[((size_t)mr * Ncols + col) * 9 + tap] = s;
      } else {
        dw[(size_t)col * M + mr] = s;
      }
    }
    if (LANES > 1) __syncthreads();
  }
}

template <int MODE>
void launch_wgrad_reduce(const float* slabs, float* dw, int splits, int M, int Ncols, hipStream_t st) {
  const long long per = (long long)(MODE == 0 ? 9 : 1) * M * Ncols;
  if (splits >= 64) {
    const int g = (int)(ceil_div64(per, 64) < 8192 ? ceil_div64(per, 64) : 8192);
    hipLaunchKernelGGL((wgrad_reduce_kernel<MODE, 16>), dim3(g), dim3(1024), 0, st, slabs, dw, splits, M, Ncols);
  } else if (splits >= 8) {
    const int g = (int)(ceil_div64(per, 64) < 8192 ? ceil_div64(per, 64) : 8192);
    hipLaunchKernelGGL((wgrad_reduce_kernel<MODE, 4>), dim3(g), dim3(256), 0, st, slabs, dw, splits, M, Ncols);
  } else {
    const int g = (int)(ceil_div64(per, 256) < 4096 ? ceil_div64(per, 256) : 4096);
    hipLaunchKernelGGL((wgrad_reduce_kernel<MODE, 1>), dim3(g), dim3(256), 0, st, slabs, dw, splits, M, Ncols);
  }
}

// out[k] = sum_{n, p} x[n][k][p]  -- two deterministic stages (G=64 groups per channel).
__global__ void sum_planes_stage1(const float* __restrict__ x, int N, int K, long long HW, float* __restrict__ ws) {
  const int k = blockIdx.x, g = blockIdx.y, G = gridDim.y;
  const long long total = (long long)N * HW;
  const long long per = (total + G - 1) / G;
  const long long b = (long long)g * per, e = b + per < total ? b + per : total;
  double s = 0.0;
  // (image, pixel) carried along instead of a 64-bit division per element: the same elements in the same order
  long long i = b + threadIdx.x;
  long long n = i / HW, p = i - n * HW;
  const long long step = blockDim.x, nstep = step / HW, pstep = step - nstep * HW;
  for (; i < e; i += step) {
    s += (double)x[((size_t)n * K + k) * HW + p];
    n += nstep;
    p += pstep;
    if (p >= HW) {
      p -= HW;
      ++n;
    }
  }
  __shared__ double red[16];   // up to 1024 threads: with few planes (the output conv: K = 1) the 64 blocks are all there is
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
    ws[(size_t)k * G + g] = (float)t;
  }
}
__global__ void sum_planes_stage2(const float* __restrict__ ws, int K, int G, float* __restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < K) {
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += (double)ws[(size_t)k * G + g];
    out[k] = (float)s;
  }
}

namespace {

void choose_wgrad_tile(int H, int W, int* TH, int* TW) {
  // Stage = TH x TW pixels, TH*TW <= 64, TW % 4 == 0, halo window <= 256 positions.  First the least MFMA work
  // (stages * pixels per stage); then the WIDEST rows: a DMA instruction that covers one 256-byte row segment is
  // measurably faster than one that covers two 128-byte segments (TH 2 x TW 32 was 13 % slower than 1 x 64 although
  // its halo traffic is a third lower) -- the cost is per cache line touched, not per byte; preferring the least halo
  // traffic instead measured slower.
  long min_work = -1;
  for (int pass = 0; pass < 2; ++pass) {
    long best = -1;
    for (int tw = 4; tw <= 64; tw += 4) {
      int th = 64 / tw;
      if (th > H) th = H;
      while (th > 1 && (th + 2) * (tw + 2) > 256) --th;
      if ((th + 2) * (tw + 2) > 256) continue;
      const int ty = ceil_div(H, th);
      th = ceil_div(H, ty);
      const long stages = (long)ty * ceil_div(W, tw);
      const long work = stages * (long)(th * tw);
      if (pass == 0) {
        if (min_work < 0 || work < min_work) min_work = work;
        continue;
      }
      if (work * 100 > min_work * 103) continue;
      const long cost = work * 1000 + stages * 10 - tw;
      if (best < 0 || cost < best) {
        best = cost;
        *TH = th;
        *TW = tw;
      }
    }
  }
}

int plane_stride_2mod32(int n) {
  int ps = (n / 32) * 32 + 2;
  if (ps < n) ps += 32;
  return ps;
}

struct WgradPlan {
  bool ksplit;  // conv3x3 with <= 16 input channels and M <= 64: one 64 x 16 tile, waves split the pixels
  bool wide;  // WM=1,WN=4 (M<=64) else WM=2,WN=2
  int BMw, BNw, mblocks, nblocks, TH, TW, tiles_y, tiles_x, tiles_flat, stages_total, splits;
  int64_t slab_elems;
};

WgradPlan plan_wgrad(int mode, int N, int H, int W, int M, int Ncols) {
  WgradPlan p;
  p.wide = M <= 64;
  p.ksplit = mode == 0 && p.wide && Ncols <= 16;
  p.BMw = p.wide ? 64 : 128;
  const int WN = p.wide ? 4 : 2;
  p.BNw = mode == 0 ? (p.ksplit ? 16 : WN * 16) : WN * 64;
  p.mblocks = ceil_div(M, p.BMw);
  p.nblocks = ceil_div(Ncols, p.BNw);
  p.TH = p.TW = p.tiles_y = p.tiles_x = p.tiles_flat = 0;
  if (mode == 0) {
    choose_wgrad_tile(H, W, &p.TH, &p.TW);
    p.tiles_y = ceil_div(H, p.TH);
    p.tiles_x = ceil_div(W, p.TW);
    p.stages_total = N * p.tiles_y * p.tiles_x;
  } else {
    p.tiles_flat = ceil_div(H * W, 64);
    p.stages_total = N * p.tiles_flat;
  }
  const int tiles = p.mblocks * p.nblocks;
  const int target3 = gsd_env_int("GSD_WGRAD_BLOCKS", 512);   // tuning knob (512: one round of 2 blocks/CU; 1024 measured 1 % slower end to end)
  int splits = ceil_div(target3, tiles);   // one round of 2 resident blocks per CU x 256 CUs
  if (splits > p.stages_total) splits = p.stages_total;
  if (splits > 2048) splits = 2048;
  if (splits < 1) splits = 1;
  p.splits = splits;
  // conv3x3: 9 taps per slab, and the k-split form writes one slab per wave
  p.slab_elems = (int64_t)splits * (mode == 0 ? (p.ksplit ? 36 : 9) : 1) * M * Ncols;
  return p;
}

int check_plain(const gsd_src& s, const char* what) {
  GSD_REQUIRE(s.ptr != nullptr && s.scale == nullptr && s.shift == nullptr && s.relu == 0 && s.off_h == 0 &&
                  s.off_w == 0,
              GSD_ERR_BAD_ARG, "%s: gradient operand must be a plain tensor", what);
  GSD_REQUIRE(s.w_stride >= s.W && s.c_stride >= (int64_t)s.H * s.w_stride && s.n_stride >= s.c_stride, GSD_ERR_BAD_ARG,
              "%s: strides too small", what);
  return 0;
}

}  // namespace

extern "C" int64_t gsd_conv3x3_wgrad_workspace(int N, int H, int W, int Cin, int Cout) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
  const int64_t direct = plan_wgrad(0, N, H, W, Cout, Cin).slab_elems, wino = gsd_wgrad_w43_workspace(N, H, W, Cin, Cout);
  const int64_t w2d = gsd_wgrad_w2d_workspace(N, H, W, Cin, Cout);
  const int64_t m = direct > wino ? direct : wino;   // any form may serve the call (GSD_WGRAD_ALGO, GSD_WGRAD_W2D, the operands)
  return m > w2d ? m : w2d;
}

extern "C" int gsd_conv3x3_wgrad_form(const gsd_src* a, int nsrc, const gsd_src* dy, int Cin, int Cout, int N, int H, int W) {
  if (!a || !dy || nsrc < 1 || nsrc > 2 || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
  if (!gsd_wgrad_w43_use(N, H, W, Cin, Cout)) return 0;
  return gsd_wgrad_w2d_use(a, nsrc, dy, Cin, Cout, N, H, W) ? 2 : 1;
}

// 1 when gsd_conv3x3_wgrad serves this shape with a kernel that takes PITCHED activation segments (w_stride > W): the Winograd forms
extern "C" int gsd_conv3x3_wgrad_takes_pitched_act(int N, int H, int W, int Cin, int Cout) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
  return gsd_wgrad_w43_use(N, H, W, Cin, Cout) ? 1 : 0;
}

extern "C" int64_t gsd_conv3x3_wgrad_mfma_count(int form, int N, int H, int W, int Cin, int Cout) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
  if (form == 2) return gsd_wgrad_w2d_mfma_count(N, H, W, Cin, Cout);
  if (form == 1) return gsd_wgrad_w43_mfma_count(N, H, W, Cin, Cout);
  return 0;
}

extern "C" int gsd_conv3x3_wgrad(const gsd_src* a, int nsrc, const gsd_src* dy, int Cin, int Cout, float* dw,
                                 float* workspace, int64_t workspace_elems, int N, int H, int W, void* stream) {
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
  // the two Winograd kernels address activation rows through w_stride and mask by W (a pitched activation or concat buffer is
  // read in place); the direct form's rows must be contiguous
  for (int i = 0; i < nsrc; ++i) {
    GSD_REQUIRE(a[i].w_stride >= a[i].W && a[i].c_stride >= (int64_t)a[i].H * a[i].w_stride && a[i].n_stride >= a[i].c_stride,
                GSD_ERR_BAD_ARG, "gsd_conv3x3_wgrad: activation segment %d: strides too small", i);
    if (!gsd_conv3x3_wgrad_takes_pitched_act(N, H, W, Cin, Cout))
      if (int e = gsd_require_rows_contiguous(a[i], "gsd_conv3x3_wgrad activation (direct form)")) return e;
  }
  if (int e = check_plain(*dy, "gsd_conv3x3_wgrad dy")) return e;
  // dy may be pitched (w_stride > W) for the Winograd form, which then moves it as aligned 16-byte pieces
  if (!gsd_wgrad_w43_use(N, H, W, Cin, Cout))
    if (int e = gsd_require_rows_contiguous(*dy, "gsd_conv3x3_wgrad dy (direct form)")) return e;
  GSD_REQUIRE(dy->C == Cout && dy->H == H && dy->W == W, GSD_ERR_BAD_ARG, "gsd_conv3x3_wgrad: dy must be (Cout,H,W)");
  for (int i = 0; i < nsrc; ++i)
    GSD_REQUIRE(a[i].scale == nullptr || a[i].relu != 0, GSD_ERR_UNSUPPORTED,
                "gsd_conv3x3_wgrad: an affine activation segment must also have relu (zero padding uses a NaN sentinel)");
  GSD_REQUIRE(workspace_elems >= gsd_conv3x3_wgrad_workspace(N, H, W, Cin, Cout), GSD_ERR_WORKSPACE,
              "gsd_conv3x3_wgrad: workspace %lld < %lld elements", (long long)workspace_elems,
              (long long)gsd_conv3x3_wgrad_workspace(N, H, W, Cin, Cout));
  if (gsd_wgrad_w43_use(N, H, W, Cin, Cout)) {
    if (gsd_wgrad_w2d_use(a, nsrc, dy, Cin, Cout, N, H, W)) {
      int splits = 0;
      if (int e = gsd_wgrad_w2d_run(a, nsrc, dy, Cin, Cout, workspace, workspace_elems, N, H, W, &splits, stream)) return e;
      return gsd_wgrad_w43_reduce_run(workspace, dw, splits, Cout, Cin, stream);
    }
    return gsd_wgrad_w43_run(a, nsrc, dy, Cin, Cout, dw, workspace, workspace_elems, N, H, W, stream);
  }
  WgradPlan pl = plan_wgrad(0, N, H, W, Cout, Cin);
  GSD_REQUIRE(workspace_elems >= pl.slab_elems, GSD_ERR_WORKSPACE, "gsd_conv3x3_wgrad: workspace %lld < %lld elements",
              (long long)workspace_elems, (long long)pl.slab_elems);
  WgradParams P;
  P.a0 = to_srcd(a[0]);
  P.a1 = nsrc > 1 ? to_srcd(a[1]) : null_srcd();
  P.dy = to_srcd(*dy);
  P.slabs = workspace;
  P.M = Cout; P.Ncols = Cin; P.Cact = Cin;
  P.N = N; P.H = H; P.W = W;
  P.TH = pl.TH; P.TW = pl.TW; P.tiles_y = pl.tiles_y; P.tiles_x = pl.tiles_x;
  P.WR = pl.TH + 2; P.WC = pl.TW + 2;
  P.PS = plane_stride_2mod32(P.WR * P.WC);
  P.tiles_flat = 0;
  P.stages_total = pl.stages_total; P.splits = pl.splits; P.mblocks = pl.mblocks; P.nblocks = pl.nblocks;
  const int grid = pl.splits * pl.mblocks * pl.nblocks;
  const size_t lds = (size_t)(pl.BMw * 66 + pl.BNw * P.PS) * sizeof(float);
  for (int i = 0; i < nsrc; ++i)
    GSD_REQUIRE(a[i].scale == nullptr || a[i].relu != 0, GSD_ERR_UNSUPPORTED,
                "gsd_conv3x3_wgrad: an affine activation segment must also have relu (zero padding uses a NaN sentinel)");
  const int nslabs = pl.ksplit ? 4 * pl.splits : pl.splits;
  const char* const what = "gsd_conv3x3_wgrad";
  const hipStream_t st = (hipStream_t)stream;
  if (int e = pl.ksplit ? gsd_launch<wgrad3x3_dma_kernel<1, 4, true>>(what, dim3(grid), dim3(256), lds, st, P)
              : pl.wide ? gsd_launch<wgrad3x3_dma_kernel<1, 4, false>>(what, dim3(grid), dim3(256), lds, st, P)
                        : gsd_launch<wgrad3x3_dma_kernel<2, 2, false>>(what, dim3(grid), dim3(256), lds, st, P))
    return e;
  launch_wgrad_reduce<0>(workspace, dw, nslabs, Cout, Cin, (hipStream_t)stream);
  GSD_LAUNCH_CHECK("gsd_conv3x3_wgrad reduce");
  return GSD_OK;
}

extern "C" int64_t gsd_convT2x2_wgrad_workspace(int N, int H, int W, int Cin, int Cout) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
  return plan_wgrad(1, N, H, W, Cout * 4, Cin).slab_elems + (int64_t)Cout * 64;
}

extern "C" int gsd_convT2x2_wgrad(const gsd_src* x, const gsd_src* dy, int Cin, int Cout, float* dw, float* dbias,
                                  float* workspace, int64_t workspace_elems, int N, int H, int W, void* stream) {
  GSD_REQUIRE(x && dy && dw && workspace, GSD_ERR_BAD_ARG, "gsd_convT2x2_wgrad: null argument");
  GSD_REQUIRE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, GSD_ERR_BAD_ARG, "gsd_convT2x2_wgrad: bad sizes");
  GSD_REQUIRE(x->ptr != nullptr && x->C == Cin && x->H == H && x->W == W && x->off_h == 0 && x->off_w == 0,
              GSD_ERR_BAD_ARG, "gsd_convT2x2_wgrad: x must be the full (Cin,H,W) tensor");
  GSD_REQUIRE((x->scale == nullptr) == (x->shift == nullptr), GSD_ERR_BAD_ARG,
              "gsd_convT2x2_wgrad: scale/shift must come together");
  if (int e = check_plain(*dy, "gsd_convT2x2_wgrad dy")) return e;
  if (int e = gsd_require_rows_contiguous(*dy, "gsd_convT2x2_wgrad dy")) return e;
  if (int e = gsd_require_rows_contiguous(*x, "gsd_convT2x2_wgrad x")) return e;
  GSD_REQUIRE(dy->C == Cout && dy->H == 2 * H && dy->W == 2 * W, GSD_ERR_BAD_ARG,
              "gsd_convT2x2_wgrad: dy must be (Cout,2H,2W)");
  GSD_REQUIRE(((uintptr_t)dy->ptr & 7) == 0 && (dy->c_stride & 1) == 0 && (dy->n_stride & 1) == 0, GSD_ERR_UNSUPPORTED,
              "gsd_convT2x2_wgrad: dy must be 8-byte aligned with even strides");
  const int M = Cout * 4;
  WgradPlan pl = plan_wgrad(1, N, H, W, M, Cin);
  const int64_t need = pl.slab_elems + (int64_t)Cout * 64;
  GSD_REQUIRE(workspace_elems >= need, GSD_ERR_WORKSPACE, "gsd_convT2x2_wgrad: workspace %lld < %lld elements",
              (long long)workspace_elems, (long long)need);
  WgradParams P;
  P.a0 = to_srcd(*x);
  P.a1 = null_srcd();
  P.dy = to_srcd(*dy);
  P.slabs = workspace;
  P.M = M; P.Ncols = Cin; P.Cact = Cin;
  P.N = N; P.H = H; P.W = W;
  P.TH = P.TW = P.tiles_y = P.tiles_x = P.WR = P.WC = P.PS = 0;
  P.tiles_flat = pl.tiles_flat;
  P.stages_total = pl.stages_total; P.splits = pl.splits; P.mblocks = pl.mblocks; P.nblocks = pl.nblocks;
  const int grid = pl.splits * pl.mblocks * pl.nblocks;
  const size_t lds = (size_t)(pl.BMw * 66 + pl.BNw * 66) * sizeof(float);
  // activation rows as aligned 16-byte pieces when 64 consecutive pixels of a plane are 256 aligned bytes
  const bool bx = gsd_env_int("GSD_CONVT_WG_BX", 1) != 0 && (H * W) % 4 == 0 && ((uintptr_t)x->ptr & 15) == 0 &&
                  x->c_stride % 4 == 0 && x->n_stride % 4 == 0;
  // ... and the gradient rows as 16-byte pieces of dy rows (8-byte aligned pixel pairs: dy is 8-byte aligned with even strides)
  const bool ax = bx && gsd_env_int("GSD_CONVT_WG_AX", 1) != 0;
  const char* const what = "gsd_convT2x2_wgrad";
  const hipStream_t st = (hipStream_t)stream;
  // (wide: M = 4*Cout <= 64, never the case for this network; the register-staged kernel keeps it working)
  if (int e = pl.wide ? gsd_launch<convT_wgrad_kernel<1, 4>>(what, dim3(grid), dim3(256), lds, st, P)
              : ax    ? gsd_launch<convT_wgrad_dma_kernel<2>>(what, dim3(grid), dim3(256), lds, st, P)
              : bx    ? gsd_launch<convT_wgrad_dma_kernel<1>>(what, dim3(grid), dim3(256), lds, st, P)
                      : gsd_launch<convT_wgrad_dma_kernel<0>>(what, dim3(grid), dim3(256), lds, st, P))
    return e;
  launch_wgrad_reduce<1>(workspace, dw, pl.splits, M, Cin, (hipStream_t)stream);
  GSD_LAUNCH_CHECK("gsd_convT2x2_wgrad reduce");
  if (dbias != nullptr) {
    GSD_REQUIRE(dy->c_stride == (int64_t)4 * H * W && dy->n_stride == (int64_t)Cout * 4 * H * W, GSD_ERR_UNSUPPORTED,
                "gsd_convT2x2_wgrad: bias gradient needs a contiguous dy");
    float* ws2 = workspace + pl.slab_elems;
    hipLaunchKernelGGL(sum_planes_stage1, dim3(Cout, 64), dim3(256), 0, (hipStream_t)stream, dy->ptr, N, Cout,
                       (long long)4 * H * W, ws2);
    GSD_LAUNCH_CHECK("gsd_convT2x2_wgrad bias stage1");
    hipLaunchKernelGGL(sum_planes_stage2, dim3(ceil_div(Cout, 256)), dim3(256), 0, (hipStream_t)stream, ws2, Cout, 64,
                       dbias);
    GSD_LAUNCH_CHECK("gsd_convT2x2_wgrad bias stage2");
  }
  return GSD_OK;
}

extern "C" int gsd_sum_planes(const float* x, int N, int K, int64_t HW, float* out, float* workspace, void* stream) {
  GSD_REQUIRE(x && out && workspace && N > 0 && K > 0 && HW > 0, GSD_ERR_BAD_ARG, "gsd_sum_planes: bad argument");
  hipLaunchKernelGGL(sum_planes_stage1, dim3(K, 64), dim3(K <= 8 ? 1024 : 256), 0, (hipStream_t)stream, x, N, K, (long long)HW, workspace);
  GSD_LAUNCH_CHECK("gsd_sum_planes stage1");
  hipLaunchKernelGGL(sum_planes_stage2, dim3(ceil_div(K, 256)), dim3(256), 0, (hipStream_t)stream, workspace, K, 64, out);
  GSD_LAUNCH_CHECK("gsd_sum_planes stage2");
  return GSD_OK;
}
