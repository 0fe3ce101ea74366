// gsd_conv3x3_w43.hip -- conv3x3 (pad 1, stride 1, no bias) forward and dX with the Winograd minimal-filtering
// identity F(4,3) applied ALONG THE IMAGE ROWS, on v_mfma_f32_16x16x4_f32 (gfx950).
//
// Same operator as gsd_conv3x3.hip (aten::convolution at /root/reference/gelslim_depth/models/unet.py:11,14 and the dX
// half of aten::convolution_backward), same fp32 storage and fp32 accumulation, half the multiplications: four
// horizontally adjacent outputs of one kernel row need 6 products instead of 12,
//
//   y[0..3] = A^T [ (G g) .* (B^T d) ],   d = 6 consecutive inputs of the row, g = the 3 taps of one kernel row,
//
// and the three kernel rows and the input channels are the contraction that stays on the MFMA:
//
//   M_f[m][tile] = sum_{ci, r} U_f[(ci,r)][m] * V_f[(ci,r)][tile],   f = 0..5
//
// i.e. six GEMMs with K = 3*Cin instead of one with K = 9*Cin, over N = pixels/4 "tiles".  Accumulators: 6 per 4
// pixels (1.5x the direct form).  U = G g is computed once per optimiser step by gsd_weight_layout (modes 4/5), V = B^T d
// by the consumer lanes between the ds_read and the MFMA (13 VALU operations per 6 values, next to the deferred
// BatchNorm+ReLU that is already applied there), y = A^T M in the epilogue.  F(4,3) in one dimension is numerically
// benign in fp32 (largest transform constants 8 and 1/24): the op-level tests bound it at 1e-5 relative L1 against
// the fp64 oracle, two orders below the 1e-3 north-star tolerance.
//
// Block = 4 waves, all on the same 64 output channels; each wave owns 16 tiles = 64 pixels: block tile 64 (m) x 256
// pixels.  Per 4-channel chunk a wave issues 18 k-steps (3 kernel rows x 6 frequencies) x 4 MFMAs; the weight image
// of a chunk is 72 x 64 floats = 18 KiB, exactly the direct kernel's (36 x 128), and it is amortised over 256 pixels
// so the L2 -> LDS rate per MFMA-second equals the direct 128 x 128 kernel's although the MFMA time halves.
// Data movement, deferred BatchNorm, NaN-sentinel padding, concat sources, two cropped destinations, BatchNorm
// partial sums and the fused BatchNorm-backward dX epilogue are those of gsd_conv3x3.hip.
#include "gsd_conv3x3_host.h"

#include <cstdlib>

__device__ const float gsd_pad_w43[2] = {0.f, __builtin_nanf("")};
__device__ __attribute__((aligned(16))) const float gsd_pad16_w43[8] = {0.f, 0.f, 0.f, 0.f, __builtin_nanf(""), __builtin_nanf(""),
                                                                          __builtin_nanf(""), __builtin_nanf("")};

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct W43Params {
  SrcD src0, src1;
  DstD dst0, dst1;
  const float* wt;   // [mblocks][nchunks*72][64]: row (ci_local*18 + r*6 + f), columns permuted (slot l*4+t = column t*16+l)
  float* partials;
  const float* bw_raw;
  const float* bw_scale;
  const float* bw_shift;
  const float* bw_mean;
  const float* bw_invstd;
  int Cin, Cout, Mpad, nchunks, mblocks;
  int N, H, W;
  int TH, TW, TWq, tiles_y, tiles_x, WR, WC, WCp, PS, NPV;
  int NP, RPI, NI, RO;   // 16-byte halo pieces (X4): pieces per window row, rows per DMA instruction, instructions per plane, read offset
  int fold;              // tile rows run over the padded flat rows of the whole batch (see w43_row)
  int nslab;             // K-slab form (SPLIT): the block's channel chunks are slab k's share, its y goes to `slabs`
  float* slabs;          // [nslab][tile blocks][64 channels][64 Winograd tiles][4 pixels]: un-reduced outputs of the K slabs
};

namespace {
constexpr int W43_BM = 64;
constexpr int W43_WTILE = 72 * W43_BM;      // floats per weight chunk
constexpr int W43_W4 = W43_WTILE / 4;       // float4s
constexpr int W43_NWI = (W43_W4 + 255) / 256;
}  // namespace

// Row folding (small images): a 20 x 26 image fills a 64-tile block to 68 %.  With P.fold the tile grid runs over the
// "padded flat rows" of the WHOLE batch, rho = n * (H + 1) + h + 1: row n * (H + 1) is a zero row that serves as the bottom
// padding of image n-1 and as the top padding of image n, so a block's halo window is still TH + 2 consecutive rows and
// nothing else in the kernel changes -- a block simply covers the tail of one image and the head of the next.  Returns the
// image and the row inside it (-1: a zero row or a row past the batch).
__device__ __forceinline__ void w43_row(const W43Params& P, int n, int rho, int& nn, int& hh) {
  if (!P.fold) {
    nn = n;
    hh = rho;
    return;
  }
  nn = rho >= 0 ? rho / (P.H + 1) : 0;
  hh = (rho >= 0 && nn < P.N) ? rho - nn * (P.H + 1) - 1 : -1;
  if (nn >= P.N) nn = 0;
}

// Epilogue shared by the convolution kernel (y = A^T M of its accumulators) and the K-slab reducer (y = sum of the slabs' tiles): NCHW
// stores into two destination segments with crop, BatchNorm partial sums, or the fused BatchNorm-backward form.  The lane owns the
// four pixels (h_t, w0 + 4 tq ..) of image n_t (fold) / n for the 16 output channels m0 + m * 16 + j * 4 + reg.
template <class GetY>
__device__ __forceinline__ void w43_epilogue(const W43Params& P, int n, int pt, int wave, int wm, int m0, int j, int l16,
                                             int n_t, int h_t, int w0, int tq, int vmask, const float* sBw, GetY&& get_y) {
  constexpr int MT = 4, BM = W43_BM;
  // ---- epilogue: y = A^T M, NCHW stores (two destination segments with crop), BatchNorm partial sums ----------------------
  // per destination: element offset of the tile's first pixel inside a plane, and the mask of its pixels that are stored
  int off0 = 0, off1 = 0, sm0 = 0, sm1 = 0;
  {
    const int h = h_t, w = w0 + 4 * tq;
    const int fo0 = P.fold ? n_t * (int)P.dst0.ns : 0, fo1 = P.fold ? n_t * (int)P.dst1.ns : 0;
    int hd = h - P.dst0.oh, wd = w - P.dst0.ow;
    if (h >= 0 && (unsigned)hd < (unsigned)P.dst0.H) {
      off0 = fo0 + hd * P.dst0.ws + wd;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if ((vmask >> i & 1) && (unsigned)(wd + i) < (unsigned)P.dst0.W) sm0 |= 1 << i;
    }
    hd = h - P.dst1.oh;
    wd = w - P.dst1.ow;
    if (h >= 0 && (unsigned)hd < (unsigned)P.dst1.H) {
      off1 = fo1 + hd * P.dst1.ws + wd;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if ((vmask >> i & 1) && (unsigned)(wd + i) < (unsigned)P.dst1.W) sm1 |= 1 << i;
    }
  }
  float* const d0 = P.dst0.p + (long long)n * P.dst0.ns;
  float* const d1 = P.dst1.p + (long long)n * P.dst1.ns;
  float* const prow = P.partials != nullptr ? P.partials + (size_t)(pt * 4 + wave) * (2 * P.Mpad) : nullptr;

  if (P.bw_raw == nullptr) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int co = m0 + m * 16 + j * 4 + reg;
        const bool first = co < P.dst0.C;
        const int cd = first ? co : co - P.dst0.C;
        const bool co_ok = co < P.Cout && (first || cd < P.dst1.C);
        float* const px = (first ? d0 + (long long)cd * P.dst0.cs : d1 + (long long)cd * P.dst1.cs) + (first ? off0 : off1);
        const int sm = co_ok ? (first ? sm0 : sm1) : 0;
        float y[4];
        get_y(m, reg, y);
        // statistics over the pixels that are STORED (the destination's window: for a cropped second destination -- the
        // backward of F.pad -- the sums are those of the crop, e.g. the ConvT bias gradient; the same pixels as `vmask` for a
        // full-size destination)
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (sm >> i & 1) {
            s1 += y[i];
            s2 = fmaf(y[i], y[i], s2);
          }
        }
        if (sm == 15) {
          *reinterpret_cast<f32x4u*>(px) = f32x4{y[0], y[1], y[2], y[3]};
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (sm >> i & 1) px[i] = y[i];
        }
        if (prow != nullptr) {
          s1 = reduce16_to_lane15(s1);
          s2 = reduce16_to_lane15(s2);
          if (l16 == 15 && co < P.Mpad) {
            prow[co] = s1;
            prow[P.Mpad + co] = s2;
          }
        }
      }
    }
  } else {
    // dst0 is the gradient buffer of a conv+BN+ReLU unit whose raw output has the same geometry: dz = relu'(bn(raw)) * dX.
    // Loads and stores share vmcnt: the raw values of one m-tile (4 rows x 4 pixels) are loaded together in front of its
    // stores, the coefficients come from LDS.
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      float xr[4][4];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int co = m0 + m * 16 + j * 4 + reg;
        const float* const rp = P.bw_raw + (long long)n * P.dst0.ns + (long long)(co < P.Cout ? co : 0) * P.dst0.cs + off0;
        if (sm0 == 15) {
          const f32x4 t = *reinterpret_cast<const f32x4u*>(rp);
          xr[reg][0] = t[0]; xr[reg][1] = t[1]; xr[reg][2] = t[2]; xr[reg][3] = t[3];
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) xr[reg][i] = (sm0 >> i & 1) ? rp[i] : 0.f;
        }
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int co = m0 + m * 16 + j * 4 + reg;
        float* const px = d0 + (long long)co * P.dst0.cs + off0;
        const int cl = wm * BM + m * 16 + j * 4 + reg;
        const float bsc = sBw[cl], bsh = sBw[BM + cl], bmu = sBw[2 * BM + cl], bis = sBw[3 * BM + cl];
        const int sm = co < P.Cout ? sm0 : 0;
        float y[4];
        get_y(m, reg, y);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float x = xr[reg][i];
          const float dz = ((sm >> i & 1) && fmaf(x, bsc, bsh) > 0.f) ? y[i] : 0.f;
          y[i] = dz;
          s1 += dz;
          s2 = fmaf(dz, (x - bmu) * bis, s2);
        }
        if (sm == 15) {
          *reinterpret_cast<f32x4u*>(px) = f32x4{y[0], y[1], y[2], y[3]};
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (sm >> i & 1) px[i] = y[i];
        }
        if (prow != nullptr) {
          s1 = reduce16_to_lane15(s1);
          s2 = reduce16_to_lane15(s2);
          if (l16 == 15 && co < P.Mpad) {
            prow[co] = s1;
            prow[P.Mpad + co] = s2;
          }
        }
      }
    }
  }
}

// X4: the halo windows move as ALIGNED 16-byte pieces (global_load_lds_dwordx4 with a per-lane source address) instead of
// dword gathers: possible when every source row starts 16-byte aligned (row pitch, plane and image strides multiples of 4
// floats, pad offset a multiple of 4) -- the engine allocates its activations that way.  A window row is then the NP =
// TW/4 + 2 pieces that cover image columns w0-4 .. w0+TW+3, and the wave-uniform LDS base is shifted by ONE float so that
// image column w0-1 lands 16-byte aligned and the consumer reads stay one b128 + one b64 per kernel row.  A quarter of the
// gather instructions (2 per channel plane instead of 6), each a coalesced run of 16-byte lanes.  Columns >= W inside the
// pitch come from memory: producers keep the padding value there (NaN under a ReLU'd BatchNorm, else 0).
//
// FAST: straight halo fills, no per-slot bookkeeping (which segment, how many channels it has left, which sentinel: a
// chain of scalar branches per slot in the general form): possible when a chunk of 4 channels never straddles the two
// source segments and Cin % 4 == 0 (always true in the U-Net).  In-kernel stamps put the per-slot form at ~1200 of the cycles a
// wave spends per chunk (docs/LOG_r01-r04.md, round 2); measured -7 % kernel time over the U-Net's layer set.
//
// PLAIN: no source segment carries a deferred BatchNorm or ReLU (every dX launch: dy is plain; the pooled and upsampled
// sources of the forward): the operand transform drops its 12 fma/max per kernel row and the per-chunk scale / shift
// reads.  Measured with the transform forced plain over the layer set: -2.5 % kernel time.
//
// X4M: 0 the dword halo gathers, 1 the X4 form above.  Ablation (fills removed, docs/LOG_r01-r04.md, round 2): the dword halo
// fills cost 9.5 % of the kernel's time, the weight fills 3 %, the barrier 2 % -- memory traffic and latency, not instruction
// count: 16-byte pieces from unaligned rows were measured neutral over the step (docs/LOG_r01-r04.md).
//
// SPLIT ("K slabs"): a launch whose tile grid covers a fraction of the chip's 512 block slots (the 40 x 53 and 20 x 26 levels at
// small per-GPU batches: 152-600 blocks of 128-256 chunks each) is cut along the input channels instead: block (tile, slab k)
// runs chunks [k nchunks / S, (k+1) nchunks / S) and stores its UN-reduced y = A^T M tile to P.slabs; w43_slab_reduce_kernel adds
// the S slabs in slab order and runs this kernel's epilogue (crop, statistics, fused BatchNorm-backward) on the sums.
template <int X4M, bool FAST, bool PLAIN, bool SPLIT = false>
__global__ __launch_bounds__(256, 2) void conv3x3_w43_kernel(const W43Params P) {
  constexpr bool X4 = X4M == 1;
  static_assert(!SPLIT || FAST, "K slabs: the straight-fill form");
  constexpr int MT = 4, BM = W43_BM, WS = BM, WTILE = W43_WTILE, NT = 256, NWAVE = 4, NWI = W43_NWI;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int PS = P.PS;
  const int BUF = WTILE + 4 * PS;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave8 = __builtin_amdgcn_readfirstlane(tid >> 6);
  // wave: pixel group of the wave.  wm (0 in a 256-thread block) stays a run-time value: folding it to 0 changes the register
  // allocation of the kernel, and this form is the one that was measured
  const int wm = wave8 >> 2, wave = wave8 & 3;
  const int j = lane >> 4, l16 = lane & 15;

  // The m-blocks of one pixel tile read the same halo: hardware deals blocks round-robin over the 8 XCDs, so give every XCD
  // a contiguous range of logical ids (pixel tile major, m-block minor) and its L2 serves the halo once.
  const int lid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int mbb = lid % P.mblocks;
  const int slab = SPLIT ? (lid / P.mblocks) % P.nslab : 0;   // SPLIT: pixel tile major, then slab, m-block minor
  const int pt = SPLIT ? lid / (P.mblocks * P.nslab) : lid / P.mblocks;
  const int c_lo = SPLIT ? (int)((long long)slab * P.nchunks / P.nslab) : 0;            // this block's channel chunks
  const int c_hi = SPLIT ? (int)((long long)(slab + 1) * P.nchunks / P.nslab) : P.nchunks;
  const int m0 = (mbb + wm) * BM;
  const int tpi = P.tiles_y * P.tiles_x;
  const int n = P.fold ? 0 : pt / tpi;            // fold: the tile rows cover the whole batch, the image is a per-lane value
  const int rt = pt - n * tpi;
  const int ty = rt / P.tiles_x;
  const int h0 = ty * P.TH, w0 = (rt - ty * P.tiles_x) * P.TW;   // fold: h0 is a padded flat row (w43_row)

  // ---- this lane's Winograd tile: 4 pixels (tr, 4*tq .. 4*tq+3) of the block's TH x TW output tile ----------------------
  const int q = wave * 16 + l16;
  const bool q_ok = q < P.TH * P.TWq;
  const int tr = q_ok ? q / P.TWq : 0;
  const int tq = q_ok ? q - tr * P.TWq : 0;
  const int baddr = WTILE + j * PS + tr * P.WCp + 4 * tq + (X4 ? 4 : 0);   // halo columns 4*tq .. 4*tq+5 of halo rows tr .. tr+2
  int vmask = 0;                                            // pixels of the tile that exist in the image
  int n_t, h_t;                                             // this lane's image and row
  w43_row(P, n, h0 + tr, n_t, h_t);
  if (q_ok && h_t >= 0 && h_t < P.H) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (w0 + 4 * tq + i < P.W) vmask |= 1 << i;
  }

  // ---- DMA lane geometry (as gsd_conv3x3.hip, window rows padded to WCp floats) ------------------------------------------
  constexpr int NPP = 2;   // dword form: position chunks of 64 per wave (the block's waves cover the 512 window positions
                                // once); X4: DMA units (channel plane, instruction) per wave and chunk
  int xo0[NPP], xo1[NPP];
  int u_ch[NPP], u_lds[NPP];    // X4: the unit's channel of the chunk and its float offset inside the channel plane
  bool p_on[NPP];
#pragma unroll
  for (int pp = 0; pp < NPP; ++pp) {
    xo0[pp] = xo1[pp] = -2;
    u_ch[pp] = u_lds[pp] = 0;
    if constexpr (X4) {
      const int u = wave8 + NWAVE * pp;            // units 0 .. 4*NI-1: channel u / NI, instruction u % NI
      p_on[pp] = u < 4 * P.NI;
      u_ch[pp] = u / P.NI;
      const int ii = u - u_ch[pp] * P.NI;
      u_lds[pp] = ii * P.RPI * P.WCp + 1;          // + 1 float: image column w0-1 then sits 16-byte aligned
      const int rl = lane / P.NP, pc = lane - rl * P.NP;
      const int rr = ii * P.RPI + rl;
      if (p_on[pp] && rl < P.RPI && rr < P.WR) {
        int nn, gh;
        w43_row(P, n, h0 - 1 + rr, nn, gh);
        const int gw = w0 - 4 + 4 * pc;
        const int fo0 = P.fold ? nn * (int)P.src0.ns : 0, fo1 = P.fold ? nn * (int)P.src1.ns : 0;
        int hs = gh - P.src0.oh, ws = gw - P.src0.ow;
        xo0[pp] = ((unsigned)hs < (unsigned)P.src0.H && ws >= 0 && ws < P.src0.W && ws + 4 <= P.src0.ws) ? fo0 + hs * P.src0.ws + ws : -1;
        hs = gh - P.src1.oh;
        ws = gw - P.src1.ow;
        xo1[pp] = ((unsigned)hs < (unsigned)P.src1.H && ws >= 0 && ws < P.src1.W && ws + 4 <= P.src1.ws) ? fo1 + hs * P.src1.ws + ws : -1;
      }
    } else {
      p_on[pp] = wave8 + NWAVE * pp < P.NPV;
      const int pos = (wave8 + NWAVE * pp) * 64 + lane;
      const int rr = pos / P.WCp, cc = pos - rr * P.WCp;
      if (rr < P.WR && cc < P.WC) {
        int nn, gh;
        w43_row(P, n, h0 - 1 + rr, nn, gh);
        const int gw = w0 - 1 + cc;
        const int fo0 = P.fold ? nn * (int)P.src0.ns : 0, fo1 = P.fold ? nn * (int)P.src1.ns : 0;
        int hs = gh - P.src0.oh, ws = gw - P.src0.ow;
        xo0[pp] = ((unsigned)hs < (unsigned)P.src0.H && (unsigned)ws < (unsigned)P.src0.W) ? fo0 + hs * P.src0.ws + ws : -1;
        hs = gh - P.src1.oh;
        ws = gw - P.src1.ow;
        xo1[pp] = ((unsigned)hs < (unsigned)P.src1.H && (unsigned)ws < (unsigned)P.src1.W) ? fo1 + hs * P.src1.ws + ws : -1;
      }
    }
  }
  const float* wsrc0 = P.wt + (size_t)mbb * P.nchunks * WTILE;   // the block's weight image
  const long long wlane = tid * 4;   // this lane's float offset inside a 1 KiB weight piece group
  long long xl0[NPP];   // first segment's offsets as 64-bit lane values (the address add is then a single instruction)
#pragma unroll
  for (int pp = 0; pp < NPP; ++pp) xl0[pp] = xo0[pp];
  // SPLIT: a slab that lies wholly in the second (concat) segment starts there -- its padding positions, plane pointer and lane offsets
  const bool s1_start = SPLIT && P.src1.C > 0 && c_lo * 4 > P.src0.C;
  // padding positions of the first segment, once, in all 2 x 4 channel planes (own positions only: the lanes that
  // would otherwise DMA the sentinel there on every fill); visible to the consumers after the first barrier
  const float pad0 = (s1_start ? P.src1.relu : P.src0.relu) ? __builtin_nanf("") : 0.f;
#pragma unroll
  for (int pp = 0; pp < NPP; ++pp)
    if (p_on[pp] && (s1_start ? xo1[pp] : xo0[pp]) == -1) {
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        if constexpr (X4) {   // the unit's own plane: the other planes' pieces belong to other units
#pragma unroll
          for (int e = 0; e < 4; ++e) smem[b * BUF + WTILE + u_ch[pp] * PS + u_lds[pp] + lane * 4 + e] = pad0;
        } else {
#pragma unroll
          for (int ch = 0; ch < 4; ++ch) smem[b * BUF + WTILE + ch * PS + (wave8 + NWAVE * pp) * 64 + lane] = pad0;
        }
      }
    }
  int d_seg = 0, d_left = P.src0.C;
  const float* d_base = P.src0.p + (long long)n * P.src0.ns;
  long long d_cs = P.src0.cs;
  if constexpr (SPLIT) {   // first channel plane of the slab
    if (s1_start) {
      d_base = P.src1.p + (long long)n * P.src1.ns + (long long)(c_lo * 4 - P.src0.C) * P.src1.cs;
      d_cs = P.src1.cs;
    } else {
      d_base += (long long)(c_lo * 4) * P.src0.cs;
    }
  }
  const float* d_sent = X4 ? (P.src0.relu ? &gsd_pad16_w43[4] : &gsd_pad16_w43[0]) : (P.src0.relu ? &gsd_pad_w43[1] : &gsd_pad_w43[0]);
  int d_xo[NPP];
#pragma unroll
  for (int pp = 0; pp < NPP; ++pp) d_xo[pp] = xo0[pp];

  // FAST ("straight fill"): no per-slot bookkeeping at all.  Every chunk lies inside one source segment (src0.C % 4 == 0,
  // Cin % 4 == 0), so a halo slot is: the lanes that have a pixel move it, the plane pointer advances by one channel.  The
  // switch to the second (concat) segment happens once per block, between two chunks: new plane pointer and lane offsets,
  // and the padding positions of that segment are written into each LDS image the first time it is filled from it.
  const int f_sw = (P.src1.C > 0 && !s1_start) ? P.src0.C / 4 : -1;   // first chunk of the second segment
  int f_xo[NPP];
  long long f_xl[NPP];
#pragma unroll
  for (int pp = 0; pp < NPP; ++pp) {
    f_xo[pp] = s1_start ? xo1[pp] : xo0[pp];
    f_xl[pp] = f_xo[pp];
  }
  auto begin_fill = [&](int chunk, int buf) {
    if (f_sw < 0 || (chunk != f_sw && chunk != f_sw + 1)) return;
    if (chunk == f_sw) {
      d_base = P.src1.p + (long long)n * P.src1.ns;
      d_cs = P.src1.cs;
#pragma unroll
      for (int pp = 0; pp < NPP; ++pp) {
        f_xo[pp] = xo1[pp];
        f_xl[pp] = xo1[pp];
      }
    }
    const float pad1 = P.src1.relu ? __builtin_nanf("") : 0.f;
#pragma unroll
    for (int pp = 0; pp < NPP; ++pp)
      if (p_on[pp] && f_xo[pp] == -1) {
        if constexpr (X4) {
#pragma unroll
          for (int e = 0; e < 4; ++e) smem[buf * BUF + WTILE + u_ch[pp] * PS + u_lds[pp] + lane * 4 + e] = pad1;
        } else {
#pragma unroll
          for (int ch = 0; ch < 4; ++ch) smem[buf * BUF + WTILE + ch * PS + (wave8 + NWAVE * pp) * 64 + lane] = pad1;
        }
      }
  };
  auto fast_halo = [&](int ch, float* Xb) {
#pragma unroll
    for (int pp = 0; pp < NPP; ++pp) {
      if constexpr (X4) {
        if (p_on[pp] && u_ch[pp] == ch && f_xo[pp] >= 0) {
          const float* gp = d_base + f_xl[pp];
          float* dstp = Xb + ch * PS + u_lds[pp];
          __builtin_amdgcn_global_load_lds(gp, dstp, 16, 0, 0);
        }
      } else {
        if (p_on[pp] && f_xo[pp] >= 0) {
          const float* gp = d_base + f_xl[pp];
          float* dstp = Xb + ch * PS + (wave8 + NWAVE * pp) * 64;
          __builtin_amdgcn_global_load_lds(gp, dstp, 4, 0, 0);
        }
      }
    }
    d_base += d_cs;
  };

  // slots 0..NWI-1: the weight chunk (16 B per lane); slot NWI+ch: input channel ch of the chunk
  auto dma_slot = [&](int slot, int chunk, int buf) {
    float* Wb = smem + buf * BUF;
    if constexpr (FAST) {
      if (slot >= NWI && slot < NWI + 4) {
        fast_halo(slot - NWI, Wb + WTILE);
        return;
      }
    }
    if (slot < NWI) {
      // scalar chunk base + the lane's fixed offset.  The last slot is half full (1152 = 4.5 x 256 pieces): it goes to waves
      // 2 and 3, because waves 0 and 1 already move two position chunks of every halo plane where waves 2 and 3 move one --
      // the barrier waits for the busiest wave.
      if (slot < NWI - 1) {
        __builtin_amdgcn_global_load_lds(wsrc0 + (size_t)chunk * WTILE + slot * (NT * 4) + wlane, Wb + (slot * NT + wave8 * 64) * 4, 16, 0, 0);
      } else if (wave8 >= 2) {
        __builtin_amdgcn_global_load_lds(wsrc0 + (size_t)chunk * WTILE + (slot * NT - 128) * 4 + wlane, Wb + (slot * NT - 128 + wave8 * 64) * 4, 16, 0, 0);
      }
    } else if (slot < NWI + 4) {
      const int ch = slot - NWI;
      float* Xb = Wb + WTILE;
      if (d_left == 0 && d_seg == 0) {
        d_seg = 1;
        d_left = P.src1.C;
        d_base = P.src1.p + (long long)n * P.src1.ns;
        d_cs = P.src1.cs;
        d_sent = X4 ? (P.src1.relu ? &gsd_pad16_w43[4] : &gsd_pad16_w43[0]) : (P.src1.relu ? &gsd_pad_w43[1] : &gsd_pad_w43[0]);
#pragma unroll
        for (int pp = 0; pp < NPP; ++pp) d_xo[pp] = xo1[pp];
      }
      const bool c_ok = d_left > 0;
      if constexpr (X4) {
        // 16-byte pieces: the unit (channel plane ch, instruction ii) of the wave that owns it; the other waves only keep the
        // channel bookkeeping below in step
#pragma unroll
        for (int pp = 0; pp < NPP; ++pp) {
          if (p_on[pp] && u_ch[pp] == ch) {
            float* dstp = Xb + ch * PS + u_lds[pp];
            if (c_ok && d_seg == 0) {
              if (xo0[pp] >= 0) {
                const float* gp = d_base + xl0[pp];
                __builtin_amdgcn_global_load_lds(gp, dstp, 16, 0, 0);
              }   // padding pieces: written once, below
            } else if (d_xo[pp] != -2) {
              const float* g = (c_ok && d_xo[pp] >= 0) ? d_base + d_xo[pp] : (c_ok ? d_sent : &gsd_pad16_w43[0]);
              __builtin_amdgcn_global_load_lds(g, dstp, 16, 0, 0);
            }
          }
        }
      } else if (c_ok && d_seg == 0) {
        // fast path, first segment: the padding positions of every plane were written once at kernel start (below), so a
        // fill only moves the lanes that have a pixel -- no select, no sentinel pointer, one v_lshl_add_u64 per instruction
#pragma unroll
        for (int pp = 0; pp < NPP; ++pp)
          if (p_on[pp] && xo0[pp] >= 0)
            __builtin_amdgcn_global_load_lds(d_base + xl0[pp], Xb + ch * PS + (wave8 + NWAVE * pp) * 64, 4, 0, 0);
      } else {
        // second (concat) segment and K padding: every window position is written, padding from the sentinel
        const float* sentinel = c_ok ? d_sent : &gsd_pad_w43[0];
#pragma unroll
        for (int pp = 0; pp < NPP; ++pp) {
          if (p_on[pp] && d_xo[pp] != -2) {
            const float* g = (c_ok && d_xo[pp] >= 0) ? d_base + d_xo[pp] : sentinel;
            __builtin_amdgcn_global_load_lds(g, Xb + ch * PS + (wave8 + NWAVE * pp) * 64, 4, 0, 0);
          }
        }
      }
      if (c_ok) {
        d_base += d_cs;
        --d_left;
      }
    }
  };

  const int Kpad = P.nchunks * 4;
  float* sAff = smem + 2 * BUF;
  for (int c = tid; c < Kpad; c += NT) {
    const bool first = c < P.src0.C;
    const SrcD& S = first ? P.src0 : P.src1;
    const int cc = first ? c : c - P.src0.C;
    float sc = 1.f, sh = 0.f;
    if (c < P.Cin && cc < S.C && S.scale != nullptr) {
      sc = S.scale[cc];
      sh = S.shift[cc];
    }
    sAff[c] = sc;
    sAff[Kpad + c] = sh;
  }
  float* sBw = sAff + 2 * Kpad;   // [4][BM]: scale, shift, mean, invstd of the fused BatchNorm-backward epilogue
  if (P.bw_raw != nullptr) {
    for (int c = tid; c < BM; c += NT) {
      const int co = mbb * BM + c < P.Cout ? mbb * BM + c : 0;
      sBw[c] = P.bw_scale[co];
      sBw[BM + c] = P.bw_shift[co];
      sBw[2 * BM + c] = P.bw_mean[co];
      sBw[3 * BM + c] = P.bw_invstd[co];
    }
  }
  const float lo0 = P.src0.relu ? 0.f : -__builtin_inff(), lo1 = P.src1.relu ? 0.f : -__builtin_inff();

  f32x4 acc[MT][6];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int f = 0; f < 6; ++f) acc[m][f] = f32x4{0.f, 0.f, 0.f, 0.f};

  // V = B^T d of one kernel row: raw halo values -> deferred BatchNorm+ReLU -> the 6 frequency operands
  auto transform = [&](const f32x4& ra, const f32x2& rb, float sc, float sh, float lo, float (&v)[6]) {
    float d0 = ra[0], d1 = ra[1], d2 = ra[2], d3 = ra[3], d4 = rb[0], d5 = rb[1];
    if constexpr (!PLAIN) {
      d0 = fmaxf(fmaf(d0, sc, sh), lo), d1 = fmaxf(fmaf(d1, sc, sh), lo), d2 = fmaxf(fmaf(d2, sc, sh), lo);
      d3 = fmaxf(fmaf(d3, sc, sh), lo), d4 = fmaxf(fmaf(d4, sc, sh), lo), d5 = fmaxf(fmaf(d5, sc, sh), lo);
    }
    const float a = fmaf(-4.f, d2, d4), b = fmaf(-4.f, d1, d3);
    const float c = d4 - d2, e = 2.f * (d3 - d1);
    v[0] = fmaf(4.f, d0, fmaf(-5.f, d2, d4));
    v[1] = a + b;
    v[2] = a - b;
    v[3] = c + e;
    v[4] = c - e;
    v[5] = fmaf(4.f, d1, fmaf(-5.f, d3, d5));
  };

  const int a_lane = wm * WTILE + l16 * 4;
  if constexpr (FAST) begin_fill(c_lo, 0);
#pragma unroll
  for (int slot = 0; slot < NWI + 4; ++slot) dma_slot(slot, c_lo, 0);
  for (int chunk = c_lo; chunk < c_hi; ++chunk) {
    const int cur = (chunk - c_lo) & 1;
    gsd_dma_barrier();
    const int kc = chunk * 4 + j;
    float sc = 1.f, sh = 0.f, lo = 0.f;
    if constexpr (!PLAIN) {
      sc = sAff[kc], sh = sAff[Kpad + kc];
      lo = kc < P.src0.C ? lo0 : (kc < P.Cin ? lo1 : -__builtin_inff());
    }
    const bool more = chunk + 1 < c_hi;
    const float* Wc = smem + cur * BUF;
    constexpr int PF = 1;   // k-steps the weight operand is read ahead of its MFMAs
    f32x4 av[PF + 1];
    f32x4 ra[2];
    f32x2 rb[2];
    float v[6];
    ra[0] = *reinterpret_cast<const f32x4*>(&Wc[baddr]);
    rb[0] = *reinterpret_cast<const f32x2*>(&Wc[baddr + 4]);
#pragma unroll
    for (int s = 0; s < PF; ++s) av[s] = *reinterpret_cast<const f32x4*>(&Wc[(j * 18 + s) * WS + a_lane]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      transform(ra[r & 1], rb[r & 1], sc, sh, lo, v);
      if (r < 2) {   // the next kernel row's raw values fly during this row's 24 MFMAs
        ra[(r + 1) & 1] = *reinterpret_cast<const f32x4*>(&Wc[baddr + (r + 1) * P.WCp]);
        rb[(r + 1) & 1] = *reinterpret_cast<const f32x2*>(&Wc[baddr + (r + 1) * P.WCp + 4]);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int f = 0; f < 6; ++f) {
        const int s = r * 6 + f, cs = s % (PF + 1);
        if (s + PF < 18)
          av[(s + PF) % (PF + 1)] = *reinterpret_cast<const f32x4*>(&Wc[(j * 18 + s + PF) * WS + a_lane]);
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m][f] = mfma16(av[cs][m], v[f], acc[m][f]);
        if constexpr (FAST) {
          // weights first, in ONE k-step: a wave's four pieces are adjacent (4 KiB), so they share one LDS base (M0) and differ
          // in the instruction's immediate offset, which moves the global and the LDS address alike -- a changed M0 between
          // two LDS-DMA instructions costs the wave ~45 cycles at two blocks per CU (profiles/ubench/dma_m0.hip); then the halo
          if (more && s < 3) {
            if (s == 0) {
              begin_fill(chunk + 1, cur ^ 1);
              float* Wn = smem + (cur ^ 1) * BUF;
              const float* wg = wsrc0 + (size_t)(chunk + 1) * WTILE + wave8 * 1024 + lane * 4;
              float* wl = Wn + wave8 * 1024;
              __builtin_amdgcn_global_load_lds(wg, wl, 16, 0, 0);
              __builtin_amdgcn_global_load_lds(wg, wl, 16, 1024, 0);
              __builtin_amdgcn_global_load_lds(wg, wl, 16, 2048, 0);
              __builtin_amdgcn_global_load_lds(wg, wl, 16, 3072, 0);
              if (wave8 >= 2) {   // pieces 16, 17 of the 18
                const float* wg2 = wsrc0 + (size_t)(chunk + 1) * WTILE + (14 + wave8) * 256 + lane * 4;
                float* wl2 = Wn + (14 + wave8) * 256;
                __builtin_amdgcn_global_load_lds(wg2, wl2, 16, 0, 0);
              }
            } else {
              dma_slot(NWI + 2 * s - 2, chunk + 1, cur ^ 1);
              dma_slot(NWI + 2 * s - 1, chunk + 1, cur ^ 1);
            }
          }
        } else if (more && s < 5) {
          dma_slot(2 * s, chunk + 1, cur ^ 1);
          dma_slot(2 * s + 1, chunk + 1, cur ^ 1);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  // ---- epilogue: y = A^T M, NCHW stores (two destination segments with crop), BatchNorm partial sums ----------------------
  auto out_transform = [&](int m, int reg, float (&y)[4]) {
    const float M0 = acc[m][0][reg], M1 = acc[m][1][reg], M2 = acc[m][2][reg];
    const float M3 = acc[m][3][reg], M4 = acc[m][4][reg], M5 = acc[m][5][reg];
    const float p12 = M1 + M2, m12 = M1 - M2, p34 = M3 + M4, m34 = M3 - M4;
    y[0] = M0 + p12 + p34;
    y[1] = fmaf(2.f, m34, m12);
    y[2] = fmaf(4.f, p34, p12);
    y[3] = fmaf(8.f, m34, m12) + M5;
  };

  if constexpr (SPLIT) {
    // K slab: the un-reduced tile, every lane its 16 B (padding tiles and channels included; the reducer masks)
    float* const tile = P.slabs + (((size_t)slab * (gridDim.x / P.nslab) + (size_t)pt * P.mblocks + mbb) * BM) * 256 + (wave * 16 + l16) * 4;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        float y[4];
        out_transform(m, reg, y);
        *reinterpret_cast<f32x4*>(tile + (m * 16 + j * 4 + reg) * 256) = f32x4{y[0], y[1], y[2], y[3]};
      }
  } else {
    w43_epilogue(P, n, pt, wave, wm, m0, j, l16, n_t, h_t, w0, tq, vmask, sBw, out_transform);
  }
}

// K-slab reducer: block (pixel tile, m-block) adds the S un-reduced 64 x 256 tiles the SPLIT blocks left in P.slabs, in slab order
// (run-to-run bitwise), and runs the convolution's epilogue on the sums -- same lane -> (channel, pixel) map, same destinations,
// same partial rows, same fused BatchNorm-backward form.  HBM-bound: (S + 1) x 64 KiB per block.
__global__ __launch_bounds__(256) void w43_slab_reduce_kernel(const W43Params P) {
  __shared__ float sBw[4 * W43_BM];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane >> 4, l16 = lane & 15;
  const int lid = blockIdx.x;
  const int mbb = lid % P.mblocks, pt = lid / P.mblocks;
  const int tpi = P.tiles_y * P.tiles_x;
  const int n = P.fold ? 0 : pt / tpi;
  const int rt = pt - n * tpi;
  const int ty = rt / P.tiles_x;
  const int h0 = ty * P.TH, w0 = (rt - ty * P.tiles_x) * P.TW;
  const int q = wave * 16 + l16;
  const bool q_ok = q < P.TH * P.TWq;
  const int tr = q_ok ? q / P.TWq : 0;
  const int tq = q_ok ? q - tr * P.TWq : 0;
  int vmask = 0, n_t, h_t;
  w43_row(P, n, h0 + tr, n_t, h_t);
  if (q_ok && h_t >= 0 && h_t < P.H) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (w0 + 4 * tq + i < P.W) vmask |= 1 << i;
  }
  if (P.bw_raw != nullptr) {
    if (tid < W43_BM) {
      const int co = mbb * W43_BM + tid < P.Cout ? mbb * W43_BM + tid : 0;
      sBw[tid] = P.bw_scale[co];
      sBw[W43_BM + tid] = P.bw_shift[co];
      sBw[2 * W43_BM + tid] = P.bw_mean[co];
      sBw[3 * W43_BM + tid] = P.bw_invstd[co];
    }
    __syncthreads();
  }
  const size_t sstride = (size_t)gridDim.x * W43_BM * 256;
  const float* const tile = P.slabs + (size_t)lid * W43_BM * 256 + q * 4;
  f32x4 ys[4][4];   // all 16 channel rows of slab 0 in flight, then one slab after the other on top
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) ys[m][reg] = *reinterpret_cast<const f32x4*>(tile + (m * 16 + j * 4 + reg) * 256);
  for (int k = 1; k < P.nslab; ++k) {
    const float* const tk = tile + (size_t)k * sstride;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) ys[m][reg] += *reinterpret_cast<const f32x4*>(tk + (m * 16 + j * 4 + reg) * 256);
  }
  auto get_y = [&](int m, int reg, float (&y)[4]) {
    y[0] = ys[m][reg][0], y[1] = ys[m][reg][1], y[2] = ys[m][reg][2], y[3] = ys[m][reg][3];
  };
  w43_epilogue(P, n, pt, wave, 0, mbb * W43_BM, j, l16, n_t, h_t, w0, tq, vmask, sBw, get_y);
}

// -------------------------------------------------------------------------------------------------
// host side
// -------------------------------------------------------------------------------------------------
namespace {

struct W43Plan {
  int TH, TW, TWq, tiles_y, tiles_x, mblocks, WR, WC, WCp, fold;
};

// TH x TW output tile of up to 64 Winograd tiles whose padded halo window fits the 512 DMA positions.  Every block does the
// work of 64 tiles whatever it covers, so: fewest blocks; among equals 32-wide rows, then the widest.
// Small images (levels 3-4 of the U-Net: 40 x 53, 20 x 26) fill such a tile badly (83 % / 68 %): for them the tile rows run
// over the padded flat rows of the whole batch (`fold`, see w43_row) and the tile may be 7 or 14 Winograd tiles wide
// (28 / 56 pixels: 53 -> 2 x 28, 26 -> 1 x 28), with the LDS row pitch chosen for the fewest bank conflicts of the halo reads.
bool plan_w43(int N, int H, int W, int M, W43Plan* best) {
  long best_cost = -1;
  const int force_tw = gsd_env_int("GSD_W43_TW", 0);   // tuning
  const int fold_mode = gsd_env_int("GSD_W43_FOLD", -1);   // tuning: 0 never, 1 whenever possible, -1 when it saves > 4 % of the blocks
  best->fold = 0;
  long plain_blocks = -1;
  for (int fold = 0; fold <= 1; ++fold) {
    if (fold && (fold_mode == 0 || N <= 1 || (long)H * W > 8192)) continue;
    static const int tws[9] = {32, 64, 16, 8, 4, 28, 56, 24, 48};
    for (int k = 0; k < (fold ? 9 : 5); ++k) {   // (7- and 14-tile rows without folding, folding at 80 x 106: measured, no gain)
      const int tw = tws[k];
      if (force_tw && tw != force_tw) continue;
      const int twq = tw / 4;
      int th = 64 / twq;
      int wcp = round_up(tw + 2, 4);
      while (th > 1 && (th + 2) * wcp > 512) --th;
      if ((th + 2) * wcp > 512) continue;
      const int rows = fold ? N * (H + 1) : H;
      if (th > rows) th = rows;
      const int ty = ceil_div(rows, th);
      if (!fold) th = ceil_div(H, ty);
      const long blocks = (long)ty * ceil_div(W, tw) * (fold ? 1 : N);
      if (!fold && (plain_blocks < 0 || blocks < plain_blocks)) plain_blocks = blocks;
      if (fold && fold_mode < 0 && blocks * 104 > plain_blocks * 100) continue;
      if ((twq & (twq - 1)) != 0 || fold) {   // odd widths: pick the LDS row pitch with the fewest bank conflicts
        int bc = -1;
        for (int c = round_up(tw + 2, 4); c <= round_up(tw + 2, 4) + 12 && (th + 2) * c <= 512; c += 4) {
          const int cyc = conv3_halo_read_cycles(4, 1, twq, c, round_up((th + 2) * c, 4) + 4, 0);
          if (bc < 0 || cyc < bc) {
            bc = cyc;
            wcp = c;
          }
        }
      }
      const long cost = blocks * 8 + (tw == 32 ? 0 : tw == 64 ? 1 : tw == 16 ? 2 : 3);
      if (best_cost < 0 || cost < best_cost) {
        best_cost = cost;
        best->fold = fold;
        best->TH = th; best->TW = tw; best->TWq = twq;
        best->tiles_y = ty; best->tiles_x = ceil_div(W, tw);
        best->WR = th + 2; best->WC = tw + 2; best->WCp = wcp;
      }
    }
  }
  best->mblocks = ceil_div(M, W43_BM);
  return best_cost >= 0;
}

template <int X4, bool FAST, bool PLAIN = false, bool SPLIT = false>
int launch_one(const W43Params& P, int grid, size_t lds, hipStream_t st) {
  return gsd_launch<conv3x3_w43_kernel<X4, FAST, PLAIN, SPLIT>>("gsd_conv3x3_w43", dim3(grid), dim3(256), lds, st, P);
}

// K-slab form: the SPLIT blocks (grid = tile blocks x slabs), then the reducer over the tile blocks
int launch_split(const W43Params& P, int base_grid, size_t lds, hipStream_t st, bool x4, bool plain) {
  const int grid = base_grid * P.nslab;
  int e = x4 ? (plain ? launch_one<1, true, true, true>(P, grid, lds, st) : launch_one<1, true, false, true>(P, grid, lds, st))
             : (plain ? launch_one<0, true, true, true>(P, grid, lds, st) : launch_one<0, true, false, true>(P, grid, lds, st));
  if (e != GSD_OK) return e;
  hipLaunchKernelGGL(w43_slab_reduce_kernel, dim3(base_grid), dim3(256), 0, st, P);
  GSD_LAUNCH_CHECK("gsd_conv3x3_w43 (slab reduce)");
  return GSD_OK;
}

int launch_w43(const W43Params& P, int grid, size_t lds, hipStream_t st, bool x4, bool fast, bool plain) {
  if (fast && plain) return x4 ? launch_one<1, true, true>(P, grid, lds, st) : launch_one<0, true, true>(P, grid, lds, st);
  if (fast) return x4 ? launch_one<1, true>(P, grid, lds, st) : launch_one<0, true>(P, grid, lds, st);
  return x4 ? launch_one<1, false>(P, grid, lds, st) : launch_one<0, false>(P, grid, lds, st);
}

// The K-slab model (gsd_conv3x3_host.h) with this kernel's constants, fitted to profiles/r05_kslabs_b{8,16,32}.txt (117 timings of
// 22 launch shapes, S = 1..8: rms error 4 %; the fitted model picks the fastest measured S on 20 of the 22 shapes and is within
// 0.5 % on the other two): 2.6 us per chunk of a block that shares its CU, 4 us per block, a lone block at 0.55 of a pair's time
// (it runs 1.8x faster).  GSD_W43_SPLIT: 0 / 1 never, S >= 2 that many wherever the shape admits it.
constexpr Conv3SlabModel w43_slabs = {2.6, 4.0, 0.55, "GSD_W43_SPLIT"};

}  // namespace

// Floats of K-slab scratch gsd_conv3x3_w43_ws wants for this shape (0: it runs unsplit).
extern "C" int64_t gsd_conv3x3_w43_workspace(int N, int H, int W, int Cin, int Cout) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || Cin % 4 != 0) return 0;
  W43Plan p;
  if (!plan_w43(N, H, W, Cout, &p)) return 0;
  const long base = (long)(p.fold ? 1 : N) * p.tiles_y * p.tiles_x * p.mblocks;
  // (the launch picks its own S with bw as it is called, and never more than fits: size for the larger of the two)
  const int Sa = w43_slabs.pick(base, Cin / 4, true), Sb = w43_slabs.pick(base, Cin / 4, false);
  const int S = Sa > Sb ? Sa : Sb;
  return S > 1 ? (int64_t)S * base * W43_BM * 256 : 0;
}

// Modelled run time of the launch in microseconds (the model of w43_slabs; slabs != 0: with the K-slab form where it pays):
// what gsd_conv3x3_prefers_w2d compares the two-dimensional form against.
extern "C" double gsd_conv3x3_w43_estimate_us(int N, int H, int W, int Cin, int Cout, int slabs) {
  W43Plan p;
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || !plan_w43(N, H, W, Cout, &p)) return 0.0;
  const long base = (long)(p.fold ? 1 : N) * p.tiles_y * p.tiles_x * p.mblocks;
  const int nchunks = ceil_div(Cin, 4);
  const int S = (slabs && Cin % 4 == 0) ? w43_slabs.pick(base, nchunks, false) : 1;
  return w43_slabs.time_us(base, nchunks, S, false);
}

extern "C" int gsd_conv3x3_w43_partial_rows(int N, int H, int W, int Cout) {
  if (N <= 0 || H <= 0 || W <= 0 || Cout <= 0) return 0;
  W43Plan p;
  if (!plan_w43(N, H, W, Cout, &p)) return 0;
  return (p.fold ? 1 : N) * p.tiles_y * p.tiles_x * 4;
}

// MFMA instructions of one launch (all blocks, padding included), for gsd_conv3x3_algo
extern "C" int64_t gsd_conv3x3_w43_mfma_count(int N, int H, int W, int Cin, int Cout) {
  W43Plan p;
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || !plan_w43(N, H, W, Cout, &p)) return 0;
  return (int64_t)(p.fold ? 1 : N) * p.tiles_y * p.tiles_x * p.mblocks * ceil_div(Cin, 4) * (4 * 72);
}

static int w43_impl(const gsd_src* src, int nsrc, const float* wt, int Cin, int Cout, const gsd_dst* dst, int ndst,
                    float* partials, const Conv3Bw& bw, int N, int H, int W, void* stream, float* ws = nullptr, int64_t ws_elems = 0) {
  if (int e = conv3_check_operands("gsd_conv3x3_w43", true, false, src, nsrc, wt, Cin, Cout, dst, ndst, N, H, W)) return e;

  W43Plan pl;
  GSD_REQUIRE(plan_w43(N, H, W, Cout, &pl), GSD_ERR_UNSUPPORTED, "gsd_conv3x3_w43: no tile shape");
  if (pl.fold) {   // folded rows carry the image offset in 32-bit lane offsets
    for (int i = 0; i < nsrc; ++i)
      GSD_REQUIRE((int64_t)N * src[i].n_stride < (1LL << 31), GSD_ERR_UNSUPPORTED, "gsd_conv3x3_w43: batch too large for row folding");
    for (int i = 0; i < ndst; ++i)
      GSD_REQUIRE((int64_t)N * dst[i].n_stride < (1LL << 31), GSD_ERR_UNSUPPORTED, "gsd_conv3x3_w43: batch too large for row folding");
  }
  W43Params P;
  conv3_fill_common(P, src, nsrc, wt, Cin, Cout, dst, ndst, partials, bw, N, H, W);
  // 4-wave blocks, two per CU: they hide each other's barriers better than one 8-wave block shares its halo (measured +6 %
  // at Cin <= 512, profiles/bench_conv_forms.py); a loader wave cannot keep up without a deeper ring
  // straight fills (no per-slot bookkeeping): every 4-channel chunk lies inside one source segment
  const bool fast = Cin % 4 == 0 && (nsrc == 1 || src[0].C % 4 == 0);
  P.mblocks = pl.mblocks;
  P.TH = pl.TH; P.TW = pl.TW; P.TWq = pl.TWq; P.tiles_y = pl.tiles_y; P.tiles_x = pl.tiles_x;
  P.WR = pl.WR; P.WC = pl.WC; P.WCp = pl.WCp;
  P.PS = round_up(P.WR * P.WCp, 4) + 4;   // + one bank group: the four channel planes of a k-step start 16 B apart (mod 4)
  P.NPV = ceil_div(P.WR * P.WCp, 64);
  GSD_REQUIRE(P.NPV <= 8, GSD_ERR_UNSUPPORTED, "gsd_conv3x3_w43: halo window too large");
  // 16-byte halo pieces: every source row must start 16-byte aligned in the consumer's column grid
  P.NP = pl.TW / 4 + 2;
  P.RPI = 64 / P.NP;
  P.NI = ceil_div(P.WR, P.RPI);
  P.RO = 0;
  bool x4 = gsd_env_int("GSD_W43_X4", 1) != 0 && P.NI <= 2;
  for (int i = 0; i < nsrc && x4; ++i)
    x4 = ((uintptr_t)src[i].ptr & 15) == 0 && src[i].off_w % 4 == 0 && src[i].n_stride % 4 == 0 && src[i].c_stride % 4 == 0 &&
         (i == 0 ? P.src0.ws : P.src1.ws) % 4 == 0;
  if (x4) {
    P.WCp = P.NP * 4;      // LDS row pitch: the NP pieces of a window row, contiguous (one instruction spans RPI rows)
    P.RO = 4;
    int best = -1;
    for (int ps = P.WR * P.WCp + 4; ps < P.WR * P.WCp + 4 + 68; ps += 4) {
      const int c = conv3_halo_read_cycles(4, 1, pl.TWq, P.WCp, ps, P.RO);
      if (best < 0 || c < best) {
        best = c;
        P.PS = ps;
      }
    }
  }
  P.fold = pl.fold;
  P.nslab = 1;
  P.slabs = nullptr;
  const long grid = (long)(pl.fold ? 1 : N) * pl.tiles_y * pl.tiles_x * P.mblocks;
  GSD_REQUIRE(grid < 2147483647L, GSD_ERR_UNSUPPORTED, "gsd_conv3x3_w43: grid too large");
  const size_t lds = (size_t)(2 * (W43_WTILE + 4 * P.PS) + 2 * 4 * P.nchunks + 4 * W43_BM) * sizeof(float);
  bool plain = gsd_env_int("GSD_W43_PLAIN", 1) != 0;   // no deferred BatchNorm / ReLU on any source segment
  for (int i = 0; i < nsrc; ++i) plain = plain && src[i].scale == nullptr && src[i].relu == 0;
  // K slabs (the caller lends scratch): straight-fill form only; the slab count shrinks to what the scratch holds
  int S = 1;
  if (ws != nullptr && fast) {
    GSD_REQUIRE(((uintptr_t)ws & 15) == 0, GSD_ERR_BAD_ARG, "gsd_conv3x3_w43: workspace must be 16-byte aligned");
    S = w43_slabs.pick(grid, P.nchunks, bw.raw != nullptr);
    while (S > 1 && (int64_t)S * grid * W43_BM * 256 > ws_elems) --S;
    if (grid * S >= 2147483647L) S = 1;
  }
  if (gsd_env_set("GSD_W43_TRACE"))   // tuning: one line per launch, the kernel instantiation that runs
    fprintf(stderr, "w43 M%d K%d %dx%d N%d nsrc %d ndst %d plain %d x4 %d fast %d fold %d tile %dx%d slabs %d\n", Cout, Cin, H, W, N, nsrc,
            ndst, (int)plain, (int)x4, (int)fast, pl.fold, pl.TH, pl.TW, S);
  if (S > 1) {
    P.nslab = S;
    P.slabs = ws;
    return launch_split(P, (int)grid, lds, (hipStream_t)stream, x4, plain);
  }
  return launch_w43(P, (int)grid, lds, (hipStream_t)stream, x4, fast, plain);
}

extern "C" int gsd_conv3x3_w43(const gsd_src* src, int nsrc, const float* wt, int Cin, int Cout, const gsd_dst* dst, int ndst,
                               float* partials, int N, int H, int W, void* stream) {
  return w43_impl(src, nsrc, wt, Cin, Cout, dst, ndst, partials, Conv3Bw{}, N, H, W, stream);
}

extern "C" int gsd_conv3x3_w43_ws(const gsd_src* src, int nsrc, const float* wt, int Cin, int Cout, const gsd_dst* dst, int ndst,
                                  float* partials, float* ws, int64_t ws_elems, int N, int H, int W, void* stream) {
  return w43_impl(src, nsrc, wt, Cin, Cout, dst, ndst, partials, Conv3Bw{}, N, H, W, stream, ws, ws_elems);
}

extern "C" int gsd_conv3x3_w43_dgrad_bnrelu(const gsd_src* src, const float* wt, int Cin, int Cout, const gsd_dst* dst,
                                            const float* raw, const float* scale, const float* shift, const float* mean,
                                            const float* invstd, float* partials, int N, int H, int W, void* stream) {
  return gsd_conv3x3_w43_dgrad_bnrelu_ws(src, wt, Cin, Cout, dst, raw, scale, shift, mean, invstd, partials, nullptr, 0, N, H, W, stream);
}

extern "C" int gsd_conv3x3_w43_dgrad_bnrelu_ws(const gsd_src* src, const float* wt, int Cin, int Cout, const gsd_dst* dst,
                                               const float* raw, const float* scale, const float* shift, const float* mean,
                                               const float* invstd, float* partials, float* ws, int64_t ws_elems, int N, int H,
                                               int W, void* stream) {
  const Conv3Bw bw{raw, scale, shift, mean, invstd};
  if (int e = conv3_check_dgrad_bnrelu("gsd_conv3x3_w43_dgrad_bnrelu", dst, bw, partials, Cout, H, W)) return e;
  return w43_impl(src, 1, wt, Cin, Cout, dst, 1, partials, bw, N, H, W, stream, ws, ws_elems);
}
