// gsd_conv3x3_w2d_kernel.h -- the device code of the two-dimensional Winograd conv3x3 (gsd_conv3x3_w2d.hip has the description):
// kernel parameters, the epilogue and the block body w2d_block -- prologue, chunk loop, accumulator trade, output transform --
// shared by conv3x3_w2d_kernel (rectangular TH x TW pixel tiles, gsd_conv3x3_w2d.hip) and conv3x3_w2d_strips_kernel (the band-major
// flat tile list of the deep levels, gsd_conv3x3_w2d_strips.hip).  The two differ in which tiles a block owns, in where the halo
// pieces of a window come from and lie in LDS, and in the image a lane's tile belongs to; every `if constexpr (STRIPS)` below is
// one of those three.
#pragma once
#include "gsd_conv3x3_host.h"

#include <cstdio>
#include <cstdlib>
#include <type_traits>

typedef float f32x4v __attribute__((ext_vector_type(4), aligned(4)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
// global-memory views at a scalar 64-bit base plus an unsigned 32-bit lane offset (the address space is spelled out: a pointer that
// went through an opaque scalar is generic otherwise, and a generic access is a flat instruction with a 64-bit vector address)
typedef __attribute__((address_space(1))) f32x4v g_f32x4v;
typedef __attribute__((address_space(1))) float g_float;
typedef __attribute__((address_space(1))) char g_char;
typedef __attribute__((address_space(3))) f32x4 l_f32x4;   // ... and LDS views
typedef __attribute__((address_space(3))) float l_float;
__device__ __forceinline__ g_f32x4v* w2d_g4(g_char* base, unsigned off) { return (g_f32x4v*)(base + off); }
__device__ __forceinline__ g_float* w2d_g1(g_char* base, unsigned off) { return (g_float*)(base + off); }

// Division of a non-negative int by a launch constant d >= 1 as a multiply-high and two shifts (Granlund & Montgomery): the host
// computes l = ceil(log2 d), mul = floor(2^32 (2^l - d) / d) + 1, and q = (t + ((x - t) >> min(l, 1))) >> max(l - 1, 0) with
// t = mulhi(x, mul) is floor(x / d) for every 32-bit x.  On wave-uniform operands it is five scalar instructions; hipcc's own
// expansion of a division is some twenty vector instructions (v_rcp_iflag_f32 and a correction), uniform operands or not.
struct W2DDiv {
  unsigned mul, s1, s2;
};
static inline W2DDiv w2d_div_of(unsigned d) {
  unsigned l = 0;
  while ((1ull << l) < d) ++l;
  W2DDiv r;
  r.mul = (unsigned)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
  r.s1 = l < 1 ? l : 1;
  r.s2 = l > 0 ? l - 1 : 0;
  return r;
}
__device__ __forceinline__ int w2d_div(int x, const W2DDiv& d) {
  const unsigned t = __umulhi((unsigned)x, d.mul);
  return (int)((t + (((unsigned)x - t) >> d.s1)) >> d.s2);
}

struct W2DParams {
  SrcD src0, src1;
  DstD dst0, dst1;
  const float* wt;   // [mblocks][nchunks][4 ci][12 frequency pairs][2 channel halves][16][2 (f & 1)][2 m-tiles]: gsd_weight_layout modes 8 / 9
  float* partials;   // [pixel tiles * NWP][2 * Mpad]: row (pixel tile, pixel group of the block)
  const float* bw_raw;
  const float* bw_scale;
  const float* bw_shift;
  const float* bw_mean;
  const float* bw_invstd;
  int Cin, Cout, Mpad, nchunks, mblocks;
  int N, H, W;
  int TH, TW, TWq, tiles_y, tiles_x, WR, WC, WCp, PS, NPV;
  int NP, NI;   // X4: 16-byte pieces per window row (TW / 4 + 2), DMA instructions per channel plane
  int mgrp, pgrp, ptiles;   // block order of the deep levels: passes of mgrp m-blocks over groups of pgrp of the ptiles pixel tiles
  W2DDiv d_mblocks, d_nslab, d_tpi, d_tiles_x, d_NP, d_WCp;   // divisions by mblocks, nslab, tiles_y * tiles_x, tiles_x, NP, WCp
  int TWq_sh;   // log2 TWq (tiles are 8, 16, 32 or 64 pixels wide)
  int dfast;    // bit d: destination d's planes are within an unsigned 32-bit byte offset of each other (the interior epilogue)
  int nslab;    // K slabs (SPLIT): block (tile, slab k, m-block) runs chunks [k n / S, (k + 1) n / S) and stores its un-reduced
  float* slabs; // 2 x 4 outputs per channel and Winograd tile to [tile][slab][m-block][64 channels][16 NWP tiles][8] floats
};

// ---- the band-major flat tile list (conv3x3_w2d_strips_kernel) --------------------------------------------------------------------
// A BAND is two Winograd tile rows (four pixel rows) of one image across its full width, from an even tile row on; an odd count of
// tile rows leaves a last band of one.  The tiles of a launch are listed image by image, band by band, inside a band column by
// column, inside a column the upper tile then the lower.  Pixel group g owns tiles [16 g, 16 g + 16), block b groups 2 b and 2 b + 1:
// no slot is empty but at the list's end.  Inside a group the tiles of one band are a STRIP: a run of whole tile columns c0 .. c0 + c - 1
// whose window is six rows of c + 2 16-byte pieces (its own left and right halo included); the strips of a group lie side by side
// in each of the six rows of the group's window, strip k from piece s0 on.  Every tile keeps the anchor it has in an image of its
// own (even row, column a multiple of 4): its 4 x 6 window, its 24 products per channel and its output transform are those of the
// rectangular form, bit for bit.
constexpr int W2D_STRIPS = 3;        // strips of a group the kernel handles
constexpr int W2D_STRIP_NP = 14;     // pieces of a window row: 8 columns and three strips' halos

struct W2DStrip {
  int n, band;      // image, band
  int c0, c;        // first tile column, tile columns (0: no such strip)
  int s0;           // first piece inside the group's window rows
  int t0, take;     // the group's tiles of this strip: flat ids [t0, t0 + take)
  int rb, two;      // position of tile t0 inside its band's list; 1: the band has two tile rows
};

// THE map of the listing: strips k = 0 .. K - 1 of pixel group g of an N-image launch with TY x TX Winograd tiles per image.
// Returns the number of strips the group has, counted up to K + 1 (so a caller sees that K did not hold them).
template <int K>
__host__ __device__ inline int w2d_group_strips(const int g, const int N, const int TY, const int TX, W2DStrip (&out)[K]) {
  const int tpi = TY * TX, nt = N * tpi;
  const int g1 = 16 * g + 16 < nt ? 16 * g + 16 : nt;
  int s = 16 * g, s0 = 0, count = 0;
#pragma unroll
  for (int k = 0; k <= K; ++k) {
    if (s >= g1) {
      if (k < K) out[k] = W2DStrip{0, 0, 0, 0, 0, s, 0, 0, 0};
      continue;
    }
    ++count;
    if (k == K) continue;
    const int n = s / tpi, r = s - n * tpi;
    const int band = r / (2 * TX), rb = r - band * (2 * TX);
    const int two = 2 * band + 1 < TY ? 1 : 0;
    const int left = (two ? 2 * TX : TX) - rb;
    const int take = left < g1 - s ? left : g1 - s;
    const int c0 = two ? rb >> 1 : rb, cl = two ? (rb + take - 1) >> 1 : rb + take - 1;
    out[k] = W2DStrip{n, band, c0, cl - c0 + 1, s0, s, take, rb, two};
    s0 += cl - c0 + 3;
    s += take;
  }
  return count;
}

// Tile t of the list: image (< 0: past the end of the list, an empty lane), tile row, tile column, and where its window lies in its
// group's: strip index and first piece (its own column's piece is one further).
struct W2DTile {
  int n, ty, tx, strip, piece;
};
template <int K>
__host__ __device__ inline W2DTile w2d_tile_of(const int t, const int N, const int TY, const int TX, const W2DStrip (&st)[K]) {
  W2DTile r = {-1, 0, 0, 0, 0};
  if (t >= N * TY * TX) return r;
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (st[k].c > 0 && t >= st[k].t0 && t < st[k].t0 + st[k].take) {
      const int p = st[k].rb + t - st[k].t0;
      const int col = st[k].two ? p >> 1 : p;
      r = W2DTile{st[k].n, 2 * st[k].band + (st[k].two ? p & 1 : 0), col, k, st[k].s0 + col - st[k].c0};
    }
  return r;
}

// Kernel arguments of the strips form beside W2DParams (whose TH / TW / tiles_* fields it does not read; WCp is the window's row
// pitch in floats, PS the plane stride, ptiles the blocks of the list)
struct W2DStrips {
  int TY, TX;       // Winograd tiles down and across an image
  int GS;           // floats between the windows of a block's two groups inside a channel plane (6 WCp)
  int nblocks;      // blocks of the list: ceil(N TY TX / 32)
  int prows;        // partial rows the caller will reduce: the rectangular form's count (w2d_strips_rows_kernel writes them)
  float* rows;      // ... and where they go (W2DParams::partials is the per-tile scratch, or null: no statistics)
};

// host side of the strips form (gsd_conv3x3_w2d_strips.hip); the launcher of gsd_conv3x3_w2d.hip decides and hands over
struct W2DStripPlan {
  int TY, TX, nblocks, max_strips, max_pieces, PS;   // PS: the windows' plane stride in floats (0: the kernel does not admit the list)
};
bool w2d_strips_plan(int N, int H, int W, W2DStripPlan* p);
int w2d_strips_launch(W2DParams P, const W2DStripPlan& pl, const gsd_dst* dst, int ndst, float* scratch, hipStream_t st);
// floats of per-tile statistics scratch a strips launch with partial rows needs
static inline int64_t w2d_strips_scratch_elems(const W2DStripPlan& pl, int Mpad) { return (int64_t)pl.nblocks * 32 * 2 * Mpad; }

namespace {
constexpr int W2D_BM = 64;
constexpr int W2D_WTILE = 96 * W2D_BM;   // floats per weight chunk (24 KiB)
constexpr int NWP = 2;                    // pixel groups of 16 tiles (128 pixels) per block
}  // namespace

// ---- epilogue (shared by the conv kernel and the K-slab reducer): a lane holds the 2 x 4 outputs of its Winograd tile for the
// wave's eight channel groups (m-tile m, register reg: channel cu + 4 j, cu = m0 + 32 mh + 16 m + reg) and hands them over two at a
// time, get_pair(p, y): y[e][row][column] of (m, reg) = (p >> 1, 2 (p & 1) + e).  NCHW stores (two destination segments with crop),
// BatchNorm partial sums, or the fused BatchNorm-backward form.  sBw: the block's [4][64] coefficients of that form in LDS.
//
// Two paths behind one wave-uniform test.  INTERIOR waves -- every lane's tile lies wholly inside the image and inside the crop of
// the one destination that holds all 32 channels of the wave -- run without a mask: unconditional 16-byte stores at a scalar plane
// base plus one unsigned 32-bit lane offset per tile row (P.dfast: the host vouches that such an offset spans the wave's planes).
// Every other wave (edge tiles, a channel tail, a wave that straddles the two destinations) takes the masked path.  Both add the
// statistics in the same order, pixel by pixel: the paths are bit-identical where both apply.
// LN (the strips form): the lanes' tiles lie in different images -- `n` is the lane's own, the interior path carries the image in
// the lane offsets (dfast then vouches for the whole tensor) and h0 = w0 = 0, tr2 / tq the tile's row and column in its image.
template <bool LN = false, class GetPair>
__device__ __forceinline__ void w2d_epilogue(const W2DParams& P, const float* sBw, const int n, const int h0, const int w0, const int tr2,
                                             const int tq, const int vmask, const int m0, const int mh, const int ph, const int j,
                                             const int l16, const int pt, GetPair get_pair) {
  constexpr int BM = 64;
  // LN: P.partials is the per-TILE scratch [tile of the list][2 Mpad] -- every lane leaves its own tile's sums, un-reduced, and
  // w2d_strips_rows_kernel adds them in the rectangular form's rows and lane order (the statistics keep their bits)
  float* const prow = P.partials != nullptr ? P.partials + (size_t)(pt * NWP + ph) * (LN ? 16 : 1) * (2 * P.Mpad) : nullptr;
  float* const prow_l = LN && prow != nullptr ? prow + (size_t)l16 * (2 * P.Mpad) : prow;
  const int mc = m0 + mh * 32;   // the wave's channels: mc .. mc + 31
  {
    const bool in1 = mc >= P.dst0.C;
    const int d_oh = in1 ? P.dst1.oh : P.dst0.oh, d_ow = in1 ? P.dst1.ow : P.dst0.ow, d_H = in1 ? P.dst1.H : P.dst0.H;
    const int d_W = in1 ? P.dst1.W : P.dst0.W, d_ws = in1 ? P.dst1.ws : P.dst0.ws;
    const long long d_cs = in1 ? P.dst1.cs : P.dst0.cs, d_ns = in1 ? P.dst1.ns : P.dst0.ns;
    const int hd = h0 + 2 * tr2 - d_oh, wd = w0 + 4 * tq - d_ow;
    const bool lane_in = vmask == 0xff && hd >= 0 && hd + 2 <= d_H && wd >= 0 && wd + 4 <= d_W;
    const bool chan_in = (in1 ? mc + 32 <= P.Cout : mc + 32 <= P.dst0.C) && (P.dfast >> (in1 ? 1 : 0) & 1) != 0;
    if (chan_in && __builtin_amdgcn_ballot_w64(lane_in) == ~0ull) {
      // lane offsets in bytes from the plane of channel cu (the lane's own plane is 4 j further)
      unsigned o0 = ((unsigned)(j * 4) * (unsigned)d_cs + (unsigned)(hd * d_ws + wd)) * 4u;
      if constexpr (LN) o0 += (unsigned)n * (unsigned)d_ns * 4u;
      unsigned o1 = o0 + (unsigned)d_ws * 4u;
      unsigned oj = (unsigned)j * 16u + (LN ? (unsigned)l16 * (unsigned)(2 * P.Mpad) * 4u : 0u);
      asm volatile("" : "+v"(o0), "+v"(o1), "+v"(oj));
      const long long pl0 = (LN ? 0ll : (long long)n * d_ns) + (long long)(mc - (in1 ? P.dst0.C : 0)) * d_cs;   // the wave's first plane
#pragma unroll
      for (int p = 0; p < 4; ++p) {
      float y[2][2][4], s1v[2], s2v[2];
      get_pair(p, y);
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int cw = (p >> 1) * 16 + (p & 1) * 2 + c;   // channel cu - mc
        g_char* dp = (g_char*)((in1 ? P.dst1.p : P.dst0.p) + pl0 + (long long)cw * d_cs);
        asm volatile("" : "+s"(dp));
        float s1 = 0.f, s2 = 0.f;
        if (P.bw_raw == nullptr) {
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              s1 += y[c][a][i];
              s2 = fmaf(y[c][a][i], y[c][a][i], s2);
            }
        } else {
          g_char* rp = (g_char*)(P.bw_raw + pl0 + (long long)cw * d_cs);
          asm volatile("" : "+s"(rp));
          asm volatile("" : "+v"(o0), "+v"(o1));
          const f32x4 x0 = *w2d_g4(rp, o0), x1 = *w2d_g4(rp, o1);
          const int cl = mh * 32 + (p >> 1) * 16 + j * 4 + (p & 1) * 2 + c;
          const float bsc = sBw[cl], bsh = sBw[BM + cl], bmu = sBw[2 * BM + cl], bis = sBw[3 * BM + cl];
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float x = a == 0 ? x0[i] : x1[i];
              const float dz = fmaf(x, bsc, bsh) > 0.f ? y[c][a][i] : 0.f;
              y[c][a][i] = dz;
              s1 += dz;
              s2 = fmaf(dz, (x - bmu) * bis, s2);
            }
        }
        asm volatile("" : "+v"(o0), "+v"(o1));   // (in the store's own block: hipcc otherwise zero-extends them once, as 64-bit vector addends)
        *w2d_g4(dp, o0) = f32x4{y[c][0][0], y[c][0][1], y[c][0][2], y[c][0][3]};
        *w2d_g4(dp, o1) = f32x4{y[c][1][0], y[c][1][1], y[c][1][2], y[c][1][3]};
        s1v[c] = LN ? s1 : reduce16_to_lane15(s1);
        s2v[c] = LN ? s2 : reduce16_to_lane15(s2);
      }
      if (prow != nullptr && (LN || l16 == 15)) {   // (mc + 32 <= Cout <= Mpad: every channel has its column)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          g_char* pp = (g_char*)(prow + mc + (p >> 1) * 16 + (p & 1) * 2 + c);
          asm volatile("" : "+s"(pp));
          asm volatile("" : "+v"(oj));
          *w2d_g1(pp, oj) = s1v[c];
          *w2d_g1(pp + (size_t)P.Mpad * 4, oj) = s2v[c];
        }
      }
      }
      return;
    }
  }
  // ---- the masked path.  Per destination and tile row: element offset of the row's first pixel inside a plane, and the mask of its
  // pixels that are stored
  // (scalars, not arrays: `first ? off0(a) : off1(a)` on arrays makes hipcc select between two ADDRESSES and keep the arrays in scratch)
  int off0_0 = 0, off0_1 = 0, off1_0 = 0, off1_1 = 0, sm0_0 = 0, sm0_1 = 0, sm1_0 = 0, sm1_1 = 0;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int h = h0 + 2 * tr2 + a, w = w0 + 4 * tq;
    const int vm = (vmask >> (4 * a)) & 15;
    int hd = h - P.dst0.oh, wd = w - P.dst0.ow;
    if ((unsigned)hd < (unsigned)P.dst0.H) {
      (a == 0 ? off0_0 : off0_1) = hd * P.dst0.ws + wd;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if ((vm >> i & 1) && (unsigned)(wd + i) < (unsigned)P.dst0.W) (a == 0 ? sm0_0 : sm0_1) |= 1 << i;
    }
    hd = h - P.dst1.oh;
    wd = w - P.dst1.ow;
    if ((unsigned)hd < (unsigned)P.dst1.H) {
      (a == 0 ? off1_0 : off1_1) = hd * P.dst1.ws + wd;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if ((vm >> i & 1) && (unsigned)(wd + i) < (unsigned)P.dst1.W) (a == 0 ? sm1_0 : sm1_1) |= 1 << i;
    }
  }
  auto OFF0 = [&](int a) { return a == 0 ? off0_0 : off0_1; };   // (a is a constant of the unrolled loops)
  auto OFF1 = [&](int a) { return a == 0 ? off1_0 : off1_1; };
  auto SM0 = [&](int a) { return a == 0 ? sm0_0 : sm0_1; };
  auto SM1 = [&](int a) { return a == 0 ? sm1_0 : sm1_1; };
  const long long lane0 = (long long)(j * 4) * P.dst0.cs, lane1 = (long long)(j * 4) * P.dst1.cs;
  float* const d0 = P.dst0.p + (long long)n * P.dst0.ns;
  float* const d1 = P.dst1.p + (long long)n * P.dst1.ns;

#pragma unroll
  for (int p = 0; p < 4; ++p) {
  float y[2][2][4];
  get_pair(p, y);
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    // channel = wave-uniform part cu + the lane's 4 j: the plane offset of cu is scalar arithmetic, the lane's share (lane0 / lane1)
    // is multiplied once -- a 64-bit vector multiply per channel otherwise
    const int m = p >> 1, reg = (p & 1) * 2 + c;
    const int cu = mc + m * 16 + reg, co = cu + j * 4;
    float s1 = 0.f, s2 = 0.f;
    if (P.bw_raw == nullptr) {
      const bool first = co < P.dst0.C;
      const int cd = first ? co : co - P.dst0.C;
      const bool co_ok = co < P.Cout && (first || cd < P.dst1.C);
      float* const plane = first ? d0 + (long long)cu * P.dst0.cs + lane0 : d1 + (long long)(cu - P.dst0.C) * P.dst1.cs + lane1;
      // statistics over the pixels that are STORED (for a cropped second destination -- the backward of F.pad -- the sums are
      // those of the crop, e.g. the ConvT bias gradient)
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int sm = co_ok ? (first ? SM0(a) : SM1(a)) : 0;
        float* const px = plane + (first ? OFF0(a) : OFF1(a));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (sm >> i & 1) {
            s1 += y[c][a][i];
            s2 = fmaf(y[c][a][i], y[c][a][i], s2);
          }
        }
        if (sm == 15) {
          *reinterpret_cast<f32x4v*>(px) = f32x4{y[c][a][0], y[c][a][1], y[c][a][2], y[c][a][3]};
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (sm >> i & 1) px[i] = y[c][a][i];
        }
      }
    } else {
      // dst0 is the gradient buffer of a conv+BN+ReLU unit whose raw output has the same geometry: dz = relu'(bn(raw)) * dX
      const long long cplane = (long long)n * P.dst0.ns + (co < P.Cout ? (long long)cu * P.dst0.cs + lane0 : 0);
      float xr[2][4];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const float* const rp = P.bw_raw + cplane + OFF0(a);
        if (SM0(a) == 15) {
          const f32x4 t = *reinterpret_cast<const f32x4v*>(rp);
          xr[a][0] = t[0], xr[a][1] = t[1], xr[a][2] = t[2], xr[a][3] = t[3];
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) xr[a][i] = (SM0(a) >> i & 1) ? rp[i] : 0.f;
        }
      }
      const int cl = mh * 32 + m * 16 + j * 4 + reg;
      const float bsc = sBw[cl], bsh = sBw[BM + cl], bmu = sBw[2 * BM + cl], bis = sBw[3 * BM + cl];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int sm = co < P.Cout ? SM0(a) : 0;
        float* const px = d0 + ((long long)cu * P.dst0.cs + lane0) + OFF0(a);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float x = xr[a][i];
          const float dz = ((sm >> i & 1) && fmaf(x, bsc, bsh) > 0.f) ? y[c][a][i] : 0.f;
          y[c][a][i] = dz;
          s1 += dz;
          s2 = fmaf(dz, (x - bmu) * bis, s2);
        }
        if (sm == 15) {
          *reinterpret_cast<f32x4v*>(px) = f32x4{y[c][a][0], y[c][a][1], y[c][a][2], y[c][a][3]};
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (sm >> i & 1) px[i] = y[c][a][i];
        }
      }
    }
    if (prow != nullptr) {
      if constexpr (!LN) {
        s1 = reduce16_to_lane15(s1);
        s2 = reduce16_to_lane15(s2);
      }
      if ((LN || l16 == 15) && co < P.Mpad) {
        prow_l[co] = s1;
        prow_l[P.Mpad + co] = s2;
      }
    }
  }
  }
}

// PLAIN: no source segment carries a deferred BatchNorm or ReLU (every dX launch; the pooled / up-sampled sources of the forward)
// NWP = 2 pixel groups per block: four waves, 64 channels x 256 pixels, two blocks per CU (measured faster than one eight-wave
// block of 64 x 512 pixels per CU, profiles/r05_w2d_vs_w43.txt).
//
// X4: the halo windows move as ALIGNED 16-byte pieces (global_load_lds_dwordx4) instead of dword gathers: a quarter of the halo's
// DMA instructions (2 instead of 6 per channel plane of a 10 x 34 window), and the LDS-DMA issue -- 60-180 cycles an instruction --
// is what this kernel waits for besides its MFMAs.  Possible when every source row starts 16-byte aligned and a piece lies wholly
// inside or wholly outside a row: ONE plain source segment with a row pitch that is a multiple of 4 floats whose pad columns hold
// zeros -- the row-pitched d_raw buffer every dX launch reads (gsd_bn_bwd_apply's out-of-place form).  A window row is the NP =
// TW/4 + 2 pieces that cover image columns w0-4 .. w0+TW+3; the planes are shifted by ONE float in LDS so that image column w0-1
// lands 16-byte aligned and the consumer reads stay one b128 + one b64 per window row.
//
// HM = 2 ("U4"): the same 16-byte pieces on the same w0-4 piece grid, straight from UNALIGNED rows -- any source (a
// global_load_lds_dwordx4 takes any 4-byte aligned global address at full rate).  On that grid a piece never straddles the LEFT
// image edge of a segment that starts at column 0; one that straddles a segment's right edge (W % 4 != 0: every level of the
// U-Net) is loaded as it lies in memory -- the caller vouches for 4 readable floats around the tensor, gsd_src.slack -- and the
// lane that moved it overwrites its outside floats with the padding value once its own fills have landed, in front of the chunk's
// barrier (only lanes of blocks at that edge do anything).
//
// SPLIT (K slabs, as gsd_conv3x3_w43.hip): a launch whose tile grid leaves most of the chip's 512 block slots empty (the 40 x 53 and
// 20 x 26 levels at small batches) is cut along the input channels; the output transform is linear, so each slab stores its own
// Y = A2^T M A4 and w2d_slab_reduce_kernel adds the slabs in slab order and runs the epilogue.  A slab that starts inside the
// second (concat) segment starts its fills there.
//
// STRIPS (conv3x3_w2d_strips_kernel; PLAIN, X4, not SPLIT): the block owns 32 consecutive tiles of the band-major list instead of a
// TH x TW rectangle.  A channel plane holds the two groups' windows, six rows of W2D_STRIP_NP pieces each (168 pieces: three fill
// instructions per plane, twelve units per chunk, three per wave); every piece belongs to one (image, band, row), so its lane's
// source offset -- the image's included -- is computed once, here, and a chunk moves the wave-uniform base as in the rectangular
// form: nothing is patched per chunk, and the chunk loop is the same code.
template <bool PLAIN, int HM, bool SPLIT, bool STRIPS>
__device__ __forceinline__ void w2d_block(const W2DParams& P, const W2DStrips& SP) {
  constexpr bool X4 = HM == 1, U4 = HM == 2, PC = HM != 0;   // PC: the halo lies in LDS as 16-byte pieces
  static_assert(!STRIPS || (PLAIN && X4 && !SPLIT), "the strip list: plain aligned pieces, no K slabs");
  constexpr int NPP = STRIPS ? 3 : 2;   // fill units of a wave per chunk
  constexpr int W2D_NONE = -2147483647 - 1, W2D_PAD = -2147483647;   // lane offsets: no position / a padding position (prefilled)
  constexpr unsigned W2D_OFF_PAD = 0xFFFFFFFFu;                        // ... as a byte offset of the fills
  static_assert(!X4 || PLAIN, "aligned 16-byte halo pieces: a plain, row-pitched source");
  constexpr int BM = W2D_BM, WTILE = W2D_WTILE, NT = 128 * NWP, NW = 2 * NWP;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int PS = P.PS;
  const int BUF = WTILE + 4 * PS;
  const int Kpad = STRIPS ? 0 : P.nchunks * 4;   // (STRIPS: plain sources, no affine table -- LDS the two blocks of a CU need)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave8 = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ph = wave8 % NWP, fh = wave8 / NWP;   // the wave's pixel group (16 of the block's 16 NWP tiles) and frequency-row half
  const int j = lane >> 4, l16 = lane & 15;

  // the m-blocks of one pixel tile read the same halo: every XCD gets a contiguous range of logical ids (pixel tile major)
  const int lid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int lid_m = w2d_div(lid, P.d_mblocks);
  int mbb = lid - lid_m * P.mblocks;
  int pt = SPLIT ? w2d_div(lid_m, P.d_nslab) : lid_m;
  const int slab = SPLIT ? lid_m - pt * P.nslab : 0;
  if (!SPLIT && P.mgrp < P.mblocks) {
    // Deep levels: an m-block's weight image (24 KiB per chunk) is megabytes, and the blocks in flight on an XCD are at arbitrary
    // phases of their chunk loops once the first round is over -- with every m-block of a pixel tile in flight at once, the eight or
    // sixteen weight streams evict each other from the 4-MiB L2 and nearly every weight fill misses it (measured: 7.0 GB of L2 misses
    // per 40 x 53 512 -> 512 launch, the weight fills are 7.9 GB).  So the ids walk groups of `pgrp` pixel tiles, and inside a group
    // the m-blocks in passes of `mgrp` (as many as fit the L2): the blocks in flight share mgrp weight images; the tile windows
    // (a quarter of the weights' bytes) are what a later pass reads again.
    const int gsz = P.pgrp * P.mblocks;
    const int g = lid / gsz;
    int r = lid - g * gsz;
    const int p0 = g * P.pgrp;
    const int pn = min(P.pgrp, P.ptiles - p0);          // (the last pixel group may be short)
    const int per = pn * P.mgrp;
    const int mg = r / per;
    r -= mg * per;
    const int gn = min(P.mgrp, P.mblocks - mg * P.mgrp);   // (and the last pass)
    const int pl = r / gn;
    pt = p0 + pl;
    mbb = mg * P.mgrp + (r - pl * gn);
  }
  const int c_lo = SPLIT ? __builtin_amdgcn_readfirstlane((int)((long)slab * P.nchunks / P.nslab)) : 0;
  const int c_hi = SPLIT ? __builtin_amdgcn_readfirstlane((int)((long)(slab + 1) * P.nchunks / P.nslab)) : P.nchunks;
  const int m0 = mbb * BM;
  const int tpi = STRIPS ? 1 : P.tiles_y * P.tiles_x;
  const int n = STRIPS ? 0 : w2d_div(pt, P.d_tpi);   // (STRIPS: the image is the lane's, and part of its offsets)
  const int rt = pt - n * tpi;
  const int ty = STRIPS ? 0 : w2d_div(rt, P.d_tiles_x);
  const int h0 = STRIPS ? 0 : ty * P.TH, w0 = STRIPS ? 0 : (rt - ty * P.tiles_x) * P.TW;

  // ---- this lane's Winograd tile: 2 x 4 pixels (rows 2*tr2, 2*tr2+1; columns 4*tq .. 4*tq+3) of the block's TH x TW tile ------
  const int q = ph * 16 + l16;
  int baddr_, geo_;
  if constexpr (STRIPS) {
    // tile 16 (2 pt + ph) + l16 of the list: its window starts at piece `piece` of window rows 2 row .. 2 row + 3 of the group's six
    W2DStrip st[W2D_STRIPS];
    w2d_group_strips(2 * pt + ph, P.N, SP.TY, SP.TX, st);
    const W2DTile t = w2d_tile_of(32 * pt + q, P.N, SP.TY, SP.TX, st);
    baddr_ = WTILE + j * PS + ph * SP.GS + (t.n < 0 ? 0 : (2 * (t.ty & 1)) * P.WCp + 4 * t.piece) + 4;
    geo_ = 0;   // (the epilogue maps the tile again: nothing of it crosses the loop)
  } else {
  const bool q_ok = q < (P.TH >> 1) * P.TWq && q < 16 * NWP;
  const int tr2 = q_ok ? q >> P.TWq_sh : 0;
  const int tq = q_ok ? q - tr2 * P.TWq : 0;
  baddr_ = WTILE + j * PS + (2 * tr2) * P.WCp + 4 * tq + (PC ? 4 : 0);   // halo columns 4*tq .. 4*tq+5 of halo rows 2*tr2 .. 2*tr2+3
  int vmask = 0;   // bits 0..3: pixels of the tile's first row that exist in the image, bits 4..7: of its second row
  if (q_ok) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
      if (h0 + 2 * tr2 + a < P.H) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (w0 + 4 * tq + i < P.W) vmask |= 1 << (4 * a + i);
      }
  }

  // (the epilogue's lane geometry crosses the loop in ONE register: the accumulators leave none to spare)
  geo_ = tr2 | tq << 8 | vmask << 16;
  }
  const int baddr = baddr_;
  int geo = geo_;
  asm volatile("" : "+v"(geo));

  // ---- halo DMA lane geometry: the block's waves cover the (up to) 128 NW window positions once, dword gathers --------------------
  // seg_offsets: this lane's source element offsets in segment seg (W2D_PAD: a padding position, W2D_NONE: no position); the
  // second segment's wait in LDS for the switch rather than in registers through the chunk loop
  bool p_on[NPP];
  int pmask = 0;   // U4: floats of this lane's pieces that lie outside their row (bits 4 pp .. 4 pp + 3: first segment, + 8: second)
  auto seg_offsets = [&](const int seg, int (&xo)[NPP]) __attribute__((always_inline)) {
    const SrcD& S = seg ? P.src1 : P.src0;
    if constexpr (STRIPS) {
      // unit u = (channel plane u / 3, instruction u % 3): piece (u % 3) 64 + lane of the plane's 2 groups x 6 rows x 14 pieces.  The
      // piece lies in one strip of its group or in none; its source is row 4 band - 1 + rr, columns 4 (c0 - 1 + pc - s0) .. + 3 of
      // the strip's image, whose offset is part of the lane's (the host vouches for 32 bits)
      W2DStrip st[2][W2D_STRIPS];
      w2d_group_strips(2 * pt, P.N, SP.TY, SP.TX, st[0]);
      w2d_group_strips(2 * pt + 1, P.N, SP.TY, SP.TX, st[1]);
#pragma unroll
      for (int pp = 0; pp < NPP; ++pp) {
        xo[pp] = W2D_NONE;
        p_on[pp] = true;
        const int piece = ((wave8 + NW * pp) % 3) * 64 + lane;
        if (seg == 0 && piece < 2 * 6 * W2D_STRIP_NP) {
          const int gg = piece >= 6 * W2D_STRIP_NP ? 1 : 0, qq = piece - gg * (6 * W2D_STRIP_NP);
          const int rr = qq / W2D_STRIP_NP, pc = qq - rr * W2D_STRIP_NP;
#pragma unroll
          for (int k = 0; k < W2D_STRIPS; ++k) {
            const int kc = gg ? st[1][k].c : st[0][k].c, ks0 = gg ? st[1][k].s0 : st[0][k].s0;
            if (kc > 0 && pc >= ks0 && pc < ks0 + kc + 2) {
              const int kn = gg ? st[1][k].n : st[0][k].n, kb = gg ? st[1][k].band : st[0][k].band;
              const int gh = 4 * kb - 1 + rr, gw = 4 * ((gg ? st[1][k].c0 : st[0][k].c0) - 1 + pc - ks0);
              xo[pp] = ((unsigned)gh < (unsigned)S.H && gw >= 0 && gw + 4 <= S.ws) ? kn * (int)S.ns + gh * S.ws + gw : W2D_PAD;
            }
          }
        }
      }
      return;
    }
#pragma unroll
    for (int pp = 0; pp < 2; ++pp) {
      xo[pp] = W2D_NONE;
      if constexpr (PC) {
        // unit u = (channel plane u / NI, instruction u % NI) of the chunk: its 64 lanes are 64 consecutive pieces of the plane
        const int u = wave8 + NW * pp;
        p_on[pp] = u < 4 * P.NI;
        const int piece = (u & (P.NI - 1)) * 64 + lane;   // (NI is 1 or 2: the launcher takes the 16-byte pieces only then)
        const int rr = w2d_div(piece, P.d_NP), pc = piece - rr * P.NP;
        if (rr < P.WR) {
          const int gh = h0 - 1 + rr, gw = w0 - 4 + 4 * pc;
          if constexpr (X4) {
            xo[pp] = ((unsigned)gh < (unsigned)S.H && gw >= 0 && gw + 4 <= S.ws) ? gh * S.ws + gw : W2D_PAD;
          } else {
            const int hs = gh - S.oh, c0 = gw - S.ow;
            xo[pp] = W2D_PAD;
            if (S.C > 0 && (unsigned)hs < (unsigned)S.H && c0 + 3 >= 0 && c0 < S.W) {
              xo[pp] = hs * S.ws + c0;
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (c0 + e < 0 || c0 + e >= S.W) pmask |= 1 << (8 * seg + 4 * pp + e);
            }
          }
        }
        continue;
      }
      p_on[pp] = wave8 + NW * pp < P.NPV;
      const int pos = (wave8 + NW * pp) * 64 + lane;
      const int rr = w2d_div(pos, P.d_WCp), cc = pos - rr * P.WCp;
      if (rr < P.WR && cc < P.WC) {
        const int gh = h0 - 1 + rr, gw = w0 - 1 + cc;
        const int hs = gh - S.oh, ws = gw - S.ow;
        xo[pp] = ((unsigned)hs < (unsigned)S.H && (unsigned)ws < (unsigned)S.W) ? hs * S.ws + ws : W2D_PAD;
      }
    }
  };
  // unit pp of this wave, 16-byte pieces: its channel plane inside the chunk and its LDS offset inside a window image (scalars)
  const int nis = P.NI >> 1;
  int u_pl[NPP], u_lds[NPP];
#pragma unroll
  for (int pp = 0; pp < NPP; ++pp) {
    const int u = wave8 + NW * pp;
    u_pl[pp] = STRIPS ? u / 3 : u >> nis;
    u_lds[pp] = STRIPS ? (u / 3) * PS + 1 + (u % 3) * 256 : (u >> nis) * PS + 1 + (u & (P.NI - 1)) * 256;
  }
  int xo0[NPP], xo1[NPP];
  seg_offsets(0, xo0);
  seg_offsets(1, xo1);
  const int f_sw = P.src1.C > 0 ? P.src0.C / 4 : -1;           // first chunk of the second (concat) segment
  const int c_sw = f_sw >= 0 ? f_sw : 2147483647;              // chunks >= c_sw read the second segment
  const bool start1 = SPLIT && f_sw >= 0 && c_lo >= f_sw;      // this slab's chunks all lie in the second segment
  // U4: does any lane of the wave have outside floats to overwrite, per segment (wave-uniform: the chunks of nearly every wave skip
  // the repair without a vector instruction)
  // (lane counts in scalar registers, not bools: hipcc parks a wave-uniform bool that crosses the loop in a vector register)
  int pm_any0 = U4 ? __builtin_popcountll(__builtin_amdgcn_ballot_w64((pmask & 0xff) != 0)) : 0;
  int pm_any1 = U4 ? __builtin_popcountll(__builtin_amdgcn_ballot_w64((pmask >> 8) != 0)) : 0;
  asm volatile("" : "+s"(pm_any0), "+s"(pm_any1));
  {
    // padding positions of the block's first segment, once, in all 2 x 4 channel planes (own positions only); visible after the first barrier
    const float pad0 = (start1 ? P.src1.relu : P.src0.relu) ? __builtin_nanf("") : 0.f;
#pragma unroll
    for (int pp = 0; pp < NPP; ++pp)
      if (p_on[pp] && (start1 ? xo1[pp] : xo0[pp]) == W2D_PAD) {   // (p_on is wave-uniform)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          if constexpr (PC) {   // the unit's own plane
#pragma unroll
            for (int e = 0; e < 4; ++e) smem[b * BUF + WTILE + u_lds[pp] + lane * 4 + e] = pad0;
          } else {
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) smem[b * BUF + WTILE + ch * PS + (wave8 + NW * pp) * 64 + lane] = pad0;
          }
        }
      }
  }
  // Fill addresses: a wave-uniform 64-bit base in scalar registers plus an UNSIGNED 32-bit byte offset per lane (as
  // gsd_wgrad_w2d.hip).  The base lies 16 bytes IN FRONT of the channel plane: a U4 piece that straddles the left edge of a segment
  // with a column offset starts up to 3 floats in front of row 0, and a zero-extended negative offset is 4 GiB away.  Advancing
  // the plane is scalar arithmetic.  Which lanes move something is loop-invariant but for the one segment switch: an exec mask in
  // a scalar register pair (f_msk), not a vector compare per fill.
  long long d_csb = (start1 ? P.src1.cs : P.src0.cs) * 4;   // plane stride, bytes
  // channel plane of the next halo slot: the slab's first channel inside its segment
  const char* d_base = reinterpret_cast<const char*>((start1 ? P.src1.p + (long long)n * P.src1.ns : P.src0.p + (long long)n * P.src0.ns) +
                                                     (long long)(c_lo - (start1 ? f_sw : 0)) * 4 * (d_csb >> 2)) - 16;
  unsigned f_off[NPP];           // the current segment's lane offsets (W2D_OFF_PAD: a padding position)
  unsigned long long f_msk[NPP]; // ... and the lanes that move a piece / pixel
  // (an offset that moves something is >= 4: 0 stands for no position, W2D_OFF_PAD for a padding position)
  auto off_of = [&](const int xo) { return xo == W2D_PAD ? W2D_OFF_PAD : (xo > W2D_PAD ? (unsigned)(xo + 4) * 4u : 0u); };
  auto lane_state = [&](const unsigned (&o)[NPP]) __attribute__((always_inline)) {
#pragma unroll
    for (int pp = 0; pp < NPP; ++pp) {
      f_off[pp] = o[pp];
      f_msk[pp] = __builtin_amdgcn_ballot_w64(p_on[pp] && o[pp] + 1u > 1u);
      asm volatile("" : "+s"(f_msk[pp]));
    }
  };
  // the second segment's lane offsets wait in LDS for the switch (own values, read back by the thread that wrote them: no barrier)
  unsigned* const sSw = reinterpret_cast<unsigned*>(smem + 2 * BUF + 2 * Kpad + 4 * BM);   // (behind sAff [2][Kpad] and sBw [4][64])
  {
    unsigned o0[NPP], o1[NPP];
#pragma unroll
    for (int pp = 0; pp < NPP; ++pp) o0[pp] = off_of(xo0[pp]), o1[pp] = off_of(xo1[pp]);
    if constexpr (!X4) sSw[tid] = o1[0], sSw[NT + tid] = o1[1];
    if constexpr (U4) sSw[2 * NT + tid] = (unsigned)pmask;   // (read back by the few chunks that repair a piece)
    lane_state(start1 ? o1 : o0);
  }
  // the switch to the second segment happens once per block, between two chunks: new plane pointer and lane offsets, and that
  // segment's padding positions are written into each LDS image the first time it is filled from it
  auto begin_fill = [&](int chunk, int buf) {
    if constexpr (X4) return;   // (one source)
    if (f_sw < 0 || start1 || (chunk != f_sw && chunk != f_sw + 1)) return;
    if (chunk == f_sw) {
      d_base = reinterpret_cast<const char*>(P.src1.p + (long long)n * P.src1.ns) - 16;
      d_csb = P.src1.cs * 4;
      int t = tid;
      asm volatile("" : "+v"(t));   // (or hipcc forwards the stored values to this read: through the loop, in registers)
      unsigned o1[NPP] = {};
      o1[0] = sSw[t], o1[1] = sSw[NT + t];
      lane_state(o1);
    }
    const float pad1 = P.src1.relu ? __builtin_nanf("") : 0.f;
#pragma unroll
    for (int pp = 0; pp < 2; ++pp)
      if (p_on[pp] && f_off[pp] == W2D_OFF_PAD) {
        if constexpr (PC) {
#pragma unroll
          for (int e = 0; e < 4; ++e) smem[buf * BUF + WTILE + u_lds[pp] + lane * 4 + e] = pad1;
        } else {
#pragma unroll
          for (int ch = 0; ch < 4; ++ch) smem[buf * BUF + WTILE + ch * PS + (wave8 + NW * pp) * 64 + lane] = pad1;
        }
      }
  };
  // (the lane offset is made opaque INSIDE the predicated block: hipcc otherwise zero-extends it once, outside the loop, and adds
  //  64-bit vector registers per fill instead of taking the scalar-base form of the instruction)
  auto halo_slot = [&](int ch, float* Xb) {   // input channel ch of the chunk: the lanes that have a pixel move it
    const char* b = d_base;
    asm volatile("" : "+s"(b));
#pragma unroll
    for (int pp = 0; pp < 2; ++pp)
      if (__builtin_amdgcn_inverse_ballot_w64(f_msk[pp])) {
        asm volatile("" : "+v"(f_off[pp]));
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const float*>(b + f_off[pp]), Xb + ch * PS + (wave8 + NW * pp) * 64, 4, 0, 0);
      }
    d_base += d_csb;
  };
  // X4: unit pp of this wave (one instruction of one of the chunk's four planes); d_base stays at the chunk's first plane
  auto halo_unit = [&](int pp, float* Xb) {
    const char* b = d_base + u_pl[pp] * d_csb;
    asm volatile("" : "+s"(b));
    if (__builtin_amdgcn_inverse_ballot_w64(f_msk[pp])) {
      asm volatile("" : "+v"(f_off[pp]));
      __builtin_amdgcn_global_load_lds(reinterpret_cast<const float*>(b + f_off[pp]), Xb + u_lds[pp], 16, 0, 0);
    }
    if (pp == 1) d_base += 4 * d_csb;
  };
  constexpr int WPW = 24 / NW;   // 1-KiB weight pieces per wave and chunk (6)
  const char* const wsrc0 = reinterpret_cast<const char*>(P.wt + (size_t)mbb * P.nchunks * WTILE + wave8 * (WPW * 256));
  unsigned w_off = (unsigned)lane * 16u;
  // the wave's pieces of the 24 are adjacent: they share LDS bases (M0) and differ in the instruction's immediate offset, which
  // moves the global and the LDS address alike; the global base is scalar, the lane's 16 bytes a constant offset
  auto weight_fill = [&](int chunk, float* Wn) {
    const char* wb = wsrc0 + (size_t)chunk * (WTILE * 4);
    asm volatile("" : "+s"(wb));
    asm volatile("" : "+v"(w_off));
    const float* wg = reinterpret_cast<const float*>(wb + w_off);
    float* wl = Wn + wave8 * (WPW * 256);
    __builtin_amdgcn_global_load_lds(wg, wl, 16, 0, 0);
    __builtin_amdgcn_global_load_lds(wg, wl, 16, 1024, 0);
    __builtin_amdgcn_global_load_lds(wg, wl, 16, 2048, 0);
    if constexpr (WPW == 6) {
      __builtin_amdgcn_global_load_lds(wg, wl, 16, 3072, 0);
      const char* wb2 = wb + 4096;
      asm volatile("" : "+s"(wb2));
      const float* wg2 = reinterpret_cast<const float*>(wb2 + w_off);
      __builtin_amdgcn_global_load_lds(wg2, wl + 1024, 16, 0, 0);
      __builtin_amdgcn_global_load_lds(wg2, wl + 1024, 16, 1024, 0);
    }
  };

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
  float* sBw = sAff + 2 * Kpad;   // [4][64]: scale, shift, mean, invstd of the fused BatchNorm-backward epilogue
  if (P.bw_raw != nullptr) {
    for (int c = tid; c < BM; c += NT) {
      const int co = m0 + c < P.Cout ? m0 + c : 0;
      sBw[c] = P.bw_scale[co];
      sBw[BM + c] = P.bw_shift[co];
      sBw[2 * BM + c] = P.bw_mean[co];
      sBw[3 * BM + c] = P.bw_invstd[co];
    }
  }
  const float lo0 = P.src0.relu ? 0.f : -__builtin_inff(), lo1 = P.src1.relu ? 0.f : -__builtin_inff();

  // ---- the wave's three window rows: its frequency rows (2 fh, 2 fh + 1) of B2^T d are tA = A - B and tB = B + sg C, with
  //   fh = 0: A, B, C = window rows 0, 2, 1 and sg = +1   (t0 = d0 - d2, t1 = d1 + d2)
  //   fh = 1: A, B, C = window rows 2, 1, 3 and sg = -1   (t2 = d2 - d1, t3 = d1 - d3)
  // -- the same code for both halves, and 18 window values each (the pairing {t1, t2} / {t0, t3} would need 12 / 24).  A fused
  // multiply-add by +-1 rounds as the addition or subtraction it stands for: V is bit for bit what the channel-half split computed.
  // (the rows' offsets from the lane's window corner `baddr` are scalars, added per chunk with the image's offset: one address
  //  register held through the loop instead of three)
  const int rowA = (2 * fh) * P.WCp, rowB = (2 - fh) * P.WCp, rowC = (1 + 2 * fh) * P.WCp;   // (arithmetic in fh: they stay scalar)
  const f32x2v sg2 = {fh ? -1.f : 1.f, fh ? -1.f : 1.f};

  f32x4 acc[4][12];   // [m-tile][frequency 6 r + fc of the wave's rows r = 0, 1]; zeroed below, behind the first fills

  // A operands: MFMA group g = 0..11 of a chunk is frequency pair g / 2 of the wave (weight-image pair 6 fh + g / 2) for two m-tiles
  // of the pair's two frequencies -- one ds_read_b128 (16 lanes read 256 contiguous bytes), four MFMAs.  acc[0..1] are the m-tiles the
  // wave keeps (2 fh, 2 fh + 1: the even groups read that half of the image pair), acc[2..3] the two it hands to its partner.
  const int a_keep = (j * 12 + fh * 6) * 128 + l16 * 4 + fh * 64, a_give = 64 - 128 * fh;   // (a_give: scalar, from a_keep)
  begin_fill(c_lo, 0);
  weight_fill(c_lo, smem);
  if constexpr (PC) {
    halo_unit(0, smem + WTILE);
    if constexpr (STRIPS) halo_unit(2, smem + WTILE);
    halo_unit(1, smem + WTILE);
  } else {
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) halo_slot(ch, smem + WTILE);
  }

  // The accumulators start at zero without a vector instruction: 192 v_mov contend with the MFMAs of the CU's other block like
  // any vector work, LDS reads do not.  The wave writes 16 bytes of zeros where nothing else lands before the first chunk's
  // barrier -- the weight half of image 1, which the first chunk's group 0 starts to fill -- and reads them back 48 times (the
  // LDS instructions of a wave execute in order; every lane reads the same address: a broadcast; the barrier's release fence has
  // the reads complete before any wave goes on to fill the image).  A zero C operand in a peeled first chunk would need a third
  // copy of the loop body.
  {
    l_f32x4* zp = (l_f32x4*)(smem + BUF + wave8 * 4);   // (an LDS pointer by type: 32 bits, and no base to add per read)
#pragma unroll
    for (int e = 0; e < 4; ++e) {   // (four dword stores of one zero register: a 16-byte store wants four)
      asm volatile("" : "+v"(zp));
      ((l_float*)zp)[e] = 0.f;
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int f = 0; f < 12; ++f) {
        asm volatile("" : "+v"(zp));   // (an address hipcc cannot see through: 48 reads, not one read and 188 copies)
        acc[m][f] = *zp;
      }
  }

  // PLAIN: the lane's LDS byte addresses in both images -- window rows A, B, C, the A operands it keeps and those it gives -- wait
  // in ten registers (the plain forms have them to spare, the activated ones do not): the loop adds no address, every read is a
  // register plus an immediate
  const l_float* l_adr[2][5] = {};   // (LDS pointers by type: 32 bits each)
  if constexpr (PLAIN) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      l_adr[b][0] = (const l_float*)(smem + b * BUF + rowA + baddr);
      l_adr[b][1] = (const l_float*)(smem + b * BUF + rowB + baddr);
      l_adr[b][2] = (const l_float*)(smem + b * BUF + rowC + baddr);
      l_adr[b][3] = (const l_float*)(smem + b * BUF + a_keep);
      l_adr[b][4] = (const l_float*)(smem + b * BUF + a_give + a_keep);
#pragma unroll
      for (int k = 0; k < 5; ++k) asm volatile("" : "+v"(l_adr[b][k]));
    }
  }

  // the chunk loop, unrolled by two: the LDS image a chunk reads (`cur`) is a constant of each copy
  auto run_chunk = [&](const int chunk, auto cur_c) {
    constexpr int cur = decltype(cur_c)::value;
    if constexpr (U4) {
      __builtin_amdgcn_s_waitcnt(0x0F70);   // this wave's fills of the chunk have landed
      // the outside floats of the straddling pieces this lane moved (the lane state still is the one the chunk was filled with)
      const bool seg1 = chunk >= c_sw;
      if ((seg1 ? pm_any1 : pm_any0) != 0) {
        int t = tid;
        asm volatile("" : "+v"(t));
        const int pmk = (int)sSw[2 * NT + t];
        const int pm = seg1 ? pmk >> 8 : pmk & 0xff;
        const float padv = (seg1 ? P.src1.relu : P.src0.relu) ? __builtin_nanf("") : 0.f;
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
          float* pq = smem + cur * BUF + WTILE + u_lds[pp] + lane * 4;
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (pm >> (4 * pp + e) & 1) pq[e] = padv;
        }
      }
      __syncthreads();
    } else {
      gsd_dma_barrier();   // the chunk's fills have landed; everyone has left the other image
    }
    const int kc = chunk * 4 + j;
    float sc = 1.f, sh = 0.f, lo = 0.f;
    if constexpr (!PLAIN) {
      sc = sAff[kc], sh = sAff[Kpad + kc];
      lo = chunk < c_sw ? lo0 : lo1;   // (a chunk lies inside one segment and Cin is a multiple of 4: a scalar select)
    }
    // chunks behind this one, as a scalar the compiler cannot see through: a comparison it recognises (chunk + 1 < c_hi is the
    // loop's own) travels as a bool through a vector register (v_cndmask + v_readfirstlane per chunk)
    int more = c_hi - 1 - chunk;
    asm volatile("" : "+s"(more));
    const float *pA, *pB, *pC, *Wc, *Wg;   // the lane's three window rows and its two A-operand streams in image `cur`
    if constexpr (PLAIN) {
      pA = (const float*)l_adr[cur][0], pB = (const float*)l_adr[cur][1], pC = (const float*)l_adr[cur][2];
      Wc = (const float*)l_adr[cur][3], Wg = (const float*)l_adr[cur][4];
    } else {
      // the image's offset as an opaque scalar: the LDS bases of the two images are then one set of registers plus an addition each,
      // not two sets held through the loop (registers the activated forms do not have)
      int ioff = cur * BUF, ioA = cur * BUF + rowA, ioB = cur * BUF + rowB, ioC = cur * BUF + rowC, ioG = cur * BUF + a_give;
      __asm__ volatile("" : "+s"(ioff), "+s"(ioA), "+s"(ioB), "+s"(ioC), "+s"(ioG));
      pA = smem + ioA + baddr, pB = smem + ioB + baddr, pC = smem + ioC + baddr;
      Wc = smem + ioff + a_keep, Wg = smem + ioG + a_keep;
    }
    auto load_row = [&](const float* Wr, float (&r)[6]) {
      const f32x4 ra = *reinterpret_cast<const f32x4*>(Wr);
      const f32x2v rb = *reinterpret_cast<const f32x2v*>(Wr + 4);
      r[0] = ra[0], r[1] = ra[1], r[2] = ra[2], r[3] = ra[3], r[4] = rb[0], r[5] = rb[1];
    };
    float dA[6], dB[6], dC[6];
    load_row(pA, dA);
    load_row(pB, dB);
    load_row(pC, dC);
    f32x4 av[2];   // read one group (four MFMAs) ahead
    av[0] = *reinterpret_cast<const f32x4*>(Wc);
    auto affine = [&](float (&r)[6]) {
      if constexpr (!PLAIN) {
        const f32x2v sc2 = {sc, sc}, sh2 = {sh, sh};
#pragma unroll
        for (int c = 0; c < 6; c += 2) {   // (the fused multiply-add on pairs; there is no packed fp32 max)
          const f32x2v y = __builtin_elementwise_fma(f32x2v{r[c], r[c + 1]}, sc2, sh2);
          r[c] = fmaxf(y[0], lo);
          r[c + 1] = fmaxf(y[1], lo);
        }
      }
    };
    // V row = B4^T t of one frequency row, on pairs of floats (v_pk_add_f32 / v_pk_fma_f32: about half the vector instructions), in
    // three stages so that the second row's can be spread over the first row's MFMAs: pairs (t0,t1), (t2,t3), (t4,t5) of the
    // column-transformed row, then
    //   (a, c) = t4 + (-4,-1) t2      (b, e) = t3 + (-4,-1) t1      (v1, v2) = a + (1,-1) b      (v3, v4) = c + (2,-2) e
    //   (v0, v5) = 4 (t0,t1) + ((t4,t5) - 5 (t2,t3))
    // -- element for element the fused multiply-adds of the scalar transform (a multiplication by 1, 2 or -1 is exact)
    const f32x2v m41 = {-4.f, -1.f}, p1m1 = {1.f, -1.f}, p2m2 = {2.f, -2.f}, m5 = {-5.f, -5.f}, p4 = {4.f, 4.f};
    auto rt_a = [&](const f32x2v (&tp)[3], f32x2v& ac, f32x2v& be) {
      ac = __builtin_elementwise_fma(f32x2v{tp[1][0], tp[1][0]}, m41, f32x2v{tp[2][0], tp[2][0]});
      be = __builtin_elementwise_fma(f32x2v{tp[0][1], tp[0][1]}, m41, f32x2v{tp[1][1], tp[1][1]});
    };
    auto rt_b = [&](const f32x2v& ac, const f32x2v& be, float (&v)[6]) {
      const f32x2v v12 = __builtin_elementwise_fma(f32x2v{be[0], be[0]}, p1m1, f32x2v{ac[0], ac[0]});
      const f32x2v v34 = __builtin_elementwise_fma(f32x2v{be[1], be[1]}, p2m2, f32x2v{ac[1], ac[1]});
      v[1] = v12[0], v[2] = v12[1], v[3] = v34[0], v[4] = v34[1];
    };
    auto rt_c = [&](const f32x2v (&tp)[3], float (&v)[6]) {
      const f32x2v v05 = __builtin_elementwise_fma(tp[0], p4, __builtin_elementwise_fma(tp[1], m5, tp[2]));
      v[0] = v05[0], v[5] = v05[1];
    };
    // frequency row 2 fh: tA = A - B; tB = B + sg C as well where the sources are activated (the activated rows would otherwise
    // stay live into the MFMAs beside the affine's coefficients: more than the 256 registers hold)
    affine(dA);
    affine(dB);
    f32x2v tA[3], tB[3], acB, beB;
#pragma unroll
    for (int k = 0; k < 3; ++k) tA[k] = f32x2v{dA[2 * k], dA[2 * k + 1]} - f32x2v{dB[2 * k], dB[2 * k + 1]};
    auto col_b = [&]() {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        tB[k] = __builtin_elementwise_fma(f32x2v{dC[2 * k], dC[2 * k + 1]}, sg2, f32x2v{dB[2 * k], dB[2 * k + 1]});
    };
    if constexpr (!PLAIN) {
      affine(dC);
      col_b();
    }
    float v[2][6];
    {
      f32x2v ac, be;
      rt_a(tA, ac, be);
      rt_b(ac, be, v[0]);
      rt_c(tA, v[0]);
    }
    __builtin_amdgcn_sched_barrier(0);
    // the chunk's 48 MFMAs in 12 groups of four (one A read each, issued a group ahead).  What an MFMA stream pays for is the
    // number of MFMA-to-MFMA gaps that carry vector work, far more than the instructions in them, and the SIMD's two waves pay it
    // one after the other (profiles/r05_mfma_f32_issue_ubench.txt).  So everything the vector pipe and the DMA have to do under
    // the MFMAs sits in THREE gaps, behind the four MFMAs of groups 0, 1 and 2: the next chunk's weight fills, one halo unit, and
    // the other halo unit with the whole transform of row 2 fh + 1 (ten packed instructions; due before group 6).  The other nine
    // groups are MFMAs, LDS reads and scalar work.  (Both halo units in group 1's gap with the transform -- two gaps -- measured
    // 0.8 % slower over the 17 plain layer shapes at batch 32: profiles/w2d_gaps_layers_b32.txt.)
#pragma unroll
    for (int g = 0; g < 12; ++g) {
      const int r = g / 6, fe = (g >> 1) * 2 - 6 * r, mt = 2 * (g & 1);
      if (g + 1 < 12) av[(g + 1) & 1] = *reinterpret_cast<const f32x4*>(&((g + 1) & 1 ? Wg : Wc)[((g + 1) >> 1) * 128]);
      const f32x4& ap = av[g & 1];
      acc[mt][6 * r + fe] = mfma16(ap[0], v[r][fe], acc[mt][6 * r + fe]);
      acc[mt + 1][6 * r + fe] = mfma16(ap[1], v[r][fe], acc[mt + 1][6 * r + fe]);
      acc[mt][6 * r + fe + 1] = mfma16(ap[2], v[r][fe + 1], acc[mt][6 * r + fe + 1]);
      acc[mt + 1][6 * r + fe + 1] = mfma16(ap[3], v[r][fe + 1], acc[mt + 1][6 * r + fe + 1]);
      if (g < 3) {
        __builtin_amdgcn_sched_barrier(0);   // the group's MFMAs and its A read first, the gap's work behind them in one piece
        int more_g = more;   // (opaque per group: one scalar compare each instead of a lane mask carried from group to group)
        asm volatile("" : "+s"(more_g));
        if (more_g > 0) {
          float* Wn = smem + (cur ^ 1) * BUF;
          if (g == 0) {
            begin_fill(chunk + 1, cur ^ 1);
            weight_fill(chunk + 1, Wn);
          } else if constexpr (PC) {
            halo_unit(g - 1, Wn + WTILE);
            if constexpr (STRIPS) {   // the wave's third unit shares group 1's gap: the chunk keeps its three gaps
              if (g == 1) halo_unit(2, Wn + WTILE);
            }
          } else {
            halo_slot(2 * g - 2, Wn + WTILE);
            halo_slot(2 * g - 1, Wn + WTILE);
          }
        }
        // the second row's transform, whole: tB (plain sources), then the three stages
        if (g == 2) {
          if constexpr (PLAIN) col_b();
          rt_a(tB, acB, beB);
          rt_b(acB, beB, v[1]);
          rt_c(tB, v[1]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  for (int chunk = c_lo; chunk < c_hi; chunk += 2) {
    run_chunk(chunk, std::integral_constant<int, 0>{});
    if (chunk + 1 < c_hi) run_chunk(chunk + 1, std::integral_constant<int, 1>{});
  }

  // ---- the two frequency halves of a pixel group meet: each wave hands its accumulators of the partner's m-tiles (acc[2..3]) to the
  // partner (wave ph + NWP (1 - fh)) and takes the partner's of its own in their place, through the two chunk images (48 KiB a
  // round, two rounds).  Then acc[0..1] hold the wave's frequency rows 2 fh, 2 fh + 1 of its m-tiles 2 fh + m and acc[2..3] the other
  // two rows: the output transform below is the one of the channel-half split, bit for bit.
  {
    float* const xs = smem + (wave8 * 12) * 256 + lane * 4;
    const float* const xr = smem + ((ph + NWP * (1 - fh)) * 12) * 256 + lane * 4;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      __syncthreads();   // round 0: every wave has left the last chunk's image; round 1: the partner has read round 0
#pragma unroll
      for (int f = 0; f < 12; ++f) *reinterpret_cast<f32x4*>(xs + f * 256) = acc[2 + r][f];
      __syncthreads();
#pragma unroll
      for (int f = 0; f < 12; ++f) acc[2 + r][f] = *reinterpret_cast<const f32x4*>(xr + f * 256);
    }
  }

  // Y = A2^T M A4 of one tile: down the columns first (24 -> 12 values), then along the rows (12 -> 2 x 4 outputs), two channels at
  // once: accumulator registers (r0, r0 + 1) of a quad are an aligned pair, so the additions and fused multiply-adds run as
  // v_pk_add_f32 / v_pk_fma_f32.
  // (HI: a wave of the second frequency half, whose acc[m] hold rows 2, 3 and acc[2 + m] rows 0, 1 -- two copies of the TRANSFORM
  // behind a wave-uniform branch rather than a register shuffle; the stores and statistics behind it exist once per path)
  // (j and l16 again from the thread id: cheaper than two registers held through the loop)
  int tid_e = tid;
  asm volatile("" : "+v"(tid_e));
  const int j_e = (tid_e & 63) >> 4, l16_e = tid_e & 15, q_e = ph * 16 + l16_e;
  auto out_pair = [&](auto hi_c, const int p, float (&y)[2][2][4]) __attribute__((always_inline)) {
    constexpr bool HI = decltype(hi_c)::value;
    const int m = p >> 1, r0 = (p & 1) * 2;
    const int lo = HI ? 2 + m : m, hi = HI ? m : 2 + m;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      f32x2v R[6];
#pragma unroll
      for (int fc = 0; fc < 6; ++fc) {
        const f32x2v M0 = {acc[lo][fc][r0], acc[lo][fc][r0 + 1]}, M1 = {acc[lo][6 + fc][r0], acc[lo][6 + fc][r0 + 1]};
        const f32x2v M2 = {acc[hi][fc][r0], acc[hi][fc][r0 + 1]}, M3 = {acc[hi][6 + fc][r0], acc[hi][6 + fc][r0 + 1]};
        R[fc] = a == 0 ? M0 + M1 + M2 : M1 - M2 - M3;
      }
      const f32x2v p12 = R[1] + R[2], m12 = R[1] - R[2], p34 = R[3] + R[4], m34 = R[3] - R[4];
      const f32x2v c2 = {2.f, 2.f}, c4 = {4.f, 4.f}, c8 = {8.f, 8.f};
      const f32x2v y0 = R[0] + p12 + p34, y1 = __builtin_elementwise_fma(c2, m34, m12), y2 = __builtin_elementwise_fma(c4, p34, p12);
      const f32x2v y3 = __builtin_elementwise_fma(c8, m34, m12) + R[5];
#pragma unroll
      for (int e = 0; e < 2; ++e) y[e][a][0] = y0[e], y[e][a][1] = y1[e], y[e][a][2] = y2[e], y[e][a][3] = y3[e];
    }
  };
  auto get_pair = [&](const int p, float (&y)[2][2][4]) __attribute__((always_inline)) {
    if (fh == 0)
      out_pair(std::false_type{}, p, y);
    else
      out_pair(std::true_type{}, p, y);
  };

  if constexpr (SPLIT) {
    // the un-reduced outputs of this slab: 32 bytes per lane and channel, 512-byte runs per 16 lanes
    float* const sl = P.slabs + ((size_t)((size_t)pt * P.nslab + slab) * P.mblocks + mbb) * (size_t)(BM * 128 * NWP);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      float y[2][2][4];
      get_pair(p, y);
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        float* const o = sl + ((size_t)(fh * 32 + (p >> 1) * 16 + j_e * 4 + (p & 1) * 2 + e) * (16 * NWP) + q_e) * 8;
        *reinterpret_cast<f32x4*>(o) = f32x4{y[e][0][0], y[e][0][1], y[e][0][2], y[e][0][3]};
        *reinterpret_cast<f32x4*>(o + 4) = f32x4{y[e][1][0], y[e][1][1], y[e][1][2], y[e][1][3]};
      }
    }
  } else if constexpr (STRIPS) {
    // the lane's tile again, from the list (behind an opaque copy of the block's id: nothing of it waits through the loop)
    int pt_e = pt;
    asm volatile("" : "+s"(pt_e));
    W2DStrip st[W2D_STRIPS];
    w2d_group_strips(2 * pt_e + ph, P.N, SP.TY, SP.TX, st);
    const W2DTile t = w2d_tile_of(32 * pt_e + q_e, P.N, SP.TY, SP.TX, st);
    int vmask = 0;
    if (t.n >= 0) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
        if (2 * t.ty + a < P.H) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (4 * t.tx + i < P.W) vmask |= 1 << (4 * a + i);
        }
    }
    w2d_epilogue<true>(P, sBw, t.n < 0 ? 0 : t.n, 0, 0, t.ty, t.tx, vmask, m0, fh, ph, j_e, l16_e, pt_e, get_pair);
  } else {
    w2d_epilogue(P, sBw, n, h0, w0, geo & 255, geo >> 8 & 255, geo >> 16 & 255, m0, fh, ph, j_e, l16_e, pt, get_pair);
  }
}
