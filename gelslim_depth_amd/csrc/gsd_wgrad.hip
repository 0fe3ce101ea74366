// gsd_wgrad.hip -- dW of conv3x3: the entry points, the direct-tap form and the split-sum reducer of all three forms (gfx950).
//
//   dW[co][ci][tap] = sum_{n,h,w} dy[n,co,h,w] * a[n,ci,h+kh-1,w+kw-1]      (wgrad3x3_dma_kernel)
//   (the dW half of aten::convolution_backward for /root/reference/gelslim_depth/models/unet.py:11,14)
//
// gsd_conv3x3_wgrad picks one of three arithmetic forms per call -- direct taps (here), Winograd F(4,3) along rows
// (gsd_wgrad_w43.hip), two-dimensional Winograd F(2x4,3x3) (gsd_wgrad_w2d.hip); gsd_wgrad_host.h has what their host sides share.
// Every form splits the reduction over pixels across blocks (split-K); a block writes a partial slab [9 taps][Cout][Cin] and
// wgrad3x3_reduce_kernel sums the slabs in a fixed order => bitwise reproducible.
//
// Direct form, an implicit GEMM over pixels on v_mfma_f32_16x16x4_f32: D[m][col] = sum_pixels A[m][pixel] * B[pixel][col] with the
// pixel index on the MFMA k dimension (4 consecutive pixels of one row per instruction).  A = dy rows, B = activation with
// deferred BatchNorm+ReLU, zero padding and the two-segment channel concat recomputed on load, so the tensors the reference
// saves for backward (relu outputs, padded/concatenated inputs) are never stored.  Wave tile: 64 m-rows x (16 input channels x
// 9 taps).  It serves the layers with fewer than 16 channels on one side.
#include "gsd_wgrad_host.h"

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

// slab[split][r*3+s][co][ci] -> dW[co][ci][r][s] = sum over splits, in a fixed order, for all three forms (the Winograd blocks applied
// G^T themselves).
// Block = 64 elements x 16 split lanes: the layers with few (co, ci) pairs are the ones with hundreds of splits, and one
// thread per element would walk them serially (95 us per launch on average before, most of it latency).
template <int LANES>
__global__ __launch_bounds__(LANES == 1 ? 256 : 64 * LANES) void wgrad3x3_reduce_kernel(const float* __restrict__ slabs,
                                                                                        float* __restrict__ dw, int splits, int M,
                                                                                        int Ncols) {
  constexpr int EL = LANES == 1 ? 256 : 64;   // elements per block
  const long long plane = (long long)M * Ncols;
  const long long total = 3 * plane;
  const int el = threadIdx.x % EL, sl = threadIdx.x / EL;
  __shared__ float red[3][LANES][EL];
  for (long long e0 = (long long)blockIdx.x * EL; e0 < total; e0 += (long long)gridDim.x * EL) {
    const long long e = e0 + el;
    const bool ok = e < total;
    const int r = ok ? (int)(e / plane) : 0;
    const long long mc = ok ? e - r * plane : 0;
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      float s = 0.f;
      if (ok)
        for (int k = sl; k < splits; k += LANES) s += slabs[((size_t)k * 9 + r * 3 + f) * plane + mc];
      red[f][sl][el] = s;
    }
    __syncthreads();
    if (sl == 0 && ok) {
      float* o = dw + (size_t)mc * 9 + r * 3;
#pragma unroll
      for (int f = 0; f < 3; ++f) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < LANES; ++i) s += red[f][i][el];
        o[f] = s;
      }
    }
    __syncthreads();
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
  bool ksplit;  // <= 16 input channels and M <= 64: one 64 x 16 tile, waves split the pixels
  bool wide;  // WM=1,WN=4 (M<=64) else WM=2,WN=2
  int BMw, BNw, mblocks, nblocks, TH, TW, tiles_y, tiles_x, stages_total, splits;
  int64_t slab_elems;
};

WgradPlan plan_wgrad(int N, int H, int W, int M, int Ncols) {
  WgradPlan p;
  p.wide = M <= 64;
  p.ksplit = p.wide && Ncols <= 16;
  p.BMw = p.wide ? 64 : 128;
  p.BNw = p.ksplit ? 16 : (p.wide ? 4 : 2) * 16;
  p.mblocks = ceil_div(M, p.BMw);
  p.nblocks = ceil_div(Ncols, p.BNw);
  choose_wgrad_tile(H, W, &p.TH, &p.TW);
  p.tiles_y = ceil_div(H, p.TH);
  p.tiles_x = ceil_div(W, p.TW);
  p.stages_total = N * p.tiles_y * p.tiles_x;
  // tuning knob (512: one round of 2 resident blocks per CU x 256 CUs; 1024 measured 1 % slower end to end)
  p.splits = wgrad_pick_splits(gsd_env_int("GSD_WGRAD_BLOCKS", 512), p.mblocks * p.nblocks, p.stages_total);
  // 9 taps per slab, and the k-split form writes one slab per wave
  p.slab_elems = (int64_t)p.splits * (p.ksplit ? 36 : 9) * M * Ncols;
  return p;
}

// the direct form of gsd_conv3x3_wgrad: as the Winograd forms' _run (gsd_wgrad_host.h), returns the slab count
int wgrad_direct_run(const gsd_src* a, int nsrc, const gsd_src* dy, int Cin, int Cout, float* workspace, int N, int H, int W,
                     void* stream) {
  const WgradPlan pl = plan_wgrad(N, H, W, Cout, Cin);
  WgradParams P{};   // (tiles_flat: the ConvT kernels')
  wgrad_fill_common(P, a, nsrc, dy, Cin, Cout, workspace, N, H, W, pl.splits, pl.mblocks, pl.nblocks);
  P.Cact = Cin;
  P.TH = pl.TH; P.TW = pl.TW; P.tiles_y = pl.tiles_y; P.tiles_x = pl.tiles_x;
  P.WR = pl.TH + 2; P.WC = pl.TW + 2;
  P.PS = plane_stride_2mod32(P.WR * P.WC);
  P.stages_total = pl.stages_total;
  const dim3 grid(pl.splits * pl.mblocks * pl.nblocks);
  const size_t lds = (size_t)(pl.BMw * 66 + pl.BNw * P.PS) * sizeof(float);
  const char* const what = "gsd_conv3x3_wgrad";
  const hipStream_t st = (hipStream_t)stream;
  if (int e = pl.ksplit ? gsd_launch<wgrad3x3_dma_kernel<1, 4, true>>(what, grid, dim3(256), lds, st, P)
              : pl.wide ? gsd_launch<wgrad3x3_dma_kernel<1, 4, false>>(what, grid, dim3(256), lds, st, P)
                        : gsd_launch<wgrad3x3_dma_kernel<2, 2, false>>(what, grid, dim3(256), lds, st, P))
    return e;
  return pl.ksplit ? 4 * pl.splits : pl.splits;
}

// slab[nslabs][9][Cout][Cin] -> dW (Cout,Cin,3,3): 16 split lanes per element from 64 slabs on, 4 from 8 on; a thread sums the
// three taps of a kernel row
int wgrad_reduce_run(const float* slabs, float* dw, int nslabs, int Cout, int Cin, hipStream_t st) {
  const int lanes = nslabs >= 64 ? 16 : nslabs >= 8 ? 4 : 1;
  const int64_t blocks = ceil_div64(3LL * Cout * Cin, lanes == 1 ? 256 : 64);
  const dim3 grid((int)(blocks < 8192 ? blocks : 8192)), block(lanes == 1 ? 256 : 64 * lanes);
  if (lanes == 16) hipLaunchKernelGGL(wgrad3x3_reduce_kernel<16>, grid, block, 0, st, slabs, dw, nslabs, Cout, Cin);
  else if (lanes == 4) hipLaunchKernelGGL(wgrad3x3_reduce_kernel<4>, grid, block, 0, st, slabs, dw, nslabs, Cout, Cin);
  else hipLaunchKernelGGL(wgrad3x3_reduce_kernel<1>, grid, block, 0, st, slabs, dw, nslabs, Cout, Cin);
  GSD_LAUNCH_CHECK("gsd_conv3x3_wgrad reduce");
  return GSD_OK;
}

// The shape goes to a Winograd form (which of the two: gsd_wgrad_w2d_use).  GSD_WGRAD_ALGO=0|1 forces the direct form / a Winograd
// form (tuning, A/B runs); the 3-channel first layer keeps the pixel-split direct kernel.
bool wgrad_winograd(int Cin, int Cout) {
  const int forced = gsd_env_int("GSD_WGRAD_ALGO", -1);
  return forced == 0 ? false : forced == 1 ? true : Cin >= 16 && Cout >= 16;
}

}  // namespace

extern "C" int64_t gsd_conv3x3_wgrad_workspace(int N, int H, int W, int Cin, int Cout) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
  const int64_t direct = plan_wgrad(N, H, W, Cout, Cin).slab_elems, wino = gsd_wgrad_w43_workspace(N, H, W, Cin, Cout);
  const int64_t w2d = gsd_wgrad_w2d_workspace(N, H, W, Cin, Cout);
  const int64_t m = direct > wino ? direct : wino;   // any form may serve the call (GSD_WGRAD_ALGO, GSD_WGRAD_W2D, the operands)
  return m > w2d ? m : w2d;
}

extern "C" int gsd_conv3x3_wgrad_form(const gsd_src* a, int nsrc, const gsd_src* dy, int Cin, int Cout, int N, int H, int W) {
  if (!a || !dy || nsrc < 1 || nsrc > 2 || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
  return !wgrad_winograd(Cin, Cout) ? 0 : gsd_wgrad_w2d_use(a, nsrc, dy, Cin, Cout, N, H, W) ? 2 : 1;
}

// 1 when gsd_conv3x3_wgrad serves this shape with a kernel that takes PITCHED activation segments (w_stride > W): the Winograd forms
extern "C" int gsd_conv3x3_wgrad_takes_pitched_act(int N, int H, int W, int Cin, int Cout) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
  return wgrad_winograd(Cin, Cout) ? 1 : 0;
}

// 1 when it serves this shape with a kernel that takes a pitched dy (w_stride > W): the engine then lets gsd_bn_bwd_apply write
// d_raw into a pitched buffer.
extern "C" int gsd_conv3x3_wgrad_takes_pitched_dy(int N, int H, int W, int Cin, int Cout) {
  return gsd_conv3x3_wgrad_takes_pitched_act(N, H, W, Cin, Cout);
}

extern "C" int64_t gsd_conv3x3_wgrad_mfma_count(int form, int N, int H, int W, int Cin, int Cout) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
  if (form == 2) return gsd_wgrad_w2d_mfma_count(N, H, W, Cin, Cout);
  if (form == 1) return gsd_wgrad_w43_mfma_count(N, H, W, Cin, Cout);
  return 0;
}

extern "C" int gsd_conv3x3_wgrad(const gsd_src* a, int nsrc, const gsd_src* dy, int Cin, int Cout, float* dw,
                                 float* workspace, int64_t workspace_elems, int N, int H, int W, void* stream) {
  const bool wino = wgrad_winograd(Cin, Cout);   // the form is decided once per call (this half of it needs no valid operands)
  if (int e = wgrad_check_operands(a, nsrc, dy, Cin, Cout, dw, workspace, N, H, W, wino)) return e;
  const int64_t need = gsd_conv3x3_wgrad_workspace(N, H, W, Cin, Cout);
  GSD_REQUIRE(workspace_elems >= need, GSD_ERR_WORKSPACE, "gsd_conv3x3_wgrad: workspace %lld < %lld elements",
              (long long)workspace_elems, (long long)need);
  const int nslabs = !wino ? wgrad_direct_run(a, nsrc, dy, Cin, Cout, workspace, N, H, W, stream)
                     : gsd_wgrad_w2d_use(a, nsrc, dy, Cin, Cout, N, H, W) ? gsd_wgrad_w2d_run(a, nsrc, dy, Cin, Cout, workspace, N, H, W, stream)
                                                                          : gsd_wgrad_w43_run(a, nsrc, dy, Cin, Cout, workspace, N, H, W, stream);
  if (nslabs < 0) return nslabs;
  return wgrad_reduce_run(workspace, dw, nslabs, Cout, Cin, (hipStream_t)stream);
}
