// gsd_convT_wgrad.hip -- dW and db of ConvTranspose2d(k2,s2) as an implicit GEMM over pixels on v_mfma_f32_16x16x4_f32 (gfx950),
// and gsd_sum_planes (the per-channel sums behind every bias gradient).
//
//   dW[ci][co][kh][kw] = sum_{n,h,w} x[n,ci,h,w] * dy[n,co,2h+kh,2w+kw]      (unet.py:36 of the reference)
//
// GEMM view: D[m][col] = sum_pixels A[m][pixel] * B[pixel][col] with the pixel index on the MFMA k dimension (4 consecutive
// pixels per instruction).  A = space-to-depth rows (co,kh,kw) of dy, B = x with the deferred BatchNorm+ReLU recomputed on
// load.  Wave tile 64 x 64.  The reduction over pixels is split across blocks (split-K); every block writes a partial slab and
// convT_wgrad_reduce_kernel sums the slabs in a fixed order => bitwise reproducible.
#include "gsd_convT_host.h"
#include "gsd_wgrad_host.h"

// Register-staged form: flat 64-pixel stages, operand tiles through registers (A = space-to-depth dy rows (co,kh,kw),
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

// LDS-DMA form (default).  Same GEMM as convT_wgrad_kernel; both tiles go HBM/L2 -> LDS with
// global_load_lds_dword (one instruction = one 64-pixel row of the image; the space-to-depth gather of dy and the
// flat pixel -> (h, w) map live in the per-lane source address), one LDS image per block and two blocks per CU, so one
// block's DMA issue + flight is covered by the other's MFMAs.  The deferred BatchNorm+ReLU of x is applied after the
// ds_read (a lane owns four fixed input channels).  Measured against the register-staged kernel: see DESIGN.md.
// X4: both operands as aligned 16-byte pieces instead of dword gathers (BX and AX below name the two halves of the switch).
// BX, the activation operand: 64 consecutive pixels of a channel plane are 256 contiguous bytes (H * W % 4 == 0, 16-byte
// aligned strides): an instruction fills four channel rows, 8 instead of 32 instructions per wave and stage.  The rows are then contiguous in LDS (pitch 64), so piece q of row r is stored at slot q ^ (r & 15) (swizzle on the
// DMA's source piece and on the read) to keep the 16 rows of a read off one bank.
__device__ __attribute__((aligned(16))) const float gsd_zero16_wg[4] = {0.f, 0.f, 0.f, 0.f};
typedef float f32x2 __attribute__((ext_vector_type(2)));
// AX, the gradient operand: rows m = (co, kh, kw = 0 / 1) read the same stretch of dy row 2h + kh interleaved, so an LDS row holds a (co, kh) PAIR of m rows: 128 floats = 64 pixels x (kw 0, kw 1), a piece = two
// pixels; an instruction fills two such rows (four m rows): 8 instead of 32 instructions per wave and stage.  Slot q of row R
// holds source piece q ^ (R & 7) (eight rows a read touches -> eight bank groups).  A pixel pair that straddles the end of an
// image row (odd W only) gets its second pixel's two floats from a plain load issued beside the fills and written over the
// piece by the same lane once its fills have landed.
template <bool X4>
__global__ __launch_bounds__(256, 2) void convT_wgrad_dma_kernel(const WgradParams P) {
  constexpr bool BX = X4, AX = X4;
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
        const float* gsrc = (pix_ok && m < P.M) ? abase + (long long)(m >> 2) * P.dy.cs + ((m >> 1) & 1) * P.dy.W + (m & 1) : &gsd_zero16_wg[0];
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
        const float* gsrc = (pix_ok && c < P.a0.C) ? bbase + (long long)c * P.a0.cs : &gsd_zero16_wg[0];
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

// Sum the slabs in split order and write the reference layout: slab[split][m][ci] -> dW[ci][m]  (m = co*4+kh*2+kw).
// LANES split lanes per element (block = 64 elements x LANES): lane sl adds splits sl, sl + LANES, ..., then the lanes are added
// in order.
template <int LANES>
__global__ __launch_bounds__(LANES == 1 ? 256 : 64 * LANES) void convT_wgrad_reduce_kernel(const float* __restrict__ slabs,
                                                                                           float* __restrict__ dw, int splits, int M,
                                                                                           int Ncols) {
  constexpr int EL = LANES == 1 ? 256 : 64;
  const long long per = (long long)M * Ncols;
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
    if (sl == 0 && ok) dw[(size_t)(e % Ncols) * M + (size_t)(e / Ncols)] = s;
    if (LANES > 1) __syncthreads();
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

struct ConvTWgPlan {
  bool wide;  // M <= 64: 64 x 256 blocks of the register-staged kernel, else 128 x 128
  int mblocks, nblocks, tiles_flat, stages_total, splits;
  int64_t slab_elems;
};

ConvTWgPlan plan_convT_wgrad(int N, int H, int W, int M, int Ncols) {
  ConvTWgPlan p;
  p.wide = M <= 64;
  p.mblocks = ceil_div(M, p.wide ? 64 : 128);
  p.nblocks = ceil_div(Ncols, p.wide ? 256 : 128);
  p.tiles_flat = ceil_div(H * W, 64);   // flat 64-pixel stages
  p.stages_total = N * p.tiles_flat;
  // one round of 2 resident blocks per CU x 256 CUs (the conv3x3 forms' knob)
  p.splits = wgrad_pick_splits(gsd_env_int("GSD_WGRAD_BLOCKS", 512), p.mblocks * p.nblocks, p.stages_total);
  p.slab_elems = (int64_t)p.splits * M * Ncols;
  return p;
}

// 16 split lanes per element from 64 slabs on, 4 from 8 on
void launch_convT_wgrad_reduce(const float* slabs, float* dw, int splits, int M, int Ncols, hipStream_t st) {
  const int lanes = splits >= 64 ? 16 : splits >= 8 ? 4 : 1;
  const int64_t blocks = ceil_div64((int64_t)M * Ncols, lanes == 1 ? 256 : 64), cap = lanes == 1 ? 4096 : 8192;
  const dim3 grid((int)(blocks < cap ? blocks : cap)), block(lanes == 1 ? 256 : 64 * lanes);
  if (lanes == 16) hipLaunchKernelGGL(convT_wgrad_reduce_kernel<16>, grid, block, 0, st, slabs, dw, splits, M, Ncols);
  else if (lanes == 4) hipLaunchKernelGGL(convT_wgrad_reduce_kernel<4>, grid, block, 0, st, slabs, dw, splits, M, Ncols);
  else hipLaunchKernelGGL(convT_wgrad_reduce_kernel<1>, grid, block, 0, st, slabs, dw, splits, M, Ncols);
}

}  // namespace

extern "C" int64_t gsd_convT2x2_wgrad_workspace(int N, int H, int W, int Cin, int Cout) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
  return plan_convT_wgrad(N, H, W, Cout * 4, Cin).slab_elems + (int64_t)Cout * 64;
}

extern "C" int gsd_convT2x2_wgrad(const gsd_src* x, const gsd_src* dy, int Cin, int Cout, float* dw, float* dbias,
                                  float* workspace, int64_t workspace_elems, int N, int H, int W, void* stream) {
  const char* const what = "gsd_convT2x2_wgrad";
  GSD_REQUIRE(x && dy && dw && workspace, GSD_ERR_BAD_ARG, "%s: null argument", what);
  if (int e = convT_check_sizes(what, Cin, Cout, N, H, W)) return e;
  GSD_REQUIRE(x->ptr != nullptr && x->C == Cin && x->H == H && x->W == W && x->off_h == 0 && x->off_w == 0,
              GSD_ERR_BAD_ARG, "%s: x must be the full (Cin,H,W) tensor", what);
  GSD_REQUIRE((x->scale == nullptr) == (x->shift == nullptr), GSD_ERR_BAD_ARG, "%s: scale/shift must come together", what);
  if (int e = wgrad_check_plain(*dy, "gsd_convT2x2_wgrad dy")) return e;
  if (int e = gsd_require_rows_contiguous(*dy, "gsd_convT2x2_wgrad dy")) return e;
  if (int e = gsd_require_rows_contiguous(*x, "gsd_convT2x2_wgrad x")) return e;
  if (int e = convT_check_dy(what, "dy", *dy, Cout, H, W)) return e;
  const int M = Cout * 4;
  const ConvTWgPlan pl = plan_convT_wgrad(N, H, W, M, Cin);
  const int64_t need = pl.slab_elems + (int64_t)Cout * 64;
  GSD_REQUIRE(workspace_elems >= need, GSD_ERR_WORKSPACE, "%s: workspace %lld < %lld elements", what, (long long)workspace_elems,
              (long long)need);
  // (the plane sums of the bias gradient walk dy as one dense array; refused before anything is launched, so that dW is not
  // written by a call that fails)
  GSD_REQUIRE(dbias == nullptr || (dy->c_stride == (int64_t)4 * H * W && dy->n_stride == (int64_t)Cout * 4 * H * W), GSD_ERR_UNSUPPORTED,
              "gsd_convT2x2_wgrad: bias gradient needs a contiguous dy");
  WgradParams P{};   // (a1 and the conv3x3 stage geometry stay 0)
  wgrad_fill_common(P, x, 1, dy, Cin, M, workspace, N, H, W, pl.splits, pl.mblocks, pl.nblocks);
  P.Cact = Cin;
  P.tiles_flat = pl.tiles_flat;
  P.stages_total = pl.stages_total;
  const int grid = pl.splits * pl.mblocks * pl.nblocks;
  const size_t lds = (size_t)((pl.wide ? 64 + 256 : 128 + 128) * 66) * sizeof(float);
  // both operands as aligned 16-byte pieces when 64 consecutive pixels of an activation plane are 256 aligned bytes (the gradient
  // rows then move as 16-byte pieces of dy rows: 8-byte aligned pixel pairs, dy is 8-byte aligned with even strides)
  const bool aligned = (H * W) % 4 == 0 && ((uintptr_t)x->ptr & 15) == 0 && x->c_stride % 4 == 0 && x->n_stride % 4 == 0;
  const hipStream_t st = (hipStream_t)stream;
  // (wide: M = 4*Cout <= 64, never the case for this network; the register-staged kernel keeps it working)
  if (int e = pl.wide   ? gsd_launch<convT_wgrad_kernel<1, 4>>(what, dim3(grid), dim3(256), lds, st, P)
              : aligned ? gsd_launch<convT_wgrad_dma_kernel<true>>(what, dim3(grid), dim3(256), lds, st, P)
                        : gsd_launch<convT_wgrad_dma_kernel<false>>(what, dim3(grid), dim3(256), lds, st, P))
    return e;
  launch_convT_wgrad_reduce(workspace, dw, pl.splits, M, Cin, st);
  GSD_LAUNCH_CHECK("gsd_convT2x2_wgrad reduce");
  if (dbias != nullptr) {
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
