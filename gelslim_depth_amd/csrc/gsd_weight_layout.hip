// gsd_weight_layout.hip -- fp32 weight re-layouts: conv / ConvT weights as the images that the conv kernels' LDS fills read
// (plain GEMM rows, Winograd F(4,3) rows, two-dimensional Winograd F(2x4,3x3)), one image per launch or a pass's 2-D images in one.
#include "gsd_common.h"

// modes 0/1 (conv3x3): tiled for the LDS-DMA kernel: [mblock][k row][BM], BM = 64 if M <= 64 else 128, so that
//   one K-chunk of one m-block is ONE contiguous LDS image (36 x BM floats).  Inside every group of 64 columns
//   (one wave's output channels) the order is permuted: storage slot l*4+m holds column m*16+l, so the four
//   MFMA A operands of a lane (its 4 m-tiles) are one aligned float4 in LDS.
// mode 2: retired (the register-staged ConvT forward kernel's image; the ConvT forward layout is mode 6).
// mode 3 (convT dgrad, register-staged kernel): plain [k row][Mpad].
// mode 6 (convT forward, LDS-DMA kernel): like modes 0/1 with BM = 128 and k rows padded to 32: [mblock][k row][128],
//   one K-chunk of 32 input channels of one m-block is one contiguous 16 KiB LDS image, columns permuted as above.
// mode 7 (convT dgrad, LDS-DMA kernel): the same image shape with k = co*4+kh*2+kw (8 output channels per chunk), m = ci.
static void layout_dims(int mode, int Co, int Ci, int* rows, int* M, int* BM, int* pitch, int* mblocks) {
  switch (mode) {
    case 0: *rows = round_up(Ci, 4) * 9; *M = Co; break;        // k = ci*9+t        m = co
    case 1: *rows = round_up(Co, 4) * 9; *M = Ci; break;        // k = co*9+t (flip) m = ci
    case 3: *rows = round_up(Co, 4) * 4; *M = Ci; break;        // k = co*4+khkw     m = ci
    case 4: *rows = round_up(Ci, 4) * 18; *M = Co; break;       // k = ci*18+r*6+f   m = co   (Winograd F(4,3) rows)
    case 5: *rows = round_up(Co, 4) * 18; *M = Ci; break;       // k = co*18+r*6+f (flip) m = ci
    case 7: *rows = round_up(Co, 8) * 4; *M = Ci; break;        // k = co*4+khkw     m = ci   (convT dgrad, LDS-DMA kernel)
    case 8: *rows = round_up(Ci, 4) * 24; *M = Co; break;       // k = ci*24+fr*6+fc m = co   (Winograd F(2x4,3x3), gsd_conv3x3_w2d)
    case 9: *rows = round_up(Co, 4) * 24; *M = Ci; break;       // k = co*24+fr*6+fc (flip) m = ci
    default: *rows = round_up(Ci, 32); *M = Co * 4; break;      // k = ci            m = co*4+khkw  (mode 6)
  }
  if (mode == 6 || mode == 7) {
    *BM = 128;
    *pitch = 128;
    *mblocks = ceil_div(*M, 128);
  } else if (mode >= 4) {
    *BM = 64;
    *pitch = 64;
    *mblocks = ceil_div(*M, 64);
  } else if (mode <= 1) {
    *BM = *M <= 64 ? 64 : 128;
    *pitch = *BM;
    *mblocks = ceil_div(*M, *BM);
  } else {
    *BM = round_up(*M, 64);
    *pitch = *BM;
    *mblocks = 1;
  }
}
extern "C" int64_t gsd_weight_layout_size(int mode, int Co, int Ci) {
  if (mode < 0 || mode > 9 || mode == 2 || Co <= 0 || Ci <= 0) return 0;
  int rows, M, BM, pitch, mblocks;
  layout_dims(mode, Co, Ci, &rows, &M, &BM, &pitch, &mblocks);
  return (int64_t)mblocks * rows * pitch;
}
__global__ void weight_layout_kernel(int mode, const float* __restrict__ w, int Co, int Ci, float* __restrict__ wt,
                                     int rows, int M, int BM, int pitch, int mblocks) {
  const long long total = (long long)mblocks * rows * pitch;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int col = (int)(e % pitch);
    const long long t = e / pitch;
    const int k = (int)(t % rows);
    const int mb = (int)(t / rows);
    int m = mb * BM + col;
    if (mode <= 1 || mode >= 4) {  // un-permute: slot (l*4 + t) of a 64-column group holds column t*16 + l
      const int slot = col & 63;
      m = mb * BM + (col & ~63) + (slot & 3) * 16 + (slot >> 2);
    }
    float v = 0.f;
    if (col < BM && m < M) {
      if (mode == 0) {
        const int ci = k / 9, tp = k % 9;
        if (ci < Ci) v = w[((size_t)m * Ci + ci) * 9 + tp];
      } else if (mode == 1) {
        const int co = k / 9, tp = k % 9;
        if (co < Co) v = w[((size_t)co * Ci + m) * 9 + (8 - tp)];
      } else if (mode == 6) {
        if (k < Ci) v = w[(size_t)k * M + m];  // (Ci, Co*4) is already [k][m]
      } else if (mode == 7) {
        if ((k >> 2) < Co) v = w[(size_t)m * (Co * 4) + k];   // W[ci][co][kh][kw] -> [k = co*4+kh*2+kw][m = ci]
      } else if (mode >= 4) {
        // U = G g for the 3 taps g of kernel row r (dX: the flipped kernel, channels swapped), G of F(4,3):
        // rows (1/4,0,0) (-1/6,-1/6,-1/6) (-1/6,1/6,-1/6) (1/24,1/12,1/6) (1/24,-1/12,1/6) (0,0,1)
        const int kch = k / 18, rem = k % 18, r = rem / 6, f = rem % 6;
        if (kch < (mode == 4 ? Ci : Co)) {
          const float* g = mode == 4 ? w + ((size_t)m * Ci + kch) * 9 + r * 3 : w + ((size_t)kch * Ci + m) * 9 + (2 - r) * 3;
          const float g0 = mode == 4 ? g[0] : g[2], g1 = g[1], g2 = mode == 4 ? g[2] : g[0];
          switch (f) {
            case 0: v = g0 * 0.25f; break;
            case 1: v = -(g0 + g1 + g2) * (1.f / 6.f); break;
            case 2: v = -(g0 - g1 + g2) * (1.f / 6.f); break;
            case 3: v = g0 * (1.f / 24.f) + g1 * (1.f / 12.f) + g2 * (1.f / 6.f); break;
            case 4: v = g0 * (1.f / 24.f) - g1 * (1.f / 12.f) + g2 * (1.f / 6.f); break;
            default: v = g2; break;
          }
        }
      } else {   // mode 3
        const int co = k >> 2;
        if (co < Co) v = w[(size_t)m * (Co * 4) + k];
      }
    }
    wt[e] = v;
  }
}
// Modes 4 / 5 (Winograd U = G g), one thread per (m-block, k channel, kernel row, column): the three taps are read once and
// the six transformed values written (the generic kernel reads them, and divides its way to them, once per OUTPUT element).
__global__ __launch_bounds__(256) void weight_layout_w43_kernel(int mode, const float* __restrict__ w, int Co, int Ci,
                                                                 float* __restrict__ wt, int kpad, int M, int mblocks) {
  const long long total = (long long)mblocks * kpad * 3 * 64;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int col = (int)(e & 63);
    long long t = e >> 6;
    const int r = (int)(t % 3);
    t /= 3;
    const int kch = (int)(t % kpad);
    const int mb = (int)(t / kpad);
    const int m = mb * 64 + (col & 3) * 16 + (col >> 2);   // slot l*4 + t of a 64-column group holds column t*16 + l
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    if (m < M && kch < (mode == 4 ? Ci : Co)) {
      const float* g = mode == 4 ? w + ((size_t)m * Ci + kch) * 9 + r * 3 : w + ((size_t)kch * Ci + m) * 9 + (2 - r) * 3;
      g0 = mode == 4 ? g[0] : g[2];
      g1 = g[1];
      g2 = mode == 4 ? g[2] : g[0];
    }
    float* o = wt + (((size_t)mb * kpad + kch) * 18 + r * 6) * 64 + col;
    o[0] = g0 * 0.25f;
    o[64] = -(g0 + g1 + g2) * (1.f / 6.f);
    o[128] = -(g0 - g1 + g2) * (1.f / 6.f);
    o[192] = g0 * (1.f / 24.f) + g1 * (1.f / 12.f) + g2 * (1.f / 6.f);
    o[256] = g0 * (1.f / 24.f) - g1 * (1.f / 12.f) + g2 * (1.f / 6.f);
    o[320] = g2;
  }
}
// Modes 8 / 9 (two-dimensional Winograd U = G2 g G4^T), one thread per (m-block, k channel, output channel of the block): the nine
// taps are read once and the 24 transformed values written.  G2 of F(2,3): rows (1,0,0) (1/2,1/2,1/2) (1/2,-1/2,1/2) (0,0,1); G4 of
// F(4,3) as above.  Image of one (m-block, 4-channel chunk): [ci & 3][frequency pair f >> 1 (12)][channel half (2)][l (16)][f & 1][m-tile
// of the half (2)] with channel = half*32 + m-tile*16 + l: a wave of gsd_conv3x3_w2d owns one channel half, and its 16 lanes l read
// the two frequencies x two m-tiles of a pair as 16 consecutive 16-byte pieces.
__global__ __launch_bounds__(256) void weight_layout_w2d_kernel(int mode, const float* __restrict__ w, int Co, int Ci,
                                                                 float* __restrict__ wt, int kpad, int M, int mblocks) {
  const long long total = (long long)mblocks * kpad * 64;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int cm = (int)(e & 63);           // channel inside the m-block
    const long long t = e >> 6;
    const int kch = (int)(t % kpad);
    const int mb = (int)(t / kpad);
    const int m = mb * 64 + cm;
    float g[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) g[r][c] = 0.f;
    if (m < M && kch < (mode == 8 ? Ci : Co)) {
      // forward: g = W[m][kch]; dX: the flipped kernel with the channels swapped, g[r][c] = W[kch][m][2-r][2-c]
      const float* src = mode == 8 ? w + ((size_t)m * Ci + kch) * 9 : w + ((size_t)kch * Ci + m) * 9;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) g[r][c] = mode == 8 ? src[r * 3 + c] : src[(2 - r) * 3 + (2 - c)];
    }
    const int half = cm >> 5, mtl = (cm >> 4) & 1, l = cm & 15;
    float* o = wt + ((size_t)mb * kpad + (kch & ~3)) * (24 * 64) + (size_t)(kch & 3) * (12 * 128) + half * 64 + l * 4 + mtl;
#pragma unroll
    for (int fr = 0; fr < 4; ++fr) {
      float gr[3];   // G2 down the kernel's rows
#pragma unroll
      for (int c = 0; c < 3; ++c)
        gr[c] = fr == 0 ? g[0][c] : fr == 3 ? g[2][c] : fr == 1 ? 0.5f * (g[0][c] + g[1][c] + g[2][c]) : 0.5f * (g[0][c] - g[1][c] + g[2][c]);
      const float g0 = gr[0], g1 = gr[1], g2 = gr[2];
      float u[6];
      u[0] = g0 * 0.25f;
      u[1] = -(g0 + g1 + g2) * (1.f / 6.f);
      u[2] = -(g0 - g1 + g2) * (1.f / 6.f);
      u[3] = g0 * (1.f / 24.f) + g1 * (1.f / 12.f) + g2 * (1.f / 6.f);
      u[4] = g0 * (1.f / 24.f) - g1 * (1.f / 12.f) + g2 * (1.f / 6.f);
      u[5] = g2;
#pragma unroll
      for (int fc = 0; fc < 6; ++fc) {
        const int f = fr * 6 + fc;
        o[(f >> 1) * 128 + (f & 1) * 2] = u[fc];
      }
    }
  }
}
extern "C" int gsd_weight_layout(int mode, const float* w, int Co, int Ci, float* wt, void* stream) {
  GSD_REQUIRE(w && wt && mode >= 0 && mode <= 9 && Co > 0 && Ci > 0, GSD_ERR_BAD_ARG, "gsd_weight_layout: bad argument");
  GSD_REQUIRE(mode != 2, GSD_ERR_BAD_ARG, "gsd_weight_layout: mode 2 is retired; the ConvT forward layout is mode 6");
  int rows, M, BM, pitch, mblocks;
  layout_dims(mode, Co, Ci, &rows, &M, &BM, &pitch, &mblocks);
  if (mode == 8 || mode == 9) {
    const int kpad = rows / 24;
    const long long threads = (long long)mblocks * kpad * 64;
    const int grid = gsd_grid_256(threads, 16384);
    hipLaunchKernelGGL(weight_layout_w2d_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, mode, w, Co, Ci, wt, kpad, M,
                       mblocks);
    GSD_LAUNCH_CHECK("gsd_weight_layout (w2d)");
    return GSD_OK;
  }
  if (mode == 4 || mode == 5) {
    const int kpad = rows / 18;
    const long long threads = (long long)mblocks * kpad * 3 * 64;
    const int grid = gsd_grid_256(threads, 16384);
    hipLaunchKernelGGL(weight_layout_w43_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, mode, w, Co, Ci, wt, kpad, M,
                       mblocks);
    GSD_LAUNCH_CHECK("gsd_weight_layout (w43)");
    return GSD_OK;
  }
  const long long total = (long long)mblocks * rows * pitch;
  const int grid = gsd_grid_256(total, 8192);
  hipLaunchKernelGGL(weight_layout_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, mode, w, Co, Ci, wt, rows, M, BM,
                     pitch, mblocks);
  GSD_LAUNCH_CHECK("gsd_weight_layout");
  return GSD_OK;
}

// All 2-D Winograd weight images of a pass in ONE launch (the fp32 twin of gsd_bf16_weight_images): the per-image launches of a
// step are 33 kernels of 5-20 us whose work is 0.7 GB of traffic.  Blocks are dealt to the jobs in proportion to their size.
namespace {
constexpr int WLB_MAX = 40;
struct WlBatch {
  const float* w[WLB_MAX];
  float* wt[WLB_MAX];
  int mode[WLB_MAX], Co[WLB_MAX], Ci[WLB_MAX], kpad[WLB_MAX], M[WLB_MAX], mblocks[WLB_MAX], first[WLB_MAX + 1];
  int n;
};
}  // namespace
__global__ __launch_bounds__(256) void weight_layout_w2d_batch_kernel(const WlBatch B) {
  int jb = 0;
  while (jb + 1 < B.n && (int)blockIdx.x >= B.first[jb + 1]) ++jb;
  const int mode = B.mode[jb], Co = B.Co[jb], Ci = B.Ci[jb], kpad = B.kpad[jb], M = B.M[jb];
  const float* __restrict__ w = B.w[jb];
  float* __restrict__ wt = B.wt[jb];
  const long long total = (long long)B.mblocks[jb] * kpad * 64;
  const int nb = B.first[jb + 1] - B.first[jb];
  for (long long e = (long long)(blockIdx.x - B.first[jb]) * blockDim.x + threadIdx.x; e < total; e += (long long)nb * blockDim.x) {
    const int cm = (int)(e & 63);
    const long long t = e >> 6;
    const int kch = (int)(t % kpad);
    const int mb = (int)(t / kpad);
    const int m = mb * 64 + cm;
    float g[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) g[r][c] = 0.f;
    if (m < M && kch < (mode == 8 ? Ci : Co)) {
      const float* src = mode == 8 ? w + ((size_t)m * Ci + kch) * 9 : w + ((size_t)kch * Ci + m) * 9;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) g[r][c] = mode == 8 ? src[r * 3 + c] : src[(2 - r) * 3 + (2 - c)];
    }
    const int half = cm >> 5, mtl = (cm >> 4) & 1, l = cm & 15;
    float* o = wt + ((size_t)mb * kpad + (kch & ~3)) * (24 * 64) + (size_t)(kch & 3) * (12 * 128) + half * 64 + l * 4 + mtl;
#pragma unroll
    for (int fr = 0; fr < 4; ++fr) {
      float gr[3];
#pragma unroll
      for (int c = 0; c < 3; ++c)
        gr[c] = fr == 0 ? g[0][c] : fr == 3 ? g[2][c] : fr == 1 ? 0.5f * (g[0][c] + g[1][c] + g[2][c]) : 0.5f * (g[0][c] - g[1][c] + g[2][c]);
      const float g0 = gr[0], g1 = gr[1], g2 = gr[2];
      float u[6];
      u[0] = g0 * 0.25f;
      u[1] = -(g0 + g1 + g2) * (1.f / 6.f);
      u[2] = -(g0 - g1 + g2) * (1.f / 6.f);
      u[3] = g0 * (1.f / 24.f) + g1 * (1.f / 12.f) + g2 * (1.f / 6.f);
      u[4] = g0 * (1.f / 24.f) - g1 * (1.f / 12.f) + g2 * (1.f / 6.f);
      u[5] = g2;
#pragma unroll
      for (int fc = 0; fc < 6; ++fc) {
        const int f = fr * 6 + fc;
        o[(f >> 1) * 128 + (f & 1) * 2] = u[fc];
      }
    }
  }
}
extern "C" int gsd_weight_layout_batch(const gsd_wl_job* jobs, int n, void* stream) {
  GSD_REQUIRE(jobs != nullptr && n > 0, GSD_ERR_BAD_ARG, "gsd_weight_layout_batch: bad argument");
  WlBatch B;
  B.n = 0;
  int blocks = 0;
  auto flush = [&]() -> int {
    if (B.n == 0) return GSD_OK;
    B.first[B.n] = blocks;
    hipLaunchKernelGGL(weight_layout_w2d_batch_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, B);
    GSD_LAUNCH_CHECK("gsd_weight_layout_batch");
    B.n = 0;
    blocks = 0;
    return GSD_OK;
  };
  for (int i = 0; i < n; ++i) {
    const gsd_wl_job& J = jobs[i];
    GSD_REQUIRE(J.w && J.wt && J.Co > 0 && J.Ci > 0 && J.mode >= 0 && J.mode <= 9, GSD_ERR_BAD_ARG, "gsd_weight_layout_batch: bad job %d", i);
    if (J.mode != 8 && J.mode != 9) {   // the other layouts keep their own launches
      if (int e = gsd_weight_layout(J.mode, J.w, J.Co, J.Ci, J.wt, stream)) return e;
      continue;
    }
    int rows, M, BM, pitch, mblocks;
    layout_dims(J.mode, J.Co, J.Ci, &rows, &M, &BM, &pitch, &mblocks);
    const int kpad = rows / 24;
    const long long threads = (long long)mblocks * kpad * 64;
    int nb = (int)(ceil_div64(threads, 1024) < 2048 ? ceil_div64(threads, 1024) : 2048);   // four elements per thread
    if (nb < 1) nb = 1;
    if (B.n == WLB_MAX) {
      if (int e = flush()) return e;
    }
    const int k = B.n++;
    B.w[k] = J.w; B.wt[k] = J.wt; B.mode[k] = J.mode; B.Co[k] = J.Co; B.Ci[k] = J.Ci; B.kpad[k] = kpad; B.M[k] = M; B.mblocks[k] = mblocks;
    B.first[k] = blocks;
    blocks += nb;
  }
  return flush();
}
