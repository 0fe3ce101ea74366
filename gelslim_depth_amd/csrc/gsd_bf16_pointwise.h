// gsd_bf16_pointwise.h -- what the HBM-bound units of the bf16 path share (gsd_bf16_layout.hip, gsd_bf16_bn.hip, gsd_bf16_head.hip,
// gsd_bf16_sums.hip).  All tensors NHWC bf16 (gsd_nhwc), a thread owns 8 consecutive channels of a pixel (one 16-byte load/store:
// unpack8 / pack8 / ld16 / st16 of gsd_bf16_common.h), a wave therefore moves 1 KiB contiguous when pitch == C.  All arithmetic in fp32.
#pragma once
#include "gsd_bf16_common.h"

// ---- argument checks ----------------------------------------------------------------------------------------------------
static inline int check_c8(const gsd_nhwc* t, const char* what) {
  if (int e = gsd_check_nhwc(t, what)) return e;
  GSD_REQUIRE(t->C % 8 == 0, GSD_ERR_UNSUPPORTED, "%s: C=%d must be a multiple of 8", what, t->C);
  return 0;
}
static inline bool same_extent(const gsd_nhwc* a, const gsd_nhwc* b) { return a->N == b->N && a->H == b->H && a->W == b->W && a->C == b->C; }
static inline long long npix_of(const gsd_nhwc* t) { return (long long)t->N * t->H * t->W; }
// the block-reduce kernels: grid (chunks, N), and a block's threads walk the channel groups in steps of 256
static inline int check_reduce_grid(const gsd_nhwc* t, const char* fn) {
  GSD_REQUIRE(t->N <= 65535 && (t->C <= 2048 || t->C % 2048 == 0), GSD_ERR_UNSUPPORTED,
              "%s: N must be <= 65535 and C <= 2048 or a multiple of 2048", fn);
  return 0;
}

// pixels per block of the block-reduce kernels: target_blocks = 0 -> GSD_BF16_BN_BLOCKS (tuning) or the default
static inline int pick_pixb(int N, int HW, int target_blocks = 0) {
  if (target_blocks <= 0) target_blocks = gsd_env_int("GSD_BF16_BN_BLOCKS", 512);   // (2048 until round 4; 512 / 1024 / 2048 measured 25.9-26.1 / 26.15 / 26.3 ms per step)
  long long pixb = ((long long)N * HW + target_blocks - 1) / target_blocks;
  pixb = (pixb + 31) / 32 * 32;
  return (int)(pixb < 32 ? 32 : pixb);
}

// ---- a = relu(y * scale + shift) of a thread's 8 channels -------------------------------------------------------------------
// the coefficients of channel group gk (two 16-byte loads each), then any number of pixels
struct BnAct8 {
  f32x4 s0, s1, h0, h1;
  __device__ __forceinline__ BnAct8(const float* __restrict__ scale, const float* __restrict__ shift, int gk)
      : s0(*reinterpret_cast<const f32x4*>(scale + gk * 8)), s1(*reinterpret_cast<const f32x4*>(scale + gk * 8 + 4)),
        h0(*reinterpret_cast<const f32x4*>(shift + gk * 8)), h1(*reinterpret_cast<const f32x4*>(shift + gk * 8 + 4)) {}
  __device__ __forceinline__ void operator()(float f[8], bool relu) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[i] = fmaf(f[i], s0[i], h0[i]);
      f[4 + i] = fmaf(f[4 + i], s1[i], h1[i]);
    }
    if (relu) {
#pragma unroll
      for (int i = 0; i < 8; ++i) f[i] = fmaxf(f[i], 0.f);
    }
  }
};

// ---- block reduction of the block-reduce kernels -----------------------------------------------------------------------------
// A block's 256 threads are ppi = 256 / tpp pixel lanes x tpp channel groups (thread = pl * tpp + gl).  Each thread brings NS sums
// of its 8 channels; the threads of pixel lane 0 add the ppi lanes of their group, r = 0 .. ppi-1 in that order, and write column
// blocks 0 .. NS-1 (C floats each) of partial row `row_index` (rows of row_blocks * C floats) at channels gk*8 .. gk*8+7.  The launch
// gives BLOCK_SUMS_LDS(NS) bytes of dynamic LDS.
constexpr size_t BLOCK_SUMS_LDS(int ns) { return 256 * ns * 8 * sizeof(float); }
template <int NS>
__device__ __forceinline__ void block_sums_to_row(const float (&s)[NS][8], int tpp, int ppi, int pl, int gl, float* rows, int row_index,
                                                  int row_blocks, int C, int gk) {
  extern __shared__ float red[];   // [256][NS * 8]
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int k = 0; k < NS; ++k) red[threadIdx.x * (NS * 8) + k * 8 + i] = s[k][i];
  __syncthreads();
  if (pl == 0) {
    float* row = rows + (size_t)row_index * row_blocks * C;
    for (int q = 0; q < NS * 8; ++q) {
      float a = 0.f;
      for (int r = 0; r < ppi; ++r) a += red[(r * tpp + gl) * (NS * 8) + q];
      row[(q >> 3) * C + gk * 8 + (q & 7)] = a;
    }
  }
}
