// gsd_bf16_bn.hip -- BatchNorm of the bf16 path: apply (+ReLU, + max-pool), the stand-alone max-pool, and the BatchNorm / ReLU /
// max-pool backward (pass 1: mask, route, reduce; pass 2: apply).
#include "gsd_bf16_pointwise.h"

namespace {

constexpr int MULTI_UNR = 4;   // pixels per thread of the multi-pixel forms

// ---- a = relu(y * scale + shift) ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bn_apply_kernel(NhwcD y, const float* __restrict__ scale, const float* __restrict__ shift,
                                                       NhwcD a, int relu, long long npix) {
  const int groups = y.C >> 3;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= npix * groups) return;
  const int gk = (int)(e % groups);
  const long long p = e / groups;
  float f[8];
  unpack8(ld16(y.p + p * y.pitch + gk * 8), f);
  const BnAct8 act(scale, shift, gk);
  act(f, relu);
  st16(a.p + p * a.pitch + gk * 8, pack8(f));
}

// The same, UNR pixels per thread (C / 8 divides 256: every network shape): a block's 256 threads are (256 / groups) pixel lanes x
// groups channel groups, a thread keeps its group's coefficients and walks UNR pixels with all their loads in flight before the
// first store -- four times the bytes in flight per thread, index arithmetic and coefficient loads paid once instead of per pixel.
template <int UNR>
__global__ __launch_bounds__(256) void bn_apply_multi_kernel(NhwcD y, const float* __restrict__ scale, const float* __restrict__ shift,
                                                             NhwcD a, int relu, long long npix) {
  const int groups = y.C >> 3, ppi = 256 / groups;
  const int pl = threadIdx.x / groups, gk = threadIdx.x - pl * groups;
  const long long p0 = (long long)blockIdx.x * (ppi * UNR) + pl;
  const BnAct8 act(scale, shift, gk);
  uint4 raw[UNR];
#pragma unroll
  for (int k = 0; k < UNR; ++k) {
    const long long p = p0 + (long long)k * ppi;
    raw[k] = p < npix ? ld16(y.p + p * y.pitch + gk * 8) : make_uint4(0, 0, 0, 0);
  }
#pragma unroll
  for (int k = 0; k < UNR; ++k) {
    const long long p = p0 + (long long)k * ppi;
    float f[8];
    unpack8(raw[k], f);
    act(f, relu);
    if (p < npix) st16(a.p + p * a.pitch + gk * 8, pack8(f));
  }
}

// first maximum of a 2x2 window's four values in (0,0),(0,1),(1,0),(1,1) order: its position 0..3
template <typename T>
__device__ __forceinline__ unsigned first_max4(T v0, T v1, T v2, T v3) {
  T best = v0;
  unsigned bi = 0;
  if (v1 > best) { best = v1; bi = 1; }
  if (v2 > best) { best = v2; bi = 2; }
  if (v3 > best) { best = v3; bi = 3; }
  return bi;
}

// ---- a = relu(y * scale + shift) AND pooled = MaxPool2d(2)(a) in one pass (unet.py:15-16 followed by :26) ---------------
// The encoder's second unit feeds a max-pool: the stand-alone pool re-reads the activation the apply pass has just written.
// Thread = one 2x2 window x 8 channels over the ceil(H/2) x ceil(W/2) window grid: it reads the window's four raw values,
// writes their four activations (into the concat buffer's skip slice) and, where the window is whole (floor mode drops an
// odd last row / column), their maximum.  Rounding to bf16 is monotonic, so max of the rounded activations == rounded max:
// bit-identical to gsd_bf16_bn_apply + gsd_bf16_maxpool2.
// idx (or null): one u16 per (window, 8-channel group), [N][H/2][W/2][C/8]: two bits per channel = which of the window's four
// activations the pool took -- the first maximum in (0,0),(0,1),(1,0),(1,1) order of the STORED bf16 values, what the backward
// (bn_bwd_reduce_pool_bf16_kernel) otherwise finds by re-reading the four activations (4 x 16 B per thread instead of 2 B).
__global__ __launch_bounds__(256) void bn_apply_pool_kernel(NhwcD y, const float* __restrict__ scale, const float* __restrict__ shift,
                                                            NhwcD a, NhwcD o, int wh, int ww, u16* __restrict__ idx) {
  const int groups = y.C >> 3;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)y.N * wh * ww * groups) return;
  const int gk = (int)(e % groups);
  const long long p = e / groups;
  const int wp = (int)(p % ww);
  const int hp = (int)((p / ww) % wh);
  const int n = (int)(p / ((long long)ww * wh));
  const BnAct8 act(scale, shift, gk);
  const bool col2 = 2 * wp + 1 < y.W, row2 = 2 * hp + 1 < y.H;
  const long long pix = ((long long)n * y.H + 2 * hp) * y.W + 2 * wp;
  uint4 raw[4];
  raw[0] = ld16(y.p + pix * y.pitch + gk * 8);
  raw[1] = col2 ? ld16(y.p + (pix + 1) * y.pitch + gk * 8) : raw[0];
  raw[2] = row2 ? ld16(y.p + (pix + y.W) * y.pitch + gk * 8) : raw[0];
  raw[3] = (row2 && col2) ? ld16(y.p + (pix + y.W + 1) * y.pitch + gk * 8) : raw[0];
  float m[8];
  uint4 pk[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float f[8];
    unpack8(raw[q], f);
    act(f, true);
#pragma unroll
    for (int i = 0; i < 8; ++i) m[i] = q == 0 ? f[i] : fmaxf(m[i], f[i]);
    const bool ok = (q == 0) || (q == 1 && col2) || (q == 2 && row2) || (q == 3 && row2 && col2);
    pk[q] = pack8(f);
    if (ok) st16(a.p + (pix + (q >> 1) * y.W + (q & 1)) * a.pitch + gk * 8, pk[q]);
  }
  if (row2 && col2) {
    st16(o.p + (((long long)n * o.H + hp) * o.W + wp) * o.pitch + gk * 8, pack8(m));
    if (idx != nullptr) {
      // activations are >= 0: their bf16 bit patterns order like the values, so the arg-max is taken on the 16-bit integers
      const unsigned w0[4] = {pk[0].x, pk[0].y, pk[0].z, pk[0].w}, w1[4] = {pk[1].x, pk[1].y, pk[1].z, pk[1].w};
      const unsigned w2[4] = {pk[2].x, pk[2].y, pk[2].z, pk[2].w}, w3[4] = {pk[3].x, pk[3].y, pk[3].z, pk[3].w};
      unsigned code = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int sh_ = (i & 1) * 16, wd = i >> 1;
        code |= first_max4((w0[wd] >> sh_) & 0xffffu, (w1[wd] >> sh_) & 0xffffu, (w2[wd] >> sh_) & 0xffffu, (w3[wd] >> sh_) & 0xffffu)
                << (2 * i);
      }
      idx[(((long long)n * o.H + hp) * o.W + wp) * groups + gk] = (u16)code;
    }
  }
}

// ---- MaxPool2d(2), floor mode (unet.py:26) --------------------------------------------------------------------------
__global__ __launch_bounds__(256) void maxpool2_bf16_kernel(NhwcD a, NhwcD o) {
  const int groups = a.C >> 3;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)o.N * o.H * o.W * groups) return;
  const int gk = (int)(e % groups);
  const long long p = e / groups;
  const int wp = (int)(p % o.W);
  const int hp = (int)((p / o.W) % o.H);
  const int n = (int)(p / ((long long)o.W * o.H));
  const u16* b = a.p + (((long long)n * a.H + 2 * hp) * a.W + 2 * wp) * a.pitch + gk * 8;
  float v0[8], v1[8], v2[8], v3[8];
  unpack8(ld16(b), v0);
  unpack8(ld16(b + a.pitch), v1);
  unpack8(ld16(b + (long long)a.W * a.pitch), v2);
  unpack8(ld16(b + (long long)(a.W + 1) * a.pitch), v3);
#pragma unroll
  for (int i = 0; i < 8; ++i) v0[i] = fmaxf(fmaxf(v0[i], v1[i]), fmaxf(v2[i], v3[i]));
  st16(o.p + p * o.pitch + gk * 8, pack8(v0));
}


// ---- BatchNorm + ReLU (+ max-pool / output conv) backward, pass 1 ---------------------------------------------------
struct BnBwdB {
  NhwcD y, g, a, dpool, dz;
  const u16* idx;   // pool mode: the forward's arg-max codes instead of `a` (or null)
  const float* scale; const float* shift; const float* mean; const float* invstd;
  const float* dout; const float* wout;
  float* partials;
  int pixb, chunks;
};

// dz of one pixel's 8 channels from its raw output yv and gradient gv (+ add: a pooled gradient routed here, or null): masked by the
// sign of the activation, stored at dst, and the sums of the values AS STORED (the apply pass reads these back) added to s1 / s2
__device__ __forceinline__ void bn_bwd_pixel8(const float (&yv)[8], const float (&gv)[8], const float* add, const float (&sc)[8],
                                              const float (&sh)[8], const float (&mu)[8], const float (&is)[8], u16* dst, float (&s1)[8],
                                              float (&s2)[8]) {
  float dzv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float gsum = add != nullptr ? gv[i] + add[i] : gv[i];
    dzv[i] = fmaf(yv[i], sc[i], sh[i]) > 0.f ? gsum : 0.f;
  }
  const uint4 packed = pack8(dzv);
  st16(dst, packed);
  float dq[8];
  unpack8(packed, dq);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    s1[i] += dq[i];
    s2[i] = fmaf(dq[i], (yv[i] - mu[i]) * is[i], s2[i]);
  }
}

// modes 0 (gradient g) and 2 (gradient wout * dout of the 1x1 output conv, third sum: dout * the activation as stored); the pooling
// mode has its own kernel below.
// grid (chunks, N); block: 256 threads = (256 / groups) pixels x groups 8-channel groups per pass (groups <= 256)
template <int MODE>
__global__ __launch_bounds__(256) void bn_bwd_reduce_bf16_kernel(const BnBwdB P) {
  extern __shared__ float red[];   // BLOCK_SUMS_LDS(3)
  const int C = P.y.C, groups = C >> 3;
  const int tpp = groups < 256 ? groups : 256;     // threads per pixel
  const int ppi = 256 / tpp;                       // pixels per pass
  const int chunk = blockIdx.x, n = blockIdx.y;
  const int HW = P.y.H * P.y.W;
  const int pl = threadIdx.x / tpp, gl = threadIdx.x - pl * tpp;
  float s[3][8];
  const int p_end = min((chunk + 1) * P.pixb, HW);
  for (int gk = gl; gk < groups; gk += tpp) {      // one trip unless C > 2048
    float sc[8], sh[8], mu[8], is[8], wo[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      sc[i] = P.scale[gk * 8 + i]; sh[i] = P.shift[gk * 8 + i]; mu[i] = P.mean[gk * 8 + i]; is[i] = P.invstd[gk * 8 + i];
      wo[i] = MODE == 2 ? P.wout[gk * 8 + i] : 0.f;
      s[0][i] = s[1][i] = s[2][i] = 0.f;
    }
    // the NEXT pixel's loads go out in front of this pixel's store: dz may alias g, so the compiler keeps loads behind older
    // stores -- without the prefetch a thread has one load in flight and every pixel is a dependent round trip
    const int p_first = chunk * P.pixb + pl;
    const bool any = p_first < p_end && pl < ppi;
    uint4 y_nx = make_uint4(0, 0, 0, 0), g_nx = make_uint4(0, 0, 0, 0);
    float d_nx = 0.f;
    if (any) {
      const long long pix0 = (long long)n * HW + p_first;
      y_nx = ld16(P.y.p + pix0 * P.y.pitch + gk * 8);
      if (MODE == 2) d_nx = P.dout[pix0];
      else g_nx = ld16(P.g.p + pix0 * P.g.pitch + gk * 8);
    }
    for (int p = p_first; p < p_end && pl < ppi; p += ppi) {
      const long long pix = (long long)n * HW + p;
      float yv[8], gv[8];
      const uint4 y_cur = y_nx, g_cur = g_nx;
      const float d = d_nx;
      if (p + ppi < p_end) {
        const long long pixn = pix + ppi;
        y_nx = ld16(P.y.p + pixn * P.y.pitch + gk * 8);
        if (MODE == 2) d_nx = P.dout[pixn];
        else g_nx = ld16(P.g.p + pixn * P.g.pitch + gk * 8);
      }
      unpack8(y_cur, yv);
      if (MODE == 2) {
#pragma unroll
        for (int i = 0; i < 8; ++i) gv[i] = d * wo[i];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float av = bf16_to_f32(f32_to_bf16(fmaxf(fmaf(yv[i], sc[i], sh[i]), 0.f)));   // the activation as stored
          s[2][i] = fmaf(d, av, s[2][i]);
        }
      } else {
        unpack8(g_cur, gv);
      }
      bn_bwd_pixel8(yv, gv, nullptr, sc, sh, mu, is, P.dz.p + pix * P.dz.pitch + gk * 8, s[0], s[1]);
    }
    // reduce over the ppi pixel lanes that share this channel group: block_sums_to_row<3>, spelled out -- through the function the
    // compiler lays this kernel's epilogue out differently (other branches, two of its stores merged)
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      red[threadIdx.x * 24 + i] = s[0][i];
      red[threadIdx.x * 24 + 8 + i] = s[1][i];
      red[threadIdx.x * 24 + 16 + i] = s[2][i];
    }
    __syncthreads();
    if (pl == 0) {
      float* row = P.partials + (size_t)(n * P.chunks + chunk) * 3 * C;
      for (int q = 0; q < 24; ++q) {
        float a = 0.f;
        for (int r = 0; r < ppi; ++r) a += red[(r * tpp + gl) * 24 + q];
        row[(q >> 3) * C + gk * 8 + (q & 7)] = a;
      }
    }
  }
}

// the pooled gradient dp of a window to position bi, zero to the other three
__device__ __forceinline__ void route4(unsigned bi, float dp, float& r0, float& r1, float& r2, float& r3) {
  r0 = bi == 0 ? dp : 0.f;
  r1 = bi == 1 ? dp : 0.f;
  r2 = bi == 2 ? dp : 0.f;
  r3 = bi == 3 ? dp : 0.f;
}

// Pool mode, one 2x2 window per (thread, 8-channel group): the four activations of a window are read ONCE (the per-pixel
// form above reads each window four times), the arg-max is taken once, and the four dz are written from the same
// thread.  With odd H / W the last row / column belongs to no window (floor pooling): the threads of the last window
// row / column also carry those pixels, which only see the direct gradient g.
// grid (chunks over the Hp*Wp windows, N); same partial-row layout and count as bn_bwd_reduce_bf16_kernel.
__global__ __launch_bounds__(256) void bn_bwd_reduce_pool_bf16_kernel(const BnBwdB P) {
  const int C = P.y.C, groups = C >> 3;
  const int tpp = groups < 256 ? groups : 256, ppi = 256 / tpp;
  const int chunk = blockIdx.x, n = blockIdx.y;
  const int H = P.y.H, W = P.y.W, Hp = P.dpool.H, Wp = P.dpool.W;
  const int pl = threadIdx.x / tpp, gl = threadIdx.x - pl * tpp;
  const int p_end = min((chunk + 1) * P.pixb, Hp * Wp);
  for (int gk = gl; gk < groups; gk += tpp) {
    float sc[8], sh[8], mu[8], is[8], s[2][8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      sc[i] = P.scale[gk * 8 + i]; sh[i] = P.shift[gk * 8 + i]; mu[i] = P.mean[gk * 8 + i]; is[i] = P.invstd[gk * 8 + i];
      s[0][i] = s[1][i] = 0.f;
    }
    // the pixel at `pix` from its raw output and skip gradient (already loaded); add: pooled gradient routed here, or null
    auto pixel_from = [&](const uint4 yraw, const uint4 graw, long long pix, const float* add) {
      float yv[8], gv[8];
      unpack8(yraw, yv);
      unpack8(graw, gv);
      bn_bwd_pixel8(yv, gv, add, sc, sh, mu, is, P.dz.p + pix * P.dz.pitch + gk * 8, s[0], s[1]);
    };
    auto one_pixel = [&](int h, int w) {   // a pixel of no window: the direct gradient only
      const long long pix = ((long long)n * H + h) * W + w;
      pixel_from(ld16(P.y.p + pix * P.y.pitch + gk * 8), ld16(P.g.p + pix * P.g.pitch + gk * 8), pix, nullptr);
    };
    for (int p = chunk * P.pixb + pl; p < p_end && pl < ppi; p += ppi) {
      const int hp = p / Wp, wp = p - hp * Wp;
      float dp[8], r0[8], r1[8], r2[8], r3[8];
      unpack8(ld16(P.dpool.p + (((long long)n * Hp + hp) * Wp + wp) * P.dpool.pitch + gk * 8), dp);
      if (P.idx != nullptr) {   // the forward (gsd_bf16_bn_apply_pool_idx) left the arg-max: 2 bytes instead of the window's 64
        const unsigned code = P.idx[(((long long)n * Hp + hp) * Wp + wp) * groups + gk];
#pragma unroll
        for (int i = 0; i < 8; ++i) route4((code >> (2 * i)) & 3u, dp[i], r0[i], r1[i], r2[i], r3[i]);
      } else {
        const u16* wb = P.a.p + (((long long)n * P.a.H + 2 * hp) * P.a.W + 2 * wp) * P.a.pitch + gk * 8;
        float a0[8], a1[8], a2[8], a3[8];
        unpack8(ld16(wb), a0);
        unpack8(ld16(wb + P.a.pitch), a1);
        unpack8(ld16(wb + (long long)P.a.W * P.a.pitch), a2);
        unpack8(ld16(wb + (long long)(P.a.W + 1) * P.a.pitch), a3);
#pragma unroll
        for (int i = 0; i < 8; ++i) route4(first_max4(a0[i], a1[i], a2[i], a3[i]), dp[i], r0[i], r1[i], r2[i], r3[i]);
      }
      {
        // the window's eight loads go out together, IN FRONT of its four stores: dz may alias g, so the compiler keeps every load
        // of pixel k + 1 behind the store of pixel k -- four dependent round trips per thread instead of one
        const long long p00 = ((long long)n * H + 2 * hp) * W + 2 * wp;
        const long long px[4] = {p00, p00 + 1, p00 + W, p00 + W + 1};
        uint4 yr[4], gr[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          yr[k] = ld16(P.y.p + px[k] * P.y.pitch + gk * 8);
          gr[k] = ld16(P.g.p + px[k] * P.g.pitch + gk * 8);
        }
        pixel_from(yr[0], gr[0], px[0], r0);
        pixel_from(yr[1], gr[1], px[1], r1);
        pixel_from(yr[2], gr[2], px[2], r2);
        pixel_from(yr[3], gr[3], px[3], r3);
      }
      const bool xcol = wp == Wp - 1 && (W & 1), xrow = hp == Hp - 1 && (H & 1);
      if (xcol) {
        one_pixel(2 * hp, W - 1);
        one_pixel(2 * hp + 1, W - 1);
      }
      if (xrow) {
        one_pixel(H - 1, 2 * wp);
        one_pixel(H - 1, 2 * wp + 1);
        if (xcol) one_pixel(H - 1, W - 1);
      }
    }
    block_sums_to_row<2>(s, tpp, ppi, pl, gl, P.partials, n * P.chunks + chunk, 3, C, gk);
    if (pl == 0) {
      float* row = P.partials + (size_t)(n * P.chunks + chunk) * 3 * C;
      for (int i = 0; i < 8; ++i) row[2 * C + gk * 8 + i] = 0.f;   // third column block: unused in pool mode
    }
  }
}

// ---- pass 2: d_raw = scale * (dz - c1 - xhat * c2), in place ---------------------------------------------------------------
__device__ __forceinline__ void bn_bwd_apply8(float d[8], const float yv[8], const float* sc, const float* mu, const float* is,
                                              const float* k1, const float* k2) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float xh = (yv[i] - mu[i]) * is[i];
    d[i] = sc[i] * (d[i] - k1[i] - xh * k2[i]);
  }
}

__global__ __launch_bounds__(256) void bn_bwd_apply_bf16_kernel(NhwcD dz, NhwcD y, const float* __restrict__ scale,
                                                                const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                const float* __restrict__ c1, const float* __restrict__ c2,
                                                                long long npix) {
  const int groups = y.C >> 3;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= npix * groups) return;
  const int gk = (int)(e % groups);
  const long long p = e / groups;
  float d[8], yv[8];
  unpack8(ld16(dz.p + p * dz.pitch + gk * 8), d);
  unpack8(ld16(y.p + p * y.pitch + gk * 8), yv);
  const int c = gk * 8;
  bn_bwd_apply8(d, yv, scale + c, mean + c, invstd + c, c1 + c, c2 + c);
  st16(dz.p + p * dz.pitch + gk * 8, pack8(d));
}

// UNR pixels per thread (C / 8 divides 256), as bn_apply_multi_kernel: the 40 coefficient floats of a channel group are loaded
// once per thread instead of once per pixel, and all of a thread's loads are in flight before its first (aliasing) store.
template <int UNR>
__global__ __launch_bounds__(256) void bn_bwd_apply_bf16_multi_kernel(NhwcD dz, NhwcD y, const float* __restrict__ scale,
                                                                      const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                      const float* __restrict__ c1, const float* __restrict__ c2,
                                                                      long long npix) {
  const int groups = y.C >> 3, ppi = 256 / groups;
  const int pl = threadIdx.x / groups, gk = threadIdx.x - pl * groups;
  const long long p0 = (long long)blockIdx.x * (ppi * UNR) + pl;
  float sc[8], mu[8], is[8], k1[8], k2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = gk * 8 + i;
    sc[i] = scale[c]; mu[i] = mean[c]; is[i] = invstd[c]; k1[i] = c1[c]; k2[i] = c2[c];
  }
  uint4 dr[UNR], yr[UNR];
#pragma unroll
  for (int k = 0; k < UNR; ++k) {
    const long long p = p0 + (long long)k * ppi;
    const bool ok = p < npix;
    dr[k] = ok ? ld16(dz.p + p * dz.pitch + gk * 8) : make_uint4(0, 0, 0, 0);
    yr[k] = ok ? ld16(y.p + p * y.pitch + gk * 8) : make_uint4(0, 0, 0, 0);
  }
#pragma unroll
  for (int k = 0; k < UNR; ++k) {
    const long long p = p0 + (long long)k * ppi;
    float d[8], yv[8];
    unpack8(dr[k], d);
    unpack8(yr[k], yv);
    bn_bwd_apply8(d, yv, sc, mu, is, k1, k2);
    if (p < npix) st16(dz.p + p * dz.pitch + gk * 8, pack8(d));
  }
}

// pixels per block of the multi-pixel form of the apply kernels (C / 8 divides 256 and there is work for >= 64 of its blocks), or 0:
// the one-pixel form
long long multi_ppb(const gsd_nhwc* y) {
  const int groups = y->C / 8;
  return groups <= 256 && 256 % groups == 0 && npix_of(y) * groups >= 256 * MULTI_UNR * 64 ? (256 / groups) * MULTI_UNR : 0;
}

int check_pooled(const gsd_nhwc* a, const gsd_nhwc* pooled, const char* fn) {
  GSD_REQUIRE(a->H > 1 && a->W > 1 && pooled->N == a->N && pooled->C == a->C && pooled->H == a->H / 2 && pooled->W == a->W / 2,
              GSD_ERR_BAD_ARG, "%s: pooled must be (N,H/2,W/2,C)", fn);
  return 0;
}

}  // namespace

extern "C" int gsd_bf16_bn_apply(const gsd_nhwc* y, const float* scale, const float* shift, const gsd_nhwc* a, int relu,
                                 void* stream) {
  if (int e = check_c8(y, "gsd_bf16_bn_apply y")) return e;
  if (int e = check_c8(a, "gsd_bf16_bn_apply a")) return e;
  GSD_REQUIRE(scale && shift && same_extent(y, a), GSD_ERR_BAD_ARG, "gsd_bf16_bn_apply: bad argument");
  const long long np = npix_of(y);
  if (const long long ppb = multi_ppb(y)) {
    hipLaunchKernelGGL(bn_apply_multi_kernel<MULTI_UNR>, dim3((unsigned)ceil_div64(np, ppb)), dim3(256), 0, (hipStream_t)stream, to_nhwc(*y),
                       scale, shift, to_nhwc(*a), relu, np);
  } else {
    hipLaunchKernelGGL(bn_apply_kernel, dim3((unsigned)ceil_div64(np * (y->C / 8), 256)), dim3(256), 0, (hipStream_t)stream, to_nhwc(*y),
                       scale, shift, to_nhwc(*a), relu, np);
  }
  GSD_LAUNCH_CHECK("gsd_bf16_bn_apply");
  return GSD_OK;
}

extern "C" int gsd_bf16_bn_apply_pool_idx(const gsd_nhwc* y, const float* scale, const float* shift, const gsd_nhwc* a,
                                          const gsd_nhwc* pooled, void* idx, void* stream) {
  if (int e = check_c8(y, "gsd_bf16_bn_apply_pool y")) return e;
  if (int e = check_c8(a, "gsd_bf16_bn_apply_pool a")) return e;
  if (int e = check_c8(pooled, "gsd_bf16_bn_apply_pool pooled")) return e;
  GSD_REQUIRE(scale && shift && same_extent(y, a), GSD_ERR_BAD_ARG, "gsd_bf16_bn_apply_pool: bad argument");
  if (int e = check_pooled(y, pooled, "gsd_bf16_bn_apply_pool")) return e;
  const int wh = (y->H + 1) / 2, ww = (y->W + 1) / 2;
  const long long total = (long long)y->N * wh * ww * (y->C / 8);
  hipLaunchKernelGGL(bn_apply_pool_kernel, dim3((unsigned)ceil_div64(total, 256)), dim3(256), 0, (hipStream_t)stream, to_nhwc(*y),
                     scale, shift, to_nhwc(*a), to_nhwc(*pooled), wh, ww, (u16*)idx);
  GSD_LAUNCH_CHECK("gsd_bf16_bn_apply_pool");
  return GSD_OK;
}

extern "C" int gsd_bf16_bn_apply_pool(const gsd_nhwc* y, const float* scale, const float* shift, const gsd_nhwc* a,
                                      const gsd_nhwc* pooled, void* stream) {
  return gsd_bf16_bn_apply_pool_idx(y, scale, shift, a, pooled, nullptr, stream);
}

extern "C" int gsd_bf16_maxpool2(const gsd_nhwc* a, const gsd_nhwc* pooled, void* stream) {
  if (int e = check_c8(a, "gsd_bf16_maxpool2 a")) return e;
  if (int e = check_c8(pooled, "gsd_bf16_maxpool2 pooled")) return e;
  if (int e = check_pooled(a, pooled, "gsd_bf16_maxpool2")) return e;
  const long long total = npix_of(pooled) * (a->C / 8);
  hipLaunchKernelGGL(maxpool2_bf16_kernel, dim3((unsigned)ceil_div64(total, 256)), dim3(256), 0, (hipStream_t)stream,
                     to_nhwc(*a), to_nhwc(*pooled));
  GSD_LAUNCH_CHECK("gsd_bf16_maxpool2");
  return GSD_OK;
}

extern "C" int gsd_bf16_bn_bwd_partial_rows(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return N * ceil_div(H * W, pick_pixb(N, H * W));
}

static int bn_bwd_reduce_impl(int mode, const gsd_nhwc* y, const float* scale, const float* shift, const float* mean,
                              const float* invstd, const gsd_nhwc* g, const gsd_nhwc* a, const void* pool_idx, const gsd_nhwc* dpool,
                              const float* dout, const float* wout, const gsd_nhwc* dz, float* partials, void* stream) {
  if (int e = check_c8(y, "gsd_bf16_bn_bwd_reduce y")) return e;
  if (int e = check_c8(dz, "gsd_bf16_bn_bwd_reduce dz")) return e;
  GSD_REQUIRE(mode >= 0 && mode <= 2 && scale && shift && mean && invstd && partials && same_extent(y, dz), GSD_ERR_BAD_ARG,
              "gsd_bf16_bn_bwd_reduce: bad argument");
  if (int e = check_reduce_grid(y, "gsd_bf16_bn_bwd_reduce")) return e;
  BnBwdB P;
  P.y = to_nhwc(*y);
  P.dz = to_nhwc(*dz);
  P.g = P.a = P.dpool = P.y;
  if (mode != 2) {
    if (int e = check_c8(g, "gsd_bf16_bn_bwd_reduce g")) return e;
    GSD_REQUIRE(same_extent(y, g), GSD_ERR_BAD_ARG, "gsd_bf16_bn_bwd_reduce: g extent differs from y");
    P.g = to_nhwc(*g);
  } else {
    GSD_REQUIRE(dout && wout, GSD_ERR_BAD_ARG, "gsd_bf16_bn_bwd_reduce: mode OUTC needs dout, wout (n_classes == 1)");
  }
  P.idx = nullptr;
  if (mode == 1) {
    if (int e = check_c8(dpool, "gsd_bf16_bn_bwd_reduce dpool")) return e;
    GSD_REQUIRE(dpool->N == y->N && dpool->C == y->C && dpool->H == y->H / 2 && dpool->W == y->W / 2, GSD_ERR_BAD_ARG,
                "gsd_bf16_bn_bwd_reduce: mode POOL needs dpool (N,H/2,W/2,C)");
    if (pool_idx != nullptr) {
      P.idx = (const u16*)pool_idx;
    } else {
      if (int e = check_c8(a, "gsd_bf16_bn_bwd_reduce a")) return e;
      GSD_REQUIRE(same_extent(y, a), GSD_ERR_BAD_ARG, "gsd_bf16_bn_bwd_reduce: mode POOL needs a (N,H,W,C)");
      P.a = to_nhwc(*a);
    }
    P.dpool = to_nhwc(*dpool);
  }
  P.scale = scale; P.shift = shift; P.mean = mean; P.invstd = invstd;
  P.dout = dout; P.wout = wout; P.partials = partials;
  P.pixb = pick_pixb(y->N, y->H * y->W);
  P.chunks = ceil_div(y->H * y->W, P.pixb);
  const dim3 grid(P.chunks, y->N);
  if (mode == 0) hipLaunchKernelGGL((bn_bwd_reduce_bf16_kernel<0>), grid, dim3(256), BLOCK_SUMS_LDS(3), (hipStream_t)stream, P);
  else if (mode == 1) {
    // one thread per 2x2 window; SAME number of partial rows as the per-pixel form (the chunks now split the windows)
    P.pixb = ceil_div(P.dpool.H * P.dpool.W, P.chunks);
    hipLaunchKernelGGL(bn_bwd_reduce_pool_bf16_kernel, grid, dim3(256), BLOCK_SUMS_LDS(2), (hipStream_t)stream, P);
  } else hipLaunchKernelGGL((bn_bwd_reduce_bf16_kernel<2>), grid, dim3(256), BLOCK_SUMS_LDS(3), (hipStream_t)stream, P);
  GSD_LAUNCH_CHECK("gsd_bf16_bn_bwd_reduce");
  return GSD_OK;
}

extern "C" int gsd_bf16_bn_bwd_reduce(int mode, const gsd_nhwc* y, const float* scale, const float* shift, const float* mean,
                                      const float* invstd, const gsd_nhwc* g, const gsd_nhwc* a, const gsd_nhwc* dpool,
                                      const float* dout, const float* wout, const gsd_nhwc* dz, float* partials, void* stream) {
  return bn_bwd_reduce_impl(mode, y, scale, shift, mean, invstd, g, a, nullptr, dpool, dout, wout, dz, partials, stream);
}

extern "C" int gsd_bf16_bn_bwd_reduce_pool_idx(const gsd_nhwc* y, const float* scale, const float* shift, const float* mean,
                                               const float* invstd, const gsd_nhwc* g, const void* pool_idx, const gsd_nhwc* dpool,
                                               const gsd_nhwc* dz, float* partials, void* stream) {
  GSD_REQUIRE(pool_idx != nullptr, GSD_ERR_BAD_ARG, "gsd_bf16_bn_bwd_reduce_pool_idx: null index");
  return bn_bwd_reduce_impl(1, y, scale, shift, mean, invstd, g, nullptr, pool_idx, dpool, nullptr, nullptr, dz, partials, stream);
}

extern "C" int gsd_bf16_bn_bwd_apply(const gsd_nhwc* dz, const gsd_nhwc* y, const float* scale, const float* mean,
                                     const float* invstd, const float* c1, const float* c2, void* stream) {
  if (int e = check_c8(dz, "gsd_bf16_bn_bwd_apply dz")) return e;
  if (int e = check_c8(y, "gsd_bf16_bn_bwd_apply y")) return e;
  GSD_REQUIRE(scale && mean && invstd && c1 && c2 && same_extent(dz, y), GSD_ERR_BAD_ARG, "gsd_bf16_bn_bwd_apply: bad argument");
  const long long np = npix_of(y);
  if (const long long ppb = multi_ppb(y)) {
    hipLaunchKernelGGL(bn_bwd_apply_bf16_multi_kernel<MULTI_UNR>, dim3((unsigned)ceil_div64(np, ppb)), dim3(256), 0, (hipStream_t)stream,
                       to_nhwc(*dz), to_nhwc(*y), scale, mean, invstd, c1, c2, np);
  } else {
    hipLaunchKernelGGL(bn_bwd_apply_bf16_kernel, dim3((unsigned)ceil_div64(np * (y->C / 8), 256)), dim3(256), 0, (hipStream_t)stream,
                       to_nhwc(*dz), to_nhwc(*y), scale, mean, invstd, c1, c2, np);
  }
  GSD_LAUNCH_CHECK("gsd_bf16_bn_bwd_apply");
  return GSD_OK;
}
