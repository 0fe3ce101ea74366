// gsd_bf16_sums.hip -- per-channel sums over a window of every image of a bf16 NHWC tensor, and the ConvTranspose2d bias gradient
// that is made of them.
#include "gsd_bf16_pointwise.h"

namespace {

// stage 1: grid (chunks, N), same thread layout as the BatchNorm reduction; stage 2: one thread per channel, fp64
__global__ __launch_bounds__(256) void channel_sums_stage1(NhwcD t, int y0, int x0, int hh, int ww, int pixb, int chunks,
                                                           float* __restrict__ ws) {
  const int C = t.C, groups = C >> 3;
  const int tpp = groups < 256 ? groups : 256, ppi = 256 / tpp;
  const int chunk = blockIdx.x, n = blockIdx.y;
  const int pl = threadIdx.x / tpp, gl = threadIdx.x - pl * tpp;
  const int p_end = min((chunk + 1) * pixb, hh * ww);
  for (int gk = gl; gk < groups; gk += tpp) {
    float s[1][8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[0][i] = 0.f;
    for (int p = chunk * pixb + pl; p < p_end && pl < ppi; p += ppi) {
      const int r = p / ww, c = p - r * ww;
      float f[8];
      unpack8(ld16(t.p + (((long long)n * t.H + y0 + r) * t.W + x0 + c) * t.pitch + gk * 8), f);
#pragma unroll
      for (int i = 0; i < 8; ++i) s[0][i] += f[i];
    }
    block_sums_to_row<1>(s, tpp, ppi, pl, gl, ws, n * chunks + chunk, 1, C, gk);
  }
}
// block = 64 channels x 4 row lanes (coalesced rows), fixed summation order
__global__ __launch_bounds__(256) void channel_sums_stage2(const float* __restrict__ ws, int rows, int C, float* __restrict__ out) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
  double s = 0.0;
  if (c < C)
    for (int r = rl; r < rows; r += 4) s += (double)ws[(size_t)r * C + c];
  __shared__ double red[4][64];
  red[rl][threadIdx.x & 63] = s;
  __syncthreads();
  if (rl == 0 && c < C) out[c] = (float)(red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// ConvTranspose2d bias gradient from what the decoder's dX launch left: out[c] = sum over the partial rows of column col0 + c
// (per-channel sums of the WHOLE gradient plane, from that launch's statistics epilogue) minus the workspace rows (stage-1 sums
// over the F.pad strips outside the transposed convolution's window).  Block = 64 channels x 16 row lanes, fp64, fixed order.
__global__ __launch_bounds__(1024) void convT_bias_combine_kernel(const float* __restrict__ part, int rows, int ld, int col0,
                                                                  const float* __restrict__ ws, int wrows, int C, float* __restrict__ out) {
  constexpr int RL = 16;   // row lanes: a few hundred rows, one block per 64 channels -- the walk is a chain of dependent loads
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
  double s = 0.0;
  if (c < C) {
    for (int r = rl; r < rows; r += RL) s += (double)part[(size_t)r * ld + col0 + c];
    for (int r = rl; r < wrows; r += RL) s -= (double)ws[(size_t)r * C + c];
  }
  __shared__ double red[RL][64];
  red[rl][threadIdx.x & 63] = s;
  __syncthreads();
  if (rl == 0 && c < C) {
    double t = 0.0;
    for (int i = 0; i < RL; ++i) t += red[i][threadIdx.x];
    out[c] = (float)t;
  }
}

// stage 1 over an hh x ww window of every image: 512 partial rows, so that stage 2 stays short
struct SumsGrid { int pixb, chunks; };
SumsGrid sums_grid(int N, int area) {
  const int pixb = pick_pixb(N, area, 512);
  return SumsGrid{pixb, ceil_div(area, pixb)};
}
int launch_stage1(const gsd_nhwc* t, int y0, int x0, int hh, int ww, float* ws, hipStream_t stream) {   // returns the rows written
  const SumsGrid g = sums_grid(t->N, hh * ww);
  hipLaunchKernelGGL(channel_sums_stage1, dim3(g.chunks, t->N), dim3(256), BLOCK_SUMS_LDS(1), stream, to_nhwc(*t), y0, x0, hh, ww, g.pixb,
                     g.chunks, ws);
  return t->N * g.chunks;
}

int check_window(const gsd_nhwc* t, bool args_ok, int y0, int x0, int hh, int ww, const char* fn) {
  GSD_REQUIRE(args_ok && y0 >= 0 && x0 >= 0 && hh > 0 && ww > 0 && y0 + hh <= t->H && x0 + ww <= t->W, GSD_ERR_BAD_ARG,
              "%s: window (%d,%d)+(%d,%d) outside (%d,%d)", fn, y0, x0, hh, ww, t->H, t->W);
  return 0;
}

// the (up to four) rectangles of an (H, W) plane outside the window [oy, oy+hh) x [ox, ox+ww): {y0, x0, rows, cols}
int pad_rects(int H, int W, int oy, int ox, int hh, int ww, int (&r)[4][4]) {
  int n = 0;
  auto add = [&](int y0, int x0, int rh, int rw) {
    if (rh > 0 && rw > 0) { r[n][0] = y0; r[n][1] = x0; r[n][2] = rh; r[n][3] = rw; ++n; }
  };
  add(0, 0, oy, W);
  add(oy + hh, 0, H - oy - hh, W);
  add(oy, 0, hh, ox);
  add(oy, ox + ww, hh, W - ox - ww);
  return n;
}

}  // namespace

extern "C" int64_t gsd_bf16_channel_sums_workspace(int N, int hh, int ww, int C) {
  if (N <= 0 || hh <= 0 || ww <= 0 || C <= 0) return 0;
  return (int64_t)N * sums_grid(N, hh * ww).chunks * C;
}

extern "C" int gsd_bf16_channel_sums(const gsd_nhwc* t, int y0, int x0, int hh, int ww, float* out, float* workspace,
                                     int64_t workspace_elems, void* stream) {
  if (int e = check_c8(t, "gsd_bf16_channel_sums t")) return e;
  if (int e = check_window(t, out && workspace, y0, x0, hh, ww, "gsd_bf16_channel_sums")) return e;
  if (int e = check_reduce_grid(t, "gsd_bf16_channel_sums")) return e;
  GSD_REQUIRE(workspace_elems >= gsd_bf16_channel_sums_workspace(t->N, hh, ww, t->C), GSD_ERR_WORKSPACE,
              "gsd_bf16_channel_sums: workspace too small");
  const int rows = launch_stage1(t, y0, x0, hh, ww, workspace, (hipStream_t)stream);
  GSD_LAUNCH_CHECK("gsd_bf16_channel_sums stage1");
  hipLaunchKernelGGL(channel_sums_stage2, dim3(ceil_div(t->C, 64)), dim3(256), 0, (hipStream_t)stream, workspace, rows, t->C, out);
  GSD_LAUNCH_CHECK("gsd_bf16_channel_sums stage2");
  return GSD_OK;
}

extern "C" int64_t gsd_bf16_convT_bias_grad_workspace(int N, int H, int W, int oy, int ox, int hh, int ww, int C) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || oy < 0 || ox < 0 || hh <= 0 || ww <= 0 || oy + hh > H || ox + ww > W) return 0;
  int r[4][4];
  const int n = pad_rects(H, W, oy, ox, hh, ww, r);
  int64_t tot = 0;
  for (int i = 0; i < n; ++i) tot += (int64_t)N * sums_grid(N, r[i][2] * r[i][3]).chunks * C;
  return tot > 0 ? tot : 1;
}

extern "C" int gsd_bf16_convT_bias_grad(const float* partials, int rows, int ld, int col0, const gsd_nhwc* g, int oy, int ox, int hh,
                                        int ww, float* out, float* workspace, int64_t workspace_elems, void* stream) {
  if (int e = check_c8(g, "gsd_bf16_convT_bias_grad g")) return e;
  GSD_REQUIRE(partials && out && workspace && rows > 0 && ld > 0 && col0 >= 0 && col0 + g->C <= ld, GSD_ERR_BAD_ARG,
              "gsd_bf16_convT_bias_grad: bad partial-row layout (rows %d, ld %d, col0 %d, C %d)", rows, ld, col0, g->C);
  if (int e = check_window(g, true, oy, ox, hh, ww, "gsd_bf16_convT_bias_grad")) return e;
  if (int e = check_reduce_grid(g, "gsd_bf16_convT_bias_grad")) return e;
  GSD_REQUIRE(workspace_elems >= gsd_bf16_convT_bias_grad_workspace(g->N, g->H, g->W, oy, ox, hh, ww, g->C), GSD_ERR_WORKSPACE,
              "gsd_bf16_convT_bias_grad: workspace too small");
  int r[4][4];
  const int n = pad_rects(g->H, g->W, oy, ox, hh, ww, r);
  int wrows = 0;
  for (int i = 0; i < n; ++i) {
    wrows += launch_stage1(g, r[i][0], r[i][1], r[i][2], r[i][3], workspace + (size_t)wrows * g->C, (hipStream_t)stream);
    GSD_LAUNCH_CHECK("gsd_bf16_convT_bias_grad strips");
  }
  hipLaunchKernelGGL(convT_bias_combine_kernel, dim3(ceil_div(g->C, 64)), dim3(1024), 0, (hipStream_t)stream, partials, rows, ld, col0,
                     workspace, wrows, g->C, out);
  GSD_LAUNCH_CHECK("gsd_bf16_convT_bias_grad");
  return GSD_OK;
}
