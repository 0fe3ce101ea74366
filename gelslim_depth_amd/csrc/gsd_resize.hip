// gsd_resize.hip -- F.interpolate(size=..., mode in {'nearest', 'nearest-exact', 'bilinear', 'bicubic'}, align_corners=False,
// antialias=False) for the reference's one resampling knob, interp_method (image_utils.py:12-15, read by
// general_dataset.py:71-121, test_depth_estimation.py:15,19, complete_prediction.py:5,9).  mode='area' stays with its
// own kernels (gsd_area_resize_affine at the head of this file, gsd_ingest_images in gsd_dataset.hip); the two entry
// points below forward it there unchanged.
//
// Same fused forms as the area path, one pass, one thread per output pixel, coalesced along the output pixel index:
//   gsd_resize_affine         out = A[c'] * resize(pre(x)) + B[c']      inference pre/post step (contiguous NCHW fp32)
//   gsd_ingest_images_interp  out = resize(pre(x))                      dataset ingest (strided channel view, fp32 / uint8)
//   pre(x) = (x - base + pre_add) * pre_mul when base != NULL (the difference image, image_utils.py:6-10), else x.
// The affine is fused after the resize because the taps of every mode sum to 1.
//
// Indices and weights are those of ATen's CPU kernels (UpSample.h + UpSampleKernel.cpp of torch 2.10), op for op in fp32,
// including the places where the CPU build contracts a multiply-add into an FMA.  Those contractions move the bilinear /
// bicubic weights by up to ~1e-5 (the source coordinate is an FMA: its rounding at ~400 is 3e-5), so these modes turn
// contraction off and write every FMA the CPU build forms explicitly:
//   scale     s = (float)in / (float)out
//   nearest   min(floor((float)d * s), in-1)
//   n.-exact  min(floor((float)((d + 0.5) * (double)s)), in-1)
//   linear    src = max(fma(s, d + 0.5f, -0.5f), 0); i0 = min(floor(src), in-1); i1 = i0 + (i0 < in-1); l1 = clamp(src-i0, 0, 1);
//             l0 = 1 - l1 (an identity dimension takes i0 = i1 = d, l0 = 1, l1 = 0); a row is fma(v0, l0, v1 * l1)
//   cubic     src = fma(s, d + 0.5f, -0.5f) (unclamped); i0 = min(floor(src), in-1); t = clamp(src-i0, 0, 1); A = -0.75;
//             taps i0-1..i0+2 clamped to [0, in-1]; a row is fma(v3, w3, fma(v2, w2, fma(v0, w0, v1 * w1)))
// Rows are combined with the same expression over the row values: the separable order of ATen's generic kernel, which
// it runs for NCHW input once OH + OW > 128 (smaller outputs of bilinear go through its channels-last kernel, whose
// weights are products w_h * w_w: the same result within a few ulps).
#include "gsd_common.h"

// ---------------------------------------------------------------------------------------------
// inference pre/post-processing: F.interpolate(mode='area') == adaptive average pooling,
// fused with the difference image ((a - base + 255) / 2, image_utils.py:6-10) and the per-channel affine of
// normalize_tactile_image / denormalize_depth_image (normalization_utils.py:4-35,101-129).
//   out[n,c,oh,ow] = A[c'] * mean_{window(oh,ow)} pre(in[n,c,h,w]) + B[c'],  c' = min(c, nab-1)
//   window rows [floor(oh*H/OH), ceil((oh+1)*H/OH)), same for columns (ATen adaptive_avg_pool2d)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void area_resize_affine_kernel(const float* __restrict__ in, const float* __restrict__ base,
                                                                 int C, int H, int W, float* __restrict__ out, int OH, int OW,
                                                                 const float* __restrict__ A, const float* __restrict__ B, int nab,
                                                                 float pre_add, float pre_mul) {
  const int c = blockIdx.y, n = blockIdx.z;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= OH * OW) return;
  const int oh = e / OW, ow = e - oh * OW;
  const int h0 = (int)(((long long)oh * H) / OH), h1 = (int)(((long long)(oh + 1) * H + OH - 1) / OH);
  const int w0 = (int)(((long long)ow * W) / OW), w1 = (int)(((long long)(ow + 1) * W + OW - 1) / OW);
  const size_t plane = ((size_t)n * C + c) * H * W;
  float s = 0.f;
  for (int h = h0; h < h1; ++h)
    for (int w = w0; w < w1; ++w) {
      float v = in[plane + (size_t)h * W + w];
      if (base != nullptr) v = (v - base[plane + (size_t)h * W + w] + pre_add) * pre_mul;
      s += v;
    }
  s /= (float)((h1 - h0) * (w1 - w0));
  const int cc = c < nab ? c : nab - 1;
  out[((size_t)n * C + c) * OH * OW + e] = fmaf(s, A[cc], B[cc]);
}
extern "C" int gsd_area_resize_affine(const float* in, const float* base, int N, int C, int H, int W, float* out, int OH, int OW,
                                      const float* A, const float* B, int nab, float pre_add, float pre_mul, void* stream) {
  GSD_REQUIRE(in && out && A && B && N > 0 && C > 0 && H > 0 && W > 0 && OH > 0 && OW > 0 && nab > 0, GSD_ERR_BAD_ARG,
              "gsd_area_resize_affine: bad argument");
  GSD_REQUIRE(N <= 65535 && C <= 65535, GSD_ERR_UNSUPPORTED, "gsd_area_resize_affine: N, C must be <= 65535");
  hipLaunchKernelGGL(area_resize_affine_kernel, dim3(ceil_div(OH * OW, 256), C, N), dim3(256), 0, (hipStream_t)stream, in, base,
                     C, H, W, out, OH, OW, A, B, nab, pre_add, pre_mul);
  GSD_LAUNCH_CHECK("gsd_area_resize_affine");
  return GSD_OK;
}

// Everything below restates ATen's arithmetic and writes its FMAs out (see the head of the file); the area form above keeps
// the compiler's default contraction.
#pragma clang fp contract(off)

namespace {

enum : int { M_NEAREST = GSD_INTERP_NEAREST, M_NEAREST_EXACT = GSD_INTERP_NEAREST_EXACT, M_BILINEAR = GSD_INTERP_BILINEAR,
             M_BICUBIC = GSD_INTERP_BICUBIC };

template <int MODE> struct Taps;

template <> struct Taps<M_NEAREST> {
  static constexpr int K = 1;
  int i[1];
  float w[1];
  __device__ __forceinline__ Taps(int d, int in, int out, float s) {
    const int j = (int)floorf((float)d * s);
    i[0] = j < in - 1 ? j : in - 1;
    w[0] = 1.f;
  }
};

template <> struct Taps<M_NEAREST_EXACT> {
  static constexpr int K = 1;
  int i[1];
  float w[1];
  __device__ __forceinline__ Taps(int d, int in, int out, float s) {
    const int j = (int)floorf((float)(((double)d + 0.5) * (double)s));
    i[0] = j < in - 1 ? j : in - 1;
    w[0] = 1.f;
  }
};

template <> struct Taps<M_BILINEAR> {
  static constexpr int K = 2;
  int i[2];
  float w[2];
  __device__ __forceinline__ Taps(int d, int in, int out, float s) {
    if (in == out) {
      i[0] = i[1] = d;
      w[0] = 1.f;
      w[1] = 0.f;
      return;
    }
    float src = __builtin_fmaf(s, (float)d + 0.5f, -0.5f);
    src = src < 0.f ? 0.f : src;
    int j = (int)floorf(src);
    j = j < in - 1 ? j : in - 1;
    const float l1 = fminf(fmaxf(src - (float)j, 0.f), 1.f);
    i[0] = j;
    i[1] = j + (j < in - 1 ? 1 : 0);
    w[0] = 1.f - l1;
    w[1] = l1;
  }
};

__device__ __forceinline__ float cubic1(float x) {      // ((A + 2) x - (A + 3)) x x + 1
  const float u = __builtin_fmaf(1.25f, x, -2.25f) * x;
  return u * x + 1.f;
}
__device__ __forceinline__ float cubic2(float x) {      // ((A x - 5A) x + 8A) x - 4A
  const float u = __builtin_fmaf(__builtin_fmaf(-0.75f, x, 3.75f), x, -6.f);
  return u * x + 3.f;
}

template <> struct Taps<M_BICUBIC> {
  static constexpr int K = 4;
  int i[4];
  float w[4];
  __device__ __forceinline__ Taps(int d, int in, int out, float s) {
    const float src = __builtin_fmaf(s, (float)d + 0.5f, -0.5f);
    int j = (int)floorf(src);
    j = j < in - 1 ? j : in - 1;
    const float t = fminf(fmaxf(src - (float)j, 0.f), 1.f);
    const float t2 = 1.f - t;
    w[0] = cubic2(t + 1.f);
    w[1] = cubic1(t);
    w[2] = cubic1(t2);
    w[3] = cubic2(t2 + 1.f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int q = j + k - 1;
      i[k] = q < 0 ? 0 : (q > in - 1 ? in - 1 : q);
    }
  }
};

// ATen's generic kernel: t0 * w0 + t1 * w1 [+ t2 * w2 + t3 * w3], contracted by the CPU build as written here
template <int K>
__device__ __forceinline__ float combine(const float* v, const float* w) {
  if constexpr (K == 1) {
    return v[0];
  } else {
    float o = __builtin_fmaf(v[0], w[0], v[1] * w[1]);
#pragma unroll
    for (int k = 2; k < K; ++k) o = __builtin_fmaf(v[k], w[k], o);
    return o;
  }
}

// grid (ceil(OH*OW/256), C, N).  in / base: plane (n, c) at n*ns + c*cs elements, rows of W.  out contiguous (N,C,OH,OW).
template <int MODE, typename T>
__global__ __launch_bounds__(256) void resize_kernel(const T* __restrict__ in, const T* __restrict__ base, int C, int H, int W,
                                                     long long in_ns, long long in_cs, long long base_ns, long long base_cs,
                                                     float* __restrict__ out, int OH, int OW, float sh, float sw,
                                                     const float* __restrict__ A, const float* __restrict__ B, int nab,
                                                     float pre_add, float pre_mul) {
  const int c = blockIdx.y, n = blockIdx.z;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= OH * OW) return;
  const int oh = e / OW, ow = e - oh * OW;
  const Taps<MODE> th(oh, H, OH, sh), tw(ow, W, OW, sw);
  constexpr int K = Taps<MODE>::K;
  const T* ip = in + (long long)n * in_ns + (long long)c * in_cs;
  const T* bp = base != nullptr ? base + (long long)n * base_ns + (long long)c * base_cs : nullptr;
  float rows[K];
#pragma unroll
  for (int a = 0; a < K; ++a) {
    const size_t r = (size_t)th.i[a] * W;
    float v[K];
#pragma unroll
    for (int b = 0; b < K; ++b) {
      float x = (float)ip[r + tw.i[b]];
      if (bp != nullptr) x = (x - (float)bp[r + tw.i[b]] + pre_add) * pre_mul;
      v[b] = x;
    }
    rows[a] = combine<K>(v, tw.w);
  }
  float y = combine<K>(rows, th.w);
  if (A != nullptr) {
    const int cc = c < nab ? c : nab - 1;
    y = __builtin_fmaf(y, A[cc], B[cc]);
  }
  out[((size_t)n * C + c) * OH * OW + e] = y;
}

template <int MODE, typename T>
void launch_mode(const T* in, const T* base, int N, int C, int H, int W, long long in_ns, long long in_cs, long long base_ns,
                 long long base_cs, float* out, int OH, int OW, const float* A, const float* B, int nab, float pre_add,
                 float pre_mul, hipStream_t stream) {
  const float sh = (float)H / (float)OH, sw = (float)W / (float)OW;
  hipLaunchKernelGGL((resize_kernel<MODE, T>), dim3(ceil_div(OH * OW, 256), C, N), dim3(256), 0, stream, in, base, C, H, W,
                     in_ns, in_cs, base_ns, base_cs, out, OH, OW, sh, sw, A, B, nab, pre_add, pre_mul);
}

template <typename T>
void launch(int mode, const T* in, const T* base, int N, int C, int H, int W, long long in_ns, long long in_cs,
            long long base_ns, long long base_cs, float* out, int OH, int OW, const float* A, const float* B, int nab,
            float pre_add, float pre_mul, hipStream_t stream) {
  auto* fn = mode == M_NEAREST         ? launch_mode<M_NEAREST, T>
             : mode == M_NEAREST_EXACT ? launch_mode<M_NEAREST_EXACT, T>
             : mode == M_BILINEAR      ? launch_mode<M_BILINEAR, T>
                                       : launch_mode<M_BICUBIC, T>;
  fn(in, base, N, C, H, W, in_ns, in_cs, base_ns, base_cs, out, OH, OW, A, B, nab, pre_add, pre_mul, stream);
}

bool sizes_fit(int H, int W, int OH, int OW) {
  return (int64_t)H * W <= 0x7fffffffLL && (int64_t)OH * OW <= 0x7fffffffLL - 255;
}

}  // namespace

extern "C" int gsd_resize_affine(int mode, const float* in, const float* base, int N, int C, int H, int W, float* out, int OH,
                                 int OW, const float* A, const float* B, int nab, float pre_add, float pre_mul, void* stream) {
  GSD_REQUIRE(mode >= GSD_INTERP_AREA && mode <= GSD_INTERP_BICUBIC, GSD_ERR_BAD_ARG,
              "gsd_resize_affine: unknown mode %d (GSD_INTERP_AREA .. GSD_INTERP_BICUBIC)", mode);
  if (mode == GSD_INTERP_AREA)
    return gsd_area_resize_affine(in, base, N, C, H, W, out, OH, OW, A, B, nab, pre_add, pre_mul, stream);
  GSD_REQUIRE(in && out && A && B && N > 0 && C > 0 && H > 0 && W > 0 && OH > 0 && OW > 0 && nab > 0, GSD_ERR_BAD_ARG,
              "gsd_resize_affine: bad argument");
  GSD_REQUIRE(N <= 65535 && C <= 65535, GSD_ERR_UNSUPPORTED, "gsd_resize_affine: N, C must be <= 65535");
  GSD_REQUIRE(sizes_fit(H, W, OH, OW), GSD_ERR_UNSUPPORTED, "gsd_resize_affine: a plane must hold < 2^31 pixels");
  const long long plane = (long long)H * W;
  launch<float>(mode, in, base, N, C, H, W, C * plane, plane, C * plane, plane, out, OH, OW, A, B, nab, pre_add, pre_mul,
                (hipStream_t)stream);
  GSD_LAUNCH_CHECK("gsd_resize_affine");
  return GSD_OK;
}

extern "C" int gsd_ingest_images_interp(int mode, const void* in, const void* base, int dtype, int N, int C, int H, int W,
                                        int64_t in_n_stride, int64_t in_c_stride, int64_t base_n_stride,
                                        int64_t base_c_stride, float* out, int OH, int OW, float pre_add, float pre_mul,
                                        void* stream) {
  GSD_REQUIRE(mode >= GSD_INTERP_AREA && mode <= GSD_INTERP_BICUBIC, GSD_ERR_BAD_ARG,
              "gsd_ingest_images_interp: unknown mode %d (GSD_INTERP_AREA .. GSD_INTERP_BICUBIC)", mode);
  if (mode == GSD_INTERP_AREA)
    return gsd_ingest_images(in, base, dtype, N, C, H, W, in_n_stride, in_c_stride, base_n_stride, base_c_stride, out, OH,
                             OW, pre_add, pre_mul, stream);
  GSD_REQUIRE(in && out && N > 0 && C > 0 && H > 0 && W > 0 && OH > 0 && OW > 0, GSD_ERR_BAD_ARG,
              "gsd_ingest_images_interp: bad argument");
  GSD_REQUIRE(dtype == 0 || dtype == 1, GSD_ERR_UNSUPPORTED, "gsd_ingest_images_interp: dtype must be 0 (f32) or 1 (u8)");
  GSD_REQUIRE(in_c_stride >= (int64_t)H * W && (base == nullptr || base_c_stride >= (int64_t)H * W), GSD_ERR_BAD_ARG,
              "gsd_ingest_images_interp: channel stride smaller than a plane");
  GSD_REQUIRE(N <= 65535 && C <= 65535, GSD_ERR_UNSUPPORTED, "gsd_ingest_images_interp: N, C must be <= 65535 per call");
  GSD_REQUIRE(sizes_fit(H, W, OH, OW), GSD_ERR_UNSUPPORTED, "gsd_ingest_images_interp: a plane must hold < 2^31 pixels");
  if (dtype == 0)
    launch<float>(mode, (const float*)in, (const float*)base, N, C, H, W, (long long)in_n_stride, (long long)in_c_stride,
                  (long long)base_n_stride, (long long)base_c_stride, out, OH, OW, nullptr, nullptr, 0, pre_add, pre_mul,
                  (hipStream_t)stream);
  else
    launch<unsigned char>(mode, (const unsigned char*)in, (const unsigned char*)base, N, C, H, W, (long long)in_n_stride,
                          (long long)in_c_stride, (long long)base_n_stride, (long long)base_c_stride, out, OH, OW, nullptr,
                          nullptr, 0, pre_add, pre_mul, (hipStream_t)stream);
  GSD_LAUNCH_CHECK("gsd_ingest_images_interp");
  return GSD_OK;
}
