// gsd_api.hip -- what the library says about itself: the thread-local error message behind GSD_REQUIRE / GSD_LAUNCH_CHECK
// (gsd_common.h), the version string, and the MFMA lane-map self test.
#include "gsd_common.h"

#include <cstdarg>
#include <cstdio>

static thread_local char g_err[512] = "";
void gsd_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* gsd_last_error(void) { return g_err; }
extern "C" const char* gsd_version(void) { return "libgsd 0.1 (gfx950, fp32 MFMA 16x16x4)"; }

// ---------------------------------------------------------------------------------------------
// MFMA lane-map self test
// ---------------------------------------------------------------------------------------------
__global__ void selftest_mfma_kernel(const float* a, const float* b, float* out) {
  const int lane = threadIdx.x;
  const float av = a[(lane & 15) * 4 + (lane >> 4)];   // A[i][k], row-major 16x4
  const float bv = b[(lane >> 4) * 16 + (lane & 15)];  // B[k][j], row-major 4x16
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
  c = mfma16(av, bv, c);
#pragma unroll
  for (int r = 0; r < 4; ++r) out[((lane >> 4) * 4 + r) * 16 + (lane & 15)] = c[r];
}
extern "C" int gsd_selftest_mfma(const float* a, const float* b, float* out, void* stream) {
  GSD_REQUIRE(a && b && out, GSD_ERR_BAD_ARG, "gsd_selftest_mfma: null argument");
  hipLaunchKernelGGL(selftest_mfma_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a, b, out);
  GSD_LAUNCH_CHECK("gsd_selftest_mfma");
  return GSD_OK;
}
