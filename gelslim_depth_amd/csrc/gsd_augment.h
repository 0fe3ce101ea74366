// gsd_augment.h -- the augmentation stream of gsd_gather_augment (include/gsd.h), ONE definition compiled for the kernel and
// for the host queries gsd_augment_sample / gsd_augment_noise, so the two cannot drift apart.  Integer arithmetic and explicit
// fmaf only: every float below is either exact (a 24-bit integer times a power of two, 2u - 1 on such a value) or the result
// of ONE rounding, so nothing depends on what the compiler contracts.
#pragma once
#include <math.h>
#include <stdint.h>
#include "gsd.h"

#if defined(__HIPCC__)
#define GSD_AUG_HD __host__ __device__ __forceinline__
#else
#define GSD_AUG_HD static inline
#endif

#define GSD_AUG_GAMMA 0x9E3779B97F4A7C15ull
#define GSD_AUG_NOISE_TAG 0x6E6F697365ull          // "noise"
#define GSD_AUG_NOISE_SCALE 0x1.bb67aep-16f        // fp32(sqrt(3) / 65536)

GSD_AUG_HD uint64_t gsd_aug_fin(uint64_t z) {      // splitmix64's finaliser
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
GSD_AUG_HD uint64_t gsd_aug_mix(uint64_t z) { return gsd_aug_fin(z + GSD_AUG_GAMMA); }

// K: keyed by the dataset row, never by the position in the batch
GSD_AUG_HD uint64_t gsd_aug_key(uint64_t seed, int64_t epoch, int64_t index) {
  return gsd_aug_mix(gsd_aug_mix(gsd_aug_mix(seed) ^ (uint64_t)epoch) ^ (uint64_t)index);
}
GSD_AUG_HD uint64_t gsd_aug_draw(uint64_t key, int k) { return gsd_aug_fin(key + (uint64_t)(k + 1) * GSD_AUG_GAMMA); }

// the two 24-bit uniforms of a draw, in [0, 1): exact
GSD_AUG_HD float gsd_aug_u_hi(uint64_t r) { return (float)(uint32_t)(r >> 40) * 0x1p-24f; }
GSD_AUG_HD float gsd_aug_u_lo(uint64_t r) { return (float)(uint32_t)((r >> 16) & 0xFFFFFFu) * 0x1p-24f; }

struct gsd_aug_geom {
  int hflip, vflip, dy, dx;
};
struct gsd_aug_chan {
  float gain, offset;
};
GSD_AUG_HD gsd_aug_geom gsd_aug_geometry(const gsd_augment& a, uint64_t key) {
  const uint64_t r0 = gsd_aug_draw(key, 0), r1 = gsd_aug_draw(key, 1);
  gsd_aug_geom g;
  g.hflip = gsd_aug_u_hi(r0) < a.p_hflip ? 1 : 0;
  g.vflip = gsd_aug_u_lo(r0) < a.p_vflip ? 1 : 0;
  g.dy = -a.max_dy + (int)(((r1 >> 32) * (uint64_t)(2 * a.max_dy + 1)) >> 32);
  g.dx = -a.max_dx + (int)(((r1 & 0xFFFFFFFFull) * (uint64_t)(2 * a.max_dx + 1)) >> 32);
  return g;
}
GSD_AUG_HD gsd_aug_chan gsd_aug_channel(const gsd_augment& a, uint64_t key, int c) {
  const uint64_t r = gsd_aug_draw(key, 2 + c);
  gsd_aug_chan p;
  p.gain = fmaf(a.gain, fmaf(2.f, gsd_aug_u_hi(r), -1.f), 1.f);
  p.offset = a.offset * fmaf(2.f, gsd_aug_u_lo(r), -1.f);
  return p;
}
GSD_AUG_HD uint64_t gsd_aug_noise_key(uint64_t key) { return gsd_aug_mix(key ^ GSD_AUG_NOISE_TAG); }
// sum of four 16-bit uniforms, centred and scaled to unit variance; |n| <= 131070 * sqrt(3) / 65536 < 3.47
GSD_AUG_HD float gsd_aug_noise(uint64_t noise_key, uint64_t e) {
  const uint64_t r = gsd_aug_fin(noise_key + (e + 1) * GSD_AUG_GAMMA);
  const int s = (int)(r & 0xFFFF) + (int)((r >> 16) & 0xFFFF) + (int)((r >> 32) & 0xFFFF) + (int)(r >> 48);
  return (float)(s - 131070) * GSD_AUG_NOISE_SCALE;
}
