// gsd_conv3x3_host.h -- host-side code shared by the three conv3x3 forward / dX forms: direct taps (gsd_conv3x3.hip), Winograd
// F(4,3) along rows (gsd_conv3x3_w43.hip) and two-dimensional Winograd F(2x4,3x3) (gsd_conv3x3_w2d.hip).  Operand validation, the
// kernel-parameter fields the forms have in common, the LDS bank-conflict counter and the K-slab run-time model.
#pragma once
#include <stdio.h>
#include "gsd_common.h"

// Fused backward of relu(bn(raw)) on the destination (the *_dgrad_bnrelu entry points); all null: a plain convolution.
struct Conv3Bw {
  const float *raw = nullptr, *scale = nullptr, *shift = nullptr, *mean = nullptr, *invstd = nullptr;
};

// Operands of a conv3x3 launch of the entry point `name`.  src_pitched: the kernel addresses source rows through w_stride (else
// they must be row-contiguous); dst_plane_bound: destination planes are addressed with 32-bit offsets, as source planes always are.
static inline int conv3_check_operands(const char* name, bool src_pitched, bool dst_plane_bound, const gsd_src* src, int nsrc,
                                       const float* wt, int Cin, int Cout, const gsd_dst* dst, int ndst, int N, int H, int W) {
  GSD_REQUIRE(src && dst && wt, GSD_ERR_BAD_ARG, "%s: null argument", name);
  GSD_REQUIRE(nsrc >= 1 && nsrc <= 2 && ndst >= 1 && ndst <= 2, GSD_ERR_BAD_ARG, "%s: nsrc/ndst must be 1 or 2", name);
  GSD_REQUIRE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, GSD_ERR_BAD_ARG, "%s: bad sizes", name);
  GSD_REQUIRE(H < 32768 && W < 32768, GSD_ERR_UNSUPPORTED, "%s: H, W must be < 32768", name);
  GSD_REQUIRE(((uintptr_t)wt & 15) == 0, GSD_ERR_BAD_ARG, "%s: weight layout must be 16-byte aligned", name);
  char what[64];
  int csum = 0;
  snprintf(what, sizeof what, "%s src", name);
  for (int i = 0; i < nsrc; ++i) {
    if (int e = gsd_check_src(src[i], what, src_pitched)) return e;
    GSD_REQUIRE(src[i].scale == nullptr || src[i].relu != 0, GSD_ERR_UNSUPPORTED,
                "%s: an affine source segment must also have relu (zero padding uses a NaN sentinel)", name);
    // (w_stride == W where the rows must be contiguous)
    GSD_REQUIRE((int64_t)src[i].H * src[i].w_stride < (1LL << 31), GSD_ERR_UNSUPPORTED, "%s: plane too large", name);
    csum += src[i].C;
  }
  GSD_REQUIRE(csum == Cin, GSD_ERR_BAD_ARG, "%s: source segments hold %d channels, Cin=%d", name, csum, Cin);
  csum = 0;
  snprintf(what, sizeof what, "%s dst", name);
  for (int i = 0; i < ndst; ++i) {
    if (int e = gsd_check_dst(dst[i], what, true)) return e;   // every epilogue addresses rows through w_stride
    GSD_REQUIRE(!dst_plane_bound || (int64_t)dst[i].H * dst[i].w_stride < (1LL << 31), GSD_ERR_UNSUPPORTED, "%s: plane too large", name);
    csum += dst[i].C;
  }
  GSD_REQUIRE(csum == Cout, GSD_ERR_BAD_ARG, "%s: destination segments hold %d channels, Cout=%d", name, csum, Cout);
  return 0;
}

// The extra operands of the entry point `name` = gsd_conv3x3*_dgrad_bnrelu (the convolution's own are checked by the form's launcher).
static inline int conv3_check_dgrad_bnrelu(const char* name, const gsd_dst* dst, const Conv3Bw& bw, const float* partials, int Cout,
                                           int H, int W) {
  GSD_REQUIRE(dst && bw.raw && bw.scale && bw.shift && bw.mean && bw.invstd && partials, GSD_ERR_BAD_ARG, "%s: null argument", name);
  GSD_REQUIRE(dst->C == Cout && dst->H == H && dst->W == W && dst->off_h == 0 && dst->off_w == 0, GSD_ERR_BAD_ARG,
              "%s: dst must be the full (Cout,H,W) gradient buffer (raw shares its strides)", name);
  return 0;
}

// The kernel-parameter fields that Conv3Params, W43Params and W2DParams share by name (the structs are kernel arguments and stay
// separate: each form adds its own tile geometry).
template <class Params>
static inline void conv3_fill_common(Params& P, const gsd_src* src, int nsrc, const float* wt, int Cin, int Cout, const gsd_dst* dst,
                                     int ndst, float* partials, const Conv3Bw& bw, int N, int H, int W) {
  P.src0 = to_srcd(src[0]);
  P.src1 = nsrc > 1 ? to_srcd(src[1]) : null_srcd();
  P.dst0 = to_dstd(dst[0]);
  P.dst1 = ndst > 1 ? to_dstd(dst[1]) : null_dstd();
  P.wt = wt;
  P.partials = partials;
  P.bw_raw = bw.raw; P.bw_scale = bw.scale; P.bw_shift = bw.shift; P.bw_mean = bw.mean; P.bw_invstd = bw.invstd;
  P.Cin = Cin;
  P.Cout = Cout;
  P.Mpad = round_up(Cout, 64);
  P.nchunks = ceil_div(Cin, 4);
  P.N = N; P.H = H; P.W = W;
}

// LDS bank cost of the Winograd consumers' halo reads (one ds_read_b128 + one ds_read_b64 per window row) for a row pitch LP and a
// plane stride PS, both in floats: the sum over the block's `groups` groups of 16 tiles of the LDS cycles per read pair.  Lane ->
// tile as in the kernels: tile q = 16 group + (lane & 15) sits TWq to a tile row, tile rows are row_step window rows apart (1: the
// row form, 2: the two-dimensional form), channel plane lane >> 4; `off` shifts every address (the read offset of the 16-byte fills).
// (conv3_read_cycles: the same count for one wave whose lanes read at the given float addresses -- any lane -> tile map)
static inline int conv3_read_cycles(const int (&addr)[64]) {
  static const int g128[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                  {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
  int total = 0;
  {
    for (int half = 0; half < 2; ++half) {
      for (int g = 0; g < 2; ++g) {   // ds_read_b128: 16-lane groups, 16 slots of 16 B
        int worst = 0;
        for (int slot = 0; slot < 16; ++slot) {
          int distinct = 0, seen[16];
          for (int i = 0; i < 16; ++i) {
            const int a = addr[g128[g][i] + 32 * half];
            if ((a / 4) % 16 != slot) continue;
            bool dup = false;
            for (int k = 0; k < distinct; ++k) dup = dup || seen[k] == a;
            if (!dup) seen[distinct++] = a;
          }
          worst = distinct > worst ? distinct : worst;
        }
        total += worst;
      }
      int worst = 0;                  // ds_read_b64 at +4 floats: 32-lane halves, 32 slots of 8 B
      for (int slot = 0; slot < 32; ++slot) {
        int distinct = 0, seen[32];
        for (int i = 0; i < 32; ++i) {
          const int a = addr[i + 32 * half] + 4;
          if ((a / 2) % 32 != slot) continue;
          bool dup = false;
          for (int k = 0; k < distinct; ++k) dup = dup || seen[k] == a;
          if (!dup) seen[distinct++] = a;
        }
        worst = distinct > worst ? distinct : worst;
      }
      total += worst;
    }
  }
  return total;
}
static inline int conv3_halo_read_cycles(int groups, int row_step, int TWq, int LP, int PS, int off) {
  int total = 0;
  for (int grp = 0; grp < groups; ++grp) {
    int addr[64];
    for (int lane = 0; lane < 64; ++lane) {
      const int q = grp * 16 + (lane & 15);
      addr[lane] = (lane >> 4) * PS + row_step * (q / TWq) * LP + 4 * (q % TWq) + off;
    }
    total += conv3_read_cycles(addr);
  }
  return total;
}

// Run-time model of a Winograd launch of `base` (pixel tile, m-block) blocks of `nchunks` 4-channel chunks, cut into S K slabs
// (1: the launch runs as it is).  Two blocks are resident per CU and the dispatcher deals blocks over the 256 CUs, so a CU ends up
// with k = ceil(blocks / 256) of them and the launch takes as long as that CU: pairs of blocks at the shared rate and, for an odd
// k, one block that has the CU to itself and runs faster.  The 20 x 26 level at batch 8 is 304 (152) blocks of 128-256 chunks:
// k = 2 (1) where 1.19 (0.59) would do.  Cutting the chunks into S slabs multiplies the blocks and divides their length; it costs
// the fixed part of a block S times over and the reducer's launch and pass over (S + 1) x 64 KiB per tile block: 12 us + 6 TB/s.
struct Conv3SlabModel {
  double us_per_chunk;   // of a block that shares its CU
  double us_per_block;   // fixed part
  double lone_block;     // time of a block that has its CU to itself, as a fraction of a pair's
  const char* knob;      // environment: 0 / 1 never split, S >= 2 that many slabs wherever the shape admits it (tuning)

  double time_us(long base, int nchunks, int S, bool bw) const {
    const long cus = gsd_cu_count();
    const long k = (base * S + cus - 1) / cus;
    const double cu = (double)(k / 2) + (k & 1 ? lone_block : 0.0);
    double t = cu * (us_per_chunk * nchunks / S + us_per_block);
    if (S > 1) t += 12.0 + (double)(S + 1 + (bw ? 1 : 0)) * base * 65536.0 / 6.0e6;
    return t;
  }

  // the slab count the model picks: a split has to buy 3 %
  int pick(long base, int nchunks, bool bw) const {
    const int forced = gsd_env_int(knob, -1);
    if (forced == 0 || forced == 1) return 1;
    int best = 1;
    double tb = time_us(base, nchunks, 1, bw) * (forced > 1 ? 1e9 : 0.97);
    for (int S = 2; S <= 8 && nchunks / S >= 8; ++S) {
      if (forced > 1 && S != forced) continue;
      const double t = time_us(base, nchunks, S, bw);
      if (t < tb) {
        tb = t;
        best = S;
      }
    }
    return best;
  }
};

// Activate-once model: should relu(bn(raw)) of an (N, C, H, W) tensor be written once, row-pitched (gsd_bnrelu_pitched), so that
// its two-dimensional Winograd forward consumer runs as the plain aligned launch (the dX class) instead of activating its halo
// windows per m-block and moving them as unaligned pieces?  Both sides are linear in the batch, so among the batches at which
// the consumer keeps its form the answer is monotone:
//   saving = blocks x (chunks_act x s_full + chunks_plain x s_align) / (2 x CUs)     (two resident blocks per CU, as Conv3SlabModel)
//   cost   = launch_us + bytes the pass moves / copy_bytes_per_us
// s_full: us a block saves per 4-channel chunk that is deferred today and plain aligned then; s_align: per chunk that is plain
// but dense (unaligned 16-byte pieces, edge repair) today -- the up-sampled half of a concat, the pooled tensor.  Both grow with
// the consumer's m-blocks (the blocks that share one halo window): s = s0 + slope x log2(m-blocks), capped.
// Fitted to profiles/act_once_layers_b32.txt (batch 32, us saved per block-chunk x 512):
//   second convs (s_full)       m-blocks 1 / 2 / 4 / 8 / 16:  0.150  0.200  0.278  0.347  0.333   -> 0.15 + 0.06 log2, cap 0.33
//   encoder first convs (s_align)        2 / 4 / 8 / 16:      0.124  0.179  0.323  0.279           -> 0.07 + 0.055 log2, cap 0.28
//   decoder first convs, per skip chunk  1 / 2 / 4 / 8:       0.284  0.349  0.583  0.492  (model s_full + s_align: 0.22 0.335 0.45 0.565)
// The a-priori figure (0.205 of the K-slab model's 2.07 us per chunk = 0.42, from the two classes' static instruction counts) holds
// at the deep levels only: the shallow levels' launches save 7-10 %, not 21 %.  The copy rate is bn_bwd_apply_pitched_kernel's
// (25.6 GB in 3.87 ms).
struct ActOnceModel {
  double full0, full_slope, full_cap, align0, align_slope, align_cap, copy_bytes_per_us, launch_us;
  static double lg2(int v) { double r = 0.0; while (v > 1) { v >>= 1; r += 1.0; } return r; }
  double saving_us(long blocks, int chunks_act, int chunks_plain, int mblocks) const {
    const double l = lg2(mblocks);
    const double sf = full0 + full_slope * l < full_cap ? full0 + full_slope * l : full_cap;
    const double sa = align0 + align_slope * l < align_cap ? align0 + align_slope * l : align_cap;
    return (double)blocks * (chunks_act * sf + chunks_plain * sa) / (2.0 * gsd_cu_count());
  }
  // pass_kind 0: a pass of its own (read + write); 1: another kernel reads the tensor anyway and writes it on the way (the skip
  // tensor from the pitched max-pool); 2: the producer writes pitched rows INSTEAD of dense ones (the pooled tensor): free
  double cost_us(int N, int C, int H, int W, int pass_kind) const {
    if (pass_kind >= 2) return 0.0;
    return (pass_kind == 0 ? launch_us : 0.0) + (double)N * C * H * ((pass_kind == 0 ? W : 0) + round_up(W, 4)) * 4.0 / copy_bytes_per_us;
  }
};
