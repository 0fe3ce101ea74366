"""conv3x3_w2d_kernel at the chunk counts where its first chunk is special, element by element against fp64.

The kernel's accumulators start from 16 zero bytes a wave parks in LDS image 1 (no vector instruction zeroes them), its fills ride
in the gaps behind MFMA groups 0, 1 and 2 of the chunk before, and the "a chunk follows" flag is a scalar count.  What can go wrong
with that shows at the smallest channel counts: a block whose FIRST chunk is also its last (no fill behind it, image 1 never
filled), an even and an odd count through the loop's unroll by two, the switch to the second source segment directly behind the
first chunk, the shortest K slabs the launcher cuts, and the fused BatchNorm-backward epilogue behind a two-chunk loop.

Every case is the forward + statistics launch and the dX launch of tests/test_gpu_tile_forms_fp64.py's conv_case (or the fused
launch of its fused_case) -- every output element under fp64_ref.TAU_WINO = 6e-6 against the fp64 tap reference, sentinels around
every buffer, and a copy of the result with its largest single product removed must be rejected -- at N = 2 on 10 x 13 (one
10 x 16 tile: edge tiles on both axes, the masked epilogue) and 8 x 32 (one full tile: the unmasked epilogue), with Cout = 64
and 16 (a channel tail).  Operand forms: "x4" is one plain aligned source -- the <1,1,.> instantiations every dX launch of the
engine runs, forward and dX alike here --, "slack_bn" the deferred BatchNorm + ReLU source (<0,2,.>), "two11" / "two04" two
segments (plain / the first one deferred).  dX contracts over round_up(Cout, 4) channels: 16 and 4 chunks.
"""
import pytest

import tile_cases as T
from test_gpu_layer_shapes import gsd  # noqa: F401  (the module fixture)
from test_gpu_tile_forms_fp64 import clean_env, conv_case, fused_case  # noqa: F401  (clean_env: autouse, sets the trace knobs)

pytestmark = pytest.mark.gpu

SHAPES = [(10, 13), (8, 32)]
COUTS = [64, 16]

CASES = []
for h, w in SHAPES:
    for co in COUTS:
        for form in ("x4", "slack_bn"):
            for cin in (4, 8, 12):          # one chunk (the first is the last); an even and an odd count through the unroll by two
                CASES.append(T._cc("w2d", 2, h, w, cin, 0, co, form))
        # two segments, src0.C = 4 and src1.C = 8: the switch sits directly behind the first chunk
        CASES.append(T._cc("w2d", 2, h, w, 4, 8, co, "two11"))
        CASES.append(T._cc("w2d", 2, h, w, 4, 8, co, "two04"))
    # K slabs.  The launcher cuts a launch only into slabs of at least 8 chunks (Conv3SlabModel::pick, gsd_conv3x3_host.h: also under
    # a forced GSD_W2D_SPLIT), so slabs of ONE chunk -- Cin = 8 cut in two -- cannot be launched; the shortest slabs there are:
    # Cin = 64 in two slabs of 8 chunks, and Cin = 68 in slabs of 8 and 9 (the second starts on an odd chunk; 68 = one m-block and
    # a tail of 4 channels).  Cout = Cin, so that the dX launch is cut the same way.
    for c in (64, 68):
        CASES.append(T._cc("w2d", 2, h, w, c, 0, c, "x4", GSD_W2D_SPLIT=2))
        CASES.append(T._cc("w2d", 2, h, w, c, 0, c, "slack_bn", GSD_W2D_SPLIT=2))

# the fused BatchNorm-backward dX epilogue behind a two-chunk loop: dy has 8 channels, dz has 64 / 16
FUSED = [T.FusedCase("w2d", 2, h, w, 8, ci, ()) for h, w in SHAPES for ci in COUTS]


@pytest.mark.parametrize("case", CASES, ids=[T.case_id(c) for c in CASES])
def test_w2d_forward_and_dx_at_small_chunk_counts(gsd, monkeypatch, capfd, case):  # noqa: F811
    conv_case(gsd, monkeypatch, capfd, case, ns="first_chunk")


@pytest.mark.parametrize("case", FUSED, ids=[f"{c.n}x{c.h}x{c.w}-k{c.co}-m{c.ci}" for c in FUSED])
def test_w2d_fused_bn_backward_dx_at_two_chunks(gsd, monkeypatch, case):  # noqa: F811
    fused_case(gsd, monkeypatch, case, ns="first_chunk")
