"""The two-dimensional Winograd conv kernel (gsd_conv3x3_w2d.hip) splits a block's four waves by frequency-row half and pixel group:
a wave accumulates 4 m-tiles x 12 of the 24 frequencies, and the two halves of a pixel group trade accumulators after the chunk
loop.  On the CPU: the register budget of the kernel as compiled for gfx950, and the algebra of the split."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _resource_usage(src):
    from gelslim_depth_amd import build as b
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc on this machine")
    r = subprocess.run([hipcc] + b.CFLAGS + [f"-I{b.INCLUDE}", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(b.CSRC, src), "-o", os.devnull], capture_output=True, text=True, check=True)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    vgprs = [int(x) for x in re.findall(r"VGPRs: (\d+)", r.stderr)]
    agprs = [int(x) for x in re.findall(r"AGPRs: (\d+)", r.stderr)]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(vgprs) == len(agprs) == len(scratch), r.stderr[-2000:]
    return {n: (v, a, s) for n, v, a, s in zip(names, vgprs, agprs, scratch)}


def test_w2d_conv_kernels_fit_two_blocks_per_cu():
    """Every instantiation keeps 192 accumulators plus its loop state inside the 256 registers of two waves per SIMD, and the
    plain-source forms (every dX launch) need no scratch at all.  The deferred-BatchNorm forms hold the second source segment's
    halo offsets in scratch outside the chunk loop, as the channel-half split did (device-only compile, ~15 s)."""
    usage = _resource_usage("gsd_conv3x3_w2d.hip")
    kernels = {n: u for n, u in usage.items() if "conv3x3_w2d_kernel" in n}
    # <PLAIN, HM, SPLIT>: 2 x 3 halo forms x 2, less the aligned form (plain only) of the activated sources
    assert len(kernels) == 10, sorted(kernels)
    for name, (v, a, _) in kernels.items():
        assert v + a <= 256, (name, v, a)
    plain = {n: u for n, u in kernels.items() if n.startswith("_Z18conv3x3_w2d_kernelILb1E")}
    assert len(plain) == 6, sorted(kernels)
    assert all(s == 0 for (_, _, s) in plain.values()), plain


def test_frequency_halves_rebuild_the_output_transform():
    """The split in numbers: each half's column transform rows (fh = 0: A - B, B + C of window rows 0, 2, 1; fh = 1: A - B, B - C of
    rows 2, 1, 3) are B2^T d's rows, and A2^T M A4 over the traded accumulators is the whole tile's output."""
    rng = np.random.default_rng(7)
    d = rng.standard_normal((4, 6))
    g = rng.standard_normal((3, 3))
    B2T = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
    G2 = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=np.float64)
    A2T = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)
    B4T = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                    [0, 4, 0, -5, 0, 1]], dtype=np.float64)
    G4 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
                   [0, 0, 1]], dtype=np.float64)
    A4T = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64)
    t = B2T @ d
    for fh, (ra, rb, rc, sg) in enumerate(((0, 2, 1, 1.0), (2, 1, 3, -1.0))):
        np.testing.assert_array_equal(d[ra] - d[rb], t[2 * fh])
        np.testing.assert_array_equal(d[rb] + sg * d[rc], t[2 * fh + 1])
    U = G2 @ g @ G4.T
    M = U * (t @ B4T.T)
    halves = [M[0:2], M[2:4]]       # what the fh = 0 and fh = 1 waves accumulate
    traded = np.concatenate(halves)  # after the exchange: rows 0, 1 and 2, 3 side by side
    y = A2T @ traded @ A4T.T
    ref = np.array([[sum(d[a + u, b + v] * g[u, v] for u in range(3) for v in range(3)) for b in range(4)] for a in range(2)])
    np.testing.assert_allclose(y, ref, rtol=1e-12, atol=1e-12)
