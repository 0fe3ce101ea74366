"""What gsd_conv3x3_w2d_strips.hip compiles to (device-only compile, ~10 s, no GPU).

conv3x3_w2d_strips_kernel runs the chunk loop of conv3x3_w2d_kernel<PLAIN = 1, HM = 1, SPLIT = 0> (the shared body of
gsd_conv3x3_w2d_kernel.h) over the band-major flat tile list.  What it adds -- the listing, a third fill unit per wave, the image in
the lanes' offsets -- belongs to the prologue and the epilogue: the loop must not gain a vector instruction nor a gap, and the
kernel must still live in 256 registers without scratch (two blocks per CU).  Pinned here, as tests/test_w2d_isa.py and
tests/test_w2d_gaps.py pin the rectangular form:

  scratch    0 bytes per lane, at most 256 vector registers, occupancy 2 waves per SIMD
  mfma       96 between the first and the last (two unrolled chunks of 48)
  loop_valu  non-MFMA v_* in that window: at most 36, the bound of the rectangular plain form (the transforms' 34 + 2)
  gaps       MFMA-to-MFMA gaps that hold a non-MFMA v_* or a global_load_lds: at most 8 (the third unit shares group 1's gap)
  fills      global_load_lds in the kernel: 27 = nine per chunk (six weight pieces, three halo units) for the prologue's chunk and
             the loop's two unrolled copies -- nothing is patched or re-filled per chunk
"""
import os
import re
import shutil
import subprocess

import pytest


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    from gelslim_depth_amd import build as b
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc on this machine")
    asm = str(tmp_path_factory.mktemp("w2d_strips_isa") / "gsd_conv3x3_w2d_strips.s")
    r = subprocess.run([hipcc] + b.CFLAGS + [f"-I{b.INCLUDE}", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S",
                        os.path.join(b.CSRC, "gsd_conv3x3_w2d_strips.hip"), "-o", asm], capture_output=True, text=True, check=True)
    with open(asm) as f:
        return r.stderr, f.read()


def test_strips_kernel_fits_two_blocks_per_cu_without_scratch(compiled):
    remarks, _ = compiled
    m = re.search(r"Function Name: \S*conv3x3_w2d_strips_kernel\S*(.*?)LDS Size", remarks, re.S)
    assert m, remarks[-2000:]
    val = lambda name: int(re.search(name + r": (\d+)", m.group(1)).group(1))      # noqa: E731
    got = {k: val(k) for k in (r"ScratchSize \[bytes/lane\]", "VGPRs", "AGPRs", r"Occupancy \[waves/SIMD\]", "VGPRs Spill")}
    print(got)
    assert got[r"ScratchSize \[bytes/lane\]"] == 0 and got["VGPRs Spill"] == 0, got
    assert got["VGPRs"] + got["AGPRs"] <= 256 and got[r"Occupancy \[waves/SIMD\]"] >= 2, got


def test_strips_chunk_loop_is_the_rectangular_forms(compiled):
    _, asm = compiled
    m = re.search(r"^_Z\d+conv3x3_w2d_strips_kernel9W2DParams9W2DStrips:[^\n]*\n(.*?)^\.Lfunc_end", asm, re.S | re.M)
    assert m
    ops = [ln.split()[0] for ln in m.group(1).split("\n") if ln.startswith("\t") and not ln.startswith("\t.") and
           not ln.strip().startswith(";")]
    mf = [i for i, op in enumerate(ops) if op.startswith("v_mfma")]
    assert len(mf) == 96, len(mf)
    valu = lambda op: op.startswith("v_") and not op.startswith("v_mfma")          # noqa: E731
    win = ops[mf[0]:mf[-1] + 1]
    got = {"loop_valu": sum(valu(op) for op in win),
           "gaps": sum(any(valu(op) or op.startswith("global_load_lds") for op in ops[a + 1:b]) for a, b in zip(mf, mf[1:])),
           "fills": sum(op.startswith("global_load_lds") for op in ops),
           "scratch_ins": sum(op.startswith("scratch_") for op in ops)}
    print(got)
    assert got["loop_valu"] <= 36, got
    assert got["gaps"] <= 8, got
    assert got["fills"] == 27, got
    assert got["scratch_ins"] == 0, got
