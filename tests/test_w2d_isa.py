"""What gsd_conv3x3_w2d.hip compiles to (device-only compile, ~10 s, no GPU).

The kernel's rate is set by its vector-to-MFMA instruction ratio: an fp32 MFMA stream on gfx950 hides scalar instructions and LDS
reads but no vector instruction (profiles/r05_mfma_f32_issue_ubench.txt), and it lives at the 256-register limit of two waves per
SIMD.  Two properties of the compiled code are therefore pinned here:

  (a) no instantiation of conv3x3_w2d_kernel uses scratch -- a spilled accumulator is reloaded inside the chunk loop;
  (b) the static count of non-MFMA vector instructions between the first and the last MFMA of an instantiation (the two unrolled
      chunks, 96 MFMAs per wave, with the rarely taken segment-switch and piece-repair blocks that sit between them) stays within
      a budget: the count the kernel compiled to when the bookkeeping left the vector pipe, plus 4.

                                      forward <false,2,false>   plain U4 <true,2,false>   dX <true,1,false>
      64-bit fill addresses, per-chunk
      vector predicates                        137                      101                      80
      scalar bases + exec masks                134                       99                      44

  The figure is STATIC and is not what a chunk executes: the window starts at the first MFMA, so one chunk's transform in front
  of it lies outside, and it includes cold blocks.  Split by basic block (profiles/r07_w2d_isa_counts.txt), of the 134 / 99 / 44
  the blocks that hold MFMAs plus the fall-through transform block between the two chunks hold 119 / 85 / 44; the other 15 / 14 / 0
  sit in blocks reached only through the segment-switch and piece-repair branches.  In the parent the blocks outside the MFMA
  blocks (26 / 28 / 28) held the per-chunk fill predicates, which every chunk ran.  What still runs per chunk besides the
  arithmetic: the uniform next-chunk flag (a v_cndmask + v_readfirstlane) and 5 to 6 v_lshl_add_u32 of LDS addresses.

  Of the 134 / 99 / 44, 65 / 34 / 34 are the transforms' arithmetic; the per-chunk bookkeeping that is left is the LDS image
  offset added to the lane's address registers.  The rest of the U4 forms' count is code a wave runs at most twice per block (the
  switch to the second source segment) or only at an image edge (overwriting the outside floats of a straddling piece).
"""
import os
import re
import shutil
import subprocess

import pytest

BUDGET = {(False, 2, False): 134 + 4, (True, 2, False): 99 + 4, (True, 1, False): 44 + 4}


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    from gelslim_depth_amd import build as b
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc on this machine")
    asm = str(tmp_path_factory.mktemp("w2d_isa") / "gsd_conv3x3_w2d.s")
    r = subprocess.run([hipcc] + b.CFLAGS + [f"-I{b.INCLUDE}", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S",
                        os.path.join(b.CSRC, "gsd_conv3x3_w2d.hip"), "-o", asm], capture_output=True, text=True, check=True)
    with open(asm) as f:
        return r.stderr, f.read()


def test_w2d_kernels_use_no_scratch(compiled):
    remarks, _ = compiled
    names = re.findall(r"Function Name: (\S+)", remarks)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks)]
    kernels = {n: s for n, s in zip(names, scratch) if "conv3x3_w2d_kernel" in n or "w2d_slab_reduce_kernel" in n}
    assert len(kernels) == 11, (sorted(kernels), remarks[-2000:])      # ten instantiations and the K-slab reducer
    assert all(v == 0 for v in kernels.values()), kernels


def test_w2d_chunk_loop_vector_instruction_budget(compiled):
    _, asm = compiled
    seen = {}
    for m in re.finditer(r"^_Z\d+conv3x3_w2d_kernelILb([01])ELi(\d)ELb([01])EEv9W2DParams:[^\n]*\n(.*?)^\.Lfunc_end", asm, re.S | re.M):
        key = (m.group(1) == "1", int(m.group(2)), m.group(3) == "1")
        ops = [ln.split()[0] for ln in m.group(4).split("\n") if ln.startswith("\t") and not ln.startswith("\t.") and
               not ln.strip().startswith(";")]
        mf = [i for i, op in enumerate(ops) if op.startswith("v_mfma")]
        assert len(mf) == 96, (key, len(mf))                           # two unrolled chunks of 48
        seen[key] = sum(1 for op in ops[mf[0]:mf[-1] + 1] if op.startswith("v_") and not op.startswith("v_mfma"))
    assert len(seen) == 10, sorted(seen)
    print("non-MFMA vector instructions between the first and the last MFMA:", {str(k): v for k, v in sorted(seen.items())})
    over = {k: (seen[k], lim) for k, lim in BUDGET.items() if seen[k] > lim}
    assert not over, f"(instantiation): (count, budget) {over}"
