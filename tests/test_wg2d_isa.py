"""What the k-step loop of gsd_wgrad_w2d.hip compiles to (device-only compile, ~20 s, no GPU).

The dW kernel's rate is set by the vector instructions its loop executes: an fp32 MFMA stream on gfx950 hides scalar instructions
and LDS reads but no vector instruction (profiles/r05_mfma_f32_issue_ubench.txt), and the kernel lives at the 256-register limit.
Pinned here, per instantiation <NWM, NWN, PLAIN> of wgrad3x3_w2d_kernel: zero scratch and at most 256 registers, 96 MFMAs between
the first and the last MFMA (two unrolled k-steps), and the STATIC count of non-MFMA vector instructions in that window, counted as
tests/test_w2d_isa.py counts, split by basic block (a block = the instructions between two labels).

  Before the loop's bookkeeping left the vector pipe (uniform flags in vector registers, a branch behind every MFMA group, v_mov
  in front of the 16-byte LDS stores, per-lane compare chains in border k-steps):

    instantiation    window   arithmetic   in blocks that hold MFMAs / elsewhere   conditional branches in the window
    <4,2,true>         303        58                 116 / 187                               39
    <4,2,false>        323        78                 140 / 183                               39
    <2,4,true>         352        71                 132 / 220                               49
    <2,4,false>        364        99                 150 / 214                               49

  Now (every k-step loads and transforms, uniform state in scalar registers, a record order whose 16-byte groups are register
  pairs, border masks from per-lane class tables, border pieces out of line):

    <4,2,true>          82                            82 / 0                                  9
    <4,2,false>         97                            97 / 0                                  9
    <2,4,true>          89                            89 / 0                                 10
    <2,4,false>        111                           111 / 0                                 10

  The window is what an INTERIOR k-step pair runs: the pieces that only a border k-step runs (table lookup and offset masks 9-11,
  dy row masks 5-10, window column masks 12 per V task) are placed behind the loop and are not in it; with them in line the
  window held 150 / 165 / 165 / 187.  Both tables and the split are in profiles/wg2d_isa_counts.txt.

The budget is the count the kernel compiled to, plus 4.  The two comparisons with the earlier kernel are conditions, not measurements:
fewer vector instructions in the MFMA-holding blocks and fewer conditional branches in the window than it had.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = [(4, 2, True), (4, 2, False), (2, 4, True), (2, 4, False)]
# the parent's kernel, counted the same way: (window, in MFMA-holding blocks, conditional branches in the window)
PARENT = {(4, 2, True): (303, 116, 39), (4, 2, False): (323, 140, 39), (2, 4, True): (352, 132, 49), (2, 4, False): (364, 150, 49)}
# the finished kernel's window counts, plus 4
BUDGET = {(4, 2, True): 82 + 4, (4, 2, False): 97 + 4, (2, 4, True): 89 + 4, (2, 4, False): 111 + 4}


def analyse(asm):
    """{(NWM, NWN, PLAIN): dict(mfma, window, in_mfma_blocks, elsewhere, branches)} of the wgrad3x3_w2d_kernel instantiations."""
    out = {}
    for m in re.finditer(r"^_Z\d+wgrad3x3_w2d_kernelILi(\d)ELi(\d)ELb([01])EEv11WgW2dParams:[^\n]*\n(.*?)^\.Lfunc_end", asm, re.S | re.M):
        key = (int(m.group(1)), int(m.group(2)), m.group(3) == "1")
        # (opcode, basic block): a label or the instruction after a branch opens a block
        ops, blk = [], 0
        for ln in m.group(4).split("\n"):
            if re.match(r"^\.LBB\S*:", ln):
                blk += 1
                continue
            if not ln.startswith("\t") or ln.startswith("\t.") or ln.strip().startswith(";"):
                continue
            op = ln.split()[0]
            ops.append((op, blk))
        mf = [i for i, (op, _) in enumerate(ops) if op.startswith("v_mfma")]
        win = ops[mf[0]:mf[-1] + 1] if mf else []
        hold = {b for op, b in win if op.startswith("v_mfma")}
        vec = [(op, b) for op, b in win if op.startswith("v_") and not op.startswith("v_mfma")]
        inside = sum(1 for _, b in vec if b in hold)
        out[key] = dict(mfma=len(mf), window=len(vec), in_mfma_blocks=inside, elsewhere=len(vec) - inside,
                        branches=sum(1 for op, _ in win if op.startswith("s_cbranch")))
    return out


def table(counts):
    lines = ["instantiation <NWM,NWN,PLAIN>   window   in MFMA-holding blocks / elsewhere   conditional branches   (parent: window, in MFMA blocks, branches)"]
    for k in KEYS:
        c, p = counts[k], PARENT[k]
        lines.append("<%d,%d,%-5s>                   %5d    %5d / %-5d                      %5d                   (%d, %d, %d)" %
                     (k[0], k[1], str(k[2]).lower(), c["window"], c["in_mfma_blocks"], c["elsewhere"], c["branches"], p[0], p[1], p[2]))
    return "\n".join(lines)


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    from gelslim_depth_amd import build as b
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc on this machine")
    asm = str(tmp_path_factory.mktemp("wg2d_isa") / "gsd_wgrad_w2d.s")
    r = subprocess.run([hipcc] + b.CFLAGS + [f"-I{b.INCLUDE}", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S",
                        os.path.join(b.CSRC, "gsd_wgrad_w2d.hip"), "-o", asm], capture_output=True, text=True, check=True)
    with open(asm) as f:
        return r.stderr, analyse(f.read())


def test_wg2d_resources(compiled):
    remarks, _ = compiled
    names = re.findall(r"Function Name: (\S+)", remarks)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", remarks)]
    kern = {n: (s, v) for n, s, v in zip(names, scratch, vgprs) if "wgrad3x3_w2d_kernel" in n}
    print(kern)
    assert len(kern) == 4, sorted(kern)
    assert all(s == 0 and v <= 256 for s, v in kern.values()), kern


def test_wg2d_kstep_loop_vector_instruction_budget(compiled):
    _, counts = compiled
    assert sorted(counts) == sorted(KEYS), sorted(counts)
    text = table(counts)
    print(text)
    for k in KEYS:
        assert counts[k]["mfma"] == 96, (k, counts[k])          # two unrolled k-steps of 48
    for k in KEYS:
        c = counts[k]
        assert c["in_mfma_blocks"] < PARENT[k][1], (k, c)
        assert c["branches"] < PARENT[k][2], (k, c)
        assert c["window"] <= BUDGET[k], (k, c, BUDGET[k])
