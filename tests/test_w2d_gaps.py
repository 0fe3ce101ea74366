"""Where the vector work of conv3x3_w2d_kernel's chunk loop sits (device-only compile, ~10 s, no GPU).

An fp32 MFMA stream on gfx950 pays for every MFMA-to-MFMA gap that carries vector work -- about 8 cycles to open it and 4 per
instruction, and the two waves of a SIMD pay one after the other (profiles/r05_mfma_f32_issue_ubench.txt) -- so the loop keeps
its vector instructions and its LDS-DMA fills in few gaps, and everything that is not arithmetic of the transforms off the
vector pipe.  tests/test_w2d_isa.py pins zero scratch and the loop's instruction count with a margin; this module pins, for the
plain form <PLAIN = 1, HM = 1, SPLIT = 0> (every dX launch and the "activate once" forwards):

  gaps       MFMA-to-MFMA gaps between the first and the last MFMA of the two unrolled chunks that hold a non-MFMA v_* instruction
             or a global_load_lds: at most 8 (4 per chunk), the fills included.  The instantiation has no cold block in that window
             (one aligned source: no segment switch, no piece repair), so the window is counted as it stands; the fill blocks are
             skipped by a chunk only when no chunk follows it.  Compiled: 7 -- per chunk the gap behind group 0 (the six weight
             fills, no vector instruction), behind group 1 (one halo fill) and behind group 2 (the other halo fill and the second
             frequency row's ten packed instructions); between the two chunks the barrier with the first row's transform
             (parent: 13).  Both halo fills behind group 1 with the transform compiles to 5 and measured slower
             (profiles/w2d_gaps_layers_b32.txt).
  loop_valu  non-MFMA v_* in that window: at most 36 = the transforms' 34 + 2.  The LDS address additions are GONE (the lane's ten
             byte addresses wait in registers, reads take an immediate), not moved into a gap: this is the 36 case of the two the
             change was specified with, not the 44 one.  Compiled: 35 (parent: 44).
  pro_valu   v_* in front of the first MFMA: at least 180 fewer than the parent's 412 (the accumulators are zeroed by 48 LDS reads
             of 16 zero bytes instead of 192 v_mov).  Compiled: 230.

and for every instantiation loop_valu no higher than before (profiles/r07_w2d_isa_counts.txt, "after").

    python tests/test_w2d_gaps.py [file.s]      prints the table of profiles/w2d_gaps_isa_counts.txt (compiles when no file is given)
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

PLAIN_DX = (True, 1, False)
PARENT_LOOP_VALU = {(True, 1, True): 44, (True, 2, True): 99, (False, 2, True): 134, (True, 0, True): 74, (False, 0, True): 109,
                    (True, 1, False): 44, (True, 2, False): 99, (False, 2, False): 134, (True, 0, False): 74, (False, 0, False): 109}
PARENT_PRO_VALU_PLAIN_DX = 412


def compile_w2d(asm_path):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from gelslim_depth_amd import build as b
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        return None
    r = subprocess.run([hipcc] + b.CFLAGS + [f"-I{b.INCLUDE}", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S",
                        os.path.join(b.CSRC, "gsd_conv3x3_w2d.hip"), "-o", asm_path], capture_output=True, text=True, check=True)
    with open(asm_path) as f:
        return r.stderr, f.read()


def instructions(body):
    return [ln.split()[0] for ln in body.split("\n") if ln.startswith("\t") and not ln.startswith("\t.") and
            not ln.strip().startswith(";")]


def kernels(asm):
    """{(PLAIN, HM, SPLIT): opcodes in program order} of every conv3x3_w2d_kernel instantiation, and the reducer's under "reduce"."""
    out = {}
    for m in re.finditer(r"^_Z\d+conv3x3_w2d_kernelILb([01])ELi(\d)ELb([01])EEv9W2DParams:[^\n]*\n(.*?)^\.Lfunc_end", asm, re.S | re.M):
        out[(m.group(1) == "1", int(m.group(2)), m.group(3) == "1")] = instructions(m.group(4))
    m = re.search(r"^_Z\d+w2d_slab_reduce_kernel9W2DParams:[^\n]*\n(.*?)^\.Lfunc_end", asm, re.S | re.M)
    if m:
        out["reduce"] = instructions(m.group(1))
    return out


def is_valu(op):
    return op.startswith("v_") and not op.startswith("v_mfma")


def counts(ops):
    mf = [i for i, op in enumerate(ops) if op.startswith("v_mfma")]
    lo, hi = mf[0], mf[-1]
    epi = ops[hi + 1:]
    return {
        "total": len(ops), "mfma": len(mf),
        "loop_valu": sum(is_valu(op) for op in ops[lo:hi + 1]),
        "gaps": sum(any(is_valu(op) or op.startswith("global_load_lds") for op in ops[a + 1:b]) for a, b in zip(mf, mf[1:])),
        "pro_valu": sum(op.startswith("v_") for op in ops[:lo]),
        "epi_valu": sum(op.startswith("v_") for op in epi),
        "epi_br": sum(op.startswith("s_cbranch") or op == "s_branch" for op in epi),
        "epi_gstore": sum(op.startswith("global_store") for op in epi),
        "scratch_ins": sum(op.startswith("scratch_") for op in ops),
    }


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    got = compile_w2d(str(tmp_path_factory.mktemp("w2d_gaps") / "gsd_conv3x3_w2d.s"))
    if got is None:
        pytest.skip("no hipcc on this machine")
    ks = kernels(got[1])
    assert len(ks) == 11, sorted(map(str, ks))
    t = {k: counts(v) for k, v in ks.items() if k != "reduce"}
    for k in sorted(t, key=str):
        print(k, t[k])
    return t


def test_plain_dx_loop_has_few_vector_gaps(table):
    c = table[PLAIN_DX]
    assert c["mfma"] == 96
    assert c["gaps"] <= 8, c


def test_plain_dx_loop_holds_only_transform_arithmetic(table):
    assert table[PLAIN_DX]["loop_valu"] <= 36, table[PLAIN_DX]


def test_no_instantiation_gained_loop_vector_instructions(table):
    over = {k: (table[k]["loop_valu"], lim) for k, lim in PARENT_LOOP_VALU.items() if table[k]["loop_valu"] > lim}
    assert not over, f"(instantiation): (count, the parent's) {over}"


def test_plain_dx_prologue_lost_the_accumulator_zeroing(table):
    assert table[PLAIN_DX]["pro_valu"] <= PARENT_PRO_VALU_PLAIN_DX - 180, table[PLAIN_DX]


if __name__ == "__main__":
    if len(sys.argv) > 1:
        with open(sys.argv[1]) as f:
            text = f.read()
    else:
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            text = compile_w2d(os.path.join(d, "w2d.s"))[1]
    ks = kernels(text)
    r = ks.pop("reduce")
    print("reduce total %d valu %d" % (len(r), sum(op.startswith("v_") for op in r)))
    for k in sorted(ks, key=lambda k: (k[2], k[1] != 1, k[1] != 2, not k[0]), reverse=False):
        c = counts(ks[k])
        print("<%d,%d,%d> " % (k[0], k[1], k[2]) + " ".join(f"{n} {v}" for n, v in c.items()))
