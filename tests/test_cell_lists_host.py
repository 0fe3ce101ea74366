"""CPU: the argument checks of the cell-list build (gsd_cell_lists.h) run without a device.  tests/host/cell_lists_check.cpp is a
stand-alone program that calls them with null pointers, a short workspace, a misaligned `cells`, T out of range and a list length
out of range under all four entry-point names; it is built for the host with AddressSanitizer and UBSan and run directly."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO


def test_the_cell_list_checks_under_the_host_sanitizers(tmp_path):
    rocm = os.path.join(os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))), "llvm", "bin", "clang++")
    cxx = rocm if os.path.exists(rocm) else shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path / "cell_lists_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{os.path.join(REPO, 'include')}", f"-I{os.path.join(REPO, 'gelslim_depth_amd', 'csrc')}",
                    os.path.join(REPO, "tests", "host", "cell_lists_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("0 failure(s)") and "FAIL" not in r.stdout, r.stdout + r.stderr
    assert r.stdout.count("ok   ") == 4 * 12
