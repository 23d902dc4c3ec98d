"""The full-width d = 64 forward is ONE kernel per call: the running-max pass of the row blocks its fast passes refuse runs inside
the launch (fa_fwd_rp16_kernel.hpp, kInLaunch), so neither library carries a redo kernel (kScan = true) with D = 64 any more.
Read from the libraries' symbol tables; no GPU."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import summarize_profiles  # noqa: E402

PKG = os.path.join(ROOT, "flashattention_kernel_project_amd")
LIBS = ("libfa_mi355.so", "libfa_mi355_exp.so")


def _rp16_stubs(path):
    """demangled host-side launch stubs of fa_fwd_rp16_kernel instantiations in the library"""
    out = subprocess.run(["nm", "-C", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return [line.split(None, 2)[2] for line in out.splitlines() if "__device_stub__fa_fwd_rp16_kernel<" in line]


def _head_dim(name):
    args = [a.strip() for a in name.split("fa_fwd_rp16_kernel<", 1)[1].split(">", 1)[0].split(",")]
    return int(args[1])   # <T, D, X, ...>


@pytest.mark.parametrize("lib", LIBS)
def test_no_redo_kernel_at_d64(fa, lib):
    path = os.path.join(PKG, lib)
    assert os.path.exists(path), "build() makes both libraries"
    stubs = _rp16_stubs(path)
    # (the parsing sees the kernels at all: the full-width d = 64 forward is among them, and the one-wave family's redo kernel --
    # d = 128, kept -- is recognised as one)
    assert any(_head_dim(s) == 64 and not summarize_profiles.is_redo(s.replace("__device_stub__", "")) for s in stubs), stubs[:3]
    redo = [s for s in stubs if summarize_profiles.is_redo(s.replace("__device_stub__", ""))]
    assert redo and all(_head_dim(s) == 128 for s in redo), [s for s in redo if _head_dim(s) != 128]


def test_tail_cap_is_one_constant():
    """tests/test_gpu_single_launch.py reads the list's capacity from the header: exactly one definition to read"""
    src = open(os.path.join(PKG, "csrc", "fa_fwd_rp16_kernel.hpp")).read()
    assert len(re.findall(r"constexpr int kTailCap = (\d+);", src)) == 1
