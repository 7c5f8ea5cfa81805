"""The integer fp16 split of the k-means filter (pmarlo_amd/csrc/f16_split.h) against the fp64 library forms it
replaced, bit for bit, on the host: every fp16 number of the normal range and its fp64 neighbours, the rounding
midpoints, the range below 2^-14, the zeros, the edge of the split's domain and 10^6 seeded random doubles
(tests/filter_split_bits_main.cpp).  No GPU."""

from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_integer_split_matches_the_library_forms(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = tmp_path / "filter_split_bits"
    src = ROOT / "tests" / "filter_split_bits_main.cpp"
    # -ffp-contract=off: the reference forms are restated operation by operation
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", str(src), "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    fields = res.stdout.split()
    n_inputs, n_bad = int(fields[fields.index("inputs") + 1]), int(fields[fields.index("mismatches") + 1])
    # 2 x 30 x 1024 fp16 numbers with four neighbours each, their midpoints with two, and the 10^6 random doubles
    assert n_inputs > 2 * 30 * 1024 * 8 + 1_000_000
    assert n_bad == 0
