"""The OPES kernels must not touch scratch memory.

A lane of the bias kernel keeps its frame's CVs, its running sum and the d gradient sums in registers; every lane of the
deposit wave keeps the incoming kernel (centre, sigma, height) and the taker's in registers while they merge.  A
per-lane array indexed by a runtime value (a CV loop not unrolled over the compile-time d, a record written by "lane i
writes entry i") lands in scratch.  The check reads the `.private_segment_fixed_size` the compiler recorded for every
kernel of the built library whose name matches `opes_`, as tests/test_metad_code_objects.py does for `metad_`."""
import re
import shutil

import pytest

from pmarlo_amd._lib import LIB_PATH, METAD_MAX_D
from tests.test_code_objects import LLVM, _kernel_scratch

EXPECTED = ["opes_deposit_kernel<", "opes_bias_kernel<", "opes_live_kernel<"]


@pytest.mark.skipif(not (LLVM / "llvm-readelf").exists() or shutil.which("c++filt") is None or not LIB_PATH.exists(),
                    reason="needs the ROCm llvm tools and the built library")
def test_opes_kernels_use_no_scratch(tmp_path):
    scratch = {name: size for name, size in _kernel_scratch(tmp_path).items() if re.search(r"opes_", name)}
    for pattern in EXPECTED:
        assert any(pattern in name for name in scratch), f"no kernel matches {pattern}"
    # every kernel exists for every d; the two bias kernels with and without the gradient
    for d in range(1, METAD_MAX_D + 1):
        assert any(f"opes_deposit_kernel<{d}>" in name for name in scratch), d
        for grad in ("true", "false"):
            assert any(f"opes_bias_kernel<{d}, {grad}>" in name for name in scratch), (d, grad)
            assert any(f"opes_live_kernel<{d}, {grad}>" in name for name in scratch), (d, grad)
    offenders = {name: size for name, size in scratch.items() if size}
    assert not offenders, f"scratch memory in OPES kernels: {offenders}"
