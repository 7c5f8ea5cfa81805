"""The metadynamics kernels must not touch scratch memory.

A lane keeps its frame's CVs, its running sum, the d gradient sums and the d scaled distances of the current hill in
registers; a per-lane array indexed by a runtime value (the CV loop not unrolled over the compile-time d, or the period
table indexed dynamically) lands in scratch and turns the hills walk into HBM traffic.  The check reads the
`.private_segment_fixed_size` the compiler recorded for every kernel of the built library whose name matches `metad_`
(tests/test_code_objects.py does the same for the kernels of the bench step)."""
import re
import shutil

import pytest

from pmarlo_amd._lib import LIB_PATH, METAD_GRID_MAX_D, METAD_MAX_D
from tests.test_code_objects import LLVM, _kernel_scratch

EXPECTED = ["metad_bias_kernel<", "metad_scan_kernel<", "metad_merge_kernel", "metad_heights_kernel",
            "metad_append_kernel"]


@pytest.mark.skipif(not (LLVM / "llvm-readelf").exists() or shutil.which("c++filt") is None or not LIB_PATH.exists(),
                    reason="needs the ROCm llvm tools and the built library")
def test_metad_kernels_use_no_scratch(tmp_path):
    scratch = {name: size for name, size in _kernel_scratch(tmp_path).items() if re.search(r"metad_", name)}
    for pattern in EXPECTED:
        assert any(pattern in name for name in scratch), f"no kernel matches {pattern}"
    # the bias kernel exists for every d, with and without the gradient; the scan for every grid dimension
    for d in range(1, METAD_MAX_D + 1):
        for grad in ("true", "false"):
            assert any(f"metad_bias_kernel<{d}, {grad}>" in name for name in scratch), (d, grad)
    for d in range(1, METAD_GRID_MAX_D + 1):
        assert any(f"metad_scan_kernel<{d}>" in name for name in scratch), d
    offenders = {name: size for name, size in scratch.items() if size}
    assert not offenders, f"scratch memory in metadynamics kernels: {offenders}"
