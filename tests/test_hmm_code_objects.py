"""The HMM kernels must not touch scratch memory.

Their per-lane rows and columns of A and of the chunk product are meant to live in registers; a dynamically indexed
per-lane array, or 256 entries of A hoisted out of the step loop, lands in scratch and turns the walk into HBM traffic.
The check reads the `.private_segment_fixed_size` the compiler recorded for every kernel of the built library whose
name matches `hmm_` (tests/test_code_objects.py does the same for the kernels of the bench step)."""
import re
import shutil

import pytest

from pmarlo_amd._lib import LIB_PATH
from tests.test_code_objects import LLVM, _kernel_scratch

EXPECTED = ["hmm_product_kernel<", "hmm_boundary_kernel<", "hmm_pass_kernel<", "hmm_fold_seq_kernel<",
            "hmm_fold_all_kernel<", "hmm_emission_kernel", "hmm_emission_fold_kernel", "hmm_mstep_kernel"]


@pytest.mark.skipif(not (LLVM / "llvm-readelf").exists() or shutil.which("c++filt") is None or not LIB_PATH.exists(),
                    reason="needs the ROCm llvm tools and the built library")
def test_hmm_kernels_use_no_scratch(tmp_path):
    scratch = {name: size for name, size in _kernel_scratch(tmp_path).items() if re.search(r"hmm_", name)}
    for pattern in EXPECTED:
        assert any(pattern in name for name in scratch), f"no kernel matches {pattern}"
    # every walk kernel exists for the padded sizes 1, 2, 4, 8, 16
    for size in (1, 2, 4, 8, 16):
        assert any(f"hmm_pass_kernel<{size}>" in name for name in scratch)
    offenders = {name: size for name, size in scratch.items() if size}
    assert not offenders, f"scratch memory in HMM kernels: {offenders}"
