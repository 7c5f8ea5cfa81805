"""pytest configuration: `gpu` marker, repo root on sys.path, shared fixtures."""

from __future__ import annotations

import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

GOLDEN = ROOT / "tests" / "golden"


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden():
    def _load(name: str):
        return np.load(GOLDEN / name, allow_pickle=False)

    return _load


@pytest.fixture(scope="session")
def gpu_present() -> bool:
    """Whether torch sees a GPU, asked in a child process: torch ships its own HIP runtime, and bringing it up in the
    test process next to the one the engine's library links leaves every later Engine(0) of the session failing."""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.is_available())"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.split()[-1] == "True"


@pytest.fixture(scope="session")
def engine():
    """One Engine on cuda:0 for the whole GPU session (fails loudly without a GPU)."""
    from pmarlo_amd.device import Engine

    eng = Engine(0)
    yield eng
    eng.close()
