"""n_lead on its way to msm_tica_solve_leading, without a GPU: from Engine.tica_solve to the C call, from
MSMPipeline.tica_solve, and from ShardedMSM.step in a two-rank gloo run (the set-up of tests/test_dist_gloo.py).
tests/_host_engine.py's tica_solve has no n_lead (and ShardedMSM then passes none: the first test below); the gloo
run uses a subclass that takes it, records it and truncates as the device does."""

from __future__ import annotations

import os
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parents[1]

N, F, D, K, LAG, ITERS = 3000, 8, 3, 6, 5, 2


def _cfg(world):
    from pmarlo_amd.dist import ShardConfig

    return ShardConfig(n_frames=N, n_features=F, tica_dim=D, k=K, lag=LAG, kmeans_iters=ITERS, seed=3, n_total=N * world)


def _leading_host_engine():
    from tests._host_engine import HostEngine

    class LeadingHostEngine(HostEngine):
        """HostEngine whose tica_solve takes n_lead like the device engine: columns and eigenvalues from n_lead on
        are zero."""

        def __init__(self):
            super().__init__()
            self.n_lead_seen = []

        def tica_solve(self, moments, F, *, scale=None, epsilon=1e-6, kinetic_map=True, out=None, n_lead=0):
            self.n_lead_seen.append(n_lead)
            eig, W, m2, rank = super().tica_solve(moments, F, scale=scale, epsilon=epsilon, kinetic_map=kinetic_map,
                                                  out=out)
            if 0 < n_lead < F:
                eig.a[n_lead:] = 0.0
                W.a[:, n_lead:] = 0.0
            return out

    return LeadingHostEngine()


def test_engine_passes_n_lead_to_the_c_entry(monkeypatch):
    from pmarlo_amd import device

    calls = []

    class Recorder:
        def __getattr__(self, name):
            def call(*args):
                calls.append((name, args))
                return 0
            return call

    monkeypatch.setattr(device, "lib", Recorder())
    eng = device.Engine.__new__(device.Engine)
    eng.handle = 1234
    try:
        arr = [SimpleNamespace(ptr=p) for p in (10, 20, 30, 40, 50, 60)]
        out = tuple(arr[2:])
        assert eng.tica_solve(arr[0], 64, scale=arr[1], out=out, n_lead=10) == out
        assert eng.tica_solve(arr[0], 64, out=out) == out
    finally:
        eng.handle = None
    assert calls == [("msm_tica_solve_leading", (1234, 10, 20, 64, 1e-6, 1, 30, 40, 50, 60, 10)),
                     ("msm_tica_solve_leading", (1234, 10, None, 64, 1e-6, 1, 30, 40, 50, 60, 0))]


def test_pipeline_solves_for_dim_components_unless_told_otherwise():
    from pmarlo_amd.pipeline import MSMPipeline

    seen = []

    class Eng:
        def tica_solve(self, moments, F, **kw):
            seen.append((F, kw))
            return "eig", "W", "mean", "rank"

    pipe = MSMPipeline(Eng())
    mu = SimpleNamespace(shape=(12,))
    model = pipe.tica_solve("mom", mu, "sigma", "inv", 7, 4, epsilon=1e-5, kinetic_map=False)
    assert (model.eigenvalues, model.coefficients, model.mean, model.rank, model.lag, model.dim) == (
        "eig", "W", "mean", "rank", 7, 4)
    pipe.tica_solve("mom", mu, "sigma", "inv", 7, 4, all_pairs=True)
    assert seen == [(12, {"scale": "sigma", "epsilon": 1e-5, "kinetic_map": False, "n_lead": 4}),
                    (12, {"scale": "sigma", "epsilon": 1e-6, "kinetic_map": True, "n_lead": 0})]


def test_step_leaves_n_lead_out_for_an_engine_without_it():
    from pmarlo_amd.dist import ShardedMSM
    from tests import _gen
    from tests._host_engine import HostEngine

    eng = HostEngine()
    msm = ShardedMSM(eng, _cfg(1), eng.to_device(_gen.correlated_series(N, F, seed=1000)))
    assert msm._lead_kw == {}
    msm.step()
    assert np.count_nonzero(msm.eig.a) == F


def _worker(rank: int, world: int, port: int, out_dir: str) -> None:
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, str(ROOT))
    import torch
    import torch.distributed as dist

    from pmarlo_amd.dist import ShardedMSM, TorchComm, exchange_aliases, exchange_shapes
    from tests import _gen
    from tests._host_engine import HostArray

    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = _cfg(world)
    arrays = {nm: np.zeros(shape, np.dtype(dt)) for nm, (shape, dt) in exchange_shapes(cfg).items()}
    tensors = {nm: torch.from_numpy(a) for nm, a in arrays.items()}
    views = {nm: HostArray(a) for nm, a in arrays.items()}
    for name, (parent, first, length) in exchange_aliases(cfg).items():
        tensors[name] = tensors[parent][first:first + length]
        views[name] = views[parent].view((length,), offset_elems=first)
    eng = _leading_host_engine()
    msm = ShardedMSM(eng, cfg, eng.to_device(_gen.correlated_series(N, F, seed=1000 + rank)),
                     comm=TorchComm(tensors, views), shared=views)
    msm.step()
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), n_lead=np.asarray(eng.n_lead_seen), eig=msm.eig.a, W=msm.W.a,
             Y=np.asarray(msm.Y.a, np.float64), labels=msm.labels.a)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_step_asks_for_tica_dim_components(tmp_path):
    """Every rank asks for cfg.tica_dim components, solves identical bits, and nothing downstream reads past them: Y is
    the projection onto the kept columns."""
    import torch.multiprocessing as mp

    from oracle import npport
    from tests import _gen

    world, port = 2, 29500 + 2000 + (os.getpid() % 2000)
    mp.start_processes(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True, start_method="spawn")
    g = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
    for r in range(world):
        assert g[r]["n_lead"].tolist() == [D]
        assert not g[r]["eig"][D:].any() and not g[r]["W"][:, D:].any() and g[r]["eig"][:D].all()
    np.testing.assert_array_equal(g[0]["eig"], g[1]["eig"])
    np.testing.assert_array_equal(g[0]["W"], g[1]["W"])
    Xall = np.vstack([_gen.correlated_series(N, F, seed=1000 + r).astype(np.float64) for r in range(world)])
    Xp = npport.preprocess(Xall, scale=True)
    model = npport.tica_fit([Xp[r * N:(r + 1) * N] for r in range(world)], LAG, dim=D)
    np.testing.assert_allclose(g[0]["eig"][:D], model["eigenvalues"][:D], rtol=1e-9, atol=1e-12)
    assert g[0]["Y"].shape == (N, D) and np.isfinite(g[0]["Y"]).all()
