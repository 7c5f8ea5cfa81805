#!/usr/bin/env python3
"""Time one DeepTICA training step on the device with HIP events: tools/time_deeptica_train.py [--reference]

The flagship network (64 -> 128 -> 64 -> 3, gelu, both LayerNorms, dropout 0.1 everywhere) at batch 256 and 8192:
  * the step's device time: msm_mlp_loss_grad + msm_adamw_step called back to back through the C ABI with no host
    synchronisation in between, the median of the timed runs over the steps of a run;
  * the step as the trainer takes it (Engine.mlp_loss_grad + Engine.adamw_step, which read the loss and the norms
    back every step, as the reference reads loss.item());
  * one whole epoch of fit() over 32768 + 8192 frames at batch 256 (128 steps and the validation pass).
--reference times the same step with plain torch modules on this machine's CPU threads (the reference's loop is
this: two forward passes, the loss in fp64, backward, clip_grad_norm_, AdamW.step), for the figure DESIGN.md puts
next to the device's; it restates the law with torch operators and needs no reference checkout."""
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

CONFIG = {"lag": 5, "n_out": 3, "hidden": [128, 64], "activation": "gelu", "layer_norm_in": True,
          "layer_norm_hidden": True, "linear_head": False, "dropout": 0.1, "hidden_dropout": [0.1, 0.1]}
F, N_FRAMES = 64, 32768 + 8192


def frames():
    rng = np.random.default_rng(0)
    walk = np.cumsum(rng.standard_normal((N_FRAMES, F)), axis=0) / 50.0
    return (np.sin(walk) + 0.1 * rng.standard_normal((N_FRAMES, F))).astype(np.float32)


def device():
    from pmarlo_amd import _lib
    from pmarlo_amd._lib import check, lib
    from pmarlo_amd.device import Engine
    from pmarlo_amd.features.deeptica import CurriculumConfig, DeepTICACurriculumTrainer, DeepTICAModel

    eng = Engine(0)
    x = frames()
    xd = eng.to_device(x)
    rng = np.random.default_rng(1)
    for batch in (256, 8192):
        model = DeepTICAModel.initialize(CONFIG, x.mean(0), x.std(0), seed=0)
        trainer = DeepTICACurriculumTrainer(model, CurriculumConfig(seed=0, batch_size=batch), engine=eng)
        trainer.set_frames(xd)
        spec = model.spec
        it = rng.integers(0, N_FRAMES - 5, size=batch)
        itd, itaud = eng.to_device(it), eng.to_device(it + 5)
        for _ in range(3):
            trainer.train_step(itd, itaud)
        eng.sync()
        # through the C ABI, nothing read back between the steps
        params, mean, scale = eng._mlp_on_device(spec)
        widths = np.ascontiguousarray(spec.widths, np.int32)
        drop = np.ascontiguousarray(trainer.dropout, np.float64)
        work = trainer._work
        stats, out = eng.empty((_lib.VAMP2_STATS,), np.float64), eng.empty((4,), np.float64)
        grad = eng.empty((params.size,), np.float64)
        steps, times = 20, []
        for rep in range(7):
            e0 = eng.event().record()
            for k in range(steps):
                check(lib.msm_mlp_loss_grad(eng.handle, xd.ptr, 0, N_FRAMES, F, F, mean.ptr, scale.ptr, 3,
                                            widths.ctypes.data, spec.activation, 1, 1, 1, params.ptr, params.size,
                                            itd.ptr, itaud.ptr, batch, drop.ctypes.data, 0, 100 + k, 1e-3, 1e-6, 0.15,
                                            1e-4, work.ptr, work.nbytes, stats.ptr, grad.ptr, None, 3), eng.handle)
                check(lib.msm_adamw_step(eng.handle, params.ptr, grad.ptr, trainer._m.ptr, trainer._v.ptr, params.size,
                                         100 + k, 3e-4, 0.9, 0.999, 1e-8, 1e-4, 1.0, out.ptr), eng.handle)
            e1 = eng.event().record()
            eng.sync()
            times.append(e0.elapsed_ms(e1) / steps)
        t0 = time.perf_counter()
        for _ in range(steps):
            trainer.train_step(itd, itaud)
        eng.sync()
        host_ms = (time.perf_counter() - t0) * 1e3 / steps
        print(f"batch {batch:5d}: device {np.median(times) * 1e3:8.1f} us per step (min {min(times) * 1e3:.1f}); "
              f"through the trainer {host_ms * 1e3:8.1f} us per step (wall)", flush=True)
    model = DeepTICAModel.initialize(CONFIG, x.mean(0), x.std(0), seed=0)
    cfg = CurriculumConfig(seed=0, tau_schedule=(5,), epochs_per_tau=1, warmup_epochs=0, batch_size=256)
    trainer = DeepTICACurriculumTrainer(model, cfg, engine=eng)
    trainer.fit([x[:1024]])                                    # warm: allocations, code objects
    trainer = DeepTICACurriculumTrainer(DeepTICAModel.initialize(CONFIG, x.mean(0), x.std(0), seed=0), cfg, engine=eng)
    t0 = time.perf_counter()
    hist = trainer.fit([x])
    wall = time.perf_counter() - t0
    print(f"fit, one epoch: {trainer.step} steps + validation in {wall * 1e3:.1f} ms wall "
          f"(val score {hist['best_val_score']:.4f})", flush=True)


def reference():
    import torch

    torch.manual_seed(0)
    x = torch.tensor(frames())
    x = (x - x.mean(0)) / x.std(0)
    net = torch.nn.Sequential(
        torch.nn.LayerNorm(F), torch.nn.Dropout(0.1), torch.nn.Linear(F, 128), torch.nn.LayerNorm(128), torch.nn.GELU(),
        torch.nn.Dropout(0.1), torch.nn.Linear(128, 64), torch.nn.LayerNorm(64), torch.nn.GELU(), torch.nn.Dropout(0.1),
        torch.nn.Linear(64, 3), torch.nn.GELU())
    opt = torch.optim.AdamW(net.parameters(), lr=3e-4, weight_decay=1e-4)

    def loss_fn(z0, zt):
        z0, zt = z0.double(), zt.double()
        m, d = z0.shape
        cov = torch.cov(torch.cat((z0, zt), 1).T, correction=0)
        eye = torch.eye(d, dtype=torch.float64)
        parts = []
        for C in (cov[:d, :d], cov[d:, d:]):
            mu = torch.clamp(torch.trace(C), min=1e-12) / d
            A = 0.85 * C + (0.15 * mu + mu * 1e-3) * eye
            A = 0.5 * (A + A.T)
            w = torch.linalg.eigvalsh(A)
            parts.append((torch.linalg.cholesky(A), w.max() / w.min()))
        left = torch.linalg.solve_triangular(parts[0][0], cov[:d, d:], upper=False)
        K = torch.linalg.solve_triangular(parts[1][0], left.T, upper=False).T
        return -(K * K).sum() + 1e-4 * (torch.log(parts[0][1]) + torch.log(parts[1][1]))

    print(f"torch {torch.__version__}, {torch.get_num_threads()} threads")
    for batch in (256, 8192):
        it = torch.randint(0, N_FRAMES - 5, (batch,))
        times = []
        for k in range(13):
            t0 = time.perf_counter()
            opt.zero_grad(set_to_none=True)
            loss = loss_fn(net(x[it]), net(x[it + 5]))
            loss.backward()
            torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
            opt.step()
            float(loss.item())
            times.append(time.perf_counter() - t0)
        print(f"batch {batch:5d}: torch on the CPU {np.median(times[3:]) * 1e6:9.1f} us per step", flush=True)


if __name__ == "__main__":
    reference() if "--reference" in sys.argv else device()
