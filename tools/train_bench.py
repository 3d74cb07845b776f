#!/usr/bin/env python3
"""Training step time: the HIP trainer (vaenmf.train.Trainer) against the same vaenmf.models module trained by PyTorch eager
with torch.optim.Adam on the same GPU -- what a user could do before the trainer existed.

Shapes of the reference's scripts: batch 128, x_dim 513; M1 (h=[128], z=16), M2 (h=[128,128], z=32, y_dim 513 and 1), the
classifier (h=[128,128], y_dim 513 and 1).  Both sides gather their batch from a device-resident frame matrix through a
device index vector, draw eps on the device and keep the losses on the device; nothing synchronises inside the timed loop.
Timing: device events around `--steps` steps (>= 200) after `--warmup` steps, best and median of `--repeats` such loops.

Prints one JSON line per model:  {"model", "hip_ms", "hip_steps_per_s", "eager_ms", "eager_steps_per_s", "speedup"}.
--no-eager: the HIP side alone (for a kernel trace of it)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "guided-vae-nmf_amd"))

import vaenmf  # noqa: E402
from vaenmf import train as vt  # noqa: E402

X_DIM, BATCH, NT = 513, 128, 16384
MODELS = {
    "M1": lambda: vaenmf.VariationalAutoencoder([X_DIM, 16, [128]]),
    "M2_ibm": lambda: vaenmf.DeepGenerativeModel([X_DIM, 513, 32, [128, 128]], None),
    "M2_vad": lambda: vaenmf.DeepGenerativeModel([X_DIM, 1, 32, [128, 128]], None),
    "Classifier_ibm": lambda: vaenmf.Classifier([X_DIM, [128, 128], 513]),
    "Classifier_vad": lambda: vaenmf.Classifier([X_DIM, [128, 128], 1]),
}


def timed(fn, steps, warmup, repeats):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(steps):
            fn(i)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / steps)
    return min(ms), float(np.median(ms))


def eager_step(model, opt, kind, X, Y, mean, std, eps=1e-8):
    def step(idx):
        x = X[idx]
        if kind == "Classifier":
            y = Y[idx]
            yh = model((x - mean) / (std + eps))
            loss = -torch.mean(torch.sum(y * torch.log(yh + eps) + (1 - y) * torch.log(1 - yh + eps), dim=-1))
        else:
            r, mu, logvar = model(x, Y[idx]) if kind == "M2" else model(x)
            recon = torch.mean(torch.sum(x / r - torch.log(x + eps) + torch.log(r) - 1, dim=-1))
            loss = recon - 0.5 * torch.mean(torch.sum(logvar - mu.pow(2) - logvar.exp(), dim=-1))
        loss.backward()
        opt.step()
        opt.zero_grad()
        return loss
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="*", default=list(MODELS))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    X = (torch.empty(NT, X_DIM).exponential_(1.0, generator=g) * torch.exp(torch.randn(NT, 1, generator=g))).to(dev)
    perms = [torch.randperm(NT, generator=g)[:BATCH].to(torch.int32).to(dev) for _ in range(64)]
    perms64 = [p.long() for p in perms]
    for name in a.models:
        torch.manual_seed(0)
        model = MODELS[name]()
        spec = vt.model_spec(model)
        Y = (torch.rand(NT, spec.y_dim, generator=g) < 0.4).float().to(dev) if spec.y_dim else None
        tr = vt.Trainer(model, max_batch=BATCH, seed=1, device=dev)
        tr.bind(X, Y)
        mean, std = X.mean(0), X.std(0)
        if spec.kind == "Classifier":
            tr.set_norm(mean.cpu().numpy(), std.cpu().numpy())
        out = torch.zeros(8, dtype=torch.float64, device=dev)
        best, med = timed(lambda i: tr.step(perms[i % 64], out=out), a.steps, a.warmup, a.repeats)
        res = {"model": name, "batch": BATCH, "x_dim": X_DIM, "steps": a.steps, "hip_ms": round(best, 4), "hip_ms_median": round(med, 4),
               "hip_steps_per_s": round(1e3 / best, 1)}
        if not a.no_eager:
            em = model.to(dev)
            opt = torch.optim.Adam(em.parameters(), lr=1e-3, betas=(0.9, 0.999))
            step = eager_step(em, opt, spec.kind, X, Y, mean, std)
            best_e, med_e = timed(lambda i: step(perms64[i % 64]), a.steps, a.warmup, a.repeats)
            res.update({"eager_ms": round(best_e, 4), "eager_ms_median": round(med_e, 4), "eager_steps_per_s": round(1e3 / best_e, 1),
                        "speedup": round(best_e / best, 2)})
        print(json.dumps(res), flush=True)
        tr.close()


if __name__ == "__main__":
    main()
