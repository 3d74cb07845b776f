#!/usr/bin/env python3
"""Golden trajectories for the wide decoder shapes (z_dim 128, h_dim [256, 128] and [128]:
scripts/evaluate_M1.py:41-51), generated like the others by IMPORTING THE REFERENCE through
make_golden.run_case (full run() of the reference's generic classes, every draw recorded, the
seed with the widest decision margin kept).

Runs only where the reference is checked out next to the build (see make_golden.py).  Eight
frames keep the files small (128 latent draws per frame and step are most of the bytes).  A file
that would still pass 1 MiB drops its weights: they are oracle.xavier_normal_params of the stored
seed -- checked here bit for bit before they are dropped -- and the tests rebuild them
(tests/wide_cases.py) and compare their SHA-256 with the stored one.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wide.py [name ...]
"""
import hashlib
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import run_case, orc  # noqa: E402

MAX_BYTES = 1 << 20


def params_digest(params):
    h = hashlib.sha256()
    for k in sorted(params):
        h.update(k.encode())
        h.update(np.ascontiguousarray(params[k], dtype=np.float32).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def slim(name, dims_h, Dy):
    """Drop the weights of a fixture over 1 MiB after checking that its seed regenerates them."""
    path = os.path.join(HERE, name + ".npz")
    if os.path.getsize(path) <= MAX_BYTES:
        return
    z = dict(np.load(path, allow_pickle=False))
    F, L = int(z["meta"][0]), int(z["meta"][3])
    again = orc.xavier_normal_params([F, L, list(dims_h)], seed=int(z["seed"]), y_dim=Dy, bias_std=0.05)
    stored = {k[2:]: z.pop(k) for k in list(z) if k.startswith("p:")}
    assert sorted(again) == sorted(stored) and all(np.array_equal(again[k], stored[k]) for k in stored)
    z["params_seed"] = z["seed"]
    z["params_sha256"] = params_digest(stored)
    np.savez_compressed(path, **z)
    print("%s: weights dropped (seed %d regenerates them), %d bytes" % (name, int(z["seed"]), os.path.getsize(path)))

CASES = {
    "m1_f65_z128_h256": dict(model="M1", F=65, N=8, K=4, dims_h=[256, 128], L=128, niter=3, counts=(10, 6, 25, 8), seed=17),
    "m1_f65_z128_h128": dict(model="M1", F=65, N=8, K=4, dims_h=[128], L=128, niter=3, counts=(10, 6, 25, 8), seed=19),
    "m2_vad_f65_z128_h256": dict(model="M2", F=65, N=8, K=4, dims_h=[256, 128], L=128, niter=3, counts=(5, 7, 6, 9), Dy=1, seed=23),
}

if __name__ == "__main__":
    for name in (sys.argv[1:] or CASES):
        run_case(name, **CASES[name])
        slim(name, CASES[name]["dims_h"], CASES[name].get("Dy", 0))
