"""Shared by the wide-decoder tests: the three reference trajectories of tests/golden/make_golden_wide.py.
A fixture that dropped its weights to stay under 1 MiB carries the seed that regenerates them
(oracle.xavier_normal_params) and their SHA-256."""
import hashlib

import numpy as np

import vaenmf_oracle as orc
from em_support import oracle_iteration
from helpers import load_case

# name, model; the reference's h_dim (the decoder runs over reversed(h_dim), models.py:133)
WIDE_CASES = [("m1_f65_z128_h256", "M1"), ("m1_f65_z128_h128", "M1"), ("m2_vad_f65_z128_h256", "M2")]


def params_digest(params):
    h = hashlib.sha256()
    for k in sorted(params):
        h.update(k.encode())
        h.update(np.ascontiguousarray(params[k], dtype=np.float32).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


_cache = {}


def load_wide_case(name):
    """load_case, with the weights rebuilt from the stored seed where the file does not hold them."""
    if name not in _cache:
        z, params, draws, meta = load_case(name)
        if not params:
            params = orc.xavier_normal_params([meta["F"], meta["L"], [int(v) for v in z["dims_h"]]], seed=int(z["params_seed"]),
                                              y_dim=meta["Dy"], bias_std=0.05)
            assert np.array_equal(params_digest(params), z["params_sha256"]), "the seed no longer regenerates the fixture's weights"
        _cache[name] = (z, params, draws, meta)
    return _cache[name]


def make_X(n, F, g):
    return ((g.standard_normal((n, F)) + 1j * g.standard_normal((n, F))) * (0.5 + 3 * np.exp(-np.arange(F) / (F / 6.0 + 1.0)))
            * np.exp(0.5 * g.standard_normal((n, 1)))).astype(np.complex64)


# The shape and edge sweep: (F, z_dim, the reference's h_dim, frame counts, K, model).  F = 1, 17, 65, 130, 257, 640 are 1, 2, 5, 9,
# 17 and 40 bin tiles (idle wavefronts in the output layer, tile counts that are no multiple of 4, ten tiles per wavefront);
# h_dim [256, 128] is the decoder z -> 128 -> 256 -> F, [128, 256] its mirror z -> 256 -> 128 -> F (with labels: B1 [NT][256]).
SWEEP_COUNTS = (6, 5, 5, 3)
RAGGED = [1, 2, 19, 16, 1]
SWEEP = [
    (640, 128, [256, 128], RAGGED, 8, "M1"),
    (1, 128, [128], [3], 1, "M1"),
    (17, 64, [256, 128], [17], 32, "M1"),
    (65, 32, [256, 128], [5], 1, "M1"),
    (130, 128, [128], [20], 8, "M1"),
    (257, 128, [256, 128], [33], 8, "M1"),
    (65, 16, [128, 256], [18, 3], 8, "M2"),
    (130, 128, [256, 128], RAGGED, 32, "M2"),
]
SEED_SHIFT = {4: 1}       # draw seeds are 7000 + 100 case + utterance (+ 1000 shift): chosen on the CPU, see cut_short
_sweep_cache = {}


def sweep_case(i):
    """Weights, spectrograms, labels and the oracle's runs of sweep case i (computed once per process)."""
    if i not in _sweep_cache:
        F, L, hdim, counts, K, model = SWEEP[i]
        Dy = 1 if model == "M2" else 0
        params = orc.xavier_normal_params([F, L, hdim], seed=40 + i, y_dim=Dy, bias_std=0.05)
        g = np.random.default_rng(900 + i)
        Xs = [make_X(n, F, g) for n in counts]
        ys = [(g.random((n, Dy)) > 0.5).astype(np.float32) if Dy else None for n in counts]
        outs = [oracle_iteration(model, X, params, K, 7000 + 100 * i + u + 1000 * SEED_SHIFT.get(i, 0), SWEEP_COUNTS, y=ys[u]) for u, X in enumerate(Xs)]
        _sweep_cache[i] = (params, Xs, ys, outs)
    return _sweep_cache[i]


def cut_short(outs):
    """Frames of a case with a narrow decision in either chain, and the frame count."""
    e = np.concatenate([o["e_cut"] for o in outs]) < outs[0]["acc"].shape[0]
    w = np.concatenate([o["w_cut"] for o in outs]) < outs[0]["w_acc"].shape[0]
    return int((e | w).sum()), e.size
