"""Shared by the wide-decoder tests: the three reference trajectories of tests/golden/make_golden_wide.py.
A fixture that dropped its weights to stay under 1 MiB carries the seed that regenerates them
(oracle.xavier_normal_params) and their SHA-256."""
import hashlib

import numpy as np

import vaenmf_oracle as orc
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


# ---------------------------------------------------------------------------------------------------------------
# engines and oracle runs shared by tests/test_gpu_wide_decoders.py (and the CPU check of the sweep's seeds)
# ---------------------------------------------------------------------------------------------------------------
def dec_list(params):
    keys = ["decoder.hidden.%d.%s" % (i, k) for i in range(orc.n_hidden(params, "decoder")) for k in ("weight", "bias")]
    return [params[k] for k in keys + ["decoder.reconstruction.weight", "decoder.reconstruction.bias"]]


def enc_list(params):
    enc = [(params["encoder.hidden.%d.weight" % i], params["encoder.hidden.%d.bias" % i]) for i in range(orc.n_hidden(params, "encoder"))]
    return enc + [(params["encoder.sample.mu.weight"], params["encoder.sample.mu.bias"])]


def make_engine(params, F, K, counts, Rcap, precision="bf16x3", seeds=None):
    from vaenmf.engine import BatchEngine
    eng = BatchEngine(F, K, dec_list(params), precision=precision, max_frames=sum(counts), max_utts=len(counts),
                      z_dim=int(params["encoder.sample.mu.weight"].shape[0]))
    return eng.bind(counts, Rcap=Rcap, seeds=seeds)


class RecordingRNG:
    """Seeded numpy generator (the oracle's NumpyRNG) that keeps what it drew, in order."""

    def __init__(self, seed):
        self.g, self.draws = orc.NumpyRNG(seed), []

    def rand(self, *shape):
        self.draws.append(self.g.rand(*shape))
        return self.draws[-1]

    def randn(self, *shape):
        self.draws.append(self.g.randn(*shape))
        return self.draws[-1]


MIN_MARGIN = 5e-4      # a replayed decision is comparable when the oracle's own margin |log u - acc| is at least this


def first_narrow(draws, acc):
    """Per frame: the first step whose decision sits closer than MIN_MARGIN to its threshold (the number of steps: none)."""
    u = np.stack([draws[2 * m + 1] for m in range(acc.shape[0])])
    narrow = np.abs(np.log(u) - acc) < MIN_MARGIN
    return np.where(narrow.any(0), narrow.argmax(0), acc.shape[0])


def make_X(n, F, g):
    return ((g.standard_normal((n, F)) + 1j * g.standard_normal((n, F))) * (0.5 + 3 * np.exp(-np.arange(F) / (F / 6.0 + 1.0)))
            * np.exp(0.5 * g.standard_normal((n, 1)))).astype(np.complex64)


def oracle_iteration(model, X, params, K, seed, counts, y=None):
    """One EM iteration and the Wiener chain of the oracle for one utterance on a recorded numpy stream."""
    nsE, biE, nsW, biW = counts
    o = orc.MCEMOracle(model, 1, nsE, biE, nsW, biW, 0.01, reference_compat=False)
    r = RecordingRNG(seed)
    o.init_parameters(X, params, K, 1e-8, r, y=y)
    out = dict(o=o, W0=o.W.copy(), H0=o.H.copy(), Z0=o.Z.copy())
    tr, p0 = [], len(r.draws)
    Zs = o.sample_posterior(o.Z, nsE, biE, trace=tr)
    out["e_draws"], out["acc"], out["Zs"] = r.draws[p0:], np.stack([t["acc"] for t in tr]), Zs
    o.Z = Zs[:, -1, :].T.copy()
    o.compute_Vs(Zs); o.compute_Vs_scaled(); o.compute_Vx()
    out["Vs"] = o.Vs.copy()
    o.M_step()
    out["W"], out["H"], out["g"], out["cost"] = o.W.copy(), o.H.copy(), o.g.copy(), float(o.compute_expected_neg_log_like())
    tr2, p1 = [], len(r.draws)
    Zw = o.sample_posterior(o.Z, nsW, biW, trace=tr2)
    out["w_draws"], out["w_acc"] = r.draws[p1:], np.stack([t["acc"] for t in tr2])
    o.compute_Vs(Zw); o.compute_Vs_scaled(); o.compute_Vx()
    out["WFs"], out["WFn"] = o.compute_WF(sample=False)
    out["e_cut"], out["w_cut"] = first_narrow(out["e_draws"], out["acc"]), first_narrow(out["w_draws"], out["w_acc"])
    return out


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
