"""Shared by the tests of the EM kernels: engines bound to a batch, oracle runs on recorded draws, the float64 formulas and
the comparisons against them.  Nothing here needs a GPU or the built library to be imported: vaenmf.engine and the
library are loaded inside the functions that use them.

The module is not a test module, so pytest does not rewrite its asserts: each one carries its own message with the
compared values."""
import contextlib
import os
from types import SimpleNamespace

import numpy as np
import torch

import vaenmf_oracle as orc
from dispatch_model import COUNTS
from helpers import load_case, nrm_err, rel_err


# ---------------------------------------------------------------------------------------------------------------------
# engines and small queries
def dec_list(params):
    keys = ["decoder.hidden.%d.%s" % (i, k) for i in range(orc.n_hidden(params, "decoder")) for k in ("weight", "bias")]
    return [params[k] for k in keys + ["decoder.reconstruction.weight", "decoder.reconstruction.bias"]]


def enc_list(params):
    enc = [(params["encoder.hidden.%d.weight" % i], params["encoder.hidden.%d.bias" % i]) for i in range(orc.n_hidden(params, "encoder"))]
    return enc + [(params["encoder.sample.mu.weight"], params["encoder.sample.mu.bias"])]


def make_engine(params, F, K, counts, Rcap, precision="bf16x3", seeds=None):
    """A BatchEngine sized for and bound to `counts`; z_dim 32 where the weights hold no encoder."""
    from vaenmf.engine import BatchEngine
    z_dim = int(params["encoder.sample.mu.weight"].shape[0]) if "encoder.sample.mu.weight" in params else 32
    eng = BatchEngine(F, K, dec_list(params), precision=precision, max_frames=sum(counts), max_utts=len(counts), z_dim=z_dim)
    eng.bind(counts, Rcap=Rcap, seeds=seeds)
    return eng


def query(eng, what):
    """vaenmf_plan_query; what: the query's value or its name in vaenmf._lib ("Q_FS")."""
    from vaenmf import _lib
    return _lib.lib().vaenmf_plan_query(eng._plan, getattr(_lib, what) if isinstance(what, str) else what)


def n_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@contextlib.contextmanager
def env(**kv):
    """Environment variables set for the block; what they held before (nothing, as a rule) is put back after it."""
    before = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def to_c(t, N, F):
    """An interleaved (re, im) device spectrogram [N][>= F][2] as complex64 (F, N)."""
    return np.ascontiguousarray(t[:, :F].cpu().numpy()).view(np.complex64).reshape(N, F).T


# ---------------------------------------------------------------------------------------------------------------------
# the reference's recorded trajectories (tests/golden) and oracle runs on recorded numpy draws
def setup_from_case(name, model, precision="bf16x3", load=load_case):
    """Oracle, replay stream and engine of a golden case in the state before the first E-step."""
    z, params, draws, meta = load(name)
    nsE, biE, nsW, biW = meta["counts"]
    o = orc.MCEMOracle(model, meta["niter"], nsE, biE, nsW, biW, 0.01, reference_compat=True)
    rng = orc.ReplayRNG(draws)
    y = z["y"] if model == "M2" else None
    o.init_parameters(z["X"], params, meta["K"], 1e-8, rng, y=y)
    ns, bi = o.e_step_counts()
    nw, bw = o.wf_counts()
    eng = make_engine(params, meta["F"], meta["K"], [meta["N"]], Rcap=max(ns, nw), precision=precision)
    eng.set_spectrogram([z["X"]])
    eng.init_nmf([z["W0"]], [z["H0"]])
    if y is not None:
        eng.set_labels(torch.from_numpy(y))
    eng.Z.zero_()
    eng.Z[:, :meta["L"]].copy_(torch.from_numpy(np.ascontiguousarray(z["Z0"].T)))
    return z, params, meta, o, rng, eng


def replay_buffers(rng, S, N, Lp, dev):
    """The next S (randn(L,N), rand(N)) pairs of the recorded stream in the engine's layout [S][N][Lp]: the recorded draws
    fill columns 0..L-1 of the engine's rows, the padding columns stay zero."""
    eps = np.zeros((S, N, Lp), np.float32)
    u = np.empty((S, N), np.float32)
    for m in range(S):
        eps[m, :, :rng.draws[rng.pos].shape[0]] = rng.draws[rng.pos].T
        u[m] = rng.draws[rng.pos + 1]
        rng.pos += 2
    return torch.from_numpy(eps).to(dev), torch.from_numpy(u).to(dev)


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


def oracle_iteration(model, X, params, K, seed, counts, y=None, reference_compat=False, min_margin=None):
    """One EM iteration and the Wiener chain of the oracle for one utterance on a recorded numpy stream.  counts: (nsE, biE,
    nsW, biW) as the oracle's constructor takes them (reference_compat: with the reference's reading of them).
    min_margin None: the stream of `seed`; e_cut / w_cut say per frame where its first narrow decision is (first_narrow).
    min_margin given: the seed is advanced by 1000 until every accept / reject decision of both chains sits at least that
    far from its threshold (a replayed trajectory is only comparable while the decisions agree; the reference-generated
    goldens were selected the same way, at 1e-3; the HIP path's log-acceptances are within 1e-4 of the oracle's)."""
    for k in range(1 if min_margin is None else 200):
        o = orc.MCEMOracle(model, 1, *counts, 0.01, reference_compat=reference_compat)
        r = RecordingRNG(seed + 1000 * k)
        o.init_parameters(X, params, K, 1e-8, r, y=y)
        out = dict(o=o, W0=o.W.copy(), H0=o.H.copy(), Z0=o.Z.copy())
        ns, bi = o.e_step_counts()
        nw, bw = o.wf_counts()
        tr, p0 = [], len(r.draws)
        Zs = o.sample_posterior(o.Z, ns, bi, trace=tr)
        out["e_draws"], out["acc"], out["Zs"] = r.draws[p0:], np.stack([t["acc"] for t in tr]), Zs
        o.Z = Zs[:, -1, :].T.copy()
        o.compute_Vs(Zs); o.compute_Vs_scaled(); o.compute_Vx()
        out["Vs"] = o.Vs.copy()
        o.M_step()
        out["W"], out["H"], out["g"], out["cost"] = o.W.copy(), o.H.copy(), o.g.copy(), float(o.compute_expected_neg_log_like())
        tr2, p1 = [], len(r.draws)
        Zw = o.sample_posterior(o.Z, nw, bw, trace=tr2)
        out["w_draws"], out["w_acc"] = r.draws[p1:], np.stack([t["acc"] for t in tr2])
        o.compute_Vs(Zw); o.compute_Vs_scaled(); o.compute_Vx()
        out["WFs"], out["WFn"] = o.compute_WF(sample=False)
        out["e_cut"], out["w_cut"] = first_narrow(out["e_draws"], out["acc"]), first_narrow(out["w_draws"], out["w_acc"])
        if min_margin is None:
            return out
        margins = [np.abs(np.log(d[2 * m + 1]) - t["acc"]).min() for d, trc in ((out["e_draws"], tr), (out["w_draws"], tr2)) for m, t in enumerate(trc)]
        if min(margins) > min_margin:
            return out
    raise AssertionError("no stream with clear decisions found")


def replay_tensors(outs, key, S, dev):
    # (ascontiguousarray: stacking transposed views keeps THEIR memory order, and the C ABI takes dense row-major buffers)
    eps = np.ascontiguousarray(np.concatenate([np.stack([o[key][2 * m].T for m in range(S)]) for o in outs], 1))      # [S, NT, L]
    u = np.ascontiguousarray(np.concatenate([np.stack([o[key][2 * m + 1] for m in range(S)]) for o in outs], 1))      # [S, NT]
    return torch.from_numpy(eps).to(dev), torch.from_numpy(u).to(dev), u


# ---------------------------------------------------------------------------------------------------------------------
# the sweeps over F, K and R: one recipe of inputs, the oracle in the engine's state, comparisons at stated tolerances
# generator seed of a case's inputs when it is not 1000 + F (a case whose oracle margins leave out more than 15 % of the frames)
INPUT_SEEDS = {}


def inputs(F, K, R, Dy=0, counts=None, seed=None):
    """The recipe of test_m_step_and_chain_other_shapes: ragged batch, tilted spectrogram, Xavier decoder.  counts: the
    frames per utterance (COUNTS); seed: the generator seed of the inputs (INPUT_SEEDS, else 1000 + F)."""
    params = orc.xavier_normal_params([F, 32, [128, 128]], seed=7, y_dim=Dy, bias_std=0.05)
    g = np.random.default_rng(INPUT_SEEDS.get((F, K, R), 1000 + F) if seed is None else seed)
    counts = list(COUNTS if counts is None else counts)
    NT = sum(counts)
    c = SimpleNamespace(F=F, K=K, R=R, Dy=Dy, params=params, NT=NT, S_steps=6, ns=3, counts=counts)
    c.Xs = [((g.standard_normal((n, F)) + 1j * g.standard_normal((n, F))) * (0.5 + 3 * np.exp(-np.arange(F) / 60.0))).astype(np.complex64) for n in counts]
    c.W0 = [np.maximum(g.random((F, K)), 1e-8).astype(np.float32) for _ in counts]
    c.H0 = [np.maximum(g.random((K, n)), 1e-8).astype(np.float32) for n in counts]
    c.ys = [(g.random((n, Dy)) > 0.5).astype(np.float32) for n in counts] if Dy else [None] * len(counts)
    c.Zs = (0.7 * g.standard_normal((NT, R, 32))).astype(np.float32)
    c.gains = (0.5 + g.random(NT)).astype(np.float32)
    c.eps = g.standard_normal((c.S_steps, NT, 32)).astype(np.float32)
    c.uu = g.random((c.S_steps, NT)).astype(np.float32)
    c.Z0 = (0.5 * g.standard_normal((NT, 32))).astype(np.float32)
    c.off = np.concatenate([[0], np.cumsum(counts)])
    return c


def engine(c, precision, Rcap=None, seeds=None):
    eng = make_engine(c.params, c.F, c.K, c.counts, Rcap=Rcap or c.R, precision=precision, seeds=seeds)
    eng.set_spectrogram(c.Xs)
    eng.init_nmf(c.W0, c.H0)
    if c.Dy:
        eng.set_labels(torch.from_numpy(np.concatenate(c.ys)))
    eng.g.copy_(torch.from_numpy(c.gains))
    return eng


def oracle_at(c, eng, u, Zs=None):
    """The oracle of utterance u in the engine's present state (W, H, g), with the variances of the samples Zs."""
    sl = eng.utt_slice(u)
    o = orc.MCEMOracle("M2" if c.Dy else "M1", 1)
    o.init_parameters(c.Xs[u], c.params, c.K, 1e-8, orc.NumpyRNG(0), y=c.ys[u], W0=eng.W[u, :c.F, :c.K].cpu().numpy(),
                      H0=eng.Ht[sl, :c.K].cpu().numpy().T.copy())
    o.g = eng.g[sl].cpu().numpy().copy()
    if Zs is not None:
        o.compute_Vs(Zs[sl]); o.compute_Vs_scaled(); o.compute_Vx()
    return o


def all_finite(t, name, tag=""):
    bad = int((~torch.isfinite(t)).sum())
    assert bad == 0, "%s: %s holds %d non-finite of %d values" % (tag, name, bad, t.numel())


def padding_is_zero(eng, *tensors):
    """W, Ht beyond F and K, and the columns beyond F of `tensors` (as the callers pass them: WFs, WFn, |S_hat|, |N_hat|)."""
    F, K = eng.F, eng.K
    names = ("WFs", "WFn", "|S_hat|", "|N_hat|") if len(tensors) == 4 else tuple("tensor %d" % i for i in range(len(tensors)))
    pads = [("W rows past F", eng.W[:, F:] if eng.Fs > F else None), ("W columns past K", eng.W[:, :, K:] if eng.Kp > K else None),
            ("Ht columns past K", eng.Ht[:, K:] if eng.Kp > K else None)]
    pads += [(name + " columns past F", t[:, F:] if eng.Fs > F else None) for name, t in zip(names, tensors)]
    for name, pad in pads:
        m = float(pad.abs().max() if pad is not None else 0)
        assert m == 0, "%s not zero: largest |value| %g (F=%d Fs=%d K=%d Kp=%d)" % (name, m, F, eng.Fs, K, eng.Kp)


def m_step_against(c, eng, oracles, R, cost, tu, tc, tag):
    """W, H, g, cost of the engine after its M-step against the oracles' M_step() from the same state and samples."""
    for name in ("W", "Ht", "g"):
        all_finite(getattr(eng, name), name, tag)
    assert np.all(np.isfinite(cost)), "%s: cost not finite: %s" % (tag, cost)
    for u, o in enumerate(oracles):
        o.M_step()
        sl = eng.utt_slice(u)
        e = (rel_err(eng.W[u, :c.F, :c.K].cpu().numpy(), o.W), rel_err(eng.Ht[sl, :c.K].cpu().numpy().T, o.H),
             rel_err(eng.g[sl].cpu().numpy(), o.g), abs(cost[u] - o.compute_expected_neg_log_like()) / abs(cost[u]))
        print("%s F=%d K=%d utt %d: W %.2e H %.2e g %.2e cost %.2e" % ((tag, c.F, c.K, u) + e))
        assert e[0] < tu and e[1] < tu and e[2] < tu and e[3] < tc, (tag, u, e, "bounds", tu, tc)
    padding_is_zero(eng)


def wiener_against(c, eng, oracles, out, tol, tag, absolute=False):
    S, Nn, WFs, WFn = out
    for name, t in zip(("S_hat", "N_hat", "WFs", "WFn"), out):
        all_finite(t, name, tag)
    F = c.F
    for u, o in enumerate(oracles):
        ws, wn = o.compute_WF(sample=False)
        sl = eng.utt_slice(u)
        gs, gn = WFs[sl, :F].cpu().numpy().T, WFn[sl, :F].cpu().numpy().T
        if absolute:      # bf16 mode: masks in [0, 1] to an absolute bound, the filtered spectrograms in L2
            Sg = np.ascontiguousarray(S[sl, :F].cpu().numpy()).view(np.complex64)[..., 0].T
            Ng = np.ascontiguousarray(Nn[sl, :F].cpu().numpy()).view(np.complex64)[..., 0].T
            e = (float(np.max(np.abs(gs - ws))), float(np.max(np.abs(gn - wn))), nrm_err(Sg, ws * o.X), nrm_err(Ng, wn * o.X))
        else:
            e = (rel_err(gs, ws), rel_err(gn, wn))
        print("%s F=%d K=%d utt %d: Wiener " % (tag, F, c.K, u) + " ".join("%.2e" % v for v in e))
        assert max(e) < tol, (tag, u, e, "bound", tol)
    padding_is_zero(eng, WFs, WFn, S.abs().sum(-1), Nn.abs().sum(-1))


# ---------------------------------------------------------------------------------------------------------------------
# the float64 formulas and the bounds of tests/test_gpu_rank_and_samples.py (its docstring states them)
FLOOR = dict(W=2e-5, H=2e-5, g=2e-5, mask=2e-5, S_hat=2e-5, N_hat=2e-5, cost=1e-6)
E32_FACTOR = 16


def m_step64(X2, Vs, W, H, g):
    """mcem.py:90-152 and :70 in float64.  X2 (F, N), Vs (R, F, N), W (F, K), H (K, N), g (N,)."""
    iv = 1.0 / (g * Vs + W @ H)
    W = W * np.sqrt(((X2 * np.sum(iv * iv, 0)) @ H.T) / (np.sum(iv, 0) @ H.T))          # :107-110
    iv = 1.0 / (g * Vs + W @ H)                                                          # :113-114
    H = H * np.sqrt((W.T @ (X2 * np.sum(iv * iv, 0))) / (W.T @ np.sum(iv, 0)))          # :118-121
    Vb = W @ H                                                                           # :124-125
    nrm = np.sum(np.abs(W), 0)                                                           # :129-133
    W, H = W / nrm[None, :], H * nrm[:, None]
    g, cost = gains_step64(X2, Vs, Vb, g)
    return W, H, g, cost


def gains_step64(X2, Vs, Vb, g):
    """mcem.py:138-152 (= :564-578) and :70 in float64."""
    iv = 1.0 / (g * Vs + Vb)
    g = g * np.sqrt(np.sum(X2 * np.sum(Vs * iv * iv, 0), 0) / np.sum(np.sum(Vs * iv, 0), 0))
    Vx = g * Vs + Vb
    return g, float(np.mean(np.log(Vx) + X2 / Vx))


def wiener64(Vs, Vb, g):
    """mcem.py:486-488 in float64."""
    Vx = g * Vs + Vb
    return np.mean(g * Vs / Vx, 0), np.mean(Vb / Vx, 0)


def reference(o, variant, Vs64=None):
    """From an oracle that holds the state before the M-step and the samples' variances o.Vs: the float64 results
    (of Vs64 instead of o.Vs where given), and the float32 oracle's own (which runs its M-step)."""
    f8 = lambda a: np.asarray(a, np.float64)
    X2, Vs, g, X = f8(o.X_abs_2), (f8(o.Vs) if Vs64 is None else Vs64), f8(o.g), o.X.astype(np.complex128)
    if variant == "noNMF":
        Vb = f8(o.Vb)
        g2, cost = gains_step64(X2, Vs, Vb, g)
        ref = dict(g=g2, cost=cost)
    else:
        Vb = f8(o.W) @ f8(o.H)
        W2, H2, g2, cost = m_step64(X2, Vs, f8(o.W), f8(o.H), g)
        ref = dict(W=W2, H=H2, g=g2, cost=cost)
    ws, wn = wiener64(Vs, Vb, g)
    ref.update(mask=np.stack([ws, wn]), S_hat=ws * X, N_hat=wn * X)
    if Vs64 is not None:
        return ref, None
    o.compute_Vs_scaled(); o.compute_Vx()
    ws, wn = o.compute_WF(sample=False)
    o32 = dict(mask=np.stack([ws, wn]), S_hat=ws * o.X, N_hat=wn * o.X)
    o.M_step()
    o32.update(g=o.g, cost=float(o.compute_expected_neg_log_like()))
    if variant != "noNMF":
        o32.update(W=o.W, H=o.H)
    return ref, o32


def errors(got, ref):
    """Per quantity: W, H, g, cost relative (largest over the elements), the masks absolute, S_hat / N_hat relative in L2."""
    e = {}
    for k, v in got.items():
        if k == "mask":
            e[k] = float(np.max(np.abs(np.asarray(v, np.float64) - ref[k])))
        elif k in ("S_hat", "N_hat"):
            e[k] = nrm_err(v, ref[k])
        elif k == "cost":
            e[k] = abs(float(v) - ref[k]) / abs(ref[k])
        else:
            e[k] = rel_err(v, ref[k])
    return e


def bounds(e32):
    return {k: max(FLOOR[k], E32_FACTOR * v) for k, v in e32.items()}


def violations(err, bound):
    return [k for k in err if not err[k] <= bound[k]]


def fmt(err, bound=None):
    return " ".join("%s %.2e" % (k, err[k]) + ("/%.1e" % bound[k] if bound else "") for k in err)


def case_inputs(F, K, R, variant):
    """inputs() (labels with M2 and the fixed noise PSD).  From 65 samples per frame up the
    given samples are spread twice as wide: one row in 65 or 75 of the recipe's draws moves g by 3.0 to 3.5 bounds only
    at rank 32 ((513, 32, 75), (529, 32, 65), (640, 32, 75)), short of the four the condition asks for; 4.5 and more so."""
    c = inputs(F, K, R, Dy=0 if variant == "M1" else 1)
    if R >= 65:
        c.Zs *= np.float32(2.0)
    return c


def noise_psd(c):
    return (np.random.default_rng(c.F).random((c.NT, c.F)) + 0.1).astype(np.float32)


def prepare(c, variant, precision, Rcap):
    eng = engine(c, precision, Rcap=Rcap, seeds=[3, 4, 5])
    Vb = None
    if variant == "noNMF":
        Vb = noise_psd(c)
        Vbp = torch.zeros(eng.NT, eng.Fs)
        Vbp[:, :c.F] = torch.from_numpy(Vb)
        eng.set_noise_psd(Vbp.cuda())
    return eng, Vb


def reset(c, eng):
    eng.init_nmf(c.W0, c.H0)
    eng.g.copy_(torch.from_numpy(c.gains))
    eng.Z.copy_(torch.from_numpy(c.Z0))


def oracles_from(c, eng, variant, Vb, V):
    """The oracles in the engine's present state, holding the variances V [NT, R, F] the device produced."""
    out = []
    for u in range(len(COUNTS)):
        sl = eng.utt_slice(u)
        if variant == "noNMF":
            o = orc.MCEMOracleNoNMF(c.Xs[u], Vb[sl], eng.g[sl].cpu().numpy(), c.Z0[sl], c.ys[u], c.params, 1, orc.NumpyRNG(0))
        else:
            o = oracle_at(c, eng, u)
        o.Vs = np.ascontiguousarray(np.moveaxis(V[sl], 0, -1))           # (R, F, N)
        out.append(o)
    return out


def device_wiener(c, eng, u, out):
    S, Nn, WFs, WFn = out
    sl, F = eng.utt_slice(u), c.F
    cplx = lambda t: np.ascontiguousarray(t[sl, :F].cpu().numpy()).view(np.complex64)[..., 0].T
    return dict(mask=np.stack([WFs[sl, :F].cpu().numpy().T, WFn[sl, :F].cpu().numpy().T]), S_hat=cplx(S), N_hat=cplx(Nn))


def device_m_step(c, eng, u, cost, variant):
    sl = eng.utt_slice(u)
    d = dict(g=eng.g[sl].cpu().numpy(), cost=cost[u])
    if variant != "noNMF":
        d.update(W=eng.W[u, :c.F, :c.K].cpu().numpy(), H=eng.Ht[sl, :c.K].cpu().numpy().T)
    return d


def compare(tag, refs, got_of, failures):
    """Print every figure with its bound; collect what exceeds it (asserted at the end of the case, after every figure)."""
    for u, (ref, o32) in enumerate(refs):
        got = got_of(u)
        err, bound = errors(got, ref), bounds(errors({k: o32[k] for k in got}, ref))
        print("%s utt %d: %s" % (tag, u, fmt(err, bound)))
        failures += [(tag, u, k, err[k], bound[k]) for k in violations(err, bound)]
