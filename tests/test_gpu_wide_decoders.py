"""GPU: the wide decoder shapes -- z_dim up to 128 and a hidden layer of 256 units -- on the wide chain kernel
(csrc/wide.hip) and the streaming M-step / Wiener kernels behind it.  Every test here fails without the wide path
(NotImplementedError from the engine, or a query the library does not know).

The reference builds its decoder over reversed(h_dim) (models.py:133): h_dim [256, 128] is z -> 128 -> 256 -> F, and the
mirrored z -> 256 -> 128 -> F is h_dim [128, 256]; both run.

Tolerances are those tests/test_gpu_parity.py uses for the same quantities on m1_f65_z16 (bf16x3 mode): log-acceptance 2e-3
absolute, decisions equal, Zs 5e-6, Z 1e-5, Vs 2e-4; after the first M-step W / H / g / Vb 5e-4 and the cost 1e-4; after the
full run cost 2e-4, S_hat / N_hat 2e-3 (L2), WFs 5e-3, W / g 2e-3.  bf16 mode: Vs 5e-2.  Trajectories on recorded numpy
draws are compared frame by frame up to the first decision the ORACLE itself makes closer than 5e-4 to its threshold
(em_support.first_narrow); at most 15 % of a case's frames may be cut short that way, and
tests/test_wide_decoders_cpu.py checks on the CPU that the chosen seeds stay under that cap.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vaenmf_oracle as orc
from em_support import RecordingRNG, dec_list, enc_list, first_narrow, make_engine, query, replay_buffers, setup_from_case, to_c
from helpers import need_gpu, rel_err, nrm_err
from wide_cases import WIDE_CASES, load_wide_case, sweep_case, SWEEP, SWEEP_COUNTS, RAGGED, cut_short, make_X


# ------------------------------------------------------------------------------------------------------------------
# 1. reference trajectories
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,model", WIDE_CASES)
def test_encoder_init(name, model):
    need_gpu()
    z, params, meta, o, rng, eng = setup_from_case(name, model, load=load_wide_case)
    assert eng.wide and eng.Lp == 128 and eng.Z.shape[1] == 128
    y = torch.from_numpy(z["y"]).to(eng.device) if model == "M2" else None
    eng.encode(enc_list(params), y)
    L = meta["L"]
    assert np.max(np.abs(eng.Z[:, :L].cpu().numpy().T - z["Z0"])) < 2e-5
    assert rel_err(eng.X2[:, :meta["F"]].cpu().numpy().T, o.X_abs_2) < 1e-6


@pytest.mark.parametrize("name,model", WIDE_CASES)
def test_first_em_iteration(name, model):
    """E-step chain (every log-acceptance of every frame, every decision, the samples, the store's variances), then the
    M-step, against the reference's recorded first iteration."""
    need_gpu()
    z, params, meta, o, rng, eng = setup_from_case(name, model, load=load_wide_case)
    assert eng.wide and eng.Lp == 128 and eng.Z.shape[1] == 128
    ns, bi = o.e_step_counts()
    S, N, F, K, L = ns + bi, meta["N"], meta["F"], meta["K"], meta["L"]
    pos0 = rng.pos
    eps, u = replay_buffers(rng, S, N, eng.Lp, eng.device)
    acc = eng.mh_chain(ns, bi, 0.01, eps=eps, u=u, want_acc=True).cpu().numpy()
    assert query(eng, 10) == 3                                              # VAENMF_Q_CHAIN_KERNEL: the wide kernel
    ref_acc = z["acc"][:S]
    assert acc.shape == ref_acc.shape == (S, N)
    print("max |acc - ref|", np.max(np.abs(acc - ref_acc)))
    assert np.max(np.abs(acc - ref_acc)) < 2e-3
    lu = np.log(u.cpu().numpy())
    assert np.array_equal(lu < acc, lu < ref_acc)
    rng.pos = pos0
    Zs_ref = o.sample_posterior(o.Z, ns, bi)
    assert np.max(np.abs(eng.Zs[:, :ns, :L].cpu().numpy() - Zs_ref)) < 5e-6
    assert L == eng.Lp or float(eng.Zs[:, :ns, L:].abs().max()) == 0.0
    assert np.max(np.abs(eng.Z[:, :L].cpu().numpy().T - z["E1_Z"])) < 1e-5
    Vs = eng.stored_variances(ns).cpu().numpy()
    assert rel_err(np.moveaxis(Vs[:, :, :F], 0, -1), z["E1_Vs"]) < 2e-4
    assert np.all(Vs[:, :, F:] == 0)
    eng.m_step(ns)
    assert rel_err(eng.W[0, :F, :K].cpu().numpy(), z["M1_W"]) < 5e-4
    assert rel_err(eng.Ht[:, :K].cpu().numpy().T, z["M1_H"]) < 5e-4
    assert rel_err(eng.g.cpu().numpy(), z["M1_g"]) < 5e-4
    assert rel_err(eng.Vb(0).cpu().numpy(), z["M1_Vb"]) < 5e-4
    cost = eng.cost_from_frames(ns)[0]
    assert abs(cost - z["cost"][0]) / abs(z["cost"][0]) < 1e-4


@pytest.mark.parametrize("name,model", WIDE_CASES)
def test_full_run_replay(name, model):
    need_gpu()
    z, params, meta, o, rng, eng = setup_from_case(name, model, load=load_wide_case)
    assert eng.wide and eng.Lp == 128 and eng.Z.shape[1] == 128
    ns, bi = o.e_step_counts()
    nw, bw = o.wf_counts()
    N, F = meta["N"], meta["F"]
    cost = np.zeros(meta["niter"])
    for it in range(meta["niter"]):
        eps, u = replay_buffers(rng, ns + bi, N, eng.Lp, eng.device)
        eng.mh_chain(ns, bi, 0.01, eps=eps, u=u)
        eng.m_step(ns)
        cost[it] = eng.cost_from_frames(ns)[0]
    eps, u = replay_buffers(rng, nw + bw, N, eng.Lp, eng.device)
    eng.mh_chain(nw, bw, 0.01, eps=eps, u=u, update_Z=False)
    S, Nn, WFs, WFn = eng.wiener(nw, want_masks=True)
    assert rng.pos == len(rng.draws)
    assert np.max(np.abs(cost - z["cost"]) / np.abs(z["cost"])) < 2e-4
    assert nrm_err(to_c(S, N, F), z["S_hat"]) < 2e-3
    assert nrm_err(to_c(Nn, N, F), z["N_hat"]) < 2e-3
    assert rel_err(WFs[:, :F].cpu().numpy().T, z["WFs"]) < 5e-3
    assert np.max(np.abs(eng.Z[:, :meta["L"]].cpu().numpy().T - z["Z"])) < 1e-5
    assert rel_err(eng.W[0, :F, :meta["K"]].cpu().numpy(), z["W"]) < 2e-3
    assert rel_err(eng.g.cpu().numpy(), z["g"]) < 2e-3


def _model_for(z, params, meta, model):
    import vaenmf
    hdim = [int(v) for v in z["dims_h"]]
    if model == "M1":
        vae = vaenmf.VariationalAutoencoder([meta["F"], meta["L"], hdim])            # the reference's constructor arguments
    else:
        vae = vaenmf.DeepGenerativeModel([meta["F"], meta["Dy"], meta["L"], hdim], None)
    vae.load_state_dict({k: torch.tensor(v) for k, v in params.items()})
    return vae


class _replayed_torch_draws:
    """torch.rand / torch.randn hand out a recorded stream (the reference's own draws, in its order)."""

    def __init__(self, draws):
        self.it = iter(draws)

    def __enter__(self):
        self._r, self._n = torch.rand, torch.randn
        torch.rand = lambda *s, **k: torch.tensor(next(self.it))
        torch.randn = lambda *s, **k: torch.tensor(next(self.it))

    def __exit__(self, *a):
        torch.rand, torch.randn = self._r, self._n


@pytest.mark.parametrize("name,model", WIDE_CASES)
def test_drop_in_classes_run_the_reference_models(name, model):
    """MCEM_M1 / MCEM_M2 with VariationalAutoencoder([F, 128, [256, 128]]) and friends: rng="replay" against the recorded
    run, rng="device" through the fused driver (stored path, wide kernel)."""
    need_gpu()
    import vaenmf
    z, params, draws, meta = load_wide_case(name)
    nsE, biE, nsW, biW = meta["counts"]
    vae = _model_for(z, params, meta, model)
    kw = dict(niter=meta["niter"], nsamples_E_step=nsE, burnin_E_step=biE, nsamples_WF=nsW, burnin_WF=biW, var_RW=0.01)
    for rng in ("replay", "device"):
        m = (vaenmf.MCEM_M1 if model == "M1" else vaenmf.MCEM_M2)(rng=rng, **kw)
        with _replayed_torch_draws(draws):
            if model == "M1":
                m.init_parameters(X=z["X"], vae=vae, nmf_rank=meta["K"], eps=1e-8, device="cuda:0")
            else:
                m.init_parameters(X=z["X"], y=torch.tensor(z["y"]), vae=vae, nmf_rank=meta["K"], eps=1e-8, device="cuda:0")
            assert rel_err(m.W.cpu().numpy(), z["W0"]) == 0
            assert np.max(np.abs(m.Z.cpu().numpy() - z["Z0"])) < 2e-5
            cost = m.run()
        assert cost.dtype == np.float64 and cost.shape == (meta["niter"],) and np.all(np.isfinite(cost))
        assert m.S_hat.dtype == np.complex64 and m.S_hat.shape == (meta["F"], meta["N"]) and np.all(np.isfinite(m.S_hat))
        assert query(m._eng, 10) == 3
        if rng == "replay":
            assert np.max(np.abs(cost - z["cost"]) / np.abs(z["cost"])) < 2e-4
            assert nrm_err(m.S_hat, z["S_hat"]) < 2e-3 and nrm_err(m.N_hat, z["N_hat"]) < 2e-3
            assert rel_err(m.W.cpu().numpy(), z["W"]) < 2e-3 and rel_err(m.g.cpu().numpy(), z["g"]) < 2e-3
            m._refresh(m._R)                                                    # the (R,F,N) views come from the store
            assert tuple(m.Vs.shape) == tuple(z["Vs_shape"])
        else:
            assert query(m._eng, 5) == 1                                        # VAENMF_Q_MSTEP_PATH: stored


# ------------------------------------------------------------------------------------------------------------------
# 2. the store contract against the oracle
# ------------------------------------------------------------------------------------------------------------------
_store_cache = {}


def _store_oracle(R, burnin):
    """Oracle chains (recorded numpy draws) of a ragged batch at F = 130 (9 bin tiles), decoder 128 -> 128 -> 256 -> F."""
    key = (R, burnin)
    if key not in _store_cache:
        F, L, K, counts = 130, 128, 4, [19, 5]
        params = orc.xavier_normal_params([F, L, [256, 128]], seed=77, bias_std=0.05)
        g = np.random.default_rng(78)
        Xs = [make_X(n, F, g) for n in counts]
        outs = []
        for u, X in enumerate(Xs):
            o = orc.MCEMOracle("M1", 1, R, burnin, 1, 0, 0.01, reference_compat=False)
            r = RecordingRNG(500 + 10 * u + R + burnin)
            o.init_parameters(X, params, K, 1e-8, r)
            p0, tr = len(r.draws), []
            Zs = o.sample_posterior(o.Z, R, burnin, trace=tr)
            outs.append(dict(W0=o.W.copy(), H0=o.H.copy(), Z0=o.Z.copy(), Zs=Zs, draws=r.draws[p0:], acc=np.stack([t["acc"] for t in tr]),
                             is_acc=np.stack([t["is_acc"] for t in tr])))
        _store_cache[key] = (params, Xs, counts, outs)
    return _store_cache[key]


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
@pytest.mark.parametrize("R,burnin", [(1, 0), (10, 0), (30, 0), (1, 7), (10, 7), (30, 7)])
def test_store_rows_and_src_against_the_oracle(R, burnin, prec):
    """VsS[frame][src[r][frame]] is the variance of the state after post-burn-in step r: the gathered rows equal
    decoder_forward of the oracle's samples (2e-4 bf16x3, 5e-2 bf16), padding bins are exactly 0, src is the oracle's
    accept history (slot R: the state at the end of the burn-in).  A frame is compared up to the first decision the oracle
    makes within 5e-4 (bf16x3) of its threshold; in bf16 mode -- whose log-acceptances carry the products' 2^-9 relative
    error -- up to the first decision on which device and oracle disagree, which may only be one within 0.5 of its threshold
    (the bound tests/test_gpu_parity.py::test_tiny_and_ragged_utterances_against_the_oracle uses for that mode)."""
    need_gpu()
    params, Xs, counts, outs = _store_oracle(R, burnin)
    F, NT, S, L = 130, sum(counts), R + burnin, 128
    eng = make_engine(params, F, 4, counts, Rcap=R, precision=prec)
    eng.set_spectrogram(Xs)
    eng.init_nmf([o["W0"] for o in outs], [o["H0"] for o in outs])
    eng.Z.copy_(torch.from_numpy(np.ascontiguousarray(np.concatenate([o["Z0"].T for o in outs], 0))))
    eps = np.ascontiguousarray(np.concatenate([np.stack([o["draws"][2 * m].T for m in range(S)]) for o in outs], 1))
    u = np.ascontiguousarray(np.concatenate([np.stack([o["draws"][2 * m + 1] for m in range(S)]) for o in outs], 1))
    acc = eng.mh_chain(R, burnin, 0.01, eps=torch.from_numpy(eps).to(eng.device), u=torch.from_numpy(u).to(eng.device), want_acc=True).cpu().numpy()
    acc_ref = np.concatenate([o["acc"] for o in outs], 1)
    is_acc = np.concatenate([o["is_acc"] for o in outs], 1)                   # [S][NT]
    if prec == "bf16x3":
        good = np.concatenate([first_narrow(o["draws"], o["acc"]) for o in outs])   # steps of a frame that are comparable
        assert (good < S).sum() <= 0.15 * NT
    else:
        differ = (np.log(u) < acc) != is_acc
        good = np.where(differ.any(0), differ.argmax(0), S)
        for n in np.nonzero(good < S)[0]:
            assert abs(np.log(u[good[n], n]) - acc_ref[good[n], n]) < 0.5, (n, good[n])
    # the oracle's accept history as the slot map: slot R until the first accepted post-burn-in step, then that step
    src_ref = np.full((R, NT), R, np.int64)
    for r in range(R):
        prev = src_ref[r - 1] if r else np.full(NT, R)
        src_ref[r] = np.where(is_acc[burnin + r], r, prev)
    Vs = eng.stored_variances(R).cpu().numpy()                                # [NT][R][Fs]
    assert np.all(Vs[:, :, F:] == 0) and np.all(np.isfinite(Vs))
    Zs_ref = np.concatenate([o["Zs"] for o in outs], 0)                       # [NT][R][L]
    Vs_ref = orc.decoder_forward(params, Zs_ref.reshape(NT * R, L)).reshape(NT, R, F)
    Zs = eng.Zs[:, :R].cpu().numpy()
    tol = 2e-4 if prec == "bf16x3" else 5e-2
    n_rows = 0
    for n in range(NT):
        rr = max(0, min(R, int(good[n]) - burnin))                            # post-burn-in steps of the frame that are comparable
        if good[n] < burnin:
            continue
        n_rows += rr
        assert rel_err(Vs[n, :rr, :F], Vs_ref[n, :rr]) < tol, (n, rr)
        assert np.max(np.abs(Zs[n, :rr] - Zs_ref[n, :rr]), initial=0.0) < 5e-6
        # src through the rows it names: the gathered row r of a frame is bit for bit its row src_ref[r] (an accepted
        # proposal's own row; slot R before the first one)
        for r in range(rr):
            s = int(src_ref[r, n])
            if s < R:
                assert np.array_equal(Vs[n, r], Vs[n, s]), (n, r, s)
    print("rows compared: %d of %d" % (n_rows, NT * R))
    assert n_rows >= 0.25 * NT * R          # (a frame that accepts nothing after the burn-in gathers slot R, the burn-in's end state, in every row)


# ------------------------------------------------------------------------------------------------------------------
# 3. shape and edge sweep
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(SWEEP)), ids=["F%d-z%d-h%s-%s" % (c[0], c[1], "x".join(map(str, c[2])), c[5]) for c in SWEEP])
def test_one_iteration_over_shapes_and_edges(i):
    need_gpu()
    F, L, hdim, counts, K, model = SWEEP[i]
    params, Xs, ys, outs = sweep_case(i)
    nsE, biE, nsW, biW = SWEEP_COUNTS
    NT, S = sum(counts), nsE + biE
    n_cut, n_all = cut_short(outs)
    assert n_all == NT and n_cut <= 0.15 * NT
    eng = make_engine(params, F, K, counts, Rcap=max(nsE, nsW))
    assert eng.wide and eng.Lp == 128 and eng.H1 == hdim[-1]
    dev = eng.device
    eng.set_spectrogram(Xs)
    eng.init_nmf([o["W0"] for o in outs], [o["H0"] for o in outs])
    if model == "M2":
        eng.set_labels(torch.from_numpy(np.concatenate(ys)))
        assert tuple(eng.B1.shape) == (NT, hdim[-1])
    eng.Z.zero_()
    eng.Z[:, :L].copy_(torch.from_numpy(np.ascontiguousarray(np.concatenate([o["Z0"].T for o in outs], 0))))

    def tensors(key, steps):
        eps = np.zeros((steps, NT, eng.Lp), np.float32)
        eps[:, :, :L] = np.concatenate([np.stack([o[key][2 * m].T for m in range(steps)]) for o in outs], 1)
        u = np.ascontiguousarray(np.concatenate([np.stack([o[key][2 * m + 1] for m in range(steps)]) for o in outs], 1))
        return torch.from_numpy(eps).to(dev), torch.from_numpy(u).to(dev), u

    def check_chain(acc, acc_ref, u, cut):
        steps = acc.shape[0]
        assert acc.shape == acc_ref.shape and np.all(np.isfinite(acc))
        m_idx = np.arange(steps)[:, None]
        upto = m_idx <= cut[None, :]                   # a frame's log-acceptances are comparable through its first narrow step
        print("max |acc - ref| %.2e" % np.max(np.abs(acc - acc_ref)[upto]))
        assert np.max(np.abs(acc - acc_ref)[upto]) < 2e-3
        before = m_idx < cut[None, :]
        assert np.array_equal((np.log(u) < acc)[before], (np.log(u) < acc_ref)[before])

    eps, u_d, u = tensors("e_draws", S)
    acc = eng.mh_chain(nsE, biE, 0.01, eps=eps, u=u_d, want_acc=True).cpu().numpy()
    assert query(eng, 10) == 3
    e_cut = np.concatenate([o["e_cut"] for o in outs])
    check_chain(acc, np.concatenate([o["acc"] for o in outs], 1), u, e_cut)
    whole = e_cut >= S
    Zs_ref = np.concatenate([o["Zs"] for o in outs], 0)
    Zs = eng.Zs[:, :nsE].cpu().numpy()
    assert np.max(np.abs(Zs[whole][:, :, :L] - Zs_ref[whole])) < 5e-6
    assert L == eng.Lp or float(np.abs(Zs[:, :, L:]).max()) == 0.0
    Vs = eng.stored_variances(nsE).cpu().numpy()
    assert np.all(Vs[:, :, F:] == 0)
    Vs_ref = np.concatenate([np.moveaxis(o["Vs"], -1, 0) for o in outs], 0)       # (R,F,N) -> [N][R][F]
    assert rel_err(Vs[whole][:, :, :F], Vs_ref[whole]) < 2e-4
    eng.m_step(nsE)
    cost = eng.cost_from_frames(nsE)
    off = np.concatenate([[0], np.cumsum(counts)])
    ok_utt = [bool(whole[off[j]:off[j + 1]].all()) for j in range(len(counts))]
    assert any(ok_utt)
    for j, o in enumerate(outs):
        sl = slice(off[j], off[j + 1])
        assert bool(torch.isfinite(eng.W[j]).all()) and bool(torch.isfinite(eng.g[sl]).all())
        if not ok_utt[j]:
            continue
        assert rel_err(eng.W[j, :F, :K].cpu().numpy(), o["W"]) < 5e-4
        assert rel_err(eng.Ht[sl, :K].cpu().numpy().T, o["H"]) < 5e-4
        assert rel_err(eng.g[sl].cpu().numpy(), o["g"]) < 5e-4
        assert abs(cost[j] - o["cost"]) / abs(o["cost"]) < 1e-4
    assert float(eng.W[:, F:].abs().max() if eng.Fs > F else 0) == 0 and float(eng.Ht[:, K:].abs().max() if eng.Kp > K else 0) == 0
    # the Wiener chain and filter, for utterances whose two chains are comparable throughout
    eps, u_d, u = tensors("w_draws", nsW + biW)
    eng.mh_chain(nsW, biW, 0.01, eps=eps, u=u_d, update_Z=False)
    w_cut = np.concatenate([o["w_cut"] for o in outs])
    Sh, Nh, WFs, WFn = eng.wiener(nsW, want_masks=True)
    for j, o in enumerate(outs):
        sl = slice(off[j], off[j + 1])
        if ok_utt[j] and bool((w_cut[sl] >= nsW + biW).all()):
            assert rel_err(WFs[sl, :F].cpu().numpy().T, o["WFs"]) < 5e-3
            assert nrm_err(to_c(Sh[sl], counts[j], F), o["WFs"] * o["o"].X) < 2e-3


def test_unaccepted_shapes_raise_with_the_accepted_set():
    """z_dim 16 with h_dim [256] (one hidden layer of 256), three hidden layers, H1 = 512, z_dim 256: NotImplementedError from
    the engine, and a non-zero code with a message that names the accepted set from vaenmf_plan_create itself."""
    need_gpu()
    from vaenmf import _lib
    from vaenmf.engine import BatchEngine
    for L, hdim in ((16, [256]), (128, [128, 128, 128]), (128, [128, 512]), (256, [128, 128])):
        params = orc.xavier_normal_params([65, L, hdim], seed=1)
        with pytest.raises(NotImplementedError):
            BatchEngine(65, 4, dec_list(params), max_frames=16, max_utts=1, z_dim=L)
    for L, H1, H2 in ((16, 256, 0), (128, 512, 128), (256, 128, 128), (128, 256, 256)):
        plan = C.c_void_p()
        cfg = _lib.Config(65, 4, L, H1, H2, 16, 1, _lib.PREC_BF16X3)
        assert _lib.lib().vaenmf_plan_create(C.byref(cfg), C.byref(plan)) != 0
        msg = _lib.lib().vaenmf_last_error().decode()
        assert "128" in msg and ("256" in msg or "64" in msg), msg


# ------------------------------------------------------------------------------------------------------------------
# 4. bit-for-bit properties
# ------------------------------------------------------------------------------------------------------------------
_BB = dict(F=130, L=128, hdim=[256, 128], K=8, counts=RAGGED, seeds=[3, 4, 5, 6, 7])


def _bb_inputs():
    if "params" not in _BB:
        g = np.random.default_rng(21)
        _BB["params"] = orc.xavier_normal_params([_BB["F"], _BB["L"], _BB["hdim"]], seed=9, bias_std=0.05)
        _BB["Xs"] = [make_X(n, _BB["F"], g) for n in _BB["counts"]]
        _BB["W0"] = [np.maximum(g.random((_BB["F"], _BB["K"])), 1e-8).astype(np.float32) for _ in _BB["counts"]]
        _BB["H0"] = [np.maximum(g.random((_BB["K"], n)), 1e-8).astype(np.float32) for n in _BB["counts"]]
    return _BB


def _bb_engine(prec, idx, Rcap=12, seeds=None, eng=None):
    b = _bb_inputs()
    if eng is None:
        eng = make_engine(b["params"], b["F"], b["K"], [b["counts"][i] for i in idx], Rcap=Rcap, precision=prec,
                          seeds=seeds or [b["seeds"][i] for i in idx])
    else:
        eng.bind([b["counts"][i] for i in idx], Rcap=Rcap, seeds=seeds or [b["seeds"][i] for i in idx])
    eng.set_spectrogram([b["Xs"][i] for i in idx])
    eng.init_nmf([b["W0"][i] for i in idx], [b["H0"][i] for i in idx])
    eng.encode(enc_list(b["params"]))
    return eng


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
def test_device_generator_equals_the_replay_of_rng_fill(prec):
    need_gpu()
    all_u = list(range(len(RAGGED)))
    eng = _bb_engine(prec, all_u)
    ns, bi = 6, 5
    eps, u = eng.rng_fill(3, ns + bi)
    assert tuple(eps.shape) == (ns + bi, eng.NT, 128) and tuple(u.shape) == (ns + bi, eng.NT)
    e = eps.cpu().numpy()
    assert abs(e.mean()) < 0.02 and abs(e.std() - 1) < 0.02 and 0 <= float(u.min()) and float(u.max()) < 1
    Z0 = eng.Z.clone()
    acc_d = eng.mh_chain(ns, bi, 0.01, call=3, want_acc=True)
    Zs_d, Z_d, Vs_d = eng.Zs.clone(), eng.Z.clone(), eng.stored_variances(ns)
    eng.Z.copy_(Z0)
    acc_r = eng.mh_chain(ns, bi, 0.01, eps=eps, u=u, want_acc=True)
    assert torch.equal(eng.Zs, Zs_d) and torch.equal(eng.Z, Z_d) and torch.equal(acc_r, acc_d) and torch.equal(eng.stored_variances(ns), Vs_d)
    assert float((Z_d - Z0).abs().max()) > 0
    # an utterance alone draws the same streams
    eng1 = _bb_engine(prec, [2])
    eps1, u1 = eng1.rng_fill(3, ns + bi)
    sl = eng.utt_slice(2)
    assert torch.equal(eps[:, sl], eps1) and torch.equal(u[:, sl], u1)


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
def test_an_utterance_alone_equals_itself_inside_the_ragged_batch(prec):
    need_gpu()
    ns, bi = 6, 5
    eng = _bb_engine(prec, list(range(len(RAGGED))))
    eng.mh_chain(ns, bi, 0.01, call=0)
    Vs = eng.stored_variances(ns)
    eng.m_step(ns)
    cost = eng.cost_from_frames(ns)
    for j in (2, 3, 4):                                  # 19 frames (two wave tiles), 16 (exactly one), 1
        e1 = _bb_engine(prec, [j])
        e1.mh_chain(ns, bi, 0.01, call=0)
        sl = eng.utt_slice(j)
        assert torch.equal(e1.Z, eng.Z[sl]) and torch.equal(e1.stored_variances(ns), Vs[sl])
        e1.m_step(ns)
        assert torch.equal(e1.W[0], eng.W[j]) and torch.equal(e1.Ht, eng.Ht[sl]) and torch.equal(e1.g, eng.g[sl])
        assert e1.cost_from_frames(ns)[0] == cost[j]


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
def test_fused_run_equals_the_stepwise_stored_calls(prec):
    need_gpu()
    niter, nsE, biE, nsW, biW = 2, 6, 5, 12, 4
    all_u = list(range(len(RAGGED)))
    eng = _bb_engine(prec, all_u)
    cost, S, N = eng.run(niter, nsE, biE, nsW, biW, 0.01)
    assert query(eng, 10) == 3 and query(eng, 5) == 1
    eng2 = _bb_engine(prec, all_u)
    c2 = np.zeros((len(all_u), niter))
    for it in range(niter):
        eng2.mh_chain(nsE, biE, 0.01, call=it)
        eng2.m_step_stored()
        c2[:, it] = eng2.cost_from_frames(nsE)
    eng2.mh_chain(nsW, biW, 0.01, call=niter, update_Z=False)
    S2, N2, _, _ = eng2.wiener_stored()
    assert torch.equal(S, S2) and torch.equal(N, N2) and torch.equal(eng.W, eng2.W) and torch.equal(eng.g, eng2.g) and torch.equal(eng.Z, eng2.Z)
    assert np.max(np.abs(c2 - cost.cpu().numpy()) / np.abs(c2)) < 1e-12
    assert np.all(np.isfinite(c2)) and bool(torch.isfinite(S).all())


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
def test_em_run_eager_capture_and_replays_are_equal(prec):
    """Four identical vaenmf_em_run calls -- launch by launch, captured, replayed, replayed -- give the same bits; a fifth with
    other seeds goes through the same graph and differs."""
    need_gpu()
    niter, nsE, biE, nsW, biW = 2, 6, 5, 12, 4
    all_u = list(range(len(RAGGED)))
    eng, outs, paths = None, [], []
    for call in range(4):
        eng = _bb_engine(prec, all_u, eng=eng)
        cost, S, N = eng.run(niter, nsE, biE, nsW, biW, 0.01)
        outs.append((cost.cpu().numpy(), S.cpu().numpy(), N.cpu().numpy(), eng.W.cpu().numpy()))
        paths.append(query(eng, 7))                      # VAENMF_Q_EM_GRAPH
        assert query(eng, 10) == 3 and query(eng, 5) == 1
    assert paths == [0, 1, 1, 1], paths
    for o in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(o, outs[0]))
    eng = _bb_engine(prec, all_u, seeds=[13, 14, 15, 16, 17], eng=eng)
    cost, S, N = eng.run(niter, nsE, biE, nsW, biW, 0.01)
    assert query(eng, 7) == 1
    assert not np.array_equal(S.cpu().numpy(), outs[0][1]) and np.all(np.isfinite(cost.cpu().numpy()))


# ------------------------------------------------------------------------------------------------------------------
# 5. fixed noise (the *_noNMF model) on a wide model with labels
# ------------------------------------------------------------------------------------------------------------------
def test_nonmf_variant_with_a_wide_model_against_the_oracle():
    """MCEM_M2_noNMF with DeepGenerativeModel([F, 1, 128, [256, 128]]), one iteration, against MCEMOracleNoNMF on the same
    recorded draws (tolerances of test_gpu_parity.py::test_nonmf_variant_against_reference)."""
    need_gpu()
    import vaenmf
    F, N, L, Dy, hdim = 65, 8, 128, 1, [256, 128]
    counts = (5, 7, 6, 9)
    params = orc.xavier_normal_params([F, L, hdim], seed=31, y_dim=Dy, bias_std=0.05)
    g0 = np.random.default_rng(32)
    X = make_X(N, F, g0)
    Vb = (0.2 + g0.random((N, F))).astype(np.float32)
    gains = (0.5 + g0.random(N)).astype(np.float32)
    Z0 = (0.5 * g0.standard_normal((N, L))).astype(np.float32)
    y = (g0.random((N, Dy)) > 0.5).astype(np.float32)
    r = RecordingRNG(33)
    o = orc.MCEMOracleNoNMF(X, Vb, gains, Z0, y, params, 1, r, *counts, 0.01)
    cost_ref = o.run()
    vae = vaenmf.DeepGenerativeModel([F, Dy, L, hdim], None)
    vae.load_state_dict({k: torch.tensor(v) for k, v in params.items()})
    with _replayed_torch_draws(r.draws):
        m = vaenmf.MCEM_M2_noNMF(X=X, Vb=Vb, g=torch.tensor(gains), Z=torch.tensor(Z0), y=torch.tensor(y), vae=vae, niter=1,
                                 device="cuda:0", nsamples_E_step=counts[0], burnin_E_step=counts[1], nsamples_WF=counts[2],
                                 burnin_WF=counts[3], var_RW=0.01)
        cost = m.run()
    assert query(m._eng, 10) == 3
    assert np.max(np.abs(cost - cost_ref) / np.abs(cost_ref)) < 2e-4
    assert rel_err(m.g.cpu().numpy(), o.g) < 2e-3
    assert np.max(np.abs(m.Z.cpu().numpy() - o.Z)) < 1e-5
    assert nrm_err(m.S_hat, o.S_hat) < 2e-3 and nrm_err(m.N_hat, o.N_hat) < 2e-3


# ------------------------------------------------------------------------------------------------------------------
# 6. refusals, and the narrow plans' kernels
# ------------------------------------------------------------------------------------------------------------------
def test_decoding_entries_refuse_a_wide_plan_and_name_the_stored_ones():
    need_gpu()
    from vaenmf import _lib
    from vaenmf.engine import _ptr, _stream
    l = _lib.lib()
    eng = _bb_engine("bf16x3", [3], Rcap=4)
    eng.mh_chain(4, 2, 0.01, call=0)
    Vs = torch.empty(eng.NT, 4, eng.Fs, device=eng.device)
    S = torch.empty_like(eng.X)
    calls = {
        "vaenmf_decode": lambda: l.vaenmf_decode(eng._plan, _ptr(eng.Zs), 4, 4, None, _ptr(Vs), _stream()),
        "vaenmf_m_step": lambda: l.vaenmf_m_step(eng._plan, _ptr(eng.X2), _ptr(eng.W), _ptr(eng.Ht), _ptr(eng.g), _ptr(eng.Zs), 4, 4, None,
                                                 _ptr(eng.cost_frames), _stream()),
        "vaenmf_wiener": lambda: l.vaenmf_wiener(eng._plan, _ptr(eng.X2), _ptr(eng.W), _ptr(eng.Ht), _ptr(eng.g), _ptr(eng.Zs), 4, 4, None,
                                                 _ptr(eng.X), _ptr(S), _ptr(S), None, None, _stream()),
    }
    W_before = eng.W.clone()
    for name, call in calls.items():
        assert call() != 0, name
        msg = l.vaenmf_last_error().decode()
        assert name in msg and "vaenmf_m_step_stored" in msg and "vaenmf_wiener_stored" in msg, msg
    assert torch.equal(eng.W, W_before)
    assert l.vaenmf_plan_query(eng._plan, _lib.Q_LP) == 128


@pytest.mark.parametrize("F,prec,kernel", [(513, "bf16x3", 0), (65, "bf16x3", 1), (257, "bf16", 2)])
def test_narrow_plans_keep_their_chain_kernel(F, prec, kernel):
    need_gpu()
    from vaenmf import _lib
    params = orc.xavier_normal_params([F, 32, [128, 128]], seed=2, bias_std=0.05)
    g = np.random.default_rng(4)
    eng = make_engine(params, F, 4, [19], Rcap=3, precision=prec, seeds=[1])
    assert not eng.wide and eng.Lp == 32 and query(eng, _lib.Q_LP) == 32
    eng.set_spectrogram([make_X(19, F, g)])
    eng.init_nmf([np.maximum(g.random((F, 4)), 1e-8).astype(np.float32)], [np.maximum(g.random((4, 19)), 1e-8).astype(np.float32)])
    eng.mh_chain(3, 2, 0.01, call=0)
    assert query(eng, 10) == kernel
    assert bool(torch.isfinite(eng.Zs).all())
