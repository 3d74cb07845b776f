"""Every narrow kernel form at the decoder shapes beside z_dim 32 / h_dim [128, 128].

The reference's evaluation script lists z_dim 16 or 32 over h_dim [128] or [128, 128].  The decoder's shape does not enter
the dispatch, and each kernel treats it with code of its own: Dec::hidden's one-hidden branch (team and decoding kernels,
with its own partial dot for the odd last bin), the fragment copy that stands for layer 2 in wchain_kernel and
wchain4_kernel (hi and lo halves), the team kernel's noise mask per latent quad and the wave kernels' zero step for the
latent columns 16..31, and the re-packing of W1 as [32 latent columns | Dy label columns].  The sweeps over F, K and R run
at 32 / [128, 128] only, so here the other three shapes (decoder_shape_cases.D) cross the bin counts at which the dispatch
changes, through the very bodies of the bin-count sweep (em_support.split_mode_case / bench_mode_case / fused_run_case)
and at its bounds -- a 16-term first layer and one tanh layer fewer round no worse than the shape those bounds were set for:

  bf16x3   decode 2e-4, Wiener 5e-4, M-step W / H / g 1e-3, cost 2e-4 (relative); log-acceptance 3e-3, Zs / Z 1e-5 (absolute)
  bf16     decode 5e-2, M-step W / H / g 3e-2, cost 3e-3, Wiener 1e-2, first-step acceptance 0.5, wave - team 0.1

Every case asserts VAENMF_Q_CHAIN_KERNEL, Q_W_FUSED and Q_MSTEP_PATH against shape_class(): the decoder's shape must not
change the dispatch.  Every test prints what it measured (pytest -s)."""
import numpy as np
import pytest
import torch

import em_support as es
import vaenmf_oracle as orc
from decoder_shape_cases import (BF16_CASES, BF16_K, BF16_R, D, D_IDS, LABEL_CASES, NOISE_PSD_F, PADDING_CASES, PADDING_D, RUN_CASES,
                                 X3_CASES, X3_K, X3_R, case_id)
from dispatch_model import COUNTS, N_WAVE_TILES, shape_class
from helpers import need_gpu, rel_err

gpu = pytest.mark.gpu
C2 = 2.0 * 1.4426950408889634       # plan.hip scales the hidden layers by 2 log2(e): B1 holds C2 (b1 + W1[:, L:] y)


def _inputs(F, K, R, d, Dy=0):
    return es.inputs(F, K, R, Dy=Dy, z_dim=D[d][0], h_dim=D[d][1])


@gpu
@pytest.mark.parametrize("F,d", X3_CASES, ids=[case_id(F, d) for F, d in X3_CASES])
def test_split_mode_kernels_at_the_decoder_shape(F, d):
    """bf16x3 mode: decode, decoding Wiener filter, decoding M-step, one replayed chain with the default kernel and with the
    team kernel, then the store with device draws, with and without burn-in."""
    need_gpu()
    es.split_mode_case(_inputs(F, X3_K, X3_R, d))


@gpu
@pytest.mark.parametrize("F,d", BF16_CASES, ids=[case_id(F, d) for F, d in BF16_CASES])
def test_bench_mode_kernels_at_the_decoder_shape(F, d):
    """bf16 mode: decode, a replayed chain with every chain kernel the shape has, the stored M-step and Wiener filter with
    every W-statistics kernel the shape has."""
    need_gpu()
    es.bench_mode_case(_inputs(F, BF16_K, BF16_R, d))


def _dispatch(eng, sc):
    got = (es.query(eng, "Q_CHAIN_KERNEL"), es.query(eng, "Q_W_FUSED"), es.query(eng, "Q_MSTEP_PATH"))
    assert got == (sc["chain_kernel"], sc["w_fused"], 0), (got, sc)


@gpu
@pytest.mark.parametrize("d,F,precision,Dy", LABEL_CASES, ids=["%s_f%d_%s_dy%d" % (D_IDS[d], F, p, Dy) for d, F, p, Dy in LABEL_CASES])
def test_labels_behind_a_16_column_latent_block(d, F, precision, Dy):
    """M2 at z_dim 16: vaenmf_set_decoder_weights re-packs W1 as [32 latent columns, zero past 16 | Dy label columns], and
    vaenmf_layer1_bias folds the label block into a per-frame bias.  Dy = 1 (VAD labels) and Dy = F (IBM labels).
    B1 / (2 log2 e) against b1 + W1[:, 16:] y in float64 at 2e-4 (the bound of test_decoder_forward_m2_label_bias), relative
    to |b1| + |W1[:, 16:]| y, the size of what is summed: an element of a sum of Dy signed terms may cancel to nothing, and
    no float32 sum is relatively exact there.  Then that test's own assertion (decode against the oracle; 5e-2 in bf16 mode,
    the sweep's bound), and the stored M-step and Wiener filter as in test_stored_path_variants_against_the_oracle."""
    need_gpu()
    split = precision == "bf16x3"
    K, R = (X3_K, X3_R) if split else (BF16_K, BF16_R)
    c = _inputs(F, K, R, d, Dy=Dy)
    sc = shape_class(F, K, precision, N_WAVE_TILES, R, es.n_cus())
    nu = len(COUNTS)
    eng = es.engine(c, precision, seeds=[3, 4, 5])
    L = c.L
    W1, b1 = [np.asarray(a, np.float64) for a in es.dec_list(c.params)[:2]]
    y = np.concatenate(c.ys).astype(np.float64)
    ref = b1[None, :] + y @ W1[:, L:].T
    size = np.abs(b1)[None, :] + y @ np.abs(W1[:, L:]).T
    e = float(np.max(np.abs(eng.B1.cpu().numpy().astype(np.float64) / C2 - ref) / size))
    print("labels %s F=%d Dy=%d %s: layer-1 bias %.2e" % (D_IDS[d], F, Dy, precision, e))
    assert e < 2e-4
    eng.Zs.copy_(torch.from_numpy(c.Zs))
    Vs = eng.decode(R).cpu().numpy()
    e = rel_err(Vs[:, :, :F], es.decoder_of(c, c.Zs))
    print("labels %s F=%d Dy=%d %s: decode %.2e" % (D_IDS[d], F, Dy, precision, e))
    assert e < (2e-4 if split else 5e-2) and np.all(Vs[:, :, F:] == 0)
    eng.Z.copy_(torch.from_numpy(c.Z0))
    eng.sample_store(True)
    eng.mh_chain(R, 4, 0.01, call=0)
    Zs = eng.Zs[:, :R].cpu().numpy().copy()
    assert np.abs(Zs - c.Z0[:, None, :]).max() > 0.05 and np.all(Zs[:, :, L:] == 0)
    oracles = [es.oracle_at(c, eng, u, Zs) for u in range(nu)]
    eng.m_step_stored()
    _dispatch(eng, sc)
    tu, tc, tw = (1e-3, 2e-4, 5e-4) if split else (3e-2, 3e-3, 1e-2)
    es.m_step_against(c, eng, oracles, R, eng.cost_from_frames(R), tu, tc, "M2 stored M-step")
    es.wiener_against(c, eng, oracles, eng.wiener_stored(want_masks=True), tw, "M2 stored", absolute=not split)


@gpu
@pytest.mark.parametrize("path", ["decoding", "store"])
@pytest.mark.parametrize("F", NOISE_PSD_F)
def test_gains_only_m_step_with_one_hidden_layer(F, path):
    """A fixed noise PSD (mcem.py:543-578) at (32, [128]) in bf16x3 mode: the gains-only M-step and the Wiener filter through
    decode_kernel over given samples, and through the store over the chain's own, against the oracle: g 1e-3, cost 2e-4,
    Wiener 5e-4."""
    need_gpu()
    K, R = 1, 10
    c = _inputs(F, K, R, 1, Dy=1)
    sc = shape_class(F, K, "bf16x3", N_WAVE_TILES, R, es.n_cus())
    eng, Vb = es.prepare(c, "noNMF", "bf16x3", R)
    es.reset(c, eng)
    if path == "decoding":
        Zs = c.Zs
        eng.Zs.copy_(torch.from_numpy(Zs))
    else:
        eng.sample_store(True)
        eng.mh_chain(R, 4, 0.01, call=0)
        assert es.query(eng, "Q_CHAIN_KERNEL") == sc["chain_kernel"]
        Zs = eng.Zs[:, :R].cpu().numpy().copy()
        assert np.abs(Zs - c.Z0[:, None, :]).max() > 0.05
    oracles = []
    for u in range(len(COUNTS)):
        sl = eng.utt_slice(u)
        o = orc.MCEMOracleNoNMF(c.Xs[u], Vb[sl], c.gains[sl], c.Z0[sl], c.ys[u], c.params, 1, orc.NumpyRNG(0))
        o.compute_Vs(Zs[sl]); o.compute_Vs_scaled(); o.compute_Vx()
        o.M_step()
        oracles.append(o)
    if path == "decoding":
        eng.m_step(R)
    else:
        eng.m_step_stored()
    assert es.query(eng, "Q_MSTEP_PATH") == 0
    cost = eng.cost_from_frames(R)
    assert bool(torch.isfinite(eng.g).all()) and np.all(np.isfinite(cost))
    for u, o in enumerate(oracles):
        sl = eng.utt_slice(u)
        e = (rel_err(eng.g[sl].cpu().numpy(), o.g), abs(cost[u] - o.compute_expected_neg_log_like()) / abs(cost[u]))
        print("noNMF %s F=%d utt %d: g %.2e cost %.2e" % (path, F, u, e[0], e[1]))
        assert e[0] < 1e-3 and e[1] < 2e-4
    out = eng.wiener(R, want_masks=True) if path == "decoding" else eng.wiener_stored(want_masks=True)
    es.wiener_against(c, eng, oracles, out, 5e-4, "noNMF " + path)


# ---------------------------------------------------------------------------------------------------------------------
# the latent padding of z_dim 16: columns 16..31 of every latent row
PAD_NS, PAD_BURNIN = 4, 3
_PAD = [(F, p, k, d) for F, p, k in PADDING_CASES for d in PADDING_D]
_PAD_IDS = ["f%d_%s_%s" % (F, p, D_IDS[d]) for F, p, k, d in _PAD]


class _Padded:
    """An engine at z_dim 16 and one chain of PAD_NS samples after PAD_BURNIN steps from the state of inputs().  Zs is filled
    with 100 before every chain, so that what the chain leaves in the padding of its sample rows is what it wrote."""

    def __init__(self, F, precision, kernel, d):
        self.c = c = _inputs(F, X3_K if precision == "bf16x3" else BF16_K, 10, d)
        assert c.L == 16
        self.eng = es.engine(c, precision, seeds=[3, 4, 5])
        self.kernel = kernel
        assert shape_class(F, c.K, precision, N_WAVE_TILES, c.R, es.n_cus())["chain_kernel"] == kernel

    def chain(self, eps=None, u=None, call=2):
        eng = self.eng
        eng.Z.copy_(torch.from_numpy(self.c.Z0))
        eng.Zs.fill_(100.0)
        acc = eng.mh_chain(PAD_NS, PAD_BURNIN, 0.01, call=call, eps=eps, u=u, want_acc=True).cpu().numpy()
        assert es.query(eng, "Q_CHAIN_KERNEL") == self.kernel
        return acc, eng.Zs[:, :PAD_NS].cpu().numpy().copy(), eng.Z.cpu().numpy().copy()

    def replay(self, g):
        """Replay draws of the generator g [S][NT][32], all 32 columns drawn."""
        S, NT = PAD_NS + PAD_BURNIN, self.c.NT
        return g.standard_normal((S, NT, 32)).astype(np.float32), g.random((S, NT)).astype(np.float32)


def _moved(Zs, c):
    assert np.abs(Zs[:, :, :16] - c.Z0[:, None, :16]).max() > 0.05, "the chain did not move"


@gpu
@pytest.mark.parametrize("F,precision,kernel,d", _PAD, ids=_PAD_IDS)
def test_latent_padding_is_written_as_zero(F, precision, kernel, d):
    """After a chain with update_Z, columns 16..31 of Z and of the nsamples rows of Zs are exactly zero, with replayed draws
    (whose padding columns hold N(0, 1) draws here) and with the device's."""
    need_gpu()
    p = _Padded(F, precision, kernel, d)
    eps, u = p.replay(np.random.default_rng(F))
    for mode, kw in (("replay", dict(eps=torch.from_numpy(eps).cuda(), u=torch.from_numpy(u).cuda())), ("device", {})):
        acc, Zs, Z = p.chain(**kw)
        _moved(Zs, p.c)
        assert np.all(np.isfinite(acc)), mode
        worst = (float(np.abs(Z[:, 16:]).max()), float(np.abs(Zs[:, :, 16:]).max()))
        print("padding F=%d %s %s: largest |Z| %g, |Zs| %g in columns 16..31" % (F, precision, mode, worst[0], worst[1]))
        assert worst == (0.0, 0.0), (mode, worst)
        assert np.array_equal(Z, Zs[:, -1]), mode


@gpu
@pytest.mark.parametrize("F,precision,kernel,d", _PAD, ids=_PAD_IDS)
def test_finite_draws_in_the_padding_columns_change_no_bit(F, precision, kernel, d):
    """include/vaenmf.h, eps of a narrow plan with L = 16: columns 16..31 `must be finite`.  Uniform draws in +-1e30 there give
    the bits that zeros give: log-acceptances, samples and Z."""
    need_gpu()
    p = _Padded(F, precision, kernel, d)
    g = np.random.default_rng(F + 1)
    eps, u = p.replay(g)
    eps[:, :, 16:] = 0
    big = eps.copy()
    big[:, :, 16:] = g.uniform(-1e30, 1e30, big[:, :, 16:].shape).astype(np.float32)
    a = p.chain(eps=torch.from_numpy(eps).cuda(), u=torch.from_numpy(u).cuda())
    b = p.chain(eps=torch.from_numpy(big).cuda(), u=torch.from_numpy(u).cuda())
    _moved(a[1], p.c)
    for x, y, name in zip(a, b, ("acc", "Zs", "Z")):
        assert np.array_equal(x, y), name


@gpu
@pytest.mark.parametrize("F,precision,kernel,d", _PAD, ids=_PAD_IDS)
def test_replay_of_the_device_draws_equals_the_device_run(F, precision, kernel, d):
    """A REPLAY run fed from vaenmf_rng_fill (which fills all 32 columns of a narrow plan) equals the DEVICE run bit for bit,
    as test_device_rng_streams shows at z_dim 32."""
    need_gpu()
    p = _Padded(F, precision, kernel, d)
    eps, u = p.eng.rng_fill(2, PAD_NS + PAD_BURNIN)
    assert bool(torch.isfinite(eps).all()) and float(eps[:, :, 16:].abs().max()) > 0       # (the padding columns are drawn too)
    a = p.chain(call=2)
    b = p.chain(eps=eps, u=u)
    _moved(a[1], p.c)
    for x, y, name in zip(a, b, ("acc", "Zs", "Z")):
        assert np.array_equal(x, y), name


# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("F,precision,d", RUN_CASES, ids=["f%d_%s_%s" % (F, p, D_IDS[d]) for F, p, d in RUN_CASES])
def test_fused_run_at_the_decoder_shape(F, precision, d):
    """run() equals the stepped calls bit for bit, and the middle utterance alone gives the bits it has inside the batch:
    one case per chain kernel (wave, four-wavefront, team)."""
    need_gpu()
    c = _inputs(F, 10, 12, d)
    sc = shape_class(F, c.K, precision, N_WAVE_TILES, 6, es.n_cus())
    eng, eng2 = es.fused_run_case(c, precision)
    assert (eng.L, eng.H2) == (D[d][0], 128 if len(D[d][1]) == 2 else 0)
    for e in (eng, eng2):        # (the last chain of either is the Wiener chain)
        assert es.query(e, "Q_CHAIN_KERNEL") == sc["chain_kernel"]
    assert es.query(eng2, "Q_W_FUSED") == sc["w_fused"] == 0 and es.query(eng2, "Q_MSTEP_PATH") == 0
