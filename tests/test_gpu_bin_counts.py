"""The EM kernels at bin counts other than 16k + 1.

Every power-of-two STFT gives F = n_fft/2 + 1 = 16k + 1 bins, and the kernels are laid out round that: the plan takes the
odd last bin out of the MFMA tiles (Fm = F - 1), the streaming kernels give a lane four consecutive bins.  Any other F --
stft() takes any n_fft in [16, 4096], vaenmf_plan_create any F in 1..640 -- leaves a partly filled last bin tile, and
often a partly filled last 4-bin chunk (Fm % 4 != 0).  One sweep over F runs every EM kernel against the numpy oracle
from identical inputs; shape_class() (tests/dispatch_model.py) restates the dispatch of plan.hip / chain.hip / stream.hip, a CPU test checks that
the sweep reaches every kernel form the dispatch has, and the GPU tests check that the library reports the kernels
shape_class() predicts -- a later change of the dispatch makes the sweep fail instead of silently uncovering a kernel.

Tolerances are the ones tests/test_gpu_parity.py states for the same operations (its docstring and the docstrings of
test_m_step_and_chain_other_shapes, test_bench_mode_m_step_against_the_oracle, test_wave_chain_bf16_mode,
test_stored_m_step_and_wiener_match_the_decoding_ones, test_fused_w_statistics_equal_the_two_kernel_path).
"""
import numpy as np
import pytest
import torch

import vaenmf_oracle as orc
import em_support as es
from dispatch_model import COUNTS, N_WAVE_TILES, shape_class
from em_support import RecordingRNG
from helpers import GOLDEN, need_gpu, nrm_err, rel_err

gpu = pytest.mark.gpu        # (per test, not per module: test_sweep_reaches_every_dispatch_class runs without a GPU)

# F -> why it is in the sweep
SWEEP = {
    9: "n_fft 16, the smallest; one partial tile; F <= 16 keeps Fm = F; F % 4 = 1",
    16: "Fs == F, one exact tile",
    17: "smallest odd-last-bin shape, Fm = 16",
    64: "4 tiles, exact multiple",
    80: "5 tiles exact: last F with the W3 lo fragments in LDS in bf16x3 mode",
    81: "Fm = 80, the chain sees 6 tiles: first L2-streamed lo fragments",
    201: "n_fft 400 (25 ms): F % 4 = 1, F % 16 = 9",
    221: "n_fft 440 / 441: F % 16 = 13; 14 chain tiles, even Tm",
    250: "team geometry 3 with a partial tile; F % 4 = 2",
    251: "n_fft 500: F % 4 = 3 (three real bins and one padding bin in the last chunk)",
    256: "n_fft 510: Fs == F, one full chunk",
    260: "F % 4 = 0, F % 16 = 4: the 17-tile kernels with a partial tile",
    272: "upper edge of 17 tiles, Fs == F",
    273: "Fm = 272, 18 chain tiles: first shape on the team chain; NCH = 2",
    321: "n_fft 640: team geometry 0 at its 20-tile edge",
    442: "n_fft 882",
    501: "n_fft 1000: geometry 4 with a partial tile, F % 16 = 5",
    512: "Fs == F, 32 tiles",
    514: "the 33-tile bf16 kernels with a nearly empty last tile; NCH = 3",
    528: "33 tiles full, Fs == F",
    529: "Fm = 528, 34 tiles: team chain",
    640: "the maximum; 40 tiles; NCH = 3 ends at lane 31",
}
# bf16x3 mode: (F, rank, samples per frame)
X3_CASES = [(F, 10, 10) for F in SWEEP] + [(201, 8, 30), (260, 8, 30), (514, 8, 30), (250, 32, 10), (640, 32, 10)]
RUN_F = [9, 201, 250, 273, 501, 514, 640]
# bf16 (the bench mode)
BF16_F = [9, 64, 81, 201, 221, 250, 251, 260, 272, 442, 501, 514, 528, 640]
BF16_CASES = [(F, 8, 30) for F in BF16_F] + [(201, 10, 10), (514, 10, 10)]


def test_sweep_reaches_every_dispatch_class():
    """No GPU: the sweep holds at least one F for every kernel form that no 16k + 1 shape reaches, and every F % 4."""
    x3 = [shape_class(F, K, "bf16x3", N_WAVE_TILES, R) for F, K, R in X3_CASES]
    bf = [shape_class(F, K, "bf16", N_WAVE_TILES, R) for F, K, R in BF16_CASES]
    both = x3 + bf
    Fx3, Fbf = [c[0] for c in X3_CASES], [c[0] for c in BF16_CASES]
    assert set(Fx3) == set(SWEEP) and set(Fbf) <= set(SWEEP) and set(RUN_F) <= set(SWEEP)
    for prec, cls in (("bf16x3", x3), ("bf16", bf)):
        # wave chain with fewer than 5 bin tiles (MAXT = 5, not exact), with and without a partial tile
        assert any(c["chain_form"] == "wchain<5>" and c["partial_tile"] for c in cls), prec
        assert any(c["chain_form"] == "wchain<5>" and not c["partial_tile"] for c in cls), prec
        # 6..16 tiles (MAXT = 17, not exact) with a partial last tile
        assert any(c["chain_form"] == "wchain<17>" and c["partial_tile"] for c in cls), prec
        # the 17-tile kernels with a partial last tile and with Fs == F
        assert any(c["chain_tiles"] == 17 and c["partial_tile"] for c in cls), prec
        assert any(c["chain_tiles"] == 17 and not c["partial_tile"] for c in cls), prec
        # three 256-bin chunks in the streaming kernels; a partly filled 4-bin chunk with 1, 2 and 3 chunks
        assert any(c["nch"] == 3 for c in cls), prec
        assert {c["nch"] for c in cls if c["tail"]} == {1, 2, 3}, prec
        # W of a rank above 16 read from global memory because it does not fit LDS (bf16x3 sweep), and one that fits
        assert prec == "bf16" or any(not c["w_in_lds"] for c in cls)
    assert any(c["chain_form"] == "wchain<5,exact>" and c["lo_in_lds"] for c in x3)       # F = 80
    assert any(c["chain_form"] == "wchain<17>" and not c["lo_in_lds"] and c["chain_tiles"] == 6 for c in x3)   # F = 81
    # the 33-tile bf16 kernels, nearly empty and full last tile; both the four-wavefront and the one-wavefront form exist
    assert any(c["chain_tiles"] == 33 and c["partial_tile"] for c in bf) and any(c["chain_tiles"] == 33 and not c["partial_tile"] for c in bf)
    assert {c["chain_kernel"] for c in bf} == {0, 1, 2} and {c["chain_kernel"] for c in x3} == {0, 1}
    # team kernel geometries 3 / 4 ("no tile checks") with a partial last tile, geometry 2 above 32 tiles, geometry 0 at 20 tiles
    assert any(c["geom"] == 3 and c["partial_tile"] for c in both) and any(c["geom"] == 4 and c["partial_tile"] for c in both)
    assert any(c["geom"] == 2 and c["team_tiles"] > 32 for c in both)
    assert any(c["geom"] == 0 and c["team_tiles"] == 20 for c in both)
    assert {c["geom"] for c in x3 if c["chain_form"] == "team"} == {0, 2, 4}       # (geometry 3 runs under VAENMF_TEAM_CHAIN=1)
    # F <= 16 (Fm = F even when F % 16 == 1 could hold) and Fs == F (no padding at all) at 1, 2 and 3 chunks
    assert any(F <= 16 and F % 16 != 0 for F in SWEEP) and {shape_class(F, 10, "bf16x3", 6)["nch"] for F in SWEEP if F % 16 == 0} == {1, 2, 3}
    # bf16 tile pairing Tm = (tiles - 1) & ~1: even and odd tile counts with a partial last tile
    assert any(c["partial_tile"] and c["chain_kernel"] and c["chain_tiles"] % 2 == 0 for c in bf)
    assert any(c["partial_tile"] and c["chain_kernel"] and c["chain_tiles"] % 2 == 1 for c in bf)
    # the fused / group W-statistics kernels with a partly filled chunk
    assert any(c["w_fused"] == 2 and c["tail"] for c in bf)
    # every residue of F mod 4 beside the 16k + 1 shapes
    for Fl in (Fx3, Fbf):
        assert {F % 4 for F in Fl if F % 16 != 1} == {0, 1, 2, 3}
        assert any(F % 16 == 1 and F > 16 for F in Fl)


# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("F", [0, 641])
def test_bin_counts_out_of_range_are_refused(F):
    need_gpu()
    from vaenmf._lib import VaenmfError
    from vaenmf.engine import BatchEngine
    dec = [np.zeros((128, 32), np.float32), np.zeros(128, np.float32), np.zeros((128, 128), np.float32), np.zeros(128, np.float32),
           np.zeros((F, 128), np.float32), np.zeros(F, np.float32)]
    with pytest.raises(VaenmfError, match=r"F=%d out of range \(1\.\.640\)" % F):
        BatchEngine(F, 4, dec, max_frames=16, max_utts=1)


@gpu
@pytest.mark.parametrize("F,K,R", X3_CASES)
def test_split_mode_kernels_against_the_oracle(F, K, R):
    """bf16x3 mode at one F: decoding kernel, Wiener filter and M-step over given samples, a replayed MH chain with the
    default kernel and with the team kernel, then the sample store: stored variances, streaming M-step and streaming
    Wiener filter against the oracle from the chain's own samples."""
    need_gpu()
    es.split_mode_case(es.inputs(F, K, R))


@gpu
@pytest.mark.parametrize("F", RUN_F)
def test_fused_run_at_other_bin_counts(F):
    """BatchEngine.run() (the sample store on by default): finite, bit-identical to the same run stepped through mh_chain /
    m_step_stored / wiener_stored, and the middle utterance alone gives the bits it gives inside the batch."""
    need_gpu()
    es.fused_run_case(es.inputs(F, 10, 12))


@gpu
@pytest.mark.parametrize("F,K,R", BF16_CASES)
def test_bench_mode_kernels_against_the_oracle(F, K, R):
    """bf16 mode at one F: decoding kernel; a replayed chain with every chain kernel the shape has (first-step
    log-acceptances against the oracle, wave against team kernel, four-wavefront against one-wavefront form); the
    stored M-step and Wiener filter against the oracle's from the chain's own samples, with every W-statistics kernel the
    shape has."""
    need_gpu()
    es.bench_mode_case(es.inputs(F, K, R))


@gpu
@pytest.mark.parametrize("variant", ["m2_labels", "nonmf_gains_only"])
@pytest.mark.parametrize("F", [201, 514])
def test_stored_path_variants_against_the_oracle(F, variant):
    """bf16 mode, stored path, the two configurations beside M1 + NMF: M2 (Dy = 1 labels folded into a per-frame layer-1
    bias) and a fixed noise PSD (gains-only M-step, mcem.py:543-578), against the oracle from the chain's own samples."""
    need_gpu()
    K, R = (8, 10) if variant == "m2_labels" else (1, 10)
    c = es.inputs(F, K, R, Dy=1)
    nu = len(COUNTS)
    eng = es.engine(c, "bf16", seeds=[3, 4, 5])
    eng.Z.copy_(torch.from_numpy(c.Z0))
    Vb = None
    if variant == "nonmf_gains_only":
        Vb = (np.random.default_rng(F).random((c.NT, F)) + 0.1).astype(np.float32)
        Vbp = torch.zeros(eng.NT, eng.Fs)
        Vbp[:, :F] = torch.from_numpy(Vb)
        eng.set_noise_psd(Vbp.cuda())
    eng.sample_store(True)
    eng.mh_chain(R, 4, 0.01, call=0)
    Zs = eng.Zs[:, :R].cpu().numpy().copy()
    assert np.abs(Zs - c.Z0[:, None, :]).max() > 0.05
    if variant == "m2_labels":
        oracles = [es.oracle_at(c, eng, u, Zs) for u in range(nu)]
        eng.m_step_stored()
        es.m_step_against(c, eng, oracles, R, eng.cost_from_frames(R), 3e-2, 3e-3, "M2 stored M-step")
        es.wiener_against(c, eng, oracles, eng.wiener_stored(want_masks=True), 1e-2, "M2 stored", absolute=True)
        return
    oracles = []
    for u in range(nu):
        sl = eng.utt_slice(u)
        o = orc.MCEMOracleNoNMF(c.Xs[u], Vb[sl], c.gains[sl], c.Z0[sl], c.ys[u], c.params, 1, orc.NumpyRNG(0))
        o.compute_Vs(Zs[sl]); o.compute_Vs_scaled(); o.compute_Vx()
        o.M_step()
        oracles.append(o)
    eng.m_step_stored()
    cost = eng.cost_from_frames(R)
    assert bool(torch.isfinite(eng.g).all()) and np.all(np.isfinite(cost))
    for u, o in enumerate(oracles):
        sl = eng.utt_slice(u)
        e = (rel_err(eng.g[sl].cpu().numpy(), o.g), abs(cost[u] - o.compute_expected_neg_log_like()) / abs(cost[u]))
        print("noNMF F=%d utt %d: g %.2e cost %.2e" % (F, u, e[0], e[1]))
        assert e[0] < 3e-2 and e[1] < 3e-3
    out = eng.wiener_stored(want_masks=True)
    es.wiener_against(c, eng, oracles, out, 1e-2, "noNMF stored", absolute=True)


# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_reconstructor_at_25_ms():
    """wav -> stft (n_fft 400, F = 201) -> fused EM run in bench mode -> istft on three synthetic utterances."""
    need_gpu()
    from vaenmf.pipeline import Reconstructor
    from vaenmf.synth import synth_utterance
    lens = [16000, 23457, 12001]
    xs = [synth_utterance(10 + i, n_samples=T)[2] for i, T in enumerate(lens)]
    params = orc.xavier_normal_params([201, 32, [128, 128]], seed=0)
    rec = Reconstructor(params, 201, 10, niter=3, fs=16000, wlen_sec=25e-3, precision="bf16", max_frames=1024, max_utts=4)
    wav = torch.from_numpy(np.concatenate(xs).astype(np.float32)).cuda()
    s_hat, n_hat, cost = rec.enhance(wav, lens)
    assert es.query(rec.eng, "Q_MSTEP_PATH") == 1
    assert s_hat.shape[0] == sum(lens) and n_hat.shape[0] == sum(lens) and cost.shape == (3, 3)
    assert torch.isfinite(s_hat).all() and torch.isfinite(n_hat).all() and torch.isfinite(cost).all()
    o = 0
    for T in lens:
        assert float(s_hat[o:o + T].abs().max()) > 0
        o += T


@gpu
def test_mcem_at_25_ms():
    """stft (F = 201) -> MCEM_M1 in bf16x3 mode with replayed draws, against the oracle run on the oracle's STFT with the
    same draws: the bounds of test_mcem_at_the_reference_default_window."""
    need_gpu()
    import vaenmf
    from vaenmf import stft as vstft
    x = (np.load(GOLDEN + "/metrics_dummy_m2.npz")["a_s"] / 32768.0)[:24000]
    F, K, niter = 201, 10, 3
    params = orc.xavier_normal_params([F, 32, [128, 128]], seed=3)
    Xo = orc.stft(x, fs=16000, wlen_sec=25e-3).T                       # (N, F)
    rec = RecordingRNG(7)
    o = orc.MCEMOracle("M1", niter, 10, 10, 10, 10, 0.01)
    o.init_parameters(Xo, params, K, 1e-8, rec)                         # records the draws it takes
    c_ref = o.run()
    vae = vaenmf.VariationalAutoencoder([F, 32, [128, 128]])
    vae.load_state_dict({k: torch.tensor(v) for k, v in params.items()})
    m = vaenmf.MCEM_M1(niter, 10, 10, 10, 10, 0.01, rng="replay", precision="bf16x3")
    X = vstft.stft(x, fs=16000, wlen_sec=25e-3)
    assert X.shape == (F, Xo.shape[0])
    it = iter(rec.draws)
    _r, _n = torch.rand, torch.randn
    torch.rand = lambda *s, **k: torch.tensor(next(it))
    torch.randn = lambda *s, **k: torch.tensor(next(it))
    try:
        m.init_parameters(X=X.T, vae=vae, nmf_rank=K, eps=1e-8, device="cuda:0")
        c = m.run()
    finally:
        torch.rand, torch.randn = _r, _n
    ec, es = float(np.max(np.abs(c - c_ref) / np.abs(c_ref))), nrm_err(m.S_hat, o.S_hat)
    print("MCEM_M1 F=201: cost %.2e S_hat %.2e" % (ec, es))
    assert ec < 2e-4 and es < 2e-3
    s = vstft.istft(m.S_hat, fs=16000, wlen_sec=25e-3, max_len=len(x))
    assert len(s) == len(x) and np.all(np.isfinite(s)) and np.abs(s).max() > 0
