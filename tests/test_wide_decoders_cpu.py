"""CPU: the wide decoder shapes (z_dim up to 128, a hidden layer of 256 units) without a GPU.

  * the three reference trajectories of tests/golden/make_golden_wide.py replay through both oracles
    (oracle/vaenmf_oracle.py, oracle/vaenmf_torch_cpu.py) within the tolerances tests/test_oracle_golden.py uses for
    the same quantities;
  * vaenmf.engine.decoder_shape, the one place that decides which decoders run and which are wide;
  * the built library exports the entry points of the wide path.
"""
import os

import numpy as np
import pytest

import vaenmf_oracle as orc
from helpers import rel_err, nrm_err
from wide_cases import WIDE_CASES, load_wide_case, SWEEP, RAGGED, sweep_case, cut_short


def run_oracle(name, model):
    z, params, draws, meta = load_wide_case(name)
    nsE, biE, nsW, biW = meta["counts"]
    m = orc.MCEMOracle(model, meta["niter"], nsE, biE, nsW, biW, 0.01, reference_compat=True)
    rng = orc.ReplayRNG(draws)
    m.init_parameters(z["X"], params, meta["K"], 1e-8, rng, y=z["y"] if model == "M2" else None)
    return z, m, rng


@pytest.mark.parametrize("name,model", WIDE_CASES)
def test_fixture_is_a_wide_reference_shape(name, model):
    z, params, draws, meta = load_wide_case(name)
    assert meta["L"] == 128 and meta["N"] == 8 and meta["F"] == 65 and meta["K"] == 4 and meta["niter"] == 3
    hid = [params["decoder.hidden.%d.weight" % i].shape[0] for i in range(orc.n_hidden(params, "decoder"))]
    assert hid == list(reversed([int(v) for v in z["dims_h"]]))      # models.py:133: the decoder runs over reversed(h_dim)
    assert float(z["min_margin"]) >= 1e-3                            # what the existing goldens were selected for
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", name + ".npz")) <= 1 << 20


@pytest.mark.parametrize("name,model", WIDE_CASES)
def test_init_matches_reference(name, model):
    z, m, _ = run_oracle(name, model)
    assert rel_err(m.W, z["W0"]) == 0 and rel_err(m.H, z["H0"]) == 0
    assert np.max(np.abs(m.Z - z["Z0"])) < 2e-5


@pytest.mark.parametrize("name,model", WIDE_CASES)
def test_first_iteration_steps(name, model):
    z, m, rng = run_oracle(name, model)
    trace = []
    ns, bi = m.e_step_counts()
    Zs = m.sample_posterior(m.Z, ns, bi, trace=trace)
    n1 = int(z["E1_nacc"])
    assert len(trace) == n1 == ns + bi
    acc = np.stack([t["acc"] for t in trace])
    assert np.max(np.abs(acc - z["acc"][:n1])) < 2e-3 * max(1.0, np.abs(z["acc"][:n1]).max() * 1e-2)
    m.Z = Zs[:, -1, :].T.copy()
    m.compute_Vs(Zs); m.compute_Vs_scaled(); m.compute_Vx()
    assert np.max(np.abs(m.Z - z["E1_Z"])) < 1e-5
    assert rel_err(m.Vs, z["E1_Vs"]) < 2e-5
    assert rel_err(m.Vx, z["E1_Vx"]) < 2e-5
    m.M_step()
    for k, v in (("M1_W", m.W), ("M1_H", m.H), ("M1_g", m.g), ("M1_Vb", m.Vb), ("M1_Vx", m.Vx)):
        assert rel_err(v, z[k]) < 5e-5, k


@pytest.mark.parametrize("name,model", WIDE_CASES)
def test_full_run(name, model):
    z, m, rng = run_oracle(name, model)
    cost = m.run()
    assert rng.pos == len(rng.draws)
    assert np.max(np.abs(cost - z["cost"]) / np.abs(z["cost"])) < 2e-5
    assert tuple(m.Vs.shape) == tuple(z["Vs_shape"])
    for k, v in (("W", m.W), ("H", m.H), ("g", m.g)):
        assert rel_err(v, z[k]) < 2e-4, k
    assert np.max(np.abs(m.Z - z["Z"])) < 2e-5
    assert rel_err(m.WFs, z["WFs"]) < 2e-4 and rel_err(m.WFn, z["WFn"]) < 2e-4
    assert nrm_err(m.S_hat, z["S_hat"]) < 1e-5 and nrm_err(m.N_hat, z["N_hat"]) < 1e-5


@pytest.mark.parametrize("name,model", WIDE_CASES)
def test_torch_cpu_restatement_full_run(name, model):
    import torch
    import vaenmf_torch_cpu as tc
    torch.set_num_threads(1)
    z, params, draws, meta = load_wide_case(name)
    nsE, biE, nsW, biW = meta["counts"]
    m = tc.TorchMCEM(model, meta["niter"], nsE, biE, nsW, biW, 0.01, reference_compat=True)
    rng = tc.ReplayDraws(draws)
    m.init_parameters(z["X"], params, meta["K"], 1e-8, rng, y=z["y"] if model == "M2" else None)
    assert np.max(np.abs(m.Z.numpy() - z["Z0"])) < 2e-5
    cost = m.run()
    assert rng.pos == len(rng.draws)
    assert np.max(np.abs(cost - z["cost"]) / np.abs(z["cost"])) < 2e-5
    for k, v in (("W", m.W), ("H", m.H), ("g", m.g)):
        assert rel_err(v.numpy(), z[k]) < 2e-4, k
    assert nrm_err(m.S_hat, z["S_hat"]) < 1e-5 and nrm_err(m.N_hat, z["N_hat"]) < 1e-5


def test_sweep_seeds_leave_few_frames_cut_short():
    """The GPU sweep (tests/test_gpu_wide_decoders.py) compares a frame up to the first decision the oracle itself makes
    within 5e-4 of its threshold: with the committed seeds at most 15 % of a case's frames are cut short, and every value
    the sweep has to cover appears (F = 640 with the widest decoder, the ragged batch, ranks 1, 8 and 32)."""
    for i, (F, L, hdim, counts, K, model) in enumerate(SWEEP):
        n_cut, n_all = cut_short(sweep_case(i)[3])
        assert n_all == sum(counts) and n_cut <= 0.15 * n_all, (i, n_cut, n_all)
    assert {c[0] for c in SWEEP} == {1, 17, 65, 130, 257, 640} and {c[4] for c in SWEEP} == {1, 8, 32}
    assert {(c[1], tuple(c[2])) for c in SWEEP} >= {(128, (256, 128)), (128, (128,)), (64, (256, 128)), (32, (256, 128))}
    assert (640, 128, [256, 128], RAGGED) in [c[:4] for c in SWEEP] and RAGGED == [1, 2, 19, 16, 1]


class _Shape:
    def __init__(self, *shape):
        self.shape = shape


def _dec(L, hidden, F=65, Dy=0):
    """Decoder layer list (shapes only) with the given widths of its own hidden layers."""
    out, inn = [], L + Dy
    for h in hidden:
        out += [_Shape(h, inn), _Shape(h)]
        inn = h
    return out + [_Shape(F, inn), _Shape(F)]


def test_decoder_shape_classifies_every_accepted_shape():
    """(L, Lp, H1, H2, wide): narrow plans keep 32 latent columns and the kernels they run today; L > 32 or a 256-wide
    layer is wide, 128 columns.  hidden = the decoder's own layers, i.e. reversed(h_dim) of the reference's model."""
    from vaenmf.engine import decoder_shape
    for L in (16, 32, 64, 128):
        for hidden in ([128], [128, 128], [128, 256], [256, 128]):
            for Dy in (0, 1):
                wide = L > 32 or 256 in hidden
                assert decoder_shape(_dec(L, hidden, Dy=Dy), L) == (L, 128 if wide else 32, hidden[0], hidden[1] if len(hidden) > 1 else 0, wide)
    import vaenmf
    vae = vaenmf.VariationalAutoencoder([65, 128, [256, 128]])          # the reference's constructor arguments
    from vaenmf.engine import decoder_params_from_state
    assert decoder_shape(decoder_params_from_state(vae.state_dict()), vae.z_dim) == (128, 128, 128, 256, True)
    vae = vaenmf.VariationalAutoencoder([65, 32, [128, 128]])
    assert decoder_shape(decoder_params_from_state(vae.state_dict()), vae.z_dim) == (32, 32, 128, 128, False)


def test_decoder_shape_refuses_everything_else():
    from vaenmf.engine import decoder_shape
    for L, hidden in ((256, [128, 128]), (128, [512, 128]), (128, [128, 128, 128]), (16, [256]), (48, [128]), (128, [256, 256])):
        with pytest.raises(NotImplementedError) as e:
            decoder_shape(_dec(L, hidden), L)
        assert "128" in str(e.value) and "256" in str(e.value)         # the message names the accepted set
    with pytest.raises(NotImplementedError):
        decoder_shape(_dec(32, [128, 128])[:2] + [_Shape(128, 64), _Shape(128)] + _dec(32, [128, 128])[4:], 32)    # W2 does not fit W1


def test_library_exports_the_wide_entry_points():
    from vaenmf import _lib
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build)"
    blob = open(_lib.LIB_PATH, "rb").read()                            # (the dynamic string table holds the names)
    for sym in (b"vn_launch_widechain", b"vn_launch_wide_rng_fill", b"widechain_kernel", b"vaenmf_m_step_stored", b"vaenmf_wiener_stored"):
        assert sym in blob, sym
    assert _lib.Q_LP == 11 and "wide.hip" in open(os.path.join(os.path.dirname(__file__), "..", "__graft_entry__.py")).read()
