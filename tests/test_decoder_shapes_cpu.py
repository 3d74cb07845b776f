"""No GPU: what tests/test_gpu_decoder_shapes.py reaches, and that its replayed chains are comparable, from the restated
dispatch and the oracle alone; and the bytes em_support.inputs() returns at its defaults."""
import functools

import pytest

import em_support as es
from decoder_shape_cases import BF16_CASES, BF16_K, BF16_R, D, LABEL_CASES, PADDING_CASES, RUN_CASES, X3_CASES, X3_K, X3_R, case_id, chain_cases
from dispatch_model import N_WAVE_TILES, chain_form, shape_class

# sha256 of everything inputs() returns (es.digest) at its defaults, recorded from the parent of the change that gave inputs()
# its z_dim and h_dim arguments
DEFAULT_DIGESTS = {(17, 10, 10, 0): "64f8c5eab608bbc53f3ec41f6105b32d467d5d937f08ce71fa0f254f699134ce",
                   (257, 8, 30, 1): "cddbbb33c79dbe0e26a3189ba5eb6f7afe5f2d8ac85791018eb7bbe1b1949f53",
                   (513, 10, 10, 0): "9cdc4f67afa099af56ba43f803f3adb30e524693aafd1ca06173eec5e115ad5b"}


@pytest.mark.parametrize("F,K,R,Dy", sorted(DEFAULT_DIGESTS))
def test_inputs_at_their_defaults_are_unchanged(F, K, R, Dy):
    c = es.inputs(F, K, R, Dy=Dy)
    assert es.digest(c) == DEFAULT_DIGESTS[(F, K, R, Dy)]
    assert es.digest(es.inputs(F, K, R, Dy=Dy, z_dim=32, h_dim=[128, 128])) == DEFAULT_DIGESTS[(F, K, R, Dy)]
    assert (c.L, c.Lp, c.h_dim) == (32, 32, (128, 128))


@pytest.mark.parametrize("z_dim,h_dim", D)
def test_narrow_inputs_share_the_draws_and_clear_the_padding(z_dim, h_dim):
    """The arrays of a narrow case are the default case's, drawn in the same generator order, with the latent columns
    z_dim..31 cleared; the decoder alone differs."""
    a, b = es.inputs(81, 10, 10), es.inputs(81, 10, 10, z_dim=z_dim, h_dim=h_dim)
    assert (b.L, b.Lp, b.h_dim) == (z_dim, 32, tuple(h_dim))
    for name in ("gains", "uu"):
        assert (getattr(a, name) == getattr(b, name)).all(), name
    for x, y in zip(a.Xs + a.W0 + a.H0, b.Xs + b.W0 + b.H0):
        assert (x == y).all()
    for name in ("Zs", "eps", "Z0"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.shape == y.shape and (x[..., :z_dim] == y[..., :z_dim]).all() and not y[..., z_dim:].any(), name
    assert b.params["decoder.hidden.0.weight"].shape == (128, z_dim)
    assert ("decoder.hidden.1.weight" in b.params) == (len(h_dim) == 2)


@pytest.mark.parametrize("d", range(len(D)))
def test_the_cross_reaches_every_kernel_form_at_every_shape(d):
    """For each decoder shape: every chain form and chain kernel, team geometries 0, 2, 3 and 4 (the helpers run the team
    kernel at every F under VAENMF_TEAM_CHAIN=1), an F with the odd last bin and one without, the W3 lo fragments in LDS
    and from L2, the fused W statistics and the two-kernel path."""
    x3 = [shape_class(F, X3_K, "bf16x3", N_WAVE_TILES, X3_R) for F, dd in X3_CASES if dd == d]
    bf = [shape_class(F, BF16_K, "bf16", N_WAVE_TILES, BF16_R) for F, dd in BF16_CASES if dd == d]
    assert len(x3) == 7 and len(bf) == 6
    forms = {c["chain_form"] for c in x3 + bf}
    # bench_mode_case runs the one-wavefront form too wherever the four-wavefront kernel is the default
    forms |= {chain_form(F, "bf16", N_WAVE_TILES, BF16_K, BF16_R)[0] for F, dd in BF16_CASES if dd == d}
    assert forms == {"wchain<5>", "wchain<5,exact>", "wchain<17>", "wchain<17,exact>", "wchain<33,GT33>", "wchain4<17>", "wchain4<33>", "team"}
    assert {c["chain_kernel"] for c in bf} == {0, 1, 2} and {c["chain_kernel"] for c in x3} == {0, 1}
    for cls in (x3, bf):
        assert {c["geom"] for c in cls} == {0, 2, 3, 4}
    assert {c["geom"] for c in x3 if c["chain_form"] == "team"} == {0, 2, 4}        # geometry 3 runs under VAENMF_TEAM_CHAIN=1
    odd = lambda cases: {F % 16 == 1 and F > 16 for F, dd in cases if dd == d}
    assert odd(X3_CASES) == {True, False} and odd(BF16_CASES) == {True, False}
    assert {c["lo_in_lds"] for c in x3} == {True, False}
    assert {c["w_fused"] for c in bf} == {0, 2} and {c["w_fused"] for c in x3} == {0}
    # the other tests of the module: one fused run and one padding case per chain kernel
    assert sorted(shape_class(F, 10, p, N_WAVE_TILES, 6)["chain_kernel"] for F, p, _ in RUN_CASES) == [0, 1, 2]
    assert all(shape_class(F, X3_K if p == "bf16x3" else BF16_K, p, N_WAVE_TILES, 10)["chain_kernel"] == k for F, p, k in PADDING_CASES)
    assert sorted(k for _, _, k in PADDING_CASES) == [0, 1, 2]
    assert {(dd, Dy == F) for dd, F, _, Dy in LABEL_CASES} == {(0, False), (0, True), (2, False), (2, True)}


@functools.lru_cache(maxsize=None)
def _left_out(F, K, R, d, precision):
    c = es.inputs(F, K, R, z_dim=D[d][0], h_dim=D[d][1])
    return es.cpu_left_out(c, after_m_step=precision == "bf16x3")


@pytest.mark.parametrize("F,K,R,d,precision", chain_cases(), ids=["%s_%s" % (p, case_id(F, d)) for F, K, R, d, p in chain_cases()])
def test_the_oracles_margins_leave_out_few_frames(F, K, R, d, precision):
    """The share of frames with a decision closer than 1e-2 to its threshold, over the six steps of the case's replayed
    chain, is at most 15 %: from the oracle alone, before any GPU run.  (A case over the cap gets an entry in
    em_support.INPUT_SEEDS, never a wider cap.)"""
    lo = _left_out(F, K, R, d, precision)
    print("%s F=%d K=%d %s: frames left out %.1f %%" % (precision, F, K, case_id(F, d), 100 * lo))
    assert lo <= es.LEFT_OUT_CAP
