"""The EM kernels at a trained decoder's value range and at audio scales, against float64.

Every other test builds its decoder with Xavier weights: log-variances inside [-1.9, 2.4], no tanh unit near saturation,
log-acceptances of at most a few nats, a spectrogram of order 1.  tests/value_cases.py holds decoders sharpened to a
trained model's regime ("trained", "extreme"; "xavier" is the control), data drawn from the model itself, and amplitudes
(powers of two) that move the products the kernels form -- Vx of two bins, Vx of two sample rows, |X|^2 times Vx -- to
2^10 and to 2^2..2^6 inside the edges of the normal float32 range.  tests/test_value_range_cpu.py pins the cases.

Each case runs once on the device (_run): the decoding kernels from given samples, a replayed chain with the store on, a
chain with the device generator and a burn-in, the stored M-step, cost and Wiener filter, the gains-only M-step with a
fixed noise PSD.  Every reference is float64.

Decoder and store.  |log Vs(device) - log Vs(float64)| against two bounds evaluated in float64 from the inputs alone
(value_cases.decoder64_full): the worst-case first-order forward error -- per layer gamma (|W| |x| + |b|), through
(1 - h^2), plus the 2e-7 of fast_tanh, times 2 for second-order terms and fp32 accumulation; gamma = 2^-15 (bf16x3) or
2^-8 (bf16), a bf16 store row 2^-9 more -- and the root-sum-square figure of the same model times 8.  The second is the
one with teeth: tests/test_value_range_cpu.py shows that a bf16x3 decoder which drops a cross term stays inside the first.

Chain.  The float64 chain is evaluated along the device's own decisions (read off its samples: no burn-in), so every step
of every frame is compared and none is left out; the margin rule of the other sweeps would leave out 20 to 100 % here (see
tests/test_value_range_cpu.py).  |acc(device) - acc(float64)| against the decoder bound carried through s |1 - X2 / Vx|
per bin for both states plus 16 2^-24 M (M: the sum of the absolute terms), in the worst-case and the root-sum-square
form; a device decision may differ from the float64 one only where |log u - acc| is inside the bound.

M-step, cost, Wiener filter: m_step64 / gains_step64 / wiener64 and the max(floor, 16 e32) rule of
tests/test_gpu_rank_and_samples.py on the device's own variances, stored, decoding and gains-only forms.

Scale invariance.  At every other amplitude against amplitude 1: the decoder does not see the amplitude, so the two runs
hold the same variances and their log-acceptances may differ by the fp32 terms 16 2^-24 (M + M') alone -- sharper than the
sum of the two runs' bounds; masks, S_hat / amp, W, H / amp^2, g / amp^2 within the sum of the two runs' bounds.

Isolation.  A batch with an utterance that has one exactly silent frame and an utterance of zeros: the other utterances
are bit-equal to the same utterances run without the two, through vaenmf_em_run (launch by launch and as a graph) and the
stepwise stored calls.

Measured on an MI355X.  Per case: the largest log-variance error over eng.decode and the stored rows of both chains, as
it is, over its worst-case bound and over its root-sum-square bound; the largest |log-acceptance|, the largest error of one,
the largest ratios to the two bounds, and (in brackets) how many of the 420 decisions differ from float64's -- each of
them inside its bound; of the M-step, cost and Wiener figures of the stored, decoding and gains-only forms the one nearest
its bound (always the cost); against amplitude 1, the largest difference of a log-acceptance over the fp32 terms (the masks,
S_hat / amp, N_hat / amp, W, H / amp^2 and g / amp^2 are bit-equal in all 18 cases, the decisions and samples identical).
  case                            log-variance: error,       log-acceptance: largest, error,    M-step / cost / Wiener:    amplitude: acc over
                                  / worst-case, / rss bound  / worst-case, / rss bound          largest error / bound      the fp32 terms
  f65-bf16x3-xavier-one           1.6e-05 0.0015 0.080      1.86     1.2e-04 0.0001 0.028 (0)   gains_only cost  3.1e-08/1.0e-06
  f65-bf16x3-trained-one          3.3e-04 0.0025 0.071      334      3.8e-02 0.0004 0.023 (0)   decoding cost    6.1e-08/1.0e-06
  f65-bf16x3-extreme-one          6.8e-04 0.0032 0.081      4.65e+05 1.8e+02 0.0012 0.029 (0)   decoding cost    2.9e-07/1.0e-06
  f65-bf16x3-trained-small        3.3e-04 0.0025 0.071      334      3.8e-02 0.0004 0.023 (0)   decoding cost    5.7e-08/1.0e-06  0.025
  f65-bf16x3-trained-large        3.3e-04 0.0025 0.071      334      3.8e-02 0.0004 0.023 (0)   gains_only cost  5.3e-08/1.0e-06  0.019
  f65-bf16-xavier-one             1.1e-02 0.0069 0.367      1.86     4.7e-02 0.0004 0.125 (2)   gains_only cost  2.4e-08/1.0e-06
  f65-bf16-trained-one            1.6e-01 0.0109 0.299      334      2.3e+01 0.0019 0.104 (25)   stored cost      6.3e-08/1.0e-06
  f65-bf16-extreme-one            4.1e-01 0.0133 0.328      4.65e+05 3.3e+04 0.0050 0.130 (29)   decoding cost    2.7e-07/1.0e-06
  f65-bf16-trained-small          1.6e-01 0.0109 0.299      334      2.3e+01 0.0019 0.104 (25)   gains_only cost  5.6e-08/1.0e-06  0.024
  f65-bf16-trained-large          1.6e-01 0.0109 0.299      334      2.3e+01 0.0019 0.104 (25)   gains_only cost  4.1e-08/1.0e-06  0.024
  f257-bf16-xavier-one            8.7e-03 0.0098 0.418      3.26     8.4e-02 0.0002 0.129 (3)   stored cost      1.8e-08/1.0e-06
  f257-bf16-trained-one           1.2e-01 0.0124 0.280      37.7     8.8e+00 0.0011 0.118 (30)   stored cost      6.0e-08/1.0e-06
  f257-bf16-extreme-one           4.0e-01 0.0156 0.384      4.46e+03 4.9e+02 0.0022 0.126 (36)   gains_only cost  7.6e-08/1.0e-06
  f257-bf16-trained-small         1.2e-01 0.0124 0.280      37.7     8.8e+00 0.0011 0.118 (30)   gains_only cost  5.4e-08/1.0e-06  0.021
  f257-bf16-trained-large         1.2e-01 0.0124 0.280      37.7     8.8e+00 0.0011 0.118 (30)   stored cost      4.2e-08/1.0e-06  0.009
  f273-bf16x3-xavier-one          1.4e-05 0.0021 0.100      3.25     1.9e-04 0.0001 0.027 (0)   gains_only cost  3.4e-08/1.0e-06
  f273-bf16x3-trained-one         2.4e-04 0.0031 0.068      25.9     1.4e-02 0.0002 0.029 (0)   gains_only cost  6.7e-08/1.0e-06
  f273-bf16x3-extreme-one         8.7e-04 0.0033 0.094      1.28e+03 4.9e-01 0.0006 0.033 (0)   decoding cost    7.8e-08/1.0e-06
  f273-bf16x3-trained-small       2.4e-04 0.0031 0.068      25.9     1.5e-02 0.0002 0.029 (0)   stored cost      5.9e-08/1.0e-06  0.011
  f273-bf16x3-trained-large       2.4e-04 0.0031 0.068      25.9     1.4e-02 0.0002 0.029 (0)   gains_only cost  4.3e-08/1.0e-06  0.010
  f65w-bf16x3-xavier-one          2.0e-05 0.0006 0.078      5.11     1.2e-04 0.0000 0.023 (0)   stored cost      2.7e-08/1.0e-06
  f65w-bf16x3-trained-one         3.2e-04 0.0011 0.071      149      1.2e-01 0.0003 0.031 (0)   stored cost      7.6e-08/1.0e-06
  f65w-bf16x3-extreme-one         7.9e-04 0.0014 0.078      1.48e+05 1.5e+02 0.0005 0.033 (0)   gains_only cost  4.7e-07/2.4e-06
  f65w-bf16x3-trained-small       3.2e-04 0.0011 0.071      149      1.2e-01 0.0003 0.031 (0)   gains_only cost  6.1e-08/1.0e-06  0.016
  f65w-bf16x3-trained-large       3.2e-04 0.0011 0.071      149      1.2e-01 0.0003 0.031 (0)   stored cost      4.8e-08/1.0e-06  0.021
  f65w-bf16-xavier-one            1.2e-02 0.0030 0.395      5.11     5.9e-02 0.0002 0.111 (3)   stored cost      2.7e-08/1.0e-06
  f65w-bf16-trained-one           1.7e-01 0.0053 0.287      149      2.5e+01 0.0008 0.107 (28)   gains_only cost  6.6e-08/1.0e-06
  f65w-bf16-extreme-one           3.6e-01 0.0068 0.336      1.48e+05 4.5e+04 0.0015 0.140 (30)   gains_only cost  6.0e-07/3.7e-06
  f65w-bf16-trained-small         1.7e-01 0.0053 0.287      149      2.5e+01 0.0008 0.107 (28)   stored cost      5.6e-08/1.0e-06  0.015
  f65w-bf16-trained-large         1.7e-01 0.0053 0.287      149      2.5e+01 0.0008 0.107 (28)   stored cost      5.5e-08/1.0e-06  0.015
  f65-bf16x3-trained-edge_small   3.3e-04 0.0025 0.071      334      3.8e-02 0.0004 0.023 (0)   stored cost      8.0e-08/1.0e-06  0.024
  f65-bf16x3-trained-edge_large   3.3e-04 0.0025 0.071      334      3.8e-02 0.0004 0.023 (0)   gains_only cost  4.8e-08/1.0e-06  0.023
  f65-bf16-trained-edge_small     1.6e-01 0.0109 0.299      334      2.3e+01 0.0019 0.104 (25)   stored cost      5.6e-08/1.0e-06  0.023
  f65-bf16-trained-edge_large     1.6e-01 0.0109 0.299      334      2.3e+01 0.0019 0.104 (25)   decoding cost    4.0e-08/1.0e-06  0.019
  f257-bf16-trained-edge_small    1.2e-01 0.0124 0.280      37.7     8.8e+00 0.0011 0.118 (30)   gains_only cost  5.9e-08/1.0e-06  0.019
  f257-bf16-trained-edge_large    1.2e-01 0.0124 0.280      37.7     8.8e+00 0.0011 0.118 (30)   gains_only cost  4.4e-08/1.0e-06  0.014
  f65-bf16x3-trained-one-m2       2.8e-04 0.0023 0.073      52       3.0e-02 0.0006 0.030 (0)   stored cost      7.2e-08/1.0e-06
  f65-bf16-trained-one-m2         1.4e-01 0.0107 0.280      52       4.3e+00 0.0012 0.100 (24)   gains_only cost  7.8e-08/1.0e-06
No bound is met by less than a factor 2: the nearest are the bf16 decoder at 0.42 of its root-sum-square bound (0.016 of the
worst-case one) and the cost at 0.29.  Over all cases: masks <= 2.7e-7, S_hat 8.9e-8, N_hat 1.4e-7, g 2.0e-7, W 5.0e-7,
H 3.2e-7, each against 2e-5.  Every case and the four isolation cases run in 5 s together.

Scratch edits, each built once and run once against these tests:
  * mma3<true> without its w_lo a_hi term (2^-9 per product), run on the "xavier" and "trained" cases at amplitude 1: all
    seven bf16x3 decoder / store tests fail, at "xavier" too (the bf16 ones, which do not use the term, pass) --
    log-variances 22 to 27 root-sum-square bounds off, yet only 0.22 to 0.98 of the worst-case bound, as the float64
    simulation of tests/test_value_range_cpu.py predicts; all seven bf16x3 chain tests fail, more narrowly: 1.2 to 2.3
    root-sum-square bounds (the two states of a step share most of the fault), 0.002 to 0.07 of the worst-case bound.
    Without the root-sum-square bounds the edit would have failed nothing.
  * the mask of hg_stream_kernel's extra-bin term moved inside the reciprocal (rcp(0) in the lanes without a row): g and
    the cost are NaN in every frame; all four isolation cases fail (at the finiteness of the sound utterances, before the
    bit comparison) and so does every M-step test.  That mask works inside one frame; the edit says nothing about one
    utterance reaching another, which the bit comparison covers.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import value_cases as vc
import em_support as es
from em_support import make_engine
from helpers import need_gpu

pytestmark = pytest.mark.gpu

COUNTS = vc.COUNTS
BURNIN = 4                     # of the chain with the device generator
Z_STEP_ULP = 2.0 ** -21        # one step of the walk: an fma against a rounded product and sum, one ulp of |z| < 8


def _pad(a, Lp):
    """(..., L) -> (..., Lp), zero beyond L."""
    if a.shape[-1] == Lp:
        return np.ascontiguousarray(a)
    out = np.zeros(a.shape[:-1] + (Lp,), np.float32)
    out[..., :a.shape[-1]] = a
    return out


def _noise_psd(c):
    """The fixed noise PSD of the gains-only form: the case's own noise floor."""
    return vc.noise_floor(c).astype(np.float32)


def _logvar_errors(c, prec, Zs, V, bf16_rows):
    """Largest |log V - log-variance(float64)| over its worst-case bound and over its root-sum-square bound, and the
    largest error itself.  Zs (NT, R, L), V (NT, R, F) of the device."""
    assert np.all(np.isfinite(V)) and np.all(V > 0)
    full = vc.decoder64_full(c.params, vc._zin_rows(c, Zs), vc.GAMMA[prec])
    err = np.abs(np.log(V.astype(np.float64)).reshape(full.a.shape) - full.a)
    return (float(np.max(err / vc.logvar_bound(full.da, bf16_rows))), float(np.max(err / vc.logvar_bound_rss(full.sigma, bf16_rows))),
            float(np.max(err)))


def _m_step_errors(c, eng, variant, Vb, V, got_of):
    """Per quantity the largest error over the utterances against the float64 formulas fed with the device's variances V,
    the bound it is held to, and what exceeds it."""
    err, bound, bad = {}, {}, []
    for u, o in enumerate(es.oracles_from(c, eng, variant, Vb, V)):
        with np.errstate(all="ignore"):
            ref, o32 = es.reference(o, variant)
        got = got_of(u)
        e, b = es.errors(got, ref), es.bounds(es.errors({k: o32[k] for k in got}, ref))
        bad += [(u, k, e[k], b[k]) for k in es.violations(e, b)]
        for k in e:
            if k not in err or not e[k] / b[k] <= err[k] / bound[k]:
                err[k], bound[k] = e[k], b[k]
    return SimpleNamespace(err=err, bound=bound, bad=bad)


def _merge(a, b):
    a.bad += b.bad
    for k in b.err:
        if k not in a.err or not b.err[k] / b.bound[k] <= a.err[k] / a.bound[k]:
            a.err[k], a.bound[k] = b.err[k], b.bound[k]
    return a


@functools.lru_cache(maxsize=None)
def _run(case):
    """Everything the device computes for one case, as numpy (once per process)."""
    shape, prec, level, amp, dy = case
    c = vc.get_case(shape, level, amp, dy)
    wide = shape == "f65w"
    F, K, R, L, NT = c.F, c.K, c.R, c.L, c.NT
    eng = make_engine(c.params, F, K, COUNTS, Rcap=R, precision=prec, seeds=[3, 4, 5])
    assert eng.wide == wide
    dev = eng.device
    r = SimpleNamespace(case=case, c=c)

    def reset():
        eng.init_nmf(c.W0, c.H0)
        eng.g.copy_(torch.from_numpy(c.gains))
        eng.Z.copy_(torch.from_numpy(_pad(c.Z0, eng.Lp)))

    eng.set_spectrogram(c.Xs)
    if dy:
        eng.set_labels(torch.from_numpy(c.y_all))
    reset()
    states = lambda: {k: getattr(eng, k).cpu().numpy().copy() for k in ("W", "Ht", "g")}

    # 1. the decoding kernels from the given samples (a wide engine has the stored forms only)
    r.decoding = None
    if not wide:
        eng.Zs.copy_(torch.from_numpy(c.Zs))
        V = eng.decode(R).cpu().numpy()
        assert np.all(V[:, :, F:] == 0)
        r.decode = _logvar_errors(c, prec, c.Zs, V[:, :, :F], False)
        out = eng.wiener(R, want_masks=True)
        m = _m_step_errors(c, eng, "M1", None, V[:, :, :F], lambda u: es.device_wiener(c, eng, u, out))
        r.dec_wiener = [es.device_wiener(c, eng, u, out) for u in range(len(COUNTS))]
        es.padding_is_zero(eng, out[2], out[3], out[0].abs().sum(-1), out[1].abs().sum(-1))
        with np.errstate(all="ignore"):                                    # (the references before the M-step moves the state)
            refs = [es.reference(o, "M1") for o in es.oracles_from(c, eng, "M1", None, V[:, :, :F])]
        eng.m_step(R)
        cost = eng.cost_from_frames(R)
        mm = SimpleNamespace(err={}, bound={}, bad=[])
        for u, (ref, o32) in enumerate(refs):
            got = es.device_m_step(c, eng, u, cost, "M1")
            e, b = es.errors(got, ref), es.bounds(es.errors({k: o32[k] for k in got}, ref))
            _merge(mm, SimpleNamespace(err=e, bound=b, bad=[(u, k, e[k], b[k]) for k in es.violations(e, b)]))
        r.decoding = _merge(m, mm)
        r.dec_state = states()
        es.padding_is_zero(eng)
        reset()

    # 2. the replayed chain, store on: log-acceptances, samples, stored rows
    eng.sample_store(True)
    eps = torch.from_numpy(_pad(c.eps, eng.Lp)).to(dev)
    acc = eng.mh_chain(c.ns, c.S_steps - c.ns, c.var_rw, eps=eps, u=torch.from_numpy(c.uu).to(dev), want_acc=True)
    r.chain_kernel = es.query(eng, "Q_CHAIN_KERNEL")
    r.acc = acc.cpu().numpy().astype(np.float64)
    r.Zs = eng.Zs[:, :c.ns, :L].cpu().numpy().copy()
    r.Z = eng.Z[:, :L].cpu().numpy().copy()
    assert L == eng.Lp or float(eng.Zs[:, :c.ns, L:].abs().max()) == 0.0
    rows = eng.stored_variances(c.ns).cpu().numpy()
    assert np.all(rows[:, :, F:] == 0)
    r.rows_replay = _logvar_errors(c, prec, r.Zs, rows[:, :, :F], prec == "bf16")

    # 3. a chain with the device generator and a burn-in; the stored M-step, cost and Wiener filter from its rows
    reset()
    eng.mh_chain(R, BURNIN, c.var_rw, call=1)
    assert es.query(eng, "Q_CHAIN_KERNEL") == r.chain_kernel
    Zc = eng.Zs[:, :R, :L].cpu().numpy().copy()
    r.moved = float(np.abs(Zc - c.Z0[:, None, :]).max())
    rows = eng.stored_variances(R).cpu().numpy()
    r.rows_device = _logvar_errors(c, prec, Zc, rows[:, :, :F], prec == "bf16")
    V = rows[:, :, :F]
    out = eng.wiener_stored(want_masks=True)
    m = _m_step_errors(c, eng, "M1", None, V, lambda u: es.device_wiener(c, eng, u, out))
    r.st_wiener = [es.device_wiener(c, eng, u, out) for u in range(len(COUNTS))]
    es.padding_is_zero(eng, out[2], out[3], out[0].abs().sum(-1), out[1].abs().sum(-1))
    with np.errstate(all="ignore"):
        refs = [es.reference(o, "M1") for o in es.oracles_from(c, eng, "M1", None, V)]
    eng.m_step_stored()
    r.w_fused = es.query(eng, "Q_W_FUSED")
    cost = eng.cost_from_frames(R)
    for u, (ref, o32) in enumerate(refs):
        got = es.device_m_step(c, eng, u, cost, "M1")
        e, b = es.errors(got, ref), es.bounds(es.errors({k: o32[k] for k in got}, ref))
        _merge(m, SimpleNamespace(err=e, bound=b, bad=[(u, k, e[k], b[k]) for k in es.violations(e, b)]))
    r.stored = m
    r.st_state = states()
    r.st_samples = Zc
    es.padding_is_zero(eng)

    # 4. the gains-only M-step with a fixed noise PSD, from the same rows
    Vb = _noise_psd(c)
    Vbp = torch.zeros(eng.NT, eng.Fs)
    Vbp[:, :F] = torch.from_numpy(Vb)
    eng.set_noise_psd(Vbp.to(dev))
    eng.g.copy_(torch.from_numpy(c.gains))
    with np.errstate(all="ignore"):
        refs = [es.reference(o, "noNMF") for o in es.oracles_from(c, eng, "noNMF", Vb, V)]
    eng.m_step_stored()
    cost = eng.cost_from_frames(R)
    g = SimpleNamespace(err={}, bound={}, bad=[])
    for u, (ref, o32) in enumerate(refs):
        got = es.device_m_step(c, eng, u, cost, "noNMF")
        e, b = es.errors(got, {k: ref[k] for k in got}), es.bounds(es.errors({k: o32[k] for k in got}, ref))
        _merge(g, SimpleNamespace(err=e, bound=b, bad=[(u, k, e[k], b[k]) for k in es.violations(e, b)]))
    r.gains_only = g
    eng.set_noise_psd(None)
    eng.sample_store(False)
    eng.close()
    return r


def _device_decisions(c, r):
    """The decisions of the replayed chain, read off its samples (no burn-in: sample m is the state after step m)."""
    assert c.ns == c.S_steps
    prev = np.concatenate([c.Z0[:, None, :], r.Zs[:, :-1]], 1)
    return np.ascontiguousarray(np.any(r.Zs != prev, -1).T)                # (S, NT)


IDS = [vc.case_id(case) for case in vc.CASES]


@pytest.mark.parametrize("case", vc.CASES, ids=IDS)
def test_decoder_and_store_against_float64(case):
    """eng.decode of given samples, and the stored rows after the replayed chain and after a chain with the device
    generator and a burn-in, in the mode's store format: log-variances within the worst-case and the root-sum-square
    forward error bound of the float64 decoder."""
    need_gpu()
    r = _run(case)
    for name in ("decode", "rows_replay", "rows_device"):
        if getattr(r, name, None) is None:
            continue
        w, s, e = getattr(r, name)
        print("VALUE %s %s: log-variance error %.2e, %.4f of the worst-case bound, %.3f of the rss bound" % (vc.case_id(case), name, e, w, s))
        assert w <= 1 and s <= 1, (name, w, s, e)
    assert r.moved > 0.01                                                  # (the device chain left its start)


@pytest.mark.parametrize("case", vc.CASES, ids=IDS)
def test_chain_against_float64_along_the_device_decisions(case):
    """The replayed chain: the kernel the shape is meant to reach; every log-acceptance of every frame and step within its
    bound of the float64 value for the same states; the decisions equal to the float64 ones wherever the margin exceeds
    the bound; the samples those decisions imply; both accepted and rejected steps."""
    need_gpu()
    shape, prec, level, amp, dy = case
    r = _run(case)
    c = r.c
    assert r.chain_kernel == vc.SHAPES[shape]["kernel"][prec]
    assert np.all(np.isfinite(r.acc))
    dec = _device_decisions(c, r)
    assert dec.any() and not dec.all()
    ch = vc.chain64(c, vc.GAMMA[prec], decisions=dec)
    err = np.abs(r.acc - ch.acc)
    differ = dec != ch.decision
    print("VALUE %s chain: |acc| up to %.3g, error %.2e, %.4f of the worst-case bound, %.3f of the rss bound (step 0: %.3f); acceptance %.2f; "
          "%d of %d decisions differ from float64, none left out"
          % (vc.case_id(case), np.abs(ch.acc).max(), err.max(), np.max(err / ch.bound), np.max(err / ch.bound_rss), np.max(err[0] / ch.bound_rss[0]),
             dec.mean(), differ.sum(), differ.size))
    assert np.all(err <= ch.bound) and np.all(err <= ch.bound_rss), (float(np.max(err / ch.bound)), float(np.max(err / ch.bound_rss)))
    assert np.all(ch.margin[differ] <= ch.bound_rss[differ])
    assert differ.mean() <= 0.15
    ez = float(np.max(np.abs(r.Zs - ch.Zs))), float(np.max(np.abs(r.Z - ch.Z)))
    assert max(ez) <= c.S_steps * Z_STEP_ULP, ez


@pytest.mark.parametrize("case", vc.CASES, ids=IDS)
def test_m_step_cost_and_wiener_against_float64(case):
    """Stored, decoding and gains-only forms on the device's own variances: max(floor, 16 e32) of the float64 formulas."""
    need_gpu()
    shape, prec, level, amp, dy = case
    r = _run(case)
    if shape == "f257":
        assert r.w_fused == 2                                              # the fused W statistics (group form) at rank 8, R = 10
    bad = []
    for name in ("stored", "decoding", "gains_only"):
        m = getattr(r, name)
        if m is None:
            continue
        print("VALUE %s %s: " % (vc.case_id(case), name) + " ".join("%s %.1e/%.1e" % (k, m.err[k], m.bound[k]) for k in m.err))
        bad += [(name,) + b for b in m.bad]
    assert not bad, bad


def _scaled_back(d, amp):
    """A run's results divided by what the amplitude contributes."""
    a2 = amp * amp
    out = {}
    for k, v in d.items():
        out[k] = v / amp if k in ("S_hat", "N_hat") else (v / a2 if k in ("H", "g") else v)
    return out


@pytest.mark.parametrize("case", [case for case in vc.CASES if case[3] != "one"], ids=[i for i, case in zip(IDS, vc.CASES) if case[3] != "one"])
def test_results_do_not_depend_on_the_amplitude(case):
    """Against the same case at amplitude 1: the same decisions and samples; log-acceptances within the fp32 terms of the
    two runs; masks, S_hat / amp, N_hat / amp, W, H / amp^2 and g / amp^2 within the sum of the two runs' bounds."""
    need_gpu()
    shape, prec, level, amp, dy = case
    a, b = _run(case), _run((shape, prec, level, "one", dy))
    ca = a.c
    da, db = _device_decisions(ca, a), _device_decisions(b.c, b)
    cha, chb = vc.chain64(ca, vc.GAMMA[prec], decisions=da), vc.chain64(b.c, vc.GAMMA[prec], decisions=db)
    same = np.concatenate([np.ones((1, ca.NT), bool), np.cumprod(da == db, 0).astype(bool)[:-1]])      # the same state so far
    err = np.abs(a.acc - b.acc)
    tol = cha.bound_fp32 + chb.bound_fp32
    print("VALUE %s scale: amplitude 2^%d, acc against amplitude 1 %.2e, %.3f of the fp32 terms; %d decisions differ"
          % (vc.case_id(case), np.log2(ca.amp), err[same].max(), np.max(err[same] / tol[same]), int((da != db).sum())))
    assert np.all(err[same] <= tol[same])
    split = same & (da != db)                                              # the first step at which the two runs part
    assert np.all(np.minimum(cha.margin, chb.margin)[split] <= tol[split])
    # the M-step and the Wiener filter from the given samples (a wide engine: from the store, when the chains agree)
    if shape == "f65w":
        assert np.array_equal(a.st_samples, b.st_samples)
        sa, sb, wa, wb, ba, bb = a.st_state, b.st_state, a.st_wiener, b.st_wiener, a.stored.bound, b.stored.bound
    else:
        sa, sb, wa, wb, ba, bb = a.dec_state, b.dec_state, a.dec_wiener, b.dec_wiener, a.decoding.bound, b.decoding.bound
    off, F, K = ca.off, ca.F, ca.K
    worst = {}
    for u in range(len(COUNTS)):
        sl = slice(off[u], off[u + 1])
        ga = dict(wa[u], W=sa["W"][u, :F, :K], H=sa["Ht"][sl, :K].T, g=sa["g"][sl])
        gb = dict(wb[u], W=sb["W"][u, :F, :K], H=sb["Ht"][sl, :K].T, g=sb["g"][sl])
        e = es.errors(_scaled_back(ga, ca.amp), {k: np.asarray(v, np.complex128 if np.iscomplexobj(v) else np.float64) for k, v in gb.items()})
        for k in e:
            worst[k] = max(worst.get(k, 0.0), e[k] / (ba[k] + bb[k]))
    print("VALUE %s scale: against amplitude 1, over the sum of the two bounds: " % vc.case_id(case) + " ".join("%s %.3f" % kv for kv in worst.items()))
    assert max(worst.values()) <= 1, worst


# ---------------------------------------------------------------------------------------------------------------------
ISOLATION = [("f65", "bf16x3"), ("f257", "bf16"), ("f273", "bf16x3"), ("f65w", "bf16")]


@pytest.mark.parametrize("shape,prec", ISOLATION)
def test_a_degenerate_utterance_does_not_reach_its_neighbours(shape, prec):
    """Utterances [sound, one silent frame, sound, all zeros, sound] against [sound, sound, sound] with the same seeds:
    S_hat, N_hat, W, H, g and the cost of the sound ones bit-equal, through vaenmf_em_run launch by launch and as a graph
    and through the stepwise stored calls; the two degenerate utterances end non-finite, as in the reference
    (tests/test_value_range_cpu.py)."""
    need_gpu()
    c = vc.get_case(shape, "trained", "one")
    F, K, L = c.F, c.K, c.L
    # (source utterance of the case, frames, kind)
    spec = [(0, 21, "sound"), (1, 12, "frame"), (2, 9, "sound"), (1, 16, "zeros"), (1, 40, "sound")]
    seeds = [11, 12, 13, 14, 15]
    niter, nsE, biE, nsW, biW = 3, 6, 3, 6, 3

    def utt(i):
        u, n, kind = spec[i]
        X = c.Xs[u][:n].copy()
        if kind == "frame":
            X[5] = 0
        elif kind == "zeros":
            X[:] = 0
        return X, c.W0[u], c.H0[u][:, :n], c.Z0[c.off[u]:c.off[u] + n]

    def load(eng, idx):
        parts = [utt(i) for i in idx]
        eng.set_spectrogram([p[0] for p in parts])
        eng.init_nmf([p[1] for p in parts], [p[2] for p in parts])
        eng.Z.copy_(torch.from_numpy(_pad(np.concatenate([p[3] for p in parts]), eng.Lp)))

    def fused(idx):
        eng = make_engine(c.params, F, K, [spec[i][1] for i in idx], Rcap=6, precision=prec, seeds=[seeds[i] for i in idx])
        outs = []
        for _ in range(3):
            load(eng, idx)
            with np.errstate(all="ignore"):
                cost, S, N = eng.run(niter, nsE, biE, nsW, biW, c.var_rw)
            outs.append(SimpleNamespace(eng=eng, cost=cost.cpu().numpy(), S=S.cpu().numpy(), N=N.cpu().numpy(), W=eng.W.cpu().numpy().copy(),
                                        Ht=eng.Ht.cpu().numpy().copy(), g=eng.g.cpu().numpy().copy(), graph=es.query(eng, "Q_EM_GRAPH")))
        assert [o.graph for o in outs] == [0, 1, 1]
        return outs

    def stepwise(idx):
        eng = make_engine(c.params, F, K, [spec[i][1] for i in idx], Rcap=6, precision=prec, seeds=[seeds[i] for i in idx])
        load(eng, idx)
        eng.sample_store(True)
        cost = np.zeros((len(idx), niter))
        for it in range(niter):
            eng.mh_chain(nsE, biE, c.var_rw, call=it)
            eng.m_step_stored()
            cost[:, it] = eng.cost_from_frames(nsE)
        eng.mh_chain(nsW, biW, c.var_rw, call=niter, update_Z=False)
        S, N, _, _ = eng.wiener_stored()
        return [SimpleNamespace(eng=eng, cost=cost, S=S.cpu().numpy(), N=N.cpu().numpy(), W=eng.W.cpu().numpy().copy(),
                                Ht=eng.Ht.cpu().numpy().copy(), g=eng.g.cpu().numpy().copy())]

    full_idx, sound_idx = [0, 1, 2, 3, 4], [0, 2, 4]
    for how in (fused, stepwise):
        full, sound = how(full_idx), how(sound_idx)
        for call, (a, b) in enumerate(zip(full, sound)):
            for j, i in enumerate(sound_idx):
                sa, sb = a.eng.utt_slice(i), b.eng.utt_slice(j)
                for name, x, y in (("S_hat", a.S[sa], b.S[sb]), ("N_hat", a.N[sa], b.N[sb]), ("W", a.W[i], b.W[j]), ("Ht", a.Ht[sa], b.Ht[sb]),
                                   ("g", a.g[sa], b.g[sb]), ("cost", a.cost[i], b.cost[j])):
                    assert np.all(np.isfinite(y)), (how.__name__, call, i, name)
                    assert np.array_equal(x, y), (how.__name__, call, i, name)
            for i in (1, 3):
                sl = a.eng.utt_slice(i)
                finite = np.all(np.isfinite(a.cost[i])) and np.all(np.isfinite(a.W[i])) and np.all(np.isfinite(a.g[sl])) and np.all(np.isfinite(a.S[sl]))
                assert not finite, (how.__name__, call, i)
        for o in full + sound:
            o.eng.close()
