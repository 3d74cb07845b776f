"""GPU sweep of the kernels around the EM loop: the Lorenz-quantile labels, the SPP recursion, the ideal Wiener mask and
apply_mask (csrc/labels.hip), the dense layer, |X|^2 and the SI-SDR Gram sums (csrc/aux.hip), each against a plain
high-precision statement of the same operation (oracle/vaenmf_oracle.py or float64 numpy) at the sizes where these
kernels take another path.

Rules of this file:
  * Lorenz labels: thresholds and every label EQUAL to the oracle (which is pinned against numpy and the reference in
    tests/test_oracle_golden.py); where numpy raises IndexError the library raises "index -1 is out of bounds".
    Bin counts 1, 7, 8, 9, 127, 128, 129, 136, 257, 264, 640 (pw_block: n < 8, the n % 8 tail; the split n2 -= n2 % 8),
    segment sizes around 128 (one pairwise block), around 8192 (np.sum's reduction blocks) and about 20 k.
  * SPP: soft SPP within 2e-6 absolute, PSD within 1e-6 relative, hard labels `> 0.5` identical (no oracle value is
    within 2e-6 of 0.5: asserted), timo_noise_estimation exact, a ragged batch equal to the single calls bit for bit.
  * dense: max|y - ref64| / max|ref64| <= max(2e-5, 16 e32), e32 = the same layer in float32 numpy against float64,
    computed per case.  ACT_STEP: decisions identical wherever the float64 pre-activation is further from 0 than that
    bound; at most 1 % of the entries are that close (asserted).
  * ideal_wiener_mask 3e-7 absolute; apply_mask exact; power_spec within one float32 ulp of the float64 value; Gram
    sums entry (a, b) within n 2^-52 sqrt(G_aa G_bb) of float64 numpy (recursive summation, Cauchy-Schwarz) and
    ratios_from_gram within 1e-9 dB of orc.energy_ratios.
Every padded buffer carries NaN or 1e30 in its padding, every over-sized output a sentinel that must survive."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vaenmf_oracle as orc
from helpers import GOLDEN, need_gpu

SENTINEL = -7.25
POISON = (float("nan"), 1e30)
OOB = "index -1 is out of bounds"


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------------
# Lorenz labels
LABEL_BINS = (1, 7, 8, 9, 127, 128, 129, 136, 257, 264, 640)
SEGMENT_SIZES = (127, 128, 129, 8191, 8192, 8193, 20000)
QUANTILES = (0.5, 0.93, 0.98, 0.99, 0.999)
_ORACLE = {}


def _frame_counts(F):
    """Frame counts whose IBM run F N lands on (F = 1) or next to the segment sizes; the VAD run is N itself."""
    return sorted({max(1, s // F) for s in SEGMENT_SIZES} | {-(-s // F) for s in SEGMENT_SIZES})


def lorenz_oracle(X, mode, q=0.98, w=0.999, key=None):
    """(labels, threshold) of the oracle for one (F, N) utterance, or the IndexError instance numpy raises.  Computed once
    per key."""
    k = None if key is None else (key, mode, q, w)
    if k not in _ORACLE:
        v = orc.power_c64(X) if mode == "ibm" else orc.frame_power(X)
        try:
            with np.errstate(invalid="ignore", divide="ignore"):
                thr = orc.lorenz_threshold(v, q)
            lab = orc._soften(v > thr, w)
            res = (lab if mode == "ibm" else lab[None], thr)
        except IndexError as e:
            res = e
        if k is None:
            return res
        _ORACLE[k] = res
    return _ORACLE[k]


def _padded_frames(Xs, F, Fs, poison):
    """(F, N_u) utterances -> device complex64 [sum N_u][Fs], bins F.. of every row poisoned."""
    buf = np.full((sum(x.shape[1] for x in Xs), Fs), complex(poison, poison), np.complex64)
    o = 0
    for x in Xs:
        buf[o:o + x.shape[1], :F] = x.T
        o += x.shape[1]
    return _cuda(buf)


def lorenz_device(Xs, mode, q=0.98, w=0.999, pad=0, poison=POISON[0]):
    """target.lorenz_labels_batch on the (F, N_u) utterances Xs -> ([labels per utterance, shaped like the reference's],
    thresholds)."""
    from vaenmf import target
    F = Xs[0].shape[0]
    counts = [x.shape[1] for x in Xs]
    y, thr = target.lorenz_labels_batch(_padded_frames(Xs, F, F + pad, poison), counts, F, mode, q, w, want_thresholds=True)
    y = y.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(counts)])
    return [y[a:b].T if mode == "ibm" else y[a:b][None] for a, b in zip(off[:-1], off[1:])], thr.cpu().numpy()


def _single(mode):
    from vaenmf import target
    return target.clean_speech_IBM if mode == "ibm" else target.clean_speech_VAD


def _assert_labels(got, thr, ref, what):
    assert got.shape == ref[0].shape and got.dtype == np.float32, what
    assert thr == ref[1], (what, float(thr), float(ref[1]))
    assert np.array_equal(got, ref[0]), (what, int((got != ref[0]).sum()))


def _check_batch(Xs, keys, mode, q=0.98, w=0.999, pad=0, poison=POISON[0]):
    """The utterances the oracle labels go through one batched call and must equal it; each of the others must raise."""
    refs = [lorenz_oracle(X, mode, q, w, key) for X, key in zip(Xs, keys)]
    good = [i for i, r in enumerate(refs) if not isinstance(r, IndexError)]
    if good:
        ys, thr = lorenz_device([Xs[i] for i in good], mode, q, w, pad, poison)
        for j, i in enumerate(good):
            _assert_labels(ys[j], thr[j], refs[i], (keys[i], mode, q, w))
    for i in set(range(len(Xs))) - set(good):
        with pytest.raises(RuntimeError, match=OOB):
            _single(mode)(np.ascontiguousarray(Xs[i]), q, w)
    return len(good)


def _unblocked_threshold(values, q):
    """The threshold with the total taken as ONE pairwise tree over the whole sorted run (what the kernel and the oracle
    computed before np.sum's 8192-element blocks were restated); everything else as orc.lorenz_threshold."""
    srt = np.sort(np.asarray(values, np.float32), axis=None)[::-1]
    return srt[np.cumsum(srt) / orc.pairwise_sum_f32(srt) < np.float32(q)][-1]


def _block_cases():
    z = np.load(os.path.join(GOLDEN, "labels_blocks.npz"))
    for mode in ("ibm", "vad"):
        for c, (F, N, seed) in enumerate(z[mode + "_cases"]):
            yield z, mode, c, orc.heavy_tailed_stft(int(F), int(N), int(seed))


def test_the_block_crossing_inputs_tell_the_two_totals_apart():
    """No GPU.  For every input of labels_blocks.npz at q = 0.999, the total summed as one pairwise tree gives another
    threshold and at least one other label than np.sum's blocked total (which the oracle holds and the file records):
    a kernel that still sums the run in one recursion cannot pass test_block_crossing_labels_equal_the_reference."""
    n = 0
    for z, mode, c, X in _block_cases():
        v = orc.power_c64(X) if mode == "ibm" else orc.frame_power(X)
        j = list(z["q"]).index(0.999)
        thr = orc.lorenz_threshold(v, 0.999)
        assert thr == z["%s%d_q%d_thr" % (mode, c, j)]
        old = _unblocked_threshold(v, 0.999)
        assert old != thr, (mode, c)
        assert np.any((v > old) != (v > thr)), (mode, c)
        print("%s %s: blocked total -> threshold %.9g, one pairwise tree -> %.9g, %d label(s) differ"
              % (mode, X.shape, thr, old, int(((v > old) != (v > thr)).sum())))
        n += 1
    assert n == 5


@pytest.mark.parametrize("F", LABEL_BINS)
def test_lorenz_labels_over_bins_and_segment_sizes(F):
    """IBM and VAD, one ragged batch per bin count with a row stride of F + 3 and poisoned padding: thresholds and labels
    equal the oracle; the utterances numpy refuses (a single frame for VAD) raise."""
    need_gpu()
    Ns = _frame_counts(F)
    Xs = [orc.heavy_tailed_stft(F, N, 1000 * F + N) for N in Ns]
    keys = [("sweep", F, N) for N in Ns]
    for mode in ("ibm", "vad"):
        n_good = _check_batch(Xs, keys, mode, pad=3, poison=POISON[F % 2])
        assert n_good >= len(Ns) - 2, (mode, n_good, Ns)


def test_lorenz_ragged_batch_equals_the_single_calls():
    """Frame counts [1, 2, 33, 130, 9] in one call: every utterance's threshold and labels equal its single-utterance call
    (segment offsets, frame_utt) and the oracle.  VAD: the one-frame utterance raises, alone and in the batch, and the
    message names it."""
    need_gpu()
    F, counts = 129, [1, 2, 33, 130, 9]
    Xs = [orc.heavy_tailed_stft(F, N, 42 + N) for N in counts]
    keys = [("ragged", F, N) for N in counts]
    ys, thr = lorenz_device(Xs, "ibm", pad=7, poison=POISON[1])
    for u, X in enumerate(Xs):
        y1, t1 = lorenz_device([X], "ibm")
        assert t1[0] == thr[u] and np.array_equal(y1[0], ys[u]), u
        assert np.array_equal(_single("ibm")(np.ascontiguousarray(X)), ys[u]), u
        _assert_labels(ys[u], thr[u], lorenz_oracle(X, "ibm", key=keys[u]), keys[u])
    refs = [lorenz_oracle(X, "vad", key=k) for X, k in zip(Xs, keys)]
    assert [isinstance(r, IndexError) for r in refs] == [True, False, False, False, False]
    with pytest.raises(RuntimeError, match=OOB + r".*utterance 0:"):
        lorenz_device(Xs, "vad")
    with pytest.raises(RuntimeError, match=OOB + r".*utterance 2:"):
        lorenz_device([Xs[2], Xs[3], Xs[0], Xs[4]], "vad")
    ys, thr = lorenz_device(Xs[1:], "vad", pad=7)
    for u, X in enumerate(Xs[1:]):
        y1, t1 = lorenz_device([X], "vad")
        assert t1[0] == thr[u] and np.array_equal(y1[0], ys[u]), u
        assert np.array_equal(_single("vad")(np.ascontiguousarray(X)), ys[u]), u
        _assert_labels(ys[u], thr[u], refs[u + 1], keys[u + 1])


def test_lorenz_c_abi_leaves_the_output_padding_alone():
    """vaenmf_lorenz_labels with ld > F (and Fs > F, poisoned): columns >= F of the IBM output keep their sentinel."""
    need_gpu()
    from vaenmf import _lib
    F, Fs, ld, counts = 129, 136, 140, [33, 9]
    Xs = [orc.heavy_tailed_stft(F, N, 42 + N) for N in counts]
    X = torch.view_as_real(_padded_frames(Xs, F, Fs, POISON[0]))
    NT, U = sum(counts), len(counts)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    nbytes = _lib.lib().vaenmf_lorenz_work_bytes(NT, F, U, _lib.LABEL_IBM)
    work = torch.empty(int(nbytes), dtype=torch.uint8, device="cuda")
    out = torch.full((NT, ld), SENTINEL, dtype=torch.float32, device="cuda")
    thr = torch.empty(U, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().vaenmf_lorenz_labels(X.data_ptr(), U, off.ctypes.data, F, Fs, _lib.LABEL_IBM, 0.98, 0.0, 1.0, out.data_ptr(), ld,
                                               thr.data_ptr(), work.data_ptr(), int(nbytes), _stream()))
    out, thr = out.cpu().numpy(), thr.cpu().numpy()
    assert np.all(out[:, F:] == SENTINEL)
    for u, X1 in enumerate(Xs):
        _assert_labels(out[off[u]:off[u + 1], :F].T, thr[u], lorenz_oracle(X1, "ibm", key=("ragged", F, counts[u])), u)


@pytest.mark.parametrize("F,N", [(129, 33), (65, 130)])
def test_lorenz_quantiles_soft_values_and_noise_robust_variants(F, N):
    """Five fractions, the default quantile_weight and one that changes the soft values (3.0: -1 and 2 instead of 0 and
    1), and the noise-robust variants (target.py:52-102), below and above 8192 entries."""
    need_gpu()
    from vaenmf import target
    X = np.ascontiguousarray(orc.heavy_tailed_stft(F, N, 7))
    assert sorted(np.unique(orc._soften(np.array([False, True]), 3.0))) == [-1.0, 2.0]
    n_good = 0
    for q in QUANTILES:
        for w in (0.999, 3.0):
            for mode in ("ibm", "vad"):
                n_good += _check_batch([X], [("q", F, N)], mode, q, w)
    assert n_good >= 16
    assert np.array_equal(target.noise_robust_clean_speech_VAD(X), orc.noise_robust_clean_speech_VAD(X))
    assert np.array_equal(target.noise_robust_clean_speech_IBM(X), orc.noise_robust_clean_speech_IBM(X))
    assert np.array_equal(target.noise_robust_clean_speech_VAD(X, 0.9, 0.98, 3.0), orc.noise_robust_clean_speech_VAD(X, 0.9, 0.98, 3.0))


def test_block_crossing_labels_equal_the_reference():
    """The inputs of tests/golden/labels_blocks.npz (sorted runs longer than np.sum's 8192-element blocks, among them a VAD
    input of 8300 frames): labels equal the reference's stored outputs, thresholds the stored ones, through the
    single-utterance wrappers and the batched entry."""
    need_gpu()
    for z, mode, c, X in _block_cases():
        for j, q in enumerate(z["q"]):
            ref = z["%s%d_q%d" % (mode, c, j)].astype(np.float32)
            ys, thr = lorenz_device([X], mode, float(q), pad=1)
            want = z["%s%d_q%d_thr" % (mode, c, j)]
            assert thr[0] == want, (mode, c, float(q), float(thr[0]), float(want))
            assert np.array_equal(ys[0], ref), (mode, c, float(q), int((ys[0] != ref).sum()))
            assert np.array_equal(_single(mode)(np.ascontiguousarray(X), float(q)), ref), (mode, c, float(q))


def test_lorenz_degenerate_inputs():
    """All-zero, all-equal, leading silent frames with exact zeros and ties, one frame for VAD: the oracle's labels or the
    library's IndexError text; inside a batch the error names the degenerate utterance."""
    need_gpu()
    F = 9
    zero = np.zeros((F, 4), np.complex64)
    equal = np.full((F, 4), 1 + 1j, np.complex64)
    quiet = np.ascontiguousarray(orc.heavy_tailed_stft(F, 40, 3))
    quiet[:, :7] = 0
    quiet[:, 11] = quiet[:, 10]
    quiet[3, 20:24] = quiet[3, 20]
    one = np.ascontiguousarray(orc.heavy_tailed_stft(F, 1, 5))
    for mode in ("ibm", "vad"):
        assert isinstance(lorenz_oracle(zero, mode), IndexError)
        for X in (equal, quiet):
            assert not isinstance(lorenz_oracle(X, mode), IndexError)
        assert _check_batch([zero, equal, quiet, one], [None] * 4, mode, pad=2) == (3 if mode == "ibm" else 2)
        with pytest.raises(RuntimeError, match=OOB + r".*utterance 1:"):
            lorenz_device([quiet, zero, equal], mode)
    assert isinstance(lorenz_oracle(one, "vad"), IndexError)
    assert np.all(lorenz_oracle(equal, "ibm")[0] == 0)          # nothing is above the threshold when all are equal


# ---------------------------------------------------------------------------------------------------------------------
# SPP
SPP_BINS = (1, 63, 64, 65, 257, 640)
SPP_LENGTHS = (1, 9, 10, 11, 40)
SPP_INIT = (0, 1, 10)


def spp_input(F, N, seed):
    """float32 periodograms [N][F]: exponential bins (|complex Gaussian|^2) times a log-normal frame gain."""
    g = np.random.default_rng(seed)
    return ((g.standard_normal((N, F)) ** 2 + g.standard_normal((N, F)) ** 2) * np.exp(1.2 * g.standard_normal((N, 1)))).astype(np.float32)


def spp_device(pers, F, pad=0, poison=POISON[0], **kw):
    """spp_batch on the [N_u][F] periodograms -> (spp, psd) float32 [sum N_u][F]."""
    from vaenmf import spp_estimation as spp
    buf = np.full((sum(len(p) for p in pers), F + pad), poison, np.float32)
    buf[:, :F] = np.concatenate(pers)
    s, psd = spp.spp_batch(_cuda(buf), [len(p) for p in pers], F, want_psd=True, **kw)
    return s.cpu().numpy(), psd.cpu().numpy()


def _assert_spp(s, psd, per, what, **kw):
    ref_psd, ref_spp = orc.spp_recursion(per, **kw)
    assert np.min(np.abs(ref_spp - 0.5)) > 2e-6, what            # (else: another seed) no hard label hangs on the tolerance
    e_spp = float(np.max(np.abs(s - ref_spp)))
    e_psd = float(np.max(np.abs(psd - ref_psd) / (np.abs(ref_psd) + 1e-12)))
    print("spp %s: soft %.2e (2e-6), psd %.2e (1e-6)" % (what, e_spp, e_psd))
    assert e_spp < 2e-6 and e_psd < 1e-6, (what, e_spp, e_psd)
    assert np.array_equal(s > 0.5, ref_spp > 0.5), what
    return ref_spp


@pytest.mark.parametrize("F", SPP_BINS)
def test_spp_over_bins_lengths_and_init_frames(F):
    """Utterances shorter than, equal to and longer than num_frames_init in one ragged batch (row stride F + 5, poisoned)
    against orc.spp_recursion; the batch equals the single calls bit for bit."""
    need_gpu()
    pers = [spp_input(F, N, 10 * F + N) for N in SPP_LENGTHS]
    off = np.concatenate([[0], np.cumsum(SPP_LENGTHS)])
    for nfi in SPP_INIT:
        s, psd = spp_device(pers, F, pad=5, poison=POISON[nfi % 2], num_frames_init=nfi)
        assert s.shape == psd.shape == (off[-1], F)
        for u, per in enumerate(pers):
            a, b = off[u], off[u + 1]
            _assert_spp(s[a:b], psd[a:b], per, (F, len(per), nfi), num_frames_init=nfi)
            s1, psd1 = spp_device([per], F, num_frames_init=nfi)
            assert np.array_equal(s1, s[a:b]) and np.array_equal(psd1, psd[a:b]), (F, u, nfi)


def test_spp_clamp_branch_and_other_constants():
    """A quiet start followed by a sustained loud signal drives the smoothed SPP above 0.99, where the SPP is clamped to
    0.99 (spp_estimation.py:122-123); the oracle's output shows that the branch fired.  Then other smoothing constants,
    prior and SNR."""
    need_gpu()
    F, N = 65, 90
    g = np.random.default_rng(4)
    per = (g.standard_normal((N, F)) ** 2 + g.standard_normal((N, F)) ** 2).astype(np.float32)
    per[:14] *= 1e-3
    per[14:] *= 100.0
    s, psd = spp_device([per], F, pad=3)
    ref = _assert_spp(s, psd, per, "clamp")
    assert np.sum(ref == 0.99) > F and np.any(ref > 0.99)        # clamped entries, and unclamped ones above 0.99 before them
    assert np.array_equal(s == np.float32(0.99), ref == 0.99)
    kw = dict(fixed_smooth=0.7, prob_smooth=0.8, prior=0.3, snr_opt_db=10, num_frames_init=3)
    per = spp_input(F, 40, 9)
    s, psd = spp_device([per], F, **kw)
    _assert_spp(s, psd, per, "constants", **kw)


@pytest.mark.parametrize("F,N", [(1, 11), (65, 40), (257, 9), (640, 10)])
def test_spp_wrappers(F, N):
    """timo_mask_estimation, timo_vad_estimation (2e-6, hard labels identical) and timo_noise_estimation (exact)."""
    need_gpu()
    from vaenmf import spp_estimation as spp
    P = np.ascontiguousarray(spp_input(F, N, 77 + F).T)                      # (bins, frames)
    ref = orc.timo_mask_estimation(P)
    m = spp.timo_mask_estimation(P)
    assert m.shape == P.shape and m.dtype == P.dtype
    assert np.max(np.abs(m - ref)) < 2e-6 and np.array_equal(m > 0.5, ref > 0.5)
    ref_v = orc.timo_vad_estimation(P)
    v = spp.timo_vad_estimation(P)
    assert v.shape == (N,) and v.dtype == P.dtype
    assert np.min(np.abs(ref_v.astype(np.float64) - 0.5)) > 2e-6
    assert np.max(np.abs(v - ref_v)) < 2e-6 and np.array_equal(v > 0.5, ref_v > 0.5)
    mask = np.random.default_rng(F).random(P.shape).astype(np.float32)
    for mk in (ref, mask):
        assert np.array_equal(spp.timo_noise_estimation(P, mk), orc.timo_noise_estimation(P, mk))


# ---------------------------------------------------------------------------------------------------------------------
# dense
DENSE_M = (1, 63, 64, 65, 130)
DENSE_IN = (1, 15, 16, 17, 129, 262)
DENSE_OUT = (1, 5, 16, 63, 64, 65, 257)
ACTS = {"none": 0, "tanh": 1, "relu": 2, "sigmoid": 3, "step": 4}


def _act(name, v):
    if name == "tanh":
        return np.tanh(v)
    if name == "relu":
        return np.maximum(v, v.dtype.type(0))
    if name == "sigmoid":
        return v.dtype.type(1) / (v.dtype.type(1) + np.exp(-v))
    return v


def dense_refs(x, w, b, name):
    """The layer in float64 and in float32 numpy -> (pre-activation 64, output 64, bound): bound = max(2e-5, 16 e32) times
    max|ref|, e32 the float32 evaluation's own error relative to max|ref|.  For the step, ref is the pre-activation."""
    p64 = x.astype(np.float64) @ w.astype(np.float64).T + (0 if b is None else b.astype(np.float64))
    p32 = x @ w.T + (np.float32(0) if b is None else b)
    assert p32.dtype == np.float32
    r64, r32 = _act(name, p64), _act(name, p32)
    scale = float(np.max(np.abs(r64)))
    e32 = float(np.max(np.abs(r32 - r64)))                  # absolute; the rule's e32 is this over `scale`
    return p64, r64, max(2e-5 * scale, 16 * e32), e32 / max(scale, 1e-300)


def dense_device(x, w, b, act, ldx_pad=0, rows_pad=0, cols_pad=0):
    """vaenmf_dense through the C ABI: x with a row stride of in + ldx_pad (padding poisoned), Y with rows_pad more rows
    and cols_pad more columns than the layer writes, pre-filled with the sentinel."""
    from vaenmf import _lib
    M, inn = x.shape
    out = w.shape[0]
    xb = np.full((M, inn + ldx_pad), POISON[0], np.float32)
    xb[:, :inn] = x
    xd, wd, bd = _cuda(xb), _cuda(w), None if b is None else _cuda(b)
    Y = torch.full((M + rows_pad, out + cols_pad), SENTINEL, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().vaenmf_dense(xd.data_ptr(), M, inn, inn + ldx_pad, wd.data_ptr(), None if bd is None else bd.data_ptr(), out, act,
                                       Y.data_ptr(), out + cols_pad, _stream()))
    return Y.cpu().numpy()


def _dense_case(M, inn, out, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal((M, inn)).astype(np.float32)
    w = (g.standard_normal((out, inn)) / np.sqrt(inn)).astype(np.float32)
    b = (0.3 * g.standard_normal(out)).astype(np.float32)
    return x, w, b


@pytest.mark.parametrize("name", ["none", "tanh", "relu", "sigmoid", "step", "no_bias"])
def test_dense_over_shapes(name):
    """Every (M, in, out) of the grid per activation (and once without a bias): strided input, over-sized output."""
    need_gpu()
    act_name = "none" if name == "no_bias" else name
    worst, worst_e32, n_close, n_all = 0.0, 0.0, 0, 0
    for M in DENSE_M:
        for inn in DENSE_IN:
            for out in DENSE_OUT:
                x, w, b = _dense_case(M, inn, out, M * 1000003 + inn * 1009 + out)
                if name == "no_bias":
                    b = None
                p64, r64, bound, e32 = dense_refs(x, w, b, act_name)
                Y = dense_device(x, w, b, ACTS[act_name], ldx_pad=(M + inn) % 4, rows_pad=2, cols_pad=1 + out % 3)
                assert np.all(Y[M:] == SENTINEL) and np.all(Y[:, out:] == SENTINEL), (M, inn, out)
                y = Y[:M, :out]
                if name == "step":
                    sure = np.abs(p64) > bound
                    n_close += int((~sure).sum())
                    n_all += sure.size
                    assert set(np.unique(y)) <= {0.0, 1.0}
                    assert np.array_equal(y[sure], (p64[sure] > 0).astype(np.float32)), (M, inn, out)
                else:
                    err = float(np.max(np.abs(y - r64)))
                    assert err <= bound, (M, inn, out, err, bound, e32)
                    worst = max(worst, err / bound if bound else 0.0)      # (bound 0: a ReLU layer that is all zero, exactly)
                worst_e32 = max(worst_e32, e32)
    if name == "step":
        print("dense step: %d of %d pre-activations within the bound of 0 (%.3f %%)" % (n_close, n_all, 100.0 * n_close / n_all))
        assert n_close <= 0.01 * n_all
    else:
        print("dense %s: largest error / bound %.3f, largest e32 %.2e" % (name, worst, worst_e32))


def test_dense_through_the_engine():
    """eng.dense with the view X2[:, :F] (row stride Fs > F), eng.encode of an M2 encoder (in = F + Dy = 262) and
    eng.classify (normalisation folded into the first layer) against float64 numpy of the whole network; the bound is the
    rule above with e32 = the whole network in float32 numpy."""
    need_gpu()
    from vaenmf.engine import BatchEngine
    F, Dy, counts = 257, 5, [3, 65, 62]
    NT = sum(counts)
    params = orc.xavier_normal_params([F, 32, [128, 128]], seed=3, y_dim=Dy, bias_std=0.1)
    dec = [params[k] for k in ("decoder.hidden.0.weight", "decoder.hidden.0.bias", "decoder.hidden.1.weight", "decoder.hidden.1.bias",
                               "decoder.reconstruction.weight", "decoder.reconstruction.bias")]
    eng = BatchEngine(F, 4, dec, max_frames=NT, max_utts=len(counts))
    eng.bind(counts, Rcap=4)
    g = np.random.default_rng(8)
    Xs = [(0.7 * (g.standard_normal((n, F)) + 1j * g.standard_normal((n, F)))).astype(np.complex64) for n in counts]
    eng.set_spectrogram(Xs)
    assert eng.Fs > F
    x2 = eng.X2[:, :F].cpu().numpy()
    assert np.all(eng.X2[:, F:].cpu().numpy() == 0)

    def net(x, layers, acts, dt):
        h = x.astype(dt)
        for (w, b), a in zip(layers, acts):
            h = _act(a, h @ w.astype(dt).T + b.astype(dt))
        return h

    def bound_of(x, layers, acts):
        r64, r32 = net(x, layers, acts, np.float64), net(x, layers, acts, np.float32)
        scale = float(np.max(np.abs(r64)))
        e32 = float(np.max(np.abs(r32 - r64))) / scale
        return r64, max(2e-5, 16 * e32) * scale, e32

    # one layer on the strided view
    w, b = params["encoder.hidden.0.weight"][:, :F], params["encoder.hidden.0.bias"]
    r64, bound, e32 = bound_of(x2, [(w, b)], ["tanh"])
    y = eng.dense(eng.X2[:, :F], _cuda(w), _cuda(b), ACTS["tanh"]).cpu().numpy()
    print("engine dense: error %.2e, bound %.2e, e32 %.2e" % (np.max(np.abs(y - r64)), bound, e32))
    assert np.max(np.abs(y - r64)) <= bound
    # the M2 encoder
    yl = (g.random((NT, Dy)) > 0.5).astype(np.float32)
    enc = [(params["encoder.hidden.%d.weight" % i], params["encoder.hidden.%d.bias" % i]) for i in range(2)]
    enc.append((params["encoder.sample.mu.weight"], params["encoder.sample.mu.bias"]))
    assert enc[0][0].shape[1] == 262
    r64, bound, e32 = bound_of(np.concatenate([x2, yl], 1), enc, ["tanh", "tanh", "none"])
    eng.encode(enc, _cuda(yl))
    z = eng.Z.cpu().numpy()
    print("encode: error %.2e, bound %.2e, e32 %.2e" % (np.max(np.abs(z - r64)), bound, e32))
    assert np.max(np.abs(z - r64)) <= bound
    # the classifier, with and without normalisation
    cp = orc.xavier_normal_classifier([F, [128, 128], Dy], seed=5, bias_std=0.3)
    clf = [(cp["hidden.0.weight"], cp["hidden.0.bias"]), (cp["hidden.1.weight"], cp["hidden.1.bias"]), (cp["output_layer.weight"], cp["output_layer.bias"])]
    mean = (g.random((F, 1)) * 2).astype(np.float32)
    std = (0.5 + g.random((F, 1))).astype(np.float32)
    for mm, ss in ((None, None), (mean, std)):
        xin64 = x2.astype(np.float64) if mm is None else (x2.astype(np.float64) - mm.T) / (ss.astype(np.float64) + 1e-8).T
        xin32 = x2 if mm is None else (x2 - mm.T) / (ss + np.float32(1e-8)).T
        assert xin32.dtype == np.float32
        acts = ["relu", "relu", "none"]
        p64, p32 = net(xin64, clf, acts, np.float64), net(xin32, clf, acts, np.float32)
        s64, s32 = _act("sigmoid", p64), _act("sigmoid", p32)
        b_soft = max(2e-5, 16 * float(np.max(np.abs(s32 - s64))) / float(np.max(s64))) * float(np.max(s64))
        b_pre = max(2e-5, 16 * float(np.max(np.abs(p32 - p64))) / float(np.max(np.abs(p64)))) * float(np.max(np.abs(p64)))
        soft, hard = eng.classify(clf, mm, ss)
        soft, hard = soft.cpu().numpy(), hard.cpu().numpy()
        print("classify: soft error %.2e, bound %.2e" % (np.max(np.abs(soft - s64)), b_soft))
        assert np.max(np.abs(soft - s64)) <= b_soft
        sure = np.abs(p64) > b_pre
        assert (~sure).sum() <= 0.01 * sure.size
        assert np.array_equal(hard[sure], (p64[sure] > 0).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# small kernels
def test_ideal_wiener_mask_edges():
    """3e-7 against the float32 numpy statement; exact zeros in both inputs (the eps dominates) and components near 1e-19
    and 1e19, where re^2 + im^2 under- or overflows in float32 but the magnitude itself does not."""
    need_gpu()
    from vaenmf import target
    g = np.random.default_rng(6)
    S = (g.standard_normal((33, 17)) + 1j * g.standard_normal((33, 17))).astype(np.complex64)
    N = (g.standard_normal((33, 17)) + 1j * g.standard_normal((33, 17))).astype(np.complex64) * np.float32(1e-3)
    S[0, :4] = 0
    N[0, 2:6] = 0                                   # (0, n), (0, 0), (s, 0)
    S[1, :7] = np.array([1e-19 + 1e-19j, 1e-19, 1e19 + 1e19j, 1e19j, 1e-19 + 1e-19j, 1e19, 1e19 + 1e19j], np.complex64)
    N[1, :7] = np.array([1e-19j, 0, 1e-19, 1e19 + 1e19j, 1e19, 1e-19 - 1e-19j, 1e19 - 1e19j], np.complex64)
    for eps in (1e-8, 1e-30):
        with np.errstate(over="ignore", under="ignore"):
            ref = orc.ideal_wiener_mask(S, N, eps)
        got = target.ideal_wiener_mask(S, N, eps)
        assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32
        assert np.all(np.isfinite(ref)) and np.all(np.isfinite(got))
        err = float(np.max(np.abs(got - ref)))
        print("wiener mask eps %g: %.2e (3e-7)" % (eps, err))
        assert err < 3e-7
    assert ref[0, 2] == 0 and ref[0, 3] == 0


def test_apply_mask_exact():
    """vaenmf_apply_mask: S = mask * X, one float32 product per component, exact zeros in bins F .. Fs-1, mask row stride
    ldm > F (its padding and X's poisoned)."""
    need_gpu()
    from vaenmf import _lib
    for NT, F, Fs, ldm in ((1, 1, 1, 1), (37, 129, 136, 131), (3, 257, 272, 300), (300, 7, 8, 7)):
        g = np.random.default_rng(NT + F)
        X = np.full((NT, Fs), complex(POISON[0], POISON[0]), np.complex64)
        X[:, :F] = (g.standard_normal((NT, F)) + 1j * g.standard_normal((NT, F))).astype(np.complex64)
        m = np.full((NT, ldm), POISON[1], np.float32)
        m[:, :F] = g.random((NT, F)).astype(np.float32)
        Xd, md = torch.view_as_real(_cuda(X)), _cuda(m)
        S = torch.full((NT + 1, Fs, 2), SENTINEL, dtype=torch.float32, device="cuda")
        _lib.check(_lib.lib().vaenmf_apply_mask(Xd.data_ptr(), md.data_ptr(), ldm, NT, F, Fs, S.data_ptr(), _stream()))
        S = S.cpu().numpy()
        assert np.all(S[NT] == SENTINEL)
        assert np.array_equal(S[:NT, :F, 0], X[:, :F].real * m[:, :F]) and np.array_equal(S[:NT, :F, 1], X[:, :F].imag * m[:, :F])
        assert np.all(S[:NT, F:] == 0)


def test_power_spec_within_one_ulp():
    """vaenmf_power_spec: re^2 + im^2 within one float32 ulp of the float64 value.  fma(re, re, round(im^2)) rounds twice, each
    time by at most half an ulp of the sum; a separate multiply per component and an add round three times (up to 1.25 ulp:
    1.037 at n = 255 and 1.136 at n = 5000 on these inputs, which is what the kernel gave before it spelled the fma out)."""
    need_gpu()
    from vaenmf import _lib
    for n in (1, 255, 256, 257, 5000):
        g = np.random.default_rng(n)
        X = ((g.standard_normal(n) + 1j * g.standard_normal(n)) * np.exp(3 * g.standard_normal(n))).astype(np.complex64)
        out = torch.full((n + 3,), SENTINEL, dtype=torch.float32, device="cuda")
        _lib.check(_lib.lib().vaenmf_power_spec(torch.view_as_real(_cuda(X)).data_ptr(), out.data_ptr(), n, _stream()))
        out = out.cpu().numpy()
        assert np.all(out[n:] == SENTINEL)
        ref = X.real.astype(np.float64) ** 2 + X.imag.astype(np.float64) ** 2
        ulp = np.spacing(ref.astype(np.float32)).astype(np.float64)
        worst = float(np.max(np.abs(out[:n] - ref) / ulp))
        print("power_spec n=%d: %.3f ulp" % (n, worst))
        assert worst <= 1.0


def test_gram_sums_and_ratios():
    """gram3_batch_device on a ragged batch of [1, 255, 256, 257, 4000] samples against float64 numpy, entry (a, b) within
    n 2^-52 sqrt(G_aa G_bb); ratios_from_gram within 1e-9 dB of orc.energy_ratios.  (One sample: s_hat - s_target is
    identically zero, the ratios are 0/0 in either formulation -- the Gram sums alone are compared there.)"""
    need_gpu()
    from vaenmf import metrics
    counts = [1, 255, 256, 257, 4000]
    g = np.random.default_rng(12)
    s = [g.standard_normal(n).astype(np.float32) for n in counts]
    nz = [(0.5 * g.standard_normal(n)).astype(np.float32) for n in counts]
    sh = [(0.8 * a + 0.3 * b + 0.2 * g.standard_normal(len(a))).astype(np.float32) for a, b in zip(s, nz)]
    G = metrics.gram3_batch_device(_cuda(np.concatenate(sh)), _cuda(np.concatenate(s)), _cuda(np.concatenate(nz)), counts)
    assert G.dtype == torch.float64 and tuple(G.shape) == (len(counts), 6)
    G = G.cpu().numpy()
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    diag = {0: 0, 1: 3, 2: 5}
    for u, n in enumerate(counts):
        v = [a.astype(np.float64) for a in (sh[u], s[u], nz[u])]
        ref = np.array([np.dot(v[a], v[b]) for a, b in pairs])
        for k, (a, b) in enumerate(pairs):
            bound = n * 2.0 ** -52 * np.sqrt(ref[diag[a]] * ref[diag[b]])
            assert abs(G[u, k] - ref[k]) <= bound, (n, a, b, G[u, k] - ref[k], bound)
        if n > 1:
            got, want = metrics.ratios_from_gram(G[u]), orc.energy_ratios(*v)
            err = max(abs(float(x) - float(y)) for x, y in zip(got, want))
            print("gram n=%d: largest Gram error / bound %.3f, ratios differ by %.2e dB (1e-9)"
                  % (n, max(abs(G[u, k] - ref[k]) / (n * 2.0 ** -52 * np.sqrt(ref[diag[a]] * ref[diag[b]])) for k, (a, b) in enumerate(pairs)), err))
            assert err < 1e-9, (n, got, want)
