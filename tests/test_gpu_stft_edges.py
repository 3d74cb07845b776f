"""STFT / iSTFT on the GPU where tests/test_gpu_stft_any_length.py does not go, against the float64 restatement of
tests/stft_cases.py (anchored to the oracle in tests/test_stft_edges_cpu.py): the Bluestein inverse at even lengths, odd
lengths through istft_batch, hops other than a quarter window (fewer and more overlapping frames, hops that do not divide
n_fft, hop >= n_fft), signals shorter than the window (reflection that bounces more than once), and the iSTFT as a ragged
batch on exact, guard-banded buffers.

Bounds.  STFT: the module's own rule, max |X - Xr| <= 2e-7 max |Xr| per utterance.  iSTFT: the per-sample bound of
stft_cases.istft_bound, derived from the kernels' roundings; every test prints its worst error / bound (run with -s), and
DESIGN.md 3.5a holds the figures per kernel family.  Round trips: the 2e-6 of the neighbouring module, relative to the
signal's peak (its speech peaks at 1, the noise here near 4)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vaenmf_oracle as orc
from guarded import POISON, Arena, same_bits
from helpers import need_gpu
from stft_cases import (BLUESTEIN_EVEN, EDGE_FS, EDGE_HOPS, ODD_SIZES, SHORT_HOPS, edge_noise, edge_rate, istft_error_over_bound, random_window,
                        ref_geometry, ref_istft_terms, ref_stft, short_lengths)

FS = EDGE_FS
# kernel families: name -> (n_fft, analysis / synthesis window, centre settings the family takes)
FAMILIES = {
    "radix2_64": (64, "hann", (True,)),                         # the radix-2 kernels take centred frames only
    "mixed_64": (64, orc.hann_periodic(64), (True, False)),     # an explicit window sends 64 points to the mixed-radix kernels
    "mixed_400": (400, "hann", (True, False)),
    "bluestein_22": (22, "hann", (True, False)),
    "bluestein_17": (17, "hann", (True, False)),                # odd: the inverse through istft_batch
}


def _close(X, Xr, tol=2e-7):
    assert X.shape == Xr.shape, (X.shape, Xr.shape)
    err = np.max(np.abs(X - Xr))
    assert err <= tol * np.max(np.abs(Xr)), (err, np.max(np.abs(Xr)))


def _pack(specs, fill=0.0):
    """Spectrograms (F, n_frames) as one device tensor [NT][Fs][2] with Fs > F, its padding columns holding `fill`."""
    F = specs[0].shape[0]
    Fs = (F + 16) // 16 * 16                       # the next multiple of 16 above F: 1024 bins (n_fft 2046) take 1040
    S = np.full((sum(s.shape[1] for s in specs), Fs, 2), fill, np.float32)
    rows = np.ascontiguousarray(np.concatenate([np.asarray(s, dtype=np.complex64).T for s in specs]))
    S[:, :F] = rows.view(np.float32).reshape(-1, F, 2)
    return torch.from_numpy(S).cuda()


def _istft(specs, lens, n, hop_percent=0.25, win="hann", center=True, fill=0.0):
    """vaenmf.stft.istft_batch on ordinary buffers -> one float32 array per utterance."""
    from vaenmf import stft as vstft
    out = vstft.istft_batch(_pack(specs, fill), [s.shape[1] for s in specs], lens, n, int(hop_percent * n), win=win, center=center)
    return np.split(out.cpu().numpy(), np.cumsum(lens)[:-1])


def _in_bound(y, S, n, what, **kw):
    """y against the restatement of the complex64 spectrogram S under the derived bound; prints the worst error / bound."""
    fs, wl = edge_rate(n)
    r = ref_istft_terms(S, fs=fs, wlen_sec=wl, max_len=len(y), **kw)
    q = istft_error_over_bound(y, r)
    print("istft worst error / bound, %s: %.3f" % (what, q))
    assert q <= 1.0, (what, q)
    return r


# ---------------------------------------------------------------------------------------------------------------------
# A. Inverse transforms no reference had seen
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", BLUESTEIN_EVEN + ODD_SIZES)
def test_inverse_against_the_restatement(n):
    need_gpu()
    x = edge_noise(n, 4 * n + 3)
    fs, wl = edge_rate(n)
    wins = ("hann", random_window(n)) if n in (22, 1031, 2046) else ("hann",)
    for win in wins:
        tag = "n=%d %s" % (n, win if isinstance(win, str) else "random window")
        S = ref_stft(x, fs=fs, wlen_sec=wl, win=win).astype(np.complex64)
        y, = _istft([S], [len(x)], n, win=win)
        assert y.dtype == np.float32
        _in_bound(y, S, n, tag, win=win)
        assert np.max(np.abs(y - x)) < 2e-6 * np.max(np.abs(x)), (tag, "round trip", np.max(np.abs(y - x)))
        # the imaginary parts of DC and (even n) Nyquist are ignored, as a c2r transform ignores them
        g = np.random.default_rng(7 * n)
        R = (g.standard_normal(S.shape) + 1j * g.standard_normal(S.shape)).astype(np.complex64)
        Rc = R.copy()
        Rc[0] = Rc[0].real
        if n % 2 == 0:
            Rc[-1] = Rc[-1].real
        assert np.all(R[0].imag != 0) and (n % 2 or np.all(R[-1].imag != 0)) and np.all(Rc[1].imag != 0)
        T = (n // 4) * (S.shape[1] - 1)
        y, = _istft([R], [T], n, win=win)
        yc, = _istft([Rc], [T], n, win=win)
        assert np.array_equal(y.view(np.int32), yc.view(np.int32)), (tag, "imaginary part of DC / Nyquist is used")
        _in_bound(y, Rc, n, tag + ", random spectrogram", win=win)


def test_reference_signature_still_refuses_odd_lengths():
    from vaenmf import stft as vstft
    for n in ODD_SIZES:
        with pytest.raises(ValueError):
            vstft.istft(np.zeros((n // 2 + 1, 9), np.complex64), fs=FS, wlen_sec=n / FS)


# ---------------------------------------------------------------------------------------------------------------------
# B. Hops other than a quarter window
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("hop", EDGE_HOPS)
def test_other_hops(hop, family):
    need_gpu()
    from vaenmf import stft as vstft
    n, win, centers = FAMILIES[family]
    wl = n / FS
    if int(hop * n) == 0:
        with pytest.raises(NotImplementedError, match="hop must be positive"):
            vstft.stft(np.zeros(100), fs=FS, wlen_sec=wl, hop_percent=hop)
        with pytest.raises(Exception, match="hop must be positive"):
            _istft([np.ones((n // 2 + 1, 3), np.complex64)], [40], n, hop_percent=hop)
        return
    x = edge_noise(n + int(1000 * hop), 6 * n + 3)
    for center in centers:
        tag = "%s hop %g%s" % (family, hop, "" if center else " uncentred")
        nfft, h, Tp, nfr = ref_geometry(len(x), FS, wl, hop, center)
        assert vstft.frame_geometry(len(x), FS, wl, hop, center) == (nfft, h, nfr, Tp)
        X = vstft.stft(x, fs=FS, wlen_sec=wl, win=win, hop_percent=hop, center=center)
        Xr = ref_stft(x, fs=FS, wlen_sec=wl, win=win, hop_percent=hop, center=center)
        assert X.shape == (n // 2 + 1, nfr)
        _close(X, Xr)
        # 50 samples past the overlap-add's end: with hop > n_fft also samples between frames that no frame covers, with
        # hop = n_fft samples under a Hann window's first sample (sum of squares 0: not divided)
        T = n + h * (nfr - 1) + 50
        S = Xr.astype(np.complex64)
        y, = _istft([S], [T], n, hop_percent=hop, win=win, center=center)
        r = _in_bound(y, S, n, tag, win=win, hop_percent=hop, center=center)
        assert not np.any(y[-50:])
        if hop >= 1.0:
            lo = n // 2 if center else 0
            assert np.any((r.wss[:T - 50 - lo] == 0) & (r.k[:T - 50 - lo] == (1 if hop == 1.0 else 0)))
        else:
            y, = _istft([X], [len(x)], n, hop_percent=hop, win=win, center=center)
            lo = 0 if center else n                 # uncentred, the first / last n samples lie under window edges only
            assert np.max(np.abs(y - x)[lo:len(x) - lo]) < 2e-6 * np.max(np.abs(x)), (tag, "round trip")


# ---------------------------------------------------------------------------------------------------------------------
# C. Signals shorter than the window
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad_mode", ("reflect", "constant"))
@pytest.mark.parametrize("hop", SHORT_HOPS)
@pytest.mark.parametrize("family", ("radix2_64", "mixed_64", "bluestein_22"))
def test_short_signals(family, hop, pad_mode):
    """One ragged batch of the lengths 1 ... n + 1.  np.pad reflects a signal shorter than the padding as often as needed
    (period 2 (Tp - 1)); so does reflect_index of fft.hip."""
    need_gpu()
    from vaenmf import stft as vstft
    n, win, _ = FAMILIES[family]
    wl, F = n / FS, n // 2 + 1
    lens, alone = short_lengths(n)
    xs = [edge_noise(1000 * n + T, T) for T in lens]
    wav = torch.from_numpy(np.concatenate(xs).astype(np.float32)).cuda()
    X, fc = vstft.stft_batch(wav, lens, FS, wl, hop, win=win, pad_mode=pad_mode)
    Xb = np.ascontiguousarray(X[:, :F].cpu().numpy()).view(np.complex64)[..., 0]
    assert fc == [ref_geometry(T, FS, wl, hop)[3] for T in lens]
    o, bad = 0, []
    for T, x, nfr in zip(lens, xs, fc):
        Xr = ref_stft(x, fs=FS, wlen_sec=wl, win=win, hop_percent=hop, pad_mode=pad_mode)
        Xu = Xb[o:o + nfr].T
        assert Xu.shape == Xr.shape
        if np.max(np.abs(Xu - Xr)) > 2e-7 * np.max(np.abs(Xr)):
            bad.append(T)
        if T in alone:
            assert np.array_equal(vstft.stft(x, fs=FS, wlen_sec=wl, win=win, hop_percent=hop, pad_mode=pad_mode), Xu), T
        o += nfr
    assert not bad, ("lengths whose spectrogram is not the restatement's", bad)


@pytest.mark.parametrize("family", ("radix2_64", "mixed_64", "bluestein_22"))
def test_a_single_padded_sample_is_repeated(family):
    """End-padded length 1 (the geometry entry gives every one-sample signal a longer one, the C entry takes it): np.pad
    repeats the sample."""
    need_gpu()
    from vaenmf import _lib
    from vaenmf._lib import check, lib
    from vaenmf.engine import _ptr, _stream
    from vaenmf.stft import _window
    n, win, _ = FAMILIES[family]
    F = n // 2 + 1
    Fs = (F + 15) // 16 * 16
    dev = torch.device("cuda:0")
    wav = torch.tensor([0.75], dtype=torch.float32, device=dev)
    soff = torch.tensor([0, 1], dtype=torch.int64, device=dev)
    foff = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    futt = torch.tensor([0], dtype=torch.int32, device=dev)
    plen = torch.tensor([1], dtype=torch.int32, device=dev)
    X = torch.empty(1, Fs, 2, device=dev)
    w = _window(win, n, dev)
    opts = _lib.StftOpts(n, n // 4, 1, _lib.PAD_REFLECT, None if w is None else _ptr(w))
    check(lib().vaenmf_stft_batch_ex(_ptr(wav), 1, _ptr(soff), _ptr(foff), _ptr(futt), _ptr(plen), C.byref(opts), Fs, _ptr(X), _stream()))
    Xu = np.ascontiguousarray(X[:, :F].cpu().numpy()).view(np.complex64)[..., 0]
    y = np.pad(np.array([0.75]), n // 2, mode="reflect")
    _close(Xu[0], np.fft.rfft(y[:n] * orc.hann_periodic(n)))


def test_uncentred_short_signal_is_still_refused():
    from vaenmf import stft as vstft
    for n in (64, 22):
        with pytest.raises(ValueError):
            vstft.stft(np.zeros(n // 2), fs=FS, wlen_sec=n / FS, center=False)


# ---------------------------------------------------------------------------------------------------------------------
# D. The iSTFT as a ragged batch and on exact buffers
# ---------------------------------------------------------------------------------------------------------------------
def _istft_in_arena(arena, specs, lens, n, fill):
    """vaenmf_istft_batch_ex with S, work and wav_out carved from the arena at exact extents."""
    from vaenmf import _lib
    from vaenmf._lib import check, lib
    from vaenmf.engine import _ptr, _stream
    Sd = _pack(specs, fill)
    fc = [s.shape[1] for s in specs]
    S = arena.carve("S", Sd.shape, torch.float32)
    S.copy_(Sd)
    work = arena.carve("work", (Sd.shape[0], n), torch.float32)
    out = arena.carve("wav_out", (sum(lens),), torch.float32)
    soff = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64, device="cuda")
    foff = torch.tensor(np.concatenate([[0], np.cumsum(fc)]), dtype=torch.int32, device="cuda")
    arena.snapshot(["S"])
    opts = _lib.StftOpts(n, n // 4, 1, _lib.PAD_REFLECT, None)
    check(lib().vaenmf_istft_batch_ex(_ptr(S), len(fc), Sd.shape[0], _ptr(soff), _ptr(foff), C.byref(opts), Sd.shape[1], _ptr(work),
                                      _ptr(out), _stream()))
    torch.cuda.synchronize()
    arena.check("vaenmf_istft_batch_ex")
    arena.unchanged(what="vaenmf_istft_batch_ex")
    return out


@pytest.mark.parametrize("n", (64, 400, 22))
def test_inverse_as_a_ragged_batch_on_exact_buffers(n):
    """Three utterances whose output lengths end before the frames do, with them, and 700 samples after them."""
    need_gpu()
    hop = n // 4
    specs = [ref_stft(edge_noise(50 * n + i, T), fs=FS, wlen_sec=n / FS).astype(np.complex64)
             for i, T in enumerate((3 * n + 5, 5 * n, 4 * n + 7))]
    covered = [hop * (s.shape[1] - 1) + n - n // 2 for s in specs]       # the overlap-add's length less the centre trim
    lens = [covered[0] - 37, covered[1], covered[2] + 700]
    ys = _istft(specs, lens, n)
    for u, (S, T, y) in enumerate(zip(specs, lens, ys)):
        alone, = _istft([S], [T], n)
        assert np.array_equal(alone.view(np.int32), y.view(np.int32)), (n, u, "batch differs from the single call")
        _in_bound(y, S, n, "n=%d ragged batch, utterance %d" % (n, u))
    assert not np.any(ys[2][covered[2]:]) and np.any(ys[2][covered[2] - 2:covered[2]])
    ref = torch.from_numpy(np.concatenate(ys))
    for poison in POISON:
        out = _istft_in_arena(Arena(16 << 20, poison, "cuda"), specs, lens, n, 0.0)
        assert same_bits(out.cpu(), ref), (n, poison, "exact buffers")
    # the padding columns F <= f < Fs of S are not read
    for poison, fill in (("nan", np.nan), ("1e30", 1e30)):
        out = _istft_in_arena(Arena(16 << 20, poison, "cuda"), specs, lens, n, fill)
        assert same_bits(out.cpu(), ref), (n, fill, "padding columns of S are used")
        assert same_bits(torch.from_numpy(np.concatenate(_istft(specs, lens, n, fill=fill))), ref)
