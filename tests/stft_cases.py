"""Shared by the STFT tests, CPU and GPU: the numpy float64 restatement of librosa's stft / istft (anchored to the oracle
in tests/test_stft_any_length_cpu.py) and the check against the reference's committed train / validation spectrograms."""
import math
import os
from collections import namedtuple

import numpy as np

from helpers import GOLDEN

TINY = np.finfo(np.float32).tiny


def ref_window(win, nfft):
    """librosa.filters.get_window(win, nfft, fftbins=True)."""
    if isinstance(win, (str, tuple)):
        from scipy.signal import get_window
        return get_window(win, nfft, fftbins=True)
    w = np.asarray(win, dtype=np.float64)
    assert w.shape == (nfft,), (w.shape, nfft)
    return w


def ref_geometry(T, fs, wlen_sec, hop_percent, center=True):
    """(nfft, hop, end-padded length, n_frames): stft.py:37-53, then librosa's frame count."""
    nfft = int(wlen_sec * fs)
    hop = int(hop_percent * nfft)
    utt_len = T / fs
    Tp = T + (hop if math.ceil(utt_len / wlen_sec / hop_percent) != int(utt_len / wlen_sec / hop_percent) else 0)
    L = Tp + 2 * (nfft // 2) if center else Tp
    return nfft, hop, Tp, 1 + (L - nfft) // hop


def ref_stft(x, fs=16000, wlen_sec=50e-3, win="hann", hop_percent=0.25, center=True, pad_mode="reflect"):
    """stft.py:16-63 -> librosa.core.stft in float64: end pad, np.pad by n_fft//2 in `pad_mode` when centred,
    frames at hop, window, rfft.  Returns complex128 (n_fft//2+1, n_frames)."""
    nfft, hop, Tp, nfr = ref_geometry(len(x), fs, wlen_sec, hop_percent, center)
    y = np.pad(np.asarray(x, dtype=np.float64), (0, Tp - len(x)), mode="constant")
    if center:
        y = np.pad(y, nfft // 2, mode=pad_mode)
    idx = np.arange(nfft)[None, :] + hop * np.arange(nfr)[:, None]
    return np.fft.rfft(y[idx] * ref_window(win, nfft)[None, :], axis=1).T


IstftTerms = namedtuple("IstftTerms", "y A k wss scale")


def ref_istft_terms(S, fs=16000, wlen_sec=50e-3, win="hann", hop_percent=0.25, center=True, max_len=None, hop=None):
    """stft.py:66-102 -> librosa.core.istft in float64: irfft, synthesis window, overlap-add, division by the window's
    sum of squares where it exceeds float32's tiny, n_fft//2 trimmed when centred, fixed to max_len.  Beside the output y,
    per output sample: A = sum_i |frame_i[t] w| / wss (undivided where y is), the number k of frames over the sample and
    wss itself (k = 0, A = 0, wss = 0 past the last frame); scale = max |frame| before the window.  hop: in samples,
    instead of hop_percent."""
    nfft = int(wlen_sec * fs)
    hop = int(hop_percent * nfft) if hop is None else int(hop)
    nfr = S.shape[1]
    w = ref_window(win, nfft)
    raw = np.fft.irfft(np.asarray(S, dtype=np.complex128).T, n=nfft, axis=1)    # numpy transforms complex64 in single precision
    frames = raw * w[None, :]
    n_out = nfft + hop * (nfr - 1)
    y, wss, A, k = np.zeros(n_out), np.zeros(n_out), np.zeros(n_out), np.zeros(n_out, dtype=np.int64)
    for i in range(nfr):
        y[i * hop:i * hop + nfft] += frames[i]
        wss[i * hop:i * hop + nfft] += w * w
        A[i * hop:i * hop + nfft] += np.abs(frames[i])
        k[i * hop:i * hop + nfft] += 1
    nz = wss > TINY
    y[nz] /= wss[nz]
    A[nz] /= wss[nz]
    start = nfft // 2 if center else 0

    def fix(v):
        if max_len is None:
            return v[start:n_out - start]
        v = v[start:start + max_len]
        return np.pad(v, (0, max_len - len(v)))
    return IstftTerms(fix(y), fix(A), fix(k), fix(wss), float(np.max(np.abs(raw))))


def ref_istft(S, fs=16000, wlen_sec=50e-3, win="hann", hop_percent=0.25, center=True, max_len=None):
    """The output of ref_istft_terms alone."""
    return ref_istft_terms(S, fs, wlen_sec, win, hop_percent, center, max_len).y


def istft_bound(r):
    """Per-sample bound on |y - r.y| for the iSTFT kernels, from their roundings: each windowed frame sample is rounded once
    to float32 in `work` (2^-24 A in all), the radix-2 overlap-add sums its k terms one after another in float32 (k - 1
    roundings of partial sums that |.| bounds by A wss; the table path sums in double), the output is rounded once
    (2^-24 |y|); (k + 1) A leaves one A of slack.  The last term is float64 noise of the transform against numpy's."""
    return 2.0 ** -24 * ((r.k + 1) * r.A + np.abs(r.y)) + 1e-12 * r.scale


def istft_error_over_bound(y, r):
    """max over the samples of |y - r.y| / istft_bound(r).  Where no frame covers a sample, or the window's sum of
    squares does not exceed float32's tiny (no division: under the first sample of a Hann window, which is 0.0 in every
    table), the restatement's value is an exact zero and y must equal it."""
    y = np.asarray(y, dtype=np.float64)
    assert y.shape == r.y.shape, (y.shape, r.y.shape)
    exact = (r.k == 0) | (r.wss <= TINY)
    assert np.array_equal(y[exact], r.y[exact]), ("undivided / uncovered samples differ", np.flatnonzero(exact & (y != r.y))[:8])
    assert not np.any(r.y[r.k == 0])
    return float(np.max(np.abs(y - r.y) / istft_bound(r)))


# Cases of tests/test_gpu_stft_edges.py and tests/test_stft_edges_cpu.py
EDGE_FS = 16000
EDGE_HOPS = (0.5, 0.125, 0.3, 0.05, 1.0, 1.25)      # a quarter window is what every other STFT test uses
SHORT_HOPS = (0.25, 0.125, 0.5)
BLUESTEIN_EVEN = (22, 34, 802, 2046, 2050, 4094)    # convolution lengths 64, 128, 2048, 4096 (2n - 1 = 4091), 8192, 8192
ODD_SIZES = (17, 21, 441, 1031, 4093)               # 21 = 3 x 7 and 441 = 3^2 7^2 are mixed radix, the others Bluestein


def edge_rate(n):
    """(fs, wlen_sec) with wlen_sec * fs == n in floating point: 16 kHz, or 8 n Hz and an eighth of a second where
    n / 16000 * 16000 rounds below n (2046) and stft.py:37-38 would refuse the window."""
    fs, wl = (EDGE_FS, n / EDGE_FS) if n / EDGE_FS * EDGE_FS == n else (8 * n, 0.125)
    assert wl * fs == n and int(wl * fs) == n
    return fs, wl


def edge_noise(seed, T):
    """Seeded unit-scale noise as the float32 values the GPU gets, in float64."""
    return np.random.default_rng(seed).standard_normal(T).astype(np.float32).astype(np.float64)


def random_window(n):
    """The explicit non-Hann window of tests/test_gpu_stft_any_length.py."""
    return np.random.default_rng(n).uniform(0.2, 1.0, n)


def short_lengths(n):
    """Every length from one sample to n + 1, and the five of them that also run alone: among them lengths at which a
    position bounces more than once (end-padded length <= n / 2)."""
    return list(range(1, n + 2)), {64: (1, 5, 16, 32, 65), 22: (1, 2, 3, 5, 23)}[n]


def check_stft_tr_dt(stft_fn, tol_rel):
    """The reference's two other golden STFT outputs (si_tr_s_frames.p (513, 972), si_dt_05_frames.p (513, 976): same test
    recipe, tests/dataset/test_csr1_wjs0_dataset.py:17-83): first two utterances of each set."""
    z = np.load(os.path.join(GOLDEN, "stft_frames_tr_dt.npz"))
    for tag in ("tr", "dt"):
        cn = z[tag + "_frame_counts"]
        for which, n_fr in (("a", int(cn[0])), ("b", int(cn[1]))):
            x = z["%s_pcm_%s" % (tag, which)].astype(np.float64) / 32768.0
            x = x[int(0.1 * 16000):]
            x = x / np.max(np.abs(x))
            P = np.power(np.abs(stft_fn(x)), 2)
            assert P.shape == (513, n_fr), (tag, which, P.shape)
            if which == "a":
                head, tail, cs = z[tag + "_head"], z[tag + "_tail"], z[tag + "_col_sums"]
                scale = np.max(head)
                eh, et = np.max(np.abs(P[:, :48] - head)), np.max(np.abs(P[:, n_fr - 48:] - tail))
                assert eh < 2e-7 * scale and et < 2e-7 * max(scale, np.max(tail)), (tag, which, "head / tail, absolute", eh, et, scale)
                big = head > 1e-6 * scale
                er = np.max(np.abs(P[:, :48][big] / head[big] - 1))
                assert er < tol_rel, (tag, which, "head, relative", er, tol_rel)
            else:
                fb, cs = z[tag + "_first_b"], z[tag + "_col_sums_b"]
                ef = np.max(np.abs(P[:, :4] - fb))
                assert ef < 2e-7 * max(np.max(fb), 1e-30) + 1e-12, (tag, which, "first frames", ef, np.max(fb))
            es = np.max(np.abs(P.sum(0, dtype=np.float64) / cs - 1))
            assert es < 1e-6, (tag, which, "column sums", es)
