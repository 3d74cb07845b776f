"""Shared by the STFT tests, CPU and GPU: the numpy float64 restatement of librosa's stft / istft (anchored to the oracle
in tests/test_stft_any_length_cpu.py) and the check against the reference's committed train / validation spectrograms."""
import math
import os

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


def ref_istft(S, fs=16000, wlen_sec=50e-3, win="hann", hop_percent=0.25, center=True, max_len=None):
    """stft.py:66-102 -> librosa.core.istft in float64: irfft, synthesis window, overlap-add, division by the window's
    sum of squares where it exceeds float32's tiny, n_fft//2 trimmed when centred, fixed to max_len."""
    nfft = int(wlen_sec * fs)
    hop = int(hop_percent * nfft)
    nfr = S.shape[1]
    w = ref_window(win, nfft)
    frames = np.fft.irfft(np.asarray(S).T, n=nfft, axis=1) * w[None, :]
    n_out = nfft + hop * (nfr - 1)
    y, wss = np.zeros(n_out), np.zeros(n_out)
    for i in range(nfr):
        y[i * hop:i * hop + nfft] += frames[i]
        wss[i * hop:i * hop + nfft] += w * w
    nz = wss > TINY
    y[nz] /= wss[nz]
    start = nfft // 2 if center else 0
    if max_len is None:
        return y[start:n_out - start]
    y = y[start:start + max_len]
    return np.pad(y, (0, max_len - len(y)))


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
