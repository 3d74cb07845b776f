"""Any-length STFT / iSTFT, host side (no GPU): frame geometry for every n_fft in [16, 4096], center on and off, the
rejections, and the numpy float64 restatement of librosa's stft / istft that the GPU tests measure against.  The
restatement is anchored here to the oracle, which is pinned to the reference's own committed spectrograms."""
import numpy as np
import pytest

import vaenmf_oracle as orc
from helpers import GOLDEN
from stft_cases import ref_geometry, ref_istft, ref_stft


def _speech():
    return np.load(GOLDEN + "/metrics_dummy_m2.npz")["a_s"] / 32768.0


def test_restatement_agrees_with_the_oracle():
    """At 512 and 1024 points (periodic Hann, center, reflect) the restatement equals oracle.stft / oracle.istft, which
    the oracle's own tests pin to the reference's committed spectrograms."""
    x = _speech()
    for wlen in (32e-3, 64e-3):
        X = ref_stft(x, wlen_sec=wlen, hop_percent=0.25)
        Xo = orc.stft(x, fs=16000, wlen_sec=wlen, hop_percent=0.25)
        assert X.shape == Xo.shape
        assert np.max(np.abs(X - Xo)) < 2e-7 * np.max(np.abs(X))
        for T in (len(x), len(x) + 700):
            y = ref_istft(Xo, wlen_sec=wlen, hop_percent=0.25, max_len=T)
            yo = orc.istft(Xo, fs=16000, wlen_sec=wlen, hop_percent=0.25, max_len=T)
            assert len(y) == T and np.max(np.abs(y - yo)) < 1e-6
        assert len(ref_istft(Xo, wlen_sec=wlen)) == len(orc.istft(Xo, fs=16000, wlen_sec=wlen))
        assert np.max(np.abs(ref_istft(X, wlen_sec=wlen, max_len=len(x)) - x)) < 1e-12


def test_restatement_round_trip_other_windows():
    """The restatement inverts itself for lengths and windows the oracle does not take (so it is not vacuous there)."""
    x = _speech()[:20000]
    for n, win, center, pad in ((800, "hann", True, "reflect"), (1000, "hamming", False, "reflect"),
                                (640, ("kaiser", 8.0), True, "constant")):
        X = ref_stft(x, wlen_sec=n / 16000, win=win, center=center, pad_mode=pad)
        y = ref_istft(X, wlen_sec=n / 16000, win=win, center=center, max_len=len(x))
        lo = 0 if center else n                     # without centring the first / last samples see one frame only
        assert np.max(np.abs(y - x)[lo:len(x) - lo]) < 1e-10


def test_frame_geometry_any_length():
    from vaenmf.stft import frame_geometry
    cases = [(16000, n / 16000) for n in (320, 400, 800, 801, 1031, 1280, 2400, 4096)] + [(44100, 10e-3)]
    for fs, wlen in cases:
        for T in (16000, 16001, 40000, 64000, 70001):
            for center in (True, False):
                nfft, hop, Tp, nfr = ref_geometry(T, fs, wlen, 0.25, center)
                assert frame_geometry(T, fs, wlen, 0.25, center) == (nfft, hop, nfr, Tp), (fs, wlen, T, center)
            assert frame_geometry(T, fs, wlen, 0.25) == frame_geometry(T, fs, wlen, 0.25, True)
    assert frame_geometry(44100, 44100, 10e-3, 0.25)[0] == 441


def test_frame_counts_match_the_restated_stft():
    from vaenmf.stft import frame_geometry
    x = np.zeros(20011)
    for n in (17, 441, 801, 1031):
        for center in (True, False):
            assert frame_geometry(len(x), 16000, n / 16000, 0.25, center)[2] == \
                ref_stft(x, wlen_sec=n / 16000, center=center).shape[1]


def test_rejections():
    from vaenmf import stft as vstft
    for n in (8, 4097):
        with pytest.raises(NotImplementedError):
            vstft.frame_geometry(64000, 16000, n / 16000, 0.25)
        with pytest.raises(NotImplementedError):
            vstft.frame_geometry(64000, 16000, n / 16000, 0.25, center=False)
    with pytest.raises(ValueError):
        vstft.frame_geometry(64000, 16000, 50.01e-3, 0.25)          # stft.py:37-38
    with pytest.raises(ValueError):
        vstft.frame_geometry(500, 16000, 50e-3, 0.25, center=False)  # 700 samples after the end pad < n_fft


def test_istft_odd_window_rejected_before_the_device():
    """librosa infers n_fft = 2 (F - 1) and rejects win_length = n_fft + 1, so the reference's istft fails on odd
    windows; so does this one, without touching the GPU (this test runs on hosts without one)."""
    from vaenmf import stft as vstft
    S = np.zeros((401, 10), np.complex64)
    with pytest.raises(ValueError):
        vstft.istft(S, fs=16000, wlen_sec=801 / 16000)
    with pytest.raises(NotImplementedError):
        vstft.istft(np.zeros((5, 10), np.complex64), fs=16000, wlen_sec=8 / 16000)


def test_stft_option_rejections_before_the_device():
    from vaenmf import stft as vstft
    x = np.zeros(16000)
    with pytest.raises(NotImplementedError):
        vstft.stft(x, pad_mode="edge")
    with pytest.raises(NotImplementedError):
        vstft.stft(x, pad_at_end=False)
    with pytest.raises(NotImplementedError):
        vstft.stft(x, wlen_sec=4097 / 16000)
