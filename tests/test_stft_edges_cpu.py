"""STFT / iSTFT edges, host side (no GPU): the float64 restatement of tests/stft_cases.py anchored to the oracle where
tests/test_gpu_stft_edges.py takes it -- hops other than a quarter window, signals shorter than the window -- its
per-sample error terms against a dense computation, and vaenmf_stft_geometry (a host call) over every short length."""
import numpy as np
import pytest

import vaenmf_oracle as orc
from stft_cases import (EDGE_FS, EDGE_HOPS, SHORT_HOPS, TINY, edge_noise, istft_bound, ref_geometry, ref_istft, ref_istft_terms,
                        ref_stft, short_lengths)

FS = EDGE_FS


def _same(a, b, what):
    """float64 against float64: the two differ by the order of a few additions at most."""
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.max(np.abs(a - b)) <= 1e-12 * max(np.max(np.abs(b)), 1e-300), (what, np.max(np.abs(a - b)))


@pytest.mark.parametrize("hop", (0.5, 0.125, 0.3))
@pytest.mark.parametrize("n", (64, 400, 22, 17))
def test_restatement_agrees_with_the_oracle_at_other_hops(n, hop):
    x = edge_noise(100 + n, 6 * n + 3)
    wl = n / FS
    X = ref_stft(x, wlen_sec=wl, hop_percent=hop)
    _same(X, orc.stft(x, fs=FS, wlen_sec=wl, hop_percent=hop, dtype="complex128"), "stft")
    for T in (None, len(x), len(x) + 700, 2 * n + 1):
        _same(ref_istft(X, wlen_sec=wl, hop_percent=hop, max_len=T),
              orc.istft(X, fs=FS, wlen_sec=wl, hop_percent=hop, max_len=T, dtype="float64"), ("istft", T))
    if n % 2 == 0:
        assert np.max(np.abs(ref_istft(X, wlen_sec=wl, hop_percent=hop, max_len=len(x)) - x)) < 1e-12 * np.max(np.abs(x))


@pytest.mark.parametrize("hop", SHORT_HOPS)
@pytest.mark.parametrize("n", (64, 22))
def test_restatement_agrees_with_the_oracle_on_short_signals(n, hop):
    """T = 1 ... n + 1: np.pad reflects such a signal several times, in the oracle and in the restatement alike."""
    wl = n / FS
    for T in short_lengths(n)[0]:
        x = edge_noise(1000 * n + T, T)
        X = ref_stft(x, wlen_sec=wl, hop_percent=hop)
        _same(X, orc.stft(x, fs=FS, wlen_sec=wl, hop_percent=hop, dtype="complex128"), ("stft", T))
        assert X.shape[1] == ref_geometry(T, FS, wl, hop)[3]
        _same(ref_istft(X, wlen_sec=wl, hop_percent=hop, max_len=T + 9),
              orc.istft(X, fs=FS, wlen_sec=wl, hop_percent=hop, max_len=T + 9, dtype="float64"), ("istft", T))


@pytest.mark.parametrize("hop", EDGE_HOPS)
def test_restated_frame_counts_are_the_oracles(hop):
    for n in (64, 22):
        for T in range(1, 201):
            assert orc.stft(np.zeros(T), fs=FS, wlen_sec=n / FS, hop_percent=hop).shape[1] == ref_geometry(T, FS, n / FS, hop)[3], (n, T)


@pytest.mark.parametrize("center", (True, False))
@pytest.mark.parametrize("hop", (0.25, 0.3, 1.0, 1.25))
def test_error_terms_against_a_dense_computation(hop, center):
    """y, A, k and wss of ref_istft_terms at n = 16: every (frame, sample) pair visited, nothing sliced."""
    n, nfr = 16, 7
    g = np.random.default_rng(5)
    S = g.standard_normal((n // 2 + 1, nfr)) + 1j * g.standard_normal((n // 2 + 1, nfr))
    w = orc.hann_periodic(n)
    h = int(hop * n)
    n_out = n + h * (nfr - 1)
    fr = np.fft.irfft(S.T, n=n, axis=1)
    num, A, k, wss = np.zeros(n_out), np.zeros(n_out), np.zeros(n_out, dtype=np.int64), np.zeros(n_out)
    for p in range(n_out):
        for i in range(nfr):
            t = p - i * h
            if 0 <= t < n:
                num[p] += fr[i, t] * w[t]
                A[p] += abs(fr[i, t] * w[t])
                wss[p] += w[t] * w[t]
                k[p] += 1
    div = np.where(wss > TINY, wss, 1.0)
    lo = n // 2 if center else 0
    max_len = n_out + 5
    r = ref_istft_terms(S, wlen_sec=n / FS, win=w, hop_percent=hop, center=center, max_len=max_len)
    pad = lambda v: np.pad(v[lo:], (0, max_len - (n_out - lo)))
    assert np.allclose(r.y, pad(num / div), rtol=1e-13, atol=0) and np.allclose(r.A, pad(A / div), rtol=1e-13, atol=0)
    assert np.array_equal(r.k, pad(k)) and np.allclose(r.wss, pad(wss), rtol=1e-13, atol=0)
    assert r.scale == np.max(np.abs(fr)) and not np.any(r.k[n_out - lo:]) and not np.any(r.y[n_out - lo:])
    if hop >= 1.0:
        assert np.any((r.wss <= TINY) & (r.k > 0)) and (hop == 1.0 or np.any(r.k[:n_out - lo] == 0))
    assert np.all(istft_bound(r) >= 1e-12 * r.scale) and np.all(r.A >= np.abs(r.y) * (1 - 1e-13))
    short = ref_istft_terms(S, wlen_sec=n / FS, win=w, hop_percent=hop, center=center)
    assert len(short.y) == n_out - 2 * lo and np.array_equal(short.y, r.y[:n_out - 2 * lo])


@pytest.mark.parametrize("n", (64, 400))
def test_geometry_entry_over_short_lengths_and_hops(n):
    """vaenmf_stft_geometry against ref_geometry for T = 1 ... 2000 at every hop, centred and not."""
    from vaenmf.stft import frame_geometry
    wl = n / FS
    for hop in EDGE_HOPS + (0.25,):
        for center in (True, False):
            for T in range(1, 2001):
                nfft, h, Tp, nfr = ref_geometry(T, FS, wl, hop, center)
                if not center and Tp < nfft:
                    with pytest.raises(ValueError):
                        frame_geometry(T, FS, wl, hop, center)
                else:
                    assert frame_geometry(T, FS, wl, hop, center) == (nfft, h, nfr, Tp), (n, hop, center, T)


def test_a_hop_of_zero_samples_is_refused():
    from vaenmf.stft import frame_geometry
    assert int(0.05 * 17) == 0
    with pytest.raises(NotImplementedError, match="hop must be positive"):
        frame_geometry(100, FS, 17 / FS, 0.05)
    assert frame_geometry(100, FS, 22 / FS, 0.05)[1] == 1
