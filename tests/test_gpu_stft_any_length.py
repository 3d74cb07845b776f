"""Any-length STFT / iSTFT on the GPU (mixed-radix and Bluestein kernels of fft.hip) against the numpy float64
restatement of librosa's stft / istft (tests/test_stft_any_length_cpu.py, anchored there to the oracle), the new
kernels against the untouched power-of-two ones, and the reference pipeline at its default 50 ms window."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vaenmf_oracle as orc
from em_support import RecordingRNG
from helpers import GOLDEN, need_gpu, nrm_err
from stft_cases import ref_istft, ref_stft

SIZES = (17, 320, 400, 441, 480, 800, 801, 1000, 1031, 1280, 1536, 2401, 3840, 4093, 4096)


def _speech():
    return np.load(GOLDEN + "/metrics_dummy_m2.npz")["a_s"] / 32768.0


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _close(X, Xr, tol=2e-7):
    assert X.shape == Xr.shape, (X.shape, Xr.shape)
    err = np.max(np.abs(X - Xr))
    assert err <= tol * np.max(np.abs(Xr)), (err, np.max(np.abs(Xr)))


def test_default_call_is_the_reference_default():
    """stft(x) with every argument at its default: 800 points at 16 kHz, F = 401."""
    need_gpu()
    from vaenmf import stft as vstft
    x = _speech()
    X = vstft.stft(x)
    assert X.dtype == np.complex64 and X.shape[0] == 401
    _close(X, ref_stft(_f32(x)))


@pytest.mark.parametrize("n", SIZES)
def test_any_length_against_the_restatement(n):
    need_gpu()
    from vaenmf import stft as vstft
    x = _speech()
    wl = n / 16000
    X = vstft.stft(x, fs=16000, wlen_sec=wl)
    assert X.shape[0] == n // 2 + 1
    Xr = ref_stft(_f32(x), wlen_sec=wl)
    _close(X, Xr)
    if n % 2 == 0:
        xr = vstft.istft(X, fs=16000, wlen_sec=wl, max_len=len(x))
        assert xr.dtype == np.float32 and len(xr) == len(x)
        assert np.max(np.abs(xr - x)) < 2e-6
        S = Xr.astype(np.complex64)
        y = vstft.istft(S, fs=16000, wlen_sec=wl, max_len=len(x))
        assert np.max(np.abs(y - ref_istft(S, wlen_sec=wl, max_len=len(x)))) < 2e-6
        # past the input the last frame's tail is divided by its own tiny window-sum-square (both implementations
        # amplify rounding there; the reference's float32 librosa more so): only lengths and the zero fill are compared
        y700 = vstft.istft(S, fs=16000, wlen_sec=wl, max_len=len(x) + 700)
        n_out = n + int(0.25 * n) * (S.shape[1] - 1) - n // 2
        assert len(y700) == len(x) + 700 and np.array_equal(y700[:len(x)], y) and not np.any(y700[n_out:])
        y = vstft.istft(S, fs=16000, wlen_sec=wl)
        assert len(y) == int(0.25 * n) * (S.shape[1] - 1)


@pytest.mark.parametrize("n", (800, 1031))
def test_windows_centring_and_pad_modes(n):
    need_gpu()
    from vaenmf import stft as vstft
    x = _speech()
    wl = n / 16000
    arr = np.random.default_rng(n).uniform(0.2, 1.0, n)
    for win in ("hamming", "blackman", ("kaiser", 8.0), arr):
        for center, pad in ((True, "reflect"), (False, "reflect"), (True, "constant")):
            X = vstft.stft(x, fs=16000, wlen_sec=wl, win=win, center=center, pad_mode=pad)
            Xr = ref_stft(_f32(x), wlen_sec=wl, win=win, center=center, pad_mode=pad)
            _close(X, Xr)
            if n % 2 == 0:
                S = Xr.astype(np.complex64)
                y = vstft.istft(S, fs=16000, wlen_sec=wl, win=win, center=center)
                yr = ref_istft(S, wlen_sec=wl, win=win, center=center)
                lo = 0 if center else n         # uncentred, the first / last n samples lie under window edges only
                assert len(y) == len(yr) and np.max(np.abs(y - yr)[lo:len(y) - lo]) < 2e-6
                y = vstft.istft(X, fs=16000, wlen_sec=wl, win=win, center=center, max_len=len(x))
                assert np.max(np.abs(y - x)[lo:len(x) - lo]) < 2e-6


def test_new_kernels_match_the_power_of_two_kernels():
    """An explicit periodic-Hann array forces the new kernels at 512 / 1024 points; the default call runs the radix-2
    kernels of fft.hip."""
    need_gpu()
    from vaenmf import stft as vstft
    x = _speech()
    for n in (512, 1024):
        wl = n / 16000
        hann = orc.hann_periodic(n)
        X_old = vstft.stft(x, fs=16000, wlen_sec=wl)
        X_new = vstft.stft(x, fs=16000, wlen_sec=wl, win=hann)
        _close(X_new, X_old)
        y_old = vstft.istft(X_old, fs=16000, wlen_sec=wl, max_len=len(x))
        y_new = vstft.istft(X_old, fs=16000, wlen_sec=wl, win=hann, max_len=len(x))
        assert np.max(np.abs(y_new - y_old)) < 2e-6


def test_ragged_batch_equals_single_calls():
    need_gpu()
    from vaenmf import stft as vstft
    from vaenmf.synth import synth_utterance
    lens = [16000, 23457, 8001, 40000, 12345, 31999, 20200]
    xs = [synth_utterance(i, n_samples=T)[2] for i, T in enumerate(lens)]
    wav = torch.from_numpy(np.concatenate(xs).astype(np.float32)).cuda()
    X, fc = vstft.stft_batch(wav, lens, 16000, 50e-3, 0.25)
    Xb = np.ascontiguousarray(X[:, :401].cpu().numpy()).view(np.complex64)[..., 0]
    o = 0
    for x, nfr in zip(xs, fc):
        Xs = vstft.stft(x, fs=16000, wlen_sec=50e-3)
        assert Xs.shape == (401, nfr)
        assert np.array_equal(Xb[o:o + nfr].T, Xs)
        o += nfr


def test_mcem_at_the_reference_default_window():
    """stft (F = 401, the team chain kernel at 26 bin tiles) -> MCEM_M1 with replayed draws -> istft, against the oracle
    run on the oracle's STFT with the same draws (bounds of test_full_run_replay)."""
    need_gpu()
    import vaenmf
    from vaenmf import stft as vstft
    x = _speech()[:24000]
    F, K, niter = 401, 10, 3
    params = orc.xavier_normal_params([F, 32, [128, 128]], seed=3)
    Xo = orc.stft(x, fs=16000, wlen_sec=50e-3).T                       # (N, F)
    rec = RecordingRNG(7)
    o = orc.MCEMOracle("M1", niter, 10, 10, 10, 10, 0.01)
    o.init_parameters(Xo, params, K, 1e-8, rec)                         # records the draws it takes
    c_ref = o.run()
    draws = rec.draws
    vae = vaenmf.VariationalAutoencoder([F, 32, [128, 128]])
    vae.load_state_dict({k: torch.tensor(v) for k, v in params.items()})
    m = vaenmf.MCEM_M1(niter, 10, 10, 10, 10, 0.01, rng="replay")
    X = vstft.stft(x)
    assert X.shape == (F, Xo.shape[0])
    it = iter(draws)
    _r, _n = torch.rand, torch.randn
    torch.rand = lambda *s, **k: torch.tensor(next(it))
    torch.randn = lambda *s, **k: torch.tensor(next(it))
    try:
        m.init_parameters(X=X.T, vae=vae, nmf_rank=K, eps=1e-8, device="cuda:0")
        c = m.run()
    finally:
        torch.rand, torch.randn = _r, _n
    assert np.max(np.abs(c - c_ref) / np.abs(c_ref)) < 2e-4
    assert nrm_err(m.S_hat, o.S_hat) < 2e-3
    s = vstft.istft(m.S_hat, max_len=len(x))
    assert len(s) == len(x) and np.all(np.isfinite(s))


def test_reconstructor_at_50_ms():
    need_gpu()
    from vaenmf import stft as vstft
    from vaenmf.pipeline import Reconstructor
    from vaenmf.synth import synth_utterance
    lens = [16000, 23457, 12001]
    xs = [synth_utterance(10 + i, n_samples=T)[2] for i, T in enumerate(lens)]
    params = orc.xavier_normal_params([401, 32, [128, 128]], seed=0)
    rec = Reconstructor(params, 401, 10, niter=3, fs=16000, wlen_sec=50e-3, precision="bf16x3", max_frames=400, max_utts=4)
    wav = torch.from_numpy(np.concatenate(xs).astype(np.float32)).cuda()
    X, fc = vstft.stft_batch(wav, lens, 16000, 50e-3, 0.25, Fs=rec.eng.Fs)
    Xb = np.ascontiguousarray(X[:, :401].cpu().numpy()).view(np.complex64)[..., 0]
    o = 0
    for x, nfr in zip(xs, fc):
        assert np.array_equal(Xb[o:o + nfr].T, vstft.stft(x, fs=16000, wlen_sec=50e-3))
        o += nfr
    out = rec.enhance(wav, lens)
    s_hat, n_hat = out[0], out[1]
    assert s_hat.shape[0] == sum(lens) and n_hat.shape[0] == sum(lens)
    assert torch.isfinite(s_hat).all() and torch.isfinite(n_hat).all()
    assert float(s_hat.abs().max()) > 0
