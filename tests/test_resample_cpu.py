"""Host side of the resampler (vaenmf_resample_ratio / _length / _taps) and the numpy oracle of the GPU tests; no GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import resample_cases as rc
from vaenmf import _lib


def _ratio(fs_in, fs_out):
    up, down = C.c_int32(), C.c_int32()
    return _lib.lib().vaenmf_resample_ratio(fs_in, fs_out, C.byref(up), C.byref(down)), up.value, down.value


def test_ratio_and_length():
    lib = _lib.lib()
    for fs_in, fs_out in [(48000, 16000), (44100, 16000), (16000, 44100), (11025, 16000), (16000, 16000), (32000, 48000)]:
        g = math.gcd(fs_in, fs_out)
        code, up, down = _ratio(fs_in, fs_out)
        assert (code, up, down) == (0, fs_out // g, fs_in // g)
        for n in [0, 1, 2, 7, 440, 441, 442, 64000]:
            assert lib.vaenmf_resample_length(n, up, down) == math.ceil(n * up / down) == rc.out_length(n, up, down)
    assert _ratio(11025, 16000)[1:] == (640, 441)
    for bad in [(0, 16000), (16000, 0), (-8000, 16000)]:
        assert _ratio(*bad)[0] != 0
        assert b"positive" in lib.vaenmf_last_error()
    assert _ratio(16000, 16001)[0] != 0                                  # 16001/16000: over the limit
    assert b"1024" in lib.vaenmf_last_error()
    assert lib.vaenmf_resample_length(-1, 1, 3) < 0 and lib.vaenmf_resample_length(5, 0, 3) < 0


def test_python_rate_checks():
    from vaenmf.resample import ratio
    assert ratio(48000, 16000) == (1, 3) and ratio(16000.0, 44100) == (441, 160)
    for bad in [44100.5, 0, -16000, "16000", None, True]:
        with pytest.raises(ValueError):
            ratio(bad, 16000)
    with pytest.raises(NotImplementedError, match="1024"):
        ratio(16000, 16001)


@pytest.mark.parametrize("up,down,zeros,beta", rc.TAP_CASES)
def test_taps_against_scipy(up, down, zeros, beta):
    """vaenmf_resample_taps (long double, rounded once) against up * scipy.signal.firwin(2 half + 1, 1 / M, window=('kaiser',
    beta)): max |h_lib - h_scipy| <= 4e-15 max|h|.  scipy's own taps lie within 7.8e-16 max|h| of a 40-digit evaluation for
    these ratios and the rounding of the long-double table adds about one ulp; the bound is about five times that.
    Measured: between 8.3e-17 (2/1) and 1.0e-15 (441/160) times max|h| over the eight cases."""
    from scipy.signal import firwin
    from vaenmf.resample import taps
    M = max(up, down)
    half = zeros * M
    h = taps(up, down, zeros, beta)
    ref = up * firwin(2 * half + 1, 1.0 / M, window=("kaiser", beta))
    err = np.max(np.abs(h - ref)) / np.max(np.abs(ref))
    print("taps %d/%d zeros %d beta %g: max|h_lib - h_scipy| = %.2e max|h|" % (up, down, zeros, beta, err))
    assert h.shape == ref.shape
    assert err <= 4e-15
    assert np.array_equal(h.view(np.int64), h[::-1].view(np.int64))      # h[i] == h[2 half - i], bit for bit
    assert abs(np.sum(h) - up) <= 1e-13
    assert np.max(np.abs(rc.taps(up, down, zeros, beta) - ref)) <= 4e-15 * np.max(np.abs(ref))   # the oracle's own taps


def test_taps_refusals():
    lib = _lib.lib()
    h = np.empty(2 * 10 * 1025 + 1)
    for args in [(0, 1, 10, 5.0), (1, 3, 0, 5.0), (1, 3, 10, -1.0), (1, 3, 10, float("nan")), (1025, 1, 10, 5.0)]:
        assert lib.vaenmf_resample_taps(*args, h.ctypes.data) != 0


@pytest.mark.parametrize("up,down", rc.RATIOS)
def test_closed_form_against_scipy(up, down):
    """The numpy oracle against scipy.signal.resample_poly on float64 inputs, <= 1e-14 max|x|, over the GPU test's grid."""
    from scipy.signal import resample_poly
    g = np.random.default_rng(5)
    worst = 0.0
    for n in rc.LENGTHS:
        x = g.standard_normal(n)
        y = rc.resample_ref(x, up, down)
        assert y.shape == (rc.out_length(n, *rc.reduced(up, down)),)
        if n == 0:
            continue                                                     # nothing to compare: scipy takes no empty signal
        ref = resample_poly(x, up, down, window=("kaiser", 5.0))
        assert ref.shape == y.shape
        err = np.max(np.abs(y - ref)) / np.max(np.abs(x))
        worst = max(worst, err)
        assert err <= 1e-14, (n, err)
    print("closed form %d/%d: worst |y - scipy| = %.2e max|x|" % (up, down, worst))
