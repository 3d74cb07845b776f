"""The resampler's definition restated in numpy (the oracle of tests/test_gpu_resample.py, itself checked against
scipy.signal.resample_poly in tests/test_resample_cpu.py) and the cases both test files share.

With M = max(up, down) after reducing the ratio, half = zeros M:
  h[i] = up s[i] w[i] / sum(s w),  t = i - half,  s = sin(pi t / M) / (pi t),  w = I0(beta sqrt(1 - (t/half)^2)) / I0(beta)
  y[m] = sum_n x[n] h[half + m down - n up],  n in [0, n_in), tap index in [0, 2 half],  n_out = ceil(n_in up / down)
summed in float64 in ascending n."""
import math

import numpy as np

RATIOS = [(1, 3), (2, 1), (4, 6), (160, 441), (441, 160), (640, 441), (1, 1)]      # 4/6: the library reduces it to 2/3
LENGTHS = [1, 2, 7, 441, 1001, 4410, 0, 4411]
SCALES = [1.0, 3e4]
TAP_CASES = [(1, 3, 10, 5.0), (2, 1, 10, 5.0), (2, 3, 10, 5.0), (160, 441, 10, 5.0), (441, 160, 10, 5.0), (640, 441, 10, 5.0),
             (2, 3, 10, 8.6), (2, 3, 16, 5.0)]


def reduced(up, down):
    g = math.gcd(up, down)
    return up // g, down // g


def out_length(n_in, up, down):
    return -((-n_in * up) // down)


def taps(up, down, zeros=10, beta=5.0):
    """The 2 half + 1 taps for up / down as given (float64)."""
    M = max(up, down)
    half = zeros * M
    t = np.arange(-half, half + 1, dtype=np.float64)
    s = np.sinc(t / M) / M                                           # sin(pi t / M) / (pi t), 1 / M at t = 0
    w = np.i0(beta * np.sqrt(1.0 - (t / half) ** 2)) / np.i0(beta)
    return up * s * w / np.sum(s * w)


def resample_ref(x, up, down, zeros=10, beta=5.0, h=None):
    """float64 [ceil(n up / down)]: the closed form, every output summed in ascending n."""
    up, down = reduced(up, down)
    x = np.asarray(x, dtype=np.float64)
    n_in = len(x)
    if up == down:
        return x.copy()
    half = zeros * max(up, down)
    if h is None:
        h = taps(up, down, zeros, beta)
    m = np.arange(out_length(n_in, up, down), dtype=np.int64)
    c = half + m * down
    q, p = c // up, c % up
    y = np.zeros(len(m))
    for j in range(2 * half // up, -1, -1):                          # n = q - j grows as j falls
        n, k = q - j, p + j * up
        ok = (n >= 0) & (n < n_in) & (k <= 2 * half)
        y[ok] += x[n[ok]] * h[k[ok]]
    return y


def batch_inputs(scale, seed=0):
    """One Gaussian signal per entry of LENGTHS (float32)."""
    g = np.random.default_rng(seed)
    return [(scale * g.standard_normal(n)).astype(np.float32) for n in LENGTHS]
