"""STOI / ESTOI in plain float64 numpy: the checker of vaenmf_stoi_* (tests only, never on the product path), written
from the published algorithm (Taal et al. 2011; Jensen & Taal 2016) as include/vaenmf.h states it, and the cases the
CPU and GPU tests share.

  core(x, y, extended)   10 kHz signals -> dict with every intermediate: norms, energies (dB), keep, src, k, tob_x, tob_y
                         [15][M], seg (per-segment sums), d, counts = (n_frames, k, J) and margin, the distance in dB of
                         the closest frame to the 40 dB threshold (what decides whether float-level differences can flip
                         a keep decision)
  score(x, y, fs, ...)   the same after scipy.signal.resample_poly to 10 kHz, rounded to float32 as the library's
                         resampler rounds

Deviations from pystoi, as in the library: no dither (a row or column of norm exactly zero is scaled by 0), and the
rate change uses scipy's default Kaiser filter."""
import os
from fractions import Fraction

import numpy as np

FS, N_FRAME, HOP, NFFT, N_BANDS, MIN_FREQ, N_SEG, BETA, DYN_RANGE = 10000, 256, 128, 512, 15, 150.0, 30, -15.0, 40.0
EPS = 2.0 ** -52
NO_SCORE = 1e-5            # pystoi's value when there are fewer than 30 frames
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def window():
    """The symmetric Hann of 258 points without its two zero ends (pystoi: np.hanning(258)[1:-1])."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(N_FRAME, dtype=np.float64) + 1.0) / (N_FRAME + 1))


def n_frames_of(T):
    return len(range(0, int(T) - N_FRAME, HOP))


def geometry(T):
    """(n_frames, max_spec_frames, max_segments) of T samples at 10 kHz."""
    nf = n_frames_of(T)
    ms = max(nf - 1, 0)
    return nf, ms, max(ms - (N_SEG - 1), 0)


def bands():
    """(lo, hi) [15]: the bins of the grid 10000 i / 512 nearest to the third-octave band edges."""
    f = np.linspace(0.0, FS, NFFT + 1)[:NFFT // 2 + 1]
    b = np.arange(N_BANDS, dtype=np.float64)
    fl = MIN_FREQ * 2.0 ** ((2.0 * b - 1.0) / 6.0)
    fh = MIN_FREQ * 2.0 ** ((2.0 * b + 1.0) / 6.0)
    lo = np.array([int(np.argmin((f - v) ** 2)) for v in fl], np.int32)
    hi = np.array([int(np.argmin((f - v) ** 2)) for v in fh], np.int32)
    return lo, hi


def _rebuild(s, src, w):
    k = len(src)
    out = np.zeros((k - 1) * HOP + N_FRAME)
    for q, j in enumerate(src):
        out[q * HOP:q * HOP + N_FRAME] += w * s[j * HOP:j * HOP + N_FRAME]
    return out


def _tob(s, w, lo, hi):
    starts = range(0, len(s) - N_FRAME, HOP)
    out = np.zeros((N_BANDS, len(starts)))
    for m, i in enumerate(starts):
        p = np.abs(np.fft.rfft(w * s[i:i + N_FRAME], NFFT)) ** 2
        for b in range(N_BANDS):
            out[b, m] = np.sqrt(p[lo[b]:hi[b]].sum())
    return out


def _unit(v, axis):
    """Subtract the mean along axis and divide by the 2-norm; a norm of exactly zero scales by 0."""
    v = v - v.mean(axis=axis, keepdims=True)
    n = np.sqrt((v * v).sum(axis=axis, keepdims=True))
    return v * np.where(n > 0.0, 1.0 / np.where(n > 0.0, n, 1.0), 0.0)


def segment_sum(xs, ys, extended):
    """One segment [15][30] of each signal -> its sum (ESTOI: sum x_n y_n; STOI: the 15 row correlations)."""
    if extended:
        xn = _unit(_unit(xs, 1), 0)
        yn = _unit(_unit(ys, 1), 0)
        return float((xn * yn).sum())
    clip = 1.0 + 10.0 ** (-BETA / 20.0)
    c = np.sqrt((xs * xs).sum(1, keepdims=True)) / (np.sqrt((ys * ys).sum(1, keepdims=True)) + EPS)
    yp = np.minimum(c * ys, xs * clip)
    xm = xs - xs.mean(1, keepdims=True)
    ym = yp - yp.mean(1, keepdims=True)
    xm = xm / (np.sqrt((xm * xm).sum(1, keepdims=True)) + EPS)
    ym = ym / (np.sqrt((ym * ym).sum(1, keepdims=True)) + EPS)
    return float((xm * ym).sum())


def core(x, y, extended=True):
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    assert x.shape == y.shape and x.ndim == 1
    w = window()
    lo, hi = bands()
    nf = n_frames_of(len(x))
    r = dict(n_frames=nf, k=0, M=0, J=0, d=NO_SCORE, margin=np.inf, keep=np.zeros(0, np.int32), src=np.zeros(0, np.int32),
             norms=np.zeros(0), energies=np.zeros(0), tob_x=np.zeros((N_BANDS, 0)), tob_y=np.zeros((N_BANDS, 0)), seg=np.zeros(0))
    if nf > 0:
        r["norms"] = np.array([np.sqrt(((w * x[j * HOP:j * HOP + N_FRAME]) ** 2).sum()) for j in range(nf)])
        e = r["energies"] = 20.0 * np.log10(r["norms"] + EPS)
        t = e.max() - DYN_RANGE - e
        r["margin"] = float(np.abs(t).min())
        r["keep"] = (t < 0).astype(np.int32)
        src = r["src"] = np.nonzero(r["keep"])[0].astype(np.int32)
        k = r["k"] = len(src)
        r["M"] = k - 1
        if k > 1:
            r["tob_x"] = _tob(_rebuild(x, src, w), w, lo, hi)
            r["tob_y"] = _tob(_rebuild(y, src, w), w, lo, hi)
            assert r["tob_x"].shape[1] == k - 1
    M = r["M"]
    if M >= N_SEG:
        J = r["J"] = M - N_SEG + 1
        r["seg"] = np.array([segment_sum(r["tob_x"][:, m - N_SEG:m], r["tob_y"][:, m - N_SEG:m], extended) for m in range(N_SEG, M + 1)])
        r["d"] = float(r["seg"].sum() / (N_SEG * J if extended else N_BANDS * J))
    r["counts"] = (nf, r["k"], r["J"])
    return r


def to_10k(x, fs):
    """resample_poly with scipy's default filter, rounded to float32 (how the library's resampler is specified)."""
    if fs == FS:
        return np.asarray(x, np.float32)
    from scipy.signal import resample_poly
    fr = Fraction(FS, int(fs))
    return resample_poly(np.asarray(x, np.float32).astype(np.float64), fr.numerator, fr.denominator).astype(np.float32)


def score(x, y, fs, extended=True):
    return core(to_10k(x, fs), to_10k(y, fs), extended)


# ---------------------------------------------------------------------------------------------------------------- cases
def reference_utterances():
    """{'a' | 'b' | 'c': (s, s_est, printed ESTOI)}: the reference's committed 16 kHz pairs as float32 in [-1, 1) and the
    value its figure title prints."""
    za = np.load(GOLDEN + "/metrics_dummy_m2.npz")
    zb = np.load(GOLDEN + "/stoi_dummy_m2.npz")
    f = lambda a: (a.astype(np.float32) / np.float32(32768.0))
    printed = {str(n): float(v) for n, v in zip(zb["names"], zb["printed_estoi"])}
    out = {"a": (f(za["a_s"]), f(za["a_s_est"]), printed["a"])}
    for u in "bc":
        if u + "_s" in zb.files:
            out[u] = (f(zb[u + "_s"]), f(zb[u + "_s_est"]), printed[u])
    return out


def _enveloped_noise(rng, T):
    """Seeded noise with a slow envelope (0.25 .. 1: every frame within 40 dB of the loudest)."""
    t = np.arange(T, dtype=np.float64)
    env = 0.625 + 0.375 * np.sin(2.0 * np.pi * t / 3000.0 + rng.uniform(0, 2 * np.pi))
    return rng.standard_normal(T) * env * 0.1


def _pair(rng, T):
    x = _enveloped_noise(rng, T)
    return x.astype(np.float32), (x + 0.5 * _enveloped_noise(rng, T)).astype(np.float32)


def _gapped(rng, a, b):
    x, y = _pair(rng, 9000)
    x[a:b] *= np.float32(1e-4)
    y[a:b] *= np.float32(1e-4)
    return x, y


def boundary_batch(seed=20241):
    """[(name, x, y)] float32 at 10 kHz: every length at which the framing changes, the first segments, silent stretches
    in the middle, at the head and at the tail, digital silence and y = x."""
    rng = np.random.default_rng(seed)
    cases = [("T%d" % T,) + _pair(rng, T) for T in (0, 255, 256, 257, 384, 385)]
    cases += [("k%d" % (n + 1),) + _pair(rng, 256 + 128 * n + 1) for n in (29, 30, 31, 32)]
    cases.append(("gap_mid",) + _gapped(rng, 2000, 3500))
    cases.append(("gap_head",) + _gapped(rng, 0, 1500))
    cases.append(("gap_tail",) + _gapped(rng, 7500, 9000))
    cases.append(("zeros", np.zeros(5000, np.float32), np.zeros(5000, np.float32)))
    x, _ = _pair(rng, 6000)
    cases.append(("same", x, x.copy()))
    return cases
