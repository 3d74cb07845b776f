"""Cases and float64 numpy restatements for the data-set kernels (csrc/dataset.hip, vaenmf/dataset.py).  The restatements
follow the reference's scripts line by line; nothing here imports the package under test."""
import functools

import numpy as np

# ---- mixing ----------------------------------------------------------------------------------------------------------
LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 40000]     # samples kept after the cut
CUTS = [0, 7, 1600]
SNRS = [-5.0, 0.0, 2.5, 5.0]
SCALES = [2.0 ** -10, 1.0, 30.0]
NOISE_LEN = 50000
STAT_NAMES = ("p", "Es", "En", "k", "m")


def batch_params():
    """(cuts, starts, snr_db) of the ragged batch: cuts and SNRs cycle through their sets; the first utterance starts at 0,
    the second and the last at the last valid start L - T', the others at seeded random starts."""
    g = np.random.default_rng(7)
    U = len(LENGTHS)
    cuts = [CUTS[u % len(CUTS)] for u in range(U)]
    snr = [SNRS[u % len(SNRS)] for u in range(U)]
    starts = [int(g.integers(0, NOISE_LEN - T + 1)) for T in LENGTHS]
    starts[0] = 0
    starts[1] = NOISE_LEN - LENGTHS[1]
    starts[-1] = NOISE_LEN - LENGTHS[-1]
    return cuts, starts, snr


@functools.lru_cache(maxsize=None)
def batch_inputs(scale, seed=0):
    """(speech rows incl. their cut region, noise buffer): float32, read-only."""
    g = np.random.default_rng(100 + seed)
    cuts, _, _ = batch_params()
    rows = []
    for T, c in zip(LENGTHS, cuts):
        a = (g.standard_normal(T + c) * np.exp(g.standard_normal(T + c)) * 0.1 * scale).astype(np.float32)
        a.setflags(write=False)
        rows.append(a)
    noise = (g.standard_normal(NOISE_LEN) * 0.3).astype(np.float32)
    noise.setflags(write=False)
    return tuple(rows), noise


def mix_ref(a, cut, noise, start, snr_db, joint_norm):
    """One utterance in float64, scripts/create_test_set.py:80-103 (joint_norm) / scripts/create_noisy_train_set.py:219-244.
    -> (s, n, x float64, stats dict)."""
    speech = np.asarray(a, np.float64)[cut:]                                   # :81  speech = speech[int(0.1*fs):]
    p = np.max(np.abs(speech))
    speech = speech / p                                                        # :84
    noise_seg = np.asarray(noise, np.float64)[start:start + len(speech)]       # qut_database / demand_database.py:125-126
    speech_power = np.sum(np.power(speech, 2))                                 # :93
    noise_power = np.sum(np.power(noise_seg, 2))                               # :94
    noise_power_target = speech_power * np.power(10, -snr_db / 10)             # :95
    k = noise_power_target / noise_power                                       # :96
    noise_seg = noise_seg * np.sqrt(k)                                         # :97
    norm = 1.0
    if joint_norm:
        norm = np.max(abs(np.concatenate([speech, noise_seg, speech + noise_seg])))   # :100
    mixture = (speech + noise_seg) / norm                                      # :101
    return speech / norm, noise_seg / norm, mixture, dict(p=p, Es=speech_power, En=noise_power, k=k, m=norm)


@functools.lru_cache(maxsize=None)
def batch_ref(scale, joint_norm):
    rows, noise = batch_inputs(scale)
    cuts, starts, snr = batch_params()
    return tuple(mix_ref(a, c, noise, b, d, joint_norm) for a, c, b, d in zip(rows, cuts, starts, snr))


def dominance_cases():
    """Three utterances at 0 dB (f = 1) whose every intermediate is a dyadic number, so that any summation order gives the
    same bits: Es = 2.25, En = 0.5625, k = 4, sqrt(k) = 2.  The joint peak comes from |s| (m = 1: the noise cancels half of the
    speech peak), from |n| (m = 1.5) and from |s + n| (m = 2).  -> list of (speech row, noise row, expected m)."""
    s = np.array([1, .5, .5, .5, .5, .5, 0, 0, 0], np.float32) * np.float32(0.5)          # p = 0.5
    from_s = np.array([-.25] * 6 + [.25] * 3, np.float32)
    from_n = np.array([0, -.75, 0, 0, 0, 0, 0, 0, 0], np.float32)
    from_x = np.array([0, .75, 0, 0, 0, 0, 0, 0, 0], np.float32)
    return [(s, from_s, 1.0), (s, from_n, 1.5), (s, from_x, 2.0)]


# ---- moments ---------------------------------------------------------------------------------------------------------
MOMENT_SHAPES = [(1, 1, 16), (2, 65, 80), (63, 65, 80), (64, 257, 272), (65, 257, 272), (1000, 513, 528), (4099, 257, 272)]


@functools.lru_cache(maxsize=None)
def moments_input(n_frames, F, ld):
    """Log-normal powers between about 1e-12 and 1e4 in the bins < F; zeros in the padding (the tests poison it)."""
    g = np.random.default_rng(n_frames * 1000 + F)
    P = np.zeros((n_frames, ld), np.float32)
    P[:, :F] = np.clip(np.exp(g.standard_normal((n_frames, F)) * 6.0 - 9.0), 1e-12, 1e4).astype(np.float32)
    P.setflags(write=False)
    return P


def moments_ref(P, F):
    """channels_sum, channels_squared_sum of scripts/create_noisy_train_set.py:302-303 in float64.  All terms are positive,
    so each sum is also the sum of its terms' magnitudes, which scales the error bound."""
    v = np.asarray(P, np.float64)[:, :F]
    return v.sum(0), (v * v).sum(0)


def mean_std_ref(X):
    """np.mean / np.std(ddof=1) over the frames of X (F, N) in float64: what :313-319 computes from the running sums."""
    X = np.asarray(X, np.float64)
    return X.mean(1), X.std(1, ddof=1)
