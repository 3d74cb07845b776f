"""The host side of the data-set path (vaenmf/dataset.py, csrc/dataset.hip) without a GPU: the random draws, what the
reference's own processed utterances say about the two mixing recipes, the mean / std formula, and the refusals and work
sizes of the C entry points."""
import ctypes as C
import os

import numpy as np
import pytest

import dataset_cases as dc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_plan_mixes_draw_order():
    """plan_mixes equals the literal call sequence of the sequential script: np.random.seed, the two size-n draws
    (create_noisy_train_set.py:167-170), then one start per file in list order (demand_database.py:125)."""
    from vaenmf.dataset import plan_mixes
    speech = [40000, 51234, 16001, 70000, 33333, 64000, 20480]
    noise_types = ["domestic", "nature", "office", "transportation"]
    noise = {"domestic": 300000, "nature": 90001, "office": 123457, "transportation": 70001}
    for snrs, seed in (([-5, -2.5, 0, 2.5, 5.0], 0), ([-5.0, 0.0, 5.0], 3)):
        state = np.random.get_state()
        np.random.seed(seed)
        noise_index = np.random.randint(len(noise_types), size=len(speech))
        snrs_index = np.random.randint(len(snrs), size=len(speech))
        start = [np.random.randint(noise[noise_types[noise_index[i]]] - speech[i]) for i in range(len(speech))]
        np.random.set_state(state)
        ni, snr_db, st = plan_mixes(speech, noise, noise_types, snrs, seed)
        assert list(ni) == list(noise_index) and list(st) == start
        assert snr_db == [float(snrs[j]) for j in snrs_index] and all(type(v) is float for v in snr_db)
        ni2, _, st2 = plan_mixes(speech, [noise[t] for t in noise_types], noise_types, snrs, seed)     # lengths as a list
        assert list(ni2) == list(ni) and list(st2) == list(st)
    assert len(set(ni)) > 1 and len(set(snr_db)) > 1


def test_plan_mixes_refuses_short_noise():
    from vaenmf.dataset import plan_mixes
    with pytest.raises(ValueError, match="longer"):
        plan_mixes([1000, 1000], [1000, 1000], ["a", "b"], [0.0])            # equal length: randint(0) in the reference
    with pytest.raises(ValueError, match="longer"):
        plan_mixes([1000], {"a": 999}, ["a"], [0.0])
    assert plan_mixes([1000], {"a": 1001}, ["a"], [0.0])[2][0] == 0


def test_reference_files_pin_the_recipes():
    """The nine processed utterances of the reference (numbers in tests/golden/mix_recipe_ref.npz).  Test set
    (create_test_set.py:92-103): the energy ratio of the written _s and _n is the recorded SNR within four standard
    deviations of the int16 rounding, the joint peak is full scale and x = s + n within 1 LSB everywhere.  Train and validation
    (create_noisy_train_set.py:222, 237-250): the speech peak is full scale in every file, and the joint-peak rule does not
    hold -- in both sets a mixture exceeded full scale and was clipped on write, which that rule makes impossible."""
    z = np.load(os.path.join(GOLDEN, "mix_recipe_ref.npz"))
    subset = [str(s) for s in z["subset"]]
    test = [i for i, s in enumerate(subset) if s == "test"]
    assert len(test) == 3 and len(z["snr_db_test"]) == 3
    for i, want in zip(test, z["snr_db_test"]):
        got = 10.0 * np.log10(float(z["sum_s2"][i]) / float(z["sum_n2"][i]))
        print("%s: %.7f dB, recorded %g, off by %.2e dB, bound %.2e dB" % (z["rel"][i], got, want, abs(got - want), 4 * z["snr_bound_db"][i]))
        assert abs(got - want) <= 4.0 * z["snr_bound_db"][i]
        assert max(z["peak_s"][i], z["peak_n"][i], z["peak_x"][i]) >= 32767
        assert z["x_off"][i] == 0
    for name in ("train", "validation"):
        idx = [i for i, s in enumerate(subset) if s == name]
        assert len(idx) == 3
        assert all(z["peak_s"][i] >= 32767 for i in idx)
        assert any(z["x_off"][i] > 0 for i in idx)
    assert not all(z["peak_s"][i] >= 32767 for i in test)                      # ... where the test set's speech is scaled down


def test_mean_std_formula():
    """moments_mean_std from float64 sums against np.mean / np.std(ddof=1): log-normal powers from 1e-12 to 1e4; relative
    tolerance of the variance the cancellation bound (1 + mean^2 / var) n 2^-52 (S2 and n mean^2 each carry n 2^-53 relative, their
    difference is var (n - 1)), half of it for the std, plus the float32 rounding of the result."""
    from vaenmf.dataset import FeatureMoments, moments_mean_std
    n, F = 1000, 513
    X = np.ascontiguousarray(dc.moments_input(n, F, 528)[:, :F].T)
    S1, S2 = dc.moments_ref(X.T, F)
    mean, std = moments_mean_std(S1, S2, n)
    assert mean.shape == std.shape == (F, 1) and mean.dtype == std.dtype == np.float32
    m_ref, s_ref = dc.mean_std_ref(X)
    u32 = 2.0 ** -24
    assert np.all(np.abs(mean[:, 0] - m_ref) <= (n * 2.0 ** -52 + u32) * np.abs(m_ref))
    rel = (1.0 + m_ref ** 2 / s_ref ** 2) * n * 2.0 ** -52
    assert float(rel.max()) < 1e-6
    assert np.all(np.abs(std[:, 0] - s_ref) <= (0.5 * rel + u32) * s_ref)
    with pytest.raises(ValueError, match="2 frames"):
        moments_mean_std(S1, S2, 1)
    with pytest.raises(ValueError, match="2 frames"):
        FeatureMoments(F).mean_std()


def test_constant_bin_has_zero_std():
    """A bin that holds the same value in every frame: S2 - n mean^2 rounds to a few ulps of either sign; the clamp makes
    the std 0 or tiny, never NaN."""
    from vaenmf.dataset import moments_mean_std
    n = 777
    vals = np.array([0.1, 3.0, 1e-12, 1e4, 0.7], np.float32).astype(np.float64)
    mean, std = moments_mean_std(vals * n, vals * vals * n, n)
    assert not np.any(np.isnan(std)) and np.all(std >= 0)
    assert np.all(std[:, 0] <= 1e-6 * vals)
    assert moments_mean_std(np.array([3.0 * n]), np.array([9.0 * n]), n)[1][0, 0] == 0.0


def test_work_bytes():
    from vaenmf._lib import lib
    l = lib()
    assert l.vaenmf_mix_work_bytes(0) == 0 and l.vaenmf_mix_work_bytes(1) == 552 and l.vaenmf_mix_work_bytes(64) == 64 * 552
    assert l.vaenmf_mix_work_bytes(-1) == -1 and b"n_utt" in l.vaenmf_last_error()
    # 2 sums x F doubles per frame span; min(256, ceil(n_frames / 64)) spans
    for n, spans in ((0, 0), (1, 1), (64, 1), (65, 2), (4099, 65), (64 * 256, 256), (32064, 256), (10 ** 9, 256)):
        assert l.vaenmf_moments_work_bytes(n, 257) == 16 * 257 * spans, n
    assert l.vaenmf_moments_work_bytes(-1, 257) == -1 and l.vaenmf_moments_work_bytes(10, 0) == -1


def test_host_refusals():
    """Everything vaenmf_mix_batch and vaenmf_feature_moments refuse is refused before a launch: with a stand-in for every
    device pointer (never dereferenced by the host) the calls return -1 and name the utterance."""
    from vaenmf._lib import lib
    l = lib()
    fake = 0x1000                                                             # aligned, non-null; no launch ever sees it

    def mix(counts, cuts, starts, L, out_counts=None, factors=None):
        U = len(counts)
        ioff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        oc = [t - c for t, c in zip(counts, cuts)] if out_counts is None else out_counts
        ooff = np.concatenate([[0], np.cumsum(oc)]).astype(np.int64)
        cu, st = np.array(cuts, np.int64), np.array(starts, np.int64)
        f = np.array([1.0] * U if factors is None else factors, np.float64)
        rc = l.vaenmf_mix_batch(fake, U, ioff.ctypes.data, cu.ctypes.data, fake, L, st.ctypes.data, f.ctypes.data, 1, ooff.ctypes.data,
                                fake, fake, fake, fake, fake, l.vaenmf_mix_work_bytes(U), None)
        return rc, l.vaenmf_last_error()

    for args, word in ((([10, 5], [0, 5], [0, 0], 100), b"utterance 1"),                   # T' = 0
                       (([10, 5], [11, 0], [0, 0], 100), b"utterance 0"),                  # T' < 0
                       (([10, 5], [0, -1], [0, 0], 100), b"negative"),
                       (([10, 5], [0, 0], [-1, 0], 100), b"utterance 0"),                  # b < 0
                       (([10, 5], [0, 0], [0, 96], 100), b"utterance 1"),                  # b + T' > L
                       (([10, 5], [0, 0], [0, 0], 9), b"utterance 0"),                     # L < T'
                       (([10, 5], [0, 0], [0, 0], 100, [10, 6]), b"out_offsets"),
                       (([10, 5], [0, 0], [0, 0], 100, None, [1.0, 0.0]), b"factor"),
                       (([10, 5], [0, 0], [0, 0], 100, None, [float("nan"), 1.0]), b"factor")):
        rc, msg = mix(*args)
        assert rc == -1 and word in msg, (args, msg)
    assert l.vaenmf_mix_batch(None, 0, None, None, None, 0, None, None, 1, None, None, None, None, None, None, 0, None) == 0
    ioff = np.array([0, 10], np.int64)
    z, one = np.zeros(1, np.int64), np.ones(1, np.float64)
    rc = l.vaenmf_mix_batch(fake, 1, ioff.ctypes.data, z.ctypes.data, fake, 100, z.ctypes.data, one.ctypes.data, 1, ioff.ctypes.data,
                            fake, fake, fake, fake, fake, 551, None)
    assert rc == -1 and b"work_bytes" in l.vaenmf_last_error()
    rc = l.vaenmf_mix_batch(fake, 1, ioff.ctypes.data, z.ctypes.data, fake, 100, z.ctypes.data, one.ctypes.data, 1, ioff.ctypes.data,
                            fake, fake, fake, fake, fake + 4, 552, None)
    assert rc == -1 and b"aligned" in l.vaenmf_last_error()
    for n, F, ld, wb, word in ((-1, 4, 4, 1 << 20, b"n_frames"), (10, 0, 4, 1 << 20, b"F=0"), (10, 8, 7, 1 << 20, b"ld=7"),
                               (10, 8, 8, 16 * 8 - 1, b"work_bytes")):
        assert l.vaenmf_feature_moments(fake, n, F, ld, 0, fake, fake, fake, wb, None) == -1 and word in l.vaenmf_last_error()
    assert l.vaenmf_feature_moments(fake, 10, 8, 8, 0, fake + 4, fake, fake, 1 << 20, None) == -1
