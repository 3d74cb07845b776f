"""No GPU: pins on the value cases of tests/value_cases.py, from the float64 / float32 references alone.

What tests/test_gpu_value_range.py relies on is asserted here: that the sharpened decoders are in the saturated, wide-range
regime and the control is not; that the amplitudes put the products the kernels form where amplitude() says; what the
degenerate utterances of the isolation test do in the reference; and how the bounds behave against a known fault.

Two findings about the bounds, both printed by these tests:
  * The worst-case first-order bound of the decoder (gamma (|W| |x| + |b|) per layer, summed in absolute value) is 400 to
    1000 times what a healthy bf16x3 evaluation shows, and a bf16x3 decoder that drops one cross term -- 2^-9 per product
    -- stays INSIDE it at every level (0.39 to 0.99 of the bound at "trained", 0.22 to 0.57 at "xavier").  That bound
    alone would not notice the fault.  The root-sum-square figure of the same model (independent roundings add in
    squares; RSS_FACTOR = 8) is exceeded by the fault 20 to 28 times and holds the healthy evaluation at under 0.1; the
    GPU tests assert both.
  * The rule "compare a frame's later steps only while all its earlier decisions have a margin above the bound" leaves out
    20 to 36 % of the frames of a sharpened bf16x3 case with the root-sum-square bound, and every frame with the worst-case
    bound or in bf16 mode: above the 15 % cap however the data are seeded.  The GPU test therefore evaluates the float64
    chain along the device's own decisions (chain64(decisions=...)): every step of every frame is compared, none is left
    out, and a device decision may differ from the float64 one only where the margin is inside the bound.
"""
import numpy as np

import value_cases as vc
import vaenmf_oracle as orc


def _distinct(fields):
    seen = []
    for case in vc.CASES:
        k = tuple(case[i] for i in fields)
        if k not in seen:
            seen.append(k)
    return seen


def test_sharpened_decoders_are_in_the_trained_regime_and_the_control_is_not():
    """float64: "trained" and "extreme" spread a frame's log-variance over >= 20 nats (median over the frames) with >= 5 %
    of the hidden pre-activations beyond |4|; "xavier" reaches neither (no frame above 5 nats, under 0.1 % of the units beyond |4|)."""
    for shape, level, dy in _distinct((0, 2, 4)):
        c = vc.get_case(shape, level, "one", dy)
        a, _, pre = vc.decoder64(c.params, vc._zin(c, c.Z_true))
        span = a.max(1) - a.min(1)
        p = np.abs(np.concatenate([x.ravel() for x in pre]))
        sat4, sat9 = float(np.mean(p > 4)), float(np.mean(p > 9))
        print("%s %s y_dim %d: log-variance [%.1f, %.1f], span per frame min %.1f median %.1f, |pre-activation| > 4: %.1f %%, > 9: %.1f %%"
              % (shape, level, dy, a.min(), a.max(), span.min(), np.median(span), 100 * sat4, 100 * sat9))
        if level == "xavier":
            assert span.max() < 5 and sat4 < 1e-3
        else:
            assert np.median(span) >= 20 and sat4 >= 0.05
        if level == "extreme":
            assert np.median(span) >= 35 and sat4 >= 0.2 and sat9 >= 0.01


def test_amplitudes_put_the_products_where_they_are_meant_to_be():
    """The products of pair_products() at every amplitude of the cases, from float64 alone: 2^10 inside the normal float32
    range at "small" / "large" (and no power of two of the amplitude further inside than needed), between 2^2 and 2^6 from
    the edge at the edge cases, and the whole of it at amplitude 1."""
    for shape, level, amp, dy in _distinct((0, 2, 3, 4)):
        c = vc.get_case(shape, level, amp, dy)
        lo, hi = np.log2(vc.pair_products(c))
        room_lo, room_hi = lo - vc.FLT_MIN_EXP, vc.FLT_MAX_EXP - hi
        print("%s %s %s y_dim %d: amplitude 2^%d, products 2^%.1f .. 2^%.1f, room 2^%.1f below, 2^%.1f above"
              % (shape, level, amp, dy, np.log2(c.amp), lo, hi, room_lo, room_hi))
        assert np.log2(c.amp) == int(np.log2(c.amp))
        if amp == "one":
            assert level == "extreme" or (room_lo >= vc.MARGIN_EXP and room_hi >= vc.MARGIN_EXP)
            assert room_lo > 0 and room_hi > 0
        elif amp == "small":
            assert vc.MARGIN_EXP <= room_lo < vc.MARGIN_EXP + 4 and c.amp < 2.0 ** -8
        elif amp == "large":
            assert vc.MARGIN_EXP <= room_hi < vc.MARGIN_EXP + 4 and c.amp > 2.0 ** 8
        elif amp == "edge_small":
            assert vc.EDGE_EXP <= room_lo < vc.EDGE_EXP + 4
        else:
            assert vc.EDGE_EXP <= room_hi < vc.EDGE_EXP + 4


def test_audio_scales_lie_inside_the_supported_range():
    """int16-scaled audio at full scale and audio at -80 dBFS with 80 dB of dynamic range inside a frame, at the longest
    window the library takes (F <= 640: n_fft <= 1278; n_fft 4096 gives F = 2049, which vaenmf_plan_create refuses): the
    square of the largest power and the square of the smallest variance stay 2^10 inside the normal float32 range."""
    n_fft, fs = 1024, 16000
    t = np.arange(4 * n_fft)
    loud = 32767.0 * np.sign(np.sin(2 * np.pi * 440.0 * t / fs))                   # full-scale square wave, int16 units
    p_max = float(np.max(np.abs(orc.stft(loud, fs=fs, wlen_sec=n_fft / fs)) ** 2))
    bound = (32768.0 * n_fft / 2) ** 2                                            # |X| <= max|x| sum(w), sum of a Hann window = n_fft / 2
    quiet = 1e-4 * np.random.default_rng(0).standard_normal(4 * n_fft)            # -80 dBFS on a full scale of 1
    p_min = float(np.median(np.abs(orc.stft(quiet, fs=fs, wlen_sec=n_fft / fs)) ** 2)) * 1e-8    # 80 dB under the median bin
    print("full-scale int16, n_fft %d: largest |X|^2 2^%.1f (bound 2^%.1f at n_fft 1278: 2^%.1f); -80 dBFS less 80 dB: 2^%.1f"
          % (n_fft, np.log2(p_max), np.log2(bound), 2 * np.log2(32768.0 * 639), np.log2(p_min)))
    assert p_max <= bound
    assert 4 * np.log2(32768.0 * 639) <= vc.FLT_MAX_EXP - vc.MARGIN_EXP
    assert 2 * np.log2(p_min) >= vc.FLT_MIN_EXP + vc.MARGIN_EXP


def test_a_dropped_cross_term_exceeds_the_root_sum_square_bound():
    """A float64 simulation of the bf16x3 decoder (decoder_split_sim) stays inside both bounds; with one cross term
    dropped it exceeds the root-sum-square bound at every level -- and does NOT exceed the worst-case bound at "trained",
    which is why the GPU tests assert both.  Prints the ratios."""
    gamma = vc.GAMMA["bf16x3"]
    for shape, level, dy in _distinct((0, 2, 4)):
        c = vc.get_case(shape, level, "one", dy)
        zin = vc._zin(c, c.Z0)
        full = vc.decoder64_full(c.params, zin, gamma)
        worst, rss = vc.logvar_bound(full.da), vc.logvar_bound_rss(full.sigma)
        ok = np.abs(vc.decoder_split_sim(c.params, zin) - full.a)
        bad = np.abs(vc.decoder_split_sim(c.params, zin, drop_cross_term=True) - full.a)
        print("%s %s y_dim %d: healthy %.4f of the worst-case bound, %.3f of the rss bound; cross term dropped %.2f / %.1f (largest), "
              "%.2f / %.1f (median)" % (shape, level, dy, np.max(ok / worst), np.max(ok / rss), np.max(bad / worst), np.max(bad / rss),
                                        np.median(bad / worst), np.median(bad / rss)))
        assert np.all(ok <= worst) and np.max(ok / rss) < 0.25
        assert np.max(bad / rss) > 10 and np.median(bad / rss) > 2
        assert np.all(rss < worst)


def test_replayed_chains_accept_and_reject_and_follow_given_decisions():
    """Every case's float64 chain accepts and rejects; chain64 along its own decisions reproduces itself, along inverted
    ones it agrees in step 0 alone.  Prints what the margin rule would leave out under either bound (see the module
    docstring)."""
    for case in vc.CASES:
        shape, prec, level, amp, dy = case
        c = vc.get_case(shape, level, amp, dy)
        ch = vc.chain64(c, vc.GAMMA[prec])
        assert ch.decision.any() and not ch.decision.all(), case
        assert np.all(np.isfinite(ch.acc)) and np.all(ch.bound_rss <= ch.bound)
        print("%s: acceptance %.2f, |acc| up to %.3g, bound median %.2e (rss %.2e); the margin rule would leave out %.0f %% (rss %.0f %%)"
              % (vc.case_id(case), ch.decision.mean(), np.abs(ch.acc).max(), np.median(ch.bound), np.median(ch.bound_rss),
                 100 * vc.left_out_share(ch, ch.bound), 100 * vc.left_out_share(ch, ch.bound_rss)))
        if amp == "one" and dy == 0:
            same = vc.chain64(c, vc.GAMMA[prec], decisions=ch.decision)
            assert np.array_equal(same.acc, ch.acc) and np.array_equal(same.Zs, ch.Zs)
            inv = vc.chain64(c, vc.GAMMA[prec], decisions=~ch.decision)
            assert np.array_equal(inv.acc[0], ch.acc[0]) and not np.array_equal(inv.acc[1], ch.acc[1])


def test_scaling_the_data_leaves_the_float64_chain_alone():
    """The metamorphic property itself, in float64: the log-acceptances at every amplitude equal those at amplitude 1 to
    rounding (1e-9 of the sum of the absolute terms)."""
    for shape, prec, level, amp, dy in vc.CASES:
        if amp == "one":
            continue
        a = vc.chain64(vc.get_case(shape, level, amp, dy), vc.GAMMA[prec])
        b = vc.chain64(vc.get_case(shape, level, "one", dy), vc.GAMMA[prec])
        assert np.array_equal(a.decision, b.decision)
        assert np.all(np.abs(a.acc - b.acc) <= 1e-9 * (a.bound + b.bound) / (vc.ACC_FACTOR * 2.0 ** -24)), (shape, level, amp)


def degenerate_oracle_run(kind, niter=3):
    """The float32 oracle on one 12-frame utterance of the f65 "trained" case whose frame 5 is exactly zero ("frame") or
    which is all zeros ("all").  Returns per iteration (W, H and g all finite, the cost finite, W holds a NaN)."""
    c = vc.get_case("f65", "trained", "one")
    X = c.Xs[0][:12].copy()
    if kind == "frame":
        X[5] = 0
    else:
        X[:] = 0
    o = orc.MCEMOracle("M1", niter, 4, 3, 4, 3, c.var_rw, reference_compat=False)
    o.init_parameters(X, c.params, c.K, 1e-8, orc.NumpyRNG(1), W0=c.W0[0], H0=c.H0[0][:, :12])
    o.Z = c.Z0[:12].T.copy()
    out = []
    with np.errstate(all="ignore"):
        for _ in range(niter):
            o.E_step()
            o.M_step()
            state = bool(np.all(np.isfinite(o.W)) and np.all(np.isfinite(o.H)) and np.all(np.isfinite(o.g)))
            out.append((state, bool(np.isfinite(o.compute_expected_neg_log_like())), bool(np.any(np.isnan(o.W)))))
    return out


def test_the_reference_turns_a_silent_frame_into_nan():
    """mcem.py:107-142 with an exactly silent frame: the first M-step sets the frame's activations and gain to zero, so
    its variance Vx is 0 and the cost -inf while W, H and g are still finite; the second M-step divides 0 by 0
    (mcem.py:107) and W is NaN from there on.  An utterance of zeros is NaN from its first M-step (mcem.py:131)."""
    run = degenerate_oracle_run("frame")
    assert run == [(True, False, False), (False, False, True), (False, False, True)], run
    run = degenerate_oracle_run("all")           # W = W sqrt(0 / den) = 0, then normalised by its column sums: 0 / 0 at once
    assert run == [(False, False, True)] * 3, run
