"""The data-set kernels (csrc/dataset.hip) and builders (vaenmf/dataset.py) on the GPU: vaenmf_mix_batch against the float64
restatement of the reference's recipe (tests/dataset_cases.py), what decides its peak and norm, its exact invariances, its
independence of the batch, its degenerate and refused inputs; vaenmf_feature_moments against float64 numpy; make_train_set
and make_test_set end to end.  Every buffer of the kernel tests is carved from a poisoned arena (tests/guarded.py): exact
sizes, 16 (mod 256) addresses, guards checked after every call, inputs checked unchanged."""
import functools
import os
import pickle

import numpy as np
import pytest
import torch

import dataset_cases as dc
from guarded import Arena, POISON
from helpers import load_case, need_gpu

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -23
U64 = 2.0 ** -52


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _mix_raw(rows, cuts, noise, starts, snr_db, joint_norm, poison="1e30", expect=0):
    """vaenmf_mix_batch on arena buffers: speech rows concatenated (odd lengths: rows at 4-byte aligned addresses and no
    better), every output poisoned before the call.  -> (s, n, x per utterance, stats [U][5]) on the host, or the return
    code when it is not `expect` = 0."""
    from vaenmf._lib import lib
    from vaenmf.dataset import snr_factor
    U = len(rows)
    counts = [len(r) for r in rows]
    kept = [t - c for t, c in zip(counts, cuts)]
    total_in, total_out = sum(counts), max(sum(max(k, 0) for k in kept), 1)
    nbytes = lib().vaenmf_mix_work_bytes(U)
    arena = Arena(4 * (total_in + len(noise) + 3 * total_out) + 40 * U + nbytes + 12 * (160 << 10), poison, device="cuda")
    speech = arena.carve("speech", (total_in,), torch.float32)
    speech.copy_(torch.from_numpy(np.concatenate(rows)))
    nz = arena.carve("noise", (len(noise),), torch.float32)
    nz.copy_(torch.from_numpy(np.array(noise)))
    s, n, x = (arena.carve(k, (total_out,), torch.float32) for k in "snx")
    stats = arena.carve("stats", (U, 5), torch.float64)
    work = arena.carve("work", (nbytes,), torch.uint8)
    arena.snapshot(["speech", "noise"])
    ioff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ooff = np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)
    cu, st = np.array(cuts, np.int64), np.array(starts, np.int64)
    f = np.array([snr_factor(v) for v in snr_db], np.float64)
    rc = lib().vaenmf_mix_batch(speech.data_ptr(), U, ioff.ctypes.data, cu.ctypes.data, nz.data_ptr(), len(noise), st.ctypes.data,
                                f.ctypes.data, int(joint_norm), ooff.ctypes.data, s.data_ptr(), n.data_ptr(), x.data_ptr(),
                                stats.data_ptr(), work.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    arena.check("mix_batch")
    arena.unchanged(what="mix_batch")
    if rc != 0 or expect != 0:
        assert rc == expect, (rc, lib().vaenmf_last_error())
        assert all(arena.is_poison(t) for t in (s, n, x)) and arena.is_poison(stats.view(torch.float32))      # nothing written
        return rc
    split = lambda t: [p.cpu().numpy() for p in torch.split(t, kept)]
    return split(s), split(n), split(x), stats.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _batch_result(scale, joint_norm):
    rows, noise = dc.batch_inputs(scale)
    cuts, starts, snr = dc.batch_params()
    return _mix_raw(rows, cuts, noise, starts, snr, joint_norm)


@pytest.mark.parametrize("scale", dc.SCALES)
@pytest.mark.parametrize("joint_norm", [True, False])
def test_mix_against_oracle(joint_norm, scale):
    """Every output sample: |y - float32(y_ref)| <= 2^-23 |y_ref| (one float32 rounding plus one flipped rounding; the
    float64 sum-order differences are at most n 2^-52 relative).  Stats: p exact; Es, En, k, m within (n + 8) 2^-52."""
    need_gpu()
    s, n, x, stats = _batch_result(scale, joint_norm)
    refs = dc.batch_ref(scale, joint_norm)
    worst, worst_st = 0.0, 0.0
    for u, (T, ref) in enumerate(zip(dc.LENGTHS, refs)):
        for got, want in zip((s[u], n[u], x[u]), ref[:3]):
            assert got.shape == (T,) and got.dtype == np.float32
            err = np.abs(got.astype(np.float64) - want.astype(np.float32).astype(np.float64))
            bound = U32 * np.abs(want)
            ratio = float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)))
            worst = max(worst, ratio)
            assert np.all(err <= bound), (u, T, ratio)
        assert stats[u, 0] == ref[3]["p"], u
        for j, name in enumerate(dc.STAT_NAMES[1:], 1):
            rel = abs(stats[u, j] - ref[3][name]) / abs(ref[3][name])
            worst_st = max(worst_st, rel / ((T + 8) * U64))
            assert rel <= (T + 8) * U64, (u, T, name, rel)
        if not joint_norm:
            assert stats[u, 4] == 1.0
    print("mix joint_norm=%d scale %g: worst sample error %.3f of its bound, worst stat %.3f of its bound" % (joint_norm, scale, worst, worst_st))


def test_what_decides_peak_and_norm():
    """The joint maximum from |s|, |n| and |s + n| (dyadic cases: m is exact and the largest output is 1.0f); a sample ten
    times larger than the rest inside the cut region does not become p; a peak on the first and on the last kept sample
    of an utterance that spans three workgroups."""
    need_gpu()
    cases = dc.dominance_cases()
    g = np.random.default_rng(5)
    burst = (g.uniform(-0.4, 0.4, 300 + 40)).astype(np.float32)
    burst[17] = 5.0                                                  # inside the cut of 40
    burst[40 + 123] = -0.5
    ends = g.uniform(-0.7, 0.7, 9000 + 7).astype(np.float32)
    ends[7], ends[-1] = 0.75, -0.75
    rows = [c[0] for c in cases] + [burst, ends]
    cuts = [0, 0, 0, 40, 7]
    tail = (g.standard_normal(9000) * 0.2).astype(np.float32)
    noise = np.concatenate([c[1] for c in cases] + [tail])
    starts = [0, 9, 18, 27, 27]
    for joint_norm in (True, False):
        s, n, x, stats = _mix_raw(rows, cuts, noise, starts, [0.0] * 5, joint_norm)
        for u, (_, _, m) in enumerate(cases):
            assert list(stats[u]) == [0.5, 2.25, 0.5625, 4.0, m if joint_norm else 1.0], (u, stats[u])
            top = max(np.abs(s[u]).max(), np.abs(n[u]).max(), np.abs(x[u]).max())
            assert top == np.float32(1.0 if joint_norm else m), (u, top)
            if not joint_norm:                                       # dyadic values: nothing is rounded
                assert np.array_equal(x[u], s[u] + n[u])
        assert stats[3, 0] == 0.5 and stats[4, 0] == 0.75
        if not joint_norm:
            assert s[3][123] == -1.0 and np.abs(s[3]).max() == 1.0
            assert s[4][0] == 1.0 and s[4][-1] == -1.0 and np.abs(s[4]).max() == 1.0
        else:
            for u in (3, 4):
                assert max(np.abs(s[u]).max(), np.abs(n[u]).max(), np.abs(x[u]).max()) == np.float32(1.0)


def test_exact_invariances():
    """Speech times 2^j, noise times 2^j (j = -9, 5): the same bits in s, n, x.  The realised SNR, from the float32 outputs
    in float64, is the target within 1e-5 dB (two float32 roundings per energy ratio are about 1e-6 dB)."""
    need_gpu()
    rows, noise = dc.batch_inputs(1.0)
    cuts, starts, snr = dc.batch_params()
    for joint_norm in (True, False):
        base = _batch_result(1.0, joint_norm)
        for j in (-9, 5):
            c = np.float32(2.0 ** j)
            for what, got in (("speech", _mix_raw([r * c for r in rows], cuts, noise, starts, snr, joint_norm)),
                              ("noise", _mix_raw(rows, cuts, noise * c, starts, snr, joint_norm))):
                for k in range(3):
                    for u in range(len(rows)):
                        assert np.array_equal(_bits(got[k][u]), _bits(base[k][u])), (what, j, "snx"[k], u)
        worst = 0.0
        for u, T in enumerate(dc.LENGTHS):
            es, en = np.sum(base[0][u].astype(np.float64) ** 2), np.sum(base[1][u].astype(np.float64) ** 2)
            off = abs(10.0 * np.log10(es / en) - snr[u])
            worst = max(worst, off)
            assert off <= 1e-5, (u, T, off)
        print("realised SNR, joint_norm=%d: worst deviation %.2e dB" % (joint_norm, worst))


def test_batch_independence_and_repeatability():
    """Every utterance alone (a batch of 1, through mix_batch) has the bits of its rows in the batch of 13, outputs and
    stats; the batch run again has them; so has every utterance of a batch of 17, more utterances than any utterance has
    workgroups, in another order."""
    need_gpu()
    from vaenmf.dataset import mix_batch
    rows, noise = dc.batch_inputs(1.0)
    cuts, starts, snr = dc.batch_params()
    nz = torch.from_numpy(np.array(noise)).cuda()
    for joint_norm in (True, False):
        base = _batch_result(1.0, joint_norm)
        again = _mix_raw(rows, cuts, noise, starts, snr, joint_norm, poison="nan")
        order = list(range(13))[::-1] + [12, 0, 5, 12]
        big = _mix_raw([rows[u] for u in order], [cuts[u] for u in order], noise, [starts[u] for u in order], [snr[u] for u in order], joint_norm)
        for u in range(13):
            s, n, x, counts, st = mix_batch(torch.from_numpy(np.array(rows[u])).cuda(), [len(rows[u])], nz, [starts[u]], snr[u], cuts[u], joint_norm)
            assert counts == [dc.LENGTHS[u]]
            alone = (s.cpu().numpy(), n.cpu().numpy(), x.cpu().numpy())
            for k in range(3):
                assert np.array_equal(_bits(alone[k]), _bits(base[k][u])), (u, "snx"[k])
                assert np.array_equal(_bits(again[k][u]), _bits(base[k][u])), (u, "snx"[k])
            assert np.array_equal(_bits(st[0]), _bits(base[3][u])) and np.array_equal(_bits(again[3][u]), _bits(base[3][u]))
        for i, u in enumerate(order):
            for k in range(3):
                assert np.array_equal(_bits(big[k][i]), _bits(base[k][u])), (i, u, "snx"[k])
            assert np.array_equal(_bits(big[3][i]), _bits(base[3][u]))


def test_degenerate_and_refused():
    """Silent speech (after the cut) and a silent noise segment: zeros in that utterance's outputs, k == 0, nothing that is
    not finite, the neighbours untouched; mix_batch raises ValueError naming the utterance.  T' < 1 and a start past
    L - T' are refused with nothing written."""
    need_gpu()
    from vaenmf.dataset import mix_batch
    g = np.random.default_rng(9)
    ok = (g.standard_normal(5000) * 0.1).astype(np.float32)
    silent = np.zeros(777, np.float32)
    silent[:5] = 0.3                                                 # the cut removes all that sounds
    noise = (g.standard_normal(20000) * 0.2).astype(np.float32)
    noise[10000:12000] = 0.0
    rows, cuts, starts = [ok, silent, ok[:1500], ok], [0, 5, 0, 100], [0, 100, 10100, 15100]
    for joint_norm in (True, False):
        s, n, x, stats = _mix_raw(rows, cuts, noise, starts, [0.0, 5.0, -5.0, 2.5], joint_norm, poison="nan")
        assert np.all(np.isfinite(stats))
        for u in (1, 2):
            assert not s[u].any() and not n[u].any() and not x[u].any()
            assert stats[u, 3] == 0.0 and stats[u, 4] == 0.0
        assert stats[1, 0] == 0.0 and stats[2, 0] > 0 and stats[2, 2] == 0.0
        for u in (0, 3):
            assert stats[u, 3] > 0 and np.all(np.isfinite(x[u])) and np.abs(s[u]).max() > 0 and np.abs(n[u]).max() > 0
    speech, nz = torch.from_numpy(np.concatenate(rows)).cuda(), torch.from_numpy(noise).cuda()
    with pytest.raises(ValueError, match="utterance 1 .*speech is silent"):
        mix_batch(speech, [len(r) for r in rows], nz, starts, 0.0, cuts)
    with pytest.raises(ValueError, match="utterance 2 .*noise segment .*silent"):
        mix_batch(speech, [len(r) for r in rows], nz, starts, 0.0, [0, 0, 0, 100])
    with pytest.raises(ValueError, match="utterance 2"):
        mix_batch(speech, [len(r) for r in rows], nz, starts, 0.0, [0, 0, 1500, 0])
    with pytest.raises(ValueError, match="utterance 3"):
        mix_batch(speech, [len(r) for r in rows], nz, [0, 0, 0, 15101], 0.0, [0, 0, 0, 100])
    assert _mix_raw(rows, [0, 0, 1500, 0], noise, starts, [0.0] * 4, True, expect=-1) == -1
    assert _mix_raw(rows, cuts, noise, [0, 0, 0, 15101], [0.0] * 4, True, expect=-1) == -1
    s, n, x, stats = _mix_raw(rows, [0, 0, 0, 100], noise, [0, 0, 0, 15100], [0.0] * 4, True)      # the last valid start is taken
    assert stats[3, 3] > 0


# ---------------------------------------------------------------------------------------------------------------------
# moments
# ---------------------------------------------------------------------------------------------------------------------
def _moments_raw(arena, P, F, accumulate, S1, S2, tag):
    from vaenmf._lib import lib
    n, ld = P.shape
    nbytes = lib().vaenmf_moments_work_bytes(n, F)
    assert nbytes == 16 * F * min(256, (n + 63) // 64)
    work = arena.carve("work" + tag, (nbytes,), torch.uint8)
    rc = lib().vaenmf_feature_moments(P.data_ptr(), n, F, ld, accumulate, S1.data_ptr(), S2.data_ptr(), work.data_ptr(), nbytes,
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib().vaenmf_last_error()
    torch.cuda.synchronize()
    arena.check("feature_moments" + tag)
    arena.unchanged(what="feature_moments" + tag)


@pytest.mark.parametrize("poison", sorted(POISON))
@pytest.mark.parametrize("n_frames,F,ld", dc.MOMENT_SHAPES)
def test_moments(n_frames, F, ld, poison):
    """|S - S_ref| <= n 2^-52 sum|terms| per bin against float64 numpy, padding columns poisoned; accumulate = 0 overwrites
    poison in S1 / S2; three ragged batches accumulated stay within the bound of the one-shot sum and give the same bits in
    two runs."""
    need_gpu()
    host = dc.moments_input(n_frames, F, ld)
    r1, r2 = dc.moments_ref(host, F)
    cuts = sorted({0, n_frames // 3, n_frames - n_frames // 5, n_frames})             # ragged: e.g. 4099 -> 1366, 1914, 819
    arena = Arena(4 * host.size * 2 + 6 * 16 * F * 260 + 40 * (160 << 10), poison, device="cuda")
    P = arena.carve("P", (n_frames, ld), torch.float32)
    P.copy_(torch.from_numpy(np.array(host)))
    if ld > F:
        arena.poison(P[:, F:])
    parts = []
    for i in range(len(cuts) - 1):                                                     # the batches as buffers of their own
        t = arena.carve("P%d" % i, (cuts[i + 1] - cuts[i], ld), torch.float32)
        t.copy_(P[cuts[i]:cuts[i + 1]])
        parts.append(t)
    S = [arena.carve("S%d" % i, (F,), torch.float64) for i in range(6)]                # poison: accumulate = 0 must overwrite it
    arena.snapshot(["P"] + ["P%d" % i for i in range(len(parts))])
    _moments_raw(arena, P, F, 0, S[0], S[1], "/one")
    worst = 0.0
    for run, (A, B) in enumerate(((S[2], S[3]), (S[4], S[5]))):
        for i, t in enumerate(parts):
            _moments_raw(arena, t, F, int(i > 0), A, B, "/run%d.%d" % (run, i))
    got = [t.cpu().numpy() for t in S]
    for a, b in ((got[0], got[1]), (got[2], got[3])):
        for g_, r in ((a, r1), (b, r2)):
            assert np.all(np.isfinite(g_))
            err, bound = np.abs(g_ - r), n_frames * U64 * r                            # the terms are positive: sum|terms| = r
            worst = max(worst, float(np.max(err / bound)))
            assert np.all(err <= bound), float(np.max(err / bound))
    assert np.array_equal(_bits(got[2]), _bits(got[4])) and np.array_equal(_bits(got[3]), _bits(got[5]))
    print("moments (%d, %d, %d) %s: worst error %.4f of the bound" % (n_frames, F, ld, poison, worst))


def test_feature_moments_class_streams_batches():
    """FeatureMoments.add over three batches and mean_std against float64 numpy over all frames, to one float32 rounding."""
    need_gpu()
    from vaenmf.dataset import FeatureMoments
    host = dc.moments_input(1000, 513, 528)
    mom = FeatureMoments(513)
    for a, b in ((0, 100), (100, 101), (101, 1000)):
        mom.add(torch.from_numpy(host[a:b].copy()).cuda())
    mom.add(torch.from_numpy(host[:7].copy()).cuda(), 0)                               # no frames: nothing changes
    S1, S2, n = mom.sums()
    assert n == 1000
    mean, std = mom.mean_std()
    m_ref, s_ref = dc.mean_std_ref(host[:, :513].T)
    assert mean.shape == std.shape == (513, 1)
    assert np.all(np.abs(mean[:, 0] - m_ref) <= (2.0 ** -24 + 1e-12) * m_ref)
    assert np.all(np.abs(std[:, 0] - s_ref) <= (2.0 ** -24 + 1e-9) * s_ref)


# ---------------------------------------------------------------------------------------------------------------------
# the two builders end to end: 5 synthetic utterances of 0.4 - 0.9 s, 3 s of coloured noise per type, an 8 ms window (F = 65)
# ---------------------------------------------------------------------------------------------------------------------
FS, WLEN, HOP, F = 16000, 8e-3, 0.25, 65
SECONDS = [0.4, 0.9, 0.55, 0.7, 0.63]
TYPES = ["domestic", "nature", "office", "transportation"]


def _tree(tmp_path):
    """raw/<rel>.wav for five utterances (with the 0.1 s the recipe cuts) and the noise recordings: three arrays at 16 kHz, one
    (array, 48000) that the builders resample."""
    from vaenmf import wavio
    from vaenmf.synth import synth_utterance
    raw = str(tmp_path) + "/raw/"
    files = []
    for i, sec in enumerate(SECONDS):
        rel = "CSR-1-WSJ-0/WAV/wsj0/si_tr_s/01%d/01%da010a.wav" % (i, i)
        os.makedirs(os.path.dirname(raw + rel), exist_ok=True)
        s = synth_utterance(i, int(sec * FS) + int(0.1 * FS) + i, FS)[0]              # + i: odd lengths
        wavio.write(raw + rel, 0.6 * s, FS)
        files.append(rel)
    g = np.random.default_rng(33)
    noise = {}
    for j, t in enumerate(TYPES):
        rate = 48000 if t == "office" else FS
        w = np.convolve(g.standard_normal(3 * rate), [1.0, 0.6, 0.3][:1 + j % 3], mode="same") * 0.1
        noise[t] = (w.astype(np.float32), rate) if rate != FS else w.astype(np.float32)
    return raw, files, noise


def _mixed(raw, files, noise, snrs, types, seed, joint_norm):
    """The builders' mixing, restated from the public pieces: lengths, plan_mixes, one noise buffer, mix_batch."""
    from vaenmf import wavio
    from vaenmf.dataset import mix_batch, plan_mixes
    from vaenmf.resample import resample_batch
    wavs = [wavio.read(raw + f)[0].astype(np.float32) for f in files]
    cut = int(0.1 * FS)
    bank = []
    for t in types:
        a = noise[t]
        if isinstance(a, tuple):
            a = resample_batch(torch.from_numpy(a[0]).cuda(), [len(a[0])], a[1], FS)[0]
        else:
            a = torch.from_numpy(a).cuda()
        bank.append(a)
    lengths = [int(b.shape[0]) for b in bank]
    base = np.concatenate([[0], np.cumsum(lengths)])
    idx, snr_db, start = plan_mixes([len(w) - cut for w in wavs], lengths, types, snrs, seed)
    s, n, x, counts, _ = mix_batch(torch.from_numpy(np.concatenate(wavs)).cuda(), [len(w) for w in wavs], torch.cat(bank),
                                   base[idx] + start, snr_db, cut, joint_norm)
    return s, n, x, counts, snr_db


@pytest.mark.parametrize("labels", ["noisy_labels", "noisy_vad_labels", "noisy_wiener_labels"])
def test_make_train_set(tmp_path, labels):
    """X is |stft_batch(x)|^2 of the mixed batch and Y the labels of the clean STFT, bit for bit (the same kernels); mean
    and std are float64 numpy over the returned X to one float32 rounding; the .npy files load as (F, 1)."""
    need_gpu()
    from vaenmf import stft as vstft, target as vtarget
    from vaenmf._lib import check, lib
    from vaenmf.dataset import make_train_set
    raw, files, noise = _tree(tmp_path)
    snrs = (-5.0, -2.5, 0.0, 2.5, 5.0)
    out_dir = str(tmp_path) + "/export"
    ts = make_train_set(files, raw, noise, labels=labels, snrs=snrs, fs=FS, wlen_sec=WLEN, hop_percent=HOP, batch_size=2, seed=4,
                        out_dir=out_dir)
    s, n, x, counts, snr_db = _mixed(raw, files, noise, snrs, TYPES, 4, False)
    assert ts.snr_db == snr_db and counts == [int(sec * FS) + i for i, sec in enumerate(SECONDS)]
    X, fc = vstft.stft_batch(x, counts, FS, WLEN, HOP)
    NT, Fs = X.shape[:2]
    P = torch.empty(NT, Fs, device="cuda")
    check(lib().vaenmf_power_spec(X.data_ptr(), P.data_ptr(), NT * Fs, torch.cuda.current_stream().cuda_stream))
    assert ts.frame_counts == fc and ts.X.shape == (F, NT) and ts.X.dtype == np.float32
    assert np.array_equal(_bits(ts.X), _bits(np.ascontiguousarray(P[:, :F].t().cpu().numpy())))
    S = torch.view_as_complex(vstft.stft_batch(s, counts, FS, WLEN, HOP)[0])[:, :F].cpu().numpy()
    N = torch.view_as_complex(vstft.stft_batch(n, counts, FS, WLEN, HOP)[0])[:, :F].cpu().numpy()
    off = np.concatenate([[0], np.cumsum(fc)])
    assert ts.Y.shape == ((1, NT) if labels == "noisy_vad_labels" else (F, NT)) and ts.Y.dtype == np.float32
    for u in range(len(files)):
        Su, Nu = np.ascontiguousarray(S[off[u]:off[u + 1]].T), np.ascontiguousarray(N[off[u]:off[u + 1]].T)
        want = {"noisy_labels": lambda: vtarget.clean_speech_IBM(Su, 0.999, 0.999),
                "noisy_vad_labels": lambda: vtarget.clean_speech_VAD(Su, 0.999, 0.999),
                "noisy_wiener_labels": lambda: vtarget.ideal_wiener_mask(Su, Nu, 1e-8)}[labels]()
        assert np.array_equal(_bits(np.ascontiguousarray(ts.Y[:, off[u]:off[u + 1]])), _bits(np.ascontiguousarray(want))), u
    m_ref, s_ref = dc.mean_std_ref(ts.X)
    assert np.all(np.abs(ts.mean[:, 0] - m_ref) <= (2.0 ** -24 + 1e-12) * m_ref)
    assert np.all(np.abs(ts.std[:, 0] - s_ref) <= (2.0 ** -24 + 1e-9) * s_ref)
    mean, std = np.load(out_dir + "/trainset_mean.npy"), np.load(out_dir + "/trainset_std.npy")
    assert mean.shape == std.shape == (F, 1) and np.array_equal(mean, ts.mean) and np.array_equal(std, ts.std)
    z = np.load(out_dir + "/CSR-1-WSJ-0_%s.npz" % labels)
    assert np.array_equal(z["X_train"], ts.X) and np.array_equal(z["Y_train"], ts.Y) and list(z["frame_counts"]) == fc


def test_make_test_set(tmp_path, capsys):
    """The written wavs hold the device s, n, x within 1 LSB (compared on the writer's scale: wavio.write stores
    round(32767 v), wavio.read returns code / 32768); the pickle holds the returned list; driver.evaluate (2 EM iterations)
    and run_metrics.main read the tree and give finite metrics."""
    need_gpu()
    from vaenmf import run_metrics, wavio
    from vaenmf.dataset import make_test_set
    from vaenmf.driver import evaluate
    from vaenmf.pipeline import Reconstructor
    raw, files, noise = _tree(tmp_path)
    proc, out = str(tmp_path) + "/processed/", str(tmp_path) + "/model/"
    snr = make_test_set(files, raw, noise, proc, "test", noise_types=TYPES, fs=FS, batch_size=2, seed=1)
    s, n, x, counts, snr_db = _mixed(raw, files, noise, (-5.0, 0.0, 5.0), TYPES, 1, True)
    assert snr == snr_db and len(snr) == 5 and all(type(v) is float for v in snr)
    with open(proc + "CSR-1-WSJ-0/si_et_05_snr_db.p", "rb") as f:
        assert pickle.load(f) == snr
    parts = [[p.cpu().numpy().astype(np.float64) for p in torch.split(t, counts)] for t in (s, n, x)]
    for i, rel in enumerate(files):
        for k, suffix in enumerate(("_s.wav", "_n.wav", "_x.wav")):
            w, fs = wavio.read(proc + os.path.splitext(rel)[0] + suffix)
            assert fs == FS and len(w) == counts[i]
            assert np.max(np.abs(w * 32768.0 - parts[k][i] * 32767.0)) <= 1.0, (rel, suffix)
        assert max(np.abs(parts[k][i]).max() for k in range(3)) == 1.0                # the joint peak is full scale
    _, params, _, meta = load_case("m1_f65")
    rec = Reconstructor(params, F, meta["K"], niter=2, model="M1", fs=FS, wlen_sec=WLEN, max_frames=4096, max_utts=8)
    written = evaluate(rec, files, proc, out, batch_size=8)
    assert len(written) == 5
    capsys.readouterr()
    rows, _ = run_metrics.main(files, proc, out, snr)
    assert len(rows) == 5 and np.all(np.isfinite(np.asarray(rows)))
