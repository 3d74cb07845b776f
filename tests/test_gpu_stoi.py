"""STOI / ESTOI on the GPU (csrc/stoi.hip, vaenmf/metrics.py) against the float64 numpy restatement of
tests/stoi_cases.py: a ragged batch of every boundary of the framing, the reference's committed utterances through the
whole path (16 kHz int16 -> device resampler -> score), independence of the batch, the buffer contract of the three
device entry points, and run_metrics with the ESTOI column.

Bounds.  Everything on the device is float64 on float32 samples, as in the restatement, so the two differ by the order of
their sums only: tob agrees to 1e-9 of the utterance's largest band magnitude and d to 1e-6 absolute -- three orders above
what rounding the 10 kHz signals to float32 moves d (1.5e-9 on the reference's utterances) and 500 times below half a
unit of the third decimal the statistics table prints.  Every case first asserts a threshold margin >= 1e-3 dB in the
restatement: a frame closer than that to the 40 dB threshold could flip its keep decision on a float-level difference."""
import functools
import os

import numpy as np
import pytest
import torch

import stoi_cases as sc
from guarded import Arena
from helpers import need_gpu

pytestmark = pytest.mark.gpu

TOB_REL, D_ABS, MIN_MARGIN_DB = 1e-9, 1e-6, 1e-3


# ------------------------------------------------------------------------------------------------------------ references
@functools.lru_cache(maxsize=None)
def _batch():
    return sc.boundary_batch()


@functools.lru_cache(maxsize=None)
def _refs(extended):
    """The restatement of every utterance of the boundary batch; computed once, never modified."""
    return [sc.core(x, y, extended) for _, x, y in _batch()]


def _geometry(counts):
    """Offsets of the concatenated per-utterance arrays: frames, tob rows."""
    g = [sc.geometry(T) for T in counts]
    return (np.concatenate([[0], np.cumsum([a for a, _, _ in g])]).astype(int),
            np.concatenate([[0], np.cumsum([b for _, b, _ in g])]).astype(int))


def _cat(xs):
    return torch.from_numpy(np.concatenate([np.asarray(x, np.float32) for x in xs])).cuda()


# --------------------------------------------------------------------------------------------------- the three entry points
def _plain(name, shape, dtype):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    if dtype == torch.float64:
        t.fill_(float("nan"))
    return t


def _run(xs, ys, extended, make=_plain, clean=None, proc=None):
    """vaenmf_stoi_tob, vaenmf_stoi_segments and vaenmf_stoi_batch on buffers from `make` of exactly the stated extents ->
    dict of device tensors (d_seg from the two-call path, d and counts_b from the one-call path)."""
    from vaenmf import metrics as vm
    from vaenmf._lib import check, lib
    from vaenmf.engine import _ptr, _stream
    counts = [len(x) for x in xs]
    off = vm.stoi_offsets(counts)
    foff, poff = _geometry(counts)
    U, NF, NS = len(xs), int(foff[-1]), int(poff[-1])
    nbytes = lib().vaenmf_stoi_work_bytes(U, off.ctypes.data)
    assert nbytes > 0
    r = dict(off=off, foff=foff, poff=poff)
    r["clean"] = _cat(xs) if clean is None else clean
    r["proc"] = _cat(ys) if proc is None else proc
    r["keep"] = make("keep", (NF,), torch.int32)
    r["counts"] = make("counts", (U, 3), torch.int32)
    r["tob_x"] = make("tob_x", (NS, 16), torch.float64)
    r["tob_y"] = make("tob_y", (NS, 16), torch.float64)
    r["d_seg"] = make("d_seg", (U,), torch.float64)
    r["d"] = make("d", (U,), torch.float64)
    r["counts_b"] = make("counts_b", (U, 3), torch.int32)
    work = make("work", ((nbytes + 7) // 8,), torch.int64)
    check(lib().vaenmf_stoi_tob(_ptr(r["clean"]), _ptr(r["proc"]), U, off.ctypes.data, _ptr(r["keep"]), _ptr(r["counts"]),
                                _ptr(r["tob_x"]), _ptr(r["tob_y"]), _ptr(work), nbytes, _stream()))
    check(lib().vaenmf_stoi_segments(_ptr(r["tob_x"]), _ptr(r["tob_y"]), _ptr(r["counts"]), U, off.ctypes.data, int(extended),
                                     _ptr(r["d_seg"]), _ptr(work), nbytes, _stream()))
    check(lib().vaenmf_stoi_batch(_ptr(r["clean"]), _ptr(r["proc"]), U, off.ctypes.data, int(extended), _ptr(r["d"]),
                                  _ptr(r["counts_b"]), _ptr(work), nbytes, _stream()))
    torch.cuda.synchronize()
    return r


@functools.lru_cache(maxsize=None)
def _device(extended):
    """The boundary batch through the three entry points; computed once, never modified."""
    cases = _batch()
    return _run([x for _, x, _ in cases], [y for _, _, y in cases], extended)


def _rows(r, u, M):
    """(tob_x, tob_y) [M][16] of utterance u as numpy."""
    p = int(r["poff"][u])
    return r["tob_x"][p:p + M].cpu().numpy(), r["tob_y"][p:p + M].cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------- tests
def test_cases_keep_their_distance_from_the_threshold():
    """No case may be skipped for a small margin; the seeds are chosen so that none has one."""
    for (name, x, _), ref in zip(_batch(), _refs(True)):
        assert ref["margin"] >= MIN_MARGIN_DB, (name, ref["margin"])
    names = [n for n, _, _ in _batch()]
    by = dict(zip(names, _refs(True)))
    assert [by[n]["counts"] for n in ("T0", "T255", "T256", "T257", "T384", "T385")] == [(0, 0, 0)] * 3 + [(1, 1, 0)] * 2 + [(2, 2, 0)]
    assert [by["k%d" % k]["counts"] for k in (30, 31, 32, 33)] == [(30, 30, 0), (31, 31, 1), (32, 32, 2), (33, 33, 3)]
    assert by["gap_mid"]["counts"] == (69, 59, 29) and by["gap_head"]["k"] < 69 and by["gap_tail"]["k"] < 69
    assert by["zeros"]["counts"] == (38, 38, 8)


@pytest.mark.parametrize("extended", [True, False])
def test_boundary_batch_against_the_restatement(extended):
    """keep and counts exactly, tob to 1e-9 of the utterance's largest band magnitude, d to 1e-6, from the two-call path
    and from vaenmf_stoi_batch; the degenerate utterances score 1e-5, digital silence 0, y = x 1."""
    need_gpu()
    refs, r = _refs(extended), _device(extended)
    counts = r["counts"].cpu().numpy()
    assert np.array_equal(counts, r["counts_b"].cpu().numpy())
    keep, d, d_seg = r["keep"].cpu().numpy(), r["d"].cpu().numpy(), r["d_seg"].cpu().numpy()
    assert np.array_equal(d.view(np.int64), d_seg.view(np.int64))           # one pass or two: the same bits
    worst_tob = worst_d = 0.0
    for u, ((name, x, _), ref) in enumerate(zip(_batch(), refs)):
        assert ref["margin"] >= MIN_MARGIN_DB, (name, ref["margin"])
        assert tuple(counts[u]) == ref["counts"], (name, counts[u], ref["counts"])
        assert np.array_equal(keep[r["foff"][u]:r["foff"][u + 1]], ref["keep"]), name
        M = max(ref["k"] - 1, 0)
        tx, ty = _rows(r, u, M)
        for got, want in ((tx, ref["tob_x"]), (ty, ref["tob_y"])):
            if M == 0:
                continue
            assert np.all(got[:, 15] == 0.0), name
            scale = float(want.max())
            err = float(np.abs(got[:, :15] - want.T).max())
            assert err <= TOB_REL * scale, (name, err, scale)
            if scale > 0:
                worst_tob = max(worst_tob, err / scale)
        err = abs(d[u] - ref["d"])
        worst_d = max(worst_d, err)
        assert err <= D_ABS, (name, d[u], ref["d"])
    print("boundary batch, extended=%s: max |tob - ref| / max band = %.2e, max |d - ref| = %.2e" % (extended, worst_tob, worst_d))
    by = {n: d[u] for u, (n, _, _) in enumerate(_batch())}
    assert all(by[n] == sc.NO_SCORE for n in ("T0", "T255", "T256", "T257", "T384", "T385", "k30"))
    assert by["zeros"] == 0.0 and abs(by["same"] - 1.0) <= D_ABS


def test_rows_past_the_kept_frames_are_left_alone():
    """tob rows >= M of an utterance (silent frames removed) keep what the buffer held."""
    need_gpu()
    r, refs = _device(True), _refs(True)
    some = 0
    for u, ref in enumerate(refs):
        M = max(ref["k"] - 1, 0)
        rest_x = r["tob_x"][int(r["poff"][u]) + M:int(r["poff"][u + 1])]
        rest_y = r["tob_y"][int(r["poff"][u]) + M:int(r["poff"][u + 1])]
        assert bool(torch.isnan(rest_x).all()) and bool(torch.isnan(rest_y).all())
        some += rest_x.shape[0]
    assert some >= 30                                                        # the three gapped utterances drop 10 frames each


@functools.lru_cache(maxsize=None)
def _known():
    utts = sc.reference_utterances()
    names = sorted(utts)
    return names, utts, {n: sc.score(utts[n][0], utts[n][1], 16000, True) for n in names}


def test_known_answers_through_the_full_path():
    """The reference's utterances a and b (16 kHz) in one batch: device resampler, then the score.  ESTOI rounds to the two
    decimals the reference printed and agrees with the restatement (fed scipy's resample_poly rounded to float32) within
    1e-6; the counts (932 frames in b: the scan carries its prefix over four chunks) are the restatement's; stoi() with
    pystoi's signature gives the batch's value."""
    need_gpu()
    from vaenmf import metrics as vm
    from vaenmf.resample import resample_batch
    from vaenmf._lib import check, lib
    from vaenmf.engine import _ptr, _stream
    names, utts, refs = _known()
    assert names[:2] == ["a", "b"]
    counts = [len(utts[n][0]) for n in names]
    clean, proc = _cat([utts[n][0] for n in names]), _cat([utts[n][1] for n in names])
    d = vm.stoi_batch(clean, proc, counts, 16000, extended=True)
    for u, n in enumerate(names):
        ref = refs[n]
        assert ref["margin"] >= MIN_MARGIN_DB
        print("%s: ESTOI %.6f, restatement %.6f (difference %.2e), printed %.2f" % (n, d[u], ref["d"], abs(d[u] - ref["d"]), utts[n][2]))
        assert round(float(d[u]), 2) == utts[n][2]
        assert abs(d[u] - ref["d"]) <= D_ABS
    # the counts of the same pass, from the C entry point
    c10, n10 = resample_batch(clean, counts, 16000, 10000)
    p10, _ = resample_batch(proc, counts, 16000, 10000)
    off = vm.stoi_offsets(n10)
    work = vm.stoi_work(off, clean.device)
    dd = torch.empty(len(names), dtype=torch.float64, device="cuda")
    cnt = torch.empty(len(names), 3, dtype=torch.int32, device="cuda")
    check(lib().vaenmf_stoi_batch(_ptr(c10), _ptr(p10), len(names), off.ctypes.data, 1, _ptr(dd), _ptr(cnt), _ptr(work), work.numel(), _stream()))
    assert [tuple(c) for c in cnt.cpu().numpy()] == [refs[n]["counts"] for n in names]
    assert np.array_equal(dd.cpu().numpy().view(np.int64), d.view(np.int64))
    # classic STOI of the same pair, and the single-signal call
    c = vm.stoi_batch(clean, proc, counts, 16000, extended=False)
    ref_c = sc.score(utts["a"][0], utts["a"][1], 16000, False)["d"]
    assert abs(c[0] - ref_c) <= D_ABS and c[0] > d[0]
    assert vm.stoi(utts["a"][0], utts["a"][1], 16000, extended=True) == d[0]
    assert vm.stoi(utts["a"][0].astype(np.float64), utts["a"][1].astype(np.float64), 16000) == c[0]      # extended=False is pystoi's default


def test_batch_independence():
    """Every utterance of the boundary batch alone, and in the reversed batch, has the bits it has in the batch: d of both
    variants, keep, counts and its tob rows."""
    need_gpu()
    cases = _batch()
    for extended in (True, False):
        r = _device(extended)
        rev = _run([x for _, x, _ in cases[::-1]], [y for _, _, y in cases[::-1]], extended)
        U = len(cases)
        for u, (name, x, y) in enumerate(cases):
            others = [(rev, U - 1 - u)]
            if extended or name in ("k31", "gap_mid", "zeros"):              # alone: every case once, three more in the classic form
                others.append((_run([x], [y], extended), 0))
            for o, v in others:
                assert torch.equal(o["d"][v].view(torch.int64), r["d"][u].view(torch.int64)), name
                assert torch.equal(o["counts"][v], r["counts"][u]), name
                assert torch.equal(o["keep"][int(o["foff"][v]):int(o["foff"][v + 1])], r["keep"][int(r["foff"][u]):int(r["foff"][u + 1])]), name
                M = max(int(r["counts"][u, 1]) - 1, 0)
                for a, b in zip(_rows(o, v, M), _rows(r, u, M)):
                    assert np.array_equal(a.view(np.int64), b.view(np.int64)), name


@pytest.mark.parametrize("poison", ["nan", "1e30"])
def test_buffer_contract(poison):
    """The three device entry points on buffers of exactly the stated extents at 16 (mod 256), carved from a poisoned
    arena: every guard intact, the inputs unchanged, tob rows >= M still poison, and every result the bits of the
    unguarded run."""
    need_gpu()
    cases = _batch()
    xs, ys = [x for _, x, _ in cases], [y for _, _, y in cases]
    arena = Arena(16 << 20, poison, device="cuda")
    clean = arena.carve("clean", (sum(len(x) for x in xs),), torch.float32)
    proc = arena.carve("proc", clean.shape, torch.float32)
    clean.copy_(_cat(xs))
    proc.copy_(_cat(ys))
    arena.snapshot(["clean", "proc"])
    for extended in (True, False):
        tag = "e%d_" % extended
        g = _run(xs, ys, extended, make=lambda name, shape, dtype: arena.carve(tag + name, shape, dtype), clean=clean, proc=proc)
        arena.check("stoi extended=%s" % extended)
        arena.unchanged(what="stoi extended=%s" % extended)
        r = _device(extended)
        for k in ("d", "d_seg", "keep", "counts", "counts_b"):
            assert torch.equal(g[k].view(torch.int32), r[k].view(torch.int32)), k
        cnt = r["counts"].cpu().numpy()
        for u in range(len(cases)):
            p0, p1, M = int(r["poff"][u]), int(r["poff"][u + 1]), max(int(cnt[u, 1]) - 1, 0)
            for k in ("tob_x", "tob_y"):
                assert torch.equal(g[k][p0:p0 + M].view(torch.int32), r[k][p0:p0 + M].view(torch.int32)), (k, u)
                assert bool((g[k][p0 + M:p1].view(torch.int32) == arena.word).all()), (k, u)


def test_refusals_and_the_empty_batch():
    need_gpu()
    from vaenmf import metrics as vm
    from vaenmf._lib import VaenmfError, check, lib
    from vaenmf.engine import _ptr, _stream
    assert vm.stoi_batch(torch.empty(0, device="cuda"), torch.empty(0, device="cuda"), [], 10000).shape == (0,)
    off = vm.stoi_offsets([5000])
    x = torch.zeros(5000, device="cuda")
    d = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    work = vm.stoi_work(off, x.device)
    with pytest.raises(VaenmfError, match="work_bytes"):
        check(lib().vaenmf_stoi_batch(_ptr(x), _ptr(x), 1, off.ctypes.data, 1, _ptr(d), None, _ptr(work), work.numel() - 8, _stream()))
    torch.cuda.synchronize()
    assert float(d[0]) == 7.0
    with pytest.raises(ValueError):
        vm.stoi_batch(x, x[:-1], [5000], 10000)
    with pytest.raises(ValueError):
        vm.stoi(np.zeros(10), np.zeros(11), 10000)


def test_run_metrics_with_the_estoi_column(tmp_path, capsys):
    """compute_metrics / main with estoi=True on the committed nine-utterance subset (ragged, 16 kHz; the noisy mixture
    stands in for the model's estimate): four columns, the first three the bits of the estoi=False call, the fourth the
    restatement's ESTOI within 1e-6, and the printed table gains its ESTOI rows."""
    need_gpu()
    from vaenmf import wavio, run_metrics
    z = np.load(sc.GOLDEN + "/processed_subset9.npz")
    proc, out = str(tmp_path) + "/processed/", str(tmp_path) + "/model/"
    files = []
    for i, rel in enumerate(z["rel"]):
        rel = str(rel)
        stem = os.path.splitext(rel)[0]
        for base in (proc, out):
            os.makedirs(os.path.dirname(base + rel), exist_ok=True)
        for k in "sn":
            wavio.write(proc + stem + "_%s.wav" % k, z["u%d_%s" % (i, k)] / 32768.0, 16000)
        wavio.write(out + stem + "_s_est.wav", z["u%d_x" % i] / 32768.0, 16000)
        files.append(rel)
    base = run_metrics.compute_metrics(files, proc, out)
    snr = [-5.0, 0.0, 5.0] * 3
    capsys.readouterr()
    rows, st = run_metrics.main(files, proc, out, snr, estoi=True)
    text = capsys.readouterr().out
    assert len(rows) == 9 and all(len(r) == 4 for r in rows) and all(len(r) == 3 for r in base)
    assert np.array_equal(np.asarray([r[:3] for r in rows]).view(np.int64), np.asarray(base).view(np.int64))
    assert rows == run_metrics.compute_metrics(files, proc, out, batch_size=4, estoi=True)      # batches of 4, 4 and 1
    for rel, r in zip(files, rows):
        stem = os.path.splitext(rel)[0]
        ref = sc.score(wavio.read(proc + stem + "_s.wav")[0], wavio.read(out + stem + "_s_est.wav")[0], 16000, True)
        assert ref["margin"] >= MIN_MARGIN_DB and ref["J"] > 0
        assert abs(r[3] - ref["d"]) <= D_ABS, (rel, r[3], ref["d"])
    assert st.shape == (4, 4, 3) and st[0, 3, 0] == 9 and abs(st[0, 3, 1] - sum(r[3] for r in rows)) < 1e-12
    assert text.count("ESTOI") == 4 and text.count("SI-SDR") == 4           # overall and three input SNRs
