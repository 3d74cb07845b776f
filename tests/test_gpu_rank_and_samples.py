"""The M-step and Wiener kernels over the NMF rank K and the samples per frame R, to fp32 bounds.

tests/test_gpu_bin_counts.py sweeps the bin count F.  The other two sizes that pick a kernel are the rank (1..32, padded
to KP = 8 / 16 / 32) and the number of posterior samples per frame, which no entry point limits: the streaming kernels of
stream.hip read a frame's stored rows in register batches of RowBatch::RB rows (and wstats_stream in halves of HB), the
decoding kernels of engine.hip in chunks of 32 samples.  stream_class() and decode_class() (tests/dispatch_model.py) restate that dispatch, a CPU
test checks that the case lists below reach every form of it, and the GPU tests check the plan queries against it.

The reference.  The oracle is given the variances the device itself produced -- eng.stored_variances(R) for the store,
eng.decode(R) for the decoding path -- so that only the arithmetic of the M-step / Wiener kernels separates the two, in
both precisions: the kernels' own arithmetic is fp32 on the stored rows.  The modes of decode_kernel share one decode
routine (decode_tiles, the odd last bin's nyq_logit included), so mode STORE writes the very variances the other modes
use.  The reference proper is a float64 evaluation of the same formulas (m_step64, gains_step64, wiener64 in tests/em_support.py: mcem.py:90-152,
:543-578, :486-488, :70 without any intermediate cast); with e32 the error of the float32 oracle against it, a device
result must lie within

    max(floor, 16 * e32)        floor: 2e-5 for W, H, g, the masks and the filtered spectrograms, 1e-6 for the cost

of the float64 values.  The floors are the project's figures for two fp32 implementations that differ in summation order
(test_stored_m_step_and_wiener_match_the_decoding_ones, float rows); the factor 16 covers v_rcp_f32 / v_sqrt_f32 /
v_log_f32 (about 1 ulp each) and per-lane sequential sums against numpy's pairwise ones.  W, H, g and the cost are
relative errors (max over the elements), the masks absolute, S_hat / N_hat relative in L2.

What keeps that honest: test_one_wrong_row_exceeds_the_bounds (no GPU) replaces one sample row by its neighbour, at every
batch edge of the case, in the float64 evaluation, and asserts that the bound is at most a quarter of the smallest change
that causes in g and in the masks -- so a kernel that reads a wrong row, skips one or counts one twice cannot pass.

The samples.  The stored path runs the chain with the device generator; a rejected step repeats a sample, so there two
neighbouring rows can be equal and the wrong-row figures, computed from the independent draws of es.inputs, stand in for
the chain's.  The decoding path is given those very draws.  What the sweep found is such a row: wstats_stream_kernel
dropped the fifth of five float rows in three 256-bin chunks (RB = 5, two half batches of 2), W off by 1e-2.

Measured on an MI355X, largest error over the sweep (every figure at most 0.05 of its bound):
                      W        H        g        cost     masks    S_hat    N_hat
  stored   bf16x3     4.7e-7   3.8e-7   2.5e-7   4.9e-8   6.9e-7   2.0e-7   2.0e-7
  stored   bf16       5.0e-7   3.7e-7   2.5e-7   4.3e-8   7.7e-7   2.2e-7   2.4e-7
  decoding bf16x3     3.9e-7   3.3e-7   1.9e-7   3.3e-8   2.2e-7   7.8e-8   7.6e-8
  decoding bf16       3.9e-7   3.3e-7   1.9e-7   3.0e-8   2.3e-7   7.7e-8   7.4e-8
  float32 oracle      1.7e-6   2.3e-6   9.1e-7   3.6e-7   4.7e-7   1.5e-7   1.3e-7      (e32; the largest bound: H 3.7e-5, cost 5.7e-6)
Stored rows against eng.decode: bf16x3 equal bit for bit (the extra bin 6.3e-6), bf16 3.9e-3 (the extra bin 6.1e-3);
eng.decode against decoder_forward 1.6e-5 / 9.5e-3.  One wrong row moves g by at least 4.1 bounds and the masks by at
least 97 (test_one_wrong_row_exceeds_the_bounds prints the figures).
"""
import functools

import numpy as np
import pytest
import torch

import vaenmf_oracle as orc
import em_support as es
from dispatch_model import COUNTS, N_WAVE_TILES, decode_class, shape_class, stream_class
from helpers import need_gpu, rel_err

gpu = pytest.mark.gpu        # (per test: the three tests on the restatement, the float64 formulas and the bound run without a GPU)

PRECISIONS = ["bf16x3", "bf16"]
BURNINS = lambda R: (0, 3, R + 5)          # none, short (shorter than R from R = 5 up), longer than R: the slot map of R + 1 slots


def _stored_runs(F, K, R, variant, precision, n_cus=256):
    """The M-steps the stored test runs at one case: the default, and where the shape has the group / fused W-statistics
    kernels also the tile kernel and the two-kernel path.  [(environment, stream_class, Q_W_FUSED)]"""
    runs = []
    for env, kw in (({}, {}), ({"VAENMF_WGROUP": "0"}, {"wgroup": False}), ({"VAENMF_WFUSED": "0"}, {"wfused": False})):
        sc = stream_class(F, K, R, precision, variant, N_WAVE_TILES, n_cus, **kw)
        name = sc["wstats"]["kernel"] if sc["wstats"] else None
        if env and [r for r in runs if r[1]["wstats"] == sc["wstats"]]:
            continue                                                       # the switch changes nothing at this shape
        runs.append((env, sc, {"wstats_group": 2, "wstats_fused": 1}.get(name, 0)))
    return runs


# ---------------------------------------------------------------------------------------------------------------------
# the cases of the stored path: (F, K, R, variant), each run in both precisions
STORED_CASES = [
    # the bench shapes' neighbours and the reference's defaults (R = 10, 25, 30, 75), large ranks, the largest shape
    (257, 8, 75, "M1"), (513, 32, 33, "M1"), (640, 17, 17, "M1"), (513, 9, 25, "M1"), (640, 32, 75, "M1"), (513, 32, 75, "M1"),
    (257, 2, 25, "M1"), (256, 8, 40, "M1"), (640, 31, 40, "M1"), (529, 32, 65, "M1"), (442, 16, 16, "M1"), (513, 31, 8, "M1"),
    (257, 16, 2, "M1"),
    # one 256-bin chunk with a partly filled last 4-bin chunk (TAIL): rank classes 8 / 16 / 32 over the row classes
    (201, 1, 1, "M1"), (201, 1, 10, "M1"), (201, 1, 16, "M1"), (201, 1, 30, "M1"), (201, 1, 32, "M1"), (201, 1, 64, "M1"),
    (201, 3, 10, "M1"), (201, 3, 30, "M1"), (201, 5, 10, "M1"), (201, 5, 30, "M1"), (201, 7, 10, "M1"), (201, 7, 30, "M1"),
    (201, 8, 30, "M1"), (201, 9, 1, "M1"), (201, 9, 9, "M1"), (201, 9, 17, "M1"), (201, 9, 33, "M1"), (201, 9, 64, "M1"),
    (201, 17, 1, "M1"), (201, 17, 9, "M1"), (201, 17, 17, "M1"), (201, 17, 33, "M1"), (201, 17, 64, "M1"),
    # two chunks, no tail
    (260, 1, 5, "M1"), (260, 1, 9, "M1"), (260, 1, 32, "M1"), (260, 1, 33, "M1"), (260, 1, 64, "M1"), (260, 9, 1, "M1"),
    (260, 9, 5, "M1"), (260, 9, 9, "M1"), (260, 9, 32, "M1"), (260, 9, 33, "M1"), (260, 9, 64, "M1"), (260, 17, 1, "M1"),
    (260, 17, 5, "M1"), (260, 17, 9, "M1"), (260, 17, 17, "M1"), (260, 17, 32, "M1"),
    # two chunks with a tail; three chunks with a tail (RB = 10 / 5, HB = 5 / 2) and with the extra bin
    (442, 1, 1, "M1"), (442, 9, 30, "M1"),
    (514, 1, 1, "M1"), (514, 1, 5, "M1"), (514, 1, 6, "M1"), (514, 1, 25, "M1"), (514, 1, 30, "M1"), (514, 9, 5, "M1"),
    (514, 9, 6, "M1"), (514, 9, 11, "M1"), (514, 9, 30, "M1"), (514, 17, 1, "M1"), (514, 17, 5, "M1"), (514, 17, 6, "M1"),
    (514, 17, 30, "M1"), (529, 9, 1, "M1"), (514, 1, 4, "M1"), (514, 9, 4, "M1"), (514, 17, 4, "M1"),
    # labels (Dy = 1) and the fixed noise PSD (gains only)
    (201, 5, 33, "M2"), (257, 8, 10, "M2"), (513, 16, 30, "M2"), (640, 17, 11, "M2"),
    (201, 1, 10, "noNMF"), (201, 1, 40, "noNMF"), (257, 7, 30, "noNMF"), (260, 32, 33, "noNMF"), (514, 8, 9, "noNMF"),
    (514, 16, 25, "noNMF"),
]
# decoding path: (F, K, R, variant, Rcap); Rcap > R: the sample stride of Zs differs from the count
DECODE_CASES = [
    (513, 32, 75, "M1", 75), (257, 8, 75, "M1", 80), (640, 17, 17, "M1", 20), (640, 32, 64, "M1", 64), (260, 2, 25, "M1", 25),
    (514, 31, 40, "M1", 44), (529, 16, 17, "M1", 17),
    (201, 1, 16, "M1", 19), (201, 1, 65, "M1", 68), (201, 17, 32, "M1", 35), (256, 1, 1, "M1", 4), (256, 9, 1, "M1", 4),
    (256, 17, 33, "M1", 33), (442, 1, 1, "M1", 4), (442, 9, 33, "M1", 33), (442, 17, 1, "M1", 4), (513, 9, 33, "M1", 33),
    (513, 17, 1, "M1", 4),
    (201, 9, 33, "M2", 40), (513, 8, 30, "M2", 30), (257, 8, 10, "noNMF", 10), (442, 16, 40, "noNMF", 48),
]


def _stream_tokens(cases):
    """What the stored test reaches with `cases`, in both precisions."""
    t = set()
    for F, K, R, variant in cases:
        for prec in PRECISIONS:
            for env, sc, _ in _stored_runs(F, K, R, variant, prec):
                ws, hg, wf = sc["wstats"], sc["hg"], sc["wf"]
                st, NCH, KP = hg["store"], hg["NCH"], hg["KP"]
                for kd, s in (("wstats", ws), ("hg", hg), ("wf", wf)):
                    if s is None:
                        continue
                    if s["kernel"] in ("wstats_stream", "wstats_stream2", "hg_stream", "wf_stream"):
                        t.add(("inst", kd, NCH, KP, st))
                    t.add(("rows", s["kernel"], NCH, KP, st, s["RB"], s["rows"]))
                    if kd != "wstats":
                        t.add(("tail", kd, NCH, st, s["TAIL"]))
                    if not s["w_in_lds"]:
                        t.add(("w_not_in_lds", kd, st))
                    t.add(("extra_bin", kd, NCH, st, s["extra_bin"]))
                if hg["RT"]:
                    t.add(("rt", NCH, KP, st, hg["RT"]))
                elif hg["rt_shape"]:
                    t.add(("rt_with_tail", NCH, KP, st, hg["rt_shape"]))
                if ws and ws["kernel"] == "wstats_stream2" and R in (1, ws["RB"]):
                    t.add(("stream2", st, "R=1" if R == 1 else "R=RB"))
                if ws and ws["kernel"] in ("wstats_group", "wstats_fused"):
                    t.add((ws["kernel"], K, R))
                if hg["gains_only"]:
                    t.add(("gains_only", st, "one" if hg["rows"] == "one" else "several"))
                t.add(("rank", KP, st, "K=1" if K == 1 else ("K=KP" if K == KP else "K<KP")))
    return t


def _stream_required():
    t = set()
    for st in ("bf16", "float"):
        for NCH in (1, 2, 3):
            RB = {"bf16": (32, 16, 10), "float": (16, 8, 5)}[st][NCH - 1]        # rows of a register batch: RowBatch::RB
            for KP in (8, 16, 32):
                for kd in ("wstats", "hg", "wf"):
                    t.add(("inst", kd, NCH, KP, st))                      # the 54 of launch_st
                # every row loop of every kernel: wstats_stream has the half-batch form below RB (stream2 takes NCH 1, KP 8)
                if NCH == 1 and KP == 8:
                    t |= {("rows", "wstats_stream", NCH, KP, st, RB, r) for r in ("exact", "partial")}
                    t.add(("rows", "wstats_stream2", NCH, KP, st, RB, "one"))
                else:
                    t |= {("rows", "wstats_stream", NCH, KP, st, RB, r) for r in ("half", "one", "exact", "partial")}
                t |= {("rows", "wf_stream", NCH, KP, st, RB, r) for r in ("one", "exact", "partial")}
                whole = (st == "bf16" and NCH == 2 and KP <= 16) or (st == "float" and NCH == 1 and KP == 8)   # hg_stream's RBX
                t |= {("rows", "hg_stream", NCH, KP, st, 32 if whole else RB, r) for r in ("one", "exact", "partial")}
            for kd in ("hg", "wf"):
                t |= {("tail", kd, NCH, st, True), ("tail", kd, NCH, st, False)}
                t |= {("extra_bin", kd, NCH, st, True), ("extra_bin", kd, NCH, st, False)}
        for RT in (10, 30):                                                # the exact-count forms, and the same R with TAIL
            t |= {("rt", 1, 8, st, RT), ("rt_with_tail", 1, 8, st, RT)}
        t |= {("stream2", st, "R=1"), ("stream2", st, "R=RB")}
        t |= {("gains_only", st, "one"), ("gains_only", st, "several")}
        t |= {("w_not_in_lds", kd, st) for kd in ("wstats", "hg", "wf")}
        for KP in (8, 16, 32):
            t |= {("rank", KP, st, "K=KP"), ("rank", KP, st, "K<KP")}
        t.add(("rank", 8, st, "K=1"))
    t |= {("rt", 2, 16, "bf16", 30), ("rt_with_tail", 2, 16, "bf16", 30)}
    t |= {("rows", k, 1, 8, "bf16", 32, "one") for k in ("wstats_group", "wstats_fused")}
    t |= {(k, K, R) for k in ("wstats_group", "wstats_fused") for K in (1, 3, 5, 7, 8) for R in (10, 30)}
    return t


def _decode_tokens(cases):
    t = set()
    for F, K, R, variant, Rcap in cases:
        for prec in PRECISIONS:
            d = decode_class(F, K, R, prec)
            more = 1 if d["chunks"] == 1 else "more"
            if variant == "noNMF":
                t.add(("mode_g", d["split"], d["chunks"]))
                modes = ("WF",)
            else:
                modes = ("WSTATS", "HG", "WF")
            for mode in modes:
                t.add(("mode", mode, d["KP"], d["geom"], d["split"]))
                t.add(("chunks", mode, d["geom"], d["split"], more))
            t |= {("nchunks", d["split"], d["chunks"]), ("rmod", d["split"], d["rmod"]), ("stride", d["split"], Rcap > R),
                  ("extra_bin", d["geom"], d["split"], d["extra_bin"])}
    return t


def _decode_required():
    t = set()
    for split in (True, False):
        for geom in (0, 2, 3, 4):
            for mode in ("WSTATS", "HG", "WF"):
                t |= {("mode", mode, KP, geom, split) for KP in (8, 16, 32)}
                t |= {("chunks", mode, geom, split, 1), ("chunks", mode, geom, split, "more")}
        t |= {("nchunks", split, n) for n in (1, 2, 3)} | {("rmod", split, m) for m in ("0", "1..15", "16", "17..31")}
        t |= {("mode_g", split, 1), ("mode_g", split, 2), ("stride", split, True), ("stride", split, False)}
        t |= {("extra_bin", 3, split, True), ("extra_bin", 3, split, False), ("extra_bin", 4, split, True)}
    return t


def test_sweep_reaches_every_kernel_form_over_rank_and_samples():
    """No GPU: the case lists reach every instantiation launch_st and launch_decode select, every row loop of every
    streaming kernel, and the forms listed in _stream_required / _decode_required."""
    missing = sorted(map(str, _stream_required() - _stream_tokens(STORED_CASES)))
    assert not missing, missing
    missing = sorted(map(str, _decode_required() - _decode_tokens(DECODE_CASES)))
    assert not missing, missing
    # the restatement itself, at shapes whose kernels are known from the code's comments: the bench shapes
    sc = stream_class(257, 8, 30, "bf16", "M1", 6)
    assert (sc["wstats"]["kernel"], sc["hg"]["RT"], sc["hg"]["RB"], sc["hg"]["TAIL"], sc["hg"]["extra_bin"]) == ("wstats_group", 30, 32, False, True)
    assert stream_class(257, 8, 30, "bf16", "M1", 1000)["wstats"]["kernel"] == "wstats_fused"
    sc = stream_class(513, 10, 30, "bf16", "M1", 6)
    assert (sc["wstats"]["kernel"], sc["wstats"]["RB"], sc["wstats"]["HB"], sc["wstats"]["rows"]) == ("wstats_stream", 16, 8, "partial")
    assert (sc["hg"]["NCH"], sc["hg"]["KP"], sc["hg"]["RT"], sc["hg"]["RB"], sc["wf"]["RB"], sc["wf"]["rows"]) == (2, 16, 30, 32, 16, "partial")
    sc = stream_class(640, 32, 10, "bf16x3", "M1", 6)
    assert (sc["hg"]["NCH"], sc["hg"]["RB"], sc["wstats"]["HB"], sc["hg"]["rows"], sc["hg"]["w_in_lds"]) == (3, 5, 2, "exact", False)
    # float rows in three chunks: RB = 5 is odd, two half batches hold 4 rows, the fifth needs the batch loop
    assert [stream_class(514, 9, R, "bf16x3", "M1", 6)["wstats"]["rows"] for R in (2, 4, 5, 6)] == ["half", "one", "exact", "partial"]
    assert stream_class(201, 1, 10, "bf16", "noNMF", 6)["wstats"] is None and stream_class(201, 1, 10, "bf16", "noNMF", 6)["hg"]["gains_only"]
    assert decode_class(513, 32, 75, "bf16") == dict(geom=4, split=False, KP=32, chunks=3, rmod="1..15", extra_bin=True)
    assert len(STORED_CASES) == len(set(STORED_CASES)) and len(DECODE_CASES) == len(set(DECODE_CASES))
    assert len(PRECISIONS) * (len(STORED_CASES) + len(DECODE_CASES)) <= 250


def _oracle_cpu(c, u, variant):
    """The oracle of utterance u in the state of es.inputs, with the variances of its samples from decoder_forward."""
    sl = slice(c.off[u], c.off[u + 1])
    if variant == "noNMF":
        o = orc.MCEMOracleNoNMF(c.Xs[u], es.noise_psd(c)[sl], c.gains[sl], c.Z0[sl], c.ys[u], c.params, 1, orc.NumpyRNG(0))
    else:
        o = orc.MCEMOracle("M2" if c.Dy else "M1", 1)
        o.init_parameters(c.Xs[u], c.params, c.K, 1e-8, orc.NumpyRNG(0), y=c.ys[u], W0=c.W0[u], H0=c.H0[u])
        o.g = c.gains[sl].copy()
    o.compute_Vs(c.Zs[sl])
    return o


def _edge_rows(F, K, R, variant):
    """Rows at the batch edges of every streaming kernel of the case, in both precisions, and of the 32-sample chunks."""
    rows = {0, R - 1, 31, 32, 63, 64}
    for prec in PRECISIONS:
        for s in stream_class(F, K, R, prec, variant, N_WAVE_TILES).values():
            if s:
                rows |= {s["HB"] - 1, s["HB"], s["RB"] - 1, s["RB"]}
    return sorted(r for r in rows if 0 <= r < R)


@functools.lru_cache(maxsize=None)
def _cpu_case(F, K, R, variant):
    """Per utterance: e32 (float32 oracle against the float64 formulas), the bounds, and per edge row the change of every
    quantity when that row is replaced by the one before it (row 0: by the last)."""
    c = es.case_inputs(F, K, R, variant)
    out = []
    for u in range(len(COUNTS)):
        o = _oracle_cpu(c, u, variant)
        Vs = np.asarray(o.Vs, np.float64)
        ref = es.reference(o, variant, Vs64=Vs)[0]
        change = {}
        if R >= 2:
            for r in _edge_rows(F, K, R, variant):
                bad = Vs.copy()
                bad[r] = Vs[r - 1]
                change[r] = es.errors(es.reference(o, variant, Vs64=bad)[0], ref)
        e32 = es.errors(es.reference(o, variant)[1], ref)                     # (last: the oracle's M-step changes its state)
        out.append((e32, es.bounds(e32), change))
    return out


def _all_cases():
    return sorted(set(STORED_CASES) | {d[:4] for d in DECODE_CASES})


def test_float64_formulas_agree_with_the_oracle():
    """No GPU: m_step64 / gains_step64 / wiener64 against the committed float32 oracle over the sweep's cases, 1e-5.
    Both sides are reference code: this tests the restatement of the formulas, not a kernel."""
    worst = {}
    for case in _all_cases():
        for e32, _, _ in _cpu_case(*case):
            for k, v in e32.items():
                worst[k] = max(worst.get(k, 0.0), v)
            assert max(e32.values()) < 1e-5, (case, e32)
    print("float32 oracle against the float64 formulas, largest: " + es.fmt(worst))


def test_one_wrong_row_exceeds_the_bounds():
    """No GPU: the condition on the bound, and the sensitivity of the comparison.  For every case with R >= 2 and every
    edge row, a result computed from the samples with that one row replaced by its neighbour -- what a kernel gives that
    reads a wrong row, skips one or counts one twice -- changes g and the masks by at least four times the bound, and
    es.violations() reports it."""
    tight = {}
    for case in _all_cases():
        if case[2] < 2:
            continue
        for u, (e32, bound, change) in enumerate(_cpu_case(*case)):
            assert change, case
            for r, ch in change.items():
                assert es.violations(ch, bound), (case, u, r, ch, bound)
                for k in ("g", "mask"):
                    assert bound[k] <= ch[k] / 4, (case, u, r, k, ch[k], bound[k])
                for k in ch:
                    tight[k] = min(tight.get(k, np.inf), ch[k] / bound[k])
    print("smallest change of one wrong row over its bound: " + es.fmt(tight))


# ---------------------------------------------------------------------------------------------------------------------
# the kernels
@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("F,K,R,variant", STORED_CASES)
def test_stored_kernels_against_the_oracle_from_the_stored_rows(F, K, R, variant, precision):
    """One chain with the device generator and the store on, at three burn-ins (the slot map); the stored rows against
    eng.decode of the chain's samples (the bounds of test_sample_store_holds_the_samples_variances); then wiener_stored and
    m_step_stored -- with every W-statistics kernel the shape has -- against the float64 formulas fed with the stored rows."""
    need_gpu()
    c = es.case_inputs(F, K, R, variant)
    shp = shape_class(F, K, precision, N_WAVE_TILES, R, es.n_cus())
    runs = _stored_runs(F, K, R, variant, precision, es.n_cus())
    eng, Vb = es.prepare(c, variant, precision, R)
    assert eng.Fs == shp["Fs"] == es.query(eng, "Q_FS") and eng.Kp == shp["Kp"] == es.query(eng, "Q_KP") == runs[0][1]["hg"]["KP"]
    assert es.query(eng, "Q_MSTEP_PATH") == 0                               # (no fused run: the path is the caller's here)
    eng.sample_store(True)
    failures = []
    for call, bi in enumerate(BURNINS(R)):
        tag = "stored %s F=%d K=%d R=%d %s bi=%d" % (precision, F, K, R, variant, bi)
        es.reset(c, eng)
        eng.mh_chain(R, bi, 0.01, call=call)
        assert es.query(eng, "Q_CHAIN_KERNEL") == shp["chain_kernel"]
        V = eng.stored_variances(R).cpu().numpy()
        assert np.all(np.isfinite(V)) and np.all(V[:, :, :F] > 0)
        B1 = eng.B1
        if precision == "bf16" and c.Dy and shp["chain_kernel"] and shp["chain_tiles"] <= 17:
            # chain.hip, wchain_kernel at 8 wavefronts (and wchain4_kernel<17> like it) holds the per-frame layer-1 bias of
            # the labels as bf16; the decoding kernel takes it in fp32.  The same products need the same bias.
            eng.B1 = B1.to(torch.bfloat16).to(torch.float32)
        D = eng.decode(R).cpu().numpy()
        eng.B1 = B1
        rel = np.abs(V[:, :, :F] - D[:, :, :F]) / D[:, :, :F]
        Fm = shp["Fm"]
        e = (float(np.max(rel[:, :, :Fm])), float(np.max(rel[:, :, Fm:], initial=0.0)))
        print("%s: rows against decode %.2e, extra bin %.2e" % (tag, e[0], e[1]))
        assert e[0] < (2e-5 if precision == "bf16x3" else 4e-3) and e[1] < (2e-5 if precision == "bf16x3" else 5e-2), (tag, e)
        if R >= 2:      # the rows are told apart: neighbouring samples' variances differ by far more than those bounds
            assert float(np.max(np.abs(V[:, 1:, :F] - V[:, :-1, :F]) / V[:, 1:, :F])) > 0.1
        refs = [es.reference(o, variant) for o in es.oracles_from(c, eng, variant, Vb, V[:, :, :F])]
        out = eng.wiener_stored(want_masks=True)
        es.compare(tag + " wiener", refs, lambda u: es.device_wiener(c, eng, u, out), failures)
        es.padding_is_zero(eng, out[2], out[3], out[0].abs().sum(-1), out[1].abs().sum(-1))
        pre = [t.clone() for t in (eng.W, eng.Ht, eng.g)]
        for env, sc, w_fused in runs:
            with es.env(**env):
                for t, p in zip((eng.W, eng.Ht, eng.g), pre):
                    t.copy_(p)
                eng.m_step_stored()
                if variant != "noNMF":
                    assert es.query(eng, "Q_W_FUSED") == w_fused, (tag, env)
            cost = eng.cost_from_frames(R)
            name = sc["wstats"]["kernel"] if sc["wstats"] else "gains only"
            es.compare(tag + " m-step (%s)" % name, refs, lambda u: es.device_m_step(c, eng, u, cost, variant), failures)
            es.padding_is_zero(eng)
    eng.sample_store(False)
    assert not failures, failures


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("F,K,R,variant,Rcap", DECODE_CASES)
def test_decoding_kernels_against_the_oracle_from_the_decoded_variances(F, K, R, variant, Rcap, precision):
    """Given samples: eng.decode against decoder_forward at the mode's stated tolerance, then wiener and m_step (the
    gains-only one with a fixed noise PSD) against the float64 formulas fed with eng.decode's variances.  Every mode of
    decode_kernel decodes through the same routine (decode_tiles; the odd last bin through nyq_logit in every mode), so
    the variances of mode STORE are the ones modes WSTATS / HG / G / WF use."""
    need_gpu()
    c = es.case_inputs(F, K, R, variant)
    dc = decode_class(F, K, R, precision)
    eng, Vb = es.prepare(c, variant, precision, Rcap)
    assert eng.Fs == es.query(eng, "Q_FS") == (F + 15) // 16 * 16 and eng.Kp == es.query(eng, "Q_KP") == dc["KP"]
    eng.Zs.fill_(100.0)                                                    # (a sample read beyond the count would show)
    eng.Zs[:, :R].copy_(torch.from_numpy(c.Zs))
    tag = "decoding %s F=%d K=%d R=%d/%d %s" % (precision, F, K, R, Rcap, variant)
    V = eng.decode(R).cpu().numpy()
    assert np.all(np.isfinite(V)) and np.all(V[:, :, F:] == 0)
    oracles = es.oracles_from(c, eng, variant, Vb, V[:, :, :F])
    for u, o in enumerate(oracles):
        sl = eng.utt_slice(u)
        mine = o.Vs
        o.compute_Vs(c.Zs[sl])
        e = rel_err(mine, o.Vs)
        print("%s utt %d: decode %.2e" % (tag, u, e))
        assert e < (2e-4 if precision == "bf16x3" else 5e-2), (tag, u, e)
        o.Vs = mine
    refs = [es.reference(o, variant) for o in oracles]
    failures = []
    out = eng.wiener(R, want_masks=True)
    es.compare(tag + " wiener", refs, lambda u: es.device_wiener(c, eng, u, out), failures)
    es.padding_is_zero(eng, out[2], out[3], out[0].abs().sum(-1), out[1].abs().sum(-1))
    eng.m_step(R)
    cost = eng.cost_from_frames(R)
    es.compare(tag + " m-step", refs, lambda u: es.device_m_step(c, eng, u, cost, variant), failures)
    es.padding_is_zero(eng)
    assert not failures, failures
