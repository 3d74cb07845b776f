"""The assembled trainer (csrc/train.hip, vaenmf.train) where tests/test_gpu_train.py does not reach: unequal layer widths
that are no multiple of the tile, batches shorter than max_batch with evaluations between the steps, resuming from a saved
Adam state, vaenmf_train_gather on its own, reductions longer than four LDS stages, Adam's bias corrections at late steps,
and fit_m2's loop against the restatement.

Every rule and constant is that of tests/test_gpu_train.py (see its docstring): FACTOR = 8 times the float32 yardstick per
tensor and on the losses, C_CHAIN = 1.5e-7 of sum |a b| per element of a dense product, u = 2^-24.  Nothing here is a new
measured tolerance.  The cases (tests/train_cases.py: SHAPE_CASES, SCHED_CASES) are the smallest that cross every tile edge
of the 32 x 64 x 64 dense kernel; none is the workload's.

What the tests catch.  Each of these mistakes was made in csrc/train.hip, one at a time, and both modules run on the MI355X:
  hidden[i] taken as hidden[nh - 1 - i] in the encoder loop of vaenmf_trainer_create
      test_shapes_step_and_trajectory[m1_uneven, m2_uneven, m2_wide] and every other test at two unequal widths (the
      trainer's tensor shapes are no longer the model's); tests/test_gpu_train.py passes.
  ldx of layer i > 0 taken from net[i].out in forward_net
      test_shapes_step_and_trajectory (all five), test_ragged_schedule_with_evaluations, test_resume, ...; test_gpu_train's
      whole steps fail as well (the [mu | logvar] layer has 2 z = 64 outputs after 128 inputs), its building blocks pass.
  dW reduced over max_batch rows instead of the batch's in backward_net
      test_ragged_schedule_with_evaluations (all three), test_fit_m2_against_restatement,
      test_independent_of_max_batch_and_layout (through its trainer whose buffers an earlier batch of 200 rows filled: two
      fresh trainers on one schedule hold the same stale rows, and rows never written are zero, which a chain ignores);
      test_gpu_train.py passes.
  col0 dropped in train_gather_kernel
      test_gather, test_gather_rows_outside_and_refusals, the M2 cases of test_shapes_step_and_trajectory; also
      test_gpu_train's M2 steps.
  the `ok` test of train_gather_kernel removed, or a row outside skipped instead of written
      test_gather_rows_outside_and_refusals (the rows are NaN and not the arena's poison, on a NaN and on a 1e30 arena).
  the t->step key of the device draws replaced by a constant
      test_resume ("the draws do not depend on the step count"), test_fit_m2_against_restatement; also
      test_gpu_train's test_reproducible_and_device_draws (its replay of eps_fill).
  sqrt(1 - beta2^t) computed from t - 1
      test_adam_single_late_steps[1, 2, 1000] (at 10^5 both are 1) and every whole step; also test_gpu_train's test_adam.

MEASURED on the MI355X: each test's docstring has its largest ratio (error to float32 yardstick, where the rule allows
FACTOR = 8; error to bound, where it allows 1): whole steps at SHAPE_CASES <= 1.86, the ragged schedule <= 1.36, long
reductions <= 0.73, Adam at steps 1 .. 10^5 <= 0.72, the gather's normalisation <= 0.48, fit_m2's checkpoint 1.55."""
import numpy as np
import pytest
import torch

import train_cases as tc
from guarded import Arena, bits, same_bits
from helpers import nrm_err
import train_support as ts
from train_support import ACTS, DEV, FACTOR, U, gemm_forms_case
from vaenmf import _lib
from vaenmf import train as vt
from vaenmf._lib import check, lib

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def _hold_tensors(case, what, got, r64, r32):
    """test_step_and_trajectory's rule on the dicts `what` (grad1 or final) of three runs, per tensor (tc.groups): the GPU's
    nrm_err against float64 is at most FACTOR times the float32 restatement's.  Returns (largest ratio, failures)."""
    worst, fails = 0.0, []
    for label, keys in tc.groups(case):
        g, a64, a32 = (tc.cat(getattr(r, what), keys) for r in (got, r64, r32))
        eg, ey = nrm_err(g, a64), nrm_err(a32, a64)
        print("%s %s %s: gpu %.3g, float32 yardstick %.3g, ratio %.2f" % (case.name, what, label, eg, ey, eg / ey if ey else float("inf")))
        worst = max(worst, eg / ey if ey else float("inf"))
        if not eg <= FACTOR * ey:
            fails.append((what, label, eg, ey))
    return worst, fails


# ------------------------------------------------------------------------------------------------ 1. whole steps
@pytest.mark.parametrize("name", sorted(tc.SHAPE_CASES))
def test_shapes_step_and_trajectory(name):
    """test_step_and_trajectory at unequal widths: hidden (72, 40) and (256, 128), x_dim 67, y_dim 3 / 65 / 67, z_dim 4, 20
    and 128, batches of 33 and 17.  Per tensor (m1_one_z4: per layer, tc.groups) the step-1 gradient and the parameters
    after 20 steps, and the per-step losses, within FACTOR float32 yardsticks of the float64 restatement.
    MEASURED on the MI355X, largest ratio per case: step-1 gradients 0.67 .. 1.86 (m2_uneven), parameters after 20 steps
    1.00 .. 1.26 (m2_wide), losses 0.01 .. 0.44."""
    case = tc.SHAPE_CASES[name]
    init, data, r64, r32 = tc.reference_runs(case)
    tr, got = ts.gpu_run(case, init, data)
    wg, fg = _hold_tensors(case, "grad1", got, r64, r32)
    wf, ff = _hold_tensors(case, "final", got, r64, r32)
    ncol = 1 if case.kind == "Classifier" else 3
    eg, ey = _rel(got.losses[:, :ncol], r64.losses[:, :ncol]), _rel(r32.losses[:, :ncol], r64.losses[:, :ncol])
    print("%s: worst ratios grad1 %.2f, final %.2f, losses %.2f (gpu %.3g, float32 yardstick %.3g)" % (case.name, wg, wf, eg / ey, eg, ey))
    assert not fg + ff, fg + ff
    assert eg <= FACTOR * ey, (eg, ey)
    if case.kind == "Classifier":
        assert np.abs(got.counts - r64.counts).max() <= 1 and np.array_equal(got.counts.sum(1), np.full(tc.STEPS, case.B * case.y_dim))
    assert tr.step_count == tc.STEPS


# ------------------------------------------------------------------------------------------------ 2., 3. ragged batches
def _nan_padded(a, extra):
    """A host matrix [n][w] as a device tensor [n][w + extra] whose extra columns are NaN."""
    t = torch.full((a.shape[0], a.shape[1] + extra), float("nan"), dtype=torch.float32, device=DEV)
    t[:, :a.shape[1]] = torch.from_numpy(a)
    return t


def _put_padded(tr, X, Y):
    return tr.put(_nan_padded(X, 3), None if Y is None else _nan_padded(Y, 2))


def _state(tr):
    return tr.state_dict(), tr.gradients(), tr.adam_state()


def _same_state(a, b):
    return (all(same_bits(a[i][k], b[i][k]) for i in (0, 1) for k in a[i]) and a[2]["step"] == b[2]["step"] and
            all(same_bits(a[2][s][k], b[2][s][k]) for s in ("exp_avg", "exp_avg_sq") for k in a[2][s]))


def _sched_run(case, init, data, max_batch, evals=None, padded=False, used=False):
    """The scheduled case on one trainer of `max_batch` rows, eps replayed.  padded: the pool as NaN-padded device tensors
    and the indices as device tensors.  evals: evaluate between the steps on its pool (NaN-padded, through Trainer.put)
    and hold every evaluation to leaving the trainer's state alone.  used: the trainer first takes a step of max_batch
    rows and other draws, which fills every row of its buffers, and is then put back to `init`, zero Adam state and step 0.
    Returns (trainer, rows [steps][8], evaluation losses or None)."""
    model = tc.make_model(case)
    model.load_state_dict(init)
    tr = vt.Trainer(model, max_batch=max_batch, seed=0, device=DEV)
    if padded:
        tr.bind(_put_padded(tr, data["X"], data["Y"]))
    else:
        tr.bind(data["X"].T, None if data["Y"] is None else data["Y"].T)
    if case.kind == "Classifier":
        tr.set_norm(data["mean"], data["std"], tc.LOSS_EPS)
    if used:
        rng = np.random.default_rng(case.seed + 9000)
        eps = None if data["eps"] is None else rng.standard_normal((max_batch, case.z_dim)).astype(np.float32)
        tr.step(rng.integers(0, tc.POOL, max_batch).astype(np.int32), eps=eps)
        zeros = {k: torch.zeros(shp) for k, shp in zip(tr.keys, tr.shapes)}
        tr.load_state_dict(init)
        tr.load_adam_state({"step": 0, "exp_avg": zeros, "exp_avg_sq": zeros})
        assert tr.step_count == 0
    steps = len(case.B)
    rows = torch.zeros(steps, 8, dtype=torch.float64, device=DEV)
    ev, pool = None, None
    if evals is not None:
        ev, pool = np.zeros((len(evals["after"]), len(evals["batches"]), 3)), _put_padded(tr, evals["X"], evals["Y"])
    for s in range(steps):
        idx = torch.from_numpy(data["idx"][s]).to(DEV) if padded else data["idx"][s]
        tr.step(idx, eps=None if data["eps"] is None else data["eps"][s], out=rows[s])
        if ev is not None and s + 1 in evals["after"]:
            a = evals["after"].index(s + 1)
            before = _state(tr)
            for j, b in enumerate(evals["batches"]):
                r = vt.read_losses(tr.evaluate(b, eps=None if evals["eps"] is None else evals["eps"][a][j], data=pool))
                ev[a, j] = [r["loss"], r["recon"], r["kl"]]
            assert _same_state(before, _state(tr)), "the evaluation after step %d changed the trainer's state" % (s + 1)
    return tr, rows, ev


def _losses(rows):
    r = vt.read_losses(rows)
    return np.stack([r["loss"], r["recon"], r["kl"]], 1)


@pytest.mark.parametrize("name", sorted(tc.SCHED_CASES))
def test_ragged_schedule_with_evaluations(name):
    """Batches of 128, 80, 1, 17, 128, 33, 15, 128, 16, 2, twice, on one trainer of max_batch 128, with evaluations on a
    second pool of 50 rows (batches of 40 and 10) after steps 2, 5, 10, 13, 17 and 20: what _fit does to a trainer.  The
    final parameters per tensor by the rule of test_step_and_trajectory.  A single evaluation loss is one rounding event
    (its float32 error: 4e-9 .. 1.5e-7 relative), so the losses are one statistic: the largest relative error over the 20
    step losses and all evaluation losses together, GPU against float32 restatement, factor FACTOR.
    MEASURED on the MI355X: parameters 1.00 .. 1.36 (m2_uneven), pooled losses 0.06 .. 0.57."""
    case = tc.SCHED_CASES[name]
    init, data, evals, r64, r32 = tc.scheduled_runs(case)
    tr, rows, ev = _sched_run(case, init, data, 128, evals=evals, padded=False)
    got = tc.Run(_losses(rows), None, None, {k: v.numpy() for k, v in tr.state_dict().items()}, ev)
    wf, ff = _hold_tensors(case, "final", got, r64, r32)
    ncol = 1 if case.kind == "Classifier" else 3
    pool = lambda r: np.concatenate([r.losses[:, :ncol].ravel(), r.evals[:, :, :ncol].ravel()])
    eg, ey = _rel(pool(got), pool(r64)), _rel(pool(r32), pool(r64))
    print("%s: worst ratios final %.2f, pooled losses %.2f (gpu %.3g, float32 yardstick %.3g)" % (case.name, wf, eg / ey, eg, ey))
    assert not ff, ff
    assert eg <= FACTOR * ey, (eg, ey)
    assert tr.step_count == len(tc.SCHED) == 20


def test_independent_of_max_batch_and_layout():
    """The m2_uneven schedule on a trainer of max_batch 128, on one of 200, from NaN-padded device tensors with device
    indices (a batch of 128 out of 96 rows repeats some), and on a trainer of max_batch 200 whose buffers an earlier step of
    200 rows has filled to the last row: the same bits in every parameter, Adam tensor and loss row.  The last run is the one
    that tells a row past the batch from one inside it: two fresh trainers on one schedule hold the same stale rows."""
    case = tc.SCHED_CASES["m2_uneven"]
    init, data, _, _, _ = tc.scheduled_runs(case)
    assert len(set(data["idx"][0].tolist())) < len(data["idx"][0])
    runs = [_sched_run(case, init, data, 128), _sched_run(case, init, data, 200), _sched_run(case, init, data, 128, padded=True),
            _sched_run(case, init, data, 200, used=True)]
    (tr0, rows0, _), s0 = runs[0], _state(runs[0][0])
    assert torch.isfinite(rows0[:, :3]).all()
    for what, (tr, rows, _) in zip(("max_batch 200", "padded device tensors", "a used trainer of max_batch 200"), runs[1:]):
        s = _state(tr)
        assert s[2]["step"] == s0[2]["step"] == len(tc.SCHED)
        assert all(same_bits(s0[0][k], s[0][k]) for k in s0[0]), "parameters differ with %s" % what
        assert all(same_bits(s0[2][m][k], s[2][m][k]) for m in ("exp_avg", "exp_avg_sq") for k in s0[2][m]), "Adam state differs with %s" % what
        assert same_bits(rows0, rows), "loss rows differ with %s" % what


# ------------------------------------------------------------------------------------------------ 4. resume
def test_resume():
    """20 steps with device draws (seed 7) against 9 steps, parameters and adam_state() read, a fresh trainer loaded with
    them (load_adam_state sets the step count), 11 more steps: the same bits.  The draws are keyed by the step number: the
    same resume with the step count left at 0 computes the loss of its first step from the same parameters and rows, so that
    loss differs only through the draws -- and must."""
    case = tc.SHAPE_CASES["m2_uneven"]
    init, data, _, _ = tc.reference_runs(case)

    def trainer(state=None):
        model = tc.make_model(case)
        model.load_state_dict(init)
        tr = vt.Trainer(model, max_batch=case.B, seed=7, device=DEV)
        tr.bind(data["X"].T, data["Y"].T)
        if state is not None:
            tr.load_state_dict(state[0])
            tr.load_adam_state(state[1])
        return tr

    def steps(tr, lo, hi):
        rows = torch.zeros(hi - lo, 8, dtype=torch.float64, device=DEV)
        for s in range(lo, hi):
            tr.step(data["idx"][s], out=rows[s - lo])
        return rows

    straight = trainer()
    rows_a = steps(straight, 0, tc.STEPS)
    first = trainer()
    steps(first, 0, 9)
    saved = (first.state_dict(), first.adam_state())
    assert saved[1]["step"] == 9
    resumed = trainer(saved)
    assert resumed.step_count == 9 and all(same_bits(saved[0][k], v) for k, v in resumed.state_dict().items())
    loaded = resumed.adam_state()
    assert all(same_bits(saved[1][m][k], loaded[m][k]) for m in ("exp_avg", "exp_avg_sq") for k in saved[1][m])
    rows_b = steps(resumed, 9, tc.STEPS)
    a, b = _state(straight), _state(resumed)
    assert a[2]["step"] == b[2]["step"] == tc.STEPS
    assert all(same_bits(a[0][k], b[0][k]) for k in a[0]), "parameters differ after the resume"
    assert all(same_bits(a[2][m][k], b[2][m][k]) for m in ("exp_avg", "exp_avg_sq") for k in a[2][m]), "Adam state differs after the resume"
    assert same_bits(rows_a[9:], rows_b), "the losses of steps 10 .. 20 differ after the resume"
    # the step count left at 0: step 10's loss comes from the same parameters and rows and from the draws of step 1
    stale = trainer((saved[0], dict(saved[1], step=0)))
    rows_c = steps(stale, 9, 10)
    assert stale.step_count == 1
    assert rows_c[0, 0].item() != rows_a[9, 0].item() and rows_c[0, 1].item() != rows_a[9, 1].item(), "the draws do not depend on the step count"
    # what the C ABI refuses
    h = resumed._h
    for bad in (-1, 2 ** 31 - 1):
        assert lib().vaenmf_trainer_set_step_count(h, bad) == -1 and b"outside" in lib().vaenmf_last_error()
    assert resumed.step_count == tc.STEPS
    t = torch.zeros(72 * 70, device=DEV)
    n = lib().vaenmf_trainer_num_tensors(h)
    assert n == len(resumed.keys) == 14
    for which, i, word in ((-1, 0, b"which=-1"), (4, 0, b"which=4"), (_lib.TRAIN_ADAM_M, n, b"tensor 14 of 14"), (_lib.TRAIN_ADAM_V, -1, b"tensor -1 of 14")):
        assert lib().vaenmf_trainer_set_tensor(h, which, i, ts.p(t), ts.st()) == -1 and word in lib().vaenmf_last_error(), (which, i)
    assert _same_state(b, _state(resumed))


# ------------------------------------------------------------------------------------------------ 5. gather
GATHER_NCOL = (1, 255, 256, 257, 513)


@pytest.mark.parametrize("B", (1, 33))
def test_gather(B):
    """vaenmf_train_gather on exact-size buffers: rows lds = ncol + 3 apart with NaN between, dst ldd = col0 + ncol + 2 wide
    and poison all over.  Without mean / std the columns [col0, col0 + ncol) of dst are src[idx] bit for bit and the rest of
    dst is still poison; with them (v - mean) / (std + eps) within 4 u |ref| of float64: three correctly rounded operations
    (u each) and eps = 1e-8 as a float, 6e-9 of itself off, beside a std of order 1."""
    rng = np.random.default_rng(80 + B)
    NT, eps = 40, 1e-8
    worst = 0.0
    for ncol in GATHER_NCOL:
        for col0 in (0, 5):
            lds, ldd = ncol + 3, col0 + ncol + 2
            src = (rng.exponential(1.0, (NT, ncol)) * np.exp(rng.normal(0.0, 2.0, (NT, ncol)))).astype(np.float32)
            src[rng.random((NT, ncol)) < 0.05] = 0.0
            idx = rng.integers(0, NT, B).astype(np.int32)
            idx[0] = NT - 1                                              # the last row, the first, and a row twice
            if B > 3:
                idx[1], idx[2], idx[3] = 0, idx[B - 1], NT - 1
            mean = src.mean(0).astype(np.float32)
            std = (src.std(0, ddof=1) + 0.1).astype(np.float32)
            for norm in (False, True):
                what = "B=%d ncol=%d col0=%d norm=%s" % (B, ncol, col0, norm)
                arena = Arena(4 << 20, "nan", device=DEV)
                src_, idx_ = ts.put(arena, "src", src, lds), ts.put(arena, "idx", idx)
                mean_, std_ = ts.put(arena, "mean", mean), ts.put(arena, "std", std)
                dst_ = ts.out(arena, "dst", B, ldd, ldd)
                arena.snapshot(["src", "idx", "mean", "std"])
                check(lib().vaenmf_train_gather(ts.p(src_), lds, NT, ts.p(idx_), B, ncol, ts.p(mean_) if norm else None, ts.p(std_) if norm else None,
                                                eps if norm else 0.0, ts.p(dst_), ldd, col0, ts.st()))
                torch.cuda.synchronize()
                arena.check(what)
                arena.unchanged(what=what)
                assert (col0 == 0 or arena.is_poison(dst_[:, :col0])) and arena.is_poison(dst_[:, col0 + ncol:]), what
                got = dst_[:, col0:col0 + ncol].cpu().numpy()
                if not norm:
                    assert np.array_equal(got.view(np.int32), src[idx].view(np.int32)), what
                else:
                    ref = (src[idx].astype(np.float64) - mean) / (std.astype(np.float64) + eps)
                    err = np.abs(got - ref)
                    assert np.all(err <= 4 * U * np.abs(ref)), (what, float((err / np.maximum(4 * U * np.abs(ref), 1e-300)).max()))
                    worst = max(worst, float((err / np.maximum(4 * U * np.abs(ref), 1e-300)).max()))
    print("gather B=%d: worst normalisation error / bound %.3g" % (B, worst))


def test_gather_rows_outside_and_refusals():
    """An index of -1 and one of NT: NaN rows (include/vaenmf.h: a row outside is not read), their neighbours right, the
    padding of dst and the guard bands intact.  The NaN has to be one the kernel WROTE: a kernel that skips such a row
    leaves dst's poison there, and one that reads src[-1] or src[NT] finds the guard band's poison (64 KiB of it, so
    nothing faults) and copies or normalises it.  So the rows must not hold the arena's poison word, and the case runs
    on an arena poisoned with NaN and on one poisoned with 1e30, where either mistake leaves a finite number."""
    rng = np.random.default_rng(90)
    NT, ncol, col0 = 12, 257, 5
    lds, ldd = ncol + 3, col0 + ncol + 2
    src = rng.exponential(1.0, (NT, ncol)).astype(np.float32)
    idx = np.array([3, -1, NT - 1, NT, 0], np.int32)
    mean, std = src.mean(0).astype(np.float32), (src.std(0, ddof=1) + 0.1).astype(np.float32)
    inside = idx[[0, 2, 4]]
    for poison, norm in ((p, n) for p in ("nan", "1e30") for n in (False, True)):
        arena = Arena(2 << 20, poison, device=DEV)
        src_, idx_, mean_, std_ = ts.put(arena, "src", src, lds), ts.put(arena, "idx", idx), ts.put(arena, "mean", mean), ts.put(arena, "std", std)
        dst_ = ts.out(arena, "dst", len(idx), ldd, ldd)
        arena.snapshot(["src", "idx", "mean", "std"])
        check(lib().vaenmf_train_gather(ts.p(src_), lds, NT, ts.p(idx_), len(idx), ncol, ts.p(mean_) if norm else None, ts.p(std_) if norm else None,
                                        1e-8 if norm else 0.0, ts.p(dst_), ldd, col0, ts.st()))
        torch.cuda.synchronize()
        arena.check("rows outside")
        arena.unchanged(what="rows outside")
        assert arena.is_poison(dst_[:, :col0]) and arena.is_poison(dst_[:, col0 + ncol:])
        got = dst_[:, col0:col0 + ncol].cpu().numpy()
        assert np.isnan(got[[1, 3]]).all(), (poison, norm)
        assert not (bits(dst_[[1, 3], col0:col0 + ncol]) == arena.word).any(), (poison, norm, "the NaN is the arena's poison")
        if not norm:
            assert np.array_equal(got[[0, 2, 4]].view(np.int32), src[inside].view(np.int32))
        else:
            ref = (src[inside].astype(np.float64) - mean) / (std.astype(np.float64) + 1e-8)
            assert np.all(np.abs(got[[0, 2, 4]] - ref) <= 4 * U * np.abs(ref))
    t, i = torch.zeros(64, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    g = lib().vaenmf_train_gather
    assert g(ts.p(t), 3, 4, ts.p(i), 2, 4, None, None, 0.0, ts.p(t), 8, 0, ts.st()) == -1 and b"lds=3 < ncol=4" in lib().vaenmf_last_error()
    assert g(ts.p(t), 4, 4, ts.p(i), 2, 4, None, None, 0.0, ts.p(t), 8, 5, ts.st()) == -1 and b"[5, 9) outside ldd=8" in lib().vaenmf_last_error()
    assert g(ts.p(t), 4, 4, ts.p(i), 2, 4, ts.p(t), None, 0.0, ts.p(t), 8, 0, ts.st()) == -1 and b"go together" in lib().vaenmf_last_error()
    assert g(ts.p(t), 4, 0, ts.p(i), 2, 4, None, None, 0.0, ts.p(t), 8, 0, ts.st()) == -1 and b"NT=0" in lib().vaenmf_last_error()
    torch.cuda.synchronize()
    assert not t.any()


# ------------------------------------------------------------------------------------------------ 6. long reductions
LONG_SHAPES = ((33, 513, 40), (33, 40, 513), (17, 1024, 33), (513, 17, 66), (257, 65, 1))


def test_gemm_long_reductions():
    """test_gemm_forms' checks, with its bounds from the operands, where the reduction is longer than its sweep's 256:
    K = 513 (eight LDS stages and a tail of one: the workload's x_dim) forward and in dX, K = 1024 (C_CHAIN's stated range),
    and dW / db over batches of 257 and 513 rows.  One activation each, all five.
    MEASURED on the MI355X, largest error / bound: forward 0.44, dX 0.45, dW 0.73 (17 rows of 1024 columns), db 0.34
    (the sweep at K <= 256: forward 0.76, dX 0.56, dW 0.81, db 0.59)."""
    rng = np.random.default_rng(771)
    worst = {"fwd": 0.0, "dx": 0.0, "dw": 0.0, "db": 0.0}
    for j, ((M, n_in, n_out), act) in enumerate(zip(LONG_SHAPES, ACTS)):
        gemm_forms_case(rng, M, n_in, n_out, act, j, worst)
        print("M=%d in=%d out=%d act=%s: worst error / bound so far %s" % (M, n_in, n_out, act, worst))
    print("long reductions: worst error / bound %s; at K <= 256 (test_gemm_forms): fwd 0.76, dx 0.56, dw 0.81, db 0.59" % worst)


# ------------------------------------------------------------------------------------------------ 7. Adam at late steps
@pytest.mark.parametrize("step", (1, 2, 1000, 100000))
def test_adam_single_late_steps(step):
    """ONE vaenmf_adam call at step t against torch.optim.Adam on the CPU in float32 from the same p, g, m, v (its
    state["step"] set to t - 1), held to test_adam's per-step bound 64 u lr + 2 u |p|.

    test_adam derives: the update lr m^ / (sqrt(v^) + eps) goes through about seven float operations (8 u of itself), and m's
    absolute error after t steps is at most 4 u t max|g| against sqrt(v^) + eps >= max|g| / sqrt(t): lr (4 t^1.5 + 8) u.  The
    t^1.5 term is ACCUMULATED m error.  Here both sides start the step from the same m and v, so only one step's rounding
    is there, at any t.  With b1(t) = 1 - beta1^t, b2(t) = 1 - beta2^t and a state as t - 1 steps of gradients |g| <= G leave
    it -- |m| <= b1(t-1) G, v = b2(t-1) c G^2 with c in [1/2, 1] (both zero at t = 1) --
      m' = m + w (g - m), w = 0.1, is off by at most u (3 w |g - m| + |m'|) <= u G (0.6 + b1(t)) (t = 1: w g, 2 u of itself),
        so m^ = m' / b1(t) by u G (0.6 / b1(t) + 1): 4.2 u G at t = 2, 1.6 u G for large t;
      v^ is the mean of c G^2 and g^2 with weights beta2 b2(t-1) / b2(t) >= 0.4997 (t >= 2) and the rest, so
        D = sqrt(v^) + eps >= G / 2 and |m^| / D <= 2 (t = 1: v^ = g^2, |m^| / D <= 1); D's own error, 5 u of itself, is
        among the seven operations;
      the update is therefore off by at most lr (4.2 / 0.5 + 8 * 2) u < 25 u lr in either implementation, 50 u lr between
      the two, under the 64 u lr of the bound; p + update then rounds differently by at most an ulp, 2 u |p|.
    Where 1 - beta1^t is 1 in float and in double (t >= 1000: 0.9^1000 = 1.7e-46) the step size is lr exactly and only
    sqrt(1 - beta2^t) is left: 0.795 at t = 1000, 1 - 1.8e-44 at 10^5.  Elements with g = 0, m = 0, v = 0 keep their bits.
    MEASURED on the MI355X, largest error / bound: 0.06 (t = 1), 0.72 (2), 0.42 (1000), 0.18 (100000); the larger
    figures are one ulp of a p of order 1 (3e-8 at 0.31) where the two updates round p + update apart, the 2 u |p| of
    the bound, not the update itself."""
    rng = np.random.default_rng(900 + step % 97)
    n, lr, b1, b2 = 4096 + 37, 1e-3, 0.9, 0.999
    zero, tiny = slice(0, 500), slice(500, 1500)
    G = np.exp(rng.normal(0, 2, n))
    G[tiny] = 1e-8                                                    # g / (|g| + eps) is steep here
    bc1p, bc2p = 1 - b1 ** (step - 1), 1 - b2 ** (step - 1)
    p0 = rng.standard_normal(n).astype(np.float32)
    g = (G * rng.uniform(-1, 1, n)).astype(np.float32)
    m0 = (bc1p * G * rng.uniform(-1, 1, n)).astype(np.float32)
    v0 = (bc2p * G * G * rng.uniform(0.5, 1.0, n)).astype(np.float32)
    g[zero], m0[zero], v0[zero] = 0.0, 0.0, 0.0
    assert (v0 >= 0).all() and (step == 1) == (not v0.any())
    pt = torch.tensor(p0.copy(), requires_grad=True)
    opt = torch.optim.Adam([pt], lr=lr, betas=(b1, b2), eps=1e-8)
    opt.state[pt] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.tensor(m0.copy()), "exp_avg_sq": torch.tensor(v0.copy())}
    pt.grad = torch.tensor(g.copy())
    opt.step()
    assert opt.state[pt]["step"].item() == step
    arena = Arena(4 << 20, "nan", device=DEV)
    p_, g_, m_, v_ = ts.put(arena, "p", p0), ts.put(arena, "g", g), ts.put(arena, "m", m0), ts.put(arena, "v", v0)
    arena.snapshot(["g"])
    check(lib().vaenmf_adam(ts.p(p_), ts.p(g_), ts.p(m_), ts.p(v_), n, step, lr, b1, b2, 1e-8, ts.st()))
    torch.cuda.synchronize()
    arena.check("adam step %d" % step)
    arena.unchanged(what="adam")
    got, ref = p_.cpu().numpy(), pt.detach().numpy()
    assert np.array_equal(got[zero].view(np.int32), p0[zero].view(np.int32)), "a zero gradient with zero m moved its parameter"
    assert np.array_equal(ref[zero], p0[zero])
    tol = 64 * U * lr + 2 * U * np.abs(ref)
    err = np.abs(got.astype(np.float64) - ref)
    print("adam step %d: worst error / bound %.3g (tiny gradients %.3g), movement %.3g" % (step, (err / tol).max(), (err[tiny] / tol[tiny]).max(), np.abs(ref - p0).max()))
    assert np.all(err <= tol), float((err / tol).max())
    assert np.abs(ref[1500:] - p0[1500:]).mean() > 1e-4 and np.abs(ref[tiny] - p0[tiny]).max() > 1e-5          # both kinds moved
    st = opt.state[pt]
    assert np.all(np.abs(m_.cpu().numpy() - st["exp_avg"].numpy()) <= 4 * U * G)
    # v' = beta2 v + ((1 - beta2) g) g: four roundings of positive terms in either implementation
    assert np.all(np.abs(v_.cpu().numpy() - st["exp_avg_sq"].numpy()) <= 8 * U * st["exp_avg_sq"].numpy())


# ------------------------------------------------------------------------------------------------ 8. the fit loop
def test_fit_m2_against_restatement(tmp_path):
    """fit_m2 for one epoch on 300 frames of m2_uneven's shape in batches of 128, 128 and 44, 70 validation frames.  The
    restatement replays the loop's permutation (np.random.default_rng(seed).permutation) and takes its draws from
    Trainer.eps_fill(step, B).  The epoch's train means of loss, recon and KL and the saved checkpoint are held to the rules
    of test_shapes_step_and_trajectory.  The validation means are NOT compared: an evaluation draws under the key
    (step + 1) | 2^31, and eps_fill / vaenmf_train_eps_fill take step numbers below 2^31 only, so the public interface
    cannot reproduce those draws; they are held to being finite and to the logged checkpoint name.
    MEASURED on the MI355X: checkpoint 1.55 yardsticks (three steps: yardsticks of 4e-8 .. 2e-7), train means 0.19."""
    base = tc.SHAPE_CASES["m2_uneven"]
    seed, n, nv, bs = 5, 300, 70, 128
    bounds = vt.batch_bounds(n, bs)
    case = base._replace(name="m2_uneven_fit", B=tuple(hi - lo for lo, hi in bounds), seed=base.seed + 200)
    assert case.B == (128, 128, 44)
    rng = np.random.default_rng(case.seed)
    X, Y = tc.make_pool(rng, case, n)
    Xv, Yv = tc.make_pool(rng, case, nv)
    model = tc.make_model(case)
    init = tc.state_of(model)
    tr, hist = vt.fit_m2(model, (X.T, Y.T), (Xv.T, Yv.T), str(tmp_path), epochs=1, batch_size=bs, seed=seed, device=DEV)
    assert tr.step_count == 3 and len(hist) == 1
    perm = np.random.default_rng(seed).permutation(n).astype(np.int32)
    data = {"X": X, "Y": Y, "mean": None, "std": None, "idx": [perm[lo:hi] for lo, hi in bounds],
            "eps": [tr.eps_fill(s + 1, hi - lo).cpu().numpy() for s, (lo, hi) in enumerate(bounds)]}
    r64, r32 = tc.run_steps(case, init, data, torch.float64, 3), tc.run_steps(case, init, data, torch.float32, 3)
    sd = torch.load(hist[0]["checkpoint"], map_location="cpu")
    assert list(sd) == tr.keys
    got = tc.Run(None, None, None, {k: v.numpy() for k, v in sd.items()})
    wf, ff = _hold_tensors(case, "final", got, r64, r32)
    means = lambda r: r.losses.mean(0)
    gm = np.array([hist[0]["train"][k] for k in ("loss", "recon", "kl")])
    eg, ey = _rel(gm, means(r64)), _rel(means(r32), means(r64))
    print("%s: worst ratios checkpoint %.2f, train means %.2f (gpu %.3g, float32 yardstick %.3g)" % (case.name, wf, eg / ey, eg, ey))
    assert not ff, ff
    assert eg <= FACTOR * ey, (eg, ey)
    va = hist[0]["valid"]
    assert all(np.isfinite(va[k]) for k in ("loss", "recon", "kl")) and abs(va["loss"] - (va["recon"] + va["kl"])) <= 1e-9 * abs(va["loss"])
    assert hist[0]["checkpoint"].endswith(vt.checkpoint_name("M2", 1, va["loss"]))
