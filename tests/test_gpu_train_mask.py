"""The mask trainer on the GPU (csrc/train_mask.hip, vaenmf.train_mask): the MSE head alone against float64, whole steps
and 20-step runs against the float64 restatement of tests/mask_train_cases.py, the steps recorded from the reference, the
trainer's state, its entry points on a side stream, and fit_mask_filter through the public interface into MaskEnhancer.

Buffers of the kernel-level tests come from guarded.Arena: exact sizes, NaN in every column between a row's width and its
leading dimension, guard bands checked after every call.

Bounds.
  u = 2^-24.  The head evaluates every term in double from float inputs and rounds a gradient to float once: a gradient is
  held to 2 u |g| (one rounding, and room for a double exponential a few double ulps from numpy's) plus 1e-12 of the terms
  before their cancellation (y against yh, y against yh x); a row sum to 1e-12 of the sum of those terms squared.
  Whole steps: per tensor group, nrm_err against the float64 restatement may be at most FACTOR = 8 times the same error of
  torch's CPU float32 run of the restatement on the same case (tests/test_gpu_train.py states why 8); the per-step losses by
  the same rule on their largest relative error.  The recorded run of the reference is within 4 yardsticks of float64
  (tests/test_train_mask_cpu.py), so the GPU is within 8 + 4 of it.
  Everything else is bit equality: the header promises the same bits for the same inputs."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import mask_train_cases as mc
import vaenmf
from guarded import Arena, same_bits
from helpers import nrm_err
from vaenmf import train as vt
from vaenmf import train_mask as vm
from vaenmf._lib import check

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DEV = "cuda:0"
HEAD_B, HEAD_D = (1, 3, 17, 128), (1, 5, 65, 513)


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def put(arena, name, host, ld):
    """A host matrix as an arena buffer with rows `ld` apart: the columns past its width stay poison."""
    t = arena.carve(name, (host.shape[0], ld), torch.float32)
    t[:, :host.shape[1]].copy_(torch.from_numpy(np.ascontiguousarray(host)))
    return t


# ---------------------------------------------------------------------------------------------------------------- 1. head
def head_inputs(rng, B, D):
    """a with saturated outputs (|a| = 40) among it, labels in [0, 1] with exact 0 and 1, power with exact zeros."""
    a = (rng.standard_normal((B, D)) * 4).astype(np.float32)
    y = rng.random((B, D)).astype(np.float32)
    P = (rng.exponential(1.0, (B, D)) * np.exp(rng.normal(0, 1.5, (B, D)))).astype(np.float32)
    sat = rng.random((B, D)) < 0.1
    a[sat] = np.where(rng.random(int(sat.sum())) < 0.5, 40.0, -40.0).astype(np.float32)
    y[rng.random((B, D)) < 0.1] = 1.0
    y[rng.random((B, D)) < 0.1] = 0.0
    P[rng.random((B, D)) < 0.1] = 0.0
    a[0, 0], y[0, 0] = 40.0, 0.0                      # a saturated output that is wrong: the gradient is still 0 in float terms
    P[-1, -1] = 0.0
    return a, y, P


def head_float64(loss, a, y, P, B):
    """(row sums, dA, bound on the row sums, bound on dA) in float64 from the float inputs."""
    a, y, x = a.astype(np.float64), y.astype(np.float64), np.sqrt(P.astype(np.float64))
    e = np.exp(-np.abs(a))
    big, small = 1 / (1 + e), e / (1 + e)
    yh, q = np.where(a >= 0, big, small), np.where(a >= 0, small, big)           # sigmoid(a) and 1 - sigmoid(a) without cancellation
    if loss == "mask":
        r, w, mag = y - yh, np.ones_like(a), np.abs(y) + yh
    elif loss == "signal":
        r, w, mag = (y - yh) * x, x, (np.abs(y) + yh) * x
    else:
        r, w, mag = y - yh * x, x, np.abs(y) + yh * x
    g = -2 * r * w * yh * q / B
    return (r * r).sum(1), g, 1e-12 * (mag * mag).sum(1) + 1e-300, 2 * U * np.abs(g) + 1e-12 * 2 * mag * w * yh * q / B + 1e-45


@pytest.mark.parametrize("B", HEAD_B)
@pytest.mark.parametrize("loss", mc.LOSS_NAMES)
def test_mse_head(loss, B):
    L = vm.lib()
    code = vm.LOSSES[loss]
    for D in HEAD_D:
        rng = np.random.default_rng(1000 * code + 10 * B + D)
        a, y, P = head_inputs(rng, B, D)
        lda, ldy, ldp, ldd = D + 3, D + 1, D + 2, D + 5
        arena = Arena(4 << 20, "nan", device=DEV)
        a_, y_, P_ = put(arena, "a", a, lda), put(arena, "y", y, ldy), put(arena, "P", P, ldp)
        dA_ = arena.carve("dA", (B, ldd), torch.float32)
        rl_, rl2_, out_ = arena.carve("rl", (B,), torch.float64), arena.carve("rl2", (B,), torch.float64), arena.carve("out", (8,), torch.float64)
        dA2_, rl3_ = arena.carve("dA2", (B, ldd), torch.float32), arena.carve("rl3", (B,), torch.float64)
        arena.snapshot(["a", "y", "P"])
        what = "%s B=%d D=%d" % (loss, B, D)
        check(L.vaenmf_mse_head(p(a_), lda, p(y_), ldy, p(P_), ldp, B, D, code, p(dA_), ldd, p(rl_), st()))
        check(L.vaenmf_loss_reduce(p(rl_), None, None, B, p(out_), st()))
        check(L.vaenmf_mse_head(p(a_), lda, p(y_), ldy, p(P_), ldp, B, D, code, None, 0, p(rl2_), st()))          # evaluation: dA = NULL
        check(L.vaenmf_mse_head(p(a_), lda, p(y_), ldy, p(P_), ldp, B, D, code, p(dA2_), ldd, p(rl3_), st()))     # a second run
        torch.cuda.synchronize()
        arena.check(what)
        arena.unchanged(what=what)
        assert arena.is_poison(dA_[:, D:]) and arena.is_poison(dA2_[:, D:]), (what, "the padding of dA was written")
        rows, g, tol_rows, tol_g = head_float64(loss, a, y, P, B)
        got_rows, got_g = rl_.cpu().numpy(), dA_[:, :D].cpu().numpy().astype(np.float64)
        assert np.isfinite(got_rows).all() and np.isfinite(got_g).all(), what
        er, eg = np.abs(got_rows - rows) / tol_rows, np.abs(got_g - g) / tol_g
        print("%s: worst error / bound: rows %.3g, dA %.3g" % (what, er.max(), eg.max()))
        assert er.max() <= 1.0 and eg.max() <= 1.0, (what, er.max(), eg.max())
        assert np.all(np.abs(got_g[np.abs(a) == 40.0]) <= 1e-15 * (1 + np.sqrt(P[np.abs(a) == 40.0].astype(np.float64))) ** 2), (what, "a saturated output has a gradient")
        if loss != "mask":
            assert np.all(got_g[P == 0.0] == 0.0), what
        assert same_bits(rl2_, rl_) and same_bits(rl3_, rl_) and same_bits(dA2_[:, :D], dA_[:, :D]), what
        o = out_.cpu()
        assert abs(o[0].item() - rows.mean()) <= tol_rows.mean() + 1e-12 * rows.mean() and o[1].item() == o[0].item() and o[2].item() == 0.0
        assert np.array_equal(o[4:].view(torch.int64).numpy(), np.zeros(4, np.int64))
        if loss == "mask":                             # the power rows are not read: NULL is taken
            rl4 = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)
            check(L.vaenmf_mse_head(p(a_), lda, p(y_), ldy, None, 0, B, D, code, None, 0, p(rl4), st()))
            assert same_bits(rl4, rl_)
        # against torch's own float64 autograd of the reference's formula, where its 1 - sigmoid cancellation allows
        at = torch.tensor(a.astype(np.float64), requires_grad=True)
        l = mc.mse_loss(loss, torch.sigmoid(at), torch.tensor(y.astype(np.float64)), torch.tensor(P.astype(np.float64)))
        l.backward()
        assert abs(l.item() - rows.mean()) <= 1e-9 * abs(rows.mean()) + 1e-300
        # (torch's yh (1 - yh) is an exact 0 at |a| = 40, where the head's is 4e-18)
        assert np.all(np.abs(at.grad.numpy() - g) <= 1e-9 * np.abs(g).max() + 1e-15 * (1 + np.sqrt(P.astype(np.float64))) ** 2), what


def test_mse_head_refuses_bad_arguments():
    L = vm.lib()
    t = torch.zeros(64, device=DEV)
    r = torch.zeros(8, dtype=torch.float64, device=DEV)
    assert L.vaenmf_mse_head(p(t), 4, p(t), 4, p(t), 4, 0, 4, 0, None, 0, p(r), st()) == -1
    assert L.vaenmf_mse_head(p(t), 3, p(t), 4, p(t), 4, 2, 4, 0, None, 0, p(r), st()) == -1               # lda < D
    assert L.vaenmf_mse_head(p(t), 4, p(t), 4, p(t), 4, 2, 4, 3, None, 0, p(r), st()) == -1 and b"loss" in L.vaenmf_last_error()
    assert L.vaenmf_mse_head(p(t), 4, p(t), 4, None, 0, 2, 4, 1, None, 0, p(r), st()) == -1 and b"power" in L.vaenmf_last_error()
    assert L.vaenmf_mse_head(p(t), 4, p(t), 4, p(t), 4, 2, 4, 2, p(t), 3, p(r), st()) == -1               # ldd < D


# ---------------------------------------------------------------------------------------------------------------- 2. steps
Got = mc.Run


def make_trainer(case, init, data, max_batch=32):
    model = mc.make_model(case)
    model.load_state_dict(init)
    tr = vm.MaskTrainer(model, loss=case.loss, max_batch=max_batch, device=DEV)
    tr.bind(data["X"].T, data["Y"].T)
    if data["mean"] is not None:
        tr.set_norm(data["mean"], data["std"], mc.NORM_EPS)
    return tr


def gpu_run(case, init, data, tr=None):
    tr = tr or make_trainer(case, init, data)
    steps = len(data["idx"])
    rows = torch.zeros(steps, 8, dtype=torch.float64, device=DEV)
    grad1 = None
    for s in range(steps):
        tr.step(data["idx"][s], out=rows[s])
        if s == 0:
            grad1 = {k: v.numpy() for k, v in tr.gradients().items()}
    r = vt.read_losses(rows)
    assert np.array_equal(r["recon"], r["loss"]) and not r["kl"].any() and not any(r[k].any() for k in ("tp", "tn", "fp", "fn"))
    return tr, Got(r["loss"], grad1, {k: v.numpy() for k, v in tr.state_dict().items()})


def hold(case, got, r64, r32, factor=mc.FACTOR):
    """Every tensor group of the step-1 gradient and of the final parameters, and the losses, within `factor` yardsticks."""
    fails, worst = [], {"grad1": 0.0, "final": 0.0}
    for label, keys in mc.groups(case):
        for what, g, a64, a32 in (("grad1", got.grad1, r64.grad1, r32.grad1), ("final", got.final, r64.final, r32.final)):
            eg, ey = nrm_err(mc.cat(g, keys), mc.cat(a64, keys)), nrm_err(mc.cat(a32, keys), mc.cat(a64, keys))
            print("%s %s %s: gpu %.3g, float32 yardstick %.3g, ratio %.2f" % (case.name, what, label, eg, ey, eg / ey if ey else float("inf")))
            worst[what] = max(worst[what], eg / ey if ey else float("inf"))
            if not eg <= factor * ey:
                fails.append((what, label, eg, ey))
    eg, ey = mc.loss_err(got.losses, r64.losses), mc.loss_err(r32.losses, r64.losses)
    print("%s losses: gpu %.3g, float32 yardstick %.3g; worst ratios %s" % (case.name, eg, ey, worst))
    assert not fails, fails
    assert eg <= factor * ey, (eg, ey)
    return ey


@pytest.mark.parametrize("case", mc.CASES, ids=[c.name for c in mc.CASES])
def test_step_and_trajectory(case):
    """Gradients after step 1, parameters after 20 steps (19 batches of 32 and one of 17), per-step losses.
    MEASURED on the MI355X, largest ratio to the yardstick over the tensor groups of a case: step-1 gradients 0.57 .. 1.35,
    parameters after 20 steps 1.00 .. 1.38, losses 0.01 .. 0.06 (1.14 without the normalisation)."""
    init, data, r64, r32 = mc.reference_runs(case)
    tr, got = gpu_run(case, init, data)
    hold(case, got, r64, r32)
    assert tr.step_count == mc.STEPS
    assert tr.keys == list(init.keys()) and tr.shapes == [tuple(v.shape) for v in init.values()]


# ---------------------------------------------------------------------------------------------------------------- 3. golden
@pytest.mark.parametrize("loss", mc.LOSS_NAMES)
def test_golden_run(loss):
    """The recorded batches from the recorded state: within FACTOR yardsticks of float64 and FACTOR + 4 of the recorded run."""
    g, r64, r32 = mc.golden_runs(loss)
    case = mc.GOLDEN_CASE._replace(loss=loss, name="golden_" + loss)
    tr, got = gpu_run(case, g["init"], g["data"][loss], make_trainer(case, g["init"], g["data"][loss], max_batch=mc.GOLDEN_B))
    ey = hold(case, got, r64, r32)
    assert mc.loss_err(got.losses, g["losses"][loss]) <= (mc.FACTOR + mc.GOLDEN_FACTOR) * ey
    for label, keys in mc.groups(case):
        ey = nrm_err(mc.cat(r32.final, keys), mc.cat(r64.final, keys))
        assert nrm_err(mc.cat(got.final, keys), mc.cat(g["final"][loss], keys)) <= (mc.FACTOR + mc.GOLDEN_FACTOR) * ey, label


# ---------------------------------------------------------------------------------------------------------------- 4. state
def _same(a, b):
    return list(a) == list(b) and all(same_bits(a[k], b[k]) for k in a)


def test_state_evaluate_resume_and_refusals():
    case = mc.BY_NAME["deep5_signal"]
    init, data, _, _ = mc.reference_runs(case)
    half = dict(data, idx=data["idx"][:10])
    tr1, a = gpu_run(case, init, half)
    tr2, b = gpu_run(case, init, half)
    assert all(np.array_equal(a.final[k].view(np.int32), b.final[k].view(np.int32)) for k in a.final), "two trainers from one state differ"
    assert np.array_equal(a.losses, b.losses) and all(np.array_equal(a.grad1[k].view(np.int32), b.grad1[k].view(np.int32)) for k in a.grad1)
    # evaluate: no parameter, no gradient, no Adam state, no step count changes; its loss is that of the step that follows
    before = (tr1.state_dict(), tr1.gradients(), tr1.adam_state())
    ev = tr1.evaluate(data["idx"][10]).clone()
    ev2 = tr1.evaluate(data["idx"][19], data=tr1.put(data["X"].T, data["Y"].T)).clone()
    after = (tr1.state_dict(), tr1.gradients(), tr1.adam_state())
    assert _same(before[0], after[0]) and _same(before[1], after[1]) and before[2]["step"] == after[2]["step"] == 10 == tr1.step_count
    assert all(_same(before[2][s], after[2][s]) for s in ("exp_avg", "exp_avg_sq"))
    assert np.isfinite(ev.cpu().numpy()).all() and np.isfinite(ev2.cpu().numpy()).all() and ev[0].item() != ev2[0].item()
    # resume: parameters and Adam state into a fresh trainer, then the same ten steps on both
    fresh = make_trainer(case, init, data)
    fresh.load_state_dict(tr1.state_dict())
    fresh.load_adam_state(tr1.adam_state())
    assert fresh.step_count == 10
    rest = dict(data, idx=data["idx"][10:])
    _, c = gpu_run(case, init, rest, tr1)
    _, d = gpu_run(case, init, rest, fresh)
    assert c.losses[0] == ev[0].item()
    assert np.array_equal(c.losses, d.losses) and all(np.array_equal(c.final[k].view(np.int32), d.final[k].view(np.int32)) for k in c.final)
    assert tr1.step_count == fresh.step_count == 20
    whole = gpu_run(case, init, data)[1]
    assert all(np.array_equal(c.final[k].view(np.int32), whole.final[k].view(np.int32)) for k in c.final), "a run in two halves differs from the whole"
    # refusals
    small = vm.MaskTrainer(vaenmf.Classifier([9, [8], 9]), max_batch=8, device=DEV)
    small.bind(np.ones((9, 20), np.float32), np.ones((9, 20), np.float32))
    small.step(np.arange(8))
    with pytest.raises(ValueError):
        small.step(np.arange(9))                               # a ninth row beyond max_batch
    with pytest.raises(ValueError):
        small.bind(np.ones((9, 20), np.float32))               # no labels
    with pytest.raises(ValueError):
        vm.MaskTrainer(vaenmf.Classifier([9, [8], 5]), loss="signal", device=DEV)
    with pytest.raises(NotImplementedError):
        vm.MaskTrainer(vaenmf.Classifier([9, [8], 9], batch_norm=True), device=DEV)
    small.close()
    small.close()


def test_create_refuses_unsupported_shapes():
    L = vm.lib()
    h = C.c_void_p()
    cfg = lambda x, y, nh, hid, loss, mb=8: vm.MaskTrainerConfig(x, y, nh, (C.c_int32 * 8)(*(list(hid) + [0] * 8)[:8]), loss, mb, 1e-3, 0.9, 0.999, 1e-8)
    for c, word in ((cfg(9, 9, 0, [], 0), b"hidden layers"), (cfg(9, 9, 9, [8] * 8, 0), b"hidden layers"), (cfg(9, 9, 2, [8, 0], 0), b"hidden[1]"),
                    (cfg(9, 5, 1, [8], 1), b"y_dim"), (cfg(9, 5, 1, [8], 2), b"y_dim"), (cfg(0, 9, 1, [8], 0), b"x_dim"), (cfg(9, 4097, 1, [8], 0), b"y_dim"),
                    (cfg(9, 9, 1, [8], 3), b"loss"), (cfg(9, 9, 1, [8], 0, 0), b"max_batch"), (cfg(9, 9, 1, [4097], 0), b"hidden[0]")):
        assert L.vaenmf_mask_trainer_create(C.byref(c), C.byref(h)) == -1 and word in L.vaenmf_last_error() and not h.value, word
    ok = cfg(9, 5, 8, [8] * 8, 0)                              # MASK with y_dim != x_dim, eight layers
    check(L.vaenmf_mask_trainer_create(C.byref(ok), C.byref(h)))
    assert L.vaenmf_mask_trainer_num_tensors(h) == 18
    r, c = C.c_int32(), C.c_int32()
    check(L.vaenmf_mask_trainer_tensor_shape(h, 16, C.byref(r), C.byref(c)))
    assert (r.value, c.value) == (5, 8)
    assert L.vaenmf_mask_trainer_tensor_shape(h, 18, C.byref(r), C.byref(c)) == -1
    assert L.vaenmf_mask_trainer_set_step_count(h, -1) == -1
    L.vaenmf_mask_trainer_destroy(h)


# ---------------------------------------------------------------------------------------------------------------- 5. streams
@functools.lru_cache(maxsize=None)
def _cycles_per_ms():
    """torch.cuda._sleep spins for a number of device clock cycles: timed once with two events."""
    need = 20_000_000
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    a.record()
    torch.cuda._sleep(need)
    b.record()
    torch.cuda.synchronize()
    return need / a.elapsed_time(b)


def _busy(ms):
    torch.cuda._sleep(int(ms * _cycles_per_ms()))


GATE_MS, PENDING_MS = 40.0, 5.0


@functools.lru_cache(maxsize=None)
def _side_stream():
    """The side stream of both tests: one whose work the default stream's synchronise does not wait for.  With a spin queued
    on the default stream, `default_stream().synchronize()` returns after that spin (5 ms) for most streams of torch's pool
    and only after the side stream's own spin for some -- MEASURED on the MI355X: one of eight pool streams, the same one
    with nothing but the spin on it and with the trainer's calls on it, and none when the default stream is idle: a
    property of the runtime's queue assignment, not of the calls.  On such a stream work that strayed to the default
    stream would be ordered behind the gate too and could not be told from work on s, so it is not used."""
    for _ in range(16):
        s, spin_end = torch.cuda.Stream(), torch.cuda.Event()
        torch.cuda.synchronize()
        _busy(PENDING_MS)
        with torch.cuda.stream(s):
            _busy(4 * PENDING_MS)
            spin_end.record(s)
        torch.cuda.default_stream().synchronize()
        independent = not spin_end.query()
        torch.cuda.synchronize()
        if independent:
            return s
    raise AssertionError("no pool stream whose work the default stream's synchronise leaves pending")


def _gated(prepare, attempt):
    """prepare() makes the trainer (first) and the NaN buffers of one attempt; attempt(state, s, open_gate) queues everything
    on the side stream s after calling open_gate(), makes no host synchronisation and returns a function that compares the
    results.  Here: the default stream gets a spin of its own first; when attempt returns the gate must still be pending
    (the calls did not wait for their stream, and every one of them was made while the inputs held NaN), and still after
    the default stream has drained (whatever went there has then run, against NaN).  A gate that had ended says nothing:
    one more attempt with a gate four times as long, then the test fails.  An attempt's trainer is closed before the next
    gate is queued: its hipFree waits for the device."""
    s = _side_stream()
    for ms in (GATE_MS, 4 * GATE_MS):
        gate_end = torch.cuda.Event()
        state = prepare()
        torch.cuda.synchronize()
        _busy(PENDING_MS)                               # the default stream has work queued

        def open_gate():
            _busy(ms)
            gate_end.record(s)
        with torch.cuda.stream(s):
            compare = attempt(state, s, open_gate)
        first = not gate_end.query()
        torch.cuda.default_stream().synchronize()
        second = not gate_end.query()
        s.synchronize()
        torch.cuda.synchronize()
        print("gate of %.0f ms: pending when the calls had returned %s, after the default stream drained %s" % (ms, first, second))
        try:
            compare()
        finally:
            state[0].close()
            del compare, state
        if first and second:
            return
    raise AssertionError("inconclusive twice: the gate of %.0f ms had ended before the default stream had drained" % (4 * GATE_MS))


def test_step_and_evaluate_on_a_side_stream():
    """All work of the run is on a side stream s behind a gate: a spin of GATE_MS, then the copies of the frames and labels
    into device buffers that hold NaN until then, then two steps and an evaluation.  The default stream has a spin of its own
    queued when the calls are made.  A launch that went to another stream reads NaN (or races with its neighbours): the
    parameters, gradients, moments and losses are those of the default-stream run bit for bit only if every launch of
    step and evaluate is ordered on s.  No capture test: a step reads its number on the host (include/vaenmf_mask.h)."""
    case = mc.BY_NAME["deep5_msa"]
    init, data, _, _ = mc.reference_runs(case)
    Xh, Yh = torch.from_numpy(data["X"]).to(DEV), torch.from_numpy(data["Y"]).to(DEV)
    idx = [torch.from_numpy(i).to(DEV) for i in data["idx"][:3]]

    def run(tr, X, Y, outs):
        d = tr.put(X, Y)
        assert d.X.data_ptr() == X.data_ptr() and d.Y.data_ptr() == Y.data_ptr()       # taken as they are: no copy on another stream
        tr.bind(d)
        tr.step(idx[0], out=outs[0])
        tr.step(idx[1], out=outs[1])
        tr.evaluate(idx[2], out=outs[2])

    ref = make_trainer(case, init, data)
    ref_out = torch.zeros(3, 8, dtype=torch.float64, device=DEV)
    run(ref, Xh.clone(), Yh.clone(), ref_out)
    torch.cuda.synchronize()
    want = (ref.state_dict(), ref.gradients(), ref.adam_state())
    assert np.isfinite(ref_out.cpu().numpy()).all()

    def prepare():
        return (make_trainer(case, init, data), torch.full_like(Xh, float("nan")), torch.full_like(Yh, float("nan")),
                torch.full((3, 8), float("nan"), dtype=torch.float64, device=DEV))

    def attempt(state, s, open_gate):
        tr, X, Y, out = state
        open_gate()
        X.copy_(Xh, non_blocking=True)
        Y.copy_(Yh, non_blocking=True)
        run(tr, X, Y, out)

        def compare():
            got = (tr.state_dict(), tr.gradients(), tr.adam_state())
            assert same_bits(out, ref_out), (out.cpu(), ref_out.cpu())
            assert _same(want[0], got[0]) and _same(want[1], got[1]) and want[2]["step"] == got[2]["step"] == 2
            assert all(_same(want[2][k], got[2][k]) for k in ("exp_avg", "exp_avg_sq"))
        return compare
    _gated(prepare, attempt)


def test_set_get_and_head_on_a_side_stream():
    """vaenmf_mask_trainer_set_tensor, vaenmf_mask_trainer_get_tensor and vaenmf_mse_head through the C ABI behind the same
    gate, with no host synchronisation between the gate and the last call.  The sources of set and the head's inputs hold NaN
    until the copies on s have run; the destinations of get and the head's outputs are NaN device tensors.  A set on
    another stream stores NaN, a get on another stream returns the state the trainer had before, a head on another stream
    computes on NaN."""
    L = vm.lib()
    case = mc.BY_NAME["uneven_mask"]
    init, data, r64, _ = mc.reference_runs(case)
    new = [torch.from_numpy(np.asarray(r64.final[k], np.float32)).to(DEV) for k in vm.state_keys(len(case.hidden))]     # any other state
    assert not any(same_bits(v.cpu(), init[k]) for v, k in zip(new, init))
    rng = np.random.default_rng(77)
    B, D = 17, 65
    a, y, P = (torch.from_numpy(v).to(DEV) for v in head_inputs(rng, B, D))
    ref_dA, ref_rows = torch.zeros(B, D, device=DEV), torch.zeros(B, dtype=torch.float64, device=DEV)
    check(L.vaenmf_mse_head(p(a), D, p(y), D, p(P), D, B, D, 2, p(ref_dA), D, p(ref_rows), st()))
    torch.cuda.synchronize()
    assert np.isfinite(ref_dA.cpu().numpy()).all() and np.isfinite(ref_rows.cpu().numpy()).all()

    def prepare():
        nan = lambda vs: [torch.full_like(v, float("nan")) for v in vs]
        return make_trainer(case, init, data), nan(new), nan(new), nan((a, y, P)), nan((ref_dA, ref_rows))

    def attempt(state, s, open_gate):
        tr, src, back, (a2, y2, P2), (dA, rows) = state
        sp = C.c_void_p(s.cuda_stream)
        open_gate()
        for dst, v in list(zip(src, new)) + [(a2, a), (y2, y), (P2, P)]:
            dst.copy_(v, non_blocking=True)
        rc = [L.vaenmf_mask_trainer_set_tensor(tr._h, vm.MASK_PARAM, i, p(v), sp) for i, v in enumerate(src)]
        rc += [L.vaenmf_mask_trainer_set_tensor(tr._h, vm.MASK_ADAM_V, i, p(v), sp) for i, v in enumerate(src)]
        rc.append(L.vaenmf_mse_head(p(a2), D, p(y2), D, p(P2), D, B, D, 2, p(dA), D, p(rows), sp))
        rc += [L.vaenmf_mask_trainer_get_tensor(tr._h, vm.MASK_PARAM if i % 2 else vm.MASK_ADAM_V, i, p(v), sp) for i, v in enumerate(back)]

        def compare():
            assert all(v == 0 for v in rc), (rc, L.vaenmf_last_error().decode())
            for i, (v, w) in enumerate(zip(back, new)):
                assert same_bits(v, w), "tensor %d read back on the side stream differs from what was set there" % i
            sd = tr.state_dict()                            # and on the default stream afterwards
            assert all(same_bits(sd[k], w.cpu()) for k, w in zip(tr.keys, new))
            assert same_bits(dA, ref_dA) and same_bits(rows, ref_rows)
        return compare
    _gated(prepare, attempt)


# ---------------------------------------------------------------------------------------------------------------- 6. fit
def test_fit_mask_filter(tmp_path):
    f, F = mc.fit_frames(), mc.FIT["x_dim"]
    model_dir = str(tmp_path)
    tr, hist = vaenmf.fit_mask_filter(mc.fit_model(), (f["Xt"], f["Yt"], f["mean"], f["std"]), (f["Xv"], f["Yv"]), model_dir, loss="mask",
                                      epochs=mc.FIT["epochs"], batch_size=mc.FIT["batch_size"], seed=mc.FIT["seed"], device=DEV)
    nb = -(-f["Xt"].shape[1] // mc.FIT["batch_size"])
    assert tr.step_count == 2 * nb and f["Xt"].shape[1] % mc.FIT["batch_size"] != 0          # a short last batch, twice
    log = open(os.path.join(model_dir, "output_epoch.log")).read()
    lines = sum([vm.epoch_log_lines(h["epoch"], h["train"]["loss"], h["valid"]["loss"]) for h in hist], [])
    assert log == "\n".join(lines) + "\n" and len(lines) == 6 and lines[0] == "Epoch: 1" and lines[3] == "Epoch: 2"
    assert lines[1].startswith("[Train]       Loss: ") and lines[1].endswith("    ") and lines[2].startswith("[Validation] Loss: ") and lines[2].endswith("    ")
    names = sorted(n for n in os.listdir(model_dir) if n.endswith(".pt"))
    assert names == sorted("Classifier_epoch_{:03d}_vloss_{:.6f}.pt".format(h["epoch"], h["valid"]["loss"]) for h in hist)
    assert [os.path.basename(h["checkpoint"]) for h in hist] == [vm.checkpoint_name(h["epoch"], h["valid"]["loss"]) for h in hist]
    assert np.array_equal(np.load(os.path.join(model_dir, "trainset_mean.npy")), f["mean"])
    assert np.array_equal(np.load(os.path.join(model_dir, "trainset_std.npy")), f["std"])
    # the float64 restatement of the loop, with the permutations fit_mask_filter draws from its seed: the epoch means
    # (total / t, the short last batch included) within FACTOR of what float32 leaves on them (the yardstick is held to be
    # neither zero nor beyond float32 rounding in tests/test_train_mask_cpu.py); the restatement's validation loss falls too
    r64, r32 = mc.fit_restatement(torch.float64), mc.fit_restatement(torch.float32)
    got = np.array([(h["train"]["loss"], h["valid"]["loss"]) for h in hist])
    eg, ey = mc.loss_err(got, np.array(r64)), mc.loss_err(np.array(r32), np.array(r64))
    print("epoch means: gpu %s, float64 %s; error %.3g, float32 yardstick %.3g" % (got.tolist(), r64, eg, ey))
    assert eg <= mc.FACTOR * ey, (eg, ey)
    assert hist[1]["valid"]["loss"] < hist[0]["valid"]["loss"] and r64[1][1] < r64[0][1], "the validation loss did not fall"
    sd = torch.load(hist[-1]["checkpoint"], map_location="cpu")
    fresh = vaenmf.Classifier([F, list(mc.FIT["hidden"]), F])
    fresh.load_state_dict(sd, strict=True)
    assert _same(sd, tr.state_dict()) and any(not torch.equal(sd[k], mc.fit_model().state_dict()[k]) for k in sd)
    # the checkpoint as it is into MaskEnhancer: its mask against the float64 forward of the checkpoint
    import vaenmf_oracle as orc
    from vaenmf.pipeline import MaskEnhancer
    layers = vaenmf.engine.classifier_layers_from_state(sd)
    assert len(layers) == 6
    mean, std = np.load(os.path.join(model_dir, "trainset_mean.npy")), np.load(os.path.join(model_dir, "trainset_std.npy"))
    enh = MaskEnhancer(layers, F, mean, std, wlen_sec=mc.FIT["wlen_sec"], device=DEV)
    wav = f["wav"]
    s_hat, mask = enh.enhance(torch.from_numpy(wav).to(DEV), [len(wav)])
    X = orc.stft(wav, fs=16000, wlen_sec=mc.FIT["wlen_sec"], hop_percent=0.25)                 # (F, N)
    xin = torch.from_numpy(((np.abs(X.T) ** 2).astype(np.float32).astype(np.float64) - mean.T) / (std.astype(np.float64) + 1e-8).T)
    with torch.no_grad():
        m_ref = mc.forward({k: v.double() for k, v in sd.items()}, 5, xin).numpy()
    assert mask.shape == m_ref.shape and s_hat.shape == (len(wav),) and bool(torch.isfinite(s_hat).all())
    err = float(np.max(np.abs(mask.cpu().numpy() - m_ref)))
    print("MaskEnhancer mask against the float64 forward: %.3g" % err)
    assert err < 2e-5                                      # the bound of tests/test_gpu_parity.py::test_mask_baseline_against_oracle
