"""Training without a GPU: the float64 / float32 restatement of tests/train_cases.py against the trajectories recorded from
the reference (tests/golden/train_*.npz, tests/golden/make_train_golden.py), the yardsticks the GPU tests measure against,
and the host-side pieces of vaenmf.train.

How the restatement is held to the goldens.  Both are float32 runs of the same mathematics in different operation orders
(nn.Linear's addmm against x @ W.T + b, log(exp(a)) against the reference's log(r)), so neither is the other's bits.  Each
has an error against the float64 restatement; the recorded run's error may be at most FACTOR = 4 times the float32
restatement's on the same case (reordering a batch moves these errors by 1.2x; 4 leaves room for the different blocking of
the two matrix products and nothing for a different formula, whose error would be orders of magnitude above float32
rounding)."""
import hashlib

import numpy as np
import pytest
import torch

import train_cases as tc
import vaenmf
from helpers import nrm_err
from vaenmf import train as vt

FACTOR = 4.0


def _digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(np.asarray(sd[k], dtype=np.float32)).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def _loss_err(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


@pytest.mark.parametrize("name", sorted(tc.GOLDEN_CASES))
def test_restatement_reproduces_reference(name):
    case = tc.GOLDEN_CASES[name]
    gold = tc.load_golden(name)
    init, data, r64, r32 = tc.reference_runs(case)
    assert np.array_equal(_digest({k: v.numpy() for k, v in init.items()}), gold["init_sha256"]), "the case's initial weights are not the recorded run's"
    z = np.load(tc.GOLDEN + "/" + name + ".npz")
    for k in ("X", "Y", "idx", "eps", "mean", "std"):
        if data[k] is not None:
            assert np.array_equal(z[k], data[k]), "make_data no longer gives the recorded %s" % k
    keys = vt.state_keys(case.kind, len(case.hidden))
    assert sorted(gold["grad1"]) == sorted(keys) and sorted(gold["final"]) == sorted(keys)
    for k in keys:
        for what, g, a64, a32 in (("grad1", gold["grad1"][k], r64.grad1[k], r32.grad1[k]), ("final", gold["final"][k], r64.final[k], r32.final[k])):
            eg, er = nrm_err(g, a64), nrm_err(a32, a64)
            print("%s %s %s: recorded %.3g, float32 restatement %.3g" % (name, what, k, eg, er))
            assert eg <= FACTOR * er, (what, k, eg, er)
    ncol = 1 if case.kind == "Classifier" else 3
    eg, er = _loss_err(gold["losses"][:, :ncol], r64.losses[:, :ncol]), _loss_err(r32.losses[:, :ncol], r64.losses[:, :ncol])
    print("%s losses: recorded %.3g, float32 restatement %.3g" % (name, eg, er))
    assert eg <= FACTOR * er
    if case.kind == "Classifier":
        assert np.array_equal(gold["counts"], r32.counts)
        assert np.abs(gold["counts"] - r64.counts).max() <= 1          # a y_hat within float32 rounding of 0.5 may fall on either side


@pytest.mark.parametrize("name", sorted(tc.GOLDEN_CASES))
def test_yardsticks(name):
    """What float32 leaves on these cases: the step-1 gradient to a few 1e-7, the parameters after 20 steps to 1e-7 .. 1e-5
    against a movement of 2e-2 -- the scale the GPU tests' factor multiplies.  A yardstick far outside would make that test
    vacuous (or impossible), so it is pinned here: (0, 1e-5] and (0, 1e-4]."""
    case = tc.GOLDEN_CASES[name]
    init, _, r64, r32 = tc.reference_runs(case)
    for k in r64.final:
        eg, ep = nrm_err(r32.grad1[k], r64.grad1[k]), nrm_err(r32.final[k], r64.final[k])
        assert 0.0 < eg <= 1e-5, (k, eg)
        assert 0.0 < ep <= 1e-4, (k, ep)
        if k.endswith("weight"):
            assert np.abs(r64.final[k] - init[k].numpy()).max() > 1e-3, "the parameters did not move: the trajectory tests nothing"
    assert r64.losses[-1, 0] < r64.losses[0, 0] or case.kind == "Classifier"


def test_checkpoint_names():
    assert vt.checkpoint_name("M1", 3, 512.3456) == "M1_epoch_003_vloss_512.35.pt"
    assert vt.checkpoint_name("M2", 12, 466.719) == "M2_epoch_012_vloss_466.72.pt"
    assert vt.checkpoint_name("Classifier", 100, 0.12345) == "Classifier_epoch_100_vloss_0.123.pt"


@pytest.mark.parametrize("name", sorted(tc.GOLDEN_CASES))
def test_key_layout_and_strict_loading(name):
    case = tc.GOLDEN_CASES[name]
    model = tc.make_model(case)
    keys = vt.state_keys(case.kind, len(case.hidden))
    assert keys == list(model.state_dict().keys())                # the trainer's tensor order is the module's registration order
    spec = vt.model_spec(model)
    assert (spec.kind, spec.x_dim, spec.y_dim, spec.z_dim, tuple(spec.hidden)) == (case.kind, case.x_dim, case.y_dim, case.z_dim, case.hidden)
    gold = tc.load_golden(name)
    fresh = tc.make_model(case._replace(seed=case.seed + 1))
    fresh.load_state_dict({k: torch.tensor(gold["final"][k]) for k in keys}, strict=True)
    for k, v in fresh.state_dict().items():
        assert np.array_equal(v.numpy(), gold["final"][k])


def test_m2_with_a_classifier_keeps_its_keys():
    clf = vaenmf.Classifier([9, [8], 1])
    model = vaenmf.DeepGenerativeModel([9, 1, 4, [8]], clf)
    keys = vt.state_keys("M2", 1)
    sd = list(model.state_dict().keys())
    assert [k for k in sd if not k.startswith("classifier.")] == keys and any(k.startswith("classifier.") for k in sd)


def test_batch_bookkeeping():
    assert vt.batch_bounds(2000, 128)[-1] == (1920, 2000) and len(vt.batch_bounds(2000, 128)) == 16       # drop_last=False
    assert vt.batch_bounds(256, 128) == [(0, 128), (128, 256)]
    assert vt.batch_bounds(1, 128) == [(0, 1)]
    b = vt.batch_bounds(333, 33)
    assert b[0][0] == 0 and b[-1][1] == 333 and all(x[1] == y[0] for x, y in zip(b, b[1:])) and b[-1][1] - b[-1][0] == 3
    with pytest.raises(ValueError):
        vt.batch_bounds(0, 128)
    rng = np.random.default_rng(5)
    p1, p2 = rng.permutation(333), rng.permutation(333)
    assert sorted(p1) == list(range(333)) and not np.array_equal(p1, p2)                                     # a fresh permutation per epoch


def test_epoch_log_lines():
    v = vt.epoch_log_lines("M1", 2, {"loss": 1.234, "recon": 1.0, "kl": 0.234}, {"loss": 2.0, "recon": 1.5, "kl": 0.5})
    assert v == ["Epoch: 2", "[Train]\t\t ELBO: 1.23, Recon.: 1.00, KL: 0.23", "[Validation]\t ELBO: 2.00, Recon.: 1.50, KL: 0.50"]
    c = vt.epoch_log_lines("Classifier", 1, {"loss": 0.5, "f1": 0.25}, {"loss": 0.75, "f1": 0.5})
    assert c == ["Epoch: 1", "[Train]       Loss: 0.50    F1_score: 0.25", "[Validation] Loss: 0.75    F1_score: 0.50"]
    assert abs(vt.f1_from_counts(5.0, 3.0, 1.0, 1.0) - 2 * (5 / 6) ** 2 / (10 / 6)) < 1e-6


def test_unsupported_shapes_are_refused():
    with pytest.raises(NotImplementedError):
        vt.model_spec(vaenmf.Classifier([9, [8], 1], batch_norm=True))
    with pytest.raises(NotImplementedError):
        vt.model_spec(vaenmf.Classifier2Classes([9, [8], 1]))
    with pytest.raises(NotImplementedError):
        vt.model_spec(vaenmf.VariationalAutoencoder([9, 4, [8, 8, 8]]))        # three hidden layers
    with pytest.raises(NotImplementedError):
        vt.model_spec(vaenmf.VariationalAutoencoder([9, 6, [8]]))              # z_dim not a multiple of 4
    with pytest.raises(NotImplementedError):
        vt.model_spec(vaenmf.VariationalAutoencoder([5000, 4, [8]]))
    with pytest.raises(NotImplementedError):
        vt.model_spec(torch.nn.Linear(3, 3))
    with pytest.raises(NotImplementedError):
        vt.fit_wiener_filter()
    with pytest.raises(NotImplementedError):
        vt._arrays("train.h5", True)
    assert vt.model_spec(vaenmf.VariationalAutoencoder([513, 16, [256]])).hidden == [256]


# ---- unequal widths, schedules, the Adam state loader ---------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tc.SHAPE_CASES))
def test_shape_case_yardsticks_are_not_zero(name):
    """The GPU tests divide by these: every tensor (tc.groups: every layer, where the biases have four elements) has a
    float32 error against float64 that is neither zero nor beyond float32 rounding, and the weights moved."""
    case = tc.SHAPE_CASES[name]
    init, _, r64, r32 = tc.reference_runs(case)
    assert list(r64.final) == list(tc.make_model(case).state_dict().keys())
    assert (len(tc.groups(case)) < len(r64.final)) == (name == "m1_one_z4")     # per layer only where a tensor has < 8 elements
    for label, keys in tc.groups(case):
        eg, ep = nrm_err(tc.cat(r32.grad1, keys), tc.cat(r64.grad1, keys)), nrm_err(tc.cat(r32.final, keys), tc.cat(r64.final, keys))
        print("%s %s: step-1 gradient %.3g, parameters after %d steps %.3g" % (name, label, eg, tc.STEPS, ep))
        assert 0.0 < eg <= 1e-5, (label, eg)
        assert 0.0 < ep <= 1e-4, (label, ep)
    for k in r64.final:
        if k.endswith("weight"):
            assert np.abs(r64.final[k] - init[k].numpy()).max() > 1e-3, "the parameters did not move: the trajectory tests nothing"
    ncol = 1 if case.kind == "Classifier" else 3
    assert _loss_err(r32.losses[:, :ncol], r64.losses[:, :ncol]) > 0.0


def test_constant_schedule_is_the_plain_case():
    """The schedule form with the same batch size at every step draws the same data and runs the same steps, bit for bit."""
    for name in ("m2_uneven", "clf_uneven"):
        case = tc.SHAPE_CASES[name]
        sched = case._replace(B=(case.B,) * tc.STEPS)
        init, data, _, r32 = tc.reference_runs(case)
        ds = tc.make_data(sched)
        assert isinstance(ds["idx"], list) and np.array_equal(np.stack(ds["idx"]), data["idx"]) and np.array_equal(ds["X"], data["X"])
        if data["eps"] is not None:
            assert np.array_equal(np.stack(ds["eps"]), data["eps"])
        got = tc.run_steps(sched, init, ds, torch.float32)
        assert np.array_equal(got.losses, r32.losses) and np.array_equal(got.counts, r32.counts) and got.evals is None
        for k in r32.final:
            assert np.array_equal(got.final[k].view(np.int32), r32.final[k].view(np.int32)), k
            assert np.array_equal(got.grad1[k].view(np.int32), r32.grad1[k].view(np.int32)), k


@pytest.mark.parametrize("name", sorted(tc.SCHED_CASES))
def test_scheduled_yardsticks(name):
    """The ragged schedule with evaluations between its steps: the yardsticks the GPU test divides by are not zero, and an
    evaluation takes part in nothing (the run without them ends in the same bits)."""
    case = tc.SCHED_CASES[name]
    init, data, evals, r64, r32 = tc.scheduled_runs(case)
    assert [len(i) for i in data["idx"]] == list(tc.SCHED) and len(set(data["idx"][0].tolist())) < 128      # 128 of 96 rows repeat
    assert r64.evals.shape == (len(tc.EVAL_AFTER), len(tc.EVAL_BATCHES), 3) and np.isfinite(r64.evals).all()
    for label, keys in tc.groups(case):
        assert 0.0 < nrm_err(tc.cat(r32.final, keys), tc.cat(r64.final, keys)) <= 1e-4, label
    plain = tc.run_steps(case, init, data, torch.float32, len(tc.SCHED))
    assert all(np.array_equal(plain.final[k].view(np.int32), r32.final[k].view(np.int32)) for k in r32.final)
    assert np.array_equal(plain.losses, r32.losses)


def test_adam_state_loader_checks():
    for name in sorted(tc.SHAPE_CASES):
        case = tc.SHAPE_CASES[name]
        model = tc.make_model(case)
        spec, keys = vt.model_spec(model), vt.state_keys(case.kind, len(case.hidden))
        shapes = vt.state_shapes(spec)
        assert shapes == [tuple(model.state_dict()[k].shape) for k in keys], name
    zeros = lambda: {k: torch.zeros(s) for k, s in zip(keys, shapes)}
    good = {"step": 9, "exp_avg": zeros(), "exp_avg_sq": zeros()}
    assert vt.check_adam_state(good, keys, shapes) == 9
    assert vt.check_adam_state(dict(good, step=0), keys, shapes) == 0
    with pytest.raises(KeyError):
        vt.check_adam_state({"step": 9, "exp_avg": zeros()}, keys, shapes)                      # no second moment
    with pytest.raises(KeyError):
        vt.check_adam_state(dict(good, max_exp_avg_sq=zeros()), keys, shapes)                    # amsgrad is not run
    lacking = zeros()
    del lacking[keys[-1]]
    with pytest.raises(KeyError):
        vt.check_adam_state(dict(good, exp_avg=lacking), keys, shapes)
    with pytest.raises(KeyError):
        vt.check_adam_state(dict(good, exp_avg_sq=dict(zeros(), extra=torch.zeros(1))), keys, shapes)
    wrong = zeros()
    wrong[keys[0]] = torch.zeros(shapes[0][::-1])                                                # the weight transposed
    with pytest.raises(ValueError):
        vt.check_adam_state(dict(good, exp_avg_sq=wrong), keys, shapes)
    assert vt.check_adam_state(dict(good, exp_avg={k: v.tolist() for k, v in zeros().items()}), keys, shapes) == 9    # nested lists
    with pytest.raises(ValueError):
        vt.check_adam_state(dict(good, exp_avg=dict(zeros(), **{keys[1]: [0.0]})), keys, shapes)
    for step in (-1, 2 ** 31 - 1, 1.5, True, "9", None, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            vt.check_adam_state(dict(good, step=step), keys, shapes)
