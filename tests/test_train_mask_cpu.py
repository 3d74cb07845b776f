"""The mask trainer without a GPU: the host-side pieces of vaenmf.train_mask, the float64 / float32 restatement of
tests/mask_train_cases.py against the steps recorded from the reference (tests/golden/train_mask_f65.npz,
tests/golden/make_train_mask_golden.py), the yardsticks the GPU tests divide by, and what the new subsystem must leave as
it was: vaenmf.train's refusals, _lib.SIGNATURES and the stream prototypes of include/vaenmf.h.

The recorded run and the float32 restatement are float32 runs of the same mathematics in different operation orders; the
recorded run's error against the float64 restatement may be at most 4 times the float32 restatement's
(tests/test_train_cpu.py)."""
import os
import re

import numpy as np
import pytest
import torch

import mask_train_cases as mc
import vaenmf
from helpers import nrm_err
from vaenmf import _lib
from vaenmf import train as vt
from vaenmf import train_mask as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mask_spec_accepts_and_refuses():
    assert vm.mask_spec(vaenmf.Classifier([9, [8], 9])) == vm.MaskSpec(9, 9, [8])
    assert vm.mask_spec(vaenmf.Classifier([513, [128] * 8, 513])).hidden == [128] * 8
    assert vm.mask_spec(vaenmf.Classifier([9, [8, 7], 5])) == vm.MaskSpec(9, 5, [8, 7])
    none = vaenmf.Classifier([9, [8], 9])
    none.hidden = torch.nn.ModuleList([])                                       # no hidden layer
    for bad in (none, vaenmf.Classifier([9, [8] * 9, 9]), vaenmf.Classifier([9, [8], 9], batch_norm=True), vaenmf.Classifier2Classes([9, [8], 9]),
                vaenmf.VariationalAutoencoder([9, 4, [8]]), vaenmf.DeepGenerativeModel([9, 1, 4, [8]], None), torch.nn.Linear(3, 3),
                vaenmf.Classifier([5000, [8], 9])):
        with pytest.raises(NotImplementedError):
            vm.mask_spec(bad)
    assert vaenmf.mask_spec is vm.mask_spec and vaenmf.MaskTrainer is vm.MaskTrainer and vaenmf.fit_mask_filter is vm.fit_mask_filter


def test_state_keys_and_shapes_for_five_layers():
    model = vaenmf.Classifier([513, [128] * 5, 513])
    sd = model.state_dict()
    keys = vm.state_keys(5)
    assert keys == list(sd.keys())                                # the trainer's tensor order is the module's registration order
    assert keys[:2] == ["hidden.0.weight", "hidden.0.bias"] and keys[-2:] == ["output_layer.weight", "output_layer.bias"] and len(keys) == 12
    shapes = vm.state_shapes(vm.mask_spec(model))
    assert shapes == [tuple(sd[k].shape) for k in keys]
    assert shapes[0] == (128, 513) and shapes[1] == (128,) and shapes[2] == (128, 128) and shapes[-2] == (513, 128) and shapes[-1] == (513,)
    for case in mc.CASES:
        m = mc.make_model(case)
        assert vm.state_shapes(vm.mask_spec(m)) == [tuple(v.shape) for v in m.state_dict().values()], case.name


def test_checkpoint_names_and_log_lines():
    assert vm.checkpoint_name(3, 0.1234567) == "Classifier_epoch_003_vloss_0.123457.pt"
    assert vm.checkpoint_name(100, 12.5) == "Classifier_epoch_100_vloss_12.500000.pt"
    assert vm.epoch_log_lines(2, 1.5, 0.25) == ["Epoch: 2", "[Train]       Loss: 1.500000    ", "[Validation] Loss: 0.250000    "]
    assert vm.epoch_log_lines(11, 0.00012345, 3.0)[1] == "[Train]       Loss: 0.000123    "


@pytest.mark.parametrize("loss", mc.LOSS_NAMES)
def test_restatement_reproduces_reference(loss):
    g, r64, r32 = mc.golden_runs(loss)
    ours = mc.state_of(mc.make_model(mc.GOLDEN_CASE))
    assert list(ours) == list(g["init"]) and all(torch.equal(ours[k], g["init"][k]) for k in ours), "the golden seed no longer draws the recorded state"
    draw = mc.golden_draw()
    z = np.load(mc.GOLDEN_FILE)
    for k in draw:
        assert np.array_equal(z[k], draw[k]), "golden_draw no longer gives the recorded %s" % k
    assert sorted(g["final"][loss]) == sorted(vm.state_keys(5))
    for label, keys in mc.groups(mc.GOLDEN_CASE):
        eg, er = nrm_err(mc.cat(g["final"][loss], keys), mc.cat(r64.final, keys)), nrm_err(mc.cat(r32.final, keys), mc.cat(r64.final, keys))
        print("%s %s: recorded %.3g, float32 restatement %.3g" % (loss, label, eg, er))
        assert eg <= mc.GOLDEN_FACTOR * er, (label, eg, er)
    eg, er = mc.loss_err(g["losses"][loss], r64.losses), mc.loss_err(r32.losses, r64.losses)
    print("%s losses: recorded %.3g, float32 restatement %.3g" % (loss, eg, er))
    assert eg <= mc.GOLDEN_FACTOR * er, (eg, er)
    assert os.path.getsize(mc.GOLDEN_FILE) < 1 << 20


@pytest.mark.parametrize("case", mc.CASES + [mc.GOLDEN_CASE], ids=lambda c: c.name)
def test_yardsticks(case):
    """The GPU tests divide by these: every tensor group's float32 error against float64 is neither zero nor beyond float32
    rounding -- (0, 1e-5] for the step-1 gradient, (0, 1e-4] for the parameters after the run, the windows of
    tests/test_train_cpu.py -- the per-step losses likewise, and the weights moved."""
    if case is mc.GOLDEN_CASE:
        runs = [(g["init"], r64, r32) for g, r64, r32 in (mc.golden_runs(loss) for loss in mc.LOSS_NAMES)]
    else:
        init, _, r64, r32 = mc.reference_runs(case)
        runs = [(init, r64, r32)]
    for init, r64, r32 in runs:
        assert list(r64.final) == vm.state_keys(len(case.hidden))
        for label, keys in mc.groups(case):
            eg, ep = nrm_err(mc.cat(r32.grad1, keys), mc.cat(r64.grad1, keys)), nrm_err(mc.cat(r32.final, keys), mc.cat(r64.final, keys))
            print("%s %s: step-1 gradient %.3g, parameters after %d steps %.3g" % (case.name, label, eg, len(r64.losses), ep))
            assert 0.0 < eg <= 1e-5, (label, eg)
            assert 0.0 < ep <= 1e-4, (label, ep)
        el = mc.loss_err(r32.losses, r64.losses)
        assert 0.0 < el <= 1e-5, el
        assert np.isfinite(r64.losses).all()
        for k in r64.final:
            if k.endswith("weight"):
                assert np.abs(r64.final[k] - np.asarray(init[k])).max() > 1e-3, "the parameters did not move: the run tests nothing"


def test_fit_restatement_validation_loss_falls():
    """The seed of the GPU fit test: in float64 on the host the validation loss of epoch 2 is below that of epoch 1."""
    f = mc.fit_frames()
    assert f["Xt"].shape[0] == 65 and 200 <= f["Xt"].shape[1] <= 600 and f["Xt"].shape[1] % mc.FIT["batch_size"] != 0      # a short last batch
    assert f["Yt"].min() >= 0.0 and f["Yt"].max() <= 1.0
    hist = mc.fit_restatement()
    print(hist)
    assert len(hist) == 2 and hist[1][1] < hist[0][1]
    ey = mc.loss_err(np.array(mc.fit_restatement(torch.float32)), np.array(hist))      # the yardstick of the epoch means on the GPU
    print("float32 yardstick of the epoch means %.3g" % ey)
    assert 0.0 < ey <= 1e-5, ey


def test_restatement_forward_is_the_classifiers():
    """The restatement's forward is written out over a parameter dict (autograd needs leaves of the run's dtype); it is
    vaenmf.models.Classifier.forward: the same values in float64, to float64 rounding, for every case's shape."""
    for case in mc.CASES:
        model = mc.make_model(case).double()
        x = torch.from_numpy(mc.make_data(case)["X"]).double()
        with torch.no_grad():
            want, got = model(x), mc.forward(dict(model.state_dict()), len(case.hidden), x)
        assert want.shape == got.shape == (mc.POOL, case.x_dim)
        assert float((want - got).abs().max()) <= 1e-12, case.name


def test_the_old_trainer_is_as_it_was():
    with pytest.raises(NotImplementedError):
        vt.fit_wiener_filter()
    with pytest.raises(NotImplementedError):
        vt.model_spec(vaenmf.Classifier([9, [8, 8, 8], 9]))
    with pytest.raises(NotImplementedError):
        vt.model_spec(vaenmf.Classifier([9, [8], 1], batch_norm=True))
    assert not set(vm.MASK_SIGNATURES) & set(_lib.SIGNATURES)
    assert not any("mask_trainer" in k or k == "vaenmf_mse_head" for k in _lib.SIGNATURES)
    strip = lambda text: re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    protos = lambda text: re.findall(r"\b(vaenmf_\w+)\s*\(([^;{}]*?)\)\s*;", strip(text), flags=re.S)
    old = protos(open(os.path.join(ROOT, "include", "vaenmf.h")).read())
    assert {n for n, _ in old} == set(_lib.SIGNATURES)
    assert len([n for n, a in old if re.search(r"\bvoid\s*\*\s*stream\b", a)]) == 50
    new = protos(open(os.path.join(ROOT, "include", "vaenmf_mask.h")).read())
    assert {n for n, _ in new} == set(vm.MASK_SIGNATURES)         # the new header's prototypes are exactly the new table's keys
    assert len(new) == len({n for n, _ in new})
    for name, args in new:                                        # and the table's arities are the prototypes'
        assert len(vm.MASK_SIGNATURES[name][1]) == len([a for a in args.split(",") if a.strip()]), name
    assert sorted(n for n, a in new if re.search(r"\bvoid\s*\*\s*stream\b", a)) == sorted(mc_stream_entries())


def mc_stream_entries():
    """The new entry points that take a stream: each has a stream test in tests/test_gpu_train_mask.py."""
    return ["vaenmf_mse_head", "vaenmf_mask_trainer_set_tensor", "vaenmf_mask_trainer_get_tensor", "vaenmf_mask_trainer_step", "vaenmf_mask_trainer_eval"]


def test_library_exports_the_mask_symbols():
    lib = vm.lib()                         # loads libvaenmf.so and binds the new table; AttributeError if a symbol is missing
    for name in vm.MASK_SIGNATURES:
        assert hasattr(lib, name), name
    assert lib is _lib.lib()
