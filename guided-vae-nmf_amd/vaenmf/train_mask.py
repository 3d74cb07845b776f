"""Training the supervised Wiener-mask baseline on the GPU: the build's counterpart of the reference's
scripts/training_wiener_filter.py (csrc/train_mask.hip; include/vaenmf_mask.h states the arithmetic).

  MaskTrainer      a vaenmf.models.Classifier (batch_norm=False, 1 .. 8 hidden layers): its parameters, gradients and Adam
                   state on the device and the step that updates them -- gather, relu layers forward and backward in fp32 on
                   the matrix pipe, one of the three MSE heads of python/models/utils.py:93-104, torch.optim.Adam
  fit_mask_filter  the loop of training_wiener_filter.py:113-188: a fresh permutation per epoch, a short last batch,
                   per-epoch means in output_epoch.log, a checkpoint per epoch under the script's name

The chain it closes: dataset.make_train_set(labels="noisy_wiener_labels") -> fit_mask_filter -> pipeline.MaskEnhancer.  A
checkpoint is a state_dict in the reference's key layout: it loads with strict=True into vaenmf.Classifier and goes as it
is through engine.classifier_layers_from_state into MaskEnhancer.

This subsystem has a header and a ctypes table of its own (MASK_SIGNATURES, applied to the handle vaenmf._lib.lib()
returns); vaenmf.train, its refusals and _lib.SIGNATURES are as they were.  There is no CPU fallback: a MaskTrainer needs the
HIP library and a GPU.  Host-only (no library): mask_spec, state_keys, state_shapes, checkpoint_name, epoch_log_lines.

Not built: Classifier(batch_norm=True), Classifier2Classes, the HDF5 loader, data-parallel training, capturing a step into a
graph (a step reads its number on the host) -- NotImplementedError where reachable."""
import collections
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from . import models as vmodels
from ._lib import check
from .train import Data, _arrays, _ptr, _stream, batch_bounds, check_adam_state, read_losses

MaskSpec = collections.namedtuple("MaskSpec", "x_dim y_dim hidden")
LOSSES = {"mask": 0, "signal": 1, "msa": 2}            # VAENMF_MSE_*
MASK_PARAM, MASK_GRAD, MASK_ADAM_M, MASK_ADAM_V = 0, 1, 2, 3
MAX_HIDDEN, MAX_DIM, MAX_BATCH = 8, 4096, 65536


class MaskTrainerConfig(C.Structure):
    _fields_ = [("x_dim", C.c_int32), ("y_dim", C.c_int32), ("n_hidden", C.c_int32), ("hidden", C.c_int32 * 8), ("loss", C.c_int32),
                ("max_batch", C.c_int32), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("adam_eps", C.c_double)]


# name -> (restype, argtypes); every symbol include/vaenmf_mask.h declares
_P, _I, _I64, _F = C.c_void_p, C.c_int32, C.c_int64, C.c_float
MASK_SIGNATURES = {
    "vaenmf_mse_head": (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _P, _I, _P, _P]),
    "vaenmf_mask_trainer_create": (_I, [C.POINTER(MaskTrainerConfig), C.POINTER(_P)]),
    "vaenmf_mask_trainer_destroy": (None, [_P]),
    "vaenmf_mask_trainer_num_tensors": (_I, [_P]),
    "vaenmf_mask_trainer_tensor_shape": (_I, [_P, _I, C.POINTER(_I), C.POINTER(_I)]),
    "vaenmf_mask_trainer_set_tensor": (_I, [_P, _I, _I, _P, _P]),
    "vaenmf_mask_trainer_get_tensor": (_I, [_P, _I, _I, _P, _P]),
    "vaenmf_mask_trainer_set_norm": (_I, [_P, _P, _P, _F]),
    "vaenmf_mask_trainer_step_count": (_I64, [_P]),
    "vaenmf_mask_trainer_set_step_count": (_I, [_P, _I64]),
    "vaenmf_mask_trainer_step": (_I, [_P, _P, _I, _P, _I, _I64, _P, _I, _P, _P]),
    "vaenmf_mask_trainer_eval": (_I, [_P, _P, _I, _P, _I, _I64, _P, _I, _P, _P]),
}

_bound = None


def lib():
    """vaenmf._lib.lib()'s handle with this module's symbols bound too; raises if the library lacks one."""
    global _bound
    l = _lib.lib()
    if _bound is not l:
        for name, (res, args) in MASK_SIGNATURES.items():
            fn = getattr(l, name)           # AttributeError if a declared symbol is missing
            fn.restype = res
            fn.argtypes = args
        _bound = l
    return l


def mask_spec(model):
    """MaskSpec(x_dim, y_dim, hidden) of a vaenmf.models.Classifier(batch_norm=False) with 1 .. 8 hidden layers, or
    NotImplementedError for what the mask trainer does not run.  Pure: needs neither the library nor a GPU."""
    if not isinstance(model, vmodels.Classifier):
        raise NotImplementedError("the mask trainer runs Classifier(batch_norm=False); got %s" % type(model).__name__)
    if any(isinstance(m, torch.nn.BatchNorm1d) for m in model.hidden):
        raise NotImplementedError("Classifier(batch_norm=True) is not trained by this build")
    if not all(isinstance(m, torch.nn.Linear) for m in model.hidden):
        raise NotImplementedError("the mask trainer runs Linear hidden layers; got %s" % [type(m).__name__ for m in model.hidden])
    hidden = [int(l.out_features) for l in model.hidden]
    if not 1 <= len(hidden) <= MAX_HIDDEN:
        raise NotImplementedError("the mask trainer runs 1 .. %d hidden layers; got h_dim=%s" % (MAX_HIDDEN, hidden))
    spec = MaskSpec(int(model.hidden[0].in_features), int(model.output_layer.out_features), hidden)
    if not all(1 <= w <= MAX_DIM for w in [spec.x_dim, spec.y_dim] + hidden):
        raise NotImplementedError("layer widths must lie in [1, %d]; got x_dim=%d, h_dim=%s, y_dim=%d" % (MAX_DIM, spec.x_dim, hidden, spec.y_dim))
    return spec


def state_keys(n_hidden):
    """The trained tensors' state_dict keys in the trainer's tensor order (the reference's registration order)."""
    return sum([["hidden.%d.weight" % i, "hidden.%d.bias" % i] for i in range(n_hidden)], []) + ["output_layer.weight", "output_layer.bias"]


def state_shapes(spec):
    """The trained tensors' shapes in state_keys' order: what vaenmf_mask_trainer_tensor_shape reports, without the library."""
    widths = [spec.x_dim] + list(spec.hidden) + [spec.y_dim]
    return sum([[(o, i), (o,)] for i, o in zip(widths, widths[1:])], [])


def checkpoint_name(epoch, vloss):
    """training_wiener_filter.py:187."""
    return "Classifier_epoch_{:03d}_vloss_{:.6f}.pt".format(epoch, vloss)


def epoch_log_lines(epoch, train_loss, valid_loss):
    """The lines the script appends to output_epoch.log for one epoch (training_wiener_filter.py:154-184), trailing blanks
    included."""
    return ["Epoch: {}".format(epoch), "[Train]       Loss: {:.6f}    ".format(train_loss), "[Validation] Loss: {:.6f}    ".format(valid_loss)]


class MaskTrainer:
    """model: a vaenmf.models.Classifier(batch_norm=False); its weights (nn.Linear's default draw, as the reference leaves
    them, or whatever it holds) are copied to the device.  loss: "mask" (mean_square_error_mask, the script's), "signal"
    (mean_square_error_signal with x = sqrt of the power frame) or "msa" (magnitude_spectrum_approxiamation_loss, labels
    |S|).  norm_eps: the eps of (x - mean) / (std + eps) when set_norm is given none."""

    def __init__(self, model, loss="mask", lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_batch=128, norm_eps=1e-8, device="cuda:0"):
        self.spec = mask_spec(model)
        if loss not in LOSSES:
            raise ValueError("loss=%r is not one of %s" % (loss, sorted(LOSSES)))
        if loss != "mask" and self.spec.y_dim != self.spec.x_dim:
            raise ValueError("the %s loss needs y_dim=%d == x_dim=%d" % (loss, self.spec.y_dim, self.spec.x_dim))
        if not 1 <= int(max_batch) <= MAX_BATCH:
            raise ValueError("max_batch=%d outside [1, %d]" % (max_batch, MAX_BATCH))
        self.loss, self.norm_eps = loss, float(norm_eps)
        self.keys = state_keys(len(self.spec.hidden))
        self.device, self.max_batch = torch.device(device), int(max_batch)
        hid = (C.c_int32 * 8)(*(list(self.spec.hidden) + [0] * 8)[:8])
        cfg = MaskTrainerConfig(self.spec.x_dim, self.spec.y_dim, len(self.spec.hidden), hid, LOSSES[loss], self.max_batch, float(lr),
                                float(betas[0]), float(betas[1]), float(eps))
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().vaenmf_mask_trainer_create(C.byref(cfg), C.byref(self._h)))
        self.shapes = []
        for i in range(lib().vaenmf_mask_trainer_num_tensors(self._h)):
            r, c = C.c_int32(), C.c_int32()
            check(lib().vaenmf_mask_trainer_tensor_shape(self._h, i, C.byref(r), C.byref(c)))
            self.shapes.append((r.value, c.value) if c.value else (r.value,))
        assert self.shapes == state_shapes(self.spec)
        self.load_state_dict(model.state_dict())
        self.data, self._norm = None, None
        self._out = torch.zeros(8, dtype=torch.float64, device=self.device)

    def close(self):
        if getattr(self, "_h", None):
            lib().vaenmf_mask_trainer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ parameters
    def _get(self, which):
        out = {}
        with torch.cuda.device(self.device):
            for i, (k, shp) in enumerate(zip(self.keys, self.shapes)):
                t = torch.empty(shp, dtype=torch.float32, device=self.device)
                check(lib().vaenmf_mask_trainer_get_tensor(self._h, which, i, _ptr(t), _stream()))
                out[k] = t
        return {k: v.cpu() for k, v in out.items()}

    def _set(self, which, tensors):
        with torch.cuda.device(self.device):
            for i, (k, shp) in enumerate(zip(self.keys, self.shapes)):
                v = torch.as_tensor(tensors[k]).detach()
                if tuple(v.shape) != tuple(shp):
                    raise ValueError("%s has shape %s, the model %s" % (k, tuple(v.shape), tuple(shp)))
                t = v.to(device=self.device, dtype=torch.float32).contiguous()
                check(lib().vaenmf_mask_trainer_set_tensor(self._h, which, i, _ptr(t), _stream()))
            torch.cuda.current_stream().synchronize()        # t is released when the loop moves on

    def state_dict(self):
        """The model's state_dict in the reference's key layout (CPU tensors)."""
        return self._get(MASK_PARAM)

    def gradients(self):
        """The gradients of the last step, under the parameters' keys."""
        return self._get(MASK_GRAD)

    def adam_state(self):
        return {"step": self.step_count, "exp_avg": self._get(MASK_ADAM_M), "exp_avg_sq": self._get(MASK_ADAM_V)}

    def load_state_dict(self, sd):
        missing = [k for k in self.keys if k not in sd]
        if missing:
            raise KeyError("state_dict lacks %s" % missing)
        self._set(MASK_PARAM, sd)

    def load_adam_state(self, state):
        """Resume: `state` as adam_state() returns it.  With load_state_dict before it, training goes on bit for bit as if it
        had not stopped."""
        step = check_adam_state(state, self.keys, self.shapes)
        self._set(MASK_ADAM_M, state["exp_avg"])
        self._set(MASK_ADAM_V, state["exp_avg_sq"])
        check(lib().vaenmf_mask_trainer_set_step_count(self._h, step))

    # ------------------------------------------------------------------ data
    def put(self, X, Y):
        """Power frames and labels on the device, once: X (x_dim, NT) and Y (y_dim, NT) host arrays as make_train_set returns
        them, or device tensors [NT, >= x_dim] / [NT, >= y_dim] as they are."""
        def rows(a, width, what):
            if isinstance(a, torch.Tensor) and a.is_cuda:
                t = a.to(torch.float32)
            else:
                t = torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float32).T)).to(self.device)
            if t.dim() != 2 or t.shape[1] < width:
                raise ValueError("%s must be [NT, >= %d] on the device ((%d, NT) on the host); got %s" % (what, width, width, tuple(t.shape)))
            return t.contiguous()
        if Y is None:
            raise ValueError("the mask trainer needs labels Y with a row per frame")
        Xd, Yd = rows(X, self.spec.x_dim, "X"), rows(Y, self.spec.y_dim, "Y")
        if Yd.shape[0] != Xd.shape[0]:
            raise ValueError("X has %d frames, Y %d" % (Xd.shape[0], Yd.shape[0]))
        return Data(Xd, Yd, int(Xd.shape[0]))

    def bind(self, X, Y=None):
        self.data = X if isinstance(X, Data) else self.put(X, Y)
        return self.data

    def set_norm(self, mean, std, eps=None):
        """The network's input becomes (x - mean) / (std + eps) (training_wiener_filter.py:122-126); mean, std (F, 1) or (F,).
        The losses go on weighing with the raw power."""
        if mean is None:
            self._norm = None
            check(lib().vaenmf_mask_trainer_set_norm(self._h, None, None, 0.0))
            return
        m = torch.as_tensor(np.asarray(mean, dtype=np.float32).reshape(-1)).to(self.device).contiguous()
        s = torch.as_tensor(np.asarray(std, dtype=np.float32).reshape(-1)).to(self.device).contiguous()
        if m.numel() != self.spec.x_dim or s.numel() != self.spec.x_dim:
            raise ValueError("mean / std must have x_dim=%d entries" % self.spec.x_dim)
        self._norm = (m, s)
        check(lib().vaenmf_mask_trainer_set_norm(self._h, _ptr(m), _ptr(s), self.norm_eps if eps is None else float(eps)))

    # ------------------------------------------------------------------ steps
    def _run(self, fn, data, idx, out):
        if data is None:
            raise ValueError("no data bound (MaskTrainer.bind)")
        if not (isinstance(idx, torch.Tensor) and idx.is_cuda and idx.dtype == torch.int32):
            idx = torch.as_tensor(np.asarray(idx, dtype=np.int32)).to(self.device)
        if idx.dim() != 1 or not 1 <= idx.numel() <= self.max_batch:
            raise ValueError("a batch is 1 .. max_batch=%d row indices; got %s" % (self.max_batch, tuple(idx.shape)))
        idx = idx.contiguous()
        out = self._out if out is None else out
        if not (out.is_cuda and out.dtype == torch.float64 and out.numel() == 8 and out.is_contiguous()):
            raise ValueError("out must be 8 contiguous float64 on the device")
        with torch.cuda.device(self.device):
            check(fn(self._h, _ptr(data.X), int(data.X.shape[1]), _ptr(data.Y), int(data.Y.shape[1]), data.NT, _ptr(idx), int(idx.numel()),
                     _ptr(out), _stream()))
        return out

    def step(self, idx, out=None):
        """One training step on rows idx of the bound data.  Returns the device buffer the step's results land in
        (vaenmf.train.read_losses: loss = recon, the rest zero); nothing synchronises."""
        return self._run(lib().vaenmf_mask_trainer_step, self.data, idx, out)

    def evaluate(self, idx, data=None, out=None):
        """Forward and loss only, on rows idx of `data` (MaskTrainer.put) or of the bound data; nothing is updated."""
        return self._run(lib().vaenmf_mask_trainer_eval, self.data if data is None else data, idx, out)

    @property
    def step_count(self):
        return int(lib().vaenmf_mask_trainer_step_count(self._h))


def fit_mask_filter(model, train_set, valid_set, model_dir, loss="mask", epochs=1, batch_size=128, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                    mean=None, std=None, std_norm=True, seed=0, device="cuda:0"):
    """scripts/training_wiener_filter.py:113-188 for `epochs` epochs (std_norm: the input is (x - mean) / (std + 1e-8), and
    trainset_mean.npy / trainset_std.npy go into model_dir).  train_set / valid_set: a TrainSet of
    dataset.make_train_set(labels="noisy_wiener_labels") or (X, Y[, mean, std]) with X, Y (F, NT); mean / std default to the
    training set's.  Returns (trainer, history); history[e]["checkpoint"] is the file written after epoch e + 1."""
    trainer = MaskTrainer(model, loss=loss, lr=lr, betas=betas, eps=eps, max_batch=batch_size, device=device)
    Xt, Yt, mt, st = _arrays(train_set, True)
    Xv, Yv, _, _ = _arrays(valid_set, True)
    os.makedirs(model_dir, exist_ok=True)
    if std_norm:
        mean, std = (mt if mean is None else mean), (st if std is None else std)
        if mean is None or std is None:
            raise ValueError("std_norm needs mean and std (a TrainSet carries them)")
        np.save(os.path.join(model_dir, "trainset_mean.npy"), np.asarray(mean))
        np.save(os.path.join(model_dir, "trainset_std.npy"), np.asarray(std))
        trainer.set_norm(mean, std, 1e-8)
    train, valid = trainer.put(Xt, Yt), trainer.put(Xv, Yv)
    log = os.path.join(model_dir, "output_epoch.log")
    open(log, "w").close()
    rng = np.random.default_rng(seed)
    tb, vb = batch_bounds(train.NT, batch_size), batch_bounds(valid.NT, batch_size)
    rows = torch.zeros(max(len(tb), len(vb)), 8, dtype=torch.float64, device=trainer.device)
    order = torch.arange(valid.NT, dtype=torch.int32, device=trainer.device)
    trainer.bind(train)
    history = []
    for epoch in range(1, epochs + 1):
        perm = torch.as_tensor(rng.permutation(train.NT).astype(np.int32)).to(trainer.device)      # shuffle=True
        for i, (lo, hi) in enumerate(tb):
            trainer.step(perm[lo:hi], out=rows[i])
        tr = float(np.mean(read_losses(rows[:len(tb)])["loss"]))          # total_loss / t, as the script
        for i, (lo, hi) in enumerate(vb):
            trainer.evaluate(order[lo:hi], data=valid, out=rows[i])
        va = float(np.mean(read_losses(rows[:len(vb)])["loss"]))
        with open(log, "a") as f:
            f.write("\n".join(epoch_log_lines(epoch, tr, va)) + "\n")
        path = os.path.join(model_dir, checkpoint_name(epoch, va))
        torch.save(trainer.state_dict(), path)
        history.append({"epoch": epoch, "train": {"loss": tr}, "valid": {"loss": va}, "checkpoint": path})
    return trainer, history
