"""Training on the GPU: the build's counterpart of the reference's scripts/training_M1.py, training_M2.py and
training_classifier.py (csrc/train.hip; include/vaenmf.h states the arithmetic).

  Trainer         a vaenmf.models module's parameters, gradients and Adam state on the device and the step that updates them:
                  gather, dense layers forward and backward in fp32 on the matrix pipe, ELBO / BCE head, torch.optim.Adam
  fit_m1, fit_m2, fit_classifier
                  the loops of the three scripts: a fresh permutation per epoch, a short last batch, per-epoch means in
                  output_epoch.log, checkpoints under the reference's names

The checkpoints are state_dicts in the reference's key layout: they load with strict=True into vaenmf.models and go as
they are into pipeline.Reconstructor and engine.classifier_layers_from_state.

There is no CPU fallback: a Trainer needs the HIP library and a GPU.  Host-only (no library): model_spec, state_keys,
state_shapes, check_adam_state, checkpoint_name, batch_bounds, epoch_log_lines.

Not built: Classifier(batch_norm=True), Classifier2Classes, the MSE losses of training_wiener_filter.py, U_loss, the HDF5
loader, data-parallel training -- NotImplementedError where reachable.  (The Wiener-mask baseline with its MSE losses and
deeper classifiers is trained by vaenmf.train_mask: MaskTrainer, fit_mask_filter.)"""
import collections
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from . import models as vmodels
from ._lib import check, lib

Spec = collections.namedtuple("Spec", "kind x_dim y_dim z_dim hidden")
KINDS = {"M1": _lib.TRAIN_M1, "M2": _lib.TRAIN_M2, "Classifier": _lib.TRAIN_CLASSIFIER}
LOSS_FIELDS = ("loss", "recon", "kl", "_", "tp", "tn", "fp", "fn")
MAX_DIM, MAX_BATCH = 4096, 65536


def model_spec(model):
    """Spec(kind, x_dim, y_dim, z_dim, hidden) of a vaenmf.models module, or NotImplementedError for what the trainer does
    not run.  Pure: needs neither the library nor a GPU."""
    if isinstance(model, vmodels.Classifier2Classes):
        raise NotImplementedError("Classifier2Classes is not trained by this build")
    if isinstance(model, vmodels.Classifier):
        if any(isinstance(m, torch.nn.BatchNorm1d) for m in model.hidden):
            raise NotImplementedError("Classifier(batch_norm=True) is not trained by this build")
        hidden = [int(l.out_features) for l in model.hidden]
        spec = Spec("Classifier", int(model.hidden[0].in_features), int(model.output_layer.out_features), 0, hidden)
    elif isinstance(model, vmodels.VariationalAutoencoder):
        m2 = isinstance(model, vmodels.DeepGenerativeModel)
        y_dim = int(model.y_dim) if m2 else 0
        hidden = [int(l.out_features) for l in model.encoder.hidden]
        spec = Spec("M2" if m2 else "M1", int(model.encoder.hidden[0].in_features) - y_dim, y_dim, int(model.z_dim), hidden)
    else:
        raise NotImplementedError("the trainer runs VariationalAutoencoder, DeepGenerativeModel and Classifier; got %s" % type(model).__name__)
    check_spec(spec)
    return spec


def check_spec(spec):
    """The shapes vaenmf_trainer_create accepts (it refuses the rest itself; this says so without a GPU)."""
    if len(spec.hidden) not in (1, 2):
        raise NotImplementedError("the trainer runs one or two hidden layers; got h_dim=%s" % (list(spec.hidden),))
    if not all(1 <= h <= MAX_DIM for h in spec.hidden) or not 1 <= spec.x_dim <= MAX_DIM:
        raise NotImplementedError("layer widths must lie in [1, %d]; got x_dim=%d, h_dim=%s" % (MAX_DIM, spec.x_dim, list(spec.hidden)))
    if spec.kind == "M1" and spec.y_dim != 0:
        raise NotImplementedError("M1 has no labels")
    if spec.kind != "M1" and not 1 <= spec.y_dim <= MAX_DIM - spec.x_dim:
        raise NotImplementedError("y_dim must lie in [1, %d]; got %d" % (MAX_DIM - spec.x_dim, spec.y_dim))
    if spec.kind != "Classifier" and (spec.z_dim < 4 or spec.z_dim % 4 or spec.z_dim > 1024):
        raise NotImplementedError("z_dim must be a multiple of 4 in [4, 1024]; got %d" % spec.z_dim)


def state_keys(kind, n_hidden):
    """The trained tensors' state_dict keys in the trainer's tensor order (the reference's registration order)."""
    wb = lambda p: [p + ".weight", p + ".bias"]
    if kind == "Classifier":
        return sum([wb("hidden.%d" % i) for i in range(n_hidden)], []) + wb("output_layer")
    return (sum([wb("encoder.hidden.%d" % i) for i in range(n_hidden)], []) + wb("encoder.sample.mu") + wb("encoder.sample.log_var") +
            sum([wb("decoder.hidden.%d" % i) for i in range(n_hidden)], []) + wb("decoder.reconstruction"))


def state_shapes(spec):
    """The trained tensors' shapes in state_keys' order: what vaenmf_trainer_tensor_shape reports, without the library."""
    wb = lambda out, n_in: [(out, n_in), (out,)]
    h = list(spec.hidden)
    if spec.kind == "Classifier":
        widths = [spec.x_dim] + h + [spec.y_dim]
        return sum([wb(o, i) for i, o in zip(widths, widths[1:])], [])
    enc, dec = [spec.x_dim + spec.y_dim] + h, [spec.z_dim + spec.y_dim] + h[::-1] + [spec.x_dim]
    return (sum([wb(o, i) for i, o in zip(enc, enc[1:])], []) + 2 * wb(spec.z_dim, enc[-1]) +
            sum([wb(o, i) for i, o in zip(dec, dec[1:])], []))


def check_adam_state(state, keys, shapes):
    """What Trainer.load_adam_state takes: dict(step, exp_avg, exp_avg_sq) as Trainer.adam_state returns it, the two moment
    dicts with exactly the trained tensors' keys and shapes, step in [0, 2^31 - 1).  Returns the step.  Pure."""
    if not isinstance(state, dict) or set(state) != {"step", "exp_avg", "exp_avg_sq"}:
        got = sorted(state, key=str) if isinstance(state, dict) else type(state).__name__
        raise KeyError("an Adam state is dict(step, exp_avg, exp_avg_sq); got %s" % (got,))
    step = state["step"]
    try:
        whole = not isinstance(step, bool) and int(step) == step and 0 <= int(step) < 2 ** 31 - 1
    except (TypeError, ValueError, OverflowError):
        whole = False
    if not whole:
        raise ValueError("step=%r is not a whole number in [0, 2^31 - 1)" % (step,))
    for name in ("exp_avg", "exp_avg_sq"):
        if not isinstance(state[name], dict) or set(state[name]) != set(keys):
            raise KeyError("%s must hold exactly the trained tensors %s" % (name, list(keys)))
        for k, shp in zip(keys, shapes):
            got = tuple(np.shape(state[name][k]))          # a tensor, an array or nested lists
            if got != tuple(shp):
                raise ValueError("%s[%s] has shape %s, the model %s" % (name, k, got, tuple(shp)))
    return int(step)


def checkpoint_name(kind, epoch, vloss):
    """training_M1.py:143, training_M2.py:168, training_classifier.py:215."""
    if kind == "Classifier":
        return "Classifier_epoch_{:03d}_vloss_{:.3f}.pt".format(epoch, vloss)
    return "{}_epoch_{:03d}_vloss_{:.2f}.pt".format(kind, epoch, vloss)


def batch_bounds(n, batch_size):
    """[(lo, hi)] of the batches of n rows: drop_last=False, so the last one may be short."""
    if n < 1 or batch_size < 1:
        raise ValueError("n=%d rows in batches of %d" % (n, batch_size))
    return [(lo, min(lo + batch_size, n)) for lo in range(0, n, batch_size)]


def f1_from_counts(tp, tn, fp, fn, eps=1e-8):
    """training_classifier.py:166-168."""
    precision, recall = tp / (tp + fp + eps), tp / (tp + fn + eps)
    return 2 * (precision * recall) / (precision + recall + eps)


def epoch_log_lines(kind, epoch, train, valid):
    """The lines the scripts append to output_epoch.log for one epoch; train / valid: dicts of the epoch's means."""
    if kind == "Classifier":
        return ["Epoch: {}".format(epoch),
                "[Train]       Loss: {:.2f}    F1_score: {:.2f}".format(train["loss"], train["f1"]),
                "[Validation] Loss: {:.2f}    F1_score: {:.2f}".format(valid["loss"], valid["f1"])]
    return ["Epoch: {}".format(epoch),
            "[Train]\t\t ELBO: {:.2f}, Recon.: {:.2f}, KL: {:.2f}".format(train["loss"], train["recon"], train["kl"]),
            "[Validation]\t ELBO: {:.2f}, Recon.: {:.2f}, KL: {:.2f}".format(valid["loss"], valid["recon"], valid["kl"])]


def _ptr(t):
    if t is None:
        return None
    if not t.is_contiguous():
        raise ValueError("the C ABI takes dense row-major buffers; got strides %s" % (tuple(t.stride()),))
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


Data = collections.namedtuple("Data", "X Y NT")


class Trainer:
    """model: a vaenmf.models VariationalAutoencoder, DeepGenerativeModel or Classifier(batch_norm=False); its weights (xavier
    as the reference draws them, or whatever it holds) are copied to the device.  seed: of the reparameterisation draws a
    step makes on the device when it is given none."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_batch=128, seed=0, loss_eps=1e-8, device="cuda:0"):
        self.spec = model_spec(model)
        if not 1 <= int(max_batch) <= MAX_BATCH:
            raise ValueError("max_batch=%d outside [1, %d]" % (max_batch, MAX_BATCH))
        self.keys = state_keys(self.spec.kind, len(self.spec.hidden))
        self.device, self.seed, self.max_batch = torch.device(device), int(seed), int(max_batch)
        sd = model.state_dict()
        self._extra = {k: v.detach().clone() for k, v in sd.items() if k not in self.keys}      # M2: classifier.* as it came
        hid = (C.c_int32 * 2)(*(list(self.spec.hidden) + [0])[:2])
        cfg = _lib.TrainerConfig(KINDS[self.spec.kind], self.spec.x_dim, self.spec.y_dim, self.spec.z_dim, len(self.spec.hidden), hid,
                                 self.max_batch, float(lr), float(betas[0]), float(betas[1]), float(eps), float(loss_eps))
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().vaenmf_trainer_create(C.byref(cfg), C.byref(self._h)))
        self.shapes = []
        for i in range(lib().vaenmf_trainer_num_tensors(self._h)):
            r, c = C.c_int32(), C.c_int32()
            check(lib().vaenmf_trainer_tensor_shape(self._h, i, C.byref(r), C.byref(c)))
            self.shapes.append((r.value, c.value) if c.value else (r.value,))
        assert len(self.shapes) == len(self.keys)
        self.load_state_dict(sd)
        self.data, self._norm = None, None
        self._out = torch.zeros(8, dtype=torch.float64, device=self.device)

    def close(self):
        if getattr(self, "_h", None):
            lib().vaenmf_trainer_destroy(self._h)
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
                check(lib().vaenmf_trainer_get_tensor(self._h, which, i, _ptr(t), _stream()))
                out[k] = t
        return {k: v.cpu() for k, v in out.items()}

    def state_dict(self):
        """The model's state_dict in the reference's key layout (CPU tensors)."""
        sd = self._get(_lib.TRAIN_PARAM)
        sd.update({k: v.clone() for k, v in self._extra.items()})
        return sd

    def gradients(self):
        """The gradients of the last step, under the parameters' keys."""
        return self._get(_lib.TRAIN_GRAD)

    def adam_state(self):
        return {"step": int(lib().vaenmf_trainer_step_count(self._h)), "exp_avg": self._get(_lib.TRAIN_ADAM_M),
                "exp_avg_sq": self._get(_lib.TRAIN_ADAM_V)}

    def load_state_dict(self, sd):
        missing = [k for k in self.keys if k not in sd]
        if missing:
            raise KeyError("state_dict lacks %s" % missing)
        self._set(_lib.TRAIN_PARAM, sd)

    def _set(self, which, tensors):
        with torch.cuda.device(self.device):
            for i, (k, shp) in enumerate(zip(self.keys, self.shapes)):
                v = torch.as_tensor(tensors[k]).detach()
                if tuple(v.shape) != tuple(shp):
                    raise ValueError("%s has shape %s, the model %s" % (k, tuple(v.shape), tuple(shp)))
                t = v.to(device=self.device, dtype=torch.float32).contiguous()
                check(lib().vaenmf_trainer_set_tensor(self._h, which, i, _ptr(t), _stream()))
            torch.cuda.current_stream().synchronize()        # t is released when the loop moves on

    def load_adam_state(self, state):
        """Resume: `state` as adam_state() returns it.  Writes Adam's m and v and sets the step count, which is Adam's t and
        the key of the draws the next steps make on the device; with load_state_dict before it, training goes on bit for
        bit as if it had not stopped."""
        step = check_adam_state(state, self.keys, self.shapes)
        self._set(_lib.TRAIN_ADAM_M, state["exp_avg"])
        self._set(_lib.TRAIN_ADAM_V, state["exp_avg_sq"])
        check(lib().vaenmf_trainer_set_step_count(self._h, step))

    # ------------------------------------------------------------------ data
    def put(self, X, Y=None):
        """Frames (and labels) on the device, once: X (F, NT) and Y (y_dim, NT) host arrays as the reference's pickles hold
        them, or device tensors [NT, F] / [NT, y_dim] as they are."""
        def rows(a, width, what):
            if a is None:
                return None
            if isinstance(a, torch.Tensor) and a.is_cuda:
                t = a.to(torch.float32)
            else:
                t = torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float32).T)).to(self.device)
            if t.dim() != 2 or t.shape[1] < width:
                raise ValueError("%s must be [NT, >= %d] on the device ((%d, NT) on the host); got %s" % (what, width, width, tuple(t.shape)))
            return t.contiguous()
        Xd = rows(X, self.spec.x_dim, "X")
        Yd = rows(Y, self.spec.y_dim, "Y") if self.spec.kind != "M1" else None
        if self.spec.kind != "M1" and (Yd is None or Yd.shape[0] != Xd.shape[0]):
            raise ValueError("this model needs labels Y with a row per frame")
        return Data(Xd, Yd, int(Xd.shape[0]))

    def bind(self, X, Y=None):
        self.data = X if isinstance(X, Data) else self.put(X, Y)
        return self.data

    def set_norm(self, mean, std, eps=1e-8):
        """The classifier's input becomes (x - mean) / (std + eps) (training_classifier.py:133-135); mean, std (F, 1) or (F,)."""
        if mean is None:
            self._norm = None
            check(lib().vaenmf_trainer_set_norm(self._h, None, None, 0.0))
            return
        m = torch.as_tensor(np.asarray(mean, dtype=np.float32).reshape(-1)).to(self.device).contiguous()
        s = torch.as_tensor(np.asarray(std, dtype=np.float32).reshape(-1)).to(self.device).contiguous()
        if m.numel() != self.spec.x_dim or s.numel() != self.spec.x_dim:
            raise ValueError("mean / std must have x_dim=%d entries" % self.spec.x_dim)
        self._norm = (m, s)
        check(lib().vaenmf_trainer_set_norm(self._h, _ptr(m), _ptr(s), float(eps)))

    # ------------------------------------------------------------------ steps
    def _idx(self, idx):
        if not (isinstance(idx, torch.Tensor) and idx.is_cuda and idx.dtype == torch.int32):
            idx = torch.as_tensor(np.asarray(idx, dtype=np.int32)).to(self.device)
        if idx.dim() != 1 or not 1 <= idx.numel() <= self.max_batch:
            raise ValueError("a batch is 1 .. max_batch=%d row indices; got %s" % (self.max_batch, tuple(idx.shape)))
        return idx.contiguous()

    def _run(self, fn, data, idx, eps, out):
        if data is None:
            raise ValueError("no data bound (Trainer.bind)")
        idx = self._idx(idx)
        B = int(idx.numel())
        if eps is not None:
            if self.spec.kind == "Classifier":
                raise ValueError("the classifier draws nothing")
            eps = torch.as_tensor(eps, dtype=torch.float32).to(self.device).contiguous()
            if tuple(eps.shape) != (B, self.spec.z_dim):
                raise ValueError("eps must be [B=%d, z_dim=%d]; got %s" % (B, self.spec.z_dim, tuple(eps.shape)))
        out = self._out if out is None else out
        if not (out.is_cuda and out.dtype == torch.float64 and out.numel() == 8 and out.is_contiguous()):
            raise ValueError("out must be 8 contiguous float64 on the device")
        with torch.cuda.device(self.device):
            check(fn(self._h, _ptr(data.X), int(data.X.shape[1]), _ptr(data.Y), int(data.Y.shape[1]) if data.Y is not None else 0,
                     data.NT, _ptr(idx), B, _ptr(eps), self.seed, _ptr(out), _stream()))
        return out

    def step(self, idx, eps=None, out=None):
        """One training step on rows idx of the bound data.  eps [B, z_dim]: the reparameterisation draws (replay); None: drawn
        on the device.  Returns the device buffer the step's results land in (see read_losses); nothing synchronises."""
        return self._run(lib().vaenmf_trainer_step, self.data, idx, eps, out)

    def evaluate(self, idx, eps=None, data=None, out=None):
        """Forward and loss only, on rows idx of `data` (Trainer.put) or of the bound data; nothing is updated."""
        return self._run(lib().vaenmf_trainer_eval, self.data if data is None else data, idx, eps, out)

    def eps_fill(self, step, B):
        """The draws device-mode step number `step` (the first is 1) makes for a batch of B rows."""
        out = torch.empty(B, self.spec.z_dim, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().vaenmf_trainer_eps_fill(self._h, int(step), int(B), self.seed, _ptr(out), _stream()))
        return out

    @property
    def step_count(self):
        return int(lib().vaenmf_trainer_step_count(self._h))


def read_losses(out):
    """dict(loss, recon, kl, tp, tn, fp, fn) of a step's result buffer (or of rows of them: arrays).  Synchronises."""
    o = out.detach().cpu().reshape(-1, 8)
    cnt = o[:, 4:].contiguous().view(torch.int64)
    d = {"loss": o[:, 0].numpy(), "recon": o[:, 1].numpy(), "kl": o[:, 2].numpy()}
    d.update({k: cnt[:, i].numpy() for i, k in enumerate(("tp", "tn", "fp", "fn"))})
    return {k: (v[0].item() if out.dim() == 1 else v) for k, v in d.items()}


def _arrays(ds, want_y):
    """(X, Y, mean, std) of a TrainSet or of (F, NT) arrays: X, (X, Y) or (X, Y, mean, std)."""
    if hasattr(ds, "X") and hasattr(ds, "Y"):
        return ds.X, (ds.Y if want_y else None), getattr(ds, "mean", None), getattr(ds, "std", None)
    if isinstance(ds, (tuple, list)):
        parts = list(ds) + [None] * (4 - len(ds))
        return parts[0], (parts[1] if want_y else None), parts[2], parts[3]
    if isinstance(ds, str) and ds.endswith((".h5", ".hdf5")):
        raise NotImplementedError("the HDF5 loader is not built: pass a TrainSet or (F, NT) arrays")
    return ds, None, None, None


def _epoch_means(kind, rows, eps):
    r = read_losses(rows)
    m = {"loss": float(np.mean(r["loss"])), "recon": float(np.mean(r["recon"])), "kl": float(np.mean(r["kl"]))}     # total / t, as the scripts
    if kind == "Classifier":
        m["f1"] = float(f1_from_counts(float(r["tp"].sum()), float(r["tn"].sum()), float(r["fp"].sum()), float(r["fn"].sum()), eps))
    return m


def _fit(trainer, train, valid, epochs, batch_size, model_dir, seed):
    kind = trainer.spec.kind
    if batch_size > trainer.max_batch:
        raise ValueError("batch_size=%d exceeds the trainer's max_batch=%d" % (batch_size, trainer.max_batch))
    os.makedirs(model_dir, exist_ok=True)
    log = os.path.join(model_dir, "output_epoch.log")
    open(log, "w").close()
    rng = np.random.default_rng(seed)
    tb, vb = batch_bounds(train.NT, batch_size), batch_bounds(valid.NT, batch_size)
    rows = torch.zeros(max(len(tb), len(vb)), 8, dtype=torch.float64, device=trainer.device)
    order = torch.arange(valid.NT, dtype=torch.int32, device=trainer.device)
    trainer.bind(train)
    history, path = [], None
    for epoch in range(1, epochs + 1):
        perm = torch.as_tensor(rng.permutation(train.NT).astype(np.int32)).to(trainer.device)      # shuffle=True
        for i, (lo, hi) in enumerate(tb):
            trainer.step(perm[lo:hi], out=rows[i])
        tr = _epoch_means(kind, rows[:len(tb)], 1e-8)
        for i, (lo, hi) in enumerate(vb):
            trainer.evaluate(order[lo:hi], data=valid, out=rows[i])
        va = _epoch_means(kind, rows[:len(vb)], 1e-8)
        with open(log, "a") as f:
            f.write("\n".join(epoch_log_lines(kind, epoch, tr, va)) + "\n")
        path = os.path.join(model_dir, checkpoint_name(kind, epoch, va["loss"]))
        torch.save(trainer.state_dict(), path)
        history.append({"epoch": epoch, "train": tr, "valid": va, "checkpoint": path})
    return history


def _fit_vae(kind, model, train_set, valid_set, model_dir, epochs, batch_size, lr, betas, eps, seed, device):
    trainer = Trainer(model, lr=lr, betas=betas, eps=eps, max_batch=batch_size, seed=seed, device=device)
    if trainer.spec.kind != kind:
        raise ValueError("fit_%s takes a %s model; got %s" % (kind.lower(), kind, trainer.spec.kind))
    Xt, Yt, _, _ = _arrays(train_set, kind == "M2")
    Xv, Yv, _, _ = _arrays(valid_set, kind == "M2")
    history = _fit(trainer, trainer.put(Xt, Yt), trainer.put(Xv, Yv), epochs, batch_size, model_dir, seed)
    return trainer, history


def fit_m1(model, train_set, valid_set, model_dir, epochs=1, batch_size=128, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, seed=0, device="cuda:0"):
    """scripts/training_M1.py:84-145 for `epochs` epochs.  train_set / valid_set: a TrainSet or X (F, NT).  Returns (trainer,
    history); history[e]["checkpoint"] is the file written after epoch e + 1."""
    return _fit_vae("M1", model, train_set, valid_set, model_dir, epochs, batch_size, lr, betas, eps, seed, device)


def fit_m2(model, train_set, valid_set, model_dir, epochs=1, batch_size=128, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, seed=0, device="cuda:0"):
    """scripts/training_M2.py:108-169: the labelled ELBO of encoder([x | y]) / decoder([z | y]) (U_loss is not built).
    train_set / valid_set: a TrainSet or (X (F, NT), Y (y_dim, NT))."""
    return _fit_vae("M2", model, train_set, valid_set, model_dir, epochs, batch_size, lr, betas, eps, seed, device)


def fit_classifier(model, train_set, valid_set, model_dir, epochs=1, batch_size=128, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, seed=0,
                   mean=None, std=None, std_norm=True, device="cuda:0"):
    """scripts/training_classifier.py:125-216 (std_norm: the input is (x - mean) / (std + 1e-8), and trainset_mean.npy /
    trainset_std.npy go into model_dir).  train_set / valid_set: a TrainSet or (X, Y[, mean, std]); mean / std default to the
    training set's."""
    trainer = Trainer(model, lr=lr, betas=betas, eps=eps, max_batch=batch_size, seed=seed, device=device)
    if trainer.spec.kind != "Classifier":
        raise ValueError("fit_classifier takes a Classifier; got %s" % trainer.spec.kind)
    Xt, Yt, mt, st = _arrays(train_set, True)
    Xv, Yv, _, _ = _arrays(valid_set, True)
    if std_norm:
        mean, std = (mt if mean is None else mean), (st if std is None else std)
        if mean is None or std is None:
            raise ValueError("std_norm needs mean and std (a TrainSet carries them)")
        os.makedirs(model_dir, exist_ok=True)
        np.save(os.path.join(model_dir, "trainset_mean.npy"), np.asarray(mean))
        np.save(os.path.join(model_dir, "trainset_std.npy"), np.asarray(std))
        trainer.set_norm(mean, std, 1e-8)
    history = _fit(trainer, trainer.put(Xt, Yt), trainer.put(Xv, Yv), epochs, batch_size, model_dir, seed)
    return trainer, history


def fit_wiener_filter(*args, **kwargs):
    raise NotImplementedError("the MSE losses of training_wiener_filter.py are not built")
