"""Shared by tests/test_train_mask_cpu.py and tests/test_gpu_train_mask.py: the cases of the mask trainer
(vaenmf.train_mask, csrc/train_mask.hip) and a torch restatement of its training step (scripts/training_wiener_filter.py:
113-146): the forward of vaenmf.models.Classifier written out over a parameter dict (relu(h W^T + b) per hidden layer, then the
sigmoid; vaenmf.models.Classifier itself draws the initial weights, and tests/test_train_mask_cpu.py holds the written-out
forward to Classifier.forward), the three MSE losses of python/models/utils.py:93-104 written from their formulas, autograd
and torch.optim.Adam, in float64 (the checker) or float32 (the yardstick: what the reference's own arithmetic leaves).  The
pattern is tests/train_cases.py's.

A case is built from its seed alone: initial weights are nn.Linear's default draws under torch.manual_seed(seed), frames are
exponential power-spectrum bins with exact zeros among them, labels are masks in [0, 1] (msa: magnitudes below sqrt(P)),
batches are rows of a small pool through an index table: 19 batches of 32 and a last one of 17.

The tolerance rule is tests/test_gpu_train.py's: a GPU error against the float64 run may be at most FACTOR = 8 times the
float32 run's error against float64, per tensor group; a recorded reference run may be within 4 yardsticks of float64."""
import collections
import os

import numpy as np
import torch

import vaenmf
from vaenmf import train_mask as vm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_FILE = os.path.join(GOLDEN, "train_mask_f65.npz")
FACTOR, GOLDEN_FACTOR = 8.0, 4.0
POOL, NORM_EPS, SMALL_TENSOR = 96, 1e-8, 8
SCHED = (32,) * 19 + (17,)
STEPS = len(SCHED)
LOSS_NAMES = ("mask", "signal", "msa")

Case = collections.namedtuple("Case", "name x_dim hidden loss norm seed")
CASES = [
    Case("deep5_mask", 65, (16,) * 5, "mask", True, 301),
    Case("deep5_signal", 65, (16,) * 5, "signal", True, 302),
    Case("deep5_msa", 65, (16,) * 5, "msa", True, 303),
    Case("deep5_mask_plain", 65, (16,) * 5, "mask", False, 304),
    Case("deep5_msa_plain", 65, (16,) * 5, "msa", False, 305),
    Case("uneven_mask", 65, (24, 8, 40), "mask", True, 306),             # unequal widths: a leading dimension from the wrong layer shows
    Case("odd_mask", 37, (7, 13), "mask", True, 307),                    # nothing is a multiple of 4
    Case("wide_mask", 65, (128,), "mask", True, 308),
    Case("deep8_mask", 9, (8,) * 8, "mask", True, 309),                  # the deepest network the trainer holds
]
BY_NAME = {c.name: c for c in CASES}
# the golden run (tests/golden/make_train_mask_golden.py): the reference's Classifier([65, [16] * 5, 65]), 3 batches of 16
GOLDEN_SEED, GOLDEN_STEPS, GOLDEN_B = 401, 3, 16
# fit_mask_filter: utterances of vaenmf.synth at x_dim 65 (a window of 128 samples), two to train on, one to validate
FIT = dict(x_dim=65, hidden=(16,) * 5, wlen_sec=8e-3, n_samples=4000, train_utts=(0, 1), valid_utt=2, batch_size=64, epochs=2, seed=5)


def make_model(case, module=vaenmf):
    """The case's model with its initial weights; module: vaenmf or the reference's models module."""
    torch.manual_seed(case.seed)
    return module.Classifier([case.x_dim, list(case.hidden), case.x_dim])


def state_of(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def make_pool(rng, x_dim, n):
    """(X [n][x] power frames, Y [n][x] masks in [0, 1], S [n][x] magnitudes below sqrt(X)), float32."""
    scale = np.exp(rng.normal(0.0, 1.0, (n, 1)) + rng.normal(0.0, 0.7, (1, x_dim)))
    X = (rng.exponential(1.0, (n, x_dim)) * scale).astype(np.float32)
    X[rng.random((n, x_dim)) < 0.02] = 0.0                               # silent bins: sqrt(0), and a weight of zero
    Y = rng.random((n, x_dim)).astype(np.float32)
    Y[rng.random((n, x_dim)) < 0.05] = 0.0
    Y[rng.random((n, x_dim)) < 0.05] = 1.0
    return X, Y, (np.sqrt(X.astype(np.float64)) * Y).astype(np.float32)


def make_data(case):
    """dict(X [POOL][x], Y [POOL][x] (the labels of the case's loss), idx: list of per-step int32 arrays, mean, std or None)."""
    rng = np.random.default_rng(case.seed)
    X, Y, S = make_pool(rng, case.x_dim, POOL)
    d = {"X": X, "Y": S if case.loss == "msa" else Y, "idx": [rng.choice(POOL, b, replace=False).astype(np.int32) for b in SCHED],
         "mean": None, "std": None}
    if case.norm:
        d["mean"], d["std"] = X.mean(0).astype(np.float32), X.std(0, ddof=1).astype(np.float32)
    return d


def groups(case):
    """[(label, [keys])]: what the whole-step tests compare as one vector.  A tensor each, except where a case has a tensor of
    fewer than SMALL_TENSOR = 8 elements (odd_mask: a bias of 7), whose float32 yardstick is a few rounding events and not a
    statistic: there a layer's weight and bias are one concatenated vector (tests/train_cases.py: groups)."""
    keys = vm.state_keys(len(case.hidden))
    shapes = vm.state_shapes(vm.MaskSpec(case.x_dim, case.x_dim, list(case.hidden)))
    if min(int(np.prod(s)) for s in shapes) < SMALL_TENSOR:
        return [(w[:-len(".weight")], [w, b]) for w, b in zip(keys[0::2], keys[1::2])]
    return [(k, [k]) for k in keys]


def cat(tensors, keys):
    return np.concatenate([np.asarray(tensors[k], np.float64).ravel() for k in keys])


# ---- the restatement ---------------------------------------------------------------------------------------------
def forward(p, n_hidden, x, mean=None, std=None):
    """y_hat of the parameter dict p on the power rows x."""
    h = (x - mean) / (std + NORM_EPS) if mean is not None else x
    for i in range(n_hidden):
        h = torch.relu(h @ p["hidden.%d.weight" % i].T + p["hidden.%d.bias" % i])
    return torch.sigmoid(h @ p["output_layer.weight"].T + p["output_layer.bias"])


def mse_loss(loss, yh, y, x):
    """python/models/utils.py:93-104 with x = sqrt of the power rows (training_wiener_filter.py:130-132)."""
    if loss == "mask":
        return torch.mean(torch.sum((y - yh) ** 2, dim=-1))
    xs = torch.sqrt(x)
    if loss == "signal":
        return torch.mean(torch.sum(((y - yh) * xs) ** 2, dim=-1))
    return torch.mean(torch.sum((y - yh * xs) ** 2, dim=-1))


Run = collections.namedtuple("Run", "losses grad1 final")


def run_steps(loss, n_hidden, init, data, dtype, lr=1e-3, betas=(0.9, 0.999), adam_eps=1e-8):
    """One training step per entry of data["idx"] from the state `init`: Run(losses [steps] float64, grad1 {key: step-1
    gradient}, final {key: parameter})."""
    keys = vm.state_keys(n_hidden)
    p = {k: torch.as_tensor(init[k]).detach().to(dtype).clone().requires_grad_(True) for k in keys}
    opt = torch.optim.Adam(list(p.values()), lr=lr, betas=betas, eps=adam_eps)
    t = lambda a: None if a is None else torch.as_tensor(a).to(dtype)
    X, Y, mean, std = t(data["X"]), t(data["Y"]), t(data["mean"]), t(data["std"])
    losses, grad1 = np.zeros(len(data["idx"])), None
    for s, rows in enumerate(data["idx"]):
        idx = torch.as_tensor(np.asarray(rows).astype(np.int64))
        l = mse_loss(loss, forward(p, n_hidden, X[idx], mean, std), Y[idx], X[idx])
        losses[s] = l.item()
        opt.zero_grad()
        l.backward()
        if s == 0:
            grad1 = {k: v.grad.detach().clone().numpy() for k, v in p.items()}
        opt.step()
    return Run(losses, grad1, {k: v.detach().numpy() for k, v in p.items()})


_CACHE = {}


def reference_runs(case):
    """(init, data, float64 run, float32 run) of a case, computed once per process and shared; nobody writes into them."""
    if case not in _CACHE:
        init, data = state_of(make_model(case)), make_data(case)
        _CACHE[case] = (init, data, run_steps(case.loss, len(case.hidden), init, data, torch.float64),
                        run_steps(case.loss, len(case.hidden), init, data, torch.float32))
    return _CACHE[case]


def loss_err(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


# ---- the golden run ----------------------------------------------------------------------------------------------
def golden_draw():
    """What tests/golden/make_train_mask_golden.py feeds the reference: dict(X [3][16][65], Y, S, mean, std [65])."""
    rng = np.random.default_rng(GOLDEN_SEED)
    X, Y, S = make_pool(rng, 65, GOLDEN_STEPS * GOLDEN_B)
    shp = (GOLDEN_STEPS, GOLDEN_B, 65)
    return {"X": X.reshape(shp), "Y": Y.reshape(shp), "S": S.reshape(shp), "mean": X.mean(0).astype(np.float32), "std": X.std(0, ddof=1).astype(np.float32)}


def load_golden():
    """dict(init {key: tensor}, data {loss: data dict of run_steps}, losses {loss: [3]}, final {loss: {key: array}})."""
    z = np.load(GOLDEN_FILE, allow_pickle=False)
    flat = lambda a: np.ascontiguousarray(a.reshape(-1, a.shape[-1]))
    idx = [np.arange(s * GOLDEN_B, (s + 1) * GOLDEN_B, dtype=np.int32) for s in range(GOLDEN_STEPS)]
    g = {"init": {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("i:")}, "data": {}, "losses": {}, "final": {}}
    for loss in LOSS_NAMES:
        g["data"][loss] = {"X": flat(z["X"]), "Y": flat(z["S"] if loss == "msa" else z["Y"]), "idx": idx, "mean": z["mean"], "std": z["std"]}
        g["losses"][loss] = z["losses:" + loss]
        g["final"][loss] = {k[len(loss) + 3:]: z[k] for k in z.files if k.startswith("f:%s:" % loss)}
    return g


def golden_runs(loss):
    """(golden, float64 run, float32 run) of the recorded batches from the recorded state, once per process."""
    key = ("golden", loss)
    if key not in _CACHE:
        g = load_golden()
        _CACHE[key] = (g, run_steps(loss, 5, g["init"], g["data"][loss], torch.float64), run_steps(loss, 5, g["init"], g["data"][loss], torch.float32))
    return _CACHE[key]


GOLDEN_CASE = Case("golden", 65, (16,) * 5, "mask", True, GOLDEN_SEED)


# ---- fit_mask_filter ---------------------------------------------------------------------------------------------
def fit_frames():
    """The data of the fit test, made on the host: dict(Xt, Yt (65, NT) power frames and ideal Wiener masks of the training
    utterances, Xv, Yv of the validation utterance, mean, std (65, 1) of Xt, wav: the validation mixture), once per process."""
    if "fit" not in _CACHE:
        import vaenmf_oracle as orc
        from vaenmf.synth import synth_utterance

        def one(u):
            s, n, x, _ = synth_utterance(u, FIT["n_samples"])
            Sx, Nx, Xx = (orc.stft(v.astype(np.float32), fs=16000, wlen_sec=FIT["wlen_sec"], hop_percent=0.25) for v in (s, n, x))
            ps, pn = np.abs(Sx).astype(np.float64) ** 2, np.abs(Nx).astype(np.float64) ** 2
            return (np.abs(Xx) ** 2).astype(np.float32), (ps / (ps + pn + 1e-8)).astype(np.float32), x.astype(np.float32)
        tr = [one(u) for u in FIT["train_utts"]]
        va = one(FIT["valid_utt"])
        Xt = np.concatenate([t[0] for t in tr], 1)
        _CACHE["fit"] = {"Xt": Xt, "Yt": np.concatenate([t[1] for t in tr], 1), "Xv": va[0], "Yv": va[1], "wav": va[2],
                         "mean": Xt.mean(1, keepdims=True).astype(np.float32), "std": Xt.std(1, ddof=1, keepdims=True).astype(np.float32)}
    return _CACHE["fit"]


def fit_model():
    torch.manual_seed(FIT["seed"])
    return vaenmf.Classifier([FIT["x_dim"], list(FIT["hidden"]), FIT["x_dim"]])


def fit_restatement(dtype=torch.float64):
    """fit_mask_filter's loop in torch on the host: [(train loss, validation loss)] per epoch, the permutations being those
    fit_mask_filter draws from its seed."""
    f, bs = fit_frames(), FIT["batch_size"]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a.T)).to(dtype)
    Xt, Yt, Xv, Yv = t(f["Xt"]), t(f["Yt"]), t(f["Xv"]), t(f["Yv"])
    mean, std = torch.as_tensor(f["mean"].reshape(-1)).to(dtype), torch.as_tensor(f["std"].reshape(-1)).to(dtype)
    n = len(FIT["hidden"])
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in state_of(fit_model()).items()}
    opt = torch.optim.Adam(list(p.values()), lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    rng = np.random.default_rng(FIT["seed"])
    out = []
    for _ in range(FIT["epochs"]):
        perm = torch.as_tensor(rng.permutation(Xt.shape[0]).astype(np.int64))
        tl = []
        for lo in range(0, Xt.shape[0], bs):
            idx = perm[lo:lo + bs]
            l = mse_loss("mask", forward(p, n, Xt[idx], mean, std), Yt[idx], Xt[idx])
            tl.append(l.item())
            opt.zero_grad()
            l.backward()
            opt.step()
        with torch.no_grad():
            vl = [mse_loss("mask", forward(p, n, Xv[lo:lo + bs], mean, std), Yv[lo:lo + bs], Xv[lo:lo + bs]).item() for lo in range(0, Xv.shape[0], bs)]
        out.append((float(np.mean(tl)), float(np.mean(vl))))
    return out
