"""Shared cases of the training tests and a torch restatement of the three training steps (scripts/training_M1.py,
training_M2.py, training_classifier.py): forward, loss (python/models/utils.py: elbo, binary_cross_entropy), autograd and
torch.optim.Adam, in float64 (the checker) or float32 (the yardstick: what the reference's own arithmetic leaves).

A case is built from its seed alone: initial weights are vaenmf.models' xavier draws under torch.manual_seed(seed) (the
goldens check that the reference draws the same), frames are exponential power-spectrum bins with exact zeros among them,
labels are 0 / 1, batches are rows of a small pool through an index table, eps are the reparameterisation draws."""
import collections
import os

import numpy as np
import torch

import vaenmf

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STEPS, POOL, LOSS_EPS = 20, 96, 1e-8
SMALL_TENSOR = 8

Case = collections.namedtuple("Case", "name kind x_dim y_dim z_dim hidden B seed")
GOLDEN_CASES = {
    "train_m1_f65": Case("train_m1_f65", "M1", 65, 0, 16, (128,), 33, 101),
    "train_m2_vad_f65": Case("train_m2_vad_f65", "M2", 65, 1, 32, (128, 128), 33, 102),
    "train_m2_ibm_f65": Case("train_m2_ibm_f65", "M2", 65, 65, 32, (128, 128), 33, 103),
    "train_clf_ibm_f65": Case("train_clf_ibm_f65", "Classifier", 65, 65, 0, (128, 128), 33, 104),
    "train_clf_vad_f65": Case("train_clf_vad_f65", "Classifier", 65, 1, 0, (128, 128), 33, 105),
}
SWEEP_B = (1, 15, 16, 17, 33, 128)
# Unequal widths, none a multiple of 16 (m2_wide: the widest decoder the engine runs), so that exchanging the two hidden
# widths, a leading dimension from the wrong layer or a wrong [mu | logvar] offset changes numbers, and every product of a
# step leaves a remainder in its 32 x 64 x 64 tile.
SHAPE_CASES = {
    "m1_uneven": Case("m1_uneven", "M1", 67, 0, 20, (72, 40), 33, 201),
    "m2_uneven": Case("m2_uneven", "M2", 67, 3, 20, (72, 40), 33, 202),
    "clf_uneven": Case("clf_uneven", "Classifier", 67, 67, 0, (72, 40), 33, 203),
    "m2_wide": Case("m2_wide", "M2", 65, 65, 128, (256, 128), 17, 204),
    "m1_one_z4": Case("m1_one_z4", "M1", 67, 0, 4, (40,), 33, 205),
}
# The schedule form: B is a tuple of batch sizes, one per step (a long batch, a short one, one row, ... on one trainer of
# max_batch 128).  128 rows of a pool of 96 repeat some.  Evaluations run after the steps EVAL_AFTER on a second pool of
# EVAL_POOL rows in the batches EVAL_BATCHES.
SCHED = (128, 80, 1, 17, 128, 33, 15, 128, 16, 2) * 2
EVAL_AFTER, EVAL_POOL, EVAL_BATCHES = (2, 5, 10, 13, 17, 20), 50, ((0, 40), (40, 50))
SCHED_CASES = {k: SHAPE_CASES[k]._replace(name=k + "_sched", B=SCHED, seed=SHAPE_CASES[k].seed + 100) for k in ("m1_uneven", "m2_uneven", "clf_uneven")}


def sweep_case(kind, B):
    """The batch sweep's shapes.  The classifier is the y_dim 65 one: with y_dim 1 its output bias is ONE float, and the
    float32 yardstick of a one-element tensor is a single rounding event, not a statistic (it came out at 0.07 ulp for the
    batch of 15, against which the GPU's 1 ulp is a factor of 15).  The y_dim 1 shapes are held by the two golden cases."""
    base = {"M1": GOLDEN_CASES["train_m1_f65"], "M2": GOLDEN_CASES["train_m2_vad_f65"], "Classifier": GOLDEN_CASES["train_clf_ibm_f65"]}[kind]
    return base._replace(name="%s_B%d" % (kind, B), B=B, seed=base.seed + 1000 + B)


def make_model(case, module=vaenmf):
    """The case's model with its initial weights; module: vaenmf (vaenmf.models' classes) or the reference's models module."""
    torch.manual_seed(case.seed)
    h = list(case.hidden)
    if case.kind == "M1":
        return module.VariationalAutoencoder([case.x_dim, case.z_dim, h])
    if case.kind == "M2":
        return module.DeepGenerativeModel([case.x_dim, case.y_dim, case.z_dim, h], None)
    return module.Classifier([case.x_dim, h, case.y_dim])        # nn.Linear's default init, as the reference leaves it


def make_pool(rng, case, n):
    """(X [n][x] float32, Y [n][y] float32 or None): n frames and their labels from rng."""
    scale = np.exp(rng.normal(0.0, 1.0, (n, 1)) + rng.normal(0.0, 0.7, (1, case.x_dim)))
    X = (rng.exponential(1.0, (n, case.x_dim)) * scale).astype(np.float32)
    X[rng.random((n, case.x_dim)) < 0.02] = 0.0                          # silent bins: log(x + eps)
    return X, ((rng.random((n, case.y_dim)) < 0.4).astype(np.float32) if case.kind != "M1" else None)


def make_data(case, steps=STEPS):
    """dict(X [POOL][x] float32, Y [POOL][y] float32 or None, idx [steps][B] int32, eps [steps][B][z] float32 or None,
    mean, std [x] float32 or None).  With a schedule (case.B a tuple of `steps` batch sizes) idx and eps are lists of
    per-step arrays [B_s] and [B_s][z]; a constant schedule gives the arrays of the plain case, row for row."""
    rng = np.random.default_rng(case.seed)
    X, Y = make_pool(rng, case, POOL)
    d = {"X": X, "Y": Y, "eps": None, "mean": None, "std": None}
    if isinstance(case.B, tuple):
        assert len(case.B) == steps, "a schedule names one batch size per step"
        d["idx"] = [rng.choice(POOL, b, replace=b > POOL).astype(np.int32) for b in case.B]
        if case.kind != "Classifier":
            d["eps"] = [rng.standard_normal((b, case.z_dim)).astype(np.float32) for b in case.B]
    else:
        d["idx"] = np.stack([rng.choice(POOL, case.B, replace=case.B > POOL) for _ in range(steps)]).astype(np.int32)
        if case.kind != "Classifier":
            d["eps"] = rng.standard_normal((steps, case.B, case.z_dim)).astype(np.float32)
    if case.kind == "Classifier":
        d["mean"] = X.mean(0).astype(np.float32)
        d["std"] = X.std(0, ddof=1).astype(np.float32)
    return d


def make_eval(case):
    """The evaluations of a scheduled run: dict(X [EVAL_POOL][x], Y or None, after: step numbers, batches: row index arrays,
    eps [len(after)][len(batches)] of [rows][z] or None).  A pool of its own with its own generator: make_data is as it was."""
    rng = np.random.default_rng(case.seed + 7000)
    X, Y = make_pool(rng, case, EVAL_POOL)
    batches = [np.arange(lo, hi, dtype=np.int32) for lo, hi in EVAL_BATCHES]
    eps = None
    if case.kind != "Classifier":
        eps = [[rng.standard_normal((len(b), case.z_dim)).astype(np.float32) for b in batches] for _ in EVAL_AFTER]
    return {"X": X, "Y": Y, "after": EVAL_AFTER, "batches": batches, "eps": eps}


def groups(case):
    """[(label, [keys])]: what the whole-step tests compare as one vector.  A tensor each, except where a case has tensors of
    a handful of elements (m1_one_z4: 4-element biases), whose float32 yardstick is a few rounding events and not a
    statistic (sweep_case): there a layer's weight and bias are one concatenated vector.  A handful: fewer than
    SMALL_TENSOR = 8 elements in the case's smallest tensor."""
    keys = vaenmf.train.state_keys(case.kind, len(case.hidden))
    shapes = vaenmf.train.state_shapes(vaenmf.train.Spec(case.kind, case.x_dim, case.y_dim, case.z_dim, list(case.hidden)))
    if min(int(np.prod(s)) for s in shapes) < SMALL_TENSOR:
        return [(w[:-len(".weight")], [w, b]) for w, b in zip(keys[0::2], keys[1::2])]
    return [(k, [k]) for k in keys]


def cat(tensors, keys):
    return np.concatenate([np.asarray(tensors[k], np.float64).ravel() for k in keys])


def state_of(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


# ---- the restatement ---------------------------------------------------------------------------------------------
def _mlp(p, prefix, n, x, act):
    for i in range(n):
        x = act(x @ p["%shidden.%d.weight" % (prefix, i)].T + p["%shidden.%d.bias" % (prefix, i)])
    return x


def forward_loss(case, p, x, y, eps, mean=None, std=None):
    """(loss, recon, KL) of the VAEs or (loss, y_hat) of the classifier from the parameter dict p, as the scripts compute them."""
    n = len(case.hidden)
    if case.kind == "Classifier":
        xn = (x - mean) / (std + LOSS_EPS) if mean is not None else x
        h = _mlp(p, "", n, xn, torch.relu)
        yh = torch.sigmoid(h @ p["output_layer.weight"].T + p["output_layer.bias"])
        loss = -torch.mean(torch.sum(y * torch.log(yh + LOSS_EPS) + (1 - y) * torch.log(1 - yh + LOSS_EPS), dim=-1))
        return loss, yh
    h = _mlp(p, "encoder.", n, torch.cat([x, y], 1) if case.kind == "M2" else x, torch.tanh)
    mu = h @ p["encoder.sample.mu.weight"].T + p["encoder.sample.mu.bias"]
    lv = h @ p["encoder.sample.log_var.weight"].T + p["encoder.sample.log_var.bias"]
    z = mu + torch.exp(0.5 * lv) * eps
    h = _mlp(p, "decoder.", n, torch.cat([z, y], 1) if case.kind == "M2" else z, torch.tanh)
    r = torch.exp(h @ p["decoder.reconstruction.weight"].T + p["decoder.reconstruction.bias"])
    recon = torch.mean(torch.sum(x / r - torch.log(x + LOSS_EPS) + torch.log(r) - 1, dim=-1))
    kl = -0.5 * torch.mean(torch.sum(lv - mu.pow(2) - lv.exp(), dim=-1))
    return recon + kl, recon, kl


Run = collections.namedtuple("Run", "losses counts grad1 final evals", defaults=(None,))


def run_steps(case, init, data, dtype, steps=STEPS, lr=1e-3, betas=(0.9, 0.999), adam_eps=1e-8, evals=None):
    """`steps` training steps from the state `init`: Run(losses [steps][3] float64 (loss, recon, KL; classifier: loss, loss, 0),
    counts [steps][4] (tp, tn, fp, fn), grad1 {key: step-1 gradient}, final {key: parameter}, evals).  data["idx"] and
    data["eps"] are [steps][B] arrays or lists of per-step arrays (a schedule).  evals (make_eval): after each step it names,
    forward and loss only, under no_grad, on each of its batches of its own pool -> Run.evals [len(after)][len(batches)][3]."""
    keys = vaenmf.train.state_keys(case.kind, len(case.hidden))
    p = {k: torch.as_tensor(init[k]).detach().to(dtype).clone().requires_grad_(True) for k in keys}
    opt = torch.optim.Adam(list(p.values()), lr=lr, betas=betas, eps=adam_eps)
    t = lambda a: None if a is None else torch.as_tensor(a).to(dtype)
    X, Y, mean, std = t(data["X"]), t(data["Y"]), t(data["mean"]), t(data["std"])
    losses, counts, grad1 = np.zeros((steps, 3)), np.zeros((steps, 4), np.int64), None
    ev = None
    if evals is not None:
        ev, EX, EY = np.zeros((len(evals["after"]), len(evals["batches"]), 3)), t(evals["X"]), t(evals["Y"])
    for s in range(steps):
        idx = torch.as_tensor(data["idx"][s].astype(np.int64))
        x, y = X[idx], (Y[idx] if Y is not None else None)
        if case.kind == "Classifier":
            loss, yh = forward_loss(case, p, x, y, None, mean, std)
            pred, lab = yh.detach() > 0.5, y > 0.5
            counts[s] = [int((pred & lab).sum()), int((~pred & ~lab).sum()), int((pred & ~lab).sum()), int((~pred & lab).sum())]
            losses[s] = [loss.item(), loss.item(), 0.0]
        else:
            loss, recon, kl = forward_loss(case, p, x, y, t(data["eps"][s]))
            losses[s] = [loss.item(), recon.item(), kl.item()]
        opt.zero_grad()
        loss.backward()
        if s == 0:
            grad1 = {k: v.grad.detach().clone().numpy() for k, v in p.items()}
        opt.step()
        if ev is not None and s + 1 in evals["after"]:
            a = evals["after"].index(s + 1)
            with torch.no_grad():
                for j, rows in enumerate(evals["batches"]):
                    r = torch.as_tensor(rows.astype(np.int64))
                    y = EY[r] if EY is not None else None
                    if case.kind == "Classifier":
                        l = forward_loss(case, p, EX[r], y, None, mean, std)[0].item()
                        ev[a, j] = [l, l, 0.0]
                    else:
                        ev[a, j] = [v.item() for v in forward_loss(case, p, EX[r], y, t(evals["eps"][a][j]))]
    return Run(losses, counts, grad1, {k: v.detach().numpy() for k, v in p.items()}, ev)


_CACHE = {}


def reference_runs(case, steps=STEPS):
    """(init, data, float64 run, float32 run) of a case, computed once per process and shared; nobody writes into them."""
    key = (case, steps)
    if key not in _CACHE:
        init, data = state_of(make_model(case)), make_data(case, steps)
        _CACHE[key] = (init, data, run_steps(case, init, data, torch.float64, steps), run_steps(case, init, data, torch.float32, steps))
    return _CACHE[key]


def scheduled_runs(case):
    """(init, data, evals, float64 run, float32 run) of a scheduled case with its evaluations, computed once per process."""
    key = (case, "sched")
    if key not in _CACHE:
        init, data, evals = state_of(make_model(case)), make_data(case, len(case.B)), make_eval(case)
        _CACHE[key] = (init, data, evals, run_steps(case, init, data, torch.float64, len(case.B), evals=evals),
                       run_steps(case, init, data, torch.float32, len(case.B), evals=evals))
    return _CACHE[key]


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return {"losses": z["losses"], "counts": z["counts"], "grad1": {k[2:]: z[k] for k in z.files if k.startswith("g:")},
            "final": {k[2:]: z[k] for k in z.files if k.startswith("f:")}, "init_sha256": z["init_sha256"]}
