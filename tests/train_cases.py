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

Case = collections.namedtuple("Case", "name kind x_dim y_dim z_dim hidden B seed")
GOLDEN_CASES = {
    "train_m1_f65": Case("train_m1_f65", "M1", 65, 0, 16, (128,), 33, 101),
    "train_m2_vad_f65": Case("train_m2_vad_f65", "M2", 65, 1, 32, (128, 128), 33, 102),
    "train_m2_ibm_f65": Case("train_m2_ibm_f65", "M2", 65, 65, 32, (128, 128), 33, 103),
    "train_clf_ibm_f65": Case("train_clf_ibm_f65", "Classifier", 65, 65, 0, (128, 128), 33, 104),
    "train_clf_vad_f65": Case("train_clf_vad_f65", "Classifier", 65, 1, 0, (128, 128), 33, 105),
}
SWEEP_B = (1, 15, 16, 17, 33, 128)


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


def make_data(case, steps=STEPS):
    """dict(X [POOL][x] float32, Y [POOL][y] float32 or None, idx [steps][B] int32, eps [steps][B][z] float32 or None,
    mean, std [x] float32 or None)."""
    rng = np.random.default_rng(case.seed)
    scale = np.exp(rng.normal(0.0, 1.0, (POOL, 1)) + rng.normal(0.0, 0.7, (1, case.x_dim)))
    X = (rng.exponential(1.0, (POOL, case.x_dim)) * scale).astype(np.float32)
    X[rng.random((POOL, case.x_dim)) < 0.02] = 0.0                       # silent bins: log(x + eps)
    d = {"X": X, "Y": None, "eps": None, "mean": None, "std": None}
    if case.kind != "M1":
        d["Y"] = (rng.random((POOL, case.y_dim)) < 0.4).astype(np.float32)
    d["idx"] = np.stack([rng.choice(POOL, case.B, replace=case.B > POOL) for _ in range(steps)]).astype(np.int32)
    if case.kind != "Classifier":
        d["eps"] = rng.standard_normal((steps, case.B, case.z_dim)).astype(np.float32)
    else:
        d["mean"] = X.mean(0).astype(np.float32)
        d["std"] = X.std(0, ddof=1).astype(np.float32)
    return d


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


Run = collections.namedtuple("Run", "losses counts grad1 final")


def run_steps(case, init, data, dtype, steps=STEPS, lr=1e-3, betas=(0.9, 0.999), adam_eps=1e-8):
    """`steps` training steps from the state `init`: Run(losses [steps][3] float64 (loss, recon, KL; classifier: loss, loss, 0),
    counts [steps][4] (tp, tn, fp, fn), grad1 {key: step-1 gradient}, final {key: parameter})."""
    keys = vaenmf.train.state_keys(case.kind, len(case.hidden))
    p = {k: torch.as_tensor(init[k]).detach().to(dtype).clone().requires_grad_(True) for k in keys}
    opt = torch.optim.Adam(list(p.values()), lr=lr, betas=betas, eps=adam_eps)
    t = lambda a: None if a is None else torch.as_tensor(a).to(dtype)
    X, Y, mean, std = t(data["X"]), t(data["Y"]), t(data["mean"]), t(data["std"])
    losses, counts, grad1 = np.zeros((steps, 3)), np.zeros((steps, 4), np.int64), None
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
    return Run(losses, counts, grad1, {k: v.detach().numpy() for k, v in p.items()})


_CACHE = {}


def reference_runs(case, steps=STEPS):
    """(init, data, float64 run, float32 run) of a case, computed once per process and shared; nobody writes into them."""
    key = (case, steps)
    if key not in _CACHE:
        init, data = state_of(make_model(case)), make_data(case, steps)
        _CACHE[key] = (init, data, run_steps(case, init, data, torch.float64, steps), run_steps(case, init, data, torch.float32, steps))
    return _CACHE[key]


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return {"losses": z["losses"], "counts": z["counts"], "grad1": {k[2:]: z[k] for k in z.files if k.startswith("g:")},
            "final": {k[2:]: z[k] for k in z.files if k.startswith("f:")}, "init_sha256": z["init_sha256"]}
