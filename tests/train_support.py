"""Shared by tests/test_gpu_train.py and tests/test_gpu_train_shapes.py: the constants of their bounds (stated in the
docstring of tests/test_gpu_train.py), arena buffers and pointers for the kernel-level calls, one layer's three GEMM forms
against float64, and a whole training run on the GPU."""
import ctypes as C

import numpy as np
import torch

import train_cases as tc
from guarded import Arena
from vaenmf import _lib
from vaenmf._lib import check, lib

U = 2.0 ** -24
C_CHAIN = 1.5e-7
FACTOR = 8.0
DEV = "cuda:0"
ACTS = {"none": _lib.ACT_NONE, "tanh": _lib.ACT_TANH, "relu": _lib.ACT_RELU, "exp": _lib.ACT_EXP, "sigmoid": _lib.ACT_SIGMOID}


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def put(arena, name, host, ld=None):
    """A host matrix as an arena buffer with rows `ld` apart: the columns past its width stay poison.  Returns the buffer."""
    host = np.asarray(host)
    if host.ndim == 1 or ld is None or ld == host.shape[1]:
        t = arena.carve(name, host.shape, torch.from_numpy(host).dtype)
        t.copy_(torch.from_numpy(np.ascontiguousarray(host)))
        return t
    t = arena.carve(name, (host.shape[0], ld), torch.float32)
    t[:, :host.shape[1]].copy_(torch.from_numpy(np.ascontiguousarray(host)))
    return t


def out(arena, name, rows, cols, ld=None, dtype=torch.float32):
    return arena.carve(name, (rows, ld or cols) if cols else (rows,), dtype)


def padding_untouched(arena, t, cols):
    return t.dim() == 1 or t.shape[1] == cols or arena.is_poison(t[:, cols:])


# ---------------------------------------------------------------------------------------------------------------- GEMM
def _act64(name, v):
    return {"none": v, "tanh": np.tanh(v), "relu": np.maximum(v, 0.0), "exp": np.exp(v), "sigmoid": 1.0 / (1.0 + np.exp(-v))}[name]


def _act_tol(name, pre, tol_pre):
    val = np.abs(_act64(name, pre))
    if name in ("none", "relu"):
        return tol_pre
    if name == "tanh":
        return tol_pre + 4 * U * val
    if name == "sigmoid":
        return 0.25 * tol_pre + 4 * U * val
    return val * np.expm1(tol_pre) + 4 * U * val


def _saved_output(rng, name, shape):
    """A previous layer's saved activated output in the activation's range, zeros and saturated units among them."""
    v = rng.standard_normal(shape) * 1.5
    y = _act64(name, v).astype(np.float32)
    if name == "relu":
        y[rng.random(shape) < 0.2] = 0.0
    return y


def _deriv64(name, y):
    y = y.astype(np.float64)
    return {"none": np.ones_like(y), "tanh": 1 - y * y, "relu": (y > 0).astype(np.float64), "exp": y, "sigmoid": y * (1 - y)}[name]


def gemm_forms_case(rng, M, n_in, n_out, act, j, worst):
    """Forward, dX, dW and db of one layer shape against float64, each element within its bound from the operands; the
    largest error / bound of each form goes into `worst`.  (tests/test_gpu_train_shapes.py runs it at long reductions.)"""
    ldx, ldw, ldy, ldz, ldp = n_in + 3, n_in + (j % 3), n_out + 5, n_out + 1, n_in + 2
    X = rng.standard_normal((M, n_in)).astype(np.float32)
    W = (rng.standard_normal((n_out, n_in)) / np.sqrt(n_in)).astype(np.float32)
    b = (rng.standard_normal(n_out) * 0.3).astype(np.float32)
    dZ = rng.standard_normal((M, n_out)).astype(np.float32)
    dZ[rng.random((M, n_out)) < 0.05] = 0.0
    Yp = _saved_output(rng, act, (M, n_in))
    arena = Arena(8 << 20, "nan", device=DEV)
    dX_, dW_, db_ = put(arena, "X", X, ldx), put(arena, "W", W, ldw), put(arena, "b", b)
    dZ_, Yp_ = put(arena, "dZ", dZ, ldz), put(arena, "Yp", Yp, ldp)
    Y_ = out(arena, "Y", M, n_out, ldy)
    gX_ = out(arena, "gX", M, n_in, ldx)
    gW_ = out(arena, "gW", n_out, n_in, ldw)
    gb_ = out(arena, "gb", n_out, 0)
    arena.snapshot(["X", "W", "b", "dZ", "Yp"])
    check(lib().vaenmf_train_dense_fwd(p(dX_), M, n_in, ldx, p(dW_), ldw, p(db_), n_out, ACTS[act], p(Y_), ldy, st()))
    check(lib().vaenmf_train_dense_dx(p(dZ_), M, n_out, ldz, p(dW_), ldw, n_in, p(Yp_), ldp, ACTS[act], p(gX_), ldx, st()))
    check(lib().vaenmf_train_dense_dw(p(dZ_), M, n_out, ldz, p(dX_), n_in, ldx, p(gW_), ldw, p(gb_), st()))
    torch.cuda.synchronize()
    what = "M=%d in=%d out=%d act=%s" % (M, n_in, n_out, act)
    arena.check(what)
    arena.unchanged(what=what)
    untouched = [padding_untouched(arena, Y_, n_out), padding_untouched(arena, gX_, n_in), padding_untouched(arena, gW_, n_in)]
    assert all(untouched), (what, "columns past the width of Y, gX, gW still poison:", untouched)
    X64, W64, dZ64 = X.astype(np.float64), W.astype(np.float64), dZ.astype(np.float64)
    # forward
    pre = X64 @ W64.T + b
    tol = _act_tol(act, pre, C_CHAIN * (np.abs(X64) @ np.abs(W64).T + np.abs(b)))
    err = np.abs(Y_[:, :n_out].cpu().numpy().astype(np.float64) - _act64(act, pre))
    assert np.all(err <= tol), (what, "fwd", float((err / tol).max()))
    worst["fwd"] = max(worst["fwd"], float((err / tol).max()))
    # data gradient
    acc, d = dZ64 @ W64, _deriv64(act, Yp)
    ref = acc * d
    tol = C_CHAIN * (np.abs(dZ64) @ np.abs(W64)) * np.abs(d) + 2 * U * np.abs(acc) + 2 * U * np.abs(ref)
    err = np.abs(gX_[:, :n_in].cpu().numpy().astype(np.float64) - ref)
    assert np.all(err <= tol), (what, "dx", float((err / np.maximum(tol, 1e-300)).max()))
    worst["dx"] = max(worst["dx"], float((err / np.maximum(tol, 1e-300)).max()))
    # weight gradient and bias gradient from the same pass
    ref, tol = dZ64.T @ X64, C_CHAIN * (np.abs(dZ64).T @ np.abs(X64))
    err = np.abs(gW_[:, :n_in].cpu().numpy().astype(np.float64) - ref)
    assert np.all(err <= tol), (what, "dw", float((err / np.maximum(tol, 1e-300)).max()))
    worst["dw"] = max(worst["dw"], float((err / np.maximum(tol, 1e-300)).max()))
    ref, tol = dZ64.sum(0), C_CHAIN * np.abs(dZ64).sum(0)
    err = np.abs(gb_.cpu().numpy().astype(np.float64) - ref)
    assert np.all(err <= tol), (what, "db", float((err / np.maximum(tol, 1e-300)).max()))
    worst["db"] = max(worst["db"], float((err / np.maximum(tol, 1e-300)).max()))


# ---------------------------------------------------------------------------------------------------------------- steps
def gpu_run(case, init, data, steps=tc.STEPS, eps_mode="replay", seed=0):
    from vaenmf import train as vt
    model = tc.make_model(case)
    model.load_state_dict(init)
    tr = vt.Trainer(model, max_batch=case.B, seed=seed, device=DEV)
    tr.bind(data["X"].T, None if data["Y"] is None else data["Y"].T)
    if case.kind == "Classifier":
        tr.set_norm(data["mean"], data["std"], tc.LOSS_EPS)
    rows = torch.zeros(steps, 8, dtype=torch.float64, device=DEV)
    grad1 = None
    for s in range(steps):
        eps = data["eps"][s] if (data["eps"] is not None and eps_mode == "replay") else None
        if eps_mode == "fill" and case.kind != "Classifier":
            eps = tr.eps_fill(s + 1, case.B)
        tr.step(data["idx"][s], eps=eps, out=rows[s])
        if s == 0:
            grad1 = {k: v.numpy() for k, v in tr.gradients().items()}
    r = vt.read_losses(rows)
    losses = np.stack([r["loss"], r["recon"], r["kl"]], 1)
    counts = np.stack([r["tp"], r["tn"], r["fp"], r["fn"]], 1)
    final = {k: v.numpy() for k, v in tr.state_dict().items()}
    return tr, tc.Run(losses, counts, grad1, final)
