"""Value cases for the EM kernels: decoders at a trained model's value range, data drawn from the model, audio scales.

Shared by tests/test_value_range_cpu.py (no GPU: the pins on the cases themselves) and tests/test_gpu_value_range.py.
Everything here is numpy in float64 and needs neither the library nor a GPU.

Decoders.  sharpened_params() scales the three decoder layers of Xavier parameters and tilts the output bias by
b3 -= 4 + 8 f/F: "xavier" (1, 1, 1) without tilt is the flat regime of every other test, "trained" (4, 3, 6) and
"extreme" (6, 4, 10) saturate a good share of the tanh units and spread a frame's log-variance over tens of nats.

Data.  Z_true ~ N(0, 1); the noise floor W0 H0 lies 40 dB under the median speech variance; X = sqrt(Vx / 2) (n1 + i n2)
amp, with W0 and g scaled by amp^2.  In exact arithmetic every log-acceptance, mask and normalised update is invariant
under amp.  The amplitudes are powers of two derived from the products the kernels form (pair_products), see amplitude().

Bounds.  decoder64_full() evaluates the decoder in float64 together with two forward error figures of its log-variance
for a relative error gamma per product (GAMMA: the number formats): the first-order worst case and the root-sum-square
of the same model.  chain64() replays a Metropolis-Hastings chain in float64 -- along its own decisions or along given
ones -- with both bounds of every log-acceptance.
"""
import functools
from types import SimpleNamespace

import numpy as np

import vaenmf_oracle as orc
from em_support import gains_step64

COUNTS = [21, 40, 9]
# level -> (scales of decoder.hidden.0 / .hidden.1 / .reconstruction, variance of the random walk)
LEVELS = {"xavier": ((1.0, 1.0, 1.0), 0.01), "trained": ((4.0, 3.0, 6.0), 1e-4), "extreme": ((6.0, 4.0, 10.0), 1e-4)}
# relative error per product of a decoder layer.  bf16x3: two operand splits at 2^-17 each (hi + lo keeps 16 bits) and the
# dropped lo * lo term at 2^-18, rounded up to a power of two; bf16: two operands rounded at 2^-9 each
GAMMA = {"bf16x3": 2.0 ** -15, "bf16": 2.0 ** -8}
BF16_ROW = 2.0 ** -9          # a variance stored as bf16: one more rounding, 2^-9 relative = 2^-9 on its logarithm
TANH_ERR = 2e-7               # fast_tanh (csrc/common.h)
SECOND_ORDER = 2.0            # second-order terms and the fp32 accumulation
# the root-sum-square bound: gamma bounds a product's error, so sigma overstates the standard deviation of a sum of
# uniformly distributed roundings by sqrt(3); 8 sigma is about 14 standard deviations, and leaves room for the second-order
# terms that SECOND_ORDER covers in the worst-case bound
RSS_FACTOR = 8.0
ACC_FACTOR = 16               # v_rcp_f32 / v_log_f32 and the summation order, in units of 2^-24 of the sum of absolute terms
S_STEPS, NS = 6, 6            # the replayed chain: steps, samples kept (no burn-in: the samples show every decision)
FLT_MIN_EXP, FLT_MAX_EXP = -126, 128      # normal float32: [2^-126, 2^128)
MARGIN_EXP, EDGE_EXP = 10, 2  # the products stay 2^10 inside the normal range; the edge cases at least 2^2, less than 2^6

# shape -> F, latent dim, the reference's h_dim (the decoder runs over reversed(h_dim)), rank, samples per frame of the
# stored M-step, {precision: VAENMF_Q_CHAIN_KERNEL}
SHAPES = {
    "f65": dict(F=65, zdim=32, hdim=[128, 128], K=8, R=10, kernel={"bf16x3": 1, "bf16": 1}),     # one wavefront per 16 frames
    "f257": dict(F=257, zdim=32, hdim=[128, 128], K=8, R=10, kernel={"bf16": 2}),                # four wavefronts; fused W forms
    "f273": dict(F=273, zdim=32, hdim=[128, 128], K=10, R=10, kernel={"bf16x3": 0}),             # team kernel
    "f65w": dict(F=65, zdim=128, hdim=[256, 128], K=8, R=10, kernel={"bf16x3": 3, "bf16": 3}),   # wide kernel
}
AMPS = ("one", "small", "large", "edge_small", "edge_large")


def _case_list():
    out = []
    for shape, s in SHAPES.items():
        for prec in s["kernel"]:
            for level in LEVELS:
                out.append((shape, prec, level, "one", 0))
            out += [(shape, prec, "trained", "small", 0), (shape, prec, "trained", "large", 0)]
    out += [("f65", p, "trained", a, 0) for p in ("bf16x3", "bf16") for a in ("edge_small", "edge_large")]
    out += [("f257", "bf16", "trained", a, 0) for a in ("edge_small", "edge_large")]
    out += [("f65", "bf16x3", "trained", "one", 1), ("f65", "bf16", "trained", "one", 1)]          # M2: one label
    return out


CASES = _case_list()          # (shape, precision, level, amplitude, y_dim)

def case_id(case):
    return "-".join(str(v) for v in case[:4]) + ("-m2" if case[4] else "")


# ---------------------------------------------------------------------------------------------------------------------
def sharpened_params(F, zdim, hdim, scales, seed, y_dim=0):
    """Xavier parameters (bias sigma 0.05) with weight and bias of the decoder's layers scaled by `scales` and, unless the
    scales are all 1 (the control), the spectral tilt b3[f] -= 4 + 8 f / F."""
    p = orc.xavier_normal_params([F, zdim, list(hdim)], seed=seed, y_dim=y_dim, bias_std=0.05)
    names = ["decoder.hidden.%d" % i for i in range(orc.n_hidden(p, "decoder"))] + ["decoder.reconstruction"]
    assert len(names) == len(scales)
    for n, s in zip(names, scales):
        p[n + ".weight"] = (p[n + ".weight"] * np.float32(s)).astype(np.float32)
        p[n + ".bias"] = (p[n + ".bias"] * np.float32(s)).astype(np.float32)
    if tuple(scales) != (1.0,) * len(scales):
        p["decoder.reconstruction.bias"] = (p["decoder.reconstruction.bias"] - (4.0 + 8.0 * np.arange(F) / F)).astype(np.float32)
    return p


def _layers(params):
    names = ["decoder.hidden.%d" % i for i in range(orc.n_hidden(params, "decoder"))] + ["decoder.reconstruction"]
    return [(np.asarray(params[n + ".weight"], np.float64), np.asarray(params[n + ".bias"], np.float64)) for n in names]


def decoder64(params, zin, gamma=0.0):
    """The decoder in float64 on the inputs zin (n, L + Dy).  Returns (a, da, pre): the log-variances (n, F); the first
    order forward error bound of a for a relative error gamma per product -- per layer gamma (|W| |x| + |b|) on top of
    |W| times the incoming error, through tanh by (1 - h^2) plus TANH_ERR -- and the hidden pre-activations."""
    r = decoder64_full(params, zin, gamma)
    return r.a, r.da, r.pre


def decoder64_full(params, zin, gamma=0.0):
    """decoder64 with, beside the worst-case figure da, the root-sum-square figure sigma of the same first-order model:
    the roundings of different products are independent, so their contributions add in squares,
    sigma_a^2 = W^2 sigma_x^2 + gamma^2 (W^2 x^2 + b^2).  Also the inputs xs of every layer (for energy_sigma)."""
    x = np.asarray(zin, np.float64)
    dx, vx = np.zeros_like(x), np.zeros_like(x)
    layers = _layers(params)
    pre, xs = [], []
    for i, (W, b) in enumerate(layers):
        aW, W2 = np.abs(W), W * W
        xs.append(x)
        a = x @ W.T + b
        da = dx @ aW.T + gamma * (np.abs(x) @ aW.T + np.abs(b))
        va = vx @ W2.T + gamma ** 2 * ((x * x) @ W2.T + b * b)
        if i == len(layers) - 1:
            return SimpleNamespace(a=a, da=da, sigma=np.sqrt(va), pre=pre, xs=xs)
        pre.append(a)
        x = np.tanh(a)
        dx = (1.0 - x * x) * da + TANH_ERR
        vx = ((1.0 - x * x) * np.sqrt(va) + TANH_ERR) ** 2


def energy_sigma(params, full, v, gamma):
    """Root-sum-square figure of the error of sum_f v[n, f] a[n, f] (n,) under the model of decoder64_full, by the adjoint
    of the decoder: a rounding of a product of layer l reaches the sum through the layers behind it, so the bins' errors are
    not treated as independent.  `full`: decoder64_full of the same inputs.  TANH_ERR adds linearly."""
    layers = _layers(params)
    var, lin = np.zeros(v.shape[0]), np.zeros(v.shape[0])
    w = np.asarray(v, np.float64)
    for i in range(len(layers) - 1, -1, -1):
        W, b = layers[i]
        x = full.xs[i]
        var += gamma ** 2 * np.sum(w * w * ((x * x) @ (W * W).T + b * b), 1)
        if i == 0:
            break
        u = w @ W                                   # adjoint of this layer's input = the tanh output of the layer before
        lin += TANH_ERR * np.sum(np.abs(u), 1)
        w = u * (1.0 - x * x)
    return np.sqrt(var) + lin


def logvar_bound(da, bf16_rows=False):
    """The bound on |log Vs(device) - log Vs(float64)| from decoder64's first-order worst-case figure."""
    return SECOND_ORDER * da + (BF16_ROW if bf16_rows else 0.0)


def logvar_bound_rss(sigma, bf16_rows=False):
    """The sharper bound from decoder64_full's root-sum-square figure: RSS_FACTOR sigma."""
    return RSS_FACTOR * sigma + (BF16_ROW if bf16_rows else 0.0)


def bf16_round(x):
    """float32 -> bf16 (round to nearest even), as float32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(np.float32)


def decoder_split_sim(params, zin, drop_cross_term=False):
    """A float64 simulation of the bf16x3 decoder: every operand split v = hi + lo into two bf16 numbers, a product
    formed as Whi xhi + Wlo xhi + Whi xlo (lo * lo dropped), exact sums.  drop_cross_term: the fault, Wlo xhi missing."""
    split = lambda v: (lambda hi: (hi.astype(np.float64), bf16_round((v - hi).astype(np.float32)).astype(np.float64)))(bf16_round(v.astype(np.float32)))
    x = np.asarray(zin, np.float64)
    layers = _layers(params)
    for i, (W, b) in enumerate(layers):
        Wh, Wl = split(W)
        xh, xl = split(x)
        a = xh @ Wh.T + xl @ Wh.T + b
        if not drop_cross_term:
            a = a + xh @ Wl.T
        if i == len(layers) - 1:
            return a
        x = np.tanh(a)


# ---------------------------------------------------------------------------------------------------------------------
def _zin(c, Z, rows=None):
    """Decoder inputs of the frames `rows` (all) for latents Z (n, L): the labels appended."""
    if not c.Dy:
        return Z
    y = c.y_all if rows is None else c.y_all[rows]
    return np.concatenate([np.asarray(Z, np.float64), y.astype(np.float64)], -1)


def _base_case(shape, level, y_dim):
    """The case at amplitude 1, everything float32 as the engine is given it (X complex64)."""
    s = SHAPES[shape]
    F, L, K, R = s["F"], s["zdim"], s["K"], s["R"]
    scales, var_rw = LEVELS[level]
    params = sharpened_params(F, L, s["hdim"], scales, seed=7, y_dim=y_dim)
    g = np.random.default_rng(2000 + F)
    NT = sum(COUNTS)
    c = SimpleNamespace(shape=shape, level=level, F=F, K=K, R=R, L=L, Dy=y_dim, params=params, NT=NT, S_steps=S_STEPS, ns=NS,
                        var_rw=var_rw, off=np.concatenate([[0], np.cumsum(COUNTS)]), amp=1.0)
    c.Z_true = g.standard_normal((NT, L)).astype(np.float32)
    c.y_all = (g.random((NT, y_dim)) > 0.5).astype(np.float32) if y_dim else None
    c.ys = [c.y_all[c.off[u]:c.off[u + 1]] for u in range(len(COUNTS))] if y_dim else [None] * len(COUNTS)
    a_true = decoder64(params, _zin(c, c.Z_true))[0]
    c.gains = (0.5 + g.random(NT)).astype(np.float32)
    speech = c.gains[:, None].astype(np.float64) * np.exp(a_true)                      # (NT, F)
    c.W0, c.H0, Vb = [], [], np.empty((NT, F))
    for u, n in enumerate(COUNTS):
        sl = slice(c.off[u], c.off[u + 1])
        W, H = np.maximum(g.random((F, K)), 1e-8), np.maximum(g.random((K, n)), 1e-8)
        W = (W * (1e-4 * np.median(speech[sl]) / np.median(W @ H))).astype(np.float32)   # the floor 40 dB under the median
        c.W0.append(W); c.H0.append(H.astype(np.float32))
        Vb[sl] = (W.astype(np.float64) @ c.H0[u].astype(np.float64)).T
    Vx = speech + Vb
    c.X_all = (np.sqrt(Vx / 2) * (g.standard_normal((NT, F)) + 1j * g.standard_normal((NT, F)))).astype(np.complex64)
    c.Zs = (c.Z_true[:, None, :] + 0.1 * g.standard_normal((NT, R, L))).astype(np.float32)      # given samples (decoding path)
    c.Z0 = (c.Z_true + 0.1 * g.standard_normal((NT, L))).astype(np.float32)                      # where the chains start
    c.eps = g.standard_normal((S_STEPS, NT, L)).astype(np.float32)
    c.uu = np.maximum(g.random((S_STEPS, NT)), 1e-30).astype(np.float32)
    return c


def _scaled(c, amp):
    """The case at amplitude amp (a power of two: every scaling below is exact in float32)."""
    d = SimpleNamespace(**vars(c))
    d.amp = float(amp)
    a2 = np.float32(amp) * np.float32(amp)
    d.X_all = (c.X_all * np.float32(amp)).astype(np.complex64)
    d.W0 = [W * a2 for W in c.W0]
    d.gains = c.gains * a2
    assert all(np.all(np.isfinite(W)) and np.all(W > 0) for W in d.W0) and np.all(np.isfinite(d.X_all))
    d.Xs = [d.X_all[c.off[u]:c.off[u + 1]] for u in range(len(COUNTS))]
    return d


def noise_floor(c):
    """W0 H0 of every frame, float64 (NT, F)."""
    return np.concatenate([(W.astype(np.float64) @ H.astype(np.float64)).T for W, H in zip(c.W0, c.H0)])


def pair_products(c):
    """Smallest and largest product of two variance-sized factors that the kernels form, in float64 at the case's own
    amplitude, over every state and proposal of the replayed float64 chain and over the given samples:
      * the chain's energy: Vx of bins (0, 2) and (1, 3) of every 4 consecutive bins of a 16-bin tile (one log and one
        reciprocal per pair), and the numerators |X|^2 of one bin times Vx of the other;
      * the cost: Vx of the same bin in neighbouring sample rows, with the gains before the update and after it;
      * the squares Vx^2 (the M-step's 1 / Vx^2, which the reference shares)."""
    ch = chain64(c, 0.0)
    g, Vb, X2 = c.gains.astype(np.float64)[:, None], noise_floor(c), np.abs(c.X_all.astype(np.complex128)) ** 2
    lo, hi = np.inf, 0.0

    def take(*arrs):
        nonlocal lo, hi
        for a in arrs:
            a = a[a > 0]           # (an exact zero of |X|^2 is no product of two variances: 0 * Vx = 0 is exact)
            lo, hi = min(lo, float(a.min())), max(hi, float(a.max()))

    Fq = c.F // 4 * 4
    for a in ch.logvars:                                                     # (NT, F) of every evaluated state
        Vx = g * np.exp(a) + Vb
        q, x = Vx[:, :Fq].reshape(c.NT, -1, 4), X2[:, :Fq].reshape(c.NT, -1, 4)
        take(q[:, :, 0] * q[:, :, 2], q[:, :, 1] * q[:, :, 3], x[:, :, 0] * q[:, :, 2], x[:, :, 2] * q[:, :, 0],
             x[:, :, 1] * q[:, :, 3], x[:, :, 3] * q[:, :, 1], Vx * Vx)
    Vs = np.exp(decoder64(c.params, _zin_rows(c, c.Zs))[0]).reshape(c.NT, c.R, c.F)
    for u in range(len(COUNTS)):
        sl = slice(c.off[u], c.off[u + 1])
        V = np.moveaxis(Vs[sl], 0, -1)                                       # (R, F, n)
        g2 = gains_step64(X2[sl].T, V, Vb[sl].T, g[sl, 0])[0]
        for gg in (g[sl, 0], g2):
            Vx = gg * V + Vb[sl].T
            take(Vx[1:] * Vx[:-1], Vx * Vx)
    return lo, hi


def _zin_rows(c, Zs):
    """Decoder inputs of samples Zs (NT, R, L): (NT R, L + Dy)."""
    NT, R, L = Zs.shape
    if not c.Dy:
        return Zs.reshape(NT * R, L)
    y = np.broadcast_to(c.y_all[:, None, :], (NT, R, c.Dy))
    return np.concatenate([Zs, y], -1).reshape(NT * R, L + c.Dy)


@functools.lru_cache(maxsize=None)
def amplitude(shape, level, y_dim, kind):
    """The amplitude of a case: 1, or the power of two that puts the products of pair_products() -- which scale with
    amp^4 -- at the named distance from the edge of the normal float32 range: "small" / "large" the last power of two
    that keeps them a factor 2^MARGIN_EXP inside, "edge_small" / "edge_large" the last one that keeps 2^EDGE_EXP."""
    if kind == "one":
        return 1.0
    lo, hi = pair_products(_scaled(_base_case_cached(shape, level, y_dim), 1.0))
    m = MARGIN_EXP if kind in ("small", "large") else EDGE_EXP
    if kind.endswith("small"):
        return 2.0 ** int(np.ceil((FLT_MIN_EXP + m - np.log2(lo)) / 4))
    return 2.0 ** int(np.floor((FLT_MAX_EXP - m - np.log2(hi)) / 4))


@functools.lru_cache(maxsize=None)
def _base_case_cached(shape, level, y_dim):
    return _base_case(shape, level, y_dim)


@functools.lru_cache(maxsize=None)
def get_case(shape, level, amp_kind, y_dim=0):
    """The inputs of a case (shared: treat as read-only)."""
    c = _scaled(_base_case_cached(shape, level, y_dim), amplitude(shape, level, y_dim, amp_kind))
    c.amp_kind = amp_kind
    return c


# ---------------------------------------------------------------------------------------------------------------------
_chain_cache = {}


def chain64(c, gamma, decisions=None):
    """The replayed chain of mcem.py:371-441 in float64 (the latents themselves in float32, as every implementation holds
    them), all frames of the batch at once.  decisions (S, NT) bool: follow these instead of the chain's own -- the
    float64 evaluation of the very states another implementation went through, which makes every step of every frame
    comparable.  Returns acc, bound, bound_rss, decision (its own: log u < acc), margin = |log u - acc|, all (S, NT); the
    samples Zs (NT, ns, L) and the last state Z of the path followed; the log-variances of every evaluated state.
    bound: the decoder's worst-case log-variance bound (logvar_bound of decoder64 at `gamma`) carried through the derivative
    of a bin's energy, s |1 - X2 / Vx| with s = g Vs / Vx, for both states, plus ACC_FACTOR 2^-24 times the sum of the
    absolute values of every term of the log-acceptance.  bound_rss: the same with the root-sum-square figure of the two
    states' energies (energy_sigma; the two states share their weights' roundings, so their figures add linearly).  bound_fp32: the last term alone -- what separates two
    evaluations that are given the same variances."""
    key = (c.shape, c.level, c.Dy, c.amp, gamma, None if decisions is None else decisions.tobytes())
    if key in _chain_cache:
        return _chain_cache[key]
    g, Vb, X2 = c.gains.astype(np.float64)[:, None], noise_floor(c), np.abs(c.X_all.astype(np.complex128)) ** 2
    sd = np.sqrt(np.float32(c.var_rw))

    def state(Z):
        full = decoder64_full(c.params, _zin(c, Z), gamma)
        Vs = g * np.exp(full.a)
        Vx = Vs + Vb
        v = Vs / Vx * (1.0 - X2 / Vx)                                        # d energy / d log-variance, per bin
        return SimpleNamespace(a=full.a, Vx=Vx, sens=np.sum(np.abs(v) * logvar_bound(full.da), 1),
                               rss=RSS_FACTOR * energy_sigma(c.params, full, v, gamma),
                               mag=np.sum(np.abs(np.log(Vx)) + X2 / Vx, 1) + 0.5 * np.sum(Z.astype(np.float64) ** 2, 1))

    Z = c.Z0.copy()
    cur = state(Z)
    out = SimpleNamespace(acc=[], bound=[], bound_rss=[], bound_fp32=[], decision=[], logvars=[cur.a], Zs=np.zeros((c.NT, c.ns, c.L), np.float32))
    for m in range(c.S_steps):
        Zp = (Z + sd * c.eps[m]).astype(np.float32)
        prop = state(Zp)
        acc = (np.sum(np.log(cur.Vx) - np.log(prop.Vx) + (1.0 / cur.Vx - 1.0 / prop.Vx) * X2, 1)
               + 0.5 * np.sum(Z.astype(np.float64) ** 2 - Zp.astype(np.float64) ** 2, 1))
        fp32 = ACC_FACTOR * 2.0 ** -24 * (cur.mag + prop.mag)
        out.acc.append(acc)
        out.bound.append(cur.sens + prop.sens + fp32)
        out.bound_rss.append(cur.rss + prop.rss + fp32)
        out.bound_fp32.append(fp32)
        dec = np.log(c.uu[m].astype(np.float64)) < acc
        out.decision.append(dec)
        out.logvars.append(prop.a)
        if decisions is not None:
            dec = decisions[m]
        Z = np.where(dec[:, None], Zp, Z)
        for k in ("a", "Vx", "sens", "rss", "mag"):
            old, new = getattr(cur, k), getattr(prop, k)
            setattr(cur, k, np.where(dec[:, None] if old.ndim == 2 else dec, new, old))
        if m >= c.S_steps - c.ns:
            out.Zs[:, m - (c.S_steps - c.ns)] = Z
    for k in ("acc", "bound", "bound_rss", "bound_fp32", "decision"):
        setattr(out, k, np.stack(getattr(out, k)))
    out.margin = np.abs(np.log(c.uu.astype(np.float64)) - out.acc)
    out.Z = Z
    _chain_cache[key] = out
    return out


def left_out_share(ch, bound):
    """Share of frames that the rule `compare a frame's later steps only while each of its earlier decisions has a margin
    above its bound` leaves out of the comparison of the samples."""
    return 1.0 - float((ch.margin > bound).all(0).mean())
