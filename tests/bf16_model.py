"""The bf16 mode's reference: the decoder evaluated EXACTLY (float64 products and sums) on the operands the bf16 kernels
really multiply, the float32-accumulating emulation of those kernels that gives each statistic its floor, the planted
numeric defects that give it its ceiling, and the sandwich rule that turns the two into a bound.  Plain numpy; no tests
here (tests/test_bf16_model_cpu.py checks this module without a GPU, tests/test_gpu_bf16_model.py holds the kernels to it).

Operands, restated from csrc/plan.hip (vaenmf_set_decoder_weights, set_weights_wide): hidden layers scaled by 2 log2(e),
the output layer by log2(e), in double, rounded to float32, then to bf16 (round to nearest even); biases stay float32.
Forward pass, as csrc/common.h states it:
    xs = bf16(W1s) bf16(z) + b1s;  h = 1 - 2 / (2^xs + 1);  h -> bf16;  the same for layer 2;  log2 v = bf16(W3s) bf16(h2) + b3s
Switches for what the kernels really differ in (each read in the code, none a tolerance):
    one hidden layer        prepare() of a decoder [W1, b1, W3, b3]: layer 2 is skipped
    z_dim 16                the latents beyond z_dim are zero padding: only the first z_dim columns of z enter
    wide shapes (wide.hip)  any widths; every bin on the MFMA tiles
    B1 (M2)                 the per-frame layer-1 bias b1s + W1y y, float32 (vaenmf_dense); b1_bf16: the 8-wavefront
                            wchain_kernel (and wchain4_kernel at 17 bin tiles) keeps its rows as bf16 in LDS
    bin F-1                 last_bin_fp32: decode_kernel and the team kernel compute it (F = 16 k + 1 > 16) as an fp32 dot
                            product of the UNROUNDED activations with the unrounded float32 row w3n; the wave kernels and
                            widechain_kernel have it on a tile of its own like every other bin
The statistics never try to predict the kernels' bits: a hidden activation that falls on the other side of a bf16 rounding
boundary moves a whole row by up to 3e-3 in log2 v, for a few per cent of the rows.  Medians, and shares taken over the
rows that were not moved as a whole, cannot be moved by that; the planted defects a statistic answers for (DEFECTS) move
it by 10^2 to 10^5 floors."""
import math
from types import SimpleNamespace

import numpy as np

from em_support import dec_list  # noqa: F401  (the decoder's layer list, for the callers of prepare())

f32, f64 = np.float32, np.float64
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
ROW_DEV = 1e-5           # a row (one frame, one sample) "deviates" when its largest |device - model| in log2 v exceeds this
ROW_SHARE = 0.25         # ... and at most this share of the rows may (the emulation leaves 3 to 4 %, every defect 100 %)
ACC_DEV = 3e-3           # the same for a log-acceptance: the bound the suite holds the bf16x3 chain to
MOVED_ROW = 0.05         # a stored row counts as moved as a whole when more than this share of its bins differs from the model's bits
SEPARATION = 100.0       # a statistic is used only where its ceiling is at least this many floors


# ---------------------------------------------------------------------------------------------------------------
# bf16
# ---------------------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """float32 -> the 16 bits of the nearest bf16, ties to even (NaN kept quiet), as plan.hip's bf16_rne and v_cvt_pk_bf16_f32."""
    a = np.asarray(x, dtype=f32)
    u = np.ascontiguousarray(a).reshape(-1).view(np.uint32)
    nan = ((u & np.uint32(0x7F800000)) == np.uint32(0x7F800000)) & ((u & np.uint32(0x007FFFFF)) != 0)
    r = (np.where(nan, np.uint32(0), u) + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)
    r = np.where(nan, (u >> np.uint32(16)) | np.uint32(0x40), r)
    return r.astype(np.uint16).reshape(a.shape)


def bf16_from_bits(b):
    b = np.asarray(b, dtype=np.uint16)
    return (b.reshape(-1).astype(np.uint32) << np.uint32(16)).view(f32).astype(f64).reshape(b.shape)


def bf16_rne(x):
    """float32 -> bf16, ties to even, returned as float64."""
    return bf16_from_bits(bf16_bits(x))


def bf16_trunc(x):
    """float32 -> bf16 by dropping the low 16 bits (a planted defect, never the kernels' rounding)."""
    a = np.asarray(x, dtype=f32)
    u = np.ascontiguousarray(a).reshape(-1).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(f32).astype(f64).reshape(a.shape)


# ---------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------
def prepare(dec, z_dim):
    """dec = [W1 (H1, z_dim + Dy), b1, (W2, b2,) W3 (F, H), b3] float32, nn.Linear layout -> the operands of the kernels."""
    def scaled(a, c):
        return (np.asarray(a, f64) * c).astype(f32)

    dec = [np.asarray(a, f32) for a in dec]
    W1, b1, W3, b3 = dec[0], dec[1], dec[-2], dec[-1]
    C2, C1 = 2.0 * LOG2E, LOG2E
    o = SimpleNamespace(Lz=int(z_dim), F=int(W3.shape[0]), Dy=int(W1.shape[1] - z_dim))
    W1s = scaled(W1, C2)
    o.W1 = bf16_rne(W1s[:, :o.Lz])
    o.W1y = W1s[:, o.Lz:]                       # float32: the label columns go through vaenmf_dense, not the MFMA
    o.b1 = scaled(b1, C2)
    o.W2 = o.b2 = None
    if len(dec) == 6:
        o.W2, o.b2 = bf16_rne(scaled(dec[2], C2)), scaled(dec[3], C2)
    o.W3_f32 = scaled(W3, C1)
    o.W3 = bf16_rne(o.W3_f32)
    o.b3 = scaled(b3, C1)
    return o


def layer1_bias(ops, y):
    """B1 = b1s + W1y y per frame, float32 (plan.hip: vaenmf_layer1_bias through vaenmf_dense)."""
    acc = np.broadcast_to(ops.b1, (y.shape[0], ops.b1.shape[0])).astype(f32)
    for d in range(ops.Dy):
        acc = (acc + ops.W1y[None, :, d] * np.asarray(y, f32)[:, d:d + 1]).astype(f32)
    return acc


def _tanh_scaled(xs):
    with np.errstate(over="ignore"):
        return 1.0 - 2.0 / (np.exp2(xs) + 1.0)


def log2_variance(ops, z, B1=None, b1_bf16=False, last_bin_fp32=False):
    """The model: log2 of the decoded variance, float64 [rows, F].  z float32 [rows, >= z_dim]; B1 float32 [rows, H1] or None."""
    z = np.asarray(z, f32)[:, :ops.Lz]
    bias = ops.b1.astype(f64) if B1 is None else (bf16_rne(B1) if b1_bf16 else np.asarray(B1, f32).astype(f64))
    h = _tanh_scaled(bf16_rne(z) @ ops.W1.T + bias)
    if ops.W2 is not None:
        h = _tanh_scaled(bf16_rne(h.astype(f32)) @ ops.W2.T + ops.b2.astype(f64))
    out = bf16_rne(h.astype(f32)) @ ops.W3.T + ops.b3.astype(f64)
    if last_bin_fp32:
        out[:, -1] = h.astype(f32).astype(f64) @ ops.W3_f32[-1].astype(f64) + f64(ops.b3[-1])
    return out


# ---------------------------------------------------------------------------------------------------------------
# the float32-accumulating emulation and the planted defects
# ---------------------------------------------------------------------------------------------------------------
# name -> the statistics it must move.  "rows": a defect in every bin of every row (medians per bin, per frame position,
# the share of rows, the log-acceptances).  "tile": confined to one 16-bin tile -- it moves that tile's per-bin medians and
# every row's largest deviation, but neither a median over all bins (the per-position statistic) nor, being nearly the
# same for the two states of a step, their energy difference (the log-acceptance statistics).
# "bias": a constant shift of one tile's bins, the smallest defect of all (5e-4 in log2 v, a sixteenth of a bf16 step): the
# decoding path's per-bin medians resolve it; the 168 bf16 rows a chain case stores do not (one element in fifty changes).
DEFECTS = {"act_trunc": "rows",        # activations truncated to bf16 instead of rounded to nearest
           "z_unrounded": "rows",      # the latents enter layer 1 unrounded
           "b1_other": "rows",         # M2: the layer-1 bias rows rounded to bf16 where the kernel keeps float32, or the reverse
           "w3_ulp": "tile",           # one 32-feature k-step of one 16-bin tile of W3 one bf16 ulp off
           "b3_bf16": "bias"}          # one bin tile's output bias rounded to bf16
DEFECT_TILE, DEFECT_KSTEP = 1, 2


def defects_for(m2):
    return [d for d in DEFECTS if m2 or d != "b1_other"]


def _mm32(a, b, reverse):
    """a b^T in float32; reverse: the features summed in the opposite order (another realisation of the same rounding)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    if reverse:
        a, b = np.ascontiguousarray(a[:, ::-1]), np.ascontiguousarray(b[:, ::-1])
    return a @ b.T


def emulate_log2_variance(ops, z, B1=None, b1_bf16=False, last_bin_fp32=False, defect=None, reverse=False):
    """A correct kernel's arithmetic, as far as numpy restates it: bf16 operands, float32 products and sums, float32
    exp2 / reciprocal in the tanh.  `defect`: one of DEFECTS, planted HERE and nowhere else.  float32 [rows, F].
    Which rows a rounding boundary flips depends on the order of the float32 sums: `reverse` gives a second correct
    kernel, and a floor is the larger of the two's statistics."""
    assert defect is None or defect in DEFECTS
    z = np.asarray(z, f32)[:, :ops.Lz]
    rnd = bf16_trunc if defect == "act_trunc" else bf16_rne
    if defect == "b1_other":
        assert B1 is not None
        b1_bf16 = not b1_bf16
    bias = ops.b1 if B1 is None else (bf16_rne(B1).astype(f32) if b1_bf16 else np.asarray(B1, f32))

    def tanh32(xs):
        with np.errstate(over="ignore"):
            return (f32(1) - f32(2) * (f32(1) / (np.exp2(xs.astype(f32)) + f32(1)))).astype(f32)

    zin = z if defect == "z_unrounded" else bf16_rne(z).astype(f32)
    h = tanh32(_mm32(zin, ops.W1, reverse) + bias)
    if ops.W2 is not None:
        h = tanh32(_mm32(rnd(h), ops.W2, reverse) + ops.b2)
    W3, b3 = ops.W3, ops.b3
    rows = slice(16 * DEFECT_TILE, min(16 * DEFECT_TILE + 16, ops.F))
    if defect == "w3_ulp":
        W3 = W3.copy()
        cols = slice(32 * DEFECT_KSTEP, 32 * DEFECT_KSTEP + 32)
        W3[rows, cols] = bf16_from_bits(bf16_bits(W3[rows, cols].astype(f32)) + np.uint16(1))
    if defect == "b3_bf16":
        b3 = b3.copy()
        b3[rows] = bf16_rne(b3[rows]).astype(f32)
    out = (_mm32(rnd(h), W3, reverse) + b3).astype(f32)
    if last_bin_fp32:
        out[:, -1] = h @ ops.W3_f32[-1] + ops.b3[-1]
    return out


# ---------------------------------------------------------------------------------------------------------------
# energy and log-acceptance (mcem.py:392-417 as oracle/vaenmf_oracle.py restates it), float64
# ---------------------------------------------------------------------------------------------------------------
def log_acceptance(l2v_t, l2v_p, z_t, z_p, g, Vb, X2):
    """The oracle's own expression for the state z_t and the proposal z_p of every frame, with v = 2^(log2 v) from the model:
    sum_f [log Vx_t - log Vx_p + (1 / Vx_t - 1 / Vx_p) X2] + .5 sum (z_t^2 - z_p^2), Vx = g v + Vb.  [frames]"""
    g, Vb, X2 = np.asarray(g, f64)[:, None], np.asarray(Vb, f64), np.asarray(X2, f64)
    Vx_t, Vx_p = g * np.exp2(l2v_t) + Vb, g * np.exp2(l2v_p) + Vb
    z_t, z_p = np.asarray(z_t, f64), np.asarray(z_p, f64)
    return np.sum(np.log(Vx_t) - np.log(Vx_p) + (1.0 / Vx_t - 1.0 / Vx_p) * X2, 1) + 0.5 * np.sum(z_t ** 2 - z_p ** 2, 1)


def emulate_energy(l2v32, g, Vb, X2):
    """E = sum_f [log Vx + X2 / Vx] the way the chain kernels add it: float32 per bin and over 32 bins, float64 across."""
    ev = np.exp2(np.asarray(l2v32, f32))
    vx = (np.asarray(g, f32)[:, None] * ev + np.asarray(Vb, f32)).astype(f32)
    t = (np.log2(vx) * f32(LN2) + np.asarray(X2, f32) * (f32(1) / vx)).astype(f32)
    e = np.zeros(t.shape[0], f64)
    for f0 in range(0, t.shape[1], 32):
        e += np.sum(t[:, f0:f0 + 32], 1, dtype=f32).astype(f64)
    return e


# ---------------------------------------------------------------------------------------------------------------
# a chain: the emulated one (the device's stand-in on the CPU) and the follower of a recorded trajectory
# ---------------------------------------------------------------------------------------------------------------
def sd_columns(var_rw, Lz, Lp):
    """Random-walk step per latent column: sqrtf(var) for the model's latents, 0 for the zero padding (driver.hip: sd, sd_hi)."""
    return np.where(np.arange(Lp) < Lz, np.sqrt(f32(var_rw)), f32(0)).astype(f32)


def propose(z, eps, sdc, fused=True):
    """Z' = Z + sd eps in float32: one fused multiply-add (what the compiler makes of the kernels' expression) or two roundings."""
    if fused:
        return (np.asarray(z, f64) + np.asarray(sdc, f64) * np.asarray(eps, f64)).astype(f32)
    return (np.asarray(z, f32) + (np.asarray(sdc, f32) * np.asarray(eps, f32)).astype(f32)).astype(f32)


def emulate_chain(ops, inp, sw, defect=None, reverse=False):
    """The MH chain (mcem.py:371-441) on the emulation: what a correct -- or, with `defect`, a subtly wrong -- kernel would
    leave behind.  inp: Z0 [NT, Lp], eps [S, NT, Lp], u [S, NT], g, Vb, X2, B1 (or None), ns, burnin, var_rw.  Returns a
    record like the device's: acc [S, NT] float32, Zs [NT, ns, Lp], Z, and the stored rows of the samples as bf16 bits."""
    S, NT, Lp = inp.eps.shape
    sdc = sd_columns(inp.var_rw, ops.Lz, Lp)
    dec = lambda zz: emulate_log2_variance(ops, zz, inp.B1, sw["b1_bf16"], sw["last_bin_fp32"], defect, reverse)
    z = inp.Z0.astype(f32).copy()
    l2 = dec(z)
    E = emulate_energy(l2, inp.g, inp.Vb, inp.X2)
    bits = bf16_bits(np.exp2(l2))
    rec = SimpleNamespace(acc=np.zeros((S, NT), f32), Zs=np.zeros((NT, inp.ns, Lp), f32), store=np.zeros((NT, inp.ns, ops.F), np.uint16))
    for m in range(S):
        zp = propose(z, inp.eps[m], sdc)
        l2p = dec(zp)
        Ep = emulate_energy(l2p, inp.g, inp.Vb, inp.X2)
        pr = np.sum(z * z - zp * zp, 1, dtype=f32)
        rec.acc[m] = (E - Ep).astype(f32) + f32(0.5) * pr
        ok = np.log(inp.u[m].astype(f32)) < rec.acc[m]
        z[ok], E[ok], bits[ok] = zp[ok], Ep[ok], bf16_bits(np.exp2(l2p))[ok]
        if m >= inp.burnin:
            rec.Zs[:, m - inp.burnin], rec.store[:, m - inp.burnin] = z, bits
    rec.Z = z.copy()
    return rec


def follow_chain(rec, inp, Lz):
    """The device's OWN trajectory: the state and the proposal of every step, rebuilt from Z0, the replayed noise, the
    decisions log u < acc and -- from the end of the burn-in on, where the samples are on record -- Zs itself.  A frame
    whose recorded sample is neither the proposal nor the state it was in, or whose last state is not Z, fails here.
    Returns (z_t, z_p) float32 [S, NT, Lp]."""
    S, NT, Lp = inp.eps.shape
    sdc = sd_columns(inp.var_rw, Lz, Lp)
    for fused in (True, False):
        z = inp.Z0.astype(f32).copy()
        zt, zp_all, good = np.zeros((S, NT, Lp), f32), np.zeros((S, NT, Lp), f32), True
        for m in range(S):
            zp = propose(z, inp.eps[m], sdc, fused)
            zt[m], zp_all[m] = z, zp
            ok = np.log(inp.u[m].astype(f32)) < rec.acc[m]
            if m >= inp.burnin:
                kept = rec.Zs[:, m - inp.burnin]
                took, stayed = np.all(kept == zp, 1), np.all(kept == z, 1)
                good = good and bool(np.all(took | stayed))
                ok = took
            z = np.where(ok[:, None], zp, z)
        if good and np.array_equal(z, rec.Z):
            return zt, zp_all
    raise AssertionError("the recorded samples are not a trajectory of the replayed noise")


# ---------------------------------------------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------------------------------------------
def decoder_stats(dev, pos):
    """dev = |device - model| in log2 v [rows, F]; pos [rows]: the row's frame position within its 16-frame tile."""
    return {"bin_median": float(np.max(np.median(dev, 0))),
            "pos_median": float(max(np.median(dev[pos == p]) for p in np.unique(pos))),
            "row_share": float(np.mean(dev.max(1) > ROW_DEV)),
            "max": float(dev.max())}


def acceptance_stats(dev, pos):
    """dev = |device - model| of the log-acceptances [steps, frames]; pos [frames]."""
    return {"step_median": float(np.max(np.median(dev, 1))),
            "pos_median": float(max(np.median(dev[:, pos == p]) for p in np.unique(pos))),
            "within": float(np.mean(dev <= ACC_DEV)),
            "max": float(dev.max())}


def store_stats(bits, model_bits):
    """Stored bf16 rows against bf16_rne(2^model), bit for bit [rows, F].  A row moved as a whole by a flipped hidden
    activation differs in a twentieth of its bins and more (MOVED_ROW): `moved` is the share of such rows, a condition like the
    decoder's row share.  The other rows give the share of elements that differ, overall and for the worst 16-bin tile.
    (Per single bin the 168 rows of a 42-frame, 4-sample case resolve 6e-3: no room for a factor of 100 under any
    defect.  A tile's 2688 elements resolve 4e-4.)"""
    diff = np.asarray(bits) != np.asarray(model_bits)
    moved = diff.mean(1) > MOVED_ROW
    d = diff[~moved] if not moved.all() else diff
    tiles = [d[:, f0:f0 + 16].mean() for f0 in range(0, d.shape[1], 16)]
    return {"share": float(d.mean()), "tile_share": float(max(tiles)), "moved": float(moved.mean()), "resolution": 1.0 / (diff.shape[0] * 16)}


def frame_positions(counts):
    return np.concatenate([np.arange(n) % 16 for n in counts])


# ---------------------------------------------------------------------------------------------------------------
# the sandwich rule
# ---------------------------------------------------------------------------------------------------------------
def sandwich(floor, ceilings, scope, resolution=0.0):
    """floor: the statistic of the correct emulation; ceilings: {defect: the statistic with it planted}; scope: the kinds
    of defect (DEFECTS) the statistic answers for.  The ceiling is the smallest over those defects, the bound
    sqrt(floor x ceiling) -- or None where the ceiling is not SEPARATION floors away: such a statistic is not used.
    resolution: the smallest non-zero value the statistic can take at this size (a share of n elements: 1 / n), which the
    floor is not allowed to undercut."""
    floor = max(float(floor), float(resolution), 1e-300)
    ceiling = min(v for d, v in ceilings.items() if DEFECTS[d] in scope)
    bound = math.sqrt(floor * ceiling) if ceiling >= SEPARATION * floor else None
    return SimpleNamespace(floor=floor, ceiling=ceiling, bound=bound)


def _larger(a, b):
    return {k: (min if k == "within" else max)(a[k], b[k]) for k in a}


def decoder_bounds(ops, z, pos, B1=None, b1_bf16=False, last_bin_fp32=False):
    """Floor, ceiling and bound of the decoding path's statistics at the inputs of a case, from the CPU alone.  The
    emulation's output goes through the kernels' last steps too: v = 2^(log2 v) in float32, compared as log2 v."""
    model = log2_variance(ops, z, B1, b1_bf16, last_bin_fp32)
    run = lambda d, rev=False: decoder_stats(np.abs(np.log2(np.exp2(emulate_log2_variance(ops, z, B1, b1_bf16, last_bin_fp32, d, rev)).astype(f64)) - model), pos)
    fl = _larger(run(None), run(None, True))
    ce = {d: run(d) for d in defects_for(B1 is not None)}
    out = {"bin_median": sandwich(fl["bin_median"], {d: s["bin_median"] for d, s in ce.items()}, ("rows", "tile", "bias")),
           "pos_median": sandwich(fl["pos_median"], {d: s["pos_median"] for d, s in ce.items()}, ("rows",))}
    return SimpleNamespace(model=model, floor=fl, defects=ce, bounds=out)


def analyse_chain(rec, ops, inp, sw):
    """The statistics of a recorded chain -- the device's, or the emulation's -- against the model on its own trajectory."""
    zt, zp = follow_chain(rec, inp, ops.Lz)
    S, NT, Lp = zt.shape
    rep = lambda a: np.tile(a, (S,) + (1,) * (np.ndim(a) - 1))
    dec = lambda zz: log2_variance(ops, zz.reshape(S * NT, Lp), None if inp.B1 is None else rep(inp.B1), sw["b1_bf16"], sw["last_bin_fp32"])
    acc = log_acceptance(dec(zt), dec(zp), zt.reshape(S * NT, Lp), zp.reshape(S * NT, Lp), rep(inp.g), rep(inp.Vb), rep(inp.X2)).reshape(S, NT)
    st = acceptance_stats(np.abs(rec.acc.astype(f64) - acc), inp.pos)
    B1s = None if inp.B1 is None else np.repeat(inp.B1, inp.ns, 0)
    model = log2_variance(ops, rec.Zs.reshape(NT * inp.ns, Lp), B1s, sw["b1_bf16"], sw["last_bin_fp32"])
    st.update(store_stats(rec.store.reshape(NT * inp.ns, -1), bf16_bits(np.exp2(model))))
    return st


def chain_bounds(ops, inp, sw):
    """Floor, ceiling and bound of a chain case's statistics: the emulated chain, clean and with each defect, analysed
    exactly as the device's record is."""
    fl = _larger(analyse_chain(emulate_chain(ops, inp, sw), ops, inp, sw), analyse_chain(emulate_chain(ops, inp, sw, reverse=True), ops, inp, sw))
    ce = {d: analyse_chain(emulate_chain(ops, inp, sw, d), ops, inp, sw) for d in defects_for(inp.B1 is not None)}
    col = lambda k: {d: s[k] for d, s in ce.items()}
    out = {"step_median": sandwich(fl["step_median"], col("step_median"), ("rows",)),
           "pos_median": sandwich(fl["pos_median"], col("pos_median"), ("rows",)),
           "share": sandwich(fl["share"], col("share"), ("rows",), fl["resolution"] / (ops.F / 16.0)),
           "tile_share": sandwich(fl["tile_share"], col("tile_share"), ("rows", "tile"), fl["resolution"])}
    return SimpleNamespace(floor=fl, defects=ce, bounds=out)


def report(title, measured, bounds):
    """One line per statistic: measured beside floor, bound and ceiling."""
    lines = [title]
    for k, b in bounds.items():
        lines.append("  %-12s measured %.3e   floor %.3e   bound %s   ceiling %.3e" %
                     (k, measured[k], b.floor, "%.3e" % b.bound if b.bound is not None else "(not used)", b.ceiling))
    for k in measured:
        if k not in bounds and k != "resolution":
            lines.append("  %-12s measured %.3e" % (k, measured[k]))
    print("\n".join(lines))


# ---------------------------------------------------------------------------------------------------------------
# seeded cases (shared by the CPU and the GPU tests): ragged batch of 21 / 16 / 5 frames -- wave tiles of 16, 5, 16 and 5
# frames, so every frame position 0..15 of a tile occurs and partly filled tiles occur; rank 8
# ---------------------------------------------------------------------------------------------------------------
COUNTS = (21, 16, 5)
RANK = 8
DECODE_R = 8
CHAIN_NS, CHAIN_BURNIN, VAR_RW = 4, 2, 0.01


def case_params(F, z_dim=32, h_dim=(128, 128), Dy=0):
    import vaenmf_oracle as orc
    return orc.xavier_normal_params([F, z_dim, list(h_dim)], seed=3, y_dim=Dy, bias_std=0.1)


def decode_inputs(F, z_dim, Dy, Lp=32):
    """Eight samples per frame, z ~ N(0, 1) (zero in the padding columns), binary labels."""
    g = np.random.default_rng([F, z_dim, Dy, 1])
    NT = sum(COUNTS)
    Zs = np.zeros((NT, DECODE_R, Lp), f32)
    Zs[:, :, :z_dim] = g.standard_normal((NT, DECODE_R, z_dim))
    y = (g.random((NT, Dy)) > 0.5).astype(f32) if Dy else None
    return SimpleNamespace(Zs=Zs, y=y, pos=frame_positions(COUNTS))


# (F, z_dim, Dy) -> further words of the generator seed of a chain case's inputs.  A 168-row case resolves a share of
# differing elements to 4e-4 per tile: where the emulation's floor at the plain seed is two or three such elements instead of
# one, a used statistic falls short of SEPARATION floors below its ceiling (tile_share 75 floors at (513, 16, 0), share 53 at
# (257, 16, 1)), which tests/test_bf16_model_cpu.py refuses.  Such a case gets other inputs, chosen on the CPU from the
# emulation alone; no bound moves.
CHAIN_INPUT_SALT = {(513, 16, 0): [1], (257, 16, 1): [3]}


def chain_inputs(F, z_dim, Dy, Lp=32):
    """A state of the engine and the replayed noise of one chain of CHAIN_BURNIN + CHAIN_NS steps."""
    g = np.random.default_rng([F, z_dim, Dy, 2] + CHAIN_INPUT_SALT.get((F, z_dim, Dy), []))
    NT, S, K = sum(COUNTS), CHAIN_NS + CHAIN_BURNIN, RANK
    c = SimpleNamespace(ns=CHAIN_NS, burnin=CHAIN_BURNIN, var_rw=VAR_RW, pos=frame_positions(COUNTS))
    c.Xs = [((g.standard_normal((n, F)) + 1j * g.standard_normal((n, F))) * (0.5 + 3 * np.exp(-np.arange(F) / 60.0))).astype(np.complex64) for n in COUNTS]
    c.W0 = [np.maximum(g.random((F, K)), 1e-8).astype(f32) for _ in COUNTS]
    c.H0 = [np.maximum(g.random((K, n)), 1e-8).astype(f32) for n in COUNTS]
    c.y = (g.random((NT, Dy)) > 0.5).astype(f32) if Dy else None
    c.eps = np.zeros((S, NT, Lp), f32)
    c.eps[:, :, :z_dim] = g.standard_normal((S, NT, z_dim))
    c.u = g.random((S, NT)).astype(f32)
    c.Z0 = np.zeros((NT, Lp), f32)
    c.Z0[:, :z_dim] = 0.5 * g.standard_normal((NT, z_dim))
    c.g = (0.5 + g.random(NT)).astype(f32)
    c.X2 = np.concatenate([(np.abs(X) ** 2).astype(f32) for X in c.Xs])
    c.Vb = np.concatenate([(W.astype(f64) @ H.astype(f64)).T for W, H in zip(c.W0, c.H0)])      # float64 W H of the float32 factors
    c.B1 = None
    return c


# id, F, z_dim, the reference's h_dim (the decoder runs over reversed(h_dim)), label width
DECODE_CASES = [("f65", 65, 32, (128, 128), 0),                # 5 bin tiles, exact
                ("f201", 201, 32, (128, 128), 0),              # 13 tiles: the non-exact <17> instantiation of the wave kernel's shape
                ("f257", 257, 32, (128, 128), 0),
                ("f513", 513, 32, (128, 128), 0),
                ("f65_z16", 65, 16, (128, 128), 0),
                ("f65_h128", 65, 32, (128,), 0),
                ("f257_labels", 257, 32, (128, 128), 1),
                ("f257_z16_h128", 257, 16, (128,), 0),         # geometry 3, the one-hidden branch of Dec::hidden with its own odd-bin dot
                ("f513_z16_h128", 513, 16, (128,), 0)]         # geometry 4, the reference's bin count
# id, F, z_dim, h_dim, label width, kernel switches, VAENMF_Q_CHAIN_KERNEL, the model's switches
_WAVE = {"b1_bf16": False, "last_bin_fp32": False}
CHAIN_CASES = [("wave8_f257", 257, 32, (128, 128), 0, {"VAENMF_WCHAIN4": "0"}, 1, _WAVE),
               ("wave8_f257_labels", 257, 32, (128, 128), 1, {"VAENMF_WCHAIN4": "0"}, 1, {"b1_bf16": True, "last_bin_fp32": False}),
               ("wave_f65", 65, 32, (128, 128), 0, {}, 1, _WAVE),
               ("wave_f201", 201, 32, (128, 128), 0, {}, 1, _WAVE),
               ("wave_f513", 513, 32, (128, 128), 0, {"VAENMF_WCHAIN4": "0"}, 1, _WAVE),      # four wavefronts, four tiles' fragments from L2
               ("wave4_f257", 257, 32, (128, 128), 0, {}, 2, _WAVE),
               ("wave4_f513", 513, 32, (128, 128), 0, {}, 2, _WAVE),
               ("wave4_f257_labels", 257, 32, (128, 128), 1, {}, 2, {"b1_bf16": True, "last_bin_fp32": False}),
               ("team_f257", 257, 32, (128, 128), 0, {"VAENMF_TEAM_CHAIN": "1"}, 0, {"b1_bf16": False, "last_bin_fp32": True}),
               ("wide_f130", 130, 128, (256, 128), 0, {}, 3, _WAVE),
               # the narrow decoders beside 32 / [128, 128]: one hidden layer (the wave kernels copy layer 1's fragments, the team
               # kernel takes Dec::hidden's one-hidden branch) and z_dim 16 (sd_hi = 0 in the wave kernels, the noise mask per
               # latent quad in the team kernel, which takes the layer-1 bias rows of the labels in float32)
               ("wave4_f257_z16_h128", 257, 16, (128,), 0, {}, 2, _WAVE),
               ("wave_f513_z16_h128", 513, 16, (128,), 0, {"VAENMF_WCHAIN4": "0"}, 1, _WAVE),
               ("team_f257_h128", 257, 32, (128,), 0, {"VAENMF_TEAM_CHAIN": "1"}, 0, {"b1_bf16": False, "last_bin_fp32": True}),
               ("team_f257_z16_labels", 257, 16, (128, 128), 1, {"VAENMF_TEAM_CHAIN": "1"}, 0, {"b1_bf16": False, "last_bin_fp32": True})]


# cases added after the first lists: tests parametrised over the SET of shapes put theirs behind the earlier ones, so that
# the ids pytest numbers (h_dim0 ..) stay what they were
LATER_CASES = ("f257_z16_h128", "f513_z16_h128", "wave4_f257_z16_h128", "wave_f513_z16_h128", "team_f257_h128", "team_f257_z16_labels")


def case_shapes():
    """(F, z_dim, h_dim, Dy) of every case, without repeats: the earlier cases' shapes sorted, then the later ones' sorted."""
    of = lambda later: {c[1:5] for c in DECODE_CASES + CHAIN_CASES if (c[0] in LATER_CASES) == later}
    return sorted(of(False)) + sorted(of(True) - of(False))


def latent_columns(z_dim, h_dim):
    return 128 if (z_dim > 32 or 256 in h_dim) else 32
