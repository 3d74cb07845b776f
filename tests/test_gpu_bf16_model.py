"""The bf16 mode's kernels against the bf16-operand model of tests/bf16_model.py: the decoder evaluated exactly (float64) on
the operands the kernels really multiply.  Every other absolute check of this mode is against the plain fp32 oracle and
has to leave 5e-2 on a variance and 0.5 on a log-acceptance for the rounding of the operands; everything else in the mode
is an equality between kernels.  Here the reference has the kernels' operands, so what is left is float32 accumulation --
and, in a few per cent of the rows, a hidden activation that fell on the other side of a bf16 rounding boundary, which
moves a whole row by up to 3e-3 in log2 v.  The statistics are ones such rows cannot move, taken over |device - model|:

  decoding path (eng.decode, fp32 output; 8 samples per frame), in log2 v
    bin_median   the median per bin over the rows (one frame, one sample), then the worst bin      sandwich bound
    pos_median   the median per frame position within a 16-frame tile, then the worst position     sandwich bound
    row_share    the share of rows whose largest deviation exceeds 1e-5                            at most 25 %
    max                                                                                            at most 2e-2
  chain kernels (replayed noise, 4 samples after a burn-in of 2, store on), in the log-acceptance, on the DEVICE'S OWN
  trajectory: the state before every step rebuilt from Z, Zs and the decisions (bf16_model.follow_chain), the model's
  log-acceptance evaluated for exactly the states the kernel evaluated, all six steps of all frames
    step_median  the median per step over the frames, then the worst step                          sandwich bound
    pos_median   as above                                                                          sandwich bound
    within       the share of (step, frame) pairs within 3e-3                                      at least 75 %
    max                                                                                            at most 0.5
  and their stored rows (bf16) against bf16_rne(2^model), bit for bit
    moved        the share of rows that differ in more than a twentieth of their bins              at most 25 %
    share        the share of elements that differ in the other rows                               sandwich bound
    tile_share   the same for the worst 16-bin tile                                                sandwich bound
    padding bins exactly 0

A sandwich bound is sqrt(floor x ceiling), computed at run time on the CPU from the case's own seeded inputs: the floor is
the statistic of a float32-accumulating numpy emulation of a correct kernel, the ceiling the smallest over the numeric
defects planted in that emulation (activations truncated, latents unrounded, the M2 bias rows rounded the other way, one
k-step of one W3 tile a bf16 ulp off, one tile's output bias rounded to bf16) that the statistic answers for; a statistic
is used only where the two are a factor of 100 apart (tests/test_bf16_model_cpu.py asserts that for every one used here).
Each case is a ragged batch of 21 / 16 / 5 frames: wave tiles of 16, 5, 16 and 5 frames, rank 8.  VAENMF_Q_CHAIN_KERNEL is
asserted in every chain case, so that none passes by running another kernel.  Every test prints what it measured beside
floor, bound and ceiling (pytest -s)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bf16_model as bm
from helpers import need_gpu

pytestmark = pytest.mark.gpu

MAX_LOG2V = 2e-2         # six times the emulation's worst row, below every tolerance the suite had for this mode
MAX_ACC = 0.5            # test_wave_chain_bf16_mode's figure


class _env:
    def __init__(self, kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _engine(dec, F, z_dim, Rcap):
    from vaenmf.engine import BatchEngine
    eng = BatchEngine(F, bm.RANK, dec, precision="bf16", max_frames=sum(bm.COUNTS), max_utts=len(bm.COUNTS), z_dim=z_dim)
    return eng.bind(bm.COUNTS, Rcap=Rcap)


def _labels(eng, ops, y):
    """The layer-1 bias rows as the engine holds them (vaenmf_dense, fp32), checked against the host's restatement."""
    eng.set_labels(torch.from_numpy(y))
    B1 = eng.B1.cpu().numpy().copy()
    host = bm.layer1_bias(ops, y)
    assert np.max(np.abs(B1 - host)) <= 2.0 ** -22 * max(1.0, float(np.abs(host).max()))
    return B1


def _check(measured, bounds):
    for k, b in bounds.items():
        assert b.bound is not None, "%s: floor %.3e and ceiling %.3e are not a factor of %g apart" % (k, b.floor, b.ceiling, bm.SEPARATION)
        assert measured[k] <= b.bound, "%s: %.3e exceeds the bound %.3e (floor %.3e, ceiling %.3e)" % (k, measured[k], b.bound, b.floor, b.ceiling)


@pytest.mark.parametrize("case", bm.DECODE_CASES, ids=[c[0] for c in bm.DECODE_CASES])
def test_decoding_path_against_the_bf16_operand_model(case):
    """decode_kernel (engine.hip) in bf16 mode: fp32 layer-1 bias rows, bin F-1 of F = 16 k + 1 as an fp32 dot product of
    the unrounded activations."""
    need_gpu()
    name, F, z_dim, h_dim, Dy = case
    dec = bm.dec_list(bm.case_params(F, z_dim, h_dim, Dy))
    ops = bm.prepare(dec, z_dim)
    di = bm.decode_inputs(F, z_dim, Dy)
    R = bm.DECODE_R
    eng = _engine(dec, F, z_dim, R)
    assert not eng.wide
    eng.Zs.copy_(torch.from_numpy(di.Zs))
    B1 = np.repeat(_labels(eng, ops, di.y), R, 0) if Dy else None
    Vs = eng.decode(R).cpu().numpy()
    eng.close()
    assert np.all(Vs[:, :, F:] == 0) and np.all(np.isfinite(Vs)) and np.all(Vs[:, :, :F] > 0)
    ref = bm.decoder_bounds(ops, di.Zs.reshape(-1, di.Zs.shape[2]), np.repeat(di.pos, R), B1, False, F % 16 == 1 and F > 16)
    dev = np.abs(np.log2(Vs[:, :, :F].reshape(-1, F).astype(np.float64)) - ref.model)
    st = bm.decoder_stats(dev, np.repeat(di.pos, R))
    bm.report("decode %s (floor row_share %.3f max %.2e)" % (name, ref.floor["row_share"], ref.floor["max"]), st, ref.bounds)
    _check(st, ref.bounds)
    assert st["row_share"] <= bm.ROW_SHARE, st
    assert st["max"] <= MAX_LOG2V, st


@pytest.mark.parametrize("case", bm.CHAIN_CASES, ids=[c[0] for c in bm.CHAIN_CASES])
def test_chain_kernels_against_the_bf16_operand_model(case):
    """wchain_kernel (8 wavefronts; 4 at F = 513), wchain4_kernel, the team kernel mh_chain_kernel and widechain_kernel
    with SPLIT = false: the log-acceptances of all six steps on the kernel's own trajectory, and the rows it stored."""
    need_gpu()
    name, F, z_dim, h_dim, Dy, env, kernel, sw = case
    from vaenmf import _lib
    dec = bm.dec_list(bm.case_params(F, z_dim, h_dim, Dy))
    ops = bm.prepare(dec, z_dim)
    Lp = bm.latent_columns(z_dim, h_dim)
    inp = bm.chain_inputs(F, z_dim, Dy, Lp)
    ns, S = inp.ns, inp.ns + inp.burnin
    with _env(env):
        eng = _engine(dec, F, z_dim, ns)
        assert eng.Lp == Lp
        eng.set_spectrogram(inp.Xs)
        eng.init_nmf(inp.W0, inp.H0)
        if Dy:
            inp.B1 = _labels(eng, ops, inp.y)
        eng.g.copy_(torch.from_numpy(inp.g))
        eng.Z.copy_(torch.from_numpy(inp.Z0))
        eng.sample_store(True)
        acc = eng.mh_chain(ns, inp.burnin, inp.var_rw, eps=torch.from_numpy(inp.eps).to(eng.device), u=torch.from_numpy(inp.u).to(eng.device),
                           want_acc=True).cpu().numpy()
        ran = _lib.lib().vaenmf_plan_query(eng._plan, _lib.Q_CHAIN_KERNEL)
        Vs = eng.stored_variances(ns).cpu().numpy()
        rec = SimpleNamespace(acc=acc, Zs=eng.Zs[:, :ns].cpu().numpy().copy(), Z=eng.Z.cpu().numpy().copy())
        # g, W H and X2 as the engine holds them (float32 on the device; W H in float64 from its float32 factors)
        inp.X2 = eng.X2[:, :F].cpu().numpy().copy()
        W, Ht = eng.W.cpu().numpy().astype(np.float64), eng.Ht.cpu().numpy().astype(np.float64)
        inp.Vb = np.concatenate([Ht[eng.utt_slice(u)] @ W[u, :F].T for u in range(eng.U)])
        eng.close()
    assert ran == kernel, "VAENMF_Q_CHAIN_KERNEL = %d, the case is about kernel %d" % (ran, kernel)
    assert acc.shape == (S, sum(bm.COUNTS)) and np.all(np.isfinite(acc))
    assert np.all(Vs[:, :, F:] == 0) and np.all(Vs[:, :, :F] > 0)
    assert np.all((Vs.view(np.uint32) & 0xFFFF) == 0)              # the rows are bf16
    rec.store = (Vs[:, :, :F].view(np.uint32) >> 16).astype(np.uint16)
    ref = bm.chain_bounds(ops, inp, sw)
    st = bm.analyse_chain(rec, ops, inp, sw)
    bm.report("chain %s, kernel %d (floor within %.3f max %.2e moved %.3f)" % (name, ran, ref.floor["within"], ref.floor["max"], ref.floor["moved"]),
              st, ref.bounds)
    _check(st, ref.bounds)
    assert st["within"] >= 1.0 - bm.ROW_SHARE, st
    assert st["max"] <= MAX_ACC, st
    assert st["moved"] <= bm.ROW_SHARE, st
