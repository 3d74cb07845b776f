"""The sample-variance store's two layouts (csrc/common.h: VnStoreLayout) hold the same values: every case runs the same seeds
with VAENMF_STORE_ALIGNED=1 (rows of F-1 bins on whole 128-byte lines, the odd bins F-1 of a frame in a block of their own)
and =0 (rows of Fs bins, the odd bin inside) and requires bit-identical results.

A run is 3 EM iterations and the Wiener chain through vaenmf_em_run (W, Ht, g, Z, the costs, S_hat, N_hat), then the Wiener
chain once more on the state the run left, step by step with the store on: vaenmf_sample_store_gather's rows and
vaenmf_wiener_stored, which must give the run's S_hat again.  The layout is written by the chain kernels (chain.hip both
wave kernels, engine.hip's team kernel) and read by every streaming kernel (stream.hip) and the gather kernel (driver.hip);
no arithmetic differs between the layouts, so the bound is equality.

Shapes: the smallest that reach each writer and reader with partly filled tiles --
  F = 257, rank 8, bf16, utterances of 21 / 16 / 5 frames: wave tiles of 16, 5, 16 and 5 frames, a 64-frame W tile that never
      fills; 30 and 10 samples per frame (the fused / grouped W statistics exist for these two counts), each through the
      8-wavefront chain (VAENMF_WCHAIN4=0), through wchain4_kernel and through the team kernel (VAENMF_TEAM_CHAIN=1).  The
      Wiener chains take 40 and 12 samples: 41 slots make a frame's block of odd bins 128 bytes, two 16-byte pieces per lane.
  F = 513, rank 10, bf16, 17 + 3 frames, 30 samples: two 256-bin chunks per row, through wchain4_kernel and the team kernel.
  F = 257, bf16x3 (float rows), 18 frames.
  F = 65 and F = 250 keep the padded layout whatever the switch says, and the switch changes nothing; nor does it at
      F = 513 where the batch runs wchain_kernel.
VAENMF_Q_STORE_ALIGNED tells which layout the last chain wrote, so that no case passes by comparing a layout with itself."""
import ctypes as C
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import vaenmf_oracle as orc
from em_support import dec_list
from helpers import need_gpu

VAR_RW = 0.01
NITER = 3

#        id                F    K   precision  counts        nsE biE nsWF biWF  env                          chain kernel
CASES = [("f257_r30_wave8", 257, 8, "bf16", (21, 16, 5), 30, 2, 40, 2, {"VAENMF_WCHAIN4": "0"}, 1),
         ("f257_r30_wave4", 257, 8, "bf16", (21, 16, 5), 30, 2, 40, 2, {}, 2),
         ("f257_r30_team", 257, 8, "bf16", (21, 16, 5), 30, 2, 40, 2, {"VAENMF_TEAM_CHAIN": "1"}, 0),
         ("f257_r10_wave8", 257, 8, "bf16", (21, 16, 5), 10, 2, 12, 2, {"VAENMF_WCHAIN4": "0"}, 1),
         ("f257_r10_wave4", 257, 8, "bf16", (21, 16, 5), 10, 2, 12, 2, {}, 2),
         ("f257_r10_team", 257, 8, "bf16", (21, 16, 5), 10, 2, 12, 2, {"VAENMF_TEAM_CHAIN": "1"}, 0),
         ("f513_wave4", 513, 10, "bf16", (17, 3), 30, 2, 25, 2, {}, 2),
         ("f513_team", 513, 10, "bf16", (17, 3), 30, 2, 25, 2, {"VAENMF_TEAM_CHAIN": "1"}, 0),
         ("f257_float_rows", 257, 8, "bf16x3", (18,), 30, 2, 25, 2, {}, 1)]
# (F = 513 on wchain_kernel: its weights fill the LDS, no room to collect the odd bins -- chain.hip: vn_wchain_park_fits)
UNALIGNED = [("f513_wave_kernel", 513, 10, "bf16", (17, 3), 30, 2, 25, 2, {"VAENMF_WCHAIN4": "0"}, 1),
             ("f65", 65, 8, "bf16", (21, 5), 10, 2, 12, 2, {}, None),
             ("f250", 250, 8, "bf16", (21, 5), 10, 2, 12, 2, {}, None)]


@functools.lru_cache(maxsize=None)
def _params(F):
    return orc.xavier_normal_params([F, 32, [128, 128]], seed=5, bias_std=0.05)


@functools.lru_cache(maxsize=None)
def _inputs(F, K, counts):
    g = np.random.default_rng([F, K] + list(counts))
    NT = sum(counts)
    Xs = [((g.standard_normal((n, F)) + 1j * g.standard_normal((n, F))) * (1 + 3 * np.exp(-np.arange(F) / 40.0))).astype(np.complex64) for n in counts]
    W0 = [np.maximum(g.random((F, K)), 1e-8).astype(np.float32) for _ in counts]
    H0 = [np.maximum(g.random((K, n)), 1e-8).astype(np.float32) for n in counts]
    Z0 = torch.from_numpy((0.3 * g.standard_normal((NT, 32))).astype(np.float32))
    return SimpleNamespace(Xs=Xs, W0=W0, H0=H0, Z0=Z0)


class _env:
    def __init__(self, **kv):
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


def _run(case, aligned):
    """Everything the store's contents reach, and the layout and chain kernel the run reports."""
    from vaenmf import _lib
    from vaenmf.engine import BatchEngine
    _, F, K, prec, counts, nsE, biE, nsWF, biWF, env, _ = case
    inp = _inputs(F, K, counts)
    with _env(VAENMF_STORE_ALIGNED="1" if aligned else "0", **env):
        eng = BatchEngine(F, K, dec_list(_params(F)), precision=prec, max_frames=sum(counts), max_utts=len(counts), z_dim=32)
        eng.bind(counts, Rcap=max(nsE, nsWF), seeds=[11 + 7 * u for u in range(len(counts))])
        eng.set_spectrogram(inp.Xs)
        eng.init_nmf(inp.W0, inp.H0)
        eng.Z.copy_(inp.Z0)
        cost, S, N = eng.run(NITER, nsE, biE, nsWF, biWF, VAR_RW)
        q = lambda name: int(_lib.lib().vaenmf_plan_query(eng._plan, getattr(_lib, name)))
        out = SimpleNamespace(cost=cost.cpu().numpy(), S=S, N=N, W=eng.W.clone(), Ht=eng.Ht.clone(), g=eng.g.clone(), Z=eng.Z.clone(),
                              path=q("Q_MSTEP_PATH"), kernel=q("Q_CHAIN_KERNEL"), aligned=q("Q_STORE_ALIGNED"))
        # the Wiener chain again on the state the run left (same call number: the same draws), its store read both ways
        eng.sample_store(True)
        eng.mh_chain(nsWF, biWF, VAR_RW, call=NITER, update_Z=False)
        out.Vs = eng.stored_variances(nsWF).clone()
        out.S2 = eng.wiener_stored()[0].clone()
        out.aligned_wf = q("Q_STORE_ALIGNED")
        torch.cuda.synchronize()
        eng.close()
    return out


def _same(a, b, tag):
    assert np.array_equal(a.cost, b.cost), (tag, "cost")
    for name in ("Vs", "W", "Ht", "g", "Z", "S", "N", "S2"):
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(x, y), (tag, name, int((x != y).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_aligned_store_holds_what_the_padded_store_holds(case):
    need_gpu()
    tag, F, kernel = case[0], case[1], case[-1]
    on, off = _run(case, True), _run(case, False)
    assert on.path == 1 and off.path == 1, (tag, "the stored M-step must have run")
    assert on.kernel == kernel and off.kernel == kernel, (tag, on.kernel, off.kernel)
    assert (on.aligned, on.aligned_wf) == (1, 1) and (off.aligned, off.aligned_wf) == (0, 0), (tag, on.aligned, on.aligned_wf, off.aligned, off.aligned_wf)
    assert np.all(np.isfinite(on.cost)) and float(on.Vs[:, :, :F].min()) > 0, tag
    assert torch.equal(on.S2, on.S), (tag, "wiener_stored over the regathered store")
    _same(on, off, tag)
    # the odd bin is a value of its own, not a copy of a neighbour or a constant
    x = on.Vs[:, :, F - 1]
    assert float(x.min()) > 0 and not torch.equal(x, on.Vs[:, :, F - 2]) and int(torch.unique(x).numel()) > 8, tag
    assert float(on.Vs[:, :, F:].abs().max()) == 0, (tag, "padding bins of the gathered rows")


@pytest.mark.gpu
@pytest.mark.parametrize("case", UNALIGNED, ids=[c[0] for c in UNALIGNED])
def test_other_bin_counts_keep_the_padded_layout(case):
    need_gpu()
    on, off = _run(case, True), _run(case, False)
    assert (on.aligned, on.aligned_wf, off.aligned, off.aligned_wf) == (0, 0, 0, 0), case[0]
    assert on.path == 1 and off.path == 1
    _same(on, off, case[0])


# ---------------------------------------------------------------------------------------------------------------------
# the layout arithmetic (host only)
# ---------------------------------------------------------------------------------------------------------------------
def _layout(F, Fs, esz, Rs, frames, aligned):
    from vaenmf import _lib
    out = (C.c_int64 * 7)()
    _lib.check(_lib.lib().vaenmf_store_layout(F, Fs, esz, Rs, frames, int(aligned), C.cast(out, C.c_void_p)))
    return SimpleNamespace(row=out[0], frame=out[1], xslot=out[2], xframe=out[3], xbase=out[4], aligned=out[5], bytes=out[6])


@pytest.mark.parametrize("F,Fs", [(257, 272), (513, 528)])
@pytest.mark.parametrize("esz", [2, 4])
@pytest.mark.parametrize("Rs", [2, 11, 31, 32, 33, 76, 106])
def test_aligned_layout_arithmetic(F, Fs, esz, Rs):
    frames = 39
    l = _layout(F, Fs, esz, Rs, frames, True)
    assert l.aligned == 1 and l.row == F - 1 and l.frame == Rs * (F - 1) and l.xslot == 1
    # every row starts on a 128-byte line and covers whole lines; rows are contiguous and no two overlap
    starts = np.array([(n * l.frame + s * l.row) * esz for n in range(frames) for s in range(Rs)], dtype=np.int64)
    assert np.all(starts % 128 == 0) and (l.row * esz) % 128 == 0
    assert np.array_equal(np.diff(starts), np.full(starts.size - 1, l.row * esz))
    # a frame's odd bins: Rs elements in a block that is a multiple of 64 bytes, no larger than needed, on a 64-byte boundary
    xb = l.xframe * esz
    assert xb % 64 == 0 and Rs * esz <= xb < Rs * esz + 64 and (l.xbase * esz) % 64 == 0
    # the blocks lie behind the rows of all frame blocks, disjoint from them and from each other, and end with the store
    assert l.xbase * esz == starts[-1] + l.row * esz
    odd = np.array([(l.xbase + n * l.xframe + s * l.xslot) * esz for n in range(frames) for s in range(Rs)], dtype=np.int64)
    assert odd.min() >= starts[-1] + l.row * esz and np.unique(odd).size == odd.size
    assert odd.max() + esz <= l.bytes == frames * (l.frame + l.xframe) * esz


@pytest.mark.parametrize("F,Fs,aligned", [(257, 272, False), (513, 528, False), (65, 80, True), (250, 256, True), (129, 144, True), (256, 256, True)])
def test_padded_layout_arithmetic(F, Fs, aligned):
    for esz in (2, 4):
        l = _layout(F, Fs, esz, 31, 5, aligned)
        assert (l.aligned, l.row, l.frame, l.xslot, l.xframe, l.xbase) == (0, Fs, 31 * Fs, Fs, 31 * Fs, F - 1)
        assert l.bytes == 5 * 31 * Fs * esz
