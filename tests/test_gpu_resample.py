"""The batched polyphase resampler (csrc/resample.hip, vaenmf/resample.py) on the GPU: against the numpy closed form of
tests/resample_cases.py, its independence of the batch, its alignment, its buffer bounds and refusals, and the paths that
use it: Reconstructor.enhance / MaskEnhancer.enhance with fs_in, driver.evaluate with resample=True."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import resample_cases as rc
import vaenmf_oracle as orc
from guarded import Arena, same_bits
from helpers import need_gpu

pytestmark = pytest.mark.gpu


def _cat(xs):
    return torch.from_numpy(np.concatenate(xs).astype(np.float32)).cuda()


def _split(y, counts):
    return [p.cpu().numpy() for p in torch.split(y, counts)]


@functools.lru_cache(maxsize=None)
def _case(up, down, scale):
    """(inputs, float64 oracle outputs) of the ragged batch of one ratio and scale; computed once, never modified."""
    xs = rc.batch_inputs(scale, seed=up * 1000 + down)
    return xs, [rc.resample_ref(x, up, down) for x in xs]


@functools.lru_cache(maxsize=None)
def _batch_result(up, down, scale):
    from vaenmf.resample import resample_batch
    xs, _ = _case(up, down, scale)
    # rates with the ratio up / down (unreduced for 4/6: 4000 -> 6000 ... the library reduces by the gcd)
    y, counts = resample_batch(_cat(xs), rc.LENGTHS, 1000 * down, 1000 * up)
    return _split(y, counts), counts


@pytest.mark.parametrize("scale", rc.SCALES)
@pytest.mark.parametrize("up,down", rc.RATIOS)
def test_against_oracle(up, down, scale):
    """|y - float32(y_ref)| <= 2^-23 |y_ref| + 1e-12 max|x| for every sample of the ragged batch: one float32 rounding
    plus one flipped rounding, and the float64 sum-order and tap differences of about 60 products with |h| <= 1."""
    need_gpu()
    xs, refs = _case(up, down, scale)
    ys, counts = _batch_result(up, down, scale)
    ru, rd = rc.reduced(up, down)
    assert counts == [rc.out_length(n, ru, rd) for n in rc.LENGTHS]
    xmax = max(float(np.max(np.abs(x))) for x in xs if len(x))
    worst = 0.0
    for y, ref in zip(ys, refs):
        assert y.shape == ref.shape and y.dtype == np.float32
        if len(ref) == 0:
            continue
        err = np.abs(y.astype(np.float64) - ref.astype(np.float32).astype(np.float64))
        bound = 2.0 ** -23 * np.abs(ref) + 1e-12 * xmax
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (len(ref), float(np.max(err / bound)))
    print("resample %d/%d scale %g: worst error = %.3f of the bound" % (up, down, scale, worst))
    if up == down:
        assert all(np.array_equal(y, x) for y, x in zip(ys, xs))


@pytest.mark.parametrize("up,down", rc.RATIOS)
def test_batch_independence(up, down):
    """Every utterance resampled alone, and inside the reversed batch, has the bits it has in the batch."""
    need_gpu()
    from vaenmf.resample import resample_batch
    xs, _ = _case(up, down, 1.0)
    ys, _ = _batch_result(up, down, 1.0)
    for x, y in zip(xs, ys):
        alone, _ = resample_batch(_cat([x]), [len(x)], 1000 * down, 1000 * up)
        assert np.array_equal(alone.cpu().numpy().view(np.int32), y.view(np.int32)), len(x)
    yr, cr = resample_batch(_cat(xs[::-1]), rc.LENGTHS[::-1], 1000 * down, 1000 * up)
    for y, r in zip(ys, _split(yr, cr)[::-1]):
        assert np.array_equal(r.view(np.int32), y.view(np.int32))


def test_impulse_alignment():
    """x = delta at sample k: y[m] = float32(h[half + m down - k up]) exactly (zero where the index leaves the taps)."""
    need_gpu()
    from vaenmf.resample import resample, taps
    up, down, n = 2, 3, 50
    half = 10 * 3
    h = taps(up, down)
    for k in (0, 3, n - 1):
        x = np.zeros(n, np.float32)
        x[k] = 1.0
        y = resample(x, 3000, 2000)
        idx = half + np.arange(rc.out_length(n, up, down)) * down - k * up
        ok = (idx >= 0) & (idx <= 2 * half)
        want = np.where(ok, h[np.clip(idx, 0, 2 * half)], 0.0).astype(np.float32)
        assert y.dtype == np.float32 and np.array_equal(y, want), k
    t = resample(torch.from_numpy(x), 3000, 2000)                        # a tensor in, a tensor on its device out
    assert isinstance(t, torch.Tensor) and t.device.type == "cpu" and np.array_equal(t.numpy(), y)


@pytest.mark.parametrize("up,down", [(160, 441), (441, 160)])
def test_exact_buffers(up, down):
    """Input and output carved from a poisoned arena (exact extents, 16 mod 256 addresses): the guards stay intact and the
    output has the bits of the same call on ordinary buffers."""
    need_gpu()
    from vaenmf.resample import resample_batch
    xs, _ = _case(up, down, 1.0)
    ys, counts = _batch_result(up, down, 1.0)
    arena = Arena(1 << 20, "1e30", device="cuda")
    x = arena.carve("x", (sum(rc.LENGTHS),), torch.float32)
    x.copy_(_cat(xs))
    arena.snapshot(["x"])
    y, cg = resample_batch(x, rc.LENGTHS, 1000 * down, 1000 * up, out=lambda shape, dtype: arena.carve("y", shape, dtype))
    torch.cuda.synchronize()
    arena.check("resample %d/%d" % (up, down))
    arena.unchanged(what="resample %d/%d" % (up, down))
    assert cg == counts and arena.name_of(y) == "y"
    assert same_bits(y, torch.from_numpy(np.concatenate(ys)))


def test_refusals():
    need_gpu()
    from vaenmf._lib import lib
    from vaenmf.resample import resample_batch
    x = torch.zeros(100, device="cuda")
    y = torch.zeros(40, device="cuda")
    ioff = np.array([0, 60, 100], np.int64)
    for ooff in ([0, 20, 33], [0, 21, 34], [0, 20, 35]):                 # 60 -> 20 and 40 -> 14 at 1/3
        ooff = np.array(ooff, np.int64)
        code = lib().vaenmf_resample_batch(x.data_ptr(), 2, ioff.ctypes.data, ooff.ctypes.data, 1, 3, 10, 5.0, y.data_ptr(), None)
        assert code != 0 and b"out_offsets" in lib().vaenmf_last_error()
    ooff = np.array([0, 20, 34], np.int64)
    assert lib().vaenmf_resample_batch(x.data_ptr(), 2, ioff.ctypes.data, ooff.ctypes.data, 1, 3, 10, 5.0, y.data_ptr(), None) == 0
    assert lib().vaenmf_resample_batch(None, 0, None, None, 1, 3, 10, 5.0, None, None) == 0     # no utterances: a no-op
    torch.cuda.synchronize()
    with pytest.raises(NotImplementedError, match="1024"):
        resample_batch(x, [100], 16000, 16001)
    with pytest.raises(ValueError):
        resample_batch(x, [100], 44100.5, 16000)
    with pytest.raises(ValueError):
        resample_batch(x, [99], 48000, 16000)                            # counts that do not add up to the buffer


# ---------------------------------------------------------------------------------------------------------------------
# The enhancers and the file driver at another rate than the model's.  Smallest engine: F = 65 (8 ms at 16 kHz), rank 4
# ---------------------------------------------------------------------------------------------------------------------
F, K, WLEN = 65, 4, 8e-3
COUNTS48 = [4800, 3000]


def _reconstructor():
    from vaenmf.pipeline import Reconstructor
    params = orc.xavier_normal_params([F, 32, [128, 128]], seed=0)
    return Reconstructor(params, F, K, niter=2, nsamples_E_step=3, burnin_E_step=4, nsamples_WF=4, burnin_WF=5, reference_compat=False,
                         fs=16000, wlen_sec=WLEN, precision="bf16x3", max_frames=512, max_utts=4)


def _audio(counts, seed):
    g = np.random.default_rng(seed)
    return [(0.1 * g.standard_normal(n)).astype(np.float32) for n in counts]


def test_reconstructor_fs_in():
    need_gpu()
    from vaenmf.resample import crop_batch, resample_batch
    rec = _reconstructor()
    wav = _cat(_audio(COUNTS48, 3))
    seeds = [11, 12]
    s, n, cost = rec.enhance(wav, COUNTS48, seeds=seeds, init_seed=1, fs_in=48000)
    fc = list(rec.frame_counts)
    # (b) the input's lengths, finite
    assert s.shape == n.shape == wav.shape and bool(torch.isfinite(s).all()) and bool(torch.isfinite(n).all())
    assert float(s.abs().max()) > 0 and tuple(cost.shape) == (2, 2)
    # (a) the same steps by hand
    w16, c16 = resample_batch(wav, COUNTS48, 48000, 16000)
    assert c16 == [1600, 1000]
    s16, n16, cost16 = rec.enhance(w16, c16, seeds=seeds, init_seed=1)
    assert list(rec.frame_counts) == fc                                  # frame counts are the model rate's
    for got, at16 in ((s, s16), (n, n16)):
        up, cu = resample_batch(at16, c16, 16000, 48000)
        assert all(a >= b for a, b in zip(cu, COUNTS48))
        assert same_bits(got, crop_batch(up, cu, COUNTS48))
    assert same_bits(cost, cost16)
    # (c) fs_in = the model's rate is the present path
    a = rec.enhance(w16, c16, seeds=seeds, init_seed=1, fs_in=16000)
    b = rec.enhance(w16, c16, seeds=seeds, init_seed=1, fs_in=None)
    assert all(same_bits(p, q) for p, q in zip(a, b)) and same_bits(a[0], s16)


def test_mask_enhancer_fs_in():
    need_gpu()
    from vaenmf.pipeline import MaskEnhancer
    from vaenmf.resample import crop_batch, resample_batch
    g = np.random.default_rng(4)
    layers = [((g.standard_normal((F, F)) / 8).astype(np.float32), g.standard_normal(F).astype(np.float32))]   # one layer: the output's
    enh = MaskEnhancer(layers, F, wlen_sec=WLEN)
    wav = _cat(_audio(COUNTS48, 5))
    s, mask = enh.enhance(wav, COUNTS48, fs_in=48000)
    assert s.shape == wav.shape and bool(torch.isfinite(s).all()) and float(s.abs().max()) > 0
    w16, c16 = resample_batch(wav, COUNTS48, 48000, 16000)
    s16, mask16 = enh.enhance(w16, c16)
    up, cu = resample_batch(s16, c16, 16000, 48000)
    assert same_bits(s, crop_batch(up, cu, COUNTS48)) and same_bits(mask, mask16)
    assert mask.shape == (sum(enh.frame_counts), F)


def test_file_driver_mixed_rates(tmp_path):
    """driver.evaluate(resample=True) on files at 16, 44.1 and 48 kHz: each estimate is written at its file's rate and
    length; the 16 kHz file gets the bytes resample=False writes for it alone; without resample the tree is refused."""
    need_gpu()
    from vaenmf import wavio
    from vaenmf.driver import evaluate
    proc, out = str(tmp_path) + "/processed/", str(tmp_path) + "/out/"
    os.makedirs(proc + "d")
    spec = {"d/a": (16000, 4000), "d/b": (44100, 5003), "d/c": (48000, 6000)}
    for (name, (fs, T)), x in zip(spec.items(), _audio([T for _, T in spec.values()], 6)):
        wavio.write(proc + name + "_x.wav", x, fs)
    files = [name + ".wav" for name in spec]
    rec = _reconstructor()
    written = evaluate(rec, files, proc, out + "mixed/", batch_size=8, seed=2, resample=True)
    assert len(written) == 3
    for (sp, np_), (fs, T) in zip(written, spec.values()):
        for path in (sp, np_):
            y, fs_y = wavio.read(path)
            assert fs_y == fs and len(y) == T and np.all(np.isfinite(y))
        assert np.abs(wavio.read(sp)[0]).max() > 0
    alone = evaluate(rec, files[:1], proc, out + "alone/", batch_size=8, seed=2, resample=False)
    for mixed_path, alone_path in zip(written[0], alone[0]):
        assert open(mixed_path, "rb").read() == open(alone_path, "rb").read()
    with pytest.raises(ValueError, match="Unexpected sampling rate"):
        evaluate(rec, files, proc, out + "refused/", batch_size=8, seed=2)
    # M2 with oracle labels: the clean files take the same trip, the labels are those of the model rate
    from vaenmf.pipeline import Reconstructor
    from vaenmf.stft import frame_geometry
    for (name, (fs, T)), x in zip(spec.items(), _audio([T for _, T in spec.values()], 7)):
        wavio.write(proc + name + "_s.wav", x, fs)
    p2 = orc.xavier_normal_params([F, 32, [128, 128]], seed=1, y_dim=1)
    rec2 = Reconstructor(p2, F, K, niter=2, nsamples_E_step=3, burnin_E_step=4, nsamples_WF=4, burnin_WF=5, model="M2", fs=16000,
                         wlen_sec=WLEN, precision="bf16", max_frames=512, max_utts=4)
    kw = dict(batch_size=8, seed=2, label_source="oracle", label_type="vad")
    w2 = evaluate(rec2, files, proc, out + "m2/", resample=True, **kw)
    a2 = evaluate(rec2, files[:1], proc, out + "m2_alone/", **kw)
    for (sp, _), (fs, T) in zip(w2, spec.values()):
        y, fs_y = wavio.read(sp)
        assert fs_y == fs and len(y) == T and np.all(np.isfinite(y))
        hard = torch.load(sp[:-len("_s_est.wav")] + "_ibm_hard_est.pt", weights_only=True)
        assert hard.shape == (frame_geometry(-(-T * 16000 // fs), 16000, WLEN, 0.25)[2], 1)
    assert open(w2[0][0], "rb").read() == open(a2[0][0], "rb").read()
    stem, stem_a = w2[0][0][:-len("_s_est.wav")], a2[0][0][:-len("_s_est.wav")]
    assert torch.equal(torch.load(stem + "_ibm_hard_est.pt", weights_only=True), torch.load(stem_a + "_ibm_hard_est.pt", weights_only=True))
    wavio.write(proc + "d/b_s.wav", np.zeros(5003), 48000)               # a clean file at another rate than its mixture
    with pytest.raises(ValueError, match="sampling rate"):
        evaluate(rec2, files, proc, out + "m2_bad/", resample=True, **kw)
