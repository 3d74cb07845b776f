"""Segment-wise enhancement of long recordings on the GPU (csrc/segment.hip, vaenmf/longform.py, Reconstructor.em /
enhance_long, driver.evaluate(segment_sec=)): the two row kernels against numpy and on exact buffers, and the path itself
against the engine on hand-cut segments -- the only oracle there is for it.

Shapes: the F = 65 golden decoders (8 ms window, hop 32 at 16 kHz), rank 4, 3 EM iterations, L = 24 and V = 4 frames
(stride 20); recordings of 23, 24, 43, 44 and 97 frames: 1, 1, 1, 2 and 4 segments, the last of 37 frames."""
import functools
import os

import numpy as np
import pytest
import torch

from guarded import Arena, same_bits
from helpers import load_case, need_gpu

pytestmark = pytest.mark.gpu

FS, WLEN, HOP, K, NITER = 16000, 8e-3, 32, 4, 3
L, V = 24, 4
SEG_SEC, OVL_SEC = 24.5 * HOP / FS, 4.5 * HOP / FS                       # floor(sec fs / hop) = 24 and 4
FRAMES = [23, 24, 43, 44, 97]
SAMPLES = [680, 710, 1320, 1350, 3050]
SEEDS = [11, 12, 13, 14, 15]
EPS32 = 2.0 ** -23


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _i32(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy() if t.dtype == torch.float32 else t.detach().cpu().numpy().view(np.int64)


@functools.lru_cache(maxsize=None)
def _audio():
    """Seeded noise with a slow envelope, one array per recording; never modified."""
    from vaenmf.stft import frame_geometry
    g = np.random.default_rng(21)
    out = []
    for T, n in zip(SAMPLES, FRAMES):
        assert frame_geometry(T, FS, WLEN, 0.25)[1:3] == (HOP, n)
        out.append((0.1 * g.standard_normal(T) * (1.0 + 0.5 * np.sin(np.arange(T) / 200.0))).astype(np.float32))
    return out


def _wav(idx):
    return _cuda(np.concatenate([_audio()[i] for i in idx])), [SAMPLES[i] for i in idx]


@functools.lru_cache(maxsize=None)
def _rec(name="m1_f65", precision="bf16x3", max_frames=4096, max_utts=8):
    from vaenmf.pipeline import Reconstructor
    _, params, _, meta = load_case(name)
    assert meta["F"] == 65
    return Reconstructor(params, 65, K, niter=NITER, model="M2" if meta["Dy"] else "M1", fs=FS, wlen_sec=WLEN, precision=precision,
                         max_frames=max_frames, max_utts=max_utts)


# ---------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------
def _blend_case(rf, seed):
    """Segment rows [40][rf], a frame list mixing single owners and overlaps with the weights of V = 1, 2, 4, 7."""
    g = np.random.default_rng(seed)
    seg = g.standard_normal((40, rf)).astype(np.float32)
    ra = g.integers(0, 40, size=60).astype(np.int32)
    rb = g.integers(0, 40, size=60).astype(np.int32)
    w = np.zeros(60, np.float32)
    for t in range(60):
        if t % 3 == 0:
            rb[t] = -1
        else:
            v = (1, 2, 4, 7)[t % 4]
            w[t] = np.float32((g.integers(0, v) + 1) / (v + 1))
    return seg, ra, rb, w


@pytest.mark.parametrize("rf", [1, 3, 65, 130, 544])
def test_gather_rows(rf):
    need_gpu()
    from vaenmf.longform import gather_rows
    g = np.random.default_rng(rf)
    src = g.standard_normal((50, rf)).astype(np.float32)
    src[7] = np.nan                                                      # rows are moved, not computed on
    rmap = np.concatenate([g.integers(0, 50, size=300), [7, 7, 49, 0, 0]]).astype(np.int32)   # repeats; more rows than one workgroup holds
    got = gather_rows(_cuda(src), _cuda(rmap))
    assert got.shape == (305, rf) and np.array_equal(_i32(got), src[rmap].view(np.int32))
    shaped = gather_rows(_cuda(src.reshape(50, rf, 1)), _cuda(rmap))     # trailing dimensions are one row
    assert shaped.shape == (305, rf, 1) and np.array_equal(_i32(shaped).reshape(305, rf), src[rmap].view(np.int32))


@pytest.mark.parametrize("rf", [1, 3, 65, 130, 544])
def test_blend_rows(rf):
    """One owner: the source row's bits.  Overlap: |out - (w_a a + w_b b)| <= 1.01 2^-23 (|w_a a| + |w_b b|) per float, w_a =
    1.0f - w_b in float32 -- each product within 2^-24 of itself, the sum within 2^-24 of (|w_a a| + |w_b b|) (1 + 2^-24).
    Derived, not measured."""
    need_gpu()
    from vaenmf.longform import blend_rows
    seg, ra, rb, w = _blend_case(rf, 100 + rf)
    got = blend_rows(_cuda(seg), _cuda(ra), _cuda(rb), _cuda(w)).cpu().numpy()
    one = rb < 0
    assert np.array_equal(got[one].view(np.int32), seg[ra[one]].view(np.int32))
    wa = (np.float32(1.0) - w[~one]).astype(np.float64)[:, None]
    wb = w[~one].astype(np.float64)[:, None]
    a, b = seg[ra[~one]].astype(np.float64), seg[rb[~one]].astype(np.float64)
    err = np.abs(got[~one].astype(np.float64) - (wa * a + wb * b))
    bound = 1.01 * EPS32 * (np.abs(wa * a) + np.abs(wb * b))
    print("blend rf=%d: worst error = %.3f of the bound" % (rf, float(np.max(err / bound))))
    assert np.all(err <= bound)
    # the roles swapped, the weight replaced by its complement: the same bits where 1 - (1 - w) == w
    wc = (np.float32(1.0) - w).astype(np.float32)
    ra2, rb2, w2 = np.where(one, ra, rb).astype(np.int32), np.where(one, -1, ra).astype(np.int32), np.where(one, 0, wc).astype(np.float32)
    swapped = blend_rows(_cuda(seg), _cuda(ra2), _cuda(rb2), _cuda(w2)).cpu().numpy()
    exact = one | ((np.float32(1.0) - wc) == w)
    assert (exact & ~one).sum() >= 10
    assert np.array_equal(swapped[exact].view(np.int32), got[exact].view(np.int32))


def test_empty_calls():
    need_gpu()
    from vaenmf._lib import lib
    from vaenmf.longform import blend_rows, gather_rows
    assert lib().vaenmf_gather_rows(None, None, 0, 65, None, None) == 0
    assert lib().vaenmf_blend_rows(None, None, None, None, 0, 65, None, None) == 0
    src, none = torch.ones(4, 65, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda")
    assert gather_rows(src, none).shape == (0, 65)
    assert blend_rows(src, none, none, torch.zeros(0, device="cuda")).shape == (0, 65)
    assert lib().vaenmf_gather_rows(src.data_ptr(), None, 3, 65, src.data_ptr(), None) != 0      # rows to move, no map


@pytest.mark.parametrize("poison", ["nan", "1e30"])
@pytest.mark.parametrize("rf", [65, 130, 544])
def test_exact_buffers(rf, poison):
    """Every buffer of both kernels carved from a poisoned arena (exact extents, addresses = 16 mod 256; 544 floats: the
    16-byte accesses, 65 and 130: float by float): the guards stay intact, the inputs unchanged, the outputs have the bits
    of the same calls on ordinary buffers."""
    need_gpu()
    from vaenmf.longform import blend_rows, gather_rows
    seg, ra, rb, w = _blend_case(rf, 200 + rf)
    rmap = np.random.default_rng(rf).integers(0, 40, size=70).astype(np.int32)
    want_g = gather_rows(_cuda(seg), _cuda(rmap))
    want_b = blend_rows(_cuda(seg), _cuda(ra), _cuda(rb), _cuda(w))
    arena = Arena(4 << 20, poison, device="cuda")
    bufs = {}
    for name, host in (("seg", seg), ("map", rmap), ("row_a", ra), ("row_b", rb), ("w_b", w)):
        bufs[name] = arena.carve(name, host.shape, torch.from_numpy(host).dtype)
        bufs[name].copy_(torch.from_numpy(host))
    out_g = arena.carve("gathered", (70, rf), torch.float32)
    out_b = arena.carve("blended", (60, rf), torch.float32)
    arena.snapshot(list(bufs))
    gather_rows(bufs["seg"], bufs["map"], out=out_g)
    blend_rows(bufs["seg"], bufs["row_a"], bufs["row_b"], bufs["w_b"], out=out_b)
    torch.cuda.synchronize()
    arena.check("rows of %d floats" % rf)
    arena.unchanged(what="rows of %d floats" % rf)
    assert same_bits(out_g, want_g) and same_bits(out_b, want_b)


# ---------------------------------------------------------------------------------------------------------------------
# the path
# ---------------------------------------------------------------------------------------------------------------------
def _labels(n_frames, seed=5):
    g = np.random.default_rng(seed)
    return _cuda((g.random((n_frames, 1)) > 0.4).astype(np.float32))


@pytest.mark.parametrize("name,precision", [("m1_f65", "bf16"), ("m1_f65", "bf16x3"), ("m2_vad_f65", "bf16x3")])
def test_single_segments_are_enhance(name, precision):
    """Recordings of 23, 24 and 43 frames (< L + stride = 44) are one segment each: the bits of enhance()."""
    need_gpu()
    rec = _rec(name, precision)
    wav, counts = _wav([0, 1, 2])
    y = _labels(sum(FRAMES[:3])) if rec.model == "M2" else None
    s0, n0, c0 = rec.enhance(wav, counts, seeds=SEEDS[:3], init_seed=2, y=y)
    s1, n1, c1 = rec.enhance_long(wav, counts, SEG_SEC, OVL_SEC, seeds=SEEDS[:3], init_seed=2, y=y)
    assert list(rec.frame_counts) == FRAMES[:3] and list(rec.segments.seg_len) == FRAMES[:3]
    assert float(s0.abs().max()) > 0 and bool(torch.isfinite(s0).all())
    assert same_bits(s1, s0) and same_bits(n1, n0)
    assert len(c1) == 3 and all(c.shape == (1, NITER) for c in c1) and same_bits(torch.cat(c1), c0)
    # without seeds: what bind() gives recording i
    s2 = rec.enhance(wav, counts, init_seed=2, y=y)[0]
    s3 = rec.enhance_long(wav, counts, SEG_SEC, OVL_SEC, init_seed=2, y=y)[0]
    assert same_bits(s3, s2) and not same_bits(s2, s0)


@functools.lru_cache(maxsize=None)
def _five(max_utts=8, max_frames=4096):
    """enhance_long of the five-recording batch on an engine of the given capacity: host copies of every output."""
    rec = _rec("m1_f65", "bf16x3", max_frames, max_utts)
    wav, counts = _wav(range(5))
    s, n, cost = rec.enhance_long(wav, counts, SEG_SEC, OVL_SEC, seeds=SEEDS, init_seed=3)
    assert list(rec.frame_counts) == FRAMES
    return dict(s=s.cpu(), n=n.cpu(), cost=[c.cpu() for c in cost], S=rec.S_frames.cpu(), N=rec.N_frames.cpu(), tab=rec.segments,
                rounds=dict(rec.long_rounds))


def _cut(X, tab):
    """The segments' rows of recording-order rows X, sliced one segment at a time, in the table's order."""
    off = np.concatenate([[0], np.cumsum(tab.frame_counts)])
    return torch.cat([X[off[u] + f:off[u] + f + n] for u, f, n in zip(tab.seg_utt, tab.seg_first, tab.seg_len)])


def test_segments_are_plain_utterances():
    """The segments cut by slicing, run as ONE em() batch with segment_seeds, blended in float64: enhance_long's frames
    are those bits where a frame has one owner and within the blend's bound in the overlaps; its waveform is the iSTFT of
    its frames; its costs are the segments' costs."""
    need_gpu()
    from vaenmf import longform as lf
    from vaenmf.stft import istft_batch, stft_batch
    got = _five()
    tab = got["tab"]
    assert list(tab.seg_len) == [24, 24, 24, 24, 23, 24, 43, 24, 37] and (tab.L, tab.V) == (L, V)
    rec = _rec("m1_f65", "bf16x3", 4096, 16)                             # an engine that holds the nine segments at once
    wav, counts = _wav(range(5))
    X, fc = stft_batch(wav, counts, FS, WLEN, 0.25, Fs=rec.eng.Fs)
    assert fc == FRAMES
    S, N, cost = rec.em(_cut(X, tab), [int(v) for v in tab.seg_len], seeds=lf.segment_seeds(SEEDS, tab), init_seed=3)
    one = tab.row_b < 0
    rb = np.where(one, 0, tab.row_b)
    wa = (np.float32(1.0) - tab.w_b).astype(np.float64)[:, None, None]
    wb = tab.w_b.astype(np.float64)[:, None, None]
    assert (~one).sum() == 4 * V
    for name, seg in (("S", S), ("N", N)):
        seg = seg.cpu().numpy()
        frames = got[name].numpy()
        assert np.array_equal(frames[one].view(np.int32), seg[tab.row_a[one]].view(np.int32)), name
        a, b = seg[tab.row_a].astype(np.float64), seg[rb].astype(np.float64)
        err = np.abs(frames.astype(np.float64) - (wa * a + wb * b))[~one]
        bound = (1.01 * EPS32 * (np.abs(wa * a) + np.abs(wb * b)))[~one]
        assert np.all(err <= bound), (name, float(np.max(err / np.maximum(bound, 1e-300))))
        assert float(np.abs(frames[~one]).max()) > 0
    assert same_bits(got["s"], istft_batch(got["S"].cuda(), FRAMES, counts, 128, HOP))
    assert same_bits(got["n"], istft_batch(got["N"].cuda(), FRAMES, counts, 128, HOP))
    assert got["s"].shape == (sum(SAMPLES),) and bool(torch.isfinite(got["s"]).all()) and bool(torch.isfinite(got["n"]).all())
    cost = cost.cpu()
    assert [tuple(c.shape) for c in got["cost"]] == [(1, NITER), (1, NITER), (1, NITER), (2, NITER), (4, NITER)]
    for p, (u, j) in enumerate(zip(tab.seg_utt, tab.seg_index)):
        assert same_bits(got["cost"][u][j], cost[p]), (u, j)
    assert got["rounds"]["rounds"] == 2                                  # the four L-frame segments, then the five last ones


@pytest.mark.parametrize("max_utts,max_frames,rounds", [(2, 4096, 5), (8, 44, 9), (2, 44, 9)])
def test_packing_does_not_show(max_utts, max_frames, rounds):
    """Engines of max_utts 2 and 8, max_frames 44 and 4096 (the fourth, 8 and 4096, is the one every other test uses)."""
    need_gpu()
    want, got = _five(), _five(max_utts, max_frames)
    assert got["rounds"]["rounds"] == rounds
    for k in ("s", "n", "S", "N"):
        assert same_bits(got[k], want[k]), k
    assert all(same_bits(a, b) for a, b in zip(got["cost"], want["cost"]))


def test_over_capacity():
    """97 frames on an engine of 44: enhance() refuses, enhance_long() runs the four segments one per round."""
    need_gpu()
    from vaenmf._lib import VaenmfError
    rec = _rec("m1_f65", "bf16x3", 44, 8)
    wav, counts = _wav([4])
    with pytest.raises(VaenmfError, match="total frames 97 exceeds capacity 44"):
        rec.enhance(wav, counts, seeds=SEEDS[4:], init_seed=3)
    s, n, cost = rec.enhance_long(wav, counts, SEG_SEC, OVL_SEC, seeds=SEEDS[4:], init_seed=3)
    assert s.shape == n.shape == (SAMPLES[4],) and bool(torch.isfinite(s).all()) and bool(torch.isfinite(n).all())
    assert float(s.abs().max()) > 0 and cost[0].shape == (4, NITER) and rec.long_rounds["rounds"] == 4
    want = _five()                                                       # and a recording does not depend on its batch
    assert same_bits(s.cpu(), want["s"][sum(SAMPLES[:4]):]) and same_bits(cost[0], want["cost"][4])
    with pytest.raises(ValueError, match="43.*max_frames=42"):
        _rec("m1_f65", "bf16x3", 42, 8).enhance_long(wav, counts, SEG_SEC, OVL_SEC)
    with pytest.raises(ValueError, match="half"):
        rec.enhance_long(wav, counts, SEG_SEC, 0.6 * SEG_SEC)
    with pytest.raises(ValueError, match="L=1 "):
        rec.enhance_long(wav, counts, 1.5 * HOP / FS, 0.0)


def test_any_rate():
    need_gpu()
    from vaenmf.resample import crop_batch, resample_batch
    rec = _rec()
    g = np.random.default_rng(8)
    T48 = 3 * SAMPLES[3] - 1                                             # ceil(T48 / 3) = 1350 samples at 16 kHz: 44 frames, 2 segments
    wav = _cuda((0.1 * g.standard_normal(T48)).astype(np.float32))
    s, n, cost = rec.enhance_long(wav, [T48], SEG_SEC, OVL_SEC, seeds=[7], init_seed=1, fs_in=48000)
    assert s.shape == n.shape == (T48,) and list(rec.frame_counts) == [44] and cost[0].shape == (2, NITER)
    w16, c16 = resample_batch(wav, [T48], 48000, FS)
    assert c16 == [SAMPLES[3]]
    s16, n16, cost16 = rec.enhance_long(w16, c16, SEG_SEC, OVL_SEC, seeds=[7], init_seed=1)
    for got, at16 in ((s, s16), (n, n16)):
        up, cu = resample_batch(at16, c16, FS, 48000)
        assert same_bits(got, crop_batch(up, cu, [T48]))
    assert same_bits(cost[0], cost16[0]) and float(s.abs().max()) > 0


def _classifier(seed=9):
    g = np.random.default_rng(seed)
    return [((g.standard_normal((16, 65)) / 4).astype(np.float32), g.standard_normal(16).astype(np.float32)),
            ((g.standard_normal((1, 16)) / 2).astype(np.float32), np.zeros(1, np.float32))]


def test_classifier_labels():
    """y_soft / y_hard come back in recording order: per frame the value of the segment with the larger weight, the earlier
    one on a tie, taken from the per-segment labels of a hand-cut em() batch."""
    need_gpu()
    from vaenmf import longform as lf
    from vaenmf.stft import stft_batch
    rec = _rec("m2_vad_f65", "bf16x3")
    clf = _classifier()
    wav, counts = _wav(range(5))
    s, n, _ = rec.enhance_long(wav, counts, SEG_SEC, OVL_SEC, seeds=SEEDS, init_seed=3, classifier=clf)
    tab, soft, hard = rec.segments, rec.y_soft.cpu(), rec.y_hard.cpu()
    assert soft.shape == hard.shape == (sum(FRAMES), 1) and bool(torch.isfinite(s).all())
    assert set(np.unique(hard.numpy())) <= {0.0, 1.0} and len(np.unique(soft.numpy())) > sum(FRAMES) // 2
    X, _ = stft_batch(wav, counts, FS, WLEN, 0.25, Fs=rec.eng.Fs)
    rec = _rec("m2_vad_f65", "bf16x3", 4096, 16)                         # an engine that holds the nine segments at once
    rec.em(_cut(X, tab), [int(v) for v in tab.seg_len], seeds=lf.segment_seeds(SEEDS, tab), init_seed=3, classifier=clf)
    seg_soft, seg_hard = rec.y_soft.cpu(), rec.y_hard.cpu()
    own = np.array([b if (b >= 0 and w > np.float32(1.0) - w) else a for a, b, w in zip(tab.row_a, tab.row_b, tab.w_b)])
    assert (own != tab.row_a).sum() == 4 * (V // 2)                      # weights 0.2, 0.4 | 0.6, 0.8
    assert same_bits(soft, seg_soft[own]) and same_bits(hard, seg_hard[own])


def test_file_driver(tmp_path):
    """evaluate(segment_sec=) writes the files evaluate() writes, at the same lengths, with enhance_long's contents."""
    need_gpu()
    from vaenmf import wavio
    from vaenmf.driver import evaluate
    proc, out = str(tmp_path) + "/processed/", str(tmp_path) + "/out/"
    os.makedirs(proc + "d")
    files = ["d/a.wav", "d/b.wav"]
    for fp, i in zip(files, (3, 4)):
        wavio.write(proc + fp[:-4] + "_x.wav", _audio()[i], FS)
    rec, clf = _rec("m2_vad_f65", "bf16x3"), _classifier()
    plain = evaluate(rec, files, proc, out + "plain/", seed=2, classifier=clf, label_type="vad")
    longf = evaluate(rec, files, proc, out + "long/", seed=2, classifier=clf, label_type="vad", segment_sec=SEG_SEC, overlap_sec=OVL_SEC)
    rel = lambda root: sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)
    assert rel(out + "plain/") == rel(out + "long/") and len(rel(out + "long/")) == 8
    assert [tuple(os.path.relpath(p, out + "long/") for p in w) for w in longf] == [tuple(os.path.relpath(p, out + "plain/") for p in w) for w in plain]
    wavs = [wavio.read(proc + fp[:-4] + "_x.wav")[0].astype(np.float32) for fp in files]
    s, n, _ = rec.enhance_long(_cuda(np.concatenate(wavs)), [len(w) for w in wavs], SEG_SEC, OVL_SEC, seeds=[2 * 1000003, 2 * 1000003 + 1],
                               init_seed=2, classifier=clf)
    assert [int(m) for m in np.bincount(rec.segments.seg_utt)] == [2, 4]
    soff, foff = np.concatenate([[0], np.cumsum([len(w) for w in wavs])]), np.concatenate([[0], np.cumsum(rec.frame_counts)])
    for i, ((sp, npth), (sp0, np0)) in enumerate(zip(longf, plain)):
        for path, path0, est in ((sp, sp0, s), (npth, np0, n)):
            y, fs = wavio.read(path)
            assert fs == FS and len(y) == len(wavs[i]) == len(wavio.read(path0)[0])
            wavio.write(str(tmp_path) + "/want.wav", est[soff[i]:soff[i + 1]].cpu().numpy(), FS)
            assert open(path, "rb").read() == open(str(tmp_path) + "/want.wav", "rb").read()
        stem, stem0 = sp[:-len("_s_est.wav")], sp0[:-len("_s_est.wav")]
        for tail, lab in ((" _ibm_soft_est.pt", rec.y_soft), ("_ibm_hard_est.pt", rec.y_hard)):
            t = torch.load(stem + tail, weights_only=True)
            assert t.shape == torch.load(stem0 + tail, weights_only=True).shape == (rec.frame_counts[i], 1)
            assert same_bits(t, lab[foff[i]:foff[i + 1]].cpu())
    assert open(longf[1][0], "rb").read() != open(plain[1][0], "rb").read()      # four segments are not one utterance
