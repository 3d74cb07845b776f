"""Recordings of any length: segment-wise EM with blended seams (csrc/segment.hip).

A recording is cut on the STFT frame grid into segments of L frames that overlap by V frames (the rule: include/vaenmf.h,
DESIGN 3.5c); every segment is an utterance of the EM engine, many of one shape per launch; the Wiener-filtered rows of
neighbouring segments are blended across their overlap.  One STFT and one iSTFT per recording: no segment sees a
reflect-padded edge in the middle of a recording.  Segments are independent EM problems -- own NMF dictionary, own noise
streams, no state carried across a seam -- so a recording's result does not depend on how its segments were packed."""
import ctypes as C
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from . import stft as vstft
from ._lib import check, lib
from .engine import _ptr, _stream
from .resample import crop_batch, resample_batch

M64 = (1 << 64) - 1

SegmentTable = namedtuple("SegmentTable", "L V frame_counts seg_utt seg_index seg_first seg_len seg_row src_row row_a row_b w_b")
SegmentTable.__doc__ = """Host arrays of vaenmf_segment_table, segments in processing order.  seg_row [n_segments + 1]: first
segment row of every segment (the cumulative sum of seg_len); the other fields as the header names them."""


def splitmix64(z):
    z = (int(z) + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def default_seeds(n_utt):
    """The seeds vaenmf_bind_batch gives utterances 0 .. n_utt-1 when the caller passes none."""
    return [splitmix64(0x5EED + u) for u in range(int(n_utt))]


def segment_table(frame_counts, L, V, max_frames):
    """SegmentTable of a batch of recordings; ValueError (with the numbers) for what vaenmf_segment_table refuses."""
    fc = np.ascontiguousarray(np.asarray(frame_counts, dtype=np.int32).reshape(-1))
    ns, nr = C.c_int64(), C.c_int64()
    if lib().vaenmf_segment_count(len(fc), fc.ctypes.data, int(L), int(V), C.byref(ns), C.byref(nr)) != 0:
        raise ValueError(lib().vaenmf_last_error().decode())
    i32 = lambda n: np.empty(n, np.int32)
    NT = int(fc.sum())
    su, sj, s0, sl, src = i32(ns.value), i32(ns.value), i32(ns.value), i32(ns.value), i32(nr.value)
    ra, rb, wb = i32(NT), i32(NT), np.empty(NT, np.float32)
    if lib().vaenmf_segment_table(len(fc), fc.ctypes.data, int(L), int(V), int(min(int(max_frames), 2 ** 31 - 1)), su.ctypes.data,
                                  sj.ctypes.data, s0.ctypes.data, sl.ctypes.data, src.ctypes.data, ra.ctypes.data, rb.ctypes.data,
                                  wb.ctypes.data) != 0:
        raise ValueError(lib().vaenmf_last_error().decode())
    row = np.concatenate([[0], np.cumsum(sl, dtype=np.int64)])
    return SegmentTable(int(L), int(V), [int(n) for n in fc], su, sj, s0, sl, row, src, ra, rb, wb)


def segment_seeds(seeds, table):
    """Per-segment seeds in the table's processing order (list of Python ints below 2^64): segment 0 of recording i runs with
    seeds[i] itself, segment j >= 1 with splitmix64(seeds[i] ^ splitmix64(j)).  The chain's stream key XORs the seed with
    small frame / sub-stream / call fields: seeds that differ in a few low bits would share streams, hence the mixing."""
    sd = [int(s) & M64 for s in seeds]
    return [sd[u] if j == 0 else splitmix64(sd[u] ^ splitmix64(int(j))) for u, j in zip(table.seg_utt, table.seg_index)]


def pack_rounds(table, max_utts, max_frames):
    """[(first segment, one past the last)] of the rounds, over the processing order: the L-frame segments that are not their
    recording's last in rounds of B = min(max_utts, max_frames // L) (every full round has one frame structure), then the
    last segments packed greedily in order, at most max_utts segments and max_frames frames a round."""
    n_seg, n_first = len(table.seg_len), len(table.seg_len) - len(table.frame_counts)
    B = max(1, min(int(max_utts), int(max_frames) // table.L))
    rounds = [(p, min(p + B, n_first)) for p in range(0, n_first, B)]
    p = n_first
    while p < n_seg:
        q, frames = p, 0
        while q < n_seg and q - p < int(max_utts) and frames + int(table.seg_len[q]) <= int(max_frames):
            frames += int(table.seg_len[q])
            q += 1
        if q == p:
            raise ValueError("a segment of %d frames does not fit an engine of max_frames=%d" % (int(table.seg_len[p]), int(max_frames)))
        rounds.append((p, q))
        p = q
    return rounds


def owner_rows(table):
    """Per recording-order frame the segment row whose value stands for the frame where values are not blended (labels):
    the segment with the larger weight, the earlier one on a tie."""
    later = (table.row_b >= 0) & (table.w_b > np.float32(1.0) - table.w_b)
    return np.where(later, table.row_b, table.row_a).astype(np.int32)


def gather_rows(src, row_map, out=None):
    """dst[r] = src[row_map[r]]: src device float32 [rows, ...] (dense), row_map device int32 [n]; returns [n, ...]."""
    if src.dtype != torch.float32 or row_map.dtype != torch.int32:
        raise ValueError("gather_rows takes float32 rows and an int32 map, got %s and %s" % (src.dtype, row_map.dtype))
    n, rf = int(row_map.shape[0]), int(np.prod(src.shape[1:], dtype=np.int64))
    dst = torch.empty((n,) + tuple(src.shape[1:]), device=src.device, dtype=torch.float32) if out is None else out
    check(lib().vaenmf_gather_rows(_ptr(src), _ptr(row_map), n, rf, _ptr(dst), _stream()))
    return dst


def blend_rows(seg, row_a, row_b, w_b, out=None):
    """dst[t] = seg[row_a[t]] where row_b[t] < 0, else (1 - w_b[t]) seg[row_a[t]] + w_b[t] seg[row_b[t]] (vaenmf_blend_rows)."""
    if seg.dtype != torch.float32 or row_a.dtype != torch.int32 or row_b.dtype != torch.int32 or w_b.dtype != torch.float32:
        raise ValueError("blend_rows takes float32 rows and weights and int32 row indices")
    n, rf = int(row_a.shape[0]), int(np.prod(seg.shape[1:], dtype=np.int64))
    if int(row_b.shape[0]) != n or int(w_b.shape[0]) != n:
        raise ValueError("row_a, row_b and w_b differ in length")
    dst = torch.empty((n,) + tuple(seg.shape[1:]), device=seg.device, dtype=torch.float32) if out is None else out
    check(lib().vaenmf_blend_rows(_ptr(seg), _ptr(row_a), _ptr(row_b), _ptr(w_b), n, rf, _ptr(dst), _stream()))
    return dst


def segment_frames(rec, segment_sec, overlap_sec, hop):
    """(L, V) = floor(seconds * fs / hop) frames on a Reconstructor's frame grid; ValueError for what cannot run."""
    if not (segment_sec > 0 and overlap_sec >= 0):
        raise ValueError("segment_sec=%r, overlap_sec=%r: a positive length and a non-negative overlap" % (segment_sec, overlap_sec))
    if overlap_sec > segment_sec / 2:
        raise ValueError("overlap_sec=%g exceeds half of segment_sec=%g" % (overlap_sec, segment_sec))
    L, V = int(math.floor(segment_sec * rec.fs / hop)), int(math.floor(overlap_sec * rec.fs / hop))
    if L < 2:
        raise ValueError("segment_sec=%g is L=%d frames at a hop of %d samples: at least 2 frames" % (segment_sec, L, hop))
    mf = rec.eng._max_frames
    if 2 * L - V - 1 > mf:
        raise ValueError("segments of L=%d frames with an overlap of V=%d run up to L + stride - 1 = %d frames; the engine holds "
                         "max_frames=%d" % (L, V, 2 * L - V - 1, mf))
    return L, V


def enhance_long(rec, wav, sample_counts, segment_sec=30.0, overlap_sec=2.0, seeds=None, init_seed=0, y=None, classifier=None,
                 mean=None, std=None, fs_in=None):
    """Reconstructor.enhance_long (pipeline.py): see there."""
    if fs_in is not None and fs_in != rec.fs:
        wav_m, counts_m = resample_batch(wav, sample_counts, fs_in, rec.fs, device=rec.device)
        s_hat, n_hat, cost = enhance_long(rec, wav_m, counts_m, segment_sec, overlap_sec, seeds=seeds, init_seed=init_seed, y=y,
                                          classifier=classifier, mean=mean, std=std)
        s_hat, back = resample_batch(s_hat, counts_m, rec.fs, fs_in, device=rec.device)
        n_hat, _ = resample_batch(n_hat, counts_m, rec.fs, fs_in, device=rec.device)
        return crop_batch(s_hat, back, sample_counts), crop_batch(n_hat, back, sample_counts), cost
    eng, dev = rec.eng, rec.device
    nfft, hop = vstft.frame_geometry(sample_counts[0], rec.fs, rec.wlen_sec, rec.hop_percent)[:2]
    L, V = segment_frames(rec, segment_sec, overlap_sec, hop)
    X, fc = vstft.stft_batch(wav, sample_counts, rec.fs, rec.wlen_sec, rec.hop_percent, Fs=eng.Fs, device=dev)
    tab = segment_table(fc, L, V, eng._max_frames)
    sseeds = segment_seeds(default_seeds(len(fc)) if seeds is None else seeds, tab)
    rounds = pack_rounds(tab, eng._max_utts, eng._max_frames)
    n_rows, NT = int(tab.seg_row[-1]), int(sum(fc))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_src, d_ra, d_rb, d_wb = up(tab.src_row), up(tab.row_a), up(tab.row_b), up(tab.w_b)
    if y is not None:
        y = y.to(dev, torch.float32).contiguous()
        if y.dim() != 2 or y.shape[0] != NT:
            raise ValueError("y must be [NT = %d, Dy] in recording frame order, got %s" % (NT, tuple(y.shape)))
    S_seg = torch.empty(n_rows, eng.Fs, 2, device=dev, dtype=torch.float32)
    N_seg = torch.empty(n_rows, eng.Fs, 2, device=dev, dtype=torch.float32)
    ys_seg = yh_seg = None
    costs, graphs = [], 0
    for p0, p1 in rounds:
        r0, r1 = int(tab.seg_row[p0]), int(tab.seg_row[p1])
        Xr = gather_rows(X, d_src[r0:r1])
        yr = None if y is None else gather_rows(y, d_src[r0:r1])
        S, N, cost = rec.em(Xr, [int(n) for n in tab.seg_len[p0:p1]], seeds=sseeds[p0:p1], init_seed=init_seed, y=yr,
                            classifier=classifier, mean=mean, std=std)
        graphs += int(lib().vaenmf_plan_query(eng._plan, _lib.Q_EM_GRAPH) == 1)
        S_seg[r0:r1].copy_(S)
        N_seg[r0:r1].copy_(N)
        costs.append(cost)
        if classifier is not None:
            if ys_seg is None:
                ys_seg = torch.empty(n_rows, rec.y_soft.shape[1], device=dev, dtype=torch.float32)
                yh_seg = torch.empty_like(ys_seg)
            ys_seg[r0:r1].copy_(rec.y_soft)
            yh_seg[r0:r1].copy_(rec.y_hard)
    rec.S_frames = blend_rows(S_seg, d_ra, d_rb, d_wb)
    rec.N_frames = blend_rows(N_seg, d_ra, d_rb, d_wb)
    if classifier is not None:
        d_own = up(owner_rows(tab))
        rec.y_soft, rec.y_hard = gather_rows(ys_seg, d_own), gather_rows(yh_seg, d_own)
    s_hat = vstft.istft_batch(rec.S_frames, fc, sample_counts, nfft, hop, device=dev)
    n_hat = vstft.istft_batch(rec.N_frames, fc, sample_counts, nfft, hop, device=dev)
    # cost rows back per recording, in segment order: [m_i, niter] each
    cost_all = torch.cat(costs)
    pos = np.lexsort((tab.seg_index, tab.seg_utt))
    m = np.bincount(tab.seg_utt, minlength=len(fc))
    cost_rec = list(torch.split(cost_all[torch.from_numpy(pos).to(dev)], [int(v) for v in m]))
    rec.frame_counts, rec.segments = fc, tab
    rec.long_rounds = {"rounds": len(rounds), "graph_rounds": graphs}
    return s_hat, n_hat, cost_rec
