"""Host side of segment-wise enhancement (csrc/segment.hip: vaenmf_segment_count / vaenmf_segment_table; vaenmf/longform.py:
segment_seeds, pack_rounds, owner_rows) against the segment rule restated here; no GPU."""
import ctypes as C

import numpy as np
import pytest

from vaenmf import _lib
from vaenmf import longform as lf

BIG = 1 << 30


def rule(n, L, V):
    """[(first frame, length)] of the segments of a recording of n frames, as the issue states the rule."""
    stride = L - V
    m = max(1, (n - V) // stride)
    return [(k * stride, L if k < m - 1 else n - k * stride) for k in range(m)]


def expected(counts, L, V):
    """The whole table of a batch, built from rule() alone: dict of arrays named as the fields of SegmentTable."""
    segs = [rule(n, L, V) for n in counts]
    off = np.concatenate([[0], np.cumsum(counts)])
    order = [(u, j) for u, s in enumerate(segs) for j in range(len(s) - 1)] + [(u, len(s) - 1) for u, s in enumerate(segs)]
    row0, src, r = {}, [], 0
    for u, j in order:
        first, ln = segs[u][j]
        row0[(u, j)] = r
        src += [off[u] + first + i for i in range(ln)]
        r += ln
    NT = int(off[-1])
    ra, rb, wb = np.empty(NT, np.int32), np.full(NT, -1, np.int32), np.zeros(NT, np.float32)
    for u, s in enumerate(segs):
        owners = [[] for _ in range(counts[u])]
        for j, (first, ln) in enumerate(s):
            for i in range(ln):
                owners[first + i].append((j, i))
        for t, own in enumerate(owners):
            assert 1 <= len(own) <= 2, (counts[u], L, V, t)                 # every frame covered once or twice
            ra[off[u] + t] = row0[(u, own[0][0])] + own[0][1]
            if len(own) == 2:
                assert own[1][0] == own[0][0] + 1 and own[1][1] < V      # consecutive segments, inside the later one's first V
                rb[off[u] + t] = row0[(u, own[1][0])] + own[1][1]
                wb[off[u] + t] = np.float32((own[1][1] + 1) / (V + 1))
    return dict(seg_utt=[u for u, _ in order], seg_index=[j for _, j in order], seg_first=[segs[u][j][0] for u, j in order],
                seg_len=[segs[u][j][1] for u, j in order], src_row=src, row_a=ra, row_b=rb, w_b=wb)


def check_table(counts, L, V):
    tab = lf.segment_table(counts, L, V, BIG)
    exp = expected(counts, L, V)
    for k, v in exp.items():
        got = getattr(tab, k)
        if k == "w_b":
            assert np.array_equal(got.view(np.int32), np.asarray(v, np.float32).view(np.int32)), (counts, L, V, k)
        else:
            assert np.array_equal(got, np.asarray(v)), (counts, L, V, k)
    ns, nr = C.c_int64(), C.c_int64()
    fc = np.asarray(counts, np.int32)
    assert _lib.lib().vaenmf_segment_count(len(fc), fc.ctypes.data, L, V, C.byref(ns), C.byref(nr)) == 0
    assert (ns.value, nr.value) == (len(tab.seg_len), len(tab.src_row)) and nr.value == int(tab.seg_row[-1])
    return tab


def check_properties(tab):
    """What the rule promises, read off the library's own table."""
    L, V, stride = tab.L, tab.V, tab.L - tab.V
    off = np.concatenate([[0], np.cumsum(tab.frame_counts)])
    n_first = len(tab.seg_len) - len(tab.frame_counts)
    # processing order: L-frame segments that are not their recording's last (recording, then segment order), then the last ones
    m = np.bincount(tab.seg_utt, minlength=len(tab.frame_counts))
    assert np.all(tab.seg_index[:n_first] < m[tab.seg_utt[:n_first]] - 1) and np.all(tab.seg_len[:n_first] == L)
    key = tab.seg_utt[:n_first].astype(np.int64) * (1 << 32) + tab.seg_index[:n_first]
    assert np.all(np.diff(key) > 0)
    assert np.array_equal(tab.seg_utt[n_first:], np.arange(len(tab.frame_counts))) and np.array_equal(tab.seg_index[n_first:], m - 1)
    assert np.array_equal(tab.seg_first, tab.seg_index * stride)
    # a segment's rows copy its frames in order
    seg_of = np.searchsorted(tab.seg_row, np.arange(len(tab.src_row)), side="right") - 1
    assert np.array_equal(tab.src_row, off[tab.seg_utt[seg_of]] + tab.seg_first[seg_of] + np.arange(len(tab.src_row)) - tab.seg_row[seg_of])
    assert np.all(tab.seg_first + tab.seg_len <= np.asarray(tab.frame_counts)[tab.seg_utt])
    cover_all = np.bincount(tab.src_row, minlength=int(off[-1]))
    assert cover_all.min() >= 1 and cover_all.max() <= 2
    for u, n in enumerate(tab.frame_counts):
        last = tab.seg_len[n_first + u]
        assert last == n if m[u] == 1 else L <= last < L + stride
        assert m[u] == 1 or n >= L + stride
        two = np.flatnonzero(cover_all[off[u]:off[u + 1]] == 2)
        assert len(two) == (m[u] - 1) * V
        if len(two):                                                     # runs of exactly V frames, at the start of segments 1 .. m-1
            assert np.array_equal(two, (np.arange(1, m[u])[:, None] * stride + np.arange(V)[None, :]).reshape(-1))
    # row_a / row_b / src_row are mutually consistent: both rows copy the frame they stand for
    t = np.arange(int(off[-1]))
    assert np.array_equal(tab.src_row[tab.row_a], t)
    ov = tab.row_b >= 0
    assert np.array_equal(tab.src_row[tab.row_b[ov]], t[ov]) and np.all(tab.w_b[~ov] == 0)
    assert np.all(tab.seg_index[seg_of[tab.row_b[ov]]] == tab.seg_index[seg_of[tab.row_a[ov]]] + 1)
    assert np.all(tab.seg_utt[seg_of[tab.row_b[ov]]] == tab.seg_utt[seg_of[tab.row_a[ov]]])
    i = tab.row_b[ov] - tab.seg_row[seg_of[tab.row_b[ov]]]              # index inside the overlap
    assert np.array_equal(tab.w_b[ov].view(np.int32), ((i + 1) / (V + 1)).astype(np.float32).view(np.int32))


@pytest.mark.parametrize("L", range(2, 41))
def test_exhaustive(L):
    """n in 1..400, V in 0..L//2: the count entry per n alone, and the table of the 400 recordings as one ragged batch
    against rule() (segments, order) and the rule's promises (check_properties pins every other array to those)."""
    lib = _lib.lib()
    ns, nr = C.c_int64(), C.c_int64()
    counts = list(range(1, 401))
    for V in range(L // 2 + 1):
        segs = [rule(n, L, V) for n in counts]
        for n, s in zip(counts, segs):
            fc = np.array([n], np.int32)
            assert lib.vaenmf_segment_count(1, fc.ctypes.data, L, V, C.byref(ns), C.byref(nr)) == 0
            assert ns.value == len(s) and nr.value == sum(ln for _, ln in s)
        tab = lf.segment_table(counts, L, V, BIG)
        order = [(u, j) for u, s in enumerate(segs) for j in range(len(s) - 1)] + [(u, len(s) - 1) for u, s in enumerate(segs)]
        assert list(zip(tab.seg_utt, tab.seg_index)) == order
        assert list(zip(tab.seg_first, tab.seg_len)) == [segs[u][j] for u, j in order]
        assert lib.vaenmf_segment_count(400, np.asarray(counts, np.int32).ctypes.data, L, V, C.byref(ns), C.byref(nr)) == 0
        assert (ns.value, nr.value) == (len(order), len(tab.src_row))
        check_properties(tab)


def test_single_recordings_every_array():
    """Every array of the table against the restated rule, one recording at a time, on a grid that holds every case of the
    exhaustive sweep's lengths (1, 2 and many segments; V = 0, 1, L//2)."""
    for L in (2, 3, 7, 24, 40):
        for V in sorted({0, 1 if L >= 2 else 0, L // 2}):
            for n in list(range(1, 3 * L + 2)) + [399, 400]:
                check_properties(check_table([n], L, V))


def test_ragged_batches():
    g = np.random.default_rng(7)
    for _ in range(300):
        L = int(g.integers(2, 41))
        V = int(g.integers(0, L // 2 + 1))
        counts = [int(v) for v in g.integers(1, 401, size=int(g.integers(1, 6)))]
        check_properties(check_table(counts, L, V))
    tab = check_table([23, 24, 43, 44, 97], 24, 4)                       # the GPU tests' batch: 1, 1, 1, 2 and 4 segments
    assert list(tab.seg_len) == [24, 24, 24, 24, 23, 24, 43, 24, 37]
    assert list(tab.seg_utt) == [3, 4, 4, 4, 0, 1, 2, 3, 4] and list(tab.seg_index) == [0, 0, 1, 2, 0, 0, 0, 1, 3]


def test_threshold_sizes():
    for L in range(2, 41):
        for V in range(L // 2 + 1):
            stride = L - V
            got = [len(lf.segment_table([n], L, V, BIG).seg_len) for n in (L - 1, L, L + stride - 1, L + stride)]
            assert got == [1, 1, 1, 2], (L, V, got)


def test_refusals():
    lib = _lib.lib()
    ns, nr = C.c_int64(), C.c_int64()
    fc = np.array([100], np.int32)
    cnt = lambda L, V: lib.vaenmf_segment_count(1, fc.ctypes.data, L, V, C.byref(ns), C.byref(nr))
    assert cnt(10, 6) != 0 and b"V=6" in lib.vaenmf_last_error() and b"L=10" in lib.vaenmf_last_error()
    assert cnt(11, 6) != 0 and cnt(12, 6) == 0 and cnt(10, -1) != 0
    assert cnt(1, 0) != 0 and b"L=1" in lib.vaenmf_last_error()
    zero = np.array([5, 0], np.int32)
    assert lib.vaenmf_segment_count(2, zero.ctypes.data, 4, 1, C.byref(ns), C.byref(nr)) != 0
    for bad in ((10, 6), (1, 0)):
        with pytest.raises(ValueError):
            lf.segment_table([100], bad[0], bad[1], BIG)
    # the longest possible segment, L + stride - 1 = 43 frames, against the engine's capacity
    with pytest.raises(ValueError, match="43.*max_frames=42"):
        lf.segment_table([30], 24, 4, 42)
    assert len(lf.segment_table([30], 24, 4, 43).seg_len) == 1
    assert lib.vaenmf_segment_count(0, None, 4, 1, C.byref(ns), C.byref(nr)) == 0 and (ns.value, nr.value) == (0, 0)


def test_splitmix_and_default_seeds():
    assert lf.splitmix64(0) == 0xE220A8397B1DCDAF                        # the published first output of splitmix64 from state 0
    assert lf.default_seeds(3) == [lf.splitmix64(0x5EED + u) for u in range(3)]


def test_segment_seeds():
    L, V = 10, 2
    tab = lf.segment_table([L + 49 * (L - V) + 3] * 64, L, V, BIG)       # 64 recordings of 50 segments
    assert len(tab.seg_len) == 64 * 50
    seeds = list(range(64))
    ss = lf.segment_seeds(seeds, tab)
    assert all(0 <= s < 2 ** 64 for s in ss)
    for s, u, j in zip(ss, tab.seg_utt, tab.seg_index):
        if j == 0:
            assert s == seeds[u]                                         # segment 0: the recording's own seed
        else:
            assert s == lf.splitmix64(seeds[u] ^ lf.splitmix64(int(j)))
    assert len(set(ss)) == len(ss)
    # distinct under XOR with any 24-bit number: the top 40 bits differ.  That can hold for the derived seeds only: segment 0
    # runs with the caller's seed itself (so that a single-segment recording keeps the bits of enhance()), and the callers'
    # seeds 0..63 share their top 40 bits among themselves.  So: the 64 x 49 derived seeds differ from one another and from
    # every caller's seed in their top 40 bits.
    derived = [s for s, j in zip(ss, tab.seg_index) if j > 0]
    tops = {s >> 24 for s in derived}
    assert len(derived) == 64 * 49 and len(tops) == len(derived)
    assert not tops & {s >> 24 for s in seeds}
    big = lf.segment_seeds([2 ** 64 - 1, 2 ** 64 + 5], lf.segment_table([40, 40], L, V, BIG))
    assert all(0 <= s < 2 ** 64 for s in big)


def test_pack_rounds_and_owner_rows():
    tab = lf.segment_table([23, 24, 43, 44, 97], 24, 4, BIG)
    assert lf.pack_rounds(tab, 8, 4096) == [(0, 4), (4, 9)]
    assert lf.pack_rounds(tab, 2, 4096) == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 9)]
    assert lf.pack_rounds(tab, 8, 44) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8), (8, 9)]
    assert lf.pack_rounds(tab, 8, 50) == [(0, 2), (2, 4), (4, 6), (6, 7), (7, 8), (8, 9)]
    for mu, mf in ((8, 4096), (2, 4096), (8, 44), (3, 70)):
        r = lf.pack_rounds(tab, mu, mf)
        assert r[0][0] == 0 and r[-1][1] == 9 and all(a[1] == b[0] for a, b in zip(r, r[1:]))
        assert all(q - p <= mu and tab.seg_row[q] - tab.seg_row[p] <= mf for p, q in r)
    own = lf.owner_rows(tab)
    ov = tab.row_b >= 0
    assert np.array_equal(own[~ov], tab.row_a[~ov])
    # V = 4: weights 0.2, 0.4 (earlier segment), 0.6, 0.8 (later segment)
    later = tab.w_b[ov] > 0.5
    assert np.array_equal(own[ov], np.where(later, tab.row_b[ov], tab.row_a[ov])) and later.sum() == ov.sum() // 2
    tie = lf.segment_table([40], 10, 1, BIG)                             # V = 1: w_b = 0.5, a tie: the earlier segment
    assert np.array_equal(lf.owner_rows(tie), tie.row_a)
