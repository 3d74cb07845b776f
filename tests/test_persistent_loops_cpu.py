"""No GPU: the cases of tests/test_gpu_persistent_loops.py reach what they are for.

wave_frames / chain_rounds / decode_trips (tests/dispatch_model.py, next to shape_class) restate which frames, wave
tiles and tiles a wavefront or workgroup of the persistent kernels walks, trip by trip, for a grid capped by
VAENMF_GRID_CAP.  The assertions below are about the capped cases of the GPU module: if a batch, a cap or the dispatch
changes so that a case stops reaching a second trip, an utterance boundary inside a block, a clipped block, an empty
wavefront, ..., this test fails instead of the GPU module silently testing less.
"""
import numpy as np

from dispatch_model import (COUNTS, N_WAVE_TILES, chain_form, chain_grid, chain_rounds, chain_waves, decode_class, decode_grid, decode_tiles,
                            decode_trips, default_chain_counts, default_stream_counts, shape_class, stream_class, stream_grid, wave_frames,
                            wave_tiles)
from persistent_cases import (CHAIN_CASES, CHAIN_COUNTS, CHAIN_FORMS, CHAIN_K, CHAIN_R, MAX_LEFT_OUT, STREAM_CAPS, STREAM_CASES, TILE_CAPS,
                              TILE_CASES, chain_reference)

N_CUS = 256


def test_restated_assignments_at_known_launches():
    """The restatements at launches whose shape the code's comments give."""
    # the sweeps: 70 frames, one frame per wavefront, 18 workgroups of 4 wavefronts
    assert stream_grid(70, N_CUS) == 18 and wave_frames(70, 18)[0] == 1
    assert stream_grid(70, N_CUS, cap=2) == 2 and stream_grid(70, N_CUS, cap=50) == 18 and stream_grid(70, N_CUS, cap=0) == 18
    # the bench batch: per > 1 needs NT > 16 n_sms (4 n_sms workgroups), 8 n_sms for wstats_stream2
    assert wave_frames(16 * N_CUS, stream_grid(16 * N_CUS, N_CUS))[0] == 1 and wave_frames(16 * N_CUS + 1, stream_grid(16 * N_CUS + 1, N_CUS))[0] == 2
    assert wave_frames(8 * N_CUS + 1, stream_grid(8 * N_CUS + 1, N_CUS, pipelined=True))[0] == 2
    per, blocks = wave_frames(70, 1)
    assert per == 18 and blocks == [(0, 18), (18, 36), (36, 54), (54, 70)]
    # the chain: tile (i NWAVES + w) gridDim + b; a second round needs more than NWAVES n_sms wave tiles
    assert chain_rounds(8 * N_CUS, chain_grid(8 * N_CUS, N_CUS), 8)[1] == 1 and chain_rounds(8 * N_CUS + 1, N_CUS, 8)[1] == 2
    assert chain_rounds(4 * N_CUS + 1, N_CUS, chain_waves("bf16x3", 17))[1] == 2 and chain_waves("bf16", 33) == 4 and chain_waves("bf16", 17) == 8
    where, rounds = chain_rounds(18, 1, 8)
    assert rounds == 3 and where[(0, 1)] == [1, 9, 17] and where[(0, 7)] == [7, 15]
    assert sorted(wt for v in chain_rounds(1000, 7, 4)[0].values() for wt in v) == list(range(1000))      # every tile once
    # the tile loop: grid min(n_tiles, 2 n_sms)
    assert decode_grid(4, N_CUS) == 4 and decode_grid(513, N_CUS) == 512 and decode_trips(513, 512)[0] == [0, 512]
    assert decode_tiles(COUNTS, 0) == [(0, 0, 21), (1, 21, 40), (2, 61, 9)]
    assert decode_tiles(COUNTS, 4) == [(0, 0, 21), (1, 21, 32), (1, 53, 8), (2, 61, 9)]
    assert len(wave_tiles(COUNTS)) == N_WAVE_TILES


def _stream_reach(NT, off, grid, rank_above_8):
    """What a streaming launch of `grid` workgroups reaches on a batch with the frame offsets `off`."""
    utt_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
    per, blocks = wave_frames(NT, grid)
    t = set()
    if per >= 3:
        t.add("per>=3")
    for b, e in blocks:
        if b >= e:
            t.add("empty wavefront")
            continue
        if len(set(utt_of[b:e])) > 1:
            t.add("straddles an utterance boundary")
        if b not in off:
            t.add("begins mid-utterance")
        if e - b < per:
            t.add("clipped last block")
    if rank_above_8:        # FrameCtx::stage_block_w: W of the utterance of the workgroup's first frame
        for wg in range(grid):
            frames = [n for b, e in blocks[4 * wg:4 * wg + 4] for n in range(b, e)]
            if not frames:
                continue
            blk_utt = utt_of[blocks[4 * wg][0]]
            inside = [utt_of[n] == blk_utt for n in frames]
            t.add("workgroup inside blk_utt" if all(inside) else "workgroup with frames outside blk_utt")
            for b, e in blocks[4 * wg:4 * wg + 4]:
                if b < e and not any(utt_of[n] == blk_utt for n in range(b, e)):
                    t.add("wavefront outside blk_utt")
    return t


def test_streaming_cases_reach_the_frame_loop():
    NT, off = sum(COUNTS), list(np.concatenate([[0], np.cumsum(COUNTS)]))
    want = {"per>=3", "straddles an utterance boundary", "begins mid-utterance", "clipped last block", "empty wavefront"}
    want16 = want | {"workgroup inside blk_utt", "workgroup with frames outside blk_utt", "wavefront outside blk_utt"}
    seen = set()
    for F, K, R, variant, precision, switches in STREAM_CASES:
        sc = stream_class(F, K, R, precision, variant, N_WAVE_TILES, N_CUS, wfused=switches.get("VAENMF_WFUSED") != "0")
        ws = sc["wstats"]
        # the capped grids are those of launch_stream: no fused / group kernel (VAENMF_WFUSED_GRID is theirs)
        assert ws is None or ws["kernel"] in ("wstats_stream", "wstats_stream2"), (F, K, R, precision)
        reach = set()
        for cap in STREAM_CAPS:
            for pipelined in ((False, True) if ws and ws["kernel"] == "wstats_stream2" else (False,)):
                grid = stream_grid(NT, N_CUS, cap, pipelined)
                assert grid == cap
                r = _stream_reach(NT, off, grid, sc["hg"]["KP"] > 8)
                assert "per>=3" in r, (cap, r)
                reach |= r
        assert reach >= (want16 if sc["hg"]["KP"] > 8 else want), (F, K, R, precision, sorted(reach))
        for kd in ("wstats", "hg", "wf"):
            if sc[kd]:
                s = sc[kd]
                seen.add((s["kernel"], s["NCH"], s["KP"], s["store"]))
                seen.add((s["kernel"], "rows", s["rows"]))
                seen.add((s["kernel"], "TAIL" if s["TAIL"] else "no tail"))
        seen.add(("w_in_lds", sc["hg"]["w_in_lds"], sc["hg"]["KP"] > 8))
        seen.add(("variant", variant))
        if sc["hg"]["RT"]:
            seen.add(("hg exact count", sc["hg"]["RT"]))
        seen.add(("extra bin", sc["hg"]["extra_bin"]))
        if ws and ws["kernel"] == "wstats_stream" and ws["KP"] == 8:
            seen.add("wstats_stream at rank 8")
    # the forms of the issue: one, two, three chunks with and without a tail; the ranks; both row types; both W-statistics kernels
    for kernel in ("wstats_stream", "hg_stream", "wf_stream"):
        assert {(n, st) for k, n, _, st in (s for s in seen if len(s) == 4) if k == kernel} == {(n, st) for n in (1, 2, 3) for st in ("bf16", "float")}, kernel
    assert {s[2] for s in seen if len(s) == 4} == {8, 16, 32}
    assert {s[3] for s in seen if len(s) == 4 and s[0] == "wstats_stream2"} == {"bf16", "float"}
    for kernel in ("hg_stream", "wf_stream"):
        assert (kernel, "TAIL") in seen and (kernel, "no tail") in seen
    assert {("wstats_stream", "rows", r) for r in ("one", "exact", "partial")} <= seen         # "one": two half batches, refilled a frame ahead
    assert {("hg exact count", 10), ("hg exact count", 30), ("variant", "M2"), ("variant", "noNMF"), "wstats_stream at rank 8"} <= seen
    assert {("w_in_lds", True, False), ("w_in_lds", True, True), ("w_in_lds", False, True)} <= seen
    assert ("extra bin", True) in seen and ("extra bin", False) in seen
    assert {c[0] for c in STREAM_CASES} == {64, 201, 251, 257, 442, 514, 640} and {c[1] for c in STREAM_CASES} == {4, 8, 10, 32}
    assert {c[2] for c in STREAM_CASES} == {10, 30, 7}


def test_chain_cases_reach_later_rounds():
    tiles = wave_tiles(CHAIN_COUNTS)
    assert len(tiles) >= 18 and 190 <= sum(CHAIN_COUNTS) <= 210
    forms = {"bf16x3": set(), "bf16": set()}
    for F, precision, labels in CHAIN_CASES:
        form, need_switch = chain_form(F, precision, len(tiles))
        sc = shape_class(F, CHAIN_K, precision, len(tiles), CHAIN_R, N_CUS)
        assert sc["chain_kernel"] in (1, 2) and need_switch == (sc["chain_kernel"] == 2), (F, precision)    # never the team kernel
        forms[precision].add(form)
        nwaves = chain_waves(precision, sc["chain_tiles"])
        grid = chain_grid(len(tiles), N_CUS, cap=1)
        assert grid == 1
        where, rounds = chain_rounds(len(tiles), grid, nwaves)
        assert rounds >= 3
        cnt = lambda wt: tiles[wt][2]
        seqs = [[cnt(wt) for wt in v] for v in where.values()]
        assert any(a < 16 and b == 16 for s in seqs for a, b in zip(s, s[1:])), "a partly filled wave tile, then a full one"
        assert any(a == 16 and b < 16 for s in seqs for a, b in zip(s, s[1:])), "a full wave tile, then a partly filled one"
        assert any(n == 1 for s in seqs for n in s[1:]), "a one-frame tile in a later round"
        assert any(len(s) < rounds for s in seqs) and all(len(s) >= rounds - 1 for s in seqs), "a wavefront without a tile in the last round"
        assert any(tiles[a][0] != tiles[b][0] for v in where.values() for a, b in zip(v, v[1:]))          # another utterance's W, seeds
    assert forms == CHAIN_FORMS
    assert {(F, p) for F, p, lab in CHAIN_CASES if lab} == {(201, "bf16x3"), (257, "bf16")}       # registers / the b1stash of 8 wavefronts
    # the default dispatch of the 17- and 33-tile bf16 shapes at this batch is wchain4_kernel: the cases switch it off
    assert {F for F, p, _ in CHAIN_CASES if chain_form(F, p, len(tiles))[1]} == {257, 514}


def test_chain_oracle_leaves_out_at_most_15_percent():
    """The decision-margin rule of the chain sweeps (a frame counts when each of its decisions is 1e-2 from the threshold)
    on the oracle's own trace: the inputs' seeds (CHAIN_SEEDS) keep the share of frames it leaves out within 15 %."""
    for F, labels in sorted({(F, labels) for F, p, labels in CHAIN_CASES if p == "bf16x3"}):
        refs, left_out = chain_reference(F, labels)
        print("chain F=%d labels=%d: %.1f %% of %d frames left out" % (F, labels, 100 * left_out, sum(CHAIN_COUNTS)))
        assert left_out <= MAX_LEFT_OUT, (F, labels, left_out)
        assert all(r.keep.any() for r in refs if len(r.keep) > 4)


def test_tile_loop_cases_reach_later_trips():
    seen, geoms = set(), set()
    for F, K, R, precision in TILE_CASES:
        dc = decode_class(F, K, R, precision)
        geoms.add((dc["geom"], dc["split"]))
        tiles = decode_tiles(COUNTS, dc["geom"])
        for cap in TILE_CAPS:
            grid = decode_grid(len(tiles), N_CUS, cap)
            assert grid == cap
            trips = decode_trips(len(tiles), grid)
            assert max(len(t) for t in trips) >= (3 if cap == 1 else 2)
            for t in trips:
                for a, b in zip(t, t[1:]):
                    seen.add(("same utterance" if tiles[a][0] == tiles[b][0] else "another utterance", dc["KP"] == 8))
        seen.add(("chunks", dc["chunks"]))
        seen.add(("K", K))
    assert geoms == {(g, split) for g in (0, 2, 3, 4) for split in (True, False)}          # every geometry in both precisions
    # W of rank <= 8 restaged in LDS behind the barrier: for the same and for another utterance
    assert {("same utterance", True), ("another utterance", True), ("same utterance", False), ("another utterance", False)} <= seen
    assert {("chunks", 1), ("chunks", 2), ("K", 8), ("K", 10), ("K", 32)} <= seen
    assert {c[0] for c in TILE_CASES} == {250, 321, 512, 640}


def test_default_launch_batches_reach_a_second_trip():
    """The batches of the two tests without a switch, for a range of CU counts."""
    for n in (64, 104, 228, 256, 304):
        counts = default_stream_counts(n)
        NT = sum(counts)
        assert NT == 16 * n + 41 and min(counts) >= 1 and 30 <= len(counts) <= 50
        per, blocks = wave_frames(NT, stream_grid(NT, n))
        assert per == 2 and any(e - b == 1 for b, e in blocks) and any(b >= e for b, e in blocks)
        assert wave_frames(NT, stream_grid(NT, n, pipelined=True))[0] == 3
        counts = default_chain_counts(n)
        assert len(wave_tiles(counts)) == len(counts) > 8 * n and set(counts) == set(range(1, 17))
        assert chain_rounds(len(counts), chain_grid(len(counts), n), 8)[1] == 2
