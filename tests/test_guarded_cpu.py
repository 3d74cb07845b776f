"""tests/guarded.py and tests/contract_cases.py without a GPU: the arena carves what it says and reports damage where it
is, bitwise; the cases of tests/test_gpu_buffer_contract.py reach every kernel form the dispatch has."""
import numpy as np
import pytest
import torch

from contract_cases import CASES, COUNTS, DECODE_CASES, DECODE_SAMPLES, LARGE_COUNTS, NS, RCAP, BY_NAME, case_class, is_wide, n_wave_tiles
from guarded import ALIGN, GUARD_ROWS, MIN_GUARD, POISON, RESIDUE, Arena, GuardError, bits

SHAPES = [("X", (53, 272, 2), torch.float32), ("g", (53,), torch.float32), ("Vs", (53, 12, 656), torch.float32),
          ("cost", (53,), torch.float64), ("Zs", (53, 12, 32), torch.float32)]


def _arena(poison):
    a = Arena(24 << 20, poison)
    for name, shape, dtype in SHAPES:
        a.carve(name, shape, dtype)
    return a


@pytest.mark.parametrize("poison", sorted(POISON))
def test_carved_buffers_are_exact_misaligned_and_guarded(poison):
    a = _arena(poison)
    word = np.array([POISON[poison]], np.uint32).view(np.int32)[0]
    assert a.mem.data_ptr() % ALIGN == 0
    end_prev = prev_need = 0
    for name, shape, dtype in SHAPES:
        b, v = a.bufs[name], a.view(name)
        item = torch.empty(0, dtype=dtype).element_size()
        assert v.shape == shape and v.dtype == dtype and v.is_contiguous()
        assert b["nbytes"] == int(np.prod(shape)) * item == v.numel() * v.element_size()      # exact: not one byte more
        assert v.data_ptr() % ALIGN == RESIDUE == 16 and v.data_ptr() == a.mem.data_ptr() + b["off"]
        row = b["nbytes"] // shape[0]
        need = max(MIN_GUARD, GUARD_ROWS * row)
        assert MIN_GUARD == 64 * 1024 and GUARD_ROWS == 32
        assert b["off"] - end_prev >= need + prev_need                      # its guard, and the previous buffer's own
        assert bool(a.is_guard[end_prev // 4:b["off"] // 4].all()) and not bool(a.is_guard[b["off"] // 4:(b["off"] + b["nbytes"]) // 4].any())
        assert bool((bits(v) == (word if item == 4 else (int(word) << 32 | int(word) & 0xFFFFFFFF))).all())    # outputs start as poison
        end_prev, prev_need = b["off"] + b["nbytes"], need
    assert a.size - end_prev >= need and a.cursor <= a.size and bool(a.is_guard[end_prev // 4:].all())   # the arena ends with a guard
    assert bool((a.words[a.is_guard] == word).all())
    a.check()
    # a float comparison could not see the poison in a guard; the bits can
    nan = a.words[:1].view(torch.float32)
    assert (poison == "nan") == bool(nan != nan)
    with pytest.raises(MemoryError):
        Arena(1 << 20, poison).carve("Vs", (53, 12, 656), torch.float32)


def _raw(a, name):
    b = a.bufs[name]
    return a.mem, b["off"], b["off"] + b["nbytes"]


def test_damage_is_found_and_named():
    a = _arena("nan")
    mem, lo, hi = _raw(a, "Vs")
    row = 12 * 656 * 4
    # one element two rows past the end: the guard after Vs, row 53 + 2
    mem[hi + 2 * row + 8:hi + 2 * row + 12].view(torch.float32).fill_(1.0)
    with pytest.raises(GuardError, match=r"guard after buffer 'Vs' damaged: first at byte \+%d past its end \(row 55 of its 53 rows" % (2 * row + 8)):
        a.check("call")
    a.poison(mem[hi + 2 * row + 8:hi + 2 * row + 12].view(torch.float32))
    a.check()
    # one element before the start of g: four bytes before, row -1
    mem, lo, hi = _raw(a, "g")
    mem[lo - 4:lo].view(torch.float32).fill_(0.0)
    with pytest.raises(GuardError, match=r"guard before buffer 'g' damaged: first at byte -4 from its start \(row -1 of its 53 rows of 4 bytes\); 1 words"):
        a.check()
    a.poison(mem[lo - 4:lo].view(torch.float32))
    # the row after the last of X (an idle lane storing to frame NT): row 53
    mem, lo, hi = _raw(a, "X")
    mem[hi:hi + 16].view(torch.float32).fill_(0.0)
    with pytest.raises(GuardError, match=r"after buffer 'X' damaged: first at byte \+0 past its end \(row 53 "):
        a.check()
    a.poison(mem[hi:hi + 16].view(torch.float32))
    a.check()
    # a buffer the call may only read
    a.view("Zs").zero_()
    a.view("cost").zero_()
    a.snapshot(["Zs", "cost", "g"])
    a.unchanged()
    a.view("Zs")[7, 3, 5] = 1.0
    with pytest.raises(GuardError, match=r"read-only buffer 'Zs' changed: first at byte %d \(row 7 of its 53 rows of 1536 bytes\); 1 words" % ((7 * 12 * 32 + 3 * 32 + 5) * 4)):
        a.unchanged(what="call")
    a.unchanged(["cost", "g"])
    a.view("Zs")[7, 3, 5] = 0.0
    a.unchanged()
    a.view("cost")[52] = -0.0                  # equal as a number, not as bits
    with pytest.raises(GuardError, match=r"'cost' changed: first at byte %d \(row 52 " % (52 * 8 + 4)):
        a.unchanged()


def test_the_comparison_is_bitwise():
    """A NaN guard overwritten with another NaN, and a NaN input replaced by another NaN: no float comparison tells them apart."""
    a = _arena("nan")
    mem, lo, hi = _raw(a, "g")
    other = np.array([0x7FC00000], np.uint32).view(np.int32)[0]
    mem[hi + 64:hi + 68].view(torch.int32).fill_(int(other))
    with pytest.raises(GuardError, match=r"guard after buffer 'g' damaged: first at byte \+64 "):
        a.check()
    a.poison(mem[hi + 64:hi + 68].view(torch.float32))
    a.check()
    a.snapshot(["g"])                          # g is all poison (NaN) here
    bits(a.view("g"))[9] = int(other)
    with pytest.raises(GuardError, match=r"'g' changed: first at byte 36 \(row 9 "):
        a.unchanged()
    b = _arena("1e30")
    assert float(b.view("g")[0]) == np.float32(1e30) and b.is_poison(b.view("g")) and not a.is_poison(a.view("g"))


def test_cases_reach_every_kernel_form():
    """The case table of tests/test_gpu_buffer_contract.py, restated, and what shape_class() says it runs."""
    table = {   # name: (F, K, precision, z_dim, h_dim, counts, chain kernel, w_fused, nch, tail, Kp, W fits LDS)
        "f9": (9, 3, "bf16x3", 32, [128, 128], COUNTS, 1, 0, 1, True, 8, True),
        "f9_one_tile": (9, 3, "bf16x3", 32, [128, 128], [3], 1, 0, 1, True, 8, True),
        "f65_z16": (65, 10, "bf16x3", 16, [128, 128], COUNTS, 1, 0, 1, False, 16, True),
        "f250_m2": (250, 17, "bf16x3", 32, [128, 128], COUNTS, 1, 0, 1, True, 32, True),
        "f257_x3_noise_psd": (257, 8, "bf16x3", 32, [128, 128], COUNTS, 1, 0, 1, False, 8, True),
        "f257": (257, 8, "bf16", 32, [128, 128], COUNTS, 2, 2, 1, False, 8, True),
        "f257_one_tile": (257, 8, "bf16", 32, [128, 128], [3], 2, 2, 1, False, 8, True),
        "f273": (273, 10, "bf16x3", 32, [128, 128], COUNTS, 0, 0, 2, False, 16, True),
        "f273_z16": (273, 10, "bf16x3", 16, [128, 128], COUNTS, 0, 0, 2, False, 16, True),
        "f514_m2": (514, 8, "bf16", 32, [128, 128], COUNTS, 2, 0, 3, True, 8, True),
        "f640": (640, 32, "bf16x3", 32, [128, 128], COUNTS, 0, 0, 3, False, 32, False),
        "wide_z128_h256_x3": (65, 10, "bf16x3", 128, [256, 128], COUNTS, 3, 0, 1, False, 16, True),
        "wide_z128_h256": (65, 10, "bf16", 128, [256, 128], COUNTS, 3, 0, 1, False, 16, True),
        "wide_z64_x3": (65, 10, "bf16x3", 64, [128, 128], COUNTS, 3, 0, 1, False, 16, True),
        "wide_z64": (65, 10, "bf16", 64, [128, 128], COUNTS, 3, 0, 1, False, 16, True),
        "f257_large": (257, 8, "bf16", 32, [128, 128], [16] * 256 + [17, 1], 1, 1, 1, False, 8, True),
    }
    assert COUNTS == [17, 1, 30, 5] and sum(COUNTS) == 53 and n_wave_tiles(COUNTS) == 6
    assert [n % 16 for n in COUNTS].count(0) == 0 and sum(1 for n in COUNTS for t in range((n + 15) // 16) if min(16, n - 16 * t) < 16) == 4
    assert list(np.cumsum(COUNTS)[:-1]) == [17, 18, 48] and 16 * ((COUNTS[-1] + 15) // 16) - COUNTS[-1] == 11      # rows 53..63
    assert n_wave_tiles(LARGE_COUNTS) == 259 > 256
    assert (NS, RCAP) == (10, 12) and DECODE_SAMPLES == [(1, 4), (10, 12), (33, 40)]
    assert [c.name for c in CASES] == list(table)
    for c in CASES:
        F, K, prec, z, hd, counts, ck, wf, nch, tail, Kp, wlds = table[c.name]
        assert (c.F, c.K, c.precision, c.z_dim, list(c.h_dim), list(c.counts)) == (F, K, prec, z, hd, counts), c.name
        sc = case_class(c)
        assert (sc["chain_kernel"], sc["w_fused"], sc["nch"], sc["tail"], sc["Kp"], sc["w_in_lds"]) == (ck, wf, nch, tail, Kp, wlds), (c.name, sc)
        assert is_wide(c) == (ck == 3)
    cls = [case_class(c) for c in CASES]
    assert {s["chain_kernel"] for s in cls} == {0, 1, 2, 3}
    assert {s["w_fused"] for s in cls} == {0, 1, 2}
    assert {s["nch"] for s in cls} == {1, 2, 3}
    assert any(s["tail"] for s in cls) and {s["nch"] for s in cls if s["tail"]} >= {1, 3}
    assert {s["Kp"] for s in cls} == {8, 16, 32}
    assert any(not s["w_in_lds"] for s in cls)
    # the one-wavefront bf16 chain at 17 tiles and the 64-frame-tile W statistics need the large batch
    big = case_class(BY_NAME["f257_large"])
    assert big["chain_form"] == "wchain<17,exact>" and big["chain_kernel"] == 1 and big["w_fused"] == 1
    assert case_class(BY_NAME["f257_large"], n_cus=304)["chain_kernel"] == 2       # (on a device with more compute units it would not)
    # variants: z_dim 16 on a narrow case, M2 labels on two, a fixed noise PSD on one, one-tile batches on two
    assert [c.name for c in CASES if c.z_dim == 16] == ["f65_z16", "f273_z16"] and sum(1 for c in CASES if c.Dy) == 2
    assert sum(1 for c in CASES if c.noise_psd) == 1 and sum(1 for c in CASES if list(c.counts) == [3]) == 2
    assert all(not is_wide(BY_NAME[n]) for n in DECODE_CASES) and any(BY_NAME[n].z_dim == 16 for n in DECODE_CASES)
    dc = [case_class(BY_NAME[n]) for n in DECODE_CASES]      # decoding entries: wave and team shapes, TAIL, W outside LDS, labels
    assert any(s["tail"] for s in dc) and any(not s["w_in_lds"] for s in dc) and {s["chain_kernel"] for s in dc} >= {0, 1, 2} and any(BY_NAME[n].Dy for n in DECODE_CASES)
    assert {(c.z_dim, tuple(c.h_dim), c.precision) for c in CASES if is_wide(c)} == {(z, h, p) for z, h in ((128, (256, 128)), (64, (128, 128))) for p in ("bf16", "bf16x3")}
