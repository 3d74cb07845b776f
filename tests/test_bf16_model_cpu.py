"""tests/bf16_model.py checked without a GPU: its bf16 rounding against torch.bfloat16, its model against the plain oracle
(the same function on rounded operands), and the floor / ceiling table every bound of tests/test_gpu_bf16_model.py comes
from -- computed here from seeded inputs, printed, and required to separate a correct kernel's arithmetic from each
planted defect by a factor of 100 for every statistic that is used (bf16_model.sandwich).  The defects live in the numpy
emulation only."""
import functools

import numpy as np
import pytest
import torch

import bf16_model as bm
import vaenmf_oracle as orc

f32 = np.float32


def _torch_bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=f32)).to(torch.bfloat16).to(torch.float32).numpy()


def test_bf16_rne_keeps_every_bf16_value():
    bits = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    vals = (bits.astype(np.uint32) << np.uint32(16)).view(f32)
    back = bm.bf16_bits(vals)
    nan = np.isnan(vals)
    assert np.array_equal(back[~nan], bits[~nan])
    assert np.all(np.isnan(bm.bf16_rne(vals[nan]))) and np.all((back[nan] & 0x7FC0) == 0x7FC0)      # NaN stays a quiet NaN
    assert np.array_equal(bm.bf16_rne(vals[~nan]).astype(f32).view(np.uint32), _torch_bf16(vals[~nan]).view(np.uint32))


@pytest.mark.parametrize("exponent", [1, 64, 126, 127, 128, 200, 254])
def test_bf16_rne_at_every_tie_and_its_neighbours(exponent):
    """All 128 mantissas of the exponent, both signs: the exact tie (low half 0x8000) goes to the even neighbour, one
    float32 step below it rounds down and one above rounds up; torch.bfloat16 agrees bit for bit."""
    hi = (np.arange(128, dtype=np.uint32) << np.uint32(16)) | np.uint32(exponent << 23)
    for sign in (np.uint32(0), np.uint32(0x80000000)):
        for low, expect_up in ((0x7FFF, False), (0x8000, None), (0x8001, True), (0x0000, False), (0xFFFF, True), (0x0001, False)):
            x = (hi | np.uint32(low) | sign).view(f32)
            got = bm.bf16_bits(x).astype(np.uint32)
            up = ((hi >> np.uint32(16)) & np.uint32(1)).astype(bool) if expect_up is None else np.full(128, expect_up)
            want = ((hi | sign) >> np.uint32(16)) + up.astype(np.uint32)
            assert np.array_equal(got, want), (exponent, hex(low))
            assert np.array_equal(bm.bf16_rne(x).astype(f32).view(np.uint32), _torch_bf16(x).view(np.uint32))


def test_bf16_rne_denormals_zeros_and_the_largest_value():
    u = np.array([0x00000000, 0x80000000, 0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x0001FFFF, 0x007FFFFF,
                  0x807F8000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F800000, 0xFF800000], dtype=np.uint32)
    x = u.view(f32)
    with np.errstate(over="ignore"):
        got = bm.bf16_rne(x).astype(f32)
    assert np.array_equal(got.view(np.uint32), _torch_bf16(x).view(np.uint32))
    assert np.signbit(got[1]) and got[1] == 0 and not np.signbit(got[0])
    assert got[4] == 0 and got[5] > 0                       # the smallest tie goes to the even side, zero
    assert np.isposinf(got[10]) and np.isneginf(got[11])    # the largest float32 is nearer to 2^128 than to the largest bf16
    assert np.isfinite(got[13]) and np.isposinf(got[14])
    rng = np.random.default_rng(0)
    r = rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32).view(f32)
    r = r[~np.isnan(r)]
    with np.errstate(over="ignore"):
        assert np.array_equal(bm.bf16_rne(r).astype(f32).view(np.uint32), _torch_bf16(r).view(np.uint32))
    t = bm.bf16_trunc(r[np.isfinite(r)])
    assert np.all(np.abs(t) <= np.abs(r[np.isfinite(r)].astype(np.float64)))


SHAPES = bm.case_shapes()


@pytest.mark.parametrize("F,z_dim,h_dim,Dy", SHAPES)
def test_model_is_the_oracles_function_on_rounded_operands(F, z_dim, h_dim, Dy):
    """Against orc.decoder_forward (float32, unrounded operands): within 2e-2 in log2 v, the bf16 mode's own distance from
    the oracle (1.0e-2 to 1.3e-2 measured, median 1.3e-3 to 1.8e-3) -- with and without the fp32 last bin."""
    params = bm.case_params(F, z_dim, h_dim, Dy)
    ops = bm.prepare(bm.dec_list(params), z_dim)
    assert ops.F == F and ops.Dy == Dy
    g = np.random.default_rng(F + z_dim)
    z = g.standard_normal((640, z_dim)).astype(f32)
    y = (g.random((640, Dy)) > 0.5).astype(f32) if Dy else None
    ref = np.log2(orc.decoder_forward(params, z if y is None else np.concatenate([z, y], 1)).astype(np.float64))
    B1 = bm.layer1_bias(ops, y) if Dy else None
    for b1_bf16 in ((False, True) if Dy else (False,)):
        for last in (False, True):
            dev = np.abs(bm.log2_variance(ops, z, B1, b1_bf16, last) - ref)
            assert dev.max() < 2e-2 and 1e-4 < np.median(dev) < 5e-3, (dev.max(), np.median(dev))
    # the padding columns of a wider z row do not enter
    zp = np.concatenate([z, g.standard_normal((640, 8)).astype(f32)], 1)
    assert np.array_equal(bm.log2_variance(ops, zp, B1), bm.log2_variance(ops, z, B1))


@functools.lru_cache(maxsize=None)
def _decode_bounds(F, z_dim, h_dim, Dy, last):
    ops = bm.prepare(bm.dec_list(bm.case_params(F, z_dim, h_dim, Dy)), z_dim)
    di = bm.decode_inputs(F, z_dim, Dy)
    B1 = np.repeat(bm.layer1_bias(ops, di.y), bm.DECODE_R, 0) if Dy else None
    return bm.decoder_bounds(ops, di.Zs.reshape(-1, di.Zs.shape[2]), np.repeat(di.pos, bm.DECODE_R), B1, False, last)


@pytest.mark.parametrize("case", bm.DECODE_CASES, ids=[c[0] for c in bm.DECODE_CASES])
def test_decoder_statistics_separate_the_emulation_from_every_defect(case):
    """The table of the decoding path (decode_kernel: fp32 layer-1 bias rows, the fp32 last bin where F = 16 k + 1)."""
    name, F, z_dim, h_dim, Dy = case
    r = _decode_bounds(F, z_dim, h_dim, Dy, F % 16 == 1)
    bm.report("decode %s (CPU: the emulation in the place of the device)" % name, r.floor, r.bounds)
    for d, s in r.defects.items():
        print("  %-12s %s" % (d, "  ".join("%s %.2e" % kv for kv in s.items())))
    # the orders of magnitude of the issue's table
    assert 1e-9 < r.floor["bin_median"] < 5e-7 and r.floor["row_share"] < 0.08 and r.floor["max"] < 7e-3
    for k, b in r.bounds.items():
        assert b.bound is not None and b.ceiling >= bm.SEPARATION * b.floor and b.bound <= b.ceiling / 5, (k, b)
    assert 1e-6 < r.bounds["bin_median"].bound < 2e-5
    for d, s in r.defects.items():
        assert s["row_share"] == 1.0 and s["max"] < 2e-2, (d, s)       # every defect moves every row, none passes today's 5e-2
        assert s["bin_median"] > 1e-4


@functools.lru_cache(maxsize=None)
def _chain_case(name):
    _, F, z_dim, h_dim, Dy, _, _, sw = next(c for c in bm.CHAIN_CASES if c[0] == name)
    ops = bm.prepare(bm.dec_list(bm.case_params(F, z_dim, h_dim, Dy)), z_dim)
    inp = bm.chain_inputs(F, z_dim, Dy, bm.latent_columns(z_dim, h_dim))
    if Dy:
        inp.B1 = bm.layer1_bias(ops, inp.y)
    return ops, inp, sw, bm.chain_bounds(ops, inp, sw)


@pytest.mark.parametrize("name", [c[0] for c in bm.CHAIN_CASES])
def test_chain_statistics_separate_the_emulation_from_every_defect(name):
    """The table of a chain case: log-acceptances over all six steps on the emulated chain's own trajectory, and its
    stored rows bit for bit."""
    ops, inp, sw, r = _chain_case(name)
    bm.report("chain %s (CPU: the emulation in the place of the device)" % name, r.floor, r.bounds)
    for d, s in r.defects.items():
        print("  %-12s %s" % (d, "  ".join("%s %.2e" % kv for kv in s.items())))
    assert r.floor["within"] >= 0.95 and r.floor["max"] < 0.05 and r.floor["moved"] <= 0.05
    for k, b in r.bounds.items():
        assert b.bound is not None and b.ceiling >= bm.SEPARATION * b.floor and b.bound <= b.ceiling / 5, (k, b)
    for d, s in r.defects.items():
        if bm.DEFECTS[d] == "rows":                 # the conditions alone refuse these
            assert s["within"] < 0.75 and s["moved"] > bm.ROW_SHARE, (d, s)


def test_follow_chain_rebuilds_the_trajectory_and_refuses_another():
    ops, inp, sw, _ = _chain_case("wave_f65")
    rec = bm.emulate_chain(ops, inp, sw)
    zt, zp = bm.follow_chain(rec, inp, ops.Lz)
    assert np.array_equal(zt[0], inp.Z0)
    S = inp.ns + inp.burnin
    took = np.any(zt[1:] != zt[:-1], axis=(2,))
    assert 0.05 < took.mean() < 0.95                # both branches of the decision occur
    for m in range(1, S):
        assert np.array_equal(zt[m][took[m - 1]], zp[m - 1][took[m - 1]])
    for m in range(inp.burnin, S - 1):
        assert np.array_equal(zt[m + 1], rec.Zs[:, m - inp.burnin])
    bad = bm.SimpleNamespace(**vars(rec))
    bad.Zs = rec.Zs.copy()
    bad.Zs[3, 1, 0] += f32(1e-3)
    with pytest.raises(AssertionError):
        bm.follow_chain(bad, inp, ops.Lz)
