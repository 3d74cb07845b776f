"""The grouped wavefront sums of common.h against the one-value ones, bit for bit.

wave_sum(v) = sum_rows4(sum_row16(v)) adds a wavefront's 64 values in a fixed tree: within each 16-lane row by DPP, then
(r0 + r1) + (r2 + r3) across the rows with v_permlane16_swap / v_permlane32_swap.  sum_rows4_x2 / sum_rows4_x4 share the
cross-row stage among two / four values by feeding the swaps two different registers; every total still comes from the
same tree, so it has to have the same bits, and it has to stand in the documented lanes: total j of sum_rows4_x4 in
lanes 16 j .. 16 j + 15, the two totals of sum_rows4_x2 in rows (0, 2) and (1, 3).  vaenmf_wave_sum_probe writes what every
lane holds after each form.

The float64 bound.  The tree has depth 6; each addition rounds its result, at most the sum of the magnitudes below it, by
2^-24 relative, so a total differs from the exact sum by at most 6 * 2^-24 * sum|x| to first order.  The test asks for
64 * 2^-24 * sum|x| (the bound of a sum of 64 terms in any order).  Magnitudes reach 1e30, 64 of them 6.4e31, far below
the float32 maximum, and 1e-30 is a normal number.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import need_gpu

pytestmark = pytest.mark.gpu


def _sets():
    """[n][4][64] float32: mixed signs and magnitudes 1e-30 .. 1e30 within one set, exact zeros, rows of zeros."""
    rng = np.random.default_rng(20)
    out = []

    def wide(shape):
        return (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-30, 30, shape)).astype(np.float32)

    for i in range(96):                                   # every value of the set at its own scale and sign
        out.append(wide((4, 64)))
    for i in range(64):                                   # the same with exact zeros sprinkled in
        x = wide((4, 64))
        x[rng.random((4, 64)) < 0.3] = 0.0
        out.append(x)
    for i in range(64):                                   # one 16-lane row of one or all values exactly zero
        x = wide((4, 64))
        q = i % 4
        if i < 32:
            x[:, 16 * q:16 * q + 16] = 0.0
        else:
            x[(i // 4) % 4, 16 * q:16 * q + 16] = 0.0
        out.append(x)
    for i in range(32):                                   # moderate values: every addition rounds
        out.append(rng.standard_normal((4, 64)).astype(np.float32))
    for i in range(16):                                   # one value per set all zero, one a single non-zero lane
        x = wide((4, 64))
        x[i % 4] = 0.0
        x[(i + 1) % 4] = 0.0
        x[(i + 1) % 4, (7 * i) % 64] = np.float32(3.0)
        out.append(x)
    out.append(np.zeros((4, 64), np.float32))
    # which value and which row a total came from: value q is 2^q in row q alone, so total q is 16 * 2^q
    x = np.zeros((4, 64), np.float32)
    for q in range(4):
        x[q, 16 * q:16 * q + 16] = 2.0 ** q
    out.append(x)
    return np.stack(out)


def _probe(x):
    from vaenmf import _lib
    lib = _lib.lib()
    n = x.shape[0]
    xd = torch.from_numpy(x).cuda().contiguous()
    one = torch.full((n, 4, 64), float("nan"), device="cuda")
    x4 = torch.full((n, 64), float("nan"), device="cuda")
    x2 = torch.full((n, 2, 64), float("nan"), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.vaenmf_wave_sum_probe(C.c_void_p(xd.data_ptr()), n, C.c_void_p(one.data_ptr()), C.c_void_p(x4.data_ptr()),
                                         C.c_void_p(x2.data_ptr()), C.c_void_p(st)))
    torch.cuda.synchronize()
    return one.cpu().numpy(), x4.cpu().numpy(), x2.cpu().numpy()


def test_grouped_wave_sums_equal_the_single_ones_bit_for_bit():
    need_gpu()
    x = _sets()
    n = x.shape[0]
    assert 200 <= n <= 400
    one, x4, x2 = _probe(x)
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert np.all(np.isfinite(one)) and np.all(np.isfinite(x4)) and np.all(np.isfinite(x2))
    # the single sums: every lane holds the total
    assert np.array_equal(bits(one), np.broadcast_to(bits(one[:, :, :1]), one.shape))
    ref = one[:, :, 0]                                                     # [n][4]
    # sum_rows4_x4: lanes 16 j .. 16 j + 15 hold total j
    want4 = np.repeat(ref, 16, axis=1)                                     # [n][64]
    bad = np.argwhere(bits(x4) != bits(want4))
    assert bad.size == 0, (bad[:5], x4[tuple(bad[0])], want4[tuple(bad[0])])
    # sum_rows4_x2 of the pairs (0, 1) and (2, 3): rows 0 and 2 the first total, rows 1 and 3 the second
    want2 = np.stack([np.tile(np.repeat(ref[:, 0:2], 16, axis=1), (1, 2)), np.tile(np.repeat(ref[:, 2:4], 16, axis=1), (1, 2))], axis=1)
    bad = np.argwhere(bits(x2) != bits(want2))
    assert bad.size == 0, (bad[:5], x2[tuple(bad[0])], want2[tuple(bad[0])])
    # both against float64
    x64 = x.astype(np.float64)
    exact, mag = x64.sum(-1), np.abs(x64).sum(-1)
    bound = 64 * 2.0 ** -24 * mag
    for name, got in (("single", ref), ("x4", x4[:, ::16]), ("x2", np.concatenate([x2[:, 0, :32:16], x2[:, 1, :32:16]], axis=1))):
        err = np.abs(got.astype(np.float64) - exact)
        worst = float(np.max(err / np.where(mag > 0, bound, 1.0)))
        print("%s against float64: largest error %.3f of the bound" % (name, worst))
        assert np.all(err <= bound), (name, np.argwhere(err > bound)[:5])
    # the marker set: value q lives in row q alone
    assert np.array_equal(ref[-1], np.array([16.0, 32.0, 64.0, 128.0], np.float32))
    assert np.array_equal(ref[-2], np.zeros(4, np.float32))
