"""Cases of tests/test_gpu_buffer_contract.py, shared with tests/test_guarded_cpu.py (which checks, without a GPU, that they
reach every kernel form): the smallest shapes at which each form of the chain, streaming and decoding kernels still runs.

Frames: counts [17, 1, 30, 5] (NT = 53) are six 16-frame wave tiles, four of them partly idle -- 16+1, 1, 16+14, 5 -- and
the idle rows of the last would be rows 53..63, past the end of every buffer; a one-frame utterance; utterances that start
at rows 17, 18 and 48, off every tile boundary.  [3] is a single tile of three frames."""
from collections import namedtuple

import numpy as np

import vaenmf_oracle as orc
from dispatch_model import shape_class

COUNTS = [17, 1, 30, 5]
ONE_TILE = [3]
LARGE_COUNTS = [16] * 256 + [17, 1]          # 259 wave tiles: more than an MI355X has compute units (256)
NS, BURNIN, RCAP = 10, 3, 12                 # stored path: the fused W forms need exactly 10 or 30 samples
DECODE_SAMPLES = [(1, 4), (10, 12), (33, 40)]   # (R, Rcap) of the decoding path; 33 crosses the 32-sample chunk with a clamped r
VAR_RW = 0.01

Case = namedtuple("Case", "name F K precision z_dim h_dim counts Dy noise_psd large", defaults=(0, False, False))
H = [128, 128]
CASES = [
    Case("f9", 9, 3, "bf16x3", 32, H, COUNTS),
    Case("f9_one_tile", 9, 3, "bf16x3", 32, H, ONE_TILE),
    Case("f65_z16", 65, 10, "bf16x3", 16, H, COUNTS),              # sd_hi = 0, latent padding inside the 32 columns
    Case("f250_m2", 250, 17, "bf16x3", 32, H, COUNTS, 1),
    Case("f257_x3_noise_psd", 257, 8, "bf16x3", 32, H, COUNTS, 0, True),
    Case("f257", 257, 8, "bf16", 32, H, COUNTS),
    Case("f257_one_tile", 257, 8, "bf16", 32, H, ONE_TILE),
    Case("f273", 273, 10, "bf16x3", 32, H, COUNTS),
    Case("f273_z16", 273, 10, "bf16x3", 16, H, COUNTS),            # z_dim 16 on the team chain, which masks the draws' padding
    Case("f514_m2", 514, 8, "bf16", 32, H, COUNTS, 1),
    Case("f640", 640, 32, "bf16x3", 32, H, COUNTS),
    Case("wide_z128_h256_x3", 65, 10, "bf16x3", 128, [256, 128], COUNTS),
    Case("wide_z128_h256", 65, 10, "bf16", 128, [256, 128], COUNTS),
    Case("wide_z64_x3", 65, 10, "bf16x3", 64, H, COUNTS),
    Case("wide_z64", 65, 10, "bf16", 64, H, COUNTS),
    Case("f257_large", 257, 8, "bf16", 32, H, LARGE_COUNTS, 0, False, True),
]
BY_NAME = {c.name: c for c in CASES}
DECODE_CASES = ["f65_z16", "f257", "f250_m2", "f640"]   # the decoding entries at (1, 4) and (33, 40); (10, 12) runs in every narrow sequence


def is_wide(case):
    return case.z_dim > 32 or 256 in case.h_dim


def n_wave_tiles(counts):
    return sum((n + 15) // 16 for n in counts)


def case_class(case, n_cus=256):
    """shape_class() of the case (the streaming kernels serve wide plans unchanged); a wide plan's chain is kernel 3."""
    sc = shape_class(case.F, case.K, case.precision, n_wave_tiles(case.counts), NS, n_cus)
    if is_wide(case):
        sc.update(chain_kernel=3, chain_form="widechain")
    return sc


_cache = {}


def inputs(case):
    """Weights, spectrograms, labels, start latents, gains, noise PSD and seeds of a case (once per process; read-only)."""
    if case.name not in _cache:
        F, L, counts = case.F, case.z_dim, case.counts
        NT = sum(counts)
        g = np.random.default_rng(4000 + F + L)
        tilt = 0.5 + 3 * np.exp(-np.arange(F) / 60.0)
        d = dict(params=orc.xavier_normal_params([F, L, list(case.h_dim)], seed=7, y_dim=case.Dy, bias_std=0.05), NT=NT)
        d["Xs"] = [((g.standard_normal((n, F)) + 1j * g.standard_normal((n, F))) * tilt).astype(np.complex64) for n in counts]
        d["y"] = (g.random((NT, case.Dy)) > 0.5).astype(np.float32) if case.Dy else None
        d["Z0"] = (0.5 * g.standard_normal((NT, L))).astype(np.float32)
        d["gains"] = (0.5 + g.random(NT)).astype(np.float32)
        d["Vb"] = (g.random((NT, F)) + 0.1).astype(np.float32) if case.noise_psd else None
        d["seeds"] = [11 + u for u in range(len(counts))]
        for R, _ in DECODE_SAMPLES:
            d["Zs%d" % R] = (0.7 * g.standard_normal((NT, R, L))).astype(np.float32)
        _cache[case.name] = d
    return _cache[case.name]


# entry point -> buffers it reads (const in the header), buffers it writes.  Everything it does not write it leaves alone.
E = namedtuple("E", "reads writes")
CONTRACT = {
    "vaenmf_power_spec": E(("X",), ("X2",)),
    "vaenmf_layer1_bias": E(("y",), ("B1",)),
    "vaenmf_init_nmf": E((), ("W", "Ht", "g")),
    "vaenmf_rng_fill": E((), ("eps", "u")),
    # Z when update_Z != 0, Zs unless NULL, acc_out unless NULL; the sample-variance store is the plan's own memory
    "vaenmf_mh_chain": E(("X2", "W", "Ht", "g", "B1", "Vb", "eps", "u"), ("Z", "Zs", "acc")),
    "vaenmf_sample_store_gather": E((), ("Vs_store",)),
    "vaenmf_m_step_stored": E(("X2", "Vb"), ("W", "Ht", "g", "cost_frames")),       # with a fixed noise PSD: g and cost_frames only
    "vaenmf_wiener_stored": E(("W", "Ht", "g", "X", "Vb"), ("S_hat", "N_hat", "WFs", "WFn")),
    "vaenmf_decode": E(("Zs", "B1"), ("Vs",)),
    "vaenmf_m_step": E(("X2", "Zs", "B1", "Vb"), ("W", "Ht", "g", "cost_frames")),
    "vaenmf_wiener": E(("X2", "W", "Ht", "g", "Zs", "B1", "X", "Vb"), ("S_hat", "N_hat", "WFs", "WFn")),
    "vaenmf_em_run": E(("X2", "B1", "X", "Vb"), ("W", "Ht", "g", "Z", "Zs", "S_hat", "N_hat", "cost")),
}
# buffer -> (documented extent, padding written as zero, padding left alone); d: F, K, L, ns.  Padding in neither list is
# unspecified after a write (X2 of vaenmf_power_spec, Vs of vaenmf_sample_store_gather, the draws' columns L..Lp-1)
_all = lambda t, d: t
BUFFERS = {
    "X2": (lambda t, d: t[:, :d.F], (), ()),
    "B1": (_all, (), ()), "g": (_all, (), ()), "u": (_all, (), ()), "acc": (_all, (), ()), "cost_frames": (_all, (), ()), "cost": (_all, (), ()),
    "W": (lambda t, d: t[:, :d.F, :d.K], (lambda t, d: t[:, d.F:], lambda t, d: t[:, :, d.K:]), ()),
    "Ht": (lambda t, d: t[:, :d.K], (lambda t, d: t[:, d.K:],), ()),
    "Z": (lambda t, d: t[:, :d.L], (lambda t, d: t[:, d.L:],), ()),
    "Zs": (lambda t, d: t[:, :d.ns, :d.L], (lambda t, d: t[:, :d.ns, d.L:],), (lambda t, d: t[:, d.ns:],)),
    "eps": (lambda t, d: t[:, :, :d.L], (), ()),
    "Vs_store": (lambda t, d: t[:, :, :d.F], (), ()),
    "Vs": (lambda t, d: t[:, :, :d.F], (lambda t, d: t[:, :, d.F:],), ()),
    "S_hat": (lambda t, d: t[:, :d.F], (lambda t, d: t[:, d.F:],), ()), "N_hat": (lambda t, d: t[:, :d.F], (lambda t, d: t[:, d.F:],), ()),
    "WFs": (lambda t, d: t[:, :d.F], (lambda t, d: t[:, d.F:],), ()), "WFn": (lambda t, d: t[:, :d.F], (lambda t, d: t[:, d.F:],), ()),
}
