"""Cases of tests/test_gpu_persistent_loops.py, shared with tests/test_persistent_loops_cpu.py (which checks, without a GPU,
that they reach a second trip of every persistent loop): the case tables and the oracle's replayed chains."""
import functools
from types import SimpleNamespace

import numpy as np

import vaenmf_oracle as orc
from em_support import inputs

# ---- the chain: a second ragged batch of 204 frames in 18 wave tiles, one workgroup
CHAIN_COUNTS = [21, 40, 9, 1, 16, 33, 17, 3, 64]
CHAIN_K, CHAIN_R = 10, 10
# (F, precision, labels): F = 9 / 64 wchain<5>, 80 <5,exact> (bf16x3: the lo fragments of W3 in LDS), 201 <17>, 257 <17,exact>,
# 514 <33> (bf16 only; VAENMF_WCHAIN4=0 keeps the 17- and 33-tile bf16 shapes of this small batch on wchain_kernel); labels:
# four wavefronts keep the layer-1 bias rows in registers (bf16x3), eight park them in LDS (bf16)
CHAIN_CASES = [(9, "bf16x3", False), (80, "bf16x3", False), (201, "bf16x3", False), (257, "bf16x3", False), (201, "bf16x3", True),
               (64, "bf16", False), (80, "bf16", False), (201, "bf16", False), (257, "bf16", False), (514, "bf16", False),
               (257, "bf16", True)]
CHAIN_FORMS = {"bf16x3": {"wchain<5>", "wchain<5,exact>", "wchain<17>", "wchain<17,exact>"},
               "bf16": {"wchain<5>", "wchain<5,exact>", "wchain<17>", "wchain<17,exact>", "wchain<33,GT33>"}}
# generator seed of a chain case's inputs when it is not 1000 + F: (F, labels) -> seed, chosen so that the ORACLE's decision
# margins leave out at most 15 % of the frames (tests/test_persistent_loops_cpu.py asserts it; no device result enters)
CHAIN_SEEDS = {}
MAX_LEFT_OUT = 0.15

# ---- the streaming kernels: the batch of the sweeps, one, two and four workgroups.  70 frames give 4 and 8 wavefronts blocks
# of 18 and 9 frames, the last one clipped, none empty (4 * 18 = 8 * 9 = 72 < 70 + per); cap 4 (blocks of 5) leaves the last
# two of 16 wavefronts without a frame and, at rank > 8, a workgroup that lies inside the utterance it staged.
STREAM_CAPS = (1, 2, 4)
# (F, K, R, variant, precision, switches)
STREAM_CASES = [
    (64, 4, 10, "M1", "bf16", {"VAENMF_WFUSED": "0"}),        # wstats_stream2 (bf16 rows), hg<RT 10>
    (64, 4, 30, "M1", "bf16x3", {}),                          # float rows: wstats_stream at rank 8 through the batch loop, hg<RT 30>
    (201, 8, 7, "M1", "bf16", {}),                            # TAIL; wstats_stream2, generic count
    (201, 8, 30, "M1", "bf16", {"VAENMF_WFUSED": "0"}),       # wstats_stream2 with 30 of 32 rows
    (201, 4, 7, "M1", "bf16x3", {}),                          # wstats_stream2 (float rows)
    (201, 10, 30, "M1", "bf16", {}),                          # rank 16, one chunk of bf16 rows: two half batches of 16 (30 rows)
    (251, 10, 10, "M1", "bf16x3", {}),                        # rank 16, W per workgroup; two half batches of 8 refilled a frame ahead
    (257, 8, 10, "M2", "bf16", {"VAENMF_WFUSED": "0"}),       # labels; the extra bin (wx / nw refreshed per utterance)
    (257, 8, 30, "noNMF", "bf16", {}),                        # fixed noise PSD: gains only
    (442, 10, 30, "M1", "bf16", {}),                          # two chunks, TAIL, rank 16
    (442, 32, 10, "M1", "bf16x3", {}),                        # two chunks, rank 32 in LDS
    (514, 10, 10, "M1", "bf16", {}),                          # three chunks: two half batches of 5
    (514, 32, 7, "M1", "bf16x3", {}),                         # three chunks, float rows (RB 5, HB 2), a partial last batch
    (640, 4, 30, "M1", "bf16", {}),                           # three chunks at rank 8: the wave-private W restaged per utterance
    (640, 32, 10, "M1", "bf16x3", {}),                        # W too large for LDS: every frame reads global memory
]

# ---- the tile loop of decode_kernel: (F, K, R, precision); caps 1 and 2
TILE_CAPS = (1, 2)
TILE_CASES = [(250, 8, 33, "bf16x3"), (250, 10, 10, "bf16"), (321, 8, 10, "bf16"), (321, 10, 33, "bf16x3"), (512, 8, 33, "bf16"),
              (512, 32, 10, "bf16x3"), (640, 8, 10, "bf16x3"), (640, 32, 33, "bf16")]


@functools.lru_cache(maxsize=None)
def chain_inputs(F, labels):
    return inputs(F, CHAIN_K, CHAIN_R, Dy=1 if labels else 0, counts=CHAIN_COUNTS, seed=CHAIN_SEEDS.get((F, labels)))


def replay_oracle(c, u):
    """The oracle's chain of utterance u from the state of inputs() on the replayed draws: (log-acceptances [steps, n],
    decisions, samples [n, ns, 32], frames whose every decision is at least 1e-2 from its threshold)."""
    sl = slice(c.off[u], c.off[u + 1])
    o = orc.MCEMOracle("M2" if c.Dy else "M1", 1)
    o.init_parameters(c.Xs[u], c.params, c.K, 1e-8, orc.NumpyRNG(0), y=c.ys[u], W0=c.W0[u], H0=c.H0[u])
    o.g = c.gains[sl].copy()
    draws = []
    for m in range(c.S_steps):
        draws += [c.eps[m, sl].T.copy(), c.uu[m, sl].copy()]
    o.rng = orc.ReplayRNG(draws)
    tr = []
    Zs_ref = o.sample_posterior(c.Z0[sl].T.copy(), c.ns, c.S_steps - c.ns, trace=tr)
    acc = np.stack([t["acc"] for t in tr])
    keep = np.abs(np.log(c.uu[:, sl]) - acc).min(0) > 1e-2
    return SimpleNamespace(sl=sl, acc=acc, is_acc=np.stack([t["is_acc"] for t in tr]), Zs=Zs_ref, keep=keep)


@functools.lru_cache(maxsize=None)
def chain_reference(F, labels):
    """Computed once per (F, labels), shared by both precisions and the CPU test, left unchanged."""
    c = chain_inputs(F, labels)
    refs = [replay_oracle(c, u) for u in range(len(c.counts))]
    return refs, 1.0 - float(np.concatenate([r.keep for r in refs]).mean())
