"""hg_stream_kernel where its rank loop and its wavefront sums can go wrong, through mh_chain / m_step_stored with the store on.

At rank <= 8 the H update takes the ranks four at a time: the lanes' partial sums of a group without a branch per rank
(lanes without real bins read bin 0's rows of W against zero statistics, padded ranks read zero columns), the in-row
chains side by side, one shared cross-row stage for the four numerators and one for the denominators, and the new
activation of rank k0 + j read from row j.  The odd-bin sums and the g / cost sums share the cross-row stage in pairs.
The shapes here are the ones where that can fail:

  F = 257     one chunk, every lane valid, the extra bin F - 1
  F = 65      one chunk, lanes 16 .. 63 without real bins, the extra bin
  K = 8, 3    full and padded groups inside KP = 8;  K = 10: KP = 16, which keeps one chain per sum
  R = 30, 10  the exact-count instantiations;  R = 7: the generic one
  counts      two utterances of 5 and 17 frames: a wavefront's block of frames crosses from one utterance's W to the next

in both precisions (bf16 and float rows).  H, g and the cost are held to the float64 formulas of
tests/test_gpu_rank_and_samples.py (in tests/em_support.py) within that file's bounds (max(floor, 16 e32), from the float32 oracle's own error), are
the same bits in a second call from the same state, and the same bits for each utterance run alone with its seed.
"""
import numpy as np
import pytest
import torch

import em_support as es
from em_support import make_engine
from helpers import need_gpu

pytestmark = pytest.mark.gpu

COUNTS2 = [5, 17]
SEEDS2 = [11, 12]
BURNIN = 3


def _prep(c, precision, idx):
    """The engine of the utterances idx of the case, in the state of es.inputs, the store on."""
    eng = make_engine(c.params, c.F, c.K, [COUNTS2[i] for i in idx], Rcap=c.R, precision=precision, seeds=[SEEDS2[i] for i in idx])
    eng.set_spectrogram([c.Xs[i] for i in idx])
    eng.init_nmf([c.W0[i] for i in idx], [c.H0[i] for i in idx])
    frames = np.concatenate([np.arange(c.off[i], c.off[i + 1]) for i in idx])
    eng.g.copy_(torch.from_numpy(c.gains[frames]))
    eng.Z.copy_(torch.from_numpy(c.Z0[frames]))
    eng.sample_store(True)
    return eng


def _m_step(eng, R):
    eng.m_step_stored()
    return dict(W=eng.W.clone(), Ht=eng.Ht.clone(), g=eng.g.clone(), cf=eng.cost_frames.clone()), eng.cost_from_frames(R)


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
@pytest.mark.parametrize("R", [30, 10, 7])
@pytest.mark.parametrize("K", [8, 3, 10])
@pytest.mark.parametrize("F", [257, 65])
def test_h_g_cost_over_rank_groups(F, K, R, precision):
    need_gpu()
    c = es.inputs(F, K, R, counts=COUNTS2)
    tag = "%s F=%d K=%d R=%d" % (precision, F, K, R)
    eng = _prep(c, precision, [0, 1])
    assert eng.Kp == (8 if K <= 8 else 16) == es.query(eng, "Q_KP")
    eng.mh_chain(R, BURNIN, 0.01, call=0)
    V = eng.stored_variances(R).cpu().numpy()
    assert np.all(np.isfinite(V)) and np.all(V[:, :, :F] > 0)
    # the float64 formulas from the state before the M-step and the rows the device stored
    refs = []
    for u in range(2):
        o = es.oracle_at(c, eng, u)
        o.Vs = np.ascontiguousarray(np.moveaxis(V[eng.utt_slice(u), :, :F], 0, -1))     # (R, F, N)
        refs.append(es.reference(o, "M1"))
    pre = [t.clone() for t in (eng.W, eng.Ht, eng.g)]
    first, cost = _m_step(eng, R)
    failures = []
    es.compare(tag, refs, lambda u: es.device_m_step(c, eng, u, cost, "M1"), failures)
    es.padding_is_zero(eng)
    # a second call from the same state: the same bits
    for t, p in zip((eng.W, eng.Ht, eng.g), pre):
        t.copy_(p)
    second, _ = _m_step(eng, R)
    for k in first:
        assert torch.equal(first[k], second[k]), (tag, k, "second call")
    # every utterance alone, with its seed: the same stored rows, the same bits
    for u in range(2):
        one = _prep(c, precision, [u])
        one.mh_chain(R, BURNIN, 0.01, call=0)
        sl = eng.utt_slice(u)
        assert np.array_equal(one.stored_variances(R).cpu().numpy(), V[sl]), (tag, u, "stored rows")
        alone, _ = _m_step(one, R)
        assert torch.equal(alone["Ht"], first["Ht"][sl]), (tag, u, "H alone")
        assert torch.equal(alone["g"], first["g"][sl]), (tag, u, "g alone")
        assert torch.equal(alone["cf"][:COUNTS2[u]], first["cf"][sl]), (tag, u, "cost alone")
        assert torch.equal(alone["W"][0], first["W"][u]), (tag, u, "W alone")
        one.sample_store(False)
    eng.sample_store(False)
    assert not failures, failures
