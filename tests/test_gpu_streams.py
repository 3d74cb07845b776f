"""Every entry point that takes a stream, on a stream that is not the null stream and inside a caller's graph.

The rest of the suite runs in a process whose current stream is the legacy null stream: every launch it has checked went
out with stream == 0.  Here every case of tests/stream_cases.py runs three ways, and the reference of each comparison is
the same C-ABI call on the default stream with ordinary torch allocations -- the path the rest of the suite holds to the
oracle and to float64.  Bit equality is the bound: the header promises run-to-run identical bits for these entry points.

Gate form.  All work of a case is on a side stream s.  Its outputs are poison, its float inputs on the device are poison
(the NaN word and 1e30 of tests/guarded.py in turn), the real values wait in staging tensors; tables and maps -- whatever
a kernel turns into an address or a loop bound -- hold their valid values throughout, so that a launch on the wrong
stream reads poison and never an invalid address.  On s: a sleep of G ms, the event gate_end, the copies from staging into
the inputs, the call.  When the call returns gate_end must not have happened (the call did not wait for its stream), nor
after the null stream has been synchronised (whatever the call put there has then run, against poison).  After s has
finished, outputs, padding and inputs are compared.  A gate that ran out before the call returned says nothing: the
attempt is repeated once with a gate four times as long, and a second such attempt fails as `inconclusive`.
The entry points the header marks as synchronising, and the capturing call of vaenmf_em_run (hipGraphInstantiate is the
runtime's), are held to the comparison alone.

Capture form.  The calls of a case are captured into a torch.cuda.CUDAGraph on s after one eager warm-up with contents A
(every call returns 0 and the capture ends: no allocation, no copy to the host, no synchronisation); the graph is then
replayed on contents B -- other float data, other in-range maps, other utterance seeds -- and on A again.  A launch that
escaped the capture, or a value baked in at capture time that the header says is read at run time, shows as A's results
or as poison.

Whole path.  Two Reconstructors on two streams, their calls interleaved on the host behind one gate each, against each
one's solo run on the default stream: the Python wrappers, the process-wide caches and any scratch that is not per call.

G is no tolerance -- the checks are sound for any G; it decides how often an attempt is inconclusive.  G_MS is 20 times
the longest warm host time of any case's call, measured on an MI355X host, rounded up to 10 ms."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import stream_cases as sc
from guarded import same_bits
from helpers import need_gpu

pytestmark = pytest.mark.gpu

G_MS = 10.0                    # 20 x 0.434 ms (the M2 trainer's 75 calls), rounded up to a whole 10 ms; DESIGN.md 4.3
CASES = sc.by_name()


# ---------------------------------------------------------------------------------------------------------------- gate
@functools.lru_cache(maxsize=None)
def _cycles_per_ms():
    """torch.cuda._sleep spins for a number of device clock cycles: timed once with two events."""
    need = 20_000_000
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    a.record()
    torch.cuda._sleep(need)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b)
    assert ms > 1.0, ms
    return need / ms


def _gate(ms):
    torch.cuda._sleep(int(ms * _cycles_per_ms()))


# --------------------------------------------------------------------------------------------------- per-case, computed once
@functools.lru_cache(maxsize=None)
def _prepared(name):
    """State, contents A and B on the device, and the default-stream results of both: computed once, never modified.  The
    default-stream runs are also the warm-up (first-use tables, kernel attributes, the plan's host state)."""
    case = CASES[name]
    specs = [case.make(seed) for seed in sc.SEEDS]
    state = case.open(specs[0]) if case.open else None
    p = SimpleNamespace(case=case, state=state, specs=specs, staged=[sc.stage(s) for s in specs], ref=[], keep=[])
    for spec, staged in zip(specs, p.staged):
        first, b = sc.run_default(case, state, spec, staged)
        prefill = {n: first[-1][n] for n in spec.prefill}
        res, b2 = sc.run_default(case, state, spec, staged, prefill)
        for x, y in zip(first, res):          # run-to-run identical bits: what makes bit equality the bound of this file
            for n in x:
                assert same_bits(x[n], y[n]), "%s: two default-stream runs differ in %s" % (name, n)
        p.ref.append(res)
        p.keep += [b, b2]                     # (their addresses stay taken: a later run is a new signature for vaenmf_em_run)
    torch.cuda.synchronize()
    return p


@pytest.fixture(scope="module", autouse=True)
def _release_prepared_cases():
    """The plans, trainers and buffers of the cases live for this file alone."""
    yield
    _prepared.cache_clear()


def _attempt(p, s, step, ms, b):
    """One gated run of one step -> (pending when the call returned, pending after the null stream drained, return codes)."""
    case, staged = p.case, p.staged[0]
    sc.repoison(case, b, {n: p.ref[0][-1][n] for n in b.spec.prefill})
    gate_end = torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        _gate(ms)
        gate_end.record(s)
        sc.load(case, b, staged, s.cuda_stream)
        rc = case.call(b, s.cuda_stream, step)
    first = not gate_end.query()
    torch.cuda.default_stream().synchronize()
    second = not gate_end.query()
    s.synchronize()
    torch.cuda.synchronize()
    return first, second, rc


@pytest.mark.parametrize("name", list(CASES))
def test_gate(name):
    need_gpu()
    p = _prepared(name)
    case, spec = p.case, p.specs[0]
    s = torch.cuda.Stream()
    problems = []
    for attempt, ms in enumerate((G_MS, 4 * G_MS)):
        if case.before is not None:
            case.before(p.state)
        b = sc.alloc(case, spec, p.state, p.staged[0], {n: p.ref[0][-1][n] for n in spec.prefill})
        p.keep.append(b)
        inconclusive = []
        for step, (label, must_pend) in enumerate(case.steps):
            what = "%s %s" % (name, label)
            first, second, rc = _attempt(p, s, step, ms, b)
            assert all(v == 0 for v in rc), (what, rc, sc.L().vaenmf_last_error().decode())
            print("%s: gate %.0f ms, pending at return %s, after the null stream %s" % (what, ms, first, second))
            if "vaenmf_em_run" in case.entries:
                from em_support import query
                assert query(p.state.eng, "Q_EM_GRAPH") == (0, 1, 1)[step], (what, query(p.state.eng, "Q_EM_GRAPH"))
            if must_pend and not case.syncs and not (first and second):
                inconclusive.append((name, label, ms, first, second))
            problems += sc.compare(case, b, p.ref[0][step], p.staged[0], what)
        assert not problems, "\n  ".join(["%d differences from the default-stream run:" % len(problems)] + problems[:12])
        if not inconclusive:
            return
        print("inconclusive at a gate of %.0f ms: %s" % (ms, inconclusive))
    raise AssertionError("inconclusive twice: the gate had ended when the call returned (a wait the header does not state, or a host "
                         "slower than %.0f ms): %s" % (4 * G_MS, inconclusive))


# ------------------------------------------------------------------------------------------------------------- capture
CAPTURABLE = [n for n, c in CASES.items() if c.capture is None]
# outputs that may or must be the same for contents A and B: STOI's frame decisions, the classifier head's counts, and the
# training draws, which are keyed by (seed, step, row) alone
SAME_IN_BOTH = ("keep", "counts", "counts_b", "row_cnt", "eps_out", "eps1")


@pytest.mark.parametrize("name", CAPTURABLE)
def test_capture(name):
    need_gpu()
    p = _prepared(name)
    case = p.case
    assert len(case.steps) == 1 and not case.syncs
    s = torch.cuda.Stream()
    b = sc.alloc(case, p.specs[0], p.state, p.staged[0], {n: p.ref[0][-1][n] for n in p.specs[0].prefill})
    p.keep.append(b)
    with torch.cuda.stream(s):                # 1. eager warm-up on s, contents A
        sc.load(case, b, p.staged[0], s.cuda_stream)
        rc = case.call(b, s.cuda_stream, 0)
    s.synchronize()
    assert all(v == 0 for v in rc), (name, "warm-up", rc)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):       # 2. / 3. the C-ABI calls alone
        rc = case.call(b, s.cuda_stream, 0)
    assert all(v == 0 for v in rc), (name, "captured", rc, sc.L().vaenmf_last_error().decode())
    problems = []
    for which in (1, 0):                      # 6. - 8. contents B, then A again
        b.spec = p.specs[which]               # (shapes, host tables and scalars are A's: the two share them)
        sc.repoison(case, b, {n: p.ref[which][-1][n] for n in b.spec.prefill})
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            sc.load(case, b, p.staged[which], s.cuda_stream)
            g.replay()
        s.synchronize()
        torch.cuda.synchronize()
        problems += sc.compare(case, b, p.ref[which][0], p.staged[which], "%s replayed on contents %s" % (name, "AB"[which]))
    for n in case.outs:                       # the two contents do give different results: a replay of stale values would show
        assert not same_bits(p.ref[0][0][n.name], p.ref[1][0][n.name]) or n.name in SAME_IN_BOTH, (name, n.name)
    assert not problems, "\n  ".join(["%d differences from the default-stream run:" % len(problems)] + problems[:12])


# ---------------------------------------------------------------------------------------------------------- whole path
def _reconstructor(F, precision, nfft):
    import vaenmf_oracle as orc
    from vaenmf.pipeline import Reconstructor
    params = orc.xavier_normal_params([F, 32, [128, 128]], seed=7, bias_std=0.05)
    return Reconstructor(params, F, 8, niter=2, nsamples_E_step=10, burnin_E_step=3, nsamples_WF=10, burnin_WF=3, model="M1",
                         reference_compat=False, fs=16000, wlen_sec=nfft / 16000.0, precision=precision, max_frames=512, max_utts=8)


def _whole(r, wav, clean, counts):
    """enhance, then the Gram sums and ESTOI of its result: -> (s_hat, n_hat, cost, G, d), nothing synchronised."""
    from vaenmf import metrics
    s_hat, n_hat, cost = r.enhance(wav, counts, seeds=[3 + u for u in range(len(counts))])
    return (s_hat, n_hat, cost, metrics.gram3_batch_device(s_hat, clean, n_hat, counts), metrics.stoi_batch_device(clean, s_hat, counts, 16000))


def test_two_reconstructors_on_two_streams():
    need_gpu()
    from vaenmf import metrics
    jobs = []
    for i, (F, precision, nfft, counts) in enumerate(((33, "bf16", 64, [1000, 700, 450]), (201, "bf16x3", 400, [6000, 4100]))):
        g = np.random.default_rng(50 + i)
        clean = torch.from_numpy(g.standard_normal(sum(counts)).astype(np.float32) * 0.1).cuda()
        wav = (clean + torch.from_numpy(g.standard_normal(sum(counts)).astype(np.float32) * 0.05).cuda()).contiguous()
        jobs.append(SimpleNamespace(r=_reconstructor(F, precision, nfft), wav=wav, clean=clean, counts=counts, s=torch.cuda.Stream()))
    for j in jobs:                            # solo on the default stream, twice: the warm-up, then the reference
        _whole(j.r, j.wav, j.clean, j.counts)
        j.ref = [t.clone() for t in _whole(j.r, j.wav, j.clean, j.counts)]
    torch.cuda.synchronize()
    parts = [[], []]
    for j in jobs:
        with torch.cuda.stream(j.s):
            _gate(G_MS / 4)
    for i, j in enumerate(jobs):              # interleaved on the host, each on its own stream, nothing synchronised until the end
        with torch.cuda.stream(j.s):
            parts[i] = list(j.r.enhance(j.wav, j.counts, seeds=[3 + u for u in range(len(j.counts))]))
    for i, j in enumerate(jobs):
        with torch.cuda.stream(j.s):
            parts[i].append(metrics.gram3_batch_device(parts[i][0], j.clean, parts[i][1], j.counts))
    for i, j in enumerate(jobs):
        with torch.cuda.stream(j.s):
            parts[i].append(metrics.stoi_batch_device(j.clean, parts[i][0], j.counts, 16000))
    torch.cuda.synchronize()
    for i, j in enumerate(jobs):
        for name, got, ref in zip(("s_hat", "n_hat", "cost", "gram", "estoi"), parts[i], j.ref):
            assert bool(torch.isfinite(ref).all()), (i, name)
            assert same_bits(got, ref), "reconstructor %d: %s on its own stream beside the other differs from its solo run" % (i, name)
