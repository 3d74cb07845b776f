"""The host driver as a state machine: vaenmf_em_run with its cost ring and graph cache (csrc/driver.hip),
vaenmf_bind_batch_async with its seed ring and vaenmf_profile_* (csrc/plan.hip), vaenmf_init_nmf and cost_reduce_kernel
(csrc/aux.hip).  What a call does depends on the calls before it on the same plan; every test here drives ONE plan through
a sequence and holds each call to a reference that has no history.

Reference: the step-by-step calls on a fresh BatchEngine -- mh_chain(call=it), m_step_stored / m_step, cost_from_frames,
then the Wiener chain (call=niter, update_Z=False) and wiener_stored / wiener -- as in
test_gpu_parity.test_fused_run_equals_stepwise_and_batches_are_independent.  Never another fused call on the same plan
(the seed-ring test alone compares with a fresh engine's FIRST fused call: the long-run test has held that to the
step-by-step calls, and what it tests is the rebind).

Bounds (those of that test, nothing new): S_hat, N_hat and W, Ht, g, Z after the run bit for bit (torch.equal); costs
1e-12 relative (the host adds the per-frame doubles in another order than cost_reduce_kernel).  vaenmf_init_nmf against
oracle.nmf_init_device: integer work and one exact conversion, bit for bit.

Three engine shapes, so that both wave-private chain kernels and more than one W-statistics form appear
(test_sweep_reaches_more_than_one_chain_kernel_and_w_statistics_form):
    F = 65,  K = 4  (Kp 8),  bf16x3, the weights of tests/golden/m1_f65.npz (M2: m2_ibm_f65.npz)
    F = 257, K = 8  (Kp 8),  bf16: the bench's small-batch kernels
    F = 129, K = 10 (Kp 16), bf16
VAENMF_GRAPH is never set here: the library reads it once per process."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vaenmf_oracle as orc
from em_support import dec_list
from helpers import load_case, need_gpu

# sample capacity and (nsE, biE, nsWF, biWF) per shape: as small as the kernels allow.  The fused / per-group W statistics run
# with exactly 10 or 30 samples per frame only (stream.hip: stream_form), so the bench-like shape takes 10
RCAP = {"f65": 6, "f257": 10, "f129": 6}
SAMPLES = {"f65": (4, 2, 5, 3), "f257": (10, 2, 5, 3), "f129": (4, 2, 5, 3)}
MF, MU = 128, 4                # frame / utterance capacity: the buffers (and so the graph signatures' pointers) do not move
COST_RTOL = 1e-12
NITERS = (1, 24, 25, 26, 51)   # around the cost ring's chunk of 25 iterations, and two chunks plus one

SHAPES = {"f65": (65, 4, "bf16x3"), "f257": (257, 8, "bf16"), "f129": (129, 10, "bf16")}
REACHED = {}                   # shape -> (VAENMF_Q_CHAIN_KERNEL, VAENMF_Q_W_FUSED) of a stored M1 run


@functools.lru_cache(maxsize=None)
def _params(shape, m2=False):
    F = SHAPES[shape][0]
    if shape == "f65":
        return load_case("m2_ibm_f65" if m2 else "m1_f65")[1]
    return orc.xavier_normal_params([F, 32, [128, 128]], seed=5, y_dim=F if m2 else 0, bias_std=0.05)


def _query(eng, name):
    from vaenmf import _lib
    return int(_lib.lib().vaenmf_plan_query(eng._plan, getattr(_lib, name)))


def _spec(shape="f65", counts=(30, 50), seeds=None, niter=3, nsE=None, biE=None, nsWF=None, biWF=None, var_rw=0.01, m2=False,
          labels=False, noise=False, store=None, data=0):
    nsE, biE, nsWF, biWF = [d if v is None else v for v, d in zip((nsE, biE, nsWF, biWF), SAMPLES[shape])]
    counts = tuple(int(n) for n in counts)
    seeds = tuple(seeds) if seeds is not None else tuple(11 + 7 * u for u in range(len(counts)))
    assert not labels or m2
    return SimpleNamespace(shape=shape, counts=counts, seeds=seeds, niter=niter, nsE=nsE, biE=biE, nsWF=nsWF, biWF=biWF,
                           var_rw=var_rw, m2=m2, labels=labels, noise=noise, store=store, data=data)


def _with(spec, **kw):
    d = dict(vars(spec))
    d.update(kw)
    return _spec(**d)


@functools.lru_cache(maxsize=None)
def _inputs(shape, counts, data):
    """Spectrogram, NMF start, latent start, labels and a noise PSD for a batch: a function of the shape, the frame
    structure and a data seed only."""
    F, K, _ = SHAPES[shape]
    NT = sum(counts)
    g = np.random.default_rng([F, data] + list(counts))
    Xs = [((g.standard_normal((n, F)) + 1j * g.standard_normal((n, F))) * (1 + 3 * np.exp(-np.arange(F) / 40.0))).astype(np.complex64) for n in counts]
    W0 = [np.maximum(g.random((F, K)), 1e-8).astype(np.float32) for _ in counts]
    H0 = [np.maximum(g.random((K, n)), 1e-8).astype(np.float32) for n in counts]
    Z0 = (0.3 * g.standard_normal((NT, 32))).astype(np.float32)
    y = (g.random((NT, F)) > 0.5).astype(np.float32)
    Vb = (g.random((NT, F)) + 0.1).astype(np.float32)
    return SimpleNamespace(Xs=Xs, W0=W0, H0=H0, Z0=torch.from_numpy(Z0), y=torch.from_numpy(y), Vb=torch.from_numpy(Vb))


def _engine(shape, m2=False, max_frames=MF, max_utts=MU):
    from vaenmf.engine import BatchEngine
    F, K, prec = SHAPES[shape]
    return BatchEngine(F, K, dec_list(_params(shape, m2)), precision=prec, max_frames=max_frames, max_utts=max_utts, z_dim=32)


def _load(eng, spec):
    """Bind the batch of `spec` and put its start state on the device: what a caller does before every eng.run."""
    inp = _inputs(spec.shape, spec.counts, spec.data)
    eng.bind(spec.counts, Rcap=RCAP[spec.shape], seeds=list(spec.seeds))
    eng.set_spectrogram(inp.Xs)
    eng.init_nmf(inp.W0, inp.H0)
    eng.Z.copy_(inp.Z0)
    if spec.labels:
        eng.set_labels(inp.y)
    if spec.noise:                                       # at one address per engine, like the engine's own buffers
        if getattr(eng, "_vb_buf", None) is None:
            eng._vb_buf = torch.zeros(MF, eng.Fs, device=eng.device)
        eng._vb_buf[:eng.NT, :eng.F].copy_(inp.Vb)
        eng.set_noise_psd(eng._vb_buf[:eng.NT])
    else:
        eng.set_noise_psd(None)


def _state(eng):
    return SimpleNamespace(W=eng.W.clone(), Ht=eng.Ht.clone(), g=eng.g.clone(), Z=eng.Z.clone())


def _stepwise(spec, niters=None):
    """{niter: result} by the step-by-step calls on a fresh engine.  E-step `it` uses call = it whatever niter is, so ONE
    loop to max(niters) gives every cost prefix; the state after each niter is kept, and restored for that niter's
    Wiener chain (call = niter) and filter."""
    niters = tuple(niters) if niters is not None else (spec.niter,)
    stored = spec.store is None
    eng = _engine(spec.shape, spec.m2)
    _load(eng, spec)
    if stored:
        eng.sample_store(True)
    cost = np.zeros((len(spec.counts), max(niters)))
    snaps = {}
    for it in range(max(niters)):
        eng.mh_chain(spec.nsE, spec.biE, spec.var_rw, call=it)
        if stored:
            eng.m_step_stored()
        else:
            eng.m_step(spec.nsE)
        cost[:, it] = eng.cost_from_frames(spec.nsE)
        if it + 1 in niters:
            snaps[it + 1] = _state(eng)
    assert np.all(np.isfinite(cost)) and np.all(cost != 0)
    out = {}
    for n in niters:
        s = snaps[n]
        eng.W.copy_(s.W); eng.Ht.copy_(s.Ht); eng.g.copy_(s.g); eng.Z.copy_(s.Z)
        eng.mh_chain(spec.nsWF, spec.biWF, spec.var_rw, call=n, update_Z=False)
        S, N, _, _ = eng.wiener_stored() if stored else eng.wiener(spec.nsWF)
        assert torch.equal(eng.Z, s.Z)                   # (the Wiener chain leaves Z alone)
        out[n] = SimpleNamespace(cost=cost[:, :n].copy(), S=S.clone(), N=N.clone(), state=s)
    eng.close()
    return out


def _fused(eng, spec):
    """One eng.run of `spec` from its start state; the outputs, the state it left and which path ran."""
    _load(eng, spec)
    cost, S, N = eng.run(spec.niter, spec.nsE, spec.biE, spec.nsWF, spec.biWF, spec.var_rw, store=spec.store)
    return SimpleNamespace(cost=cost.cpu().numpy(), S=S, N=N, state=_state(eng), graph=_query(eng, "Q_EM_GRAPH"),
                           chain_kernel=_query(eng, "Q_CHAIN_KERNEL"), w_fused=_query(eng, "Q_W_FUSED"))


def _check(out, ref, tag):
    assert out.cost.shape == ref.cost.shape, tag
    err = float(np.max(np.abs(out.cost - ref.cost) / np.abs(ref.cost)))
    print("%s: cost rel err %.2e" % (tag, err))
    assert err < COST_RTOL, (tag, err, np.argwhere(np.abs(out.cost - ref.cost) / np.abs(ref.cost) >= COST_RTOL)[:4].tolist())
    assert torch.equal(out.S, ref.S) and torch.equal(out.N, ref.N), tag
    for name in ("W", "Ht", "g", "Z"):
        assert torch.equal(getattr(out.state, name), getattr(ref.state, name)), (tag, name)


def _bit_equal(a, b):
    return (np.array_equal(a.cost, b.cost) and torch.equal(a.S, b.S) and torch.equal(a.N, b.N)
            and all(torch.equal(getattr(a.state, n), getattr(b.state, n)) for n in ("W", "Ht", "g", "Z")))


def _kernels(shape):
    """(chain kernel, W-statistics form) of a stored M1 run at this shape."""
    if shape not in REACHED:
        eng = _engine(shape)
        r = _fused(eng, _spec(shape, LONG_COUNTS[shape], niter=1))
        REACHED[shape] = (r.chain_kernel, r.w_fused)
        eng.close()
    return REACHED[shape]


# ragged, at most ~120 frames, an utterance that is no multiple of 16 frames in each
LONG_COUNTS = {"f65": (37, 16, 50), "f257": (45, 64), "f129": (21, 40, 9, 33)}

LONG_CASES = [("f65", "m1"), ("f257", "m1"), ("f129", "m1"), ("f65", "decode"), ("f65", "m2"), ("f65", "psd")]


# ---------------------------------------------------------------------------------------------------------------------
# 1. long runs: the cost ring of VN_COST_CHUNK = 25 rows and its per-chunk reduction
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,variant", LONG_CASES)
def test_long_runs_cross_the_cost_chunks(shape, variant):
    """niter 1, 24, 25, 26 and 51 -- one, almost one, exactly one, one and a bit, two chunks and a bit of the cost ring
    (row it % 25, one reduction launch per chunk with its it0 offset).  Per niter three calls on one engine from the same
    start: launch by launch, captured, replayed (VAENMF_Q_EM_GRAPH 0, 1, 1); every call equals the step-by-step reference
    in EVERY iteration's cost of every utterance, in S_hat / N_hat and in the state it leaves.  Variants at F = 65: the
    decoding path (store=False), M2 labels, a fixed noise PSD."""
    need_gpu()
    base = _spec(shape, LONG_COUNTS[shape], m2=variant == "m2", labels=variant == "m2", noise=variant == "psd",
                 store=False if variant == "decode" else None)
    refs = _stepwise(base, NITERS)
    eng = _engine(shape, base.m2)
    for niter in NITERS:
        spec = _with(base, niter=niter)
        runs = [_fused(eng, spec) for _ in range(3)]
        assert [r.graph for r in runs] == [0, 1, 1], (niter, [r.graph for r in runs])
        for i, r in enumerate(runs):
            _check(r, refs[niter], "%s/%s niter %d call %d" % (shape, variant, niter, i + 1))
            assert (r.chain_kernel, r.w_fused) == (runs[0].chain_kernel, runs[0].w_fused)
        assert _query(eng, "Q_MSTEP_PATH") == (2 if variant == "decode" else 1)
        if variant == "m1":
            assert REACHED.setdefault(shape, (runs[0].chain_kernel, runs[0].w_fused)) == (runs[0].chain_kernel, runs[0].w_fused)
    eng.close()


def test_sweep_reaches_more_than_one_chain_kernel_and_w_statistics_form():
    """The three shapes between them run more than one chain kernel and more than one form of the W statistics
    (VAENMF_Q_CHAIN_KERNEL, VAENMF_Q_W_FUSED), so the driver is checked around each."""
    need_gpu()
    got = {s: _kernels(s) for s in SHAPES}
    print("chain kernel / W form per shape:", got)
    assert len({v[0] for v in got.values()}) > 1 and len({v[1] for v in got.values()}) > 1, got


# ---------------------------------------------------------------------------------------------------------------------
# 2. one value of the call changes on a plan that already holds a graph
# ---------------------------------------------------------------------------------------------------------------------
def test_signature_changes_on_a_plan_that_holds_a_graph():
    """One M2 engine at F = 65 with a graph for the base call; then one change at a time.  A changed call must not replay
    the base graph: its first appearance runs launch by launch, its second is captured, and both equal the changed
    call's OWN step-by-step reference.  After every change the base call replays its graph (VAENMF_Q_EM_GRAPH 1) and gives
    the base result bit for bit.  [30, 50] -> [50, 30] and [31, 49] keep NT, n_utt and every tile count: only the hash of
    the frame offsets tells them apart.  New spectrogram and seeds at the unchanged signature keep the graph, and the
    result follows the data."""
    need_gpu()
    base = _spec("f65", (30, 50), m2=True, labels=True)
    changes = [("niter 3->4", dict(niter=4)), ("nsE 4->3", dict(nsE=3)), ("biE 2->3", dict(biE=3)), ("nsWF 5->4", dict(nsWF=4)),
               ("biWF 3->2", dict(biWF=2)), ("var_rw 0.01->0.02", dict(var_rw=0.02)), ("counts [50, 30]", dict(counts=(50, 30))),
               ("counts [31, 49]", dict(counts=(31, 49))), ("counts [30]", dict(counts=(30,), seeds=(11,))),
               ("labels not set", dict(labels=False)), ("noise PSD set", dict(noise=True)), ("store off", dict(store=False))]
    ref0 = _stepwise(base)[base.niter]
    eng = _engine("f65", m2=True)
    runs = [_fused(eng, base) for _ in range(3)]
    assert [r.graph for r in runs] == [0, 1, 1]
    for r in runs:
        _check(r, ref0, "base")
    for tag, kw in changes:
        spec = _with(base, **kw)
        ref = _stepwise(spec)[spec.niter]
        a, b = _fused(eng, spec), _fused(eng, spec)
        _check(a, ref, tag + " (first call)")
        _check(b, ref, tag + " (second call)")
        assert (a.graph, b.graph) == (0, 1), (tag, a.graph, b.graph)      # a signature of its own: launch by launch, then captured
        assert not torch.equal(a.S[:30], ref0.S[:30]), tag          # the change does change the result
        back = _fused(eng, base)                                     # labels / PSD / store / counts back to the base call
        assert back.graph == 1, tag
        _check(back, ref0, "base after " + tag)
        assert _bit_equal(back, runs[0]), tag
    # the same signature, other contents: the graph stays, the result is the new batch's
    spec = _with(base, seeds=(101, 202), data=1)
    out = _fused(eng, spec)
    assert out.graph == 1
    _check(out, _stepwise(spec)[spec.niter], "new spectrogram and seeds")
    assert not torch.equal(out.S, ref0.S)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. more signatures than the cache keeps (MAX_GRAPHS = 4 graphs, MAX_SEEN = 8 signatures seen once)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_struct", [6, 10])
def test_more_signatures_than_the_cache_keeps(n_struct):
    """Frame structures of equal total size (96 frames in 3 utterances) round-robin on one engine, three rounds; every
    result equals its structure's step-by-step reference (computed once).  By the code: with six structures every
    signature is still remembered when it returns, so round 1 runs launch by launch and rounds 2 and 3 as graphs (an evicted
    graph is captured again); with ten, each signature has left the eight remembered ones before it returns, so no call
    ever runs as a graph."""
    need_gpu()
    specs = [_spec("f65", (20 + i, 33, 43 - i), niter=2) for i in range(n_struct)]
    refs = [_stepwise(s)[s.niter] for s in specs]
    eng = _engine("f65")
    paths = []
    for rnd in range(3):
        row = []
        for i, s in enumerate(specs):
            r = _fused(eng, s)
            _check(r, refs[i], "%d structures, round %d, structure %d" % (n_struct, rnd + 1, i))
            row.append(r.graph)
        paths.append(row)
    print("VAENMF_Q_EM_GRAPH per round, %d structures: %s" % (n_struct, paths))
    want = [[0] * 6, [1] * 6, [1] * 6] if n_struct == 6 else [[0] * 10] * 3
    assert paths == want, paths
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the seed ring of vaenmf_bind_batch_async
# ---------------------------------------------------------------------------------------------------------------------
def test_seed_ring_over_more_than_two_laps():
    """Twenty bind(seeds=...) + run on one engine with one frame structure and twenty seed lists -- more than two laps of
    the eight pinned slots -- with every input on the device and nothing read back until the end, so that the host runs
    ahead of the GPU as far as the driver lets it.  In the middle one bind of another structure (the table upload, which
    synchronises).  Each output equals a fresh engine's first call with those seeds."""
    need_gpu()
    F, K, _ = SHAPES["f65"]
    A, B = (33, 20, 41), (41, 53)                        # both 94 frames
    inp = _inputs("f65", A, 0)
    eng = _engine("f65")
    dev = eng.device
    Xc = np.zeros((sum(A), eng.Fs), np.complex64)
    Xc[:, :F] = np.concatenate(inp.Xs)
    X = torch.from_numpy(Xc.view(np.float32).reshape(sum(A), eng.Fs, 2)).to(dev)
    Z0 = inp.Z0.to(dev)

    def go(e, counts, seeds):
        e.bind(counts, Rcap=RCAP["f65"], seeds=seeds)
        e.set_spectrogram(X)                             # device to device
        e.init_nmf_device(salt=0x5A17)                   # keyed by the bound seeds, like the chains
        e.Z.copy_(Z0)
        return e.run(2, 4, 2, 5, 3, 0.01)                # clones on the device

    seed_lists = [[(0x9E3779B97F4A7C15 * (i + 1) + 0x1000 * u) % 2 ** 64 for u in range(3)] for i in range(20)]
    calls = []
    for i, sd in enumerate(seed_lists):
        if i == 10:
            calls.append((B, [77, 78], go(eng, B, [77, 78])))
        calls.append((A, sd, go(eng, A, sd)))
    graph_last = _query(eng, "Q_EM_GRAPH")
    torch.cuda.synchronize()
    assert graph_last == 1
    seen = []
    for counts, sd, (cost, S, N) in calls:
        fresh = _engine("f65")
        cost_r, S_r, N_r = go(fresh, counts, sd)
        assert torch.equal(cost, cost_r) and torch.equal(S, S_r) and torch.equal(N, N_r), (counts, sd)
        assert all(not torch.equal(S, s) for s in seen if s.shape == S.shape)       # twenty different results
        seen.append(S)
        fresh.close()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the profiling path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", [None, False])
def test_profiling_path_equals_the_unprofiled_call(store):
    """A plan with profiling on runs launch by launch with events around every launch: same results as the unprofiled
    call bit for bit, niter + 1 chains, one Wiener launch, M-step kinds in multiples of niter, positive finite times.  With
    fewer event pairs than one call has launches: no error, same results, at most that many records.  With profiling off
    again the earlier graph is replayed."""
    need_gpu()
    from vaenmf import _lib
    lib = _lib.lib()
    spec = _spec("f65", (37, 16, 50), niter=3, store=store)
    ref = _stepwise(spec)[spec.niter]
    eng = _engine("f65")
    plain = [_fused(eng, spec) for _ in range(3)]
    assert [r.graph for r in plain] == [0, 1, 1]
    for r in plain:
        _check(r, ref, "unprofiled")

    def read():
        ms, cn = np.full(5, -1.0), np.full(5, -1, np.int64)
        _lib.check(lib.vaenmf_profile_read(eng._plan, ms.ctypes.data, cn.ctypes.data))
        return ms, cn

    niter = spec.niter
    _lib.check(lib.vaenmf_profile_enable(eng._plan, 4 * niter + 8))
    out = _fused(eng, spec)
    assert out.graph == 0
    _check(out, ref, "profiled")
    assert _bit_equal(out, plain[0])
    ms, cn = read()
    print("profile: ms %s counts %s" % (ms.tolist(), cn.tolist()))
    assert cn[0] == niter + 1 and cn[4] == 1, cn
    assert all(c >= 0 and c % niter == 0 for c in cn[1:4]) and cn[3] == niter and cn[1:4].sum() <= 3 * niter, cn
    assert np.all(np.isfinite(ms)) and np.all(ms[cn > 0] > 0) and np.all(ms[cn == 0] == 0), (ms, cn)
    ms2, cn2 = read()                                    # read resets
    assert cn2.sum() == 0 and np.all(ms2 == 0)

    n_small = 3                                          # fewer pairs than the launches of one call
    assert n_small < cn.sum()
    _lib.check(lib.vaenmf_profile_enable(eng._plan, n_small))
    out = _fused(eng, spec)
    assert out.graph == 0 and _bit_equal(out, plain[0])
    ms, cn = read()
    assert 0 < cn.sum() <= n_small and np.all(np.isfinite(ms)) and np.all(ms[cn > 0] > 0), (ms, cn)

    _lib.check(lib.vaenmf_profile_enable(eng._plan, 0))
    out = _fused(eng, spec)
    assert out.graph == 1 and _bit_equal(out, plain[0])
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. vaenmf_init_nmf against its restatement on the host
# ---------------------------------------------------------------------------------------------------------------------
INIT_COUNTS = (1, 37, 16, 23)
INIT_SEEDS = (3, 2 ** 63 + 5, 2 ** 64 - 1, 12345678901234567)


@pytest.mark.parametrize("K", [1, 4, 8, 9, 16, 17, 32])
def test_init_nmf_equals_the_host_restatement(K):
    """W / H of vaenmf_init_nmf bit for bit equal to oracle.nmf_init_device (splitmix64 of seed ^ salt ^ tag ^ index, top
    24 bits, clamp at eps) over the ranks of all three Kp, F in {1, 65, 250, 257}, a ragged batch with a 1-frame
    utterance, 64-bit seeds and salt, eps 1e-8 and 0.3 (where the clamp is seen to act); the padding bins and ranks are
    zero, g is 1, nothing beyond the bound views is written, and a rebind with other seeds / the same seeds changes /
    restores the values."""
    need_gpu()
    from vaenmf.engine import BatchEngine
    counts, U, NT = INIT_COUNTS, len(INIT_COUNTS), sum(INIT_COUNTS)
    for F in (1, 65, 250, 257):
        params = orc.xavier_normal_params([F, 32, [128, 128]], seed=2)
        eng = BatchEngine(F, K, dec_list(params), precision="bf16", max_frames=NT + 19, max_utts=U + 2, z_dim=32)
        assert eng.Kp == (8 if K <= 8 else 16 if K <= 16 else 32) and eng.Fs == (F + 15) // 16 * 16

        def init(seeds, salt, eps):
            eng.bind(counts, Rcap=6, seeds=list(seeds))
            for whole in (eng._bW, eng._bHt, eng._bg):      # the kernel writes every element of the views, and no other
                whole.fill_(-7.0)
            eng.init_nmf_device(salt=salt, eps=eps)
            assert bool((eng._bW[U:] == -7).all()) and bool((eng._bHt[NT:] == -7).all()) and bool((eng._bg[NT:] == -7).all())
            return eng.W.cpu().numpy(), eng.Ht.cpu().numpy(), eng.g.cpu().numpy()

        for salt in (0, 0xC3A5C85C97CB3127):
            for eps in (1e-8, 0.3):
                W, Ht, g = init(INIT_SEEDS, salt, eps)
                assert np.all(W[:, F:, :] == 0) and np.all(W[:, :, K:] == 0) and np.all(Ht[:, K:] == 0) and np.all(g == 1)
                for u in range(U):
                    Wr, Hr = orc.nmf_init_device(INIT_SEEDS[u], salt, F, K, counts[u], eps)
                    assert np.array_equal(W[u, :F, :K], Wr), (F, K, salt, eps, u)
                    assert np.array_equal(Ht[eng.utt_slice(u), :K], Hr), (F, K, salt, eps, u)
                if eps == 0.3 and F * K >= 64:
                    assert 0.15 < np.mean(W[:, :F, :K] == np.float32(0.3)) < 0.45      # the clamp acts
                    assert W[:, :F, :K].min() == np.float32(0.3)
        W1, H1, _ = init(INIT_SEEDS, 9, 1e-8)
        W2, H2, _ = init(tuple(s ^ 0xF0 for s in INIT_SEEDS), 9, 1e-8)
        assert not np.array_equal(W1[:, :F, :K], W2[:, :F, :K]) and not np.array_equal(H1[:, :K], H2[:, :K])
        W3, H3, _ = init(INIT_SEEDS, 9, 1e-8)
        assert np.array_equal(W1, W3) and np.array_equal(H1, H3)
        eng.close()
