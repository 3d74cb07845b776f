"""The persistent kernels past a wavefront's first tile and frame.

wchain_kernel (chain.hip), decode_kernel (engine.hip) and the streaming kernels of stream.hip are persistent: a wavefront
or workgroup walks several wave tiles, tiles or frames in a loop and keeps state across the trips -- W of the current
utterance in LDS, the next frame's rows in flight, the per-wave layer-1 bias stash, the idle-lane marks of a partly filled
wave tile.  With the default grids a second trip needs thousands of frames (DESIGN.md section 4 has the thresholds), so
every other oracle comparison of the suite runs each loop once.  VAENMF_GRID_CAP=n caps those grids (and nothing else):
the small batches of tests/test_gpu_bin_counts.py then walk every loop several times, through an utterance boundary,
into a clipped last block and past wavefronts with nothing to do.  tests/test_persistent_loops_cpu.py restates the three
assignments and checks that the cases below reach all that; this module runs them against the oracle.

Tolerances are the ones tests/test_gpu_bin_counts.py and tests/test_gpu_rank_and_samples.py state for the same operation
(the helpers are shared with them: tests/em_support.py): a capped launch does the same arithmetic per frame.  Beyond the oracle comparison the capped
results are compared with the uncapped ones bit for bit wherever the value is computed per frame:
  * the chain: log-acceptances, Z, Zs and the store rows (a frame's chain reads nothing of another frame);
  * vaenmf_wiener_stored / vaenmf_wiener: S_hat, N_hat and the masks;
  * vaenmf_m_step_stored / vaenmf_m_step: the streaming (decoding) kernels write A1 and X2 * A2 per (frame, bin), the sums
    over an utterance's frames are taken by the W-update kernel, whose grid the cap does not touch -- so W, and with it H,
    g and the per-frame cost, are bit equal as well.  (noise_var_ / w_dot_ of stream.hip use one rank order and one
    rounding whether W is read from LDS or from global memory, so the rank > 8 path does not depend on which utterance
    the workgroup staged.)
The last two tests use no switch: batches sized from the device's CU count reach a second frame per wavefront of the
streaming kernels and a second round of wchain_kernel with the default grids.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import em_support as es
from dispatch_model import (COUNTS, chain_form, chain_grid, chain_rounds, chain_waves, decode_class, default_chain_counts,
                            default_stream_counts, shape_class, stream_class, stream_grid, wave_frames, wave_tiles)
from em_support import make_engine
from helpers import need_gpu, rel_err
from persistent_cases import (CHAIN_CASES, MAX_LEFT_OUT, STREAM_CAPS, STREAM_CASES, TILE_CAPS, TILE_CASES, chain_inputs, chain_reference,
                              replay_oracle)

gpu = pytest.mark.gpu

CAP = "VAENMF_GRID_CAP"
CHAIN_BURNIN = 4


def _cap_env(cap, **env):
    return es.env(**dict(env, **({CAP: str(cap)} if cap else {})))


def _equal(a, b, names, tag):
    for x, y, name in zip(a, b, names):
        x, y = (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in (x, y))
        assert x.shape == y.shape and np.array_equal(x, y), "%s: %s differs from the reference run (uncapped / alone / stepped) in %d of %d values" % (
            tag, name, int(np.sum(x != y)), x.size)


# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("F,precision,labels", CHAIN_CASES)
def test_chain_rounds_against_the_oracle(F, precision, labels):
    """wchain_kernel with one workgroup: 18 wave tiles in 3 rounds of 8 wavefronts (5 rounds of 4).  Replayed draws, store
    off: every log-acceptance, decision, sample and Z against the oracle (bf16x3: the bounds of
    test_split_mode_kernels_against_the_oracle; bf16: the first step's log-acceptances, as in
    test_bench_mode_kernels_against_the_oracle).  Device generator, store on: the store rows against the decoder of the
    chain's own samples.  Every array of both runs equals the uncapped launch's bit for bit."""
    need_gpu()
    c = chain_inputs(F, labels)
    n_wt = len(wave_tiles(c.counts))
    form, need_switch = chain_form(F, precision, n_wt)
    sc = shape_class(F, c.K, precision, n_wt, c.R, es.n_cus())
    assert sc["chain_kernel"] == (2 if need_switch else 1)
    env = {"VAENMF_WCHAIN4": "0"} if need_switch else {}
    NT, R, dev = c.NT, c.R, "cuda:0"

    def run(cap):
        with _cap_env(cap, **env):
            eng = es.engine(c, precision, seeds=list(range(3, 3 + len(c.counts))))
            assert es.query(eng, "Q_WTILES") == n_wt
            eng.Z.copy_(torch.from_numpy(c.Z0))
            acc = eng.mh_chain(c.ns, c.S_steps - c.ns, 0.01, eps=torch.from_numpy(c.eps).to(dev), u=torch.from_numpy(c.uu).to(dev),
                               want_acc=True).cpu().numpy()
            assert es.query(eng, "Q_CHAIN_KERNEL") == 1
            r = SimpleNamespace(eng=eng, acc=acc, Zs=eng.Zs[:, :c.ns].cpu().numpy().copy(), Z=eng.Z.cpu().numpy().copy())
            eng.Z.copy_(torch.from_numpy(c.Z0))
            eng.Zs.zero_()
            eng.sample_store(True)
            r.s_acc = eng.mh_chain(R, CHAIN_BURNIN, 0.01, call=0, want_acc=True).cpu().numpy()
            assert es.query(eng, "Q_CHAIN_KERNEL") == 1
            r.s_Zs, r.s_Z = eng.Zs[:, :R].cpu().numpy().copy(), eng.Z.cpu().numpy().copy()
            r.rows = eng.stored_variances(R).cpu().numpy()
            return r

    full, capped = run(0), run(1)
    names = ("acc", "Zs", "Z", "stored acc", "stored Zs", "stored Z", "store rows")
    arrays = lambda r: (r.acc, r.Zs, r.Z, r.s_acc, r.s_Zs, r.s_Z, r.rows)
    tag = "chain %s F=%d labels=%d" % (precision, F, labels)
    for a in arrays(capped):
        assert np.all(np.isfinite(a)), tag
    # 1. the oracle on the replayed draws
    refs, left_out = chain_reference(F, labels)
    print("%s (%s): frames left out %.1f %%" % (tag, form, 100 * left_out))
    assert left_out <= MAX_LEFT_OUT
    for u, ref in enumerate(refs):
        sl, keep = ref.sl, ref.keep
        if precision == "bf16x3":
            ea = float(np.max(np.abs(capped.acc[:, sl] - ref.acc)))
            dec = np.log(c.uu[:, sl]) < capped.acc[:, sl]
            ed = int(np.sum(dec[:, keep] != ref.is_acc[:, keep]))
            ez = float(np.max(np.abs(capped.Zs[sl][keep] - ref.Zs[keep]), initial=0.0))
            ezl = float(np.max(np.abs(capped.Z[sl][keep] - ref.Zs[keep, -1]), initial=0.0))
            print("%s utt %d: acc %.2e decisions %d Zs %.2e Z %.2e" % (tag, u, ea, ed, ez, ezl))
            assert ea < 3e-3 and ed == 0 and ez < 1e-5 and ezl < 1e-5, (tag, u, ea, ed, ez, ezl)
        else:       # (only the first step is comparable for every frame: afterwards a chain whose decision differs is in another state)
            e = float(np.max(np.abs(capped.acc[0, sl] - ref.acc[0])))
            print("%s utt %d: first-step acc %.3f" % (tag, u, e))
            assert e < 0.5, (tag, u, e)
    # 2. the store rows: the variances of the chain's own samples
    assert np.abs(capped.s_Zs - c.Z0[:, None, :]).max() > 0.05 and np.all(capped.rows[:, :, :F] > 0) and np.all(capped.rows[:, :, F:] == 0)
    if precision == "bf16x3":
        for u in range(len(c.counts)):
            sl = capped.eng.utt_slice(u)
            o = es.oracle_at(c, capped.eng, u)
            o.compute_Vs(capped.s_Zs[sl])
            e = rel_err(np.moveaxis(capped.rows[sl, :, :F], 0, -1), o.Vs)
            print("%s utt %d: store rows %.2e" % (tag, u, e))
            assert e < 2e-4, (tag, u, e)
    else:           # bf16 rows against vaenmf_decode of the same samples: the bounds of test_sample_store_holds_the_samples_variances
        eng = capped.eng
        B1 = eng.B1
        if labels and sc["chain_tiles"] <= 17:      # (eight wavefronts hold the label bias as bf16: tests/test_gpu_rank_and_samples.py)
            eng.B1 = B1.to(torch.bfloat16).to(torch.float32)
        D = eng.decode(R).cpu().numpy()
        eng.B1 = B1
        rel = np.abs(capped.rows[:, :, :F] - D[:, :, :F]) / D[:, :, :F]
        e = (float(np.max(rel[:, :, :sc["Fm"]])), float(np.max(rel[:, :, sc["Fm"]:], initial=0.0)))
        print("%s: store rows against decode %.2e, extra bin %.2e" % (tag, e[0], e[1]))
        assert e[0] < 4e-3 and e[1] < 5e-2, (tag, e)
    # 3. per-frame values: the capped launch changes none of them
    _equal(arrays(capped), arrays(full), names, tag)


# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("F,K,R,variant,precision,switches", STREAM_CASES)
def test_streaming_kernels_walk_several_frames(F, K, R, variant, precision, switches):
    """vaenmf_wiener_stored and vaenmf_m_step_stored with 1, 2 and 4 workgroups (blocks of 18, 9 and 5 frames per
    wavefront) against the float64 formulas fed the device's own stored rows, to the bounds of
    tests/test_gpu_rank_and_samples.py; every output equals the uncapped launch's bit for bit (module docstring)."""
    need_gpu()
    c = es.case_inputs(F, K, R, variant)
    forms = stream_class(F, K, R, precision, variant, 6, es.n_cus(), wfused=switches.get("VAENMF_WFUSED") != "0")
    eng, Vb = es.prepare(c, variant, precision, R)
    eng.sample_store(True)
    es.reset(c, eng)
    eng.mh_chain(R, 3, 0.01, call=0)
    V = eng.stored_variances(R).cpu().numpy()
    assert np.all(np.isfinite(V)) and np.all(V[:, :, :F] > 0)
    refs = [es.reference(o, variant) for o in es.oracles_from(c, eng, variant, Vb, V[:, :, :F])]
    pre = [t.clone() for t in (eng.W, eng.Ht, eng.g)]
    failures = []

    def run(cap):
        tag = "streaming %s F=%d K=%d R=%d %s cap=%d" % (precision, F, K, R, variant, cap)
        with _cap_env(cap, **switches):
            for t, p in zip((eng.W, eng.Ht, eng.g), pre):
                t.copy_(p)
            out = eng.wiener_stored(want_masks=True)
            es.compare(tag + " wiener", refs, lambda u: es.device_wiener(c, eng, u, out), failures)
            es.padding_is_zero(eng, out[2], out[3], out[0].abs().sum(-1), out[1].abs().sum(-1))
            eng.m_step_stored()
            if variant != "noNMF":          # the two-kernel path: wstats_stream / wstats_stream2, not the fused or the group kernel
                assert es.query(eng, "Q_W_FUSED") == 0 and forms["wstats"]["kernel"] in ("wstats_stream", "wstats_stream2"), tag
        cost = eng.cost_from_frames(R)
        es.compare(tag + " m-step", refs, lambda u: es.device_m_step(c, eng, u, cost, variant), failures)
        es.padding_is_zero(eng)
        return [t.clone() for t in out] + [t.clone() for t in (eng.W, eng.Ht, eng.g, eng.cost_frames)]

    names = ("S_hat", "N_hat", "WFs", "WFn", "W", "Ht", "g", "cost_frames")
    full = run(0)
    for cap in STREAM_CAPS:
        _equal(run(cap), full, names, "streaming %s F=%d K=%d R=%d %s cap=%d" % (precision, F, K, R, variant, cap))
    eng.sample_store(False)
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("F,K,R,precision", TILE_CASES)
def test_tile_loop_walks_several_tiles(F, K, R, precision):
    """vaenmf_decode, vaenmf_wiener and vaenmf_m_step with one and two workgroups: 3 tiles of up to 64 frames (two teams) or
    4 of up to 32, W of rank <= 8 restaged in LDS behind the barrier.  Given samples; the bounds of
    test_decoding_kernels_against_the_oracle_from_the_decoded_variances; every output equals the uncapped launch's bit
    for bit."""
    need_gpu()
    c = es.case_inputs(F, K, R, "M1")
    dc = decode_class(F, K, R, precision)
    eng, _ = es.prepare(c, "M1", precision, R)
    assert es.query(eng, "Q_TILES") == sum((n + (63 if dc["geom"] in (0, 3) else 31)) // (64 if dc["geom"] in (0, 3) else 32) for n in COUNTS)
    eng.Zs.copy_(torch.from_numpy(c.Zs))
    pre = [t.clone() for t in (eng.W, eng.Ht, eng.g)]
    failures, refs = [], []

    def run(cap):
        tag = "tile loop %s F=%d K=%d R=%d cap=%d" % (precision, F, K, R, cap)
        with _cap_env(cap):
            for t, p in zip((eng.W, eng.Ht, eng.g), pre):
                t.copy_(p)
            V = eng.decode(R)
            Vn = V.cpu().numpy()
            assert np.all(np.isfinite(Vn)) and np.all(Vn[:, :, F:] == 0)
            if not refs:                    # (once: the capped runs must reproduce these variances bit for bit, checked below)
                oracles = es.oracles_from(c, eng, "M1", None, Vn[:, :, :F])
                for u, o in enumerate(oracles):
                    mine = o.Vs
                    o.compute_Vs(c.Zs[eng.utt_slice(u)])
                    e = rel_err(mine, o.Vs)
                    print("%s utt %d: decode %.2e" % (tag, u, e))
                    assert e < (2e-4 if precision == "bf16x3" else 5e-2), (tag, u, e)
                    o.Vs = mine
                refs.extend(es.reference(o, "M1") for o in oracles)
            out = eng.wiener(R, want_masks=True)
            es.compare(tag + " wiener", refs, lambda u: es.device_wiener(c, eng, u, out), failures)
            es.padding_is_zero(eng, out[2], out[3], out[0].abs().sum(-1), out[1].abs().sum(-1))
            eng.m_step(R)
        cost = eng.cost_from_frames(R)
        es.compare(tag + " m-step", refs, lambda u: es.device_m_step(c, eng, u, cost, "M1"), failures)
        es.padding_is_zero(eng)
        return [V] + [t.clone() for t in out] + [t.clone() for t in (eng.W, eng.Ht, eng.g, eng.cost_frames)]

    names = ("decode", "S_hat", "N_hat", "WFs", "WFn", "W", "Ht", "g", "cost_frames")
    full = run(0)
    for cap in TILE_CAPS:
        _equal(run(cap), full, names, "tile loop %s F=%d K=%d R=%d cap=%d" % (precision, F, K, R, cap))
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_em_run_graph_is_keyed_on_the_grid_cap():
    """vaenmf_em_run on one live plan: uncapped three times (launch by launch, captured, replayed: VAENMF_Q_EM_GRAPH 0, 1, 1),
    then with VAENMF_GRID_CAP=1 -- the captured grids differ, so the call must not replay the uncapped graph: 0, 1, 1 again --
    and uncapped once more, which replays the first graph.  Every capped run gives the results of the capped run stepped
    through mh_chain / m_step_stored / wiener_stored."""
    need_gpu()
    c = es.inputs(65, 10, 10)
    niter, nsE, biE, nsW, biW = 2, 8, 3, 10, 4
    seeds = [5, 6, 7]

    def load(eng):
        eng.init_nmf(c.W0, c.H0)
        eng.g.copy_(torch.from_numpy(c.gains))
        eng.Z.copy_(torch.from_numpy(c.Z0))

    def fused(eng):
        load(eng)
        cost, S, N = eng.run(niter, nsE, biE, nsW, biW, 0.01)
        assert es.query(eng, "Q_MSTEP_PATH") == 1
        return SimpleNamespace(cost=cost.cpu().numpy(), out=[S, N, eng.W.clone(), eng.Ht.clone(), eng.g.clone(), eng.Z.clone()],
                               graph=es.query(eng, "Q_EM_GRAPH"))

    eng = es.engine(c, "bf16", seeds=seeds)
    plain = [fused(eng) for _ in range(3)]
    with _cap_env(1):
        capped = [fused(eng) for _ in range(3)]
        ref = es.engine(c, "bf16", seeds=seeds)
        load(ref)
        ref.sample_store(True)
        cost = np.zeros((len(COUNTS), niter))
        for it in range(niter):
            ref.mh_chain(nsE, biE, 0.01, call=it)
            ref.m_step_stored()
            cost[:, it] = ref.cost_from_frames(nsE)
        state = [t.clone() for t in (ref.W, ref.Ht, ref.g, ref.Z)]
        ref.mh_chain(nsW, biW, 0.01, call=niter, update_Z=False)
        S, N, _, _ = ref.wiener_stored()
    again = fused(eng)
    assert [r.graph for r in plain] == [0, 1, 1] and [r.graph for r in capped] == [0, 1, 1] and again.graph == 1
    names = ("S_hat", "N_hat", "W", "Ht", "g", "Z")
    for i, r in enumerate(capped):
        _equal(r.out, [S, N] + state, names, "capped em_run, call %d" % (i + 1))
        assert np.max(np.abs(r.cost - cost) / np.abs(cost)) < 1e-12
    for r in plain[1:] + [again]:
        _equal(r.out, plain[0].out, names, "uncapped em_run")
        assert np.array_equal(r.cost, plain[0].cost)


@gpu
def test_default_streaming_launch_reaches_a_second_frame():
    """F = 65, K = 4, R = 10, bf16: the stored M-step, its cost and the stored Wiener filter of a batch of 16 n_cus + 41 frames
    against the oracle per utterance (the bounds of test_bench_mode_kernels_against_the_oracle), with the default W-statistics
    kernel and on the two-kernel path (wstats_stream2: 2 n_cus workgroups, three frames per wavefront)."""
    need_gpu()
    n = es.n_cus()
    counts = default_stream_counts(n)
    NT, F, K, R = sum(counts), 65, 4, 10
    per, blocks = wave_frames(NT, stream_grid(NT, n))
    per2, _ = wave_frames(NT, stream_grid(NT, n, pipelined=True))
    assert per >= 2 and per2 >= 2 and any(0 < e - b < per for b, e in blocks) and any(b >= e for b, e in blocks)
    c = es.inputs(F, K, R, counts=counts)
    for switches in ({}, {"VAENMF_WFUSED": "0"}):
        eng = es.engine(c, "bf16", seeds=list(range(3, 3 + len(counts))))
        eng.Z.copy_(torch.from_numpy(c.Z0))
        eng.sample_store(True)
        eng.mh_chain(R, 4, 0.01, call=0)
        Zs = eng.Zs[:, :R].cpu().numpy().copy()
        oracles = [es.oracle_at(c, eng, u, Zs) for u in range(len(counts))]
        with es.env(**switches):
            eng.m_step_stored()
            assert (es.query(eng, "Q_W_FUSED") == 0) == bool(switches)
        tag = "default grid, %s" % ("two kernels" if switches else "fused W statistics")
        es.m_step_against(c, eng, oracles, R, eng.cost_from_frames(R), 3e-2, 3e-3, tag)
        es.wiener_against(c, eng, oracles, eng.wiener_stored(want_masks=True), 1e-2, tag, absolute=True)
        eng.close()


@gpu
def test_default_chain_launch_reaches_a_second_round():
    """F = 65, bf16: more than 8 n_cus wave tiles from utterances of 1..16 frames.  Sixteen utterances whose tiles fall in
    the first and in the second (last) round of a wavefront, each run alone with its seed: Z, Zs and the store rows are
    bit equal (the batch independence of the device generator's chains).  Two more against the oracle on replayed draws."""
    need_gpu()
    n = es.n_cus()
    counts = default_chain_counts(n)
    U, F, K, R, bi = len(counts), 65, 8, 4, 2
    c = es.inputs(F, K, R, counts=counts)
    seeds = [100 + u for u in range(U)]
    eng = es.engine(c, "bf16", seeds=seeds)
    assert es.query(eng, "Q_WTILES") == U > 8 * n
    where, rounds = chain_rounds(U, chain_grid(U, n), chain_waves("bf16", 5))
    assert rounds >= 2
    round_of = {wt: i for tiles in where.values() for i, wt in enumerate(tiles)}
    last = [u for u in range(U) if round_of[u] == rounds - 1]
    first = [u for u in range(U) if round_of[u] == 0]
    picks = [first[0], first[3], first[n - 1], first[n], first[len(first) // 2], first[-16], first[-2], first[-1],
             last[0], last[1], last[2], last[9], last[len(last) // 2], last[-3], last[-2], last[-1]]
    assert {counts[u] for u in picks} >= {1, 16} and len(set(picks)) == 16
    eng.Z.copy_(torch.from_numpy(c.Z0))
    eng.sample_store(True)
    eng.mh_chain(R, bi, 0.01, call=0)
    assert es.query(eng, "Q_CHAIN_KERNEL") == 1
    Z, Zs, rows = eng.Z.clone(), eng.Zs[:, :R].clone(), eng.stored_variances(R)
    assert bool(torch.isfinite(rows).all()) and float((Zs - eng.Z.new_tensor(c.Z0)[:, None, :]).abs().max()) > 0.05
    one = make_engine(c.params, F, K, [16], Rcap=R, precision="bf16")       # one engine, bound again per utterance
    for u in picks:
        sl = eng.utt_slice(u)
        one.bind([counts[u]], Rcap=R, seeds=[seeds[u]])
        one.set_spectrogram([c.Xs[u]])
        one.init_nmf([c.W0[u]], [c.H0[u]])
        one.g.copy_(torch.from_numpy(c.gains[sl]))
        one.Z.copy_(torch.from_numpy(c.Z0[sl]))
        one.sample_store(True)
        one.mh_chain(R, bi, 0.01, call=0)
        assert es.query(one, "Q_CHAIN_KERNEL") == 1
        _equal((one.Z, one.Zs[:, :R], one.stored_variances(R)), (Z[sl], Zs[sl], rows[sl]), ("Z", "Zs", "store rows"),
               "utterance %d (round %d) alone" % (u, round_of[u]))
    one.close()
    # two utterances against the oracle on replayed draws (bf16: the first step's log-acceptances, 0.5)
    eng.sample_store(False)
    eng.init_nmf(c.W0, c.H0)
    eng.g.copy_(torch.from_numpy(c.gains))
    eng.Z.copy_(torch.from_numpy(c.Z0))
    acc = eng.mh_chain(c.ns, c.S_steps - c.ns, 0.01, eps=torch.from_numpy(c.eps).to(eng.device), u=torch.from_numpy(c.uu).to(eng.device),
                       want_acc=True).cpu().numpy()
    assert np.all(np.isfinite(acc))
    for u in (first[len(first) // 3], last[len(last) // 3]):
        ref = replay_oracle(c, u)
        e = float(np.max(np.abs(acc[0, ref.sl] - ref.acc[0])))
        print("default grid, utterance %d (round %d, %d frames): first-step acc %.3f" % (u, round_of[u], counts[u], e))
        assert e < 0.5
    eng.close()
