"""Which bytes the EM entry points touch.

The other GPU tests check values.  These run every EM entry point on buffers of exactly the size include/vaenmf.h states,
16-byte aligned and no better, carved from one poisoned allocation (tests/guarded.py), with poison -- a NaN, then 1e30 --
in every padding the header calls `ignored`, and beside it on a twin: an ordinary engine with the same inputs and seeds,
zero padding and the allocator's alignment, the path the rest of the suite holds to the oracle and to float64.  After
EVERY library call:
  (a) every guard round every buffer is intact, bit for bit;
  (b) every buffer the call does not write (the `const` ones, Z under update_Z = 0, Zs when NULL was passed, and all the
      rest of the arena) holds the bits it held before;
  (c) every buffer it writes is bit-equal to the twin's over its documented extent (bins < F, ranks < K, latent columns
      < L, samples < nsamples, rows < NT);
  (d) its padding is what the header says: written as zero, left alone (still poison), or unspecified but inside;
  (e) VAENMF_Q_CHAIN_KERNEL / Q_W_FUSED / Q_MSTEP_PATH report the kernels tests/test_guarded_cpu.py predicts for the case.
No tolerance: poison, alignment and exact extents must change nothing.  A read by an idle lane of a row it shadows cannot
be seen here -- a read whose value reaches no output leaves no trace; reads are caught through changed results only.

CONTRACT and BUFFERS (tests/contract_cases.py, shared with tests/stream_cases.py) are written from include/vaenmf.h, not from
the kernels."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from contract_cases import (BUFFERS, BURNIN, BY_NAME, CASES, CONTRACT, DECODE_CASES, DECODE_SAMPLES, NS, RCAP, VAR_RW, case_class, inputs,
                            is_wide)
from em_support import make_engine, query
from guarded import POISON, Arena, GuardError, bits, make_guarded_engine, power_spec, same_bits
from helpers import need_gpu

pytestmark = pytest.mark.gpu

class Pair:
    """A guarded engine and its twin, and the buffers of both by their names in CONTRACT."""

    def __init__(self, case, poison, Rcap=RCAP, arena_mb=64):
        self.case, self.inp = case, inputs(case)
        p = self.inp
        self.arena = Arena(arena_mb << 20, poison, "cuda")
        self.g = make_guarded_engine(self.arena, p["params"], case.F, case.K, case.counts, Rcap, case.precision, p["seeds"])
        self.t = make_engine(p["params"], case.F, case.K, case.counts, Rcap, case.precision, p["seeds"])
        self.engines = (self.g, self.t)
        assert self.g.wide == self.t.wide == is_wide(case)
        self.sc = case_class(case, torch.cuda.get_device_properties(0).multi_processor_count)
        assert self.g.Fs == self.sc["Fs"] and self.g.Kp == self.sc["Kp"] and self.g.NT == p["NT"]
        self.d = SimpleNamespace(F=case.F, K=case.K, L=self.g.L, ns=NS)
        self.cur, self.problems = {}, []
        for n in ("X", "X2", "W", "Ht", "g", "Z", "Zs", "cost_frames"):
            self.reg(n, getattr(self.g, n), getattr(self.t, n))
        for n in self.arena.order:                   # exact buffers: the engine's views are the whole allocations
            assert self.arena.bufs[n]["rows"] in (p["NT"], len(case.counts)), n
        self.arena.check("bind")

    def reg(self, name, gt, tt):
        self.cur[name] = (self.arena.name_of(gt), gt, tt)

    def give(self, name, host, pad_from=None):
        """A host array to both engines: carved exactly for the guarded one (columns pad_from.. of its rows poisoned), a
        plain device tensor for the twin."""
        gt = self.g.carve_like(name, host)
        if pad_from is not None and pad_from < host.shape[-1]:
            self.arena.poison(gt[..., pad_from:])
        self.reg(name, gt, torch.from_numpy(np.ascontiguousarray(host)).cuda())

    def step(self, entry, call, skip=(), ns=None):
        """One library call on both engines, then (a)-(d).  call(engine, side) -> {name: output tensor} for buffers the call
        allocated; skip: buffers of CONTRACT[entry].writes this call does not write (NULL, update_Z = 0, gains only)."""
        a, d = self.arena, self.d
        d.ns = NS if ns is None else ns
        assert all(r in self.cur or r in ("B1", "Vb", "eps", "u", "y") for r in CONTRACT[entry].reads), entry
        writes = [w for w in CONTRACT[entry].writes if w not in skip]
        written = {self.cur[w][0] for w in writes if w in self.cur}
        a.snapshot([n for n in a.order if n not in written])
        outs = [call(eng, side) for side, eng in enumerate(self.engines)]
        outs = [o if isinstance(o, dict) else {} for o in outs]
        torch.cuda.synchronize()
        for k in outs[0]:
            self.reg(k, outs[0][k], outs[1][k])

        def expect(ok, *msg):
            if not ok:
                self.problems.append("%s: %s" % (entry, " ".join(str(m) for m in msg)))

        for chk in (a.check, a.unchanged):                                  # (a), (b)
            try:
                chk(what=entry)
            except GuardError as e:
                self.problems.append(str(e))
        for w in writes:
            _, gt, tt = self.cur[w]
            extent, zero, left = BUFFERS[w]
            same = same_bits(extent(gt, d), extent(tt, d))                  # (c)
            expect(same, w, "differs from the twin's over its extent", "" if same else "(%d of %d words, %d NaN)" % (
                int((bits(extent(gt, d)) != bits(extent(tt, d))).sum()), extent(gt, d).numel(), int(torch.isnan(extent(gt, d)).sum())))
            expect(bool(torch.isfinite(extent(tt, d)).all()), w, "of the twin is not finite")
            for f in zero:                                                  # (d)
                expect(int(torch.count_nonzero(f(gt, d))) == 0, "padding of", w, "is not zero")
            for f in left:
                expect(a.is_poison(f(gt, d)), "rows of", w, "past the samples were touched")

    # every problem of a sequence is reported, not the first alone (later ones may follow from it: the engines have parted)
    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        if self.problems:
            raise AssertionError("%d contract violations (%s):\n  " % (len(self.problems), self.case.name) + "\n  ".join(self.problems[:16]))
        return False

    def side(self, name, side):
        return self.cur[name][1 + side]


def _prepare(P):
    """Calls 1-3 of the sequence, then the state no entry point sets: start latents, gains, the fixed noise PSD."""
    case, p, a = P.case, P.inp, P.arena
    P.g.load_spectrogram(p["Xs"])
    P.t.set_spectrogram(p["Xs"])
    a.poison(P.g.X2)                                 # an output: starts as poison
    P.step("vaenmf_power_spec", lambda eng, s: power_spec(eng))
    if P.g.Fs > case.F:                              # X2's padding is |X's|^2 (0, or inf under 1e30); as an INPUT it is ignored: poison
        assert not bool(torch.isnan(P.g.X2[:, case.F:]).any())
        a.poison(P.g.X2[:, case.F:])
    if case.Dy:
        P.give("y", p["y"])
        P.step("vaenmf_layer1_bias", lambda eng, s: (eng.set_labels(P.side("y", s)), {"B1": eng.B1})[1])
    a.poison(P.g.W)                                  # vaenmf_init_nmf writes its padding as zero
    a.poison(P.g.Ht)
    a.poison(P.g.g)
    P.step("vaenmf_init_nmf", lambda eng, s: eng.init_nmf_device(salt=5))
    for s, eng in enumerate(P.engines):
        eng.Z.zero_()
        eng.Z[:, :eng.L].copy_(torch.from_numpy(p["Z0"]))
        eng.g.copy_(torch.from_numpy(p["gains"]))
    if case.noise_psd:
        Vb = np.zeros((p["NT"], P.g.Fs), np.float32)
        Vb[:, :case.F] = p["Vb"]
        P.give("Vb", Vb, pad_from=case.F)
        for s, eng in enumerate(P.engines):
            eng.set_noise_psd(P.side("Vb", s))
            assert eng._Vb_ext is P.side("Vb", s)
    a.check("setup")


def _chain_checks(P):
    for eng in P.engines:
        assert query(eng, "Q_CHAIN_KERNEL") == P.sc["chain_kernel"]        # (e)


def _m_step_skip(P):
    return ("W", "Ht") if P.case.noise_psd else ()


@pytest.mark.parametrize("poison", sorted(POISON))
@pytest.mark.parametrize("name", [c.name for c in CASES if not c.large])
def test_call_sequence_on_exact_buffers(name, poison):
    need_gpu()
    case = BY_NAME[name]
    with Pair(case, poison) as P:
        _sequence(P)


def _sequence(P):
    from vaenmf import _lib
    case, a, g, S = P.case, P.arena, P.g, NS + BURNIN
    _prepare(P)
    # 4. the draws of chain invocation 0; the replay reads columns < L of them only
    P.step("vaenmf_rng_fill", lambda eng, s: dict(zip(("eps", "u"), eng.rng_fill(0, S))))
    if g.Lp > g.L:
        # Columns L..Lp-1 of the replay draws.  A wide plan never loads them and the team kernel masks them: poison.  The wave
        # chains of a narrow plan with L = 16 multiply them by a zero step: the header asks for FINITE
        # values there -- as vaenmf_rng_fill's own are, asserted here -- so under the NaN word they hold 1e30 instead.
        pad = P.side("eps", 0)[:, :, g.L:]
        assert bool(torch.isfinite(pad).all()) and bool(torch.isfinite(P.side("eps", 1)[:, :, g.L:]).all())
        if g.wide or P.sc["chain_kernel"] == 0:      # (f273_z16: every chain of the sequence is the team kernel's)
            a.poison(pad)
        else:
            pad.fill_(1e30)
            assert int(bits(pad)[0, 0, 0]) == POISON["1e30"]
    # 5. replayed chain, acceptances out, store on
    for eng in P.engines:
        eng.sample_store(True)
    P.step("vaenmf_mh_chain", lambda eng, s: {"acc": eng.mh_chain(NS, BURNIN, VAR_RW, eps=P.side("eps", s), u=P.side("u", s), want_acc=True)})
    _chain_checks(P)
    assert float((P.side("Zs", 0)[:, :NS, :g.L] - P.side("Z", 0)[:, None, :g.L]).abs().max()) > 0      # (the chain moved)
    # 6. - 8. the stored entries
    P.step("vaenmf_sample_store_gather", lambda eng, s: {"Vs_store": eng.stored_variances(NS)})
    P.step("vaenmf_m_step_stored", lambda eng, s: eng.m_step_stored(), skip=_m_step_skip(P))
    if not case.noise_psd:
        for eng in P.engines:
            assert query(eng, "Q_W_FUSED") == P.sc["w_fused"]
    P.step("vaenmf_wiener_stored", lambda eng, s: dict(zip(("S_hat", "N_hat", "WFs", "WFn"), eng.wiener_stored(want_masks=True))))
    # 9. the Wiener phase's chain: device draws, Z only read, the samples not recorded where the kernel allows it
    no_zs = g.wide or (P.sc["chain_kernel"] != 0 and
                       _lib.lib().vaenmf_wchain_addressable(g.NT, RCAP, S, g.Fs, g.Kp, g.U, 0) == 1)

    def wf_chain(eng, s):
        zs = eng.Zs
        if no_zs:
            eng.Zs = None
        try:
            eng.mh_chain(NS, BURNIN, VAR_RW, call=1, update_Z=False)
        finally:
            eng.Zs = zs
    P.step("vaenmf_mh_chain", wf_chain, skip=("Z", "acc") + (("Zs",) if no_zs else ()))
    _chain_checks(P)
    if not g.wide:
        # 10. the decoding entries from the samples in Zs
        P.step("vaenmf_decode", lambda eng, s: {"Vs": eng.decode(NS)})
        P.step("vaenmf_m_step", lambda eng, s: eng.m_step(NS), skip=_m_step_skip(P))
        P.step("vaenmf_wiener", lambda eng, s: dict(zip(("S_hat", "N_hat", "WFs", "WFn"), eng.wiener(NS, want_masks=True))))
    # 11. the fused driver, three times on one signature: launch by launch, captured, replayed
    P.reg("S_hat", g._bS, P.t._bS)
    P.reg("N_hat", g._bN, P.t._bN)
    for i, graph in enumerate((0, 1, 1)):
        def run(eng, s):
            eng.run(2, NS, BURNIN, NS, BURNIN, VAR_RW)
            return {"cost": eng._bcu[2]} if i == 0 else None
        P.step("vaenmf_em_run", run, skip=_m_step_skip(P))
        _chain_checks(P)
        for eng in P.engines:
            assert query(eng, "Q_EM_GRAPH") == graph and query(eng, "Q_MSTEP_PATH") == 1
            assert case.noise_psd or query(eng, "Q_W_FUSED") == P.sc["w_fused"]
    assert bool(torch.isfinite(g._bS[:, :case.F]).all()) and float(g._bS.abs().max()) > 0


@pytest.mark.parametrize("poison", sorted(POISON))
@pytest.mark.parametrize("R,Rcap", [rc for rc in DECODE_SAMPLES if rc != (NS, RCAP)])
@pytest.mark.parametrize("name", DECODE_CASES)
def test_decoding_entries_at_other_sample_counts(name, R, Rcap, poison):
    """vaenmf_decode / vaenmf_m_step / vaenmf_wiener from given samples with R = 1 and with R = 33 of Rcap = 40 (a second
    32-sample chunk with one real sample: r is clamped to R - 1); sample rows R..Rcap-1 are poison and stay so."""
    need_gpu()
    case = BY_NAME[name]
    with Pair(case, poison, Rcap=Rcap) as P:
        _prepare(P)
        for eng in P.engines:
            eng.Zs[:, :R].zero_()
            eng.Zs[:, :R, :eng.L].copy_(torch.from_numpy(P.inp["Zs%d" % R]))
        assert P.arena.is_poison(P.g.Zs[:, R:]) and int(torch.count_nonzero(P.t.Zs[:, R:])) == 0
        P.step("vaenmf_decode", lambda eng, s: {"Vs": eng.decode(R)}, ns=R)
        P.step("vaenmf_wiener", lambda eng, s: dict(zip(("S_hat", "N_hat", "WFs", "WFn"), eng.wiener(R, want_masks=True))), ns=R)
        P.step("vaenmf_m_step", lambda eng, s: eng.m_step(R), ns=R)
        assert P.arena.is_poison(P.g.Zs[:, R:])


@pytest.mark.parametrize("poison", sorted(POISON))
def test_large_batch_chain_and_stored_m_step(poison):
    """259 wave tiles, more than the device has compute units: the one-wavefront bf16 chain at 17 bin tiles and the
    64-frame-tile W statistics (w_fused = 1).  One chain call and the stored M-step only."""
    need_gpu()
    with Pair(BY_NAME["f257_large"], poison, arena_mb=128) as P:
        _prepare(P)
        for eng in P.engines:
            eng.sample_store(True)
        P.step("vaenmf_mh_chain", lambda eng, s: {"acc": eng.mh_chain(NS, BURNIN, VAR_RW, call=0, want_acc=True)})
        _chain_checks(P)
        P.step("vaenmf_m_step_stored", lambda eng, s: eng.m_step_stored())
        for eng in P.engines:
            assert query(eng, "Q_W_FUSED") == P.sc["w_fused"]


@pytest.mark.parametrize("poison", sorted(POISON))
@pytest.mark.parametrize("wlen_sec", [4e-3, 25e-3])
def test_producers_write_zero_padding(wlen_sec, poison):
    """X's padding is `must be zero` (the Wiener filters write mask x X there, with mask = 0).  The library's own producer,
    vaenmf_stft_batch_ex (n_fft 64: radix 2; 400: mixed radix), writes exact zeros into a pre-poisoned X of exactly
    [NT][Fs] and stays inside it, and vaenmf_power_spec of that X gives X2 a zero padding."""
    need_gpu()
    from vaenmf import stft as vstft
    from vaenmf._lib import check, lib
    from vaenmf.engine import _ptr, _stream
    arena = Arena(16 << 20, poison, "cuda")
    lens = [1000, 700, 450]
    wav = torch.from_numpy(np.random.default_rng(3).standard_normal(sum(lens)).astype(np.float32)).cuda()
    X, fc = vstft.stft_batch(wav, lens, 16000, wlen_sec, 0.25, out=lambda shape, dtype: arena.carve("X", shape, dtype))
    torch.cuda.synchronize()
    F = int(round(16000 * wlen_sec)) // 2 + 1
    assert arena.order == ["X"] and X.shape == (sum(fc), (F + 15) // 16 * 16, 2) and X.shape[1] > F
    arena.check("vaenmf_stft_batch_ex")
    assert int(torch.count_nonzero(X[:, F:])) == 0 and bool(torch.isfinite(X[:, :F]).all()) and float(X[:, :F].abs().max()) > 0
    X2 = arena.carve("X2", X.shape[:2], torch.float32)
    arena.snapshot(["X"])
    check(lib().vaenmf_power_spec(_ptr(X), _ptr(X2), X.shape[0] * X.shape[1], _stream()))
    torch.cuda.synchronize()
    arena.check("vaenmf_power_spec")
    arena.unchanged(what="vaenmf_power_spec")
    assert int(torch.count_nonzero(X2[:, F:])) == 0 and bool(torch.isfinite(X2).all()) and float(X2[:, :F].max()) > 0
