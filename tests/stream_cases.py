"""The case table of tests/test_gpu_streams.py (and of tests/test_stream_cases_cpu.py, which holds it to include/vaenmf.h
without a GPU): one entry per device entry point of the C ABI, or per natural sequence of them, that takes a `void* stream`.

A Case holds
  entries      the C functions its call() makes (every prototype with a stream parameter is in some case or in EXCLUDED);
  make(seed)   -> Spec: host arrays of every float input (`inputs`), of every device-side table or map (`maps`: offsets,
               row maps, idx -- what a kernel turns into an address or a loop bound; they are never poisoned), the shapes of
               the outputs, of scratch, and whatever host tables and scalars the call passes (`host`; contents A and B of a
               case share them).  `prefill` names integer outputs a later kernel of the same sequence reads as a loop bound
               (STOI's keep / counts): the runner starts them from the reference's values instead of poison;
  open(spec)   -> state: plans, trainers, device tables already uploaded -- everything that may allocate, block or wait;
  call(b, stream, step) -> return codes: the C-ABI calls alone, through vaenmf._lib.lib(), no torch call, no allocation;
  load(b, spec, stream)    contents that do not travel as a plain copy (the utterance seeds, through vaenmf_bind_batch_async);
  before(state)            puts host state back that a run changes (the bound frame structure);
  outs         Out(name, extent, zero, left): the documented extent (None: the whole buffer), padding written as zero,
               padding left alone;
  steps        ((label, pending), ...): a case runs its call once per step; pending says whether the step must return while
               its stream is still busy;
  syncs        the header says the call synchronises its stream;
  capture      None when the calls may be captured into a caller's graph, else the reason they may not.

Nothing here needs a GPU to be imported; make() of some cases asks the library's host-only geometry functions."""
import ctypes as C
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

import contract_cases as cc
from contract_cases import BUFFERS, BURNIN, NS, RCAP, VAR_RW

EXCLUDED = {
    "vaenmf_hbm_read_probe": "its output is a measured rate",
    "vaenmf_wave_sum_probe": "a one-launch test aid that tests/test_gpu_wave_sums.py owns",
}
# the header's own words for every call that waits (tests/test_stream_cases_cpu.py finds them in include/vaenmf.h)
SYNCHRONISES = {
    "vaenmf_lorenz_labels": "Synchronises the stream",
    "vaenmf_bind_batch_async": "A batch with\n * another frame structure synchronises `stream`",
}
# every chain_kernel / w_fused value contract_cases.case_class gives over contract_cases.CASES; w_fused = 1 (the 64-frame-tile W
# statistics) exists past one wave tile per compute unit only: f257_large
EM_SUBSET = ["f9", "f257", "f250_m2", "f257_x3_noise_psd", "f640", "wide_z128_h256", "f257_large"]
EM_RUN = ["f257", "wide_z128_h256"]
SEEDS = (1, 2)                  # contents A and B

Out = namedtuple("Out", "name extent zero left", defaults=(None, (), ()))
Case = namedtuple("Case", "name entries make call outs open load before steps syncs capture",
                  defaults=(None, None, None, (("call", True),), False, None))
CASES = []


def Spec(**kw):
    s = SimpleNamespace(inputs={}, maps={}, outputs={}, scratch={}, prefill=(), host=SimpleNamespace(), d=SimpleNamespace())
    s.__dict__.update(kw)
    return s


def _add(*a, **kw):
    CASES.append(Case(*a, **kw))


def by_name():
    return {c.name: c for c in CASES}


def L():
    from vaenmf import _lib
    return _lib.lib()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def H(a):
    """Address of a host array (kept alive by the Spec that owns it)."""
    return None if a is None else C.c_void_p(a.ctypes.data)


def _cols(w):
    return lambda t, d: t[:, :w]


def _past(w):
    return lambda t, d: t[:, w:]


def _off(counts, dtype):
    return np.concatenate([[0], np.cumsum(counts)]).astype(dtype)


f32, f64, i32, i64 = np.float32, np.float64, np.int32, np.int64


# =====================================================================================================================
# EM, step by step: the stored sequence, the decoding sequence, the fused driver, the rebinds
def _em_dims(k):
    wide = cc.is_wide(k)
    NT, U, F = sum(k.counts), len(k.counts), k.F
    return SimpleNamespace(F=F, K=k.K, L=k.z_dim, ns=NS, NT=NT, U=U, Fs=(F + 15) // 16 * 16, Kp=8 if k.K <= 8 else 16 if k.K <= 16 else 32,
                           Lp=128 if wide else 32, H1=k.h_dim[-1], S=NS + BURNIN, Dy=k.Dy, counts=list(k.counts))


def _em_common(k, seed, d):
    """Spectrogram (padding zero), |X|^2, start latents (padding zero), labels, noise PSD, seeds: contract_cases' recipe."""
    g = np.random.default_rng(4000 + k.F + k.z_dim + 7919 * seed)
    X = np.zeros((d.NT, d.Fs), np.complex64)
    X[:, :d.F] = ((g.standard_normal((d.NT, d.F)) + 1j * g.standard_normal((d.NT, d.F))) * (0.5 + 3 * np.exp(-np.arange(d.F) / 60.0))).astype(np.complex64)
    Z = np.zeros((d.NT, d.Lp), f32)
    Z[:, :d.L] = 0.5 * g.standard_normal((d.NT, d.L))
    a = dict(X=np.ascontiguousarray(X.view(f32).reshape(d.NT, d.Fs, 2)), Z=Z)
    if k.Dy:
        a["y"] = (g.random((d.NT, k.Dy)) > 0.5).astype(f32)
    if k.noise_psd:
        a["Vb"] = (g.random((d.NT, d.Fs)) + 0.1).astype(f32)
    return g, a, np.array([11 + u + 100 * seed for u in range(d.U)], np.uint64)


def _nmf_state(g, d):
    W = np.zeros((d.U, d.Fs, d.Kp), f32)
    W[:, :d.F, :d.K] = np.maximum(g.random((d.U, d.F, d.K)), 1e-8)
    Ht = np.zeros((d.NT, d.Kp), f32)
    Ht[:, :d.K] = np.maximum(g.random((d.NT, d.K)), 1e-8)
    return dict(W=W, Ht=Ht, g=(0.5 + g.random(d.NT)).astype(f32))


def _em_open(k, store, counts=None):
    def open_(spec):
        import torch
        from em_support import make_engine
        p = cc.inputs(k)
        eng = make_engine(p["params"], k.F, k.K, counts or k.counts, RCAP, k.precision, p["seeds"])
        d = spec.d
        assert (eng.Fs, eng.Kp, eng.Lp, eng.H1, eng.NT) == (d.Fs, d.Kp, d.Lp, d.H1, d.NT), "the engine's strides are not the case's"
        if store or eng.wide:
            eng.sample_store(True)
        st = SimpleNamespace(eng=eng, plan=eng._plan, fixed={})
        if k.noise_psd:          # the plan keeps the pointer: one buffer for every run of the case
            st.fixed["Vb"] = torch.empty(d.NT, d.Fs, device="cuda")
            assert L().vaenmf_set_noise_psd(st.plan, P(st.fixed["Vb"])) == 0
        torch.cuda.synchronize()
        return st
    return open_


def _rebind(b, spec, stream):
    """The utterance seeds of these contents, stream-ordered (the frame structure is the bound one: no wait)."""
    h = spec.host
    return [L().vaenmf_bind_batch_async(b.state.plan, len(h.off) - 1, H(h.off), H(h.seeds), stream)]


def _rng(mode, call, eps=None, u=None):
    from vaenmf import _lib
    return _lib.Rng(_lib.RNG_DEVICE if mode == "device" else _lib.RNG_REPLAY, call, P(eps), P(u))


def _em_outs(names, d):
    return [Out(n, *BUFFERS[n]) for n in names]


def _stored(k):
    d = _em_dims(k)

    def make(seed):
        g, a, seeds = _em_common(k, seed, d)
        o = dict(X2=((d.NT, d.Fs), f32), W=((d.U, d.Fs, d.Kp), f32), Ht=((d.NT, d.Kp), f32), g=((d.NT,), f32), eps=((d.S, d.NT, d.Lp), f32),
                 u=((d.S, d.NT), f32), Zs=((d.NT, RCAP, d.Lp), f32), acc=((d.S, d.NT), f32), cost_frames=((d.NT,), f64),
                 S_hat=((d.NT, d.Fs, 2), f32), N_hat=((d.NT, d.Fs, 2), f32), WFs=((d.NT, d.Fs), f32), WFn=((d.NT, d.Fs), f32),
                 Vs_store=((d.NT, NS, d.Fs), f32))
        if k.Dy:
            o["B1"] = ((d.NT, d.H1), f32)
        return Spec(inputs=a, outputs=o, host=SimpleNamespace(off=_off(d.counts, i32), seeds=seeds), d=d)

    def call(b, st, step):
        l, p = L(), b.state.plan
        B1 = P(b.B1) if k.Dy else None
        r = [l.vaenmf_power_spec(P(b.X), P(b.X2), d.NT * d.Fs, st)]
        if k.Dy:
            r.append(l.vaenmf_layer1_bias(p, P(b.y), k.Dy, B1, st))
        r.append(l.vaenmf_init_nmf(p, P(b.W), P(b.Ht), P(b.g), 5, 1e-8, st))
        r.append(l.vaenmf_rng_fill(p, 0, d.S, P(b.eps), P(b.u), st))
        rng = _rng("device", 0)
        r.append(l.vaenmf_mh_chain(p, P(b.X2), P(b.W), P(b.Ht), P(b.g), P(b.Z), 1, B1, P(b.Zs), RCAP, NS, BURNIN, VAR_RW, C.byref(rng), P(b.acc), st))
        r.append(l.vaenmf_m_step_stored(p, P(b.X2), P(b.W), P(b.Ht), P(b.g), P(b.cost_frames), st))
        rng = _rng("device", 1)
        r.append(l.vaenmf_mh_chain(p, P(b.X2), P(b.W), P(b.Ht), P(b.g), P(b.Z), 0, B1, P(b.Zs), RCAP, NS, BURNIN, VAR_RW, C.byref(rng), None, st))
        r.append(l.vaenmf_wiener_stored(p, P(b.W), P(b.Ht), P(b.g), P(b.X), P(b.S_hat), P(b.N_hat), P(b.WFs), P(b.WFn), st))
        r.append(l.vaenmf_sample_store_gather(p, P(b.Vs_store), st))
        return r

    names = ["X2", "W", "Ht", "g", "eps", "u", "Z", "Zs", "acc", "cost_frames", "S_hat", "N_hat", "WFs", "WFn", "Vs_store"] + (["B1"] if k.Dy else [])
    entries = ("vaenmf_power_spec", "vaenmf_init_nmf", "vaenmf_rng_fill", "vaenmf_mh_chain", "vaenmf_m_step_stored", "vaenmf_wiener_stored",
               "vaenmf_sample_store_gather") + (("vaenmf_layer1_bias",) if k.Dy else ())
    _add("em_stored_" + k.name, entries, make, call, _em_outs(names, d), open=_em_open(k, True), load=_rebind)


def _given_state(k, seed, d, draws):
    """Inputs of the entries that start from a given NMF state: |X|^2 computed here, W / Ht / g, and the replay draws."""
    g, a, seeds = _em_common(k, seed, d)
    a["X2"] = (a["X"][..., 0] ** 2 + a["X"][..., 1] ** 2).astype(f32)
    a.update(_nmf_state(g, d))
    a.pop("y", None)
    if k.Dy:
        a["B1"] = (0.1 * g.standard_normal((d.NT, d.H1))).astype(f32)
    if draws:
        a["eps"] = np.zeros((d.S, d.NT, d.Lp), f32)
        a["eps"][..., :d.L] = g.standard_normal((d.S, d.NT, d.L))
        a["u"] = np.clip(g.random((d.S, d.NT)), 1e-6, 1.0).astype(f32)
    return a, seeds


def _decoding(k):
    d = _em_dims(k)

    def make(seed):
        a, seeds = _given_state(k, seed, d, True)
        o = dict(Zs=((d.NT, RCAP, d.Lp), f32), acc=((d.S, d.NT), f32), Vs=((d.NT, NS, d.Fs), f32), cost_frames=((d.NT,), f64),
                 S_hat=((d.NT, d.Fs, 2), f32), N_hat=((d.NT, d.Fs, 2), f32), WFs=((d.NT, d.Fs), f32), WFn=((d.NT, d.Fs), f32))
        return Spec(inputs=a, outputs=o, host=SimpleNamespace(off=_off(d.counts, i32), seeds=seeds), d=d)

    def call(b, st, step):
        l, p = L(), b.state.plan
        B1 = P(b.B1) if k.Dy else None
        rng = _rng("replay", 0, b.eps, b.u)
        return [l.vaenmf_mh_chain(p, P(b.X2), P(b.W), P(b.Ht), P(b.g), P(b.Z), 1, B1, P(b.Zs), RCAP, NS, BURNIN, VAR_RW, C.byref(rng), P(b.acc), st),
                l.vaenmf_decode(p, P(b.Zs), RCAP, NS, B1, P(b.Vs), st),
                l.vaenmf_m_step(p, P(b.X2), P(b.W), P(b.Ht), P(b.g), P(b.Zs), RCAP, NS, B1, P(b.cost_frames), st),
                l.vaenmf_wiener(p, P(b.X2), P(b.W), P(b.Ht), P(b.g), P(b.Zs), RCAP, NS, B1, P(b.X), P(b.S_hat), P(b.N_hat), P(b.WFs), P(b.WFn), st)]

    names = ["Z", "Zs", "acc", "Vs", "W", "Ht", "g", "cost_frames", "S_hat", "N_hat", "WFs", "WFn"]
    _add("em_decoding_" + k.name, ("vaenmf_mh_chain", "vaenmf_decode", "vaenmf_m_step", "vaenmf_wiener"), make, call, _em_outs(names, d),
         open=_em_open(k, False), load=_rebind)


NITER = 2
EM_RUN_STEPS = (("eager", True), ("capturing", False), ("replayed", True))      # VAENMF_Q_EM_GRAPH 0, 1, 1


def _em_run(k):
    d = _em_dims(k)

    def make(seed):
        a, seeds = _given_state(k, seed, d, False)
        o = dict(Zs=((d.NT, RCAP, d.Lp), f32), S_hat=((d.NT, d.Fs, 2), f32), N_hat=((d.NT, d.Fs, 2), f32), cost=((d.U, NITER), f64))
        return Spec(inputs=a, outputs=o, host=SimpleNamespace(off=_off(d.counts, i32), seeds=seeds), d=d)

    def call(b, st, step):
        l, p = L(), b.state.plan
        return [l.vaenmf_em_run(p, P(b.X2), P(b.W), P(b.Ht), P(b.g), P(b.Z), None, P(b.Zs), RCAP, NITER, NS, BURNIN, NS, BURNIN, VAR_RW,
                                P(b.X), P(b.S_hat), P(b.N_hat), P(b.cost), st)]

    _add("em_run_" + k.name, ("vaenmf_em_run",), make, call, _em_outs(["W", "Ht", "g", "Z", "Zs", "S_hat", "N_hat", "cost"], d),
         open=_em_open(k, True), load=_rebind, steps=EM_RUN_STEPS,
         capture="vaenmf_em_run owns a graph cache and captures on a stream of its own")


OTHER_COUNTS = [20, 3, 30]        # another frame structure of the same 53 frames


def _bind(k, new):
    d = _em_dims(k)
    if new:
        d.counts, d.U = list(OTHER_COUNTS), len(OTHER_COUNTS)
        assert sum(OTHER_COUNTS) == d.NT

    def make(seed):
        a, seeds = _given_state(k, seed, d, False)
        a.pop("X")
        o = dict(Zs=((d.NT, RCAP, d.Lp), f32), acc=((d.S, d.NT), f32))
        return Spec(inputs=a, outputs=o, host=SimpleNamespace(off=_off(d.counts, i32), seeds=seeds + np.uint64(1000)), d=d)

    def call(b, st, step):
        l, p, h = L(), b.state.plan, b.spec.host
        rng = _rng("device", 0)
        return [l.vaenmf_bind_batch_async(p, d.U, H(h.off), H(h.seeds), st),
                l.vaenmf_mh_chain(p, P(b.X2), P(b.W), P(b.Ht), P(b.g), P(b.Z), 1, None, P(b.Zs), RCAP, NS, BURNIN, VAR_RW, C.byref(rng), P(b.acc), st)]

    def before(state):
        """The plan as open() left it: the case's own frame structure and seeds, every table on the device."""
        off, seeds = _off(k.counts, i32), np.array(cc.inputs(k)["seeds"], np.uint64)
        assert L().vaenmf_bind_batch(state.plan, len(k.counts), H(off), H(seeds)) == 0

    _add("bind_%s_%s" % ("new_structure" if new else "same_structure", k.name), ("vaenmf_bind_batch_async", "vaenmf_mh_chain"), make, call,
         _em_outs(["Z", "Zs", "acc"], d), open=_em_open(k, False), before=before, syncs=new,
         capture="vaenmf_bind_batch_async records an event of its own on the stream and waits on it eight binds later")


for _n in EM_SUBSET:
    _stored(cc.BY_NAME[_n])
for _n in EM_SUBSET:
    if not cc.is_wide(cc.BY_NAME[_n]):
        _decoding(cc.BY_NAME[_n])
for _n in EM_RUN:
    _em_run(cc.BY_NAME[_n])
_bind(cc.BY_NAME["f257"], False)
_bind(cc.BY_NAME["f257"], True)


# =====================================================================================================================
# STFT / iSTFT, resampler, segments
STFT_LENS = [1000, 700, 450]


def _stft(nfft):
    fs = 16000
    F, Fs = nfft // 2 + 1, (nfft // 2 + 1 + 15) // 16 * 16

    def make(seed):
        from vaenmf import stft as vstft
        geo = [vstft.frame_geometry(t, fs, nfft / fs, 0.25, True) for t in STFT_LENS]
        assert geo[0][0] == nfft
        fc = [g[2] for g in geo]
        NT = sum(fc)
        g = np.random.default_rng(300 + nfft + seed)
        maps = dict(soff=_off(STFT_LENS, i64), foff=_off(fc, i32), futt=np.repeat(np.arange(len(fc)), fc).astype(i32), plen=np.array([g_[3] for g_ in geo], i32))
        return Spec(inputs=dict(wav=g.standard_normal(sum(STFT_LENS)).astype(f32)), maps=maps,
                    outputs=dict(X=((NT, Fs, 2), f32), wav_out=((sum(STFT_LENS),), f32)), scratch=dict(work=((NT, nfft), f32)),
                    host=SimpleNamespace(hop=geo[0][1], NT=NT), d=SimpleNamespace(F=F))

    def call(b, st, step):
        from vaenmf import _lib
        h = b.spec.host
        opts = _lib.StftOpts(nfft, h.hop, 1, _lib.PAD_REFLECT, None)
        return [L().vaenmf_stft_batch_ex(P(b.wav), h.NT, P(b.soff), P(b.foff), P(b.futt), P(b.plen), C.byref(opts), Fs, P(b.X), st),
                L().vaenmf_istft_batch_ex(P(b.X), len(STFT_LENS), h.NT, P(b.soff), P(b.foff), C.byref(opts), Fs, P(b.work), P(b.wav_out), st)]

    _add("stft_%d" % nfft, ("vaenmf_stft_batch_ex", "vaenmf_istft_batch_ex"), make, call,
         [Out("X", None, (lambda t, d: t[:, F:],)), Out("wav_out")])


for _n in (64, 400, 22):          # radix 2, mixed radix, Bluestein (2 x 11)
    _stft(_n)

RESAMPLE_RATIOS = [(2, 3), (160, 441), (1, 1)]
RESAMPLE_LENGTHS = [1, 7, 441, 1001, 0]


def _resample():
    from resample_cases import out_length

    def make(seed):
        g = np.random.default_rng(500 + seed)
        h = SimpleNamespace(ioff=_off(RESAMPLE_LENGTHS, i64), ooff=[_off([out_length(n, u, dn) for n in RESAMPLE_LENGTHS], i64) for u, dn in RESAMPLE_RATIOS])
        return Spec(inputs=dict(x=g.standard_normal(sum(RESAMPLE_LENGTHS)).astype(f32)),
                    outputs={"y%d" % i: ((int(o[-1]),), f32) for i, o in enumerate(h.ooff)}, host=h)

    def call(b, st, step):
        h = b.spec.host
        return [L().vaenmf_resample_batch(P(b.x), len(RESAMPLE_LENGTHS), H(h.ioff), H(h.ooff[i]), u, dn, 10, 5.0, P(getattr(b, "y%d" % i)), st)
                for i, (u, dn) in enumerate(RESAMPLE_RATIOS)]

    _add("resample", ("vaenmf_resample_batch",), make, call, [Out("y%d" % i) for i in range(len(RESAMPLE_RATIOS))])


_resample()


def _segments():
    ROWS, N = 6, 5

    def make(seed):
        g = np.random.default_rng(600 + seed)
        a, m, o = {}, {}, {}
        for rf in (7, 8):             # float accesses, 16-byte accesses
            a["src%d" % rf] = g.standard_normal((ROWS, rf)).astype(f32)
            a["wb%d" % rf] = g.random(N).astype(f32)
            m["map%d" % rf] = np.array([[3, 0, 3, 5, 1], [2, 2, 4, 0, 5]][seed % 2], i32)                  # repeats
            m["ra%d" % rf] = np.array([[0, 1, 2, 3, 4], [5, 3, 1, 0, 2]][seed % 2], i32)
            m["rb%d" % rf] = np.array([[1, -1, 5, 0, 2], [-1, 4, 0, 2, 3]][seed % 2], i32)                # one frame with a single owner
            o["gat%d" % rf], o["ble%d" % rf] = ((N, rf), f32), ((N, rf), f32)
        return Spec(inputs=a, maps=m, outputs=o)

    def call(b, st, step):
        r = []
        for rf in (7, 8):
            v = lambda n: P(getattr(b, "%s%d" % (n, rf)))
            r.append(L().vaenmf_gather_rows(v("src"), v("map"), N, rf, v("gat"), st))
            r.append(L().vaenmf_blend_rows(v("src"), v("ra"), v("rb"), v("wb"), N, rf, v("ble"), st))
        return r

    _add("segments", ("vaenmf_gather_rows", "vaenmf_blend_rows"), make, call, [Out("%s%d" % (n, rf)) for rf in (7, 8) for n in ("gat", "ble")])


_segments()


# =====================================================================================================================
# front-ends and metrics: the ragged shapes of tests/test_gpu_front_ends.py
FE = SimpleNamespace(F=129, Fs=136, ld=140, counts=[33, 9], NT=42)


def _padded_X(seed, counts=FE.counts):
    import vaenmf_oracle as orc
    X = np.zeros((sum(counts), FE.Fs), np.complex64)
    o = 0
    for n in counts:
        X[o:o + n, :FE.F] = orc.heavy_tailed_stft(FE.F, n, 42 + n + 1000 * seed).T
        o += n
    return np.ascontiguousarray(X.view(f32).reshape(-1, FE.Fs, 2))


def _labels():
    from vaenmf import _lib
    U = len(FE.counts)

    def make(seed):
        nb = [int(L().vaenmf_lorenz_work_bytes(FE.NT, FE.F, U, m)) for m in (_lib.LABEL_IBM, _lib.LABEL_VAD)]
        # (generator 2 gives a nine-frame utterance with no Lorenz value below the fraction in VAD mode, the reference's IndexError)
        return Spec(inputs=dict(X=_padded_X({1: 1, 2: 3}[seed])),
                    outputs=dict(ibm=((FE.NT, FE.ld), f32), thr_ibm=((U,), f32), vad=((FE.NT,), f32), thr_vad=((U,), f32)),
                    scratch=dict(work=(((max(nb) + 7) // 8,), i64)), host=SimpleNamespace(off=_off(FE.counts, i32), nb=nb))

    def call(b, st, step):
        h = b.spec.host
        return [L().vaenmf_lorenz_labels(P(b.X), U, H(h.off), FE.F, FE.Fs, m, 0.98, 0.0, 1.0, P(out), ld, P(thr), P(b.work), h.nb[m], st)
                for m, out, ld, thr in ((_lib.LABEL_IBM, b.ibm, FE.ld, b.thr_ibm), (_lib.LABEL_VAD, b.vad, FE.F, b.thr_vad))]

    _add("lorenz_labels", ("vaenmf_lorenz_labels",), make, call,
         [Out("ibm", _cols(FE.F), (), (_past(FE.F),)), Out("thr_ibm"), Out("vad"), Out("thr_vad")], syncs=True,
         capture="vaenmf_lorenz_labels synchronises the stream")


_labels()


def _spp():
    ld = FE.F + 3

    def make(seed):
        g = np.random.default_rng(700 + seed)
        per = ((g.standard_normal((FE.NT, ld)) ** 2 + g.standard_normal((FE.NT, ld)) ** 2) * np.exp(1.2 * g.standard_normal((FE.NT, 1)))).astype(f32)
        n = FE.NT * FE.F
        return Spec(inputs=dict(per=per, per1=np.ascontiguousarray(per[:, :FE.F]).reshape(-1), spp1=g.random(n).astype(f32)),
                    maps=dict(off=_off(FE.counts, i32)),
                    outputs=dict(spp=((FE.NT, FE.F), f32), psd=((FE.NT, FE.F), f32), psd1=((n,), f32)))

    def call(b, st, step):
        return [L().vaenmf_spp_estimate(P(b.per), ld, len(FE.counts), P(b.off), FE.F, 0.8, 0.9, 0.5, 15.0, 10, P(b.spp), P(b.psd), FE.F, st),
                L().vaenmf_spp_noise_given(P(b.per1), P(b.spp1), FE.NT * FE.F, 0.8, P(b.psd1), st)]

    _add("spp", ("vaenmf_spp_estimate", "vaenmf_spp_noise_given"), make, call, [Out("spp"), Out("psd"), Out("psd1")])


_spp()


def _masks():
    ldm = FE.F + 2

    def make(seed):
        g = np.random.default_rng(800 + seed)
        return Spec(inputs=dict(S=_padded_X(seed), N=_padded_X(seed + 50), X=_padded_X(seed + 100), m=g.random((FE.NT, ldm)).astype(f32)),
                    outputs=dict(mask=((FE.NT, FE.Fs), f32), S_hat=((FE.NT, FE.Fs, 2), f32)))

    def call(b, st, step):
        return [L().vaenmf_wiener_mask(P(b.S), P(b.N), FE.NT * FE.Fs, 1e-8, P(b.mask), st),
                L().vaenmf_apply_mask(P(b.X), P(b.m), ldm, FE.NT, FE.F, FE.Fs, P(b.S_hat), st)]

    _add("masks", ("vaenmf_wiener_mask", "vaenmf_apply_mask"), make, call, [Out("mask"), Out("S_hat", _cols(FE.F), (_past(FE.F),))])


_masks()


def _dense():
    M, inn, out, ldx, ldy = 65, 17, 5, 20, 8

    def make(seed):
        g = np.random.default_rng(900 + seed)
        return Spec(inputs=dict(x=g.standard_normal((M, ldx)).astype(f32), w=(g.standard_normal((out, inn)) / np.sqrt(inn)).astype(f32),
                                b=(0.3 * g.standard_normal(out)).astype(f32)), outputs=dict(y=((M, ldy), f32)))

    def call(b, st, step):
        from vaenmf import _lib
        return [L().vaenmf_dense(P(b.x), M, inn, ldx, P(b.w), P(b.b), out, _lib.ACT_TANH, P(b.y), ldy, st)]

    _add("dense", ("vaenmf_dense",), make, call, [Out("y", _cols(out), (), (_past(out),))])


_dense()
GRAM_COUNTS = [1, 255, 256, 257, 4000]


def _gram3():
    def make(seed):
        g = np.random.default_rng(12 + 1000 * seed)
        n = sum(GRAM_COUNTS)
        return Spec(inputs=dict(sh=g.standard_normal(n).astype(f32), s=g.standard_normal(n).astype(f32), n=(0.5 * g.standard_normal(n)).astype(f32)),
                    maps=dict(soff=_off(GRAM_COUNTS, i64)), outputs=dict(G=((len(GRAM_COUNTS), 6), f64)))

    def call(b, st, step):
        return [L().vaenmf_gram3_batch(P(b.sh), P(b.s), P(b.n), len(GRAM_COUNTS), P(b.soff), P(b.G), st)]

    _add("gram3", ("vaenmf_gram3_batch",), make, call, [Out("G")])


_gram3()
STOI_UTTS = ["T257", "k30", "k31", "gap_mid", "zeros"]


def _stoi(extended):
    def make(seed):
        import stoi_cases as sc
        batch = {n: (x, y) for n, x, y in sc.boundary_batch(20241 + 17 * (seed - 1))}
        xs, ys = [batch[n][0] for n in STOI_UTTS], [batch[n][1] for n in STOI_UTTS]
        counts = [len(x) for x in xs]
        geo = [sc.geometry(T) for T in counts]
        U, NF, NSP = len(xs), sum(g_[0] for g_ in geo), sum(g_[1] for g_ in geo)
        off = _off(counts, i64)
        nb = int(L().vaenmf_stoi_work_bytes(U, H(off)))
        assert nb > 0
        # rows >= M of tob_x / tob_y are neither read nor written: compared whole, they must still hold the poison they started with
        return Spec(inputs=dict(clean=np.concatenate(xs).astype(f32), proc=np.concatenate(ys).astype(f32)),
                    outputs=dict(keep=((NF,), i32), counts=((U, 3), i32), tob_x=((NSP, 16), f64), tob_y=((NSP, 16), f64), d_seg=((U,), f64),
                                 d=((U,), f64), counts_b=((U, 3), i32)), prefill=("keep", "counts", "counts_b"),
                    scratch=dict(work=(((nb + 7) // 8,), i64)), host=SimpleNamespace(off=off, nb=nb, U=U))

    def call(b, st, step):
        h = b.spec.host
        return [L().vaenmf_stoi_tob(P(b.clean), P(b.proc), h.U, H(h.off), P(b.keep), P(b.counts), P(b.tob_x), P(b.tob_y), P(b.work), h.nb, st),
                L().vaenmf_stoi_segments(P(b.tob_x), P(b.tob_y), P(b.counts), h.U, H(h.off), extended, P(b.d_seg), P(b.work), h.nb, st),
                L().vaenmf_stoi_batch(P(b.clean), P(b.proc), h.U, H(h.off), extended, P(b.d), P(b.counts_b), P(b.work), h.nb, st)]

    _add("stoi" if not extended else "estoi", ("vaenmf_stoi_tob", "vaenmf_stoi_segments", "vaenmf_stoi_batch"), make, call,
         [Out(n) for n in ("keep", "counts", "tob_x", "tob_y", "d_seg", "d", "counts_b")])


_stoi(0)
_stoi(1)


# =====================================================================================================================
# data sets
MIX_T, MIX_CUTS, MIX_NOISE, MIX_STARTS, MIX_SNR = [100, 4097, 9000], [0, 7, 0], 10000, [0, 100, 1000], [-5.0, 0.0, 2.5]


def _mix():
    U = len(MIX_T)

    def make(seed):
        g = np.random.default_rng(1100 + seed)
        n_in = sum(t + c for t, c in zip(MIX_T, MIX_CUTS))
        h = SimpleNamespace(ioff=_off([t + c for t, c in zip(MIX_T, MIX_CUTS)], i64), ooff=_off(MIX_T, i64), cuts=np.array(MIX_CUTS, i64),
                            starts=np.array(MIX_STARTS, i64), factors=np.array([10.0 ** (-v / 10.0) for v in MIX_SNR], f64), nb=552 * U)
        o = {}
        for j in (0, 1):
            o.update({"s%d" % j: ((sum(MIX_T),), f32), "n%d" % j: ((sum(MIX_T),), f32), "x%d" % j: ((sum(MIX_T),), f32), "stats%d" % j: ((U, 5), f64)})
        return Spec(inputs=dict(speech=(g.standard_normal(n_in) * np.exp(g.standard_normal(n_in)) * 0.1).astype(f32),
                                noise=(0.3 * g.standard_normal(MIX_NOISE)).astype(f32)), outputs=o, scratch=dict(work=((h.nb // 8,), i64)), host=h)

    def call(b, st, step):
        h = b.spec.host
        assert L().vaenmf_mix_work_bytes(U) == h.nb
        v = lambda n, j: P(getattr(b, "%s%d" % (n, j)))
        return [L().vaenmf_mix_batch(P(b.speech), U, H(h.ioff), H(h.cuts), P(b.noise), MIX_NOISE, H(h.starts), H(h.factors), j, H(h.ooff),
                                     v("s", j), v("n", j), v("x", j), v("stats", j), P(b.work), h.nb, st) for j in (0, 1)]

    _add("mix_batch", ("vaenmf_mix_batch",), make, call, [Out("%s%d" % (n, j)) for j in (0, 1) for n in ("s", "n", "x", "stats")])


_mix()


def _moments():
    NF, F, ld = 65, 9, 12

    def make(seed):
        g = np.random.default_rng(1200 + seed)
        nb = int(L().vaenmf_moments_work_bytes(NF, F))
        return Spec(inputs=dict(P=np.clip(np.exp(g.standard_normal((NF, ld)) * 6.0 - 9.0), 1e-12, 1e4).astype(f32)),
                    outputs=dict(S1=((F,), f64), S2=((F,), f64)), scratch=dict(work=(((max(nb, 8) + 7) // 8,), i64)), host=SimpleNamespace(nb=nb))

    def call(b, st, step):
        return [L().vaenmf_feature_moments(P(b.P), NF, F, ld, acc, P(b.S1), P(b.S2), P(b.work), b.spec.host.nb, st) for acc in (0, 1)]

    _add("feature_moments", ("vaenmf_feature_moments",), make, call, [Out("S1"), Out("S2")])


_moments()


# =====================================================================================================================
# training: the eleven kernels, then whole steps
def _train_kernels():
    B, n_in, n_out, z, D, NT, NA = 33, 19, 21, 8, 5, 40, 37
    ldx, ldw, ldy, ldz, ldp, lda, ldm, ldl, ldg = n_in + 3, n_in + 1, n_out + 5, n_out + 1, n_in + 2, n_in + 4, 2 * z + 3, z + 2, n_in + 5

    def make(seed):
        g = np.random.default_rng(1300 + seed)
        r = lambda *s: g.standard_normal(s).astype(f32)
        a = dict(X=r(B, ldx), W=(r(n_out, ldw) / np.sqrt(n_in)).astype(f32), b=(0.3 * r(n_out)).astype(f32), dZ=r(B, ldz), Yp=np.tanh(r(B, ldp)),
                 Xe=g.exponential(1.0, (B, ldx)).astype(f32), A=(0.5 * r(B, lda)).astype(f32), ML=(0.5 * r(B, ldm)).astype(f32), eps=r(B, z),
                 dZl=r(B, ldl), A2=r(B, lda), Yl=(g.random((B, lda)) < 0.4).astype(f32), src=r(NT, ldg), mean=r(n_in), std=(0.5 + g.random(n_in)).astype(f32),
                 p=r(NA), g=r(NA), m=(0.1 * r(NA)).astype(f32), v=(0.01 * g.random(NA)).astype(f32))
        o = dict(Y=((B, ldy), f32), dX=((B, ldx), f32), dW=((n_out, ldw), f32), db=((n_out,), f32), dA=((B, lda), f32), row_recon=((B,), f64),
                 Zl=((B, ldl), f32), dML=((B, ldm), f32), row_kl=((B,), f64), dA2=((B, lda), f32), row_loss=((B,), f64), row_cnt=((B, 4), i32),
                 red=((8,), f64), gat=((B, ldg), f32), eps_out=((B, z), f32))
        return Spec(inputs=a, maps=dict(idx=g.integers(0, NT, B).astype(i32)), outputs=o)

    def call(b, st, step):
        from vaenmf import _lib
        l = L()
        return [l.vaenmf_train_gather(P(b.src), ldg, NT, P(b.idx), B, n_in, P(b.mean), P(b.std), 1e-8, P(b.gat), ldg, 2, st),
                l.vaenmf_train_dense_fwd(P(b.X), B, n_in, ldx, P(b.W), ldw, P(b.b), n_out, _lib.ACT_TANH, P(b.Y), ldy, st),
                l.vaenmf_train_dense_dx(P(b.dZ), B, n_out, ldz, P(b.W), ldw, n_in, P(b.Yp), ldp, _lib.ACT_TANH, P(b.dX), ldx, st),
                l.vaenmf_train_dense_dw(P(b.dZ), B, n_out, ldz, P(b.X), n_in, ldx, P(b.dW), ldw, P(b.db), st),
                l.vaenmf_elbo_out(P(b.Xe), ldx, P(b.A), lda, B, n_in, 1e-8, P(b.dA), lda, P(b.row_recon), st),
                l.vaenmf_elbo_latent_fwd(P(b.ML), ldm, P(b.eps), B, z, P(b.Zl), ldl, st),
                l.vaenmf_elbo_latent_bwd(P(b.ML), ldm, P(b.eps), P(b.dZl), ldl, B, z, P(b.dML), ldm, P(b.row_kl), st),
                l.vaenmf_bce_head(P(b.A2), lda, P(b.Yl), lda, B, D, 1e-8, P(b.dA2), lda, P(b.row_loss), P(b.row_cnt), st),
                l.vaenmf_loss_reduce(P(b.row_recon), P(b.row_kl), P(b.row_cnt), B, P(b.red), st),
                l.vaenmf_adam(P(b.p), P(b.g), P(b.m), P(b.v), NA, 1, 1e-3, 0.9, 0.999, 1e-8, st),
                l.vaenmf_train_eps_fill(5, 1, B, z, P(b.eps_out), st)]

    w = lambda name, n: Out(name, _cols(n), (), (_past(n),))          # columns between a row's width and its leading dimension: never written
    outs = [w("Y", n_out), w("dX", n_in), w("dW", n_in), Out("db"), w("dA", n_in), Out("row_recon"), w("Zl", z), w("dML", 2 * z), Out("row_kl"),
            w("dA2", D), Out("row_loss"), Out("row_cnt"), Out("red"), Out("gat", lambda t, d: t[:, 2:2 + n_in], (), (lambda t, d: t[:, :2], _past(2 + n_in))),
            Out("eps_out"), Out("p"), Out("m"), Out("v")]
    _add("train_kernels", ("vaenmf_train_gather", "vaenmf_train_dense_fwd", "vaenmf_train_dense_dx", "vaenmf_train_dense_dw", "vaenmf_elbo_out",
                           "vaenmf_elbo_latent_fwd", "vaenmf_elbo_latent_bwd", "vaenmf_bce_head", "vaenmf_loss_reduce", "vaenmf_adam",
                           "vaenmf_train_eps_fill"), make, call, outs)


_train_kernels()
TRAINER_CASES = ["train_m1_f65", "train_m2_vad_f65", "train_clf_vad_f65"]      # the smallest M1, M2 and classifier of train_cases


def _trainer(name):
    def case():
        import train_cases as tc
        return tc.GOLDEN_CASES[name]

    def make(seed):
        import train_cases as tc
        k = case()
        rng = np.random.default_rng(k.seed + 31 * seed)
        X, Y = tc.make_pool(rng, k, tc.POOL)
        sd = tc.state_of(tc.make_model(k))
        import vaenmf
        keys = vaenmf.train.state_keys(k.kind, len(k.hidden))
        a = {"X": X}
        if Y is not None:
            a["Y"] = Y
        for i, key in enumerate(keys):          # the initial weights of the case; contents B: moved a little
            a["P%d" % i] = (sd[key].numpy() + (0.01 * (seed - 1)) * rng.standard_normal(tuple(sd[key].shape))).astype(f32)
        a["zero"] = np.zeros(max(v.size for n, v in a.items() if n[0] == "P"), f32)
        o = {"loss%d" % j: ((8,), f64) for j in range(3)}
        for i in range(len(keys)):
            o["outP%d" % i], o["outG%d" % i] = (a["P%d" % i].shape, f32), (a["P%d" % i].shape, f32)
        if k.kind == "Classifier":
            a["mean"], a["std"] = X.mean(0).astype(f32), X.std(0, ddof=1).astype(f32)
        else:
            o["eps1"] = ((k.B, k.z_dim), f32)
        maps = dict(idx1=rng.choice(tc.POOL, k.B, replace=False).astype(i32), idx2=rng.choice(tc.POOL, k.B, replace=False).astype(i32))
        return Spec(inputs=a, maps=maps, outputs=o, host=SimpleNamespace(n=len(keys), k=k))

    def open_(spec):
        import torch
        import train_cases as tc
        from vaenmf import train as vt
        k = case()
        tr = vt.Trainer(tc.make_model(k), max_batch=k.B, seed=9, device="cuda:0")
        st = SimpleNamespace(tr=tr, h=tr._h, fixed={})
        if k.kind == "Classifier":          # the trainer keeps the pointers: one pair of buffers for every run of the case
            st.fixed = {"mean": torch.empty(k.x_dim, device="cuda"), "std": torch.empty(k.x_dim, device="cuda")}
            assert L().vaenmf_trainer_set_norm(st.h, P(st.fixed["mean"]), P(st.fixed["std"]), tc.LOSS_EPS) == 0
        torch.cuda.synchronize()
        return st

    def call(b, st, step):
        from vaenmf import _lib
        l, t, k, n = L(), b.state.h, b.spec.host.k, b.spec.host.n
        vae = k.kind != "Classifier"
        Y, ldy = (P(b.Y), k.y_dim) if k.kind != "M1" else (None, 0)
        r = []
        for i in range(n):
            src = P(getattr(b, "P%d" % i))
            r.append(l.vaenmf_trainer_set_params(t, i, src, st) if i % 2 else l.vaenmf_trainer_set_tensor(t, _lib.TRAIN_PARAM, i, src, st))
            r.append(l.vaenmf_trainer_set_tensor(t, _lib.TRAIN_ADAM_M, i, P(b.zero), st))
            r.append(l.vaenmf_trainer_set_tensor(t, _lib.TRAIN_ADAM_V, i, P(b.zero), st))
        r.append(l.vaenmf_trainer_set_step_count(t, 0))
        eps = None
        if vae:
            r.append(l.vaenmf_trainer_eps_fill(t, 1, k.B, 9, P(b.eps1), st))
            eps = P(b.eps1)
        run = lambda fn, idx, e, out: fn(t, P(b.X), k.x_dim, Y, ldy, b.X.shape[0], P(idx), k.B, e, 9, P(out), st)
        r.append(run(l.vaenmf_trainer_step, b.idx1, eps, b.loss0))          # the draws replayed from eps_fill
        r.append(run(l.vaenmf_trainer_step, b.idx2, None, b.loss1))         # the draws made on the device
        r.append(run(l.vaenmf_trainer_eval, b.idx1, eps, b.loss2))
        for i in range(n):
            dst = P(getattr(b, "outP%d" % i))
            r.append(l.vaenmf_trainer_get_params(t, i, dst, st) if i % 2 else l.vaenmf_trainer_get_tensor(t, _lib.TRAIN_PARAM, i, dst, st))
            r.append(l.vaenmf_trainer_get_tensor(t, _lib.TRAIN_GRAD, i, P(getattr(b, "outG%d" % i)), st))
        return r

    import train_cases as tc
    import vaenmf
    k = tc.GOLDEN_CASES[name]
    n = len(vaenmf.train.state_keys(k.kind, len(k.hidden)))
    outs = [Out("loss%d" % j) for j in range(3)] + [Out("out%s%d" % (w, i)) for i in range(n) for w in "PG"] + ([Out("eps1")] if k.kind != "Classifier" else [])
    entries = ("vaenmf_trainer_set_tensor", "vaenmf_trainer_set_params", "vaenmf_trainer_step", "vaenmf_trainer_eval", "vaenmf_trainer_get_tensor",
               "vaenmf_trainer_get_params") + (("vaenmf_trainer_eps_fill",) if k.kind != "Classifier" else ())
    _add("trainer_" + name, entries, make, call, outs, open=open_)


for _n in TRAINER_CASES:
    _trainer(_n)


# =====================================================================================================================
# the runner's pieces (tests/test_gpu_streams.py): device buffers of a case, the default-stream run
NAN_WORD, BIG_WORD = 0x7FC0A5A5, 0x7149F2CA          # tests/guarded.POISON


def _word(w):
    return int(np.array([w], np.uint32).view(np.int32)[0])


def poison(t, mixed=False):
    """Fill a dense tensor with the NaN word; mixed: the NaN word and 1e30 in turn (v_max and comparisons swallow a NaN)."""
    import torch
    if t.numel() == 0:
        return
    v = t.view(-1).view(torch.int32)
    v.fill_(_word(NAN_WORD))
    if mixed:
        v[1::2] = _word(BIG_WORD)


def stage(spec):
    """The contents of a Spec on the device: {name: tensor} of every float input and every map."""
    import torch
    return {n: torch.from_numpy(np.ascontiguousarray(a)).cuda() for n, a in list(spec.inputs.items()) + list(spec.maps.items())}


def alloc(case, spec, state, staged, prefill=None):
    """Device buffers of one run: float inputs poisoned (both words), maps valid, outputs and scratch poisoned -- except the
    `prefill` outputs, which start from the values given (the reference's) or zero."""
    import torch
    b = SimpleNamespace(state=state, spec=spec, names=[])
    fixed = getattr(state, "fixed", {}) if state is not None else {}
    for n, a in spec.inputs.items():
        t = fixed[n] if n in fixed else torch.empty_like(staged[n])
        poison(t, mixed=True)
        setattr(b, n, t)
    for n in spec.maps:
        setattr(b, n, staged[n].clone())
    for n, (shape, dt) in list(spec.outputs.items()) + list(spec.scratch.items()):
        if n in spec.inputs:                 # updated in place
            continue
        t = torch.empty(tuple(int(v) for v in shape), dtype=torch.from_numpy(np.empty(0, dt)).dtype, device="cuda")
        if n in spec.prefill:
            t.zero_() if prefill is None else t.copy_(prefill[n])
        else:
            poison(t)
        setattr(b, n, t)
    return b


def repoison(case, b, prefill=None):
    """The state before a run, on buffers that have been used: inputs and outputs poison, the prefilled outputs valid."""
    spec = b.spec
    for n in spec.inputs:
        poison(getattr(b, n), mixed=True)
    for n in list(spec.outputs) + list(spec.scratch):
        if n in spec.inputs:
            continue
        if n in spec.prefill:
            getattr(b, n).zero_() if prefill is None else getattr(b, n).copy_(prefill[n])
        else:
            poison(getattr(b, n))


def load(case, b, staged, stream):
    """Copies from staging into the inputs and maps on the current torch stream, then the case's own loading on `stream`."""
    for n, t in staged.items():
        getattr(b, n).copy_(t)
    if case.load is not None:
        rc = case.load(b, b.spec, stream)
        assert all(v == 0 for v in rc), (case.name, "load", rc)


def outputs_of(case, b):
    return {o.name: getattr(b, o.name).clone() for o in case.outs}


def run_default(case, state, spec, staged, prefill=None):
    """The reference of every comparison: the case on the default stream with ordinary allocations -> per step, {output: tensor}."""
    import torch
    if case.before is not None:
        case.before(state)
    b = alloc(case, spec, state, staged, prefill)
    res = []
    for step in range(len(case.steps)):
        if step:
            repoison(case, b, prefill)
        load(case, b, staged, None)
        rc = case.call(b, None, step)
        torch.cuda.synchronize()
        assert all(v == 0 for v in rc), (case.name, case.steps[step][0], rc, L().vaenmf_last_error().decode())
        res.append(outputs_of(case, b))
    return res, b


def compare(case, b, ref, staged, what):
    """After a run: every output bit-equal to the reference over its extent, its padding as documented, every float input
    that is not updated in place equal to its staging copy.  -> list of problems."""
    import torch
    from guarded import bits, same_bits
    d, bad = b.spec.d, []
    for o in case.outs:
        t, r = getattr(b, o.name), ref[o.name]
        ext = o.extent or (lambda t, d: t)
        if not same_bits(ext(t, d), ext(r, d)):
            x, y = bits(ext(t, d)), bits(ext(r, d))
            bad.append("%s: %s differs from the default-stream run over its extent (%d of %d words; %d still poison)"
                       % (what, o.name, int((x != y).sum()), x.numel(), int((x == _word(NAN_WORD)).sum())))
        for f in o.zero:
            if int(torch.count_nonzero(f(t, d))):
                bad.append("%s: padding of %s is not zero" % (what, o.name))
        for f in o.left:
            if not same_bits(f(t, d), f(r, d)) or not bool((bits(f(t, d)) == _word(NAN_WORD)).all()):
                bad.append("%s: padding of %s was touched" % (what, o.name))
    written = {o.name for o in case.outs}
    for n in b.spec.inputs:
        if n not in written and not same_bits(getattr(b, n), staged[n]):
            bad.append("%s: input %s changed" % (what, n))
    for n in b.spec.maps:
        if not same_bits(getattr(b, n), staged[n]):
            bad.append("%s: table %s changed" % (what, n))
    return bad
