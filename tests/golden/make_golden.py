#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ by IMPORTING THE REFERENCE.

Runs only in the build container (needs /root/reference; it never travels to the
GPU box).  The reference's classes are driven unmodified:
  python.models.mcem.{MCEM_M1, MCEM_M2}, python.models.models.{VariationalAutoencoder,
  DeepGenerativeModel, Classifier}, python.metrics.energy_ratios.
Weights come from this repo's own seeded generator (oracle.xavier_normal_params)
and are loaded with load_state_dict; every torch.randn / torch.rand call made by
the reference is recorded so the oracle and the HIP path can replay the exact
noise.  Inside the patched torch.rand the caller's frame is inspected to capture
the MH log-acceptance (`acc_prob`, mcem.py:415-417) without touching the code.

Outputs are data only (inputs + expected outputs): *.npz, a few hundred KB each.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np
import torch

import vaenmf_oracle as orc
from python.models import mcem as ref_mcem
from python.models import models as ref_models
from python import metrics as ref_metrics

torch.set_num_threads(1)   # deterministic reduction order for the fixtures


class Recorder:
    """Records every torch.randn / torch.rand result (float32 numpy) in call order."""

    def __init__(self):
        self.draws = []
        self.kinds = []
        self.acc = []          # MH log-acceptance per step (captured from the caller frame)
        self._randn, self._rand = torch.randn, torch.rand

    def __enter__(self):
        rec = self

        def randn(*a, **k):
            t = rec._randn(*a, **k)
            rec.draws.append(t.detach().cpu().numpy().astype(np.float32).copy())
            rec.kinds.append("n")
            return t

        def rand(*a, **k):
            t = rec._rand(*a, **k)
            rec.draws.append(t.detach().cpu().numpy().astype(np.float32).copy())
            rec.kinds.append("u")
            fr = sys._getframe(1)
            if "acc_prob" in fr.f_locals:
                rec.acc.append(fr.f_locals["acc_prob"].detach().cpu().numpy().copy())
            return t

        torch.randn, torch.rand = randn, rand
        return self

    def __exit__(self, *a):
        torch.randn, torch.rand = self._randn, self._rand


def to_state(params):
    return {k: torch.tensor(v) for k, v in params.items()}


def pack_draws(prefix, draws):
    return {"%s%04d" % (prefix, i): d for i, d in enumerate(draws)}


def make_X(N, F, seed):
    g = np.random.default_rng(seed)
    # speech-like spectral envelope so the posterior is not flat
    env = (1.0 + 4.0 * np.exp(-np.arange(F) / (F / 6.0)))[None, :] * (0.3 + g.random((N, 1)))
    X = (g.standard_normal((N, F)) + 1j * g.standard_normal((N, F))) * env * 0.7
    return X.astype(np.complex64)


def run_case(name, model, F, N, K, dims_h, L, niter, counts, Dy=0, seed=0, n_try=40):
    """Full run() through the reference; picks the seed (of X and of the torch
    generator) whose smallest MH decision margin |log u - acc| is largest so the
    trajectory is robust to last-bit arithmetic differences."""
    best = None
    for t in range(n_try):
        sd = seed + 1000 * t
        params = orc.xavier_normal_params([F, L, dims_h], seed=sd, y_dim=Dy, bias_std=0.05)
        if model == "M1":
            vae = ref_models.VariationalAutoencoder([F, L, dims_h])
        else:
            vae = ref_models.DeepGenerativeModel([F, Dy, L, dims_h], None)
        vae.load_state_dict(to_state(params))
        vae.eval()
        X = make_X(N, F, sd + 1)
        kw = dict(niter=niter, nsamples_E_step=counts[0], burnin_E_step=counts[1],
                  nsamples_WF=counts[2], burnin_WF=counts[3], var_RW=0.01)
        m = ref_mcem.MCEM_M1(**kw) if model == "M1" else ref_mcem.MCEM_M2(**kw)
        y = None
        if model == "M2":
            y = (np.random.default_rng(sd + 2).random((N, Dy)) > 0.5).astype(np.float32)
        torch.manual_seed(sd)
        snaps = {}
        with torch.no_grad(), Recorder() as rec:
            if model == "M1":
                m.init_parameters(X=X, vae=vae, nmf_rank=K, eps=1e-8, device="cpu")
            else:
                m.init_parameters(X=X, y=torch.tensor(y), vae=vae, nmf_rank=K, eps=1e-8, device="cpu")
            snaps["Z0"] = m.Z.numpy().copy()
            snaps["W0"] = m.W.numpy().copy()
            snaps["H0"] = m.H.numpy().copy()
            # instrument the first EM iteration by hand (same calls as EM.run, mcem.py:159-165)
            cost = np.zeros(niter)
            for it in range(niter):
                m.E_step()
                if it == 0:
                    snaps["E1_Z"] = m.Z.numpy().copy()
                    snaps["E1_Vs"] = m.Vs.numpy().copy()
                    snaps["E1_Vx"] = m.Vx.numpy().copy()
                    snaps["E1_nacc"] = np.int64(len(rec.acc))
                m.M_step()
                if it == 0:
                    snaps["M1_W"] = m.W.numpy().copy()
                    snaps["M1_H"] = m.H.numpy().copy()
                    snaps["M1_g"] = m.g.numpy().copy()
                    snaps["M1_Vb"] = m.Vb.numpy().copy()
                    snaps["M1_Vx"] = m.Vx.numpy().copy()
                cost[it] = m.compute_expected_neg_log_like()
            WFs, WFn = m.compute_WF(sample=True)
            S_hat = WFs.numpy() * m.X
            N_hat = WFn.numpy() * m.X
        # decision margins
        us = [d for d, k in zip(rec.draws, rec.kinds) if k == "u" and d.ndim == 1]
        margins = np.concatenate([np.abs(np.log(u) - a) for u, a in zip(us, rec.acc)])
        mm = float(margins.min())
        if best is None or mm > best[0]:
            best = (mm, dict(
                seed=np.int64(sd), X=X, cost=cost, WFs=WFs.numpy(), WFn=WFn.numpy(),
                S_hat=S_hat.astype(np.complex64), N_hat=N_hat.astype(np.complex64),
                W=m.W.numpy(), H=m.H.numpy(), g=m.g.numpy(), Z=m.Z.numpy(),
                acc=np.stack(rec.acc), kinds="".join(rec.kinds),
                Vs_shape=np.array(m.Vs.shape), min_margin=np.float64(mm),
                meta=np.array([F, N, K, L, Dy, niter, *counts], dtype=np.int64),
                dims_h=np.array(dims_h, dtype=np.int64),
                **({"y": y} if y is not None else {}),
                **snaps,
                **{"p:" + k: v for k, v in params.items()},
                **pack_draws("d", rec.draws)))
    print("%s: min decision margin %.3e  (%d decisions, seed %d)" %
          (name, best[0], best[1]["acc"].size, best[1]["seed"]))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **best[1])


def nonmf_case():
    """MCEM_M2_noNMF (mcem.py:606-760): fixed noise variance, gains only."""
    F, N, L, Dy, H, niter = 65, 16, 32, 1, [128, 128], 3
    counts = (5, 7, 6, 9)
    best = None
    for t in range(30):
        sd = 77 + 1000 * t
        params = orc.xavier_normal_params([F, L, H], seed=sd, y_dim=Dy, bias_std=0.05)
        vae = ref_models.DeepGenerativeModel([F, Dy, L, H], None)
        vae.load_state_dict(to_state(params)); vae.eval()
        g0 = np.random.default_rng(sd + 3)
        X = make_X(N, F, sd + 1)
        Vb = (0.2 + g0.random((N, F))).astype(np.float32)
        gains = (0.5 + g0.random(N)).astype(np.float32)
        Z0 = (0.5 * g0.standard_normal((N, L))).astype(np.float32)
        y = (g0.random((N, Dy)) > 0.5).astype(np.float32)
        torch.manual_seed(sd)
        with torch.no_grad(), Recorder() as rec:
            m = ref_mcem.MCEM_M2_noNMF(X=X, Vb=Vb, g=torch.tensor(gains), Z=torch.tensor(Z0), y=torch.tensor(y), vae=vae,
                                       niter=niter, device="cpu", nsamples_E_step=counts[0], burnin_E_step=counts[1],
                                       nsamples_WF=counts[2], burnin_WF=counts[3], var_RW=0.01)
            cost = m.run()
        us = [d for d, k in zip(rec.draws, rec.kinds) if k == "u" and d.ndim == 1]
        margins = np.concatenate([np.abs(np.log(u) - a) for u, a in zip(us, rec.acc)])
        mm = float(margins.min())
        if best is None or mm > best[0]:
            best = (mm, dict(X=X, Vb=Vb, g0=gains, Z0=Z0, y=y, cost=cost, g=m.g.numpy(), Z=m.Z.numpy(),
                             S_hat=m.S_hat.astype(np.complex64), N_hat=m.N_hat.astype(np.complex64), acc=np.stack(rec.acc),
                             meta=np.array([F, N, 0, L, Dy, niter, *counts], dtype=np.int64), min_margin=np.float64(mm),
                             **{"p:" + k: v for k, v in params.items()}, **pack_draws("d", rec.draws)))
    print("m2_nonmf_f65: min decision margin %.3e (%d decisions)" % (best[0], best[1]["acc"].size))
    np.savez_compressed(os.path.join(HERE, "m2_nonmf_f65.npz"), **best[1])


def quirk_case():
    """Reference-faithful default counts: assert the positional-shift quirk
    (mcem.py:371 vs :461-462, :477-478): M1 runs S/R = 60/30 and 105/75;
    M2 runs 40/10 and 100/25."""
    F, N, K, L, H = 33, 6, 3, 8, [16, 16]
    out = {}
    for model, Dy in (("M1", 0), ("M2", 1)):
        params = orc.xavier_normal_params([F, L, H], seed=5, y_dim=Dy)
        if model == "M1":
            vae = ref_models.VariationalAutoencoder([F, L, H]); m = ref_mcem.MCEM_M1(niter=1)
        else:
            vae = ref_models.DeepGenerativeModel([F, Dy, L, H], None); m = ref_mcem.MCEM_M2(niter=1)
        vae.load_state_dict(to_state(params)); vae.eval()
        X = make_X(N, F, 9)
        torch.manual_seed(1)
        with torch.no_grad(), Recorder() as rec:
            if model == "M1":
                m.init_parameters(X=X, vae=vae, nmf_rank=K, eps=1e-8, device="cpu")
            else:
                m.init_parameters(X=X, y=torch.zeros(N, Dy), vae=vae, nmf_rank=K, eps=1e-8, device="cpu")
            m.E_step()
            n_e = len(rec.acc); R_e = m.Vs.shape[0]
            m.compute_WF(sample=True)
            n_wf = len(rec.acc) - n_e; R_wf = m.Vs.shape[0]
        out[model] = np.array([n_e, R_e, n_wf, R_wf], dtype=np.int64)
        print("quirk", model, "E-step steps/R = %d/%d, WF steps/R = %d/%d" % (n_e, R_e, n_wf, R_wf))
    assert tuple(out["M1"]) == (60, 30, 105, 75) and tuple(out["M2"]) == (40, 10, 100, 25)
    np.savez_compressed(os.path.join(HERE, "quirk_counts.npz"), **out)


def mlp_case():
    """Encoder / decoder / classifier forwards (models.py:101-121, 57-62)."""
    F, L, H, N = 129, 32, [128, 128], 24
    out = {}
    for tag, Dy in (("m1", 0), ("m2", 3)):
        params = orc.xavier_normal_params([F, L, H], seed=11, y_dim=Dy, bias_std=0.1)
        if Dy == 0:
            vae = ref_models.VariationalAutoencoder([F, L, H])
        else:
            vae = ref_models.DeepGenerativeModel([F, Dy, L, H], None)
        vae.load_state_dict(to_state(params)); vae.eval()
        g = np.random.default_rng(3)
        x = (g.random((N, F + Dy)) * 2).astype(np.float32)
        z = g.standard_normal((N, L + Dy)).astype(np.float32)
        torch.manual_seed(2)
        with torch.no_grad(), Recorder() as rec:
            zz, mu, lv = vae.encoder(torch.tensor(x))
            dec = vae.decoder(torch.tensor(z))
        out.update({tag + "_x": x, tag + "_z": z, tag + "_eps": rec.draws[0], tag + "_zz": zz.numpy(),
                    tag + "_mu": mu.numpy(), tag + "_lv": lv.numpy(), tag + "_dec": dec.numpy()})
        out.update({tag + ":p:" + k: v for k, v in params.items()})
    cp = orc.xavier_normal_classifier([F, [128, 128], 5], seed=12, bias_std=0.1)
    clf = ref_models.Classifier([F, [128, 128], 5]); clf.load_state_dict(to_state(cp)); clf.eval()
    xc = (np.random.default_rng(4).standard_normal((N, F))).astype(np.float32)
    with torch.no_grad():
        yc = clf(torch.tensor(xc)).numpy()
    out.update({"clf_x": xc, "clf_y": yc})
    out.update({"clf:p:" + k: v for k, v in cp.items()})
    np.savez_compressed(os.path.join(HERE, "mlp_forward.npz"), **out)
    print("mlp_forward: done")


def read_wav_int16(path):
    """Minimal RIFF/WAVE PCM16 mono reader (soundfile is not installed)."""
    b = open(path, "rb").read()
    assert b[:4] == b"RIFF" and b[8:12] == b"WAVE"
    pos = 12
    fs = None
    while pos < len(b):
        cid, sz = b[pos:pos + 4], int.from_bytes(b[pos + 4:pos + 8], "little")
        if cid == b"fmt ":
            fmt = int.from_bytes(b[pos + 8:pos + 10], "little")
            ch = int.from_bytes(b[pos + 10:pos + 12], "little")
            fs = int.from_bytes(b[pos + 12:pos + 16], "little")
            bits = int.from_bytes(b[pos + 22:pos + 24], "little")
            assert fmt == 1 and ch == 1 and bits == 16
        if cid == b"data":
            return np.frombuffer(b[pos + 8:pos + 8 + sz], dtype="<i2").copy(), fs
        pos += 8 + sz + (sz & 1)
    raise ValueError("no data chunk")


def metrics_case():
    """python/metrics.py:39-60 on the reference-committed dummy-M2 outputs
    (data/subset/models/dummy_M2_.../440c020{a,b}_s_est.wav; the figure title of
    440c020a_fig.png reads SI-SDR -6.2 / SI-SIR -4.3 / SI-SAR -1.9).  int16 PCM is
    stored as-is; sf.read semantics = int16/32768 as float64."""
    proc = "/root/reference/data/subset/processed/CSR-1-WSJ-0/WAV/wsj0/si_et_05/440/"
    est = ("/root/reference/data/subset/models/dummy_M2_alpha_5.0_epoch_100_vloss_466.72/"
           "CSR-1-WSJ-0/WAV/wsj0/si_et_05/440/")
    out = {}
    for u in ("a", "b"):
        s, fs = read_wav_int16(proc + "440c020%s_s.wav" % u)
        n, _ = read_wav_int16(proc + "440c020%s_n.wav" % u)
        x, _ = read_wav_int16(proc + "440c020%s_x.wav" % u)
        sh, _ = read_wav_int16(est + "440c020%s_s_est.wav" % u)
        assert fs == 16000 and len(s) == len(n) == len(sh)
        r = ref_metrics.energy_ratios(sh / 32768.0, s / 32768.0, n / 32768.0)
        print("metrics 440c020%s:" % u, r)
        out[u + "_ratios"] = np.array(r)
        if u == "a":     # PCM of one utterance only (size); b keeps its expected ratios for the record
            out.update({u + "_s": s, u + "_n": n, u + "_s_est": sh})
    np.savez_compressed(os.path.join(HERE, "metrics_dummy_m2.npz"), **out)


def labels_case():
    """python/processing/target.py:7-102 (Lorenz-quantile IBM / VAD labels and their noise-robust
    variants, ideal Wiener mask) on the clean-speech STFTs of two seeded synthetic utterances
    (complex64, 512-pt: F=257) -- the call pattern of scripts/create_train_set.py:136-150 and
    run_metrics_M2.py:141-148."""
    from python.processing import target as ref_target
    out = {}
    for u, (seed, T) in enumerate(((3, 12000), (5, 9000))):
        s, n, x, _ = orc.synth_utterance(seed, n_samples=T)
        S = orc.stft(s, fs=16000, wlen_sec=32e-3, hop_percent=0.25)       # complex64 (F, N)
        Nn = orc.stft(n, fs=16000, wlen_sec=32e-3, hop_percent=0.25)
        assert S.dtype == np.complex64
        out["S%d" % u] = S
        out["N%d" % u] = Nn
        out["ibm%d" % u] = ref_target.clean_speech_IBM(S, quantile_fraction=0.999, quantile_weight=0.999)
        out["ibm98_%d" % u] = ref_target.clean_speech_IBM(S)
        out["vad%d" % u] = ref_target.clean_speech_VAD(S, quantile_fraction=0.999, quantile_weight=0.999)
        out["vad98_%d" % u] = ref_target.clean_speech_VAD(S)
        out["nrvad%d" % u] = ref_target.noise_robust_clean_speech_VAD(S)
        out["nribm%d" % u] = ref_target.noise_robust_clean_speech_IBM(S)
        out["iwm%d" % u] = ref_target.ideal_wiener_mask(S, Nn)
        print("labels utt", u, S.shape, "ibm on", out["ibm%d" % u].mean(), "vad on", out["vad%d" % u].mean(),
              "nrvad on", out["nrvad%d" % u].mean())
    np.savez_compressed(os.path.join(HERE, "labels_f257.npz"), **out)


def labels_blocks_case():
    """target.py:7-50 on seeded inputs whose sorted run is longer than numpy's 8192-element reduction buffer: there
    np.sum(sorted_power) is a sum of per-block pairwise sums, and a label flips when the total is rounded in any other
    order.  Four IBM inputs (F, N, seed) at q = 0.98 and 0.999 and one VAD input of 8300 frames.  Only the seeds, the
    shapes and the outputs are stored (labels as uint8; `thr`: sorted_power[lorenz < q][-1] by the same numpy calls);
    the tests rebuild the inputs with orc.heavy_tailed_stft."""
    from python.processing import target as ref_target

    def threshold(power, q):                                  # the numpy calls of target.py:18-21 / :40-43
        srt = np.sort(power, axis=None)[::-1]
        return srt[np.cumsum(srt) / np.sum(srt) < q][-1]

    ibm = [(65, 130, 2), (65, 130, 11), (257, 33, 23), (33, 257, 21)]
    vad = [(2, 8300, 4)]
    qs = [0.98, 0.999]
    out = {"ibm_cases": np.array(ibm, np.int64), "vad_cases": np.array(vad, np.int64), "q": np.array(qs, np.float64)}
    for mode, cases, fn in (("ibm", ibm, ref_target.clean_speech_IBM), ("vad", vad, ref_target.clean_speech_VAD)):
        for c, (F, N, seed) in enumerate(cases):
            X = orc.heavy_tailed_stft(F, N, seed)
            power = abs(X * X.conj())
            if mode == "vad":
                power = power.sum(axis=0)
            assert power.size > 8192 and power.dtype == np.float32
            for j, q in enumerate(qs):
                y = fn(X, quantile_fraction=q, quantile_weight=0.999)
                assert y.dtype == np.float32 and set(np.unique(y)) <= {0.0, 1.0}
                out["%s%d_q%d" % (mode, c, j)] = y.astype(np.uint8)
                out["%s%d_q%d_thr" % (mode, c, j)] = np.float32(threshold(power, q))
                print("labels_blocks", mode, (F, N, seed), q, "on", y.mean(), "thr", out["%s%d_q%d_thr" % (mode, c, j)])
    np.savez_compressed(os.path.join(HERE, "labels_blocks.npz"), **out)


def spp_case():
    """python/models/spp_estimation.py:163-235 on the noisy power spectrogram of a seeded synthetic mixture
    (float32 |X|^2 as scripts/evaluate_M2_ibm.py:137-138 builds it).  Only outputs are stored; the input
    is regenerated from the seed by the test."""
    from python.models import spp_estimation as ref_spp
    out = {}
    for u, (seed, T) in enumerate(((3, 12000), (5, 9000))):
        x = orc.synth_utterance(seed, n_samples=T)[2]
        X = orc.stft(x, fs=16000, wlen_sec=32e-3, hop_percent=0.25)
        P = np.power(np.abs(X), 2)                      # (F, N) float32
        assert P.dtype == np.float32
        m = ref_spp.timo_mask_estimation(P)
        out["P%d" % u] = P
        out["mask%d" % u] = m
        out["vad%d" % u] = ref_spp.timo_vad_estimation(P)
        out["psd%d" % u] = ref_spp.timo_noise_estimation(P, m)
        print("spp utt", u, P.shape, "mask>0.5:", (m > 0.5).mean(), "vad mean", out["vad%d" % u].mean())
    np.savez_compressed(os.path.join(HERE, "spp_f257.npz"), **out)


def classifier_variants_case():
    """Classifier(batch_norm=True) in eval mode (scripts/reconstruct_dnn_classif.py:80,125-129) and Classifier2Classes
    (models.py:64-88): forwards of the reference classes on seeded weights and non-trivial running statistics."""
    F, N, Dy = 129, 24, 5
    g = np.random.default_rng(21)
    out = {}
    x = g.standard_normal((N, F)).astype(np.float32)
    clf = ref_models.Classifier([F, [128, 128], Dy], batch_norm=True)
    sd = {}
    for k, v in clf.state_dict().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(7)
        elif "running_var" in k:
            sd[k] = torch.tensor((0.5 + g.random(tuple(v.shape))).astype(np.float32))
        elif "running_mean" in k:
            sd[k] = torch.tensor((0.3 * g.standard_normal(tuple(v.shape))).astype(np.float32))
        elif v.ndim == 1 and k.startswith("hidden") and int(k.split(".")[1]) % 2 == 1 and k.endswith("weight"):
            sd[k] = torch.tensor((0.5 + g.random(tuple(v.shape))).astype(np.float32))          # BN gamma
        else:
            sd[k] = torch.tensor((g.standard_normal(tuple(v.shape)) * (0.1 if v.ndim == 1 else 1.0 / np.sqrt(v.shape[-1]))).astype(np.float32))
    clf.load_state_dict(sd); clf.eval()
    with torch.no_grad():
        out["bn_y"] = clf(torch.tensor(x)).numpy()
    out.update({"bn:p:" + k: v.numpy() for k, v in sd.items()})
    c2 = ref_models.Classifier2Classes([F, [128, 128], Dy])
    sd2 = {k: torch.tensor((g.standard_normal(tuple(v.shape)) * (0.1 if v.ndim == 1 else 1.0 / np.sqrt(v.shape[-1]))).astype(np.float32))
           for k, v in c2.state_dict().items()}
    c2.load_state_dict(sd2); c2.eval()
    with torch.no_grad():
        out["c2_y"] = c2(torch.tensor(x)).numpy()
    out.update({"c2:p:" + k: v.numpy() for k, v in sd2.items()})
    out["x"] = x
    np.savez_compressed(os.path.join(HERE, "mlp_forward_variants.npz"), **out)
    print("mlp_forward_variants:", out["bn_y"].shape, out["c2_y"].shape)


def shapes_case():
    """Decoder shapes beside 32 -> 128 -> 128 -> F that the reference's scripts list (scripts/evaluate_M1.py:44-85: z_dim 16,
    h_dim [128]): full runs through the reference's generic classes (models.py:107-133) at those dims."""
    run_case("m1_f65_z16", "M1", F=65, N=16, K=4, dims_h=[128, 128], L=16, niter=3, counts=(10, 6, 25, 8), seed=7)
    run_case("m1_f65_h128", "M1", F=65, N=16, K=4, dims_h=[128], L=32, niter=3, counts=(10, 6, 25, 8), seed=11)
    run_case("m2_vad_f65_z16_h128", "M2", F=65, N=16, K=4, dims_h=[128], L=16, niter=3, counts=(5, 7, 6, 9), Dy=1, seed=13)


if __name__ == "__main__":
    only = sys.argv[1:]
    if only:
        for f in only:
            globals()[f]()
        sys.exit(0)
    quirk_case()
    mlp_case()
    labels_case()
    labels_blocks_case()
    spp_case()
    metrics_case()
    # real decoder dims (L=32, H=[128,128]) so the HIP path can run the same cases
    run_case("m1_f65", "M1", F=65, N=16, K=4, dims_h=[128, 128], L=32, niter=3, counts=(10, 6, 25, 8))
    run_case("m2_vad_f65", "M2", F=65, N=16, K=4, dims_h=[128, 128], L=32, niter=3, counts=(5, 7, 6, 9), Dy=1)
    run_case("m2_ibm_f65", "M2", F=65, N=16, K=4, dims_h=[128, 128], L=32, niter=2, counts=(5, 7, 6, 9), Dy=65, n_try=20)
    run_case("m1_f257", "M1", F=257, N=24, K=8, dims_h=[128, 128], L=32, niter=2, counts=(10, 3, 25, 4), n_try=12)
