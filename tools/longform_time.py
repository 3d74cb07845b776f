"""Measurement aid for DESIGN 3.5c: one long synthetic mixture through Reconstructor.enhance_long -- wall time, rounds, rounds
launched as a HIP graph, device time of the row kernels (gather + blend) next to that of the em() rounds -- and its SI-SDR
next to the same mixture enhanced as ONE utterance on an engine large enough to hold it.
usage: python tools/longform_time.py [--minutes 10] [--segment-sec 30] [--overlap-sec 2] [--max-frames 16384] [--no-whole]
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "guided-vae-nmf_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--segment-sec", type=float, default=30.0)
    ap.add_argument("--overlap-sec", type=float, default=2.0)
    ap.add_argument("--max-frames", type=int, default=16384)
    ap.add_argument("--niter", type=int, default=100)
    ap.add_argument("--no-whole", action="store_true")
    a = ap.parse_args()
    from vaenmf import longform as lf
    from vaenmf.metrics import gram3_batch, ratios_from_gram
    from vaenmf.pipeline import Reconstructor
    from vaenmf.synth import synth_utterance, xavier_normal_params
    F, K, fs = 257, 8, 16000
    pieces = [synth_utterance(k) for k in range(int(round(a.minutes * 60 / 4)))]          # 4 s each
    s, n = np.concatenate([p[0] for p in pieces]), np.concatenate([p[1] for p in pieces])
    cu = lambda v: torch.from_numpy(v.astype(np.float32)).cuda()
    s, n, x, T = cu(s), cu(n), cu(s + n), len(s)
    params = xavier_normal_params([F, 32, [128, 128]], seed=0)
    mk = lambda mf, mu: Reconstructor(params, F, K, niter=a.niter, fs=fs, wlen_sec=32e-3, precision="bf16", max_frames=mf, max_utts=mu)
    sdr = lambda est: float(ratios_from_gram(gram3_batch(est, s, n, [T])[0])[0])
    rec = mk(a.max_frames, 64)
    spans = {"rows": [], "em": []}

    def timed(kind, fn):
        def wrapped(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*args, **kw)
            e1.record()
            spans[kind].append((e0, e1))
            return out
        return wrapped

    lf.gather_rows, lf.blend_rows, rec.em = timed("rows", lf.gather_rows), timed("rows", lf.blend_rows), timed("em", rec.em)
    out = {"frames": None, "samples": T, "segment_sec": a.segment_sec, "overlap_sec": a.overlap_sec, "max_frames": a.max_frames, "calls": []}
    for _ in range(2):                                                   # the first call allocates and captures
        for v in spans.values():
            v.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s_hat, _, _ = rec.enhance_long(x, [T], a.segment_sec, a.overlap_sec, seeds=[1], init_seed=0)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        ms = {k: sum(e0.elapsed_time(e1) for e0, e1 in v) for k, v in spans.items()}
        out["calls"].append({"wall_s": wall, "rows_ms": ms["rows"], "em_ms": ms["em"], "row_launches": len(spans["rows"]), **rec.long_rounds})
    out["frames"], out["segments"] = int(sum(rec.frame_counts)), len(rec.segments.seg_len)
    out["si_sdr_segmented_db"] = sdr(s_hat)
    out["si_sdr_input_db"] = sdr(x)
    if not a.no_whole:
        del rec
        torch.cuda.empty_cache()
        whole = mk(out["frames"], 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        w_hat, _, _ = whole.enhance(x, [T], seeds=[1], init_seed=0)
        torch.cuda.synchronize()
        out["whole_wall_s"] = time.perf_counter() - t0
        out["si_sdr_whole_db"] = sdr(w_hat)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
