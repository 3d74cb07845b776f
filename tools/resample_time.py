"""dev aid: time of resample_batch (HIP events around single batched calls) next to stft_batch on the same batch.

    python tools/resample_time.py [--utts 64] [--seconds 4] [--pairs 48000:16000,16000:48000] [--reps 20] [--warmup 3]

One JSON line per rate pair: microseconds per call (median of --reps single-call timings after --warmup untimed calls),
input and output samples, nanoseconds per output sample, and the time of stft_batch (64 ms Hann window, hop 1/4) on the
16 kHz side of the same batch, taken the same way."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "guided-vae-nmf_amd"))
import numpy as np
import torch

from vaenmf import stft as vstft
from vaenmf.resample import resample_batch


def median_us(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--pairs", default="48000:16000,16000:48000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    g = np.random.default_rng(0)
    for pair in a.pairs.split(","):
        fs_in, fs_out = [int(v) for v in pair.split(":")]
        T = int(a.seconds * fs_in)
        counts = [T] * a.utts
        wav = torch.from_numpy(g.standard_normal(T * a.utts).astype(np.float32) * 0.1).cuda()
        y, counts_out = resample_batch(wav, counts, fs_in, fs_out)
        us = median_us(lambda: resample_batch(wav, counts, fs_in, fs_out), a.reps, a.warmup)
        lo, lo_counts = (y, counts_out) if fs_out <= fs_in else (wav, counts)              # the batch at the lower rate
        fs_lo = min(fs_in, fs_out)
        us_stft = median_us(lambda: vstft.stft_batch(lo, lo_counts, fs_lo, 64e-3, 0.25), a.reps, a.warmup)
        print(json.dumps({"fs_in": fs_in, "fs_out": fs_out, "utts": a.utts, "samples_in": T * a.utts, "samples_out": int(sum(counts_out)),
                          "resample_us": round(us[0], 1), "resample_us_min_max": [round(us[1], 1), round(us[2], 1)],
                          "ns_per_output": round(us[0] * 1e3 / sum(counts_out), 3),
                          "stft_us": round(us_stft[0], 1), "stft_us_min_max": [round(us_stft[1], 1), round(us_stft[2], 1)]}), flush=True)


if __name__ == "__main__":
    main()
