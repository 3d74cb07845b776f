"""dev aid: STFT / iSTFT frame rates (HIP events) on a batch of 64 utterances of 4 s, per n_fft.

    python tools/stft_rate.py [--nfft 512,800,1024,1031] [--utts 64] [--seconds 4] [--fs 16000] [--reps 20] [--hann-array]

One JSON line per n_fft: the kernel family that runs it, frames per batch, microseconds per batched call and
nanoseconds per frame for stft_batch and istft_batch.  --hann-array passes periodic Hann as an explicit window, which
sends the power-of-two sizes to the any-length kernels too (for comparing the two families at one size)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "guided-vae-nmf_amd"))
import numpy as np
import torch

from vaenmf import stft as vstft


def family(n, explicit):
    if n & (n - 1) == 0 and n <= 2048 and not explicit:
        return "radix2"
    m = n
    for f in (2, 3, 5, 7):
        while m % f == 0:
            m //= f
    if m == 1:
        return "mixed"
    conv = 1
    while conv < 2 * n - 1:
        conv <<= 1
    return "bluestein(m=%d)" % conv


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps            # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nfft", default="512,800,1024,1031,2048,4093,4096")
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--fs", type=int, default=16000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--hann-array", action="store_true")
    a = ap.parse_args()
    T = int(a.seconds * a.fs)
    counts = [T] * a.utts
    wav = torch.from_numpy(np.random.default_rng(0).standard_normal(T * a.utts).astype(np.float32) * 0.1).cuda()
    for n in [int(v) for v in a.nfft.split(",")]:
        wl = n / a.fs
        nfft, hop = vstft.frame_geometry(T, a.fs, wl, 0.25)[:2]
        win = np.asarray(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)) if a.hann_array else "hann"
        X, fc = vstft.stft_batch(wav, counts, a.fs, wl, 0.25, win=win)
        NT = int(sum(fc))
        us_s = timed(lambda: vstft.stft_batch(wav, counts, a.fs, wl, 0.25, win=win), a.reps)
        us_i = timed(lambda: vstft.istft_batch(X, fc, counts, nfft, hop, win=win), a.reps)
        print(json.dumps({"nfft": n, "kernels": family(n, a.hann_array), "frames": NT,
                          "stft_us": round(us_s, 1), "stft_ns_per_frame": round(us_s * 1e3 / NT, 1),
                          "istft_us": round(us_i, 1), "istft_ns_per_frame": round(us_i * 1e3 / NT, 1)}), flush=True)


if __name__ == "__main__":
    main()
