"""dev aid: time of mix_batch's library call and of a vaenmf_feature_moments pass (HIP events around single calls), next to
the HBM bytes each moves.

    python tools/dataset_time.py [--utts 64] [--seconds 4] [--frames 32064] [--bins 513] [--reps 20] [--warmup 3]

Two JSON lines: microseconds per call (median of --reps single-call timings after --warmup untimed calls), the bytes the
call has to move (mix: the speech and the noise segment are read by the peak / energy / norm / write passes, three signals
are written; moments: the spectrogram is read once) and the rate that makes."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "guided-vae-nmf_amd"))
import numpy as np
import torch

from vaenmf._lib import check, lib
from vaenmf.dataset import snr_factor
from resample_time import median_us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--frames", type=int, default=32064)
    ap.add_argument("--bins", type=int, default=513)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    g = np.random.default_rng(0)
    fs, U = 16000, a.utts
    cut, T = int(0.1 * fs), int(a.seconds * fs) + int(0.1 * fs)
    speech = torch.from_numpy(g.standard_normal(U * T).astype(np.float32) * 0.1).cuda()
    noise = torch.from_numpy(g.standard_normal(60 * fs).astype(np.float32) * 0.1).cuda()
    kept = T - cut
    ioff = (np.arange(U + 1) * T).astype(np.int64)
    ooff = (np.arange(U + 1) * kept).astype(np.int64)
    cuts = np.full(U, cut, np.int64)
    starts = g.integers(0, 60 * fs - kept, U).astype(np.int64)
    f = np.array([snr_factor(v) for v in g.choice([-5.0, 0.0, 5.0], U)], np.float64)
    s, n, x = (torch.empty(U * kept, device="cuda") for _ in range(3))
    stats = torch.empty(U, 5, dtype=torch.float64, device="cuda")
    nbytes = lib().vaenmf_mix_work_bytes(U)
    work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for joint in (1, 0):
        call = lambda: check(lib().vaenmf_mix_batch(speech.data_ptr(), U, ioff.ctypes.data, cuts.ctypes.data, noise.data_ptr(), noise.shape[0],
                                                    starts.ctypes.data, f.ctypes.data, joint, ooff.ctypes.data, s.data_ptr(), n.data_ptr(),
                                                    x.data_ptr(), stats.data_ptr(), work.data_ptr(), nbytes, st))
        us = median_us(call, a.reps, a.warmup)
        passes = 1 + 2 * (3 if joint else 2)             # peak reads the speech; energy, (norm,) write read speech and noise
        moved = 4 * U * kept * (passes + 3)
        print(json.dumps({"call": "mix_batch", "joint_norm": joint, "utts": U, "samples": U * kept, "us": round(us[0], 1),
                          "us_min_max": [round(us[1], 1), round(us[2], 1)], "bytes": moved, "gb_per_s": round(moved / us[0] / 1e3, 1)}), flush=True)
    F = a.bins
    ld = (F + 15) // 16 * 16
    P = torch.from_numpy(g.random((a.frames, ld), dtype=np.float32)).cuda()
    S1, S2 = (torch.empty(F, dtype=torch.float64, device="cuda") for _ in range(2))
    nb = lib().vaenmf_moments_work_bytes(a.frames, F)
    w2 = torch.empty(nb, dtype=torch.uint8, device="cuda")
    call = lambda: check(lib().vaenmf_feature_moments(P.data_ptr(), a.frames, F, ld, 0, S1.data_ptr(), S2.data_ptr(), w2.data_ptr(), nb, st))
    us = median_us(call, a.reps, a.warmup)
    moved = 4 * a.frames * F
    print(json.dumps({"call": "feature_moments", "frames": a.frames, "bins": F, "ld": ld, "us": round(us[0], 1),
                      "us_min_max": [round(us[1], 1), round(us[2], 1)], "bytes": moved, "gb_per_s": round(moved / us[0] / 1e3, 1)}), flush=True)


if __name__ == "__main__":
    main()
