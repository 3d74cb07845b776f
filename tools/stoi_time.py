"""dev aid: time of metrics.stoi_batch_device for 64 utterances of 4 s at 16 kHz on one MI355X: HIP events around single
calls, median of 20 after 5 warm-ups, the resampling and the score apart, and for scale the numpy restatement of
tests/stoi_cases.py on the same batch.  Usage: python tools/stoi_time.py"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("guided-vae-nmf_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import torch
import stoi_cases as sc
from vaenmf import metrics as vm

U, T = 64, 64000
rng = np.random.default_rng(1)
xs, ys = [], []
for u in range(U):
    t = np.arange(T) / 16000.0
    env = np.clip(np.sin(2 * np.pi * (0.7 + 0.02 * u) * t + u), 0.0, None) ** 2 + 1e-4      # pauses the silence removal cuts
    x = rng.standard_normal(T) * env * 0.1
    xs.append(x.astype(np.float32)); ys.append((x + 0.05 * rng.standard_normal(T)).astype(np.float32))
clean = torch.from_numpy(np.concatenate(xs)).cuda(); proc = torch.from_numpy(np.concatenate(ys)).cuda()
counts = [T] * U

def timed(fn, warm=5, reps=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

for ext in (True, False):
    print("stoi_batch_device 64 x 4 s @ 16 kHz, extended=%s: median %.3f ms (min %.3f, max %.3f)" % ((ext,) + timed(lambda: vm.stoi_batch_device(clean, proc, counts, 16000, ext))))
from vaenmf.resample import resample_batch
c10, n10 = resample_batch(clean, counts, 16000, 10000); p10, _ = resample_batch(proc, counts, 16000, 10000)
print("  the two resample_batch calls alone: median %.3f ms (min %.3f, max %.3f)" % timed(lambda: (resample_batch(clean, counts, 16000, 10000), resample_batch(proc, counts, 16000, 10000))))
print("  the score at 10 kHz alone (40000 samples each): median %.3f ms (min %.3f, max %.3f)" % timed(lambda: vm.stoi_batch_device(c10, p10, n10, 10000, True)))
d = vm.stoi_batch(clean, proc, counts, 16000, True)
t0 = time.perf_counter()
ref = [sc.score(x, y, 16000, True) for x, y in zip(xs, ys)]
t1 = time.perf_counter()
print("numpy restatement, same batch, one host thread: %.2f s" % (t1 - t0))
err = max(abs(d[u] - ref[u]["d"]) for u in range(U))
print("max |d - restatement| over the batch: %.2e; min margin %.3f dB; kept %.1f %%; mean ESTOI %.4f" %
      (err, min(r["margin"] for r in ref), 100.0 * sum(r["k"] for r in ref) / sum(r["n_frames"] for r in ref), float(np.mean(d))))
