"""bench.py --dump-outputs: the arrays the timed path returned in its last step, written as float32 / float64 .npy files
under a size budget, the same from run to run with the same arguments; and a plain run prints the headline only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"s_hat", "n_hat", "cost", "utterances", "si_sdr_stats"}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_samples_a_fixed_subset_under_the_budget(tmp_path, monkeypatch):
    """Host side of the dump on CPU tensors: three batches of 20 utterances over a budget that holds 7 of them."""
    import bench
    T, niter = 1000, 5
    per_utt = 2 * T * 4 + niter * 8 + 8
    stats = np.arange(12, dtype=np.float64).reshape(1, 4, 3)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 7 * per_utt + stats.nbytes)
    g = torch.Generator().manual_seed(3)
    outs = [(torch.randn(20 * T, generator=g), torch.randn(20 * T, generator=g), torch.randn(20, niter, generator=g, dtype=torch.float64))
            for _ in range(3)]
    uids = list(range(100, 160))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outs, uids, T, stats)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == NAMES and all(np.array_equal(a[k], b[k]) for k in NAMES)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BUDGET
    u = a["utterances"].astype(np.int64)
    assert len(u) == 7 and np.all(np.diff(u) > 0) and u[0] >= 100 and u[-1] < 160
    s_all = torch.cat([o[0] for o in outs]).view(60, T).numpy()
    c_all = torch.cat([o[2] for o in outs]).numpy()
    assert np.array_equal(a["s_hat"], s_all[u - 100]) and np.array_equal(a["cost"], c_all[u - 100])
    assert a["s_hat"].shape == a["n_hat"].shape == (7, T) and np.array_equal(a["si_sdr_stats"], stats)


def _bench(d):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--utts", "4", "--niter", "3", "--steps", "2", "--warmup", "1",
           "--dump-outputs", str(d)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0]), _load(d)


@pytest.mark.gpu
def test_plain_bench_dumps_its_last_timed_step_the_same_every_run(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    line, o = _bench(tmp_path / "a")
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    assert not {"kernels", "roofline", "configs", "parity_mode", "config_1_gpu", "cpu_baseline", "hbm_read_probe"} & set(line)
    assert set(o) == NAMES and all(v.dtype in (np.float32, np.float64) for v in o.values())
    assert sum(os.path.getsize(p) for p in (tmp_path / "a").iterdir()) <= 64 * 2 ** 20
    assert o["s_hat"].shape == o["n_hat"].shape == (4, 64000) and o["cost"].shape == (4, 3)
    assert np.array_equal(o["utterances"], np.arange(4)) and np.all(np.isfinite(o["s_hat"])) and np.all(np.isfinite(o["n_hat"]))
    # the dumped arrays are the ones the result line summarises
    assert abs(line["final_cost_mean"] - o["cost"][:, -1].mean()) <= 1e-12 * abs(line["final_cost_mean"])
    st = o["si_sdr_stats"]
    assert abs(line["si_sdr_mean_db"] - st[0, 0, 1] / max(st[0, 0, 0], 1)) <= 1e-12 * abs(line["si_sdr_mean_db"])
    _, o2 = _bench(tmp_path / "b")
    for k in NAMES:
        assert np.array_equal(o[k], o2[k]), k
