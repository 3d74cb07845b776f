"""STOI / ESTOI without a GPU: the numpy restatement (tests/stoi_cases.py) against the values the reference printed for
its committed utterances, the host entry points of the library against the restatement, and the statistics harness with
and without the fourth column."""
import os

import numpy as np
import pytest

import stoi_cases as sc

LENGTHS = (0, 255, 256, 257, 384, 385, 4096, 4097, 4225)
SEGMENTS = {"a": 499, "b": 696, "c": 613}


def test_restatement_reproduces_the_printed_values():
    """ESTOI of the 16 kHz pairs, resampled to 10 kHz, rounds to the two decimals of the reference's figure titles, with
    the segment counts of the prototype; classic STOI is a score of its own on the same frames."""
    utts = sc.reference_utterances()
    assert "a" in utts and "b" in utts
    for name, (s, e, printed) in utts.items():
        r = sc.score(s, e, 16000, extended=True)
        print("%s: ESTOI %.6f (printed %.2f), frames %d, kept %d, segments %d, margin %.3f dB" %
              (name, r["d"], printed, r["n_frames"], r["k"], r["J"], r["margin"]))
        assert round(r["d"], 2) == printed
        assert r["J"] == SEGMENTS[name] and r["J"] == r["k"] - 30
        c = sc.score(s, e, 16000, extended=False)
        assert c["counts"] == r["counts"] and r["d"] < c["d"] < 1.0


def test_restatement_edge_cases():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(6000)
    assert abs(sc.core(x, x, True)["d"] - 1.0) < 1e-12 and abs(sc.core(x, x, False)["d"] - 1.0) < 1e-12
    z = np.zeros(5000)
    for ext in (True, False):
        r = sc.core(z, z, ext)
        assert r["d"] == 0.0 and r["k"] == r["n_frames"] == 38          # digital silence: every frame kept, score 0
    assert sc.core(x[:256], x[:256])["d"] == sc.NO_SCORE and sc.core(x[:256], x[:256])["counts"] == (0, 0, 0)
    w = sc.window()
    assert w.shape == (256,) and w[0] > 0 and abs(w[0] - w[-1]) < 1e-15 and abs(w[127] - w[128]) < 1e-15   # symmetric, no zero end
    assert np.allclose(w, np.hanning(258)[1:-1], rtol=0, atol=1e-15)


@pytest.mark.parametrize("T", LENGTHS)
def test_geometry_matches_the_restatement(T):
    from vaenmf import metrics as vm
    assert vm.stoi_geometry(T) == sc.geometry(T)
    nf = vm.stoi_geometry(T)[0]
    assert nf == (0 if T <= 256 else -(-(T - 256) // 128))               # strict: 4096 = 256 + 30 * 128 has 30 frames, not 31


def test_geometry_refuses_a_negative_length():
    from vaenmf import metrics as vm
    from vaenmf._lib import VaenmfError
    with pytest.raises(VaenmfError):
        vm.stoi_geometry(-1)


def test_bands_match_the_restatement():
    from vaenmf import metrics as vm
    lo, hi = vm.stoi_bands()
    rlo, rhi = sc.bands()
    assert np.array_equal(lo, rlo) and np.array_equal(hi, rhi)
    assert np.array_equal(lo[1:], hi[:-1]) and lo[0] == 7 and hi[-1] == 219     # contiguous, 137 Hz .. 4.28 kHz


def test_work_bytes_covers_the_worst_case():
    """Room for every intermediate at k = n_frames, and monotone in the batch."""
    from vaenmf import metrics as vm
    from vaenmf._lib import lib
    counts = [0, 257, 4097, 9000]
    off = vm.stoi_offsets(counts)
    n = lib().vaenmf_stoi_work_bytes(len(counts), off.ctypes.data)
    g = [sc.geometry(T) for T in counts]
    need = 8 * sum(a for a, _, _ in g) + 2 * 16 * 8 * sum(b for _, b, _ in g) + 8 * sum(c for _, _, c in g)
    assert n >= need
    assert lib().vaenmf_stoi_work_bytes(3, off.ctypes.data) < n
    bad = np.array([0, 10, 5], np.int64)
    assert lib().vaenmf_stoi_work_bytes(2, bad.ctypes.data) == -1


def _subset_tree(tmp_path, n=3):
    """The first n utterances of the committed nine-utterance subset as a processed tree, the noisy mixture standing in
    for the model's estimate."""
    from vaenmf import wavio
    z = np.load(sc.GOLDEN + "/processed_subset9.npz")
    proc, out = str(tmp_path) + "/processed/", str(tmp_path) + "/model/"
    files = []
    for i in range(n):
        rel = str(z["rel"][i])
        stem = os.path.splitext(rel)[0]
        for base in (proc, out):
            os.makedirs(os.path.dirname(base + rel), exist_ok=True)
        for k in "sn":
            wavio.write(proc + stem + "_%s.wav" % k, z["u%d_%s" % (i, k)] / 32768.0, 16000)
        wavio.write(out + stem + "_s_est.wav", z["u%d_x" % i] / 32768.0, 16000)
        files.append(rel)
    return files, proc, out


def _gram3_numpy(s_hat, s, n, counts):
    v = [t.double().cpu().numpy() for t in (s_hat, s, n)]
    off = np.concatenate([[0], np.cumsum(counts)])
    rows = []
    for u in range(len(counts)):
        a, b, c = [x[off[u]:off[u + 1]] for x in v]
        rows.append([a @ a, a @ b, a @ c, b @ b, b @ c, c @ c])
    return np.array(rows)


def test_run_metrics_default_rows_have_three_values(tmp_path, monkeypatch, capsys):
    """estoi=False (the default) is what it was: rows of three, a table of three metrics, statistics [groups, 3, 3].  The
    Gram sums come from numpy here (no GPU); the STOI pass must not be touched."""
    from vaenmf import metrics as vm, run_metrics
    files, proc, out = _subset_tree(tmp_path)
    monkeypatch.setattr(vm, "gram3_batch", _gram3_numpy)
    monkeypatch.setattr(vm, "stoi_batch", lambda *a, **k: pytest.fail("the default must not compute ESTOI"))
    rows = run_metrics.compute_metrics(files, proc, out, device="cpu")
    assert len(rows) == 3 and all(len(r) == 3 for r in rows)
    assert rows == run_metrics.compute_metrics(files, proc, out, device="cpu", estoi=False)
    capsys.readouterr()
    all_metrics, st = run_metrics.main(files, proc, out, [-5.0, 0.0, 0.0], device="cpu")
    text = capsys.readouterr().out
    assert all_metrics == rows and st.shape == (3, 3, 3)
    assert "SI-SDR" in text and "ESTOI" not in text


def test_run_metrics_with_estoi_adds_a_column(tmp_path, monkeypatch, capsys):
    """estoi=True: a fourth value per row (here from the restatement standing in for the device pass), an ESTOI row in the
    table, statistics [groups, 4, 3]; the first three values are those of the default call."""
    from vaenmf import metrics as vm, run_metrics
    files, proc, out = _subset_tree(tmp_path)
    seen = {}

    def stoi_numpy(clean, proc_sig, counts, fs, extended=True):
        seen["args"] = (list(counts), fs, extended)
        off = np.concatenate([[0], np.cumsum(counts)])
        c, p = clean.numpy(), proc_sig.numpy()
        return np.array([sc.score(c[off[u]:off[u + 1]], p[off[u]:off[u + 1]], fs, extended)["d"] for u in range(len(counts))])

    monkeypatch.setattr(vm, "gram3_batch", _gram3_numpy)
    monkeypatch.setattr(vm, "stoi_batch", stoi_numpy)
    base = run_metrics.compute_metrics(files, proc, out, device="cpu")
    all_metrics, st = run_metrics.main(files, proc, out, [-5.0, 0.0, 0.0], device="cpu", estoi=True)
    text = capsys.readouterr().out
    assert seen["args"][1:] == (16000, True)
    assert [r[:3] for r in all_metrics] == base and all(len(r) == 4 and 0.0 < r[3] < 1.0 for r in all_metrics)
    assert st.shape == (3, 4, 3) and text.count("ESTOI") == 3            # overall and the two input SNRs


def test_statistics_carry_a_fourth_column():
    """sufficient_stats / allreduce_stats / stats_table with [U, 4]: the first three columns as without the fourth, the
    fourth in the same form; sums over shards equal the whole."""
    from vaenmf import metrics as vm
    from vaenmf.pipeline import allreduce_stats
    rng = np.random.default_rng(5)
    vals = rng.normal(3.0, 2.0, (40, 4))
    vals[:, 3] = rng.uniform(0.2, 0.9, 40)
    snr = rng.choice([-5.0, 0.0, 5.0], 40)
    st4 = vm.sufficient_stats(vals, snr)
    st3 = vm.sufficient_stats(vals[:, :3], snr)
    assert st4.shape == (4, 4, 3) and st3.shape == (4, 3, 3) and np.array_equal(st4[:, :3], st3)
    assert st4[0, 3, 0] == 40 and abs(st4[0, 3, 1] - vals[:, 3].sum()) < 1e-12
    parts = vm.sufficient_stats(vals[:15], snr[:15]) + vm.sufficient_stats(vals[15:], snr[15:])
    assert np.allclose(parts, st4, rtol=1e-12, atol=1e-12)
    assert np.array_equal(allreduce_stats(st4, "cpu"), st4)
    tab4, tab3 = vm.stats_table(st4), vm.stats_table(st3)
    assert all(tab4[k] == v for k, v in tab3.items()) and len(tab4) == len(tab3) + 4
    m, h, n = tab4[("all", "ESTOI")]
    rm, rh = vm.mean_confidence_interval(vals[:, 3])
    assert n == 40 and abs(m - rm) <= 1e-3 and abs(h - rh) <= 1e-3
    assert vm.METRIC_KEYS == ("SI-SDR", "SI-SIR", "SI-SAR") and vm.METRIC_KEYS_ESTOI[3] == "ESTOI"
