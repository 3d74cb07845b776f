"""The statistics harness: the build's counterpart of scripts/run_metrics_M1.py:63-176 (compute_metrics_utt / main)
for the metrics that are in scope -- SI-SDR, SI-SIR, SI-SAR (python/metrics.py:12-60) and, on request (estoi=True),
ESTOI (run_metrics_M2.py:117: stoi(s_t, s_hat_t, fs, extended=True)) from the batched device pass of
metrics.stoi_batch_device; PESQ / POLQA and the figures stay external (third-party packages).

  per utterance   read <processed>/<rel>_s.wav, _n.wav, _x.wav and <model dir>/<rel>_s_est.wav, the float64 Gram
                  sums of (s_est, s, n) on the device (vaenmf_gram3_batch), closed-form ratios; with estoi=True the
                  batch's ESTOI of (s, s_est) from the same device signals (vaenmf_stoi_batch)
  table           compute_stats (metrics.py:70-108): mean +- t-CI overall and per input SNR; the SNR list is what
                  read_dataset(processed_data_dir, dataset_type, 'snr_db') returns in the reference (run_metrics_M1.py:149)
"""
import os

import numpy as np
import torch

from . import wavio
from . import metrics as vmet


def compute_metrics(file_paths, processed_data_dir, model_data_dir, device="cuda:0", batch_size=64, estoi=False):
    """-> list of [si_sdr, si_sir, si_sar] per utterance, in file order (run_metrics_M1.py:63-98); estoi=True appends the
    utterance's ESTOI as a fourth value (the files of one batch must then share their sampling rate)."""
    out = []
    for b0 in range(0, len(file_paths), batch_size):
        files = file_paths[b0:b0 + batch_size]
        sig = {k: [] for k in ("s", "n", "e")}
        counts, rates = [], set()
        for fp in files:
            stem = os.path.splitext(fp)[0]
            s, fs = wavio.read(processed_data_dir + stem + "_s.wav")
            n, _ = wavio.read(processed_data_dir + stem + "_n.wav")
            e, fs_e = wavio.read(model_data_dir + stem + "_s_est.wav")
            if fs_e != fs or not (len(s) == len(n) == len(e)):
                raise ValueError("length / rate mismatch for " + fp)
            sig["s"].append(s); sig["n"].append(n); sig["e"].append(e)
            counts.append(len(s))
            rates.add(fs)
        t = lambda l: torch.from_numpy(np.concatenate(l).astype(np.float32)).to(device)
        e_dev, s_dev = t(sig["e"]), t(sig["s"])
        G = vmet.gram3_batch(e_dev, s_dev, t(sig["n"]), counts)
        r = np.stack(vmet.ratios_from_gram(G), 1)
        if estoi:
            if len(rates) != 1:
                raise ValueError("estoi=True needs one sampling rate per batch, got %s" % sorted(rates))
            r = np.concatenate([r, vmet.stoi_batch(s_dev, e_dev, counts, rates.pop(), extended=True)[:, None]], 1)
        out += [list(map(float, row)) for row in r]
    return out


def main(file_paths, processed_data_dir, model_data_dir, all_snr_db, confidence=0.95, device="cuda:0", estoi=False):
    """run_metrics_M1.py:147-176: per-utterance metrics, then the printed table; returns (all_metrics, sufficient statistics).
    estoi=True: a fourth value per utterance and an ESTOI row in every block of the table, as the reference prints it."""
    all_metrics = compute_metrics(file_paths, processed_data_dir, model_data_dir, device, estoi=estoi)
    vmet.compute_stats(metrics_keys=list(vmet.METRIC_KEYS_ESTOI if estoi else vmet.METRIC_KEYS), all_metrics=all_metrics, all_snr_db=np.asarray(all_snr_db),
                       model_data_dir=model_data_dir, confidence=confidence)
    bins = tuple(float(b) for b in np.unique(np.asarray(all_snr_db, dtype=np.float64)))
    return all_metrics, vmet.sufficient_stats(np.asarray(all_metrics), all_snr_db, snr_bins=bins)
