#!/usr/bin/env python3
"""What the reference's own processed utterances say about its two mixing recipes (build container only; numbers, no code).

/root/reference/data/subset/processed/CSR-1-WSJ-0/WAV/wsj0/{si_tr_s/011, si_dt_05/050, si_et_05/440} holds nine utterances x
{_s, _n, _x}.wav, PCM-16: the test set written by scripts/create_test_set.py:74-114 (joint normalisation by the peak of
speech, noise and mixture), train and validation by scripts/create_noisy_train_set.py:216-262 (speech at peak 1, no joint
normalisation).  tests/golden/mix_recipe_ref.npz keeps, per utterance in the order train, validation, test:

  rel, subset         path relative to the dataset root, 'train' / 'validation' / 'test'
  length              samples
  sum_s2, sum_n2      exact int64 sums of the squared int16 samples of _s and _n
  peak_s/_n/_x        largest |int16| of each file
  x_off               samples where |x - (s + n)| exceeds 1 LSB
  snr_bound_db        one standard deviation of what the int16 rounding of the written files does to
                      10 log10(sum_s2 / sum_n2) (rounding_bound_db below); the test allows four of them
  snr_db_test/_validation   the recorded per-utterance SNRs (si_et_05_snr_db.p, si_dt_05_snr_db.p; there is none for train)

Usage: python tests/golden/make_mix_recipe_ref.py
"""
import os

import numpy as np

from extract_ref_pickles import read_plain_pickle
from make_processed_subset import read_wav_int16

HERE = os.path.dirname(os.path.abspath(__file__))
PROC = "/root/reference/data/subset/processed/"
SETS = [("train", "CSR-1-WSJ-0/WAV/wsj0/si_tr_s/011/", ["011a010a", "011a010b", "011a010c"]),
        ("validation", "CSR-1-WSJ-0/WAV/wsj0/si_dt_05/050/", ["050a050a", "050a050b", "050a050c"]),
        ("test", "CSR-1-WSJ-0/WAV/wsj0/si_et_05/440/", ["440c020a", "440c020b", "440c020c"])]


def rounding_bound_db(T, sum_s2, sum_n2):
    """Rounding every sample v to an integer v + e, e uniform in +-1/2 LSB (variance 1/12 LSB^2), changes a sum of squares
    S = sum v^2 over T samples by sum(2 v e) + sum(e^2): the second term has the mean T/12, the first the mean 0 and the
    variance 4 S / 12 = S / 3.  Per sum: (T/12 + sqrt(S/3)) / S relative; the two sums' shares add; times 10 / ln 10 for dB."""
    rel = sum((T / 12.0 + np.sqrt(S / 3.0)) / S for S in (float(sum_s2), float(sum_n2)))
    return 10.0 / np.log(10.0) * rel


def main():
    rows = {k: [] for k in ("rel", "subset", "length", "sum_s2", "sum_n2", "peak_s", "peak_n", "peak_x", "x_off", "snr_bound_db")}
    for subset, d, names in SETS:
        for nm in names:
            s, n, x = (read_wav_int16(PROC + d + nm + "_%s.wav" % k)[0].astype(np.int64) for k in "snx")
            assert len(s) == len(n) == len(x)
            rows["rel"].append(d + nm + ".wav"); rows["subset"].append(subset); rows["length"].append(len(s))
            rows["sum_s2"].append(int(np.sum(s * s))); rows["sum_n2"].append(int(np.sum(n * n)))
            rows["peak_s"].append(int(np.abs(s).max())); rows["peak_n"].append(int(np.abs(n).max())); rows["peak_x"].append(int(np.abs(x).max()))
            rows["x_off"].append(int(np.sum(np.abs(x - (s + n)) > 1)))
            rows["snr_bound_db"].append(rounding_bound_db(len(s), rows["sum_s2"][-1], rows["sum_n2"][-1]))
    out = {k: np.array(v) for k, v in rows.items()}
    for tag, sub in (("test", "si_et_05"), ("validation", "si_dt_05")):
        out["snr_db_" + tag] = np.asarray(read_plain_pickle(PROC + "CSR-1-WSJ-0/%s_snr_db.p" % sub), dtype=np.float64)
    np.savez(os.path.join(HERE, "mix_recipe_ref.npz"), **out)
    for i in range(9):
        print(out["subset"][i], out["rel"][i].split("/")[-1], out["length"][i], "peaks", out["peak_s"][i], out["peak_n"][i], out["peak_x"][i],
              "x_off", out["x_off"][i], "snr %.6f dB" % (10 * np.log10(out["sum_s2"][i] / out["sum_n2"][i])), "bound %.2e dB" % out["snr_bound_db"][i])
    print("recorded:", out["snr_db_test"], out["snr_db_validation"])


if __name__ == "__main__":
    main()
