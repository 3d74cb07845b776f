#!/usr/bin/env python3
"""The reference's ESTOI known answers (build container only; data, no code).

/root/reference/data/subset holds, for the test utterances si_et_05/440/440c020{a,b,c}, the clean signal
processed/.../<u>_s.wav, the dummy M2 model's estimate models/dummy_M2_alpha_5.0_epoch_100_vloss_466.72/.../<u>_s_est.wav
(RIFF PCM-16 mono 16 kHz) and <u>_fig.png, whose title prints the utterance's ESTOI: "STOI = 0.26", "0.60", "0.59"
(scripts/run_metrics_M2.py: stoi(s_t, s_hat_t, fs, extended=True)).  Utterance a is in metrics_dummy_m2.npz at full
length already; this writes

  tests/golden/stoi_dummy_m2.npz    {b,c}_s, {b,c}_s_est int16 at full length, names = [a, b, c], printed_estoi = the three
                                    printed values, fs = 16000

and drops c when both would not fit the size limit for a committed file.

Usage: python tests/golden/make_stoi_dummy.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = "/root/reference/data/subset/"
UTT = "CSR-1-WSJ-0/WAV/wsj0/si_et_05/440/440c020"
MODEL = "models/dummy_M2_alpha_5.0_epoch_100_vloss_466.72/"
PRINTED = {"a": 0.26, "b": 0.60, "c": 0.59}          # read off the titles of <u>_fig.png
LIMIT = 1024 * 1024


def read_wav_int16(path):
    """Minimal RIFF/WAVE PCM16 mono reader (soundfile is not installed)."""
    b = open(path, "rb").read()
    assert b[:4] == b"RIFF" and b[8:12] == b"WAVE"
    pos, fs = 12, None
    while pos < len(b):
        cid, sz = b[pos:pos + 4], int.from_bytes(b[pos + 4:pos + 8], "little")
        if cid == b"fmt ":
            assert int.from_bytes(b[pos + 8:pos + 10], "little") == 1 and int.from_bytes(b[pos + 10:pos + 12], "little") == 1
            fs = int.from_bytes(b[pos + 12:pos + 16], "little")
            assert int.from_bytes(b[pos + 22:pos + 24], "little") == 16
        if cid == b"data":
            return np.frombuffer(b[pos + 8:pos + 8 + sz], dtype="<i2").copy(), fs
        pos += 8 + sz + (sz & 1)
    raise ValueError("no data chunk")


def main():
    za = np.load(os.path.join(HERE, "metrics_dummy_m2.npz"))
    for key, path in (("a_s", ROOT + "processed/" + UTT + "a_s.wav"), ("a_s_est", ROOT + MODEL + UTT + "a_s_est.wav")):
        w, fs = read_wav_int16(path)
        assert fs == 16000 and np.array_equal(w, za[key]), key + " of metrics_dummy_m2.npz is not the reference's file"
    sig = {}
    for u in "bc":
        s, fs = read_wav_int16(ROOT + "processed/" + UTT + u + "_s.wav")
        e, fs_e = read_wav_int16(ROOT + MODEL + UTT + u + "_s_est.wav")
        assert fs == fs_e == 16000 and len(s) == len(e)
        sig[u + "_s"], sig[u + "_s_est"] = s, e
    out = os.path.join(HERE, "stoi_dummy_m2.npz")
    meta = dict(names=np.array(list("abc")), printed_estoi=np.array([PRINTED[u] for u in "abc"]), fs=16000)
    np.savez_compressed(out, **meta, **sig)
    if os.path.getsize(out) > LIMIT:
        np.savez_compressed(out, **meta, **{k: v for k, v in sig.items() if k[0] == "b"})
    z = np.load(out)
    print("stoi_dummy_m2.npz:", {k: z[k].shape for k in z.files if k[0] in "bc"}, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
