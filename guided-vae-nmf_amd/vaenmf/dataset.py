"""Noisy data sets on the GPU: the build's counterpart of the reference's scripts/create_test_set.py and
scripts/create_noisy_train_set.py (csrc/dataset.hip; include/vaenmf.h states the arithmetic).

  plan_mixes      the random draws of the sequential scripts: noise type, SNR and noise start per file (host only)
  mix_batch       speech + noise at an SNR for a ragged batch of device signals (vaenmf_mix_batch): float64 arithmetic, one
                  rounding to float32, the same bits for an utterance in any batch
  FeatureMoments  per-bin running sums of a power spectrogram in float64 (vaenmf_feature_moments) and the mean / empirical
                  std the M2 classifier normalises with (trainset_mean.npy / trainset_std.npy)
  make_test_set   <utt>_s.wav, _n.wav, _x.wav and <set>_snr_db.p: the tree driver.evaluate and run_metrics read
  make_train_set  |STFT(mixture)|^2 frames, IBM / VAD / ideal-Wiener labels from the clean STFT, mean and std

There is no CPU fallback: everything but plan_mixes and FeatureMoments.mean_std needs the HIP library and a GPU."""
import collections
import os
import pickle

import numpy as np
import torch

from . import wavio
from ._lib import check, lib
from .engine import _ptr, _stream

STATS = ("p", "Es", "En", "k", "m")                      # columns of the stats mix_batch returns
NOISE_TYPES = {"train": ["domestic", "nature", "office", "transportation"],        # create_noisy_train_set.py:161-164
               "validation": ["nature", "office", "public", "transportation"],
               "test": ["cafe", "home", "street", "car"]}                           # create_test_set.py:126
_SET_DIR = {"train": "si_tr_s", "validation": "si_dt_05", "test": "si_et_05"}      # csr1_wjs0_dataset.py:79-88
LABELS = ("noisy_labels", "noisy_vad_labels", "noisy_wiener_labels")

TrainSet = collections.namedtuple("TrainSet", "X Y mean std snr_db frame_counts")


def plan_mixes(speech_lengths, noise_lengths, noise_types, snrs, seed=0):
    """The draws of the reference's sequential script, in its order: np.random.seed(seed), randint(len(noise_types),
    size=n), randint(len(snrs), size=n) (create_noisy_train_set.py:167-170, create_test_set.py:125-130), then per file in
    list order randint(len(noise) - len(speech)) (demand_database.py:117-126: noise_segment).
    speech_lengths: samples per file AFTER the cut at its start; noise_lengths: {noise type: samples} or a list in the order
    of noise_types.  Returns (noise_index, snr_db, start): int64 array, list of floats, int64 array.  ValueError when the
    noise recording drawn for a file is not longer than its speech.  Works on a RandomState of its own: numpy's global
    generator is left alone."""
    n = len(speech_lengths)
    lengths = [int(noise_lengths[t]) for t in noise_types] if isinstance(noise_lengths, dict) else [int(v) for v in noise_lengths]
    if len(lengths) != len(noise_types):
        raise ValueError("%d noise lengths for %d noise types" % (len(lengths), len(noise_types)))
    rs = np.random.RandomState(seed)                     # np.random.seed(seed) + np.random.randint draw the same numbers
    noise_index = rs.randint(len(noise_types), size=n)
    snr_index = rs.randint(len(snrs), size=n)
    start = np.empty(n, np.int64)
    for i in range(n):
        room = lengths[noise_index[i]] - int(speech_lengths[i])
        if room <= 0:
            raise ValueError("file %d: noise %r has %d samples, the speech %d: the noise must be longer"
                             % (i, noise_types[noise_index[i]], lengths[noise_index[i]], int(speech_lengths[i])))
        start[i] = rs.randint(room)
    return noise_index.astype(np.int64), [float(snrs[j]) for j in snr_index], start


def snr_factor(snr_db):
    """10^(-snr_db / 10) in float64: np.power(10, -snr_dB / 10) of create_test_set.py:95."""
    return float(np.power(10.0, -np.float64(snr_db) / 10.0))


def _per_utt(v, n, dtype, name):
    a = np.asarray(v, dtype=dtype)
    if a.ndim == 0:
        a = np.full(n, a, dtype)
    if a.shape != (n,):
        raise ValueError("%s: one value or one per utterance (%d), got shape %s" % (name, n, a.shape))
    return np.ascontiguousarray(a)


def mix_batch(speech, sample_counts, noise, starts, snr_db, cut=0, joint_norm=True, out=None):
    """speech: device float32 [sum T], utterances concatenated; noise: device float32 [L], ONE buffer for the batch; starts:
    first noise sample per utterance; snr_db, cut: one value or one per utterance (cut: samples dropped at the start of the
    speech, the reference's int(0.1 fs)).  joint_norm=True is the test-set recipe (s, n, x divided by their joint peak),
    False the train-set recipe.  Returns (s, n, x, counts_out, stats): device float32 [sum T'] each, T' = T - cut, and
    stats as a host float64 array [U][5] with the columns STATS, after one synchronisation.  x goes straight into
    Reconstructor.enhance(x, counts_out).
    ValueError for what the library refuses (an utterance without samples after the cut, a noise segment that leaves the
    buffer) and for an utterance that cannot be mixed: silent speech or a silent noise segment (the message names it).
    out: a callable (shape, dtype) -> dense device tensor that supplies s, n, x, the stats and the work buffer."""
    U = len(sample_counts)
    if speech.dtype != torch.float32 or speech.dim() != 1 or speech.shape[0] != int(sum(sample_counts)):
        raise ValueError("speech must be float32 [sum of sample_counts = %d], got %s %s" % (int(sum(sample_counts)), speech.dtype, tuple(speech.shape)))
    if noise.dtype != torch.float32 or noise.dim() != 1 or noise.device != speech.device:
        raise ValueError("noise must be a float32 vector on the device of speech, got %s %s on %s" % (noise.dtype, tuple(noise.shape), noise.device))
    alloc = out if out is not None else (lambda shape, dtype: torch.empty(shape, dtype=dtype, device=speech.device))
    cuts = _per_utt(cut, U, np.int64, "cut")
    b = _per_utt(starts, U, np.int64, "starts")
    f = np.array([snr_factor(v) for v in _per_utt(snr_db, U, np.float64, "snr_db")], np.float64)
    ioff = np.concatenate([[0], np.cumsum(sample_counts, dtype=np.int64)]).astype(np.int64)
    counts_out = [int(t) - int(c) for t, c in zip(sample_counts, cuts)]
    ooff = np.concatenate([[0], np.cumsum(counts_out, dtype=np.int64)]).astype(np.int64)
    if U == 0:
        e = torch.empty(0, dtype=torch.float32, device=speech.device)
        return e, e.clone(), e.clone(), [], np.zeros((0, 5))
    if min(counts_out) < 1:
        u = int(np.argmin(counts_out))
        raise ValueError("utterance %d: %d samples with the first %d cut leave none" % (u, sample_counts[u], cuts[u]))
    nbytes = lib().vaenmf_mix_work_bytes(U)
    if nbytes < 0:
        raise ValueError(lib().vaenmf_last_error().decode())
    total = int(ooff[-1])
    s, n, x = (alloc((total,), torch.float32) for _ in range(3))
    stats = alloc((U, 5), torch.float64)
    work = alloc((int(nbytes),), torch.uint8)
    rc = lib().vaenmf_mix_batch(_ptr(speech), U, ioff.ctypes.data, cuts.ctypes.data, _ptr(noise), int(noise.shape[0]), b.ctypes.data,
                                f.ctypes.data, int(bool(joint_norm)), ooff.ctypes.data, _ptr(s), _ptr(n), _ptr(x), _ptr(stats), _ptr(work),
                                int(nbytes), _stream())
    if rc == -1:
        raise ValueError(lib().vaenmf_last_error().decode())
    check(rc)
    st = stats.cpu().numpy()                             # the one synchronisation
    bad = np.nonzero(st[:, 3] == 0.0)[0]
    if len(bad):
        u = int(bad[0])
        raise ValueError("utterance %d cannot be mixed: %s" % (u, "its speech is silent after the cut" if st[u, 0] == 0.0 else
                                                              "its noise segment [%d, %d) is silent" % (b[u], b[u] + counts_out[u])))
    return s, n, x, counts_out, st


def moments_mean_std(S1, S2, n):
    """mean = S1 / n and the reference's empirical std sqrt((S2 - n mean^2) / (n - 1)) (create_noisy_train_set.py:313-319)
    with the radicand clamped at zero, in float64; float32 (F, 1) arrays as the reference stores them (:329-330)."""
    n = int(n)
    if n < 2:
        raise ValueError("mean and std need at least 2 frames, got %d" % n)
    S1, S2 = np.asarray(S1, np.float64), np.asarray(S2, np.float64)
    mean = S1 / n
    std = np.sqrt(np.maximum(0.0, (S2 - n * mean ** 2) / (n - 1)))
    return mean.astype(np.float32)[:, None], std.astype(np.float32)[:, None]


class FeatureMoments:
    """Running per-bin sums S1 = sum P, S2 = sum P^2 of power-spectrogram frames, kept in float64 on the device (the
    reference keeps them in float32, create_noisy_train_set.py:211, 302-303), streamed batch by batch."""

    def __init__(self, F, device="cuda:0"):
        self.F, self.n, self.device = int(F), 0, torch.device(device)
        self.S1 = self.S2 = None

    def add(self, P, n_frames=None):
        """P: device float32 [rows][ld], frame-major, ld >= F (columns F.. may hold anything); the first n_frames rows count
        (default: all)."""
        if P.dtype != torch.float32 or P.dim() != 2 or not P.is_contiguous() or P.shape[1] < self.F:
            raise ValueError("P must be a dense float32 [frames][ld >= %d], got %s %s" % (self.F, P.dtype, tuple(P.shape)))
        n_frames = P.shape[0] if n_frames is None else int(n_frames)
        if not 0 <= n_frames <= P.shape[0]:
            raise ValueError("n_frames=%d outside [0, %d]" % (n_frames, P.shape[0]))
        if self.S1 is None:
            self.S1 = torch.empty(self.F, dtype=torch.float64, device=P.device)
            self.S2 = torch.empty(self.F, dtype=torch.float64, device=P.device)
        nbytes = lib().vaenmf_moments_work_bytes(n_frames, self.F)
        work = torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=P.device)
        check(lib().vaenmf_feature_moments(_ptr(P), n_frames, self.F, int(P.shape[1]), int(self.n > 0), _ptr(self.S1), _ptr(self.S2),
                                           _ptr(work), int(nbytes), _stream()))
        self.n += n_frames
        return self

    def sums(self):
        """(S1, S2, n): host float64 arrays [F] and the frame count."""
        if self.S1 is None:
            return np.zeros(self.F), np.zeros(self.F), 0
        return self.S1.cpu().numpy(), self.S2.cpu().numpy(), self.n

    def mean_std(self):
        """float32 (F, 1) mean and std (moments_mean_std); ValueError with fewer than 2 frames."""
        return moments_mean_std(*self.sums())


# ---------------------------------------------------------------------------------------------------------------------
# the two builders
# ---------------------------------------------------------------------------------------------------------------------
def _noise_bank(noise_audios, noise_types, fs, device):
    """One device float32 buffer with the recordings of noise_types one behind the other.  A recording is a wav path, an
    array at fs, or (array, its rate); one at another rate is resampled on the device.  -> (buffer, first sample per type,
    samples per type)."""
    from .resample import resample_batch
    parts = []
    for t in noise_types:
        a = noise_audios[t]
        rate = fs
        if isinstance(a, (str, os.PathLike)):
            a, rate = wavio.read(a)
        elif isinstance(a, tuple):
            a, rate = a
        w = torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=np.float32)).to(device)
        if w.dim() != 1:
            raise ValueError("noise %r: one channel expected, got shape %s" % (t, tuple(w.shape)))
        if int(rate) != int(fs):
            w, _ = resample_batch(w, [int(w.shape[0])], int(rate), int(fs), device=device)
        parts.append(w)
    lengths = [int(p.shape[0]) for p in parts]
    base = np.concatenate([[0], np.cumsum(lengths)])[:-1].astype(np.int64)
    return torch.cat(parts), base, lengths


def _speech_lengths(file_paths, input_speech_dir, fs):
    out = []
    for fp in file_paths:
        x, fs_x = wavio.read(input_speech_dir + fp)
        if fs_x != fs:
            raise ValueError("Unexpected sampling rate")                 # create_test_set.py:86-87
        out.append(len(x))
    return out


def _mixed_batches(file_paths, input_speech_dir, noise_audios, dataset_type, snrs, noise_types, fs, batch_size, seed, joint_norm, device):
    """Yields (files, s, n, x, counts, snr_db of the batch) with the draws of plan_mixes over the whole list."""
    noise_types = list(NOISE_TYPES[dataset_type] if noise_types is None else noise_types)
    cut = int(0.1 * fs)                                                   # create_test_set.py:81
    lengths = _speech_lengths(file_paths, input_speech_dir, fs)
    for fp, t in zip(file_paths, lengths):
        if t - cut < 1:
            raise ValueError("%s: %d samples, the first %d are cut" % (fp, t, cut))
    bank, base, nlen = _noise_bank(noise_audios, noise_types, fs, device)
    noise_index, snr_db, start = plan_mixes([t - cut for t in lengths], nlen, noise_types, snrs, seed)
    for b0 in range(0, len(file_paths), batch_size):
        files = list(file_paths[b0:b0 + batch_size])
        wavs = [wavio.read(input_speech_dir + fp)[0] for fp in files]
        speech = torch.from_numpy(np.concatenate(wavs).astype(np.float32)).to(device)
        sl = slice(b0, b0 + len(files))
        try:
            s, n, x, counts, _ = mix_batch(speech, [len(w) for w in wavs], bank, base[noise_index[sl]] + start[sl], snr_db[sl], cut, joint_norm)
        except ValueError as e:
            raise ValueError("batch of %s ..: %s" % (files[0], e)) from None
        yield files, s, n, x, counts, snr_db[sl]


def _write_wavs(files, output_wav_dir, s, n, x, counts, fs):
    parts = [torch.split(t, counts) for t in (s.cpu(), n.cpu(), x.cpu())]
    for i, fp in enumerate(files):
        out = os.path.splitext(output_wav_dir + fp)[0]                    # create_test_set.py:105-114
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        for k, suffix in enumerate(("_s.wav", "_n.wav", "_x.wav")):
            wavio.write(out + suffix, parts[k][i].numpy(), fs)


def _write_snr(all_snr_db, output_wav_dir, dataset_type):
    """write_dataset(all_snr_dB, output_wav_dir, dataset_type, 'snr_db'), csr1_wjs0_dataset.py:59-93."""
    os.makedirs(output_wav_dir + "CSR-1-WSJ-0/", exist_ok=True)
    path = output_wav_dir + "CSR-1-WSJ-0/" + _SET_DIR[dataset_type] + "_snr_db.p"
    with open(path, "wb") as f:
        pickle.dump([float(v) for v in all_snr_db], f, protocol=4)
    return path


def make_test_set(file_paths, input_speech_dir, noise_audios, output_wav_dir, dataset_type="test", snrs=(-5.0, 0.0, 5.0),
                  noise_types=None, fs=16000, batch_size=64, seed=0, device="cuda:0"):
    """scripts/create_test_set.py:74-161.  file_paths relative to input_speech_dir (driver.speech_list), read with wavio.read
    (a file at another rate than fs is refused, as the reference does); noise_audios {type: wav path | array at fs | (array,
    rate)}, noise_types default to the reference's list for dataset_type.  Per file the first int(0.1 fs) samples are cut, the
    speech is scaled to peak 1, mixed with its noise segment at its SNR and the three signals are divided by their joint
    peak (mix_batch, joint_norm=True).  Writes <output_wav_dir><file>_s.wav, _n.wav, _x.wav and
    <output_wav_dir>CSR-1-WSJ-0/<set>_snr_db.p (a pickled list of floats, protocol 4).  Both directories end with '/', as the
    reference's do.  Returns the SNR list."""
    all_snr = []
    for files, s, n, x, counts, snr in _mixed_batches(file_paths, input_speech_dir, noise_audios, dataset_type, snrs, noise_types, fs,
                                                      batch_size, seed, True, device):
        _write_wavs(files, output_wav_dir, s, n, x, counts, fs)
        all_snr += snr
    _write_snr(all_snr, output_wav_dir, dataset_type)
    return all_snr


def make_train_set(file_paths, input_speech_dir, noise_audios, labels="noisy_labels", dataset_type="train",
                   snrs=(-5.0, -2.5, 0.0, 2.5, 5.0), noise_types=None, fs=16000, wlen_sec=64e-3, hop_percent=0.25,
                   quantile_fraction=0.999, quantile_weight=0.999, eps=1e-8, batch_size=64, seed=0, out_dir=None,
                   output_wav_dir=None, device="cuda:0"):
    """scripts/create_noisy_train_set.py:155-334 without HDF5.  Per file: cut, peak 1, noise at the SNR, NO joint
    normalisation (mix_batch, joint_norm=False); per batch on the device one stft_batch of the mixtures, of the speech and
    (Wiener labels) of the noise, X = |STFT(mixture)|^2, labels from the clean STFT -- 'noisy_labels' clean_speech_IBM,
    'noisy_vad_labels' clean_speech_VAD, 'noisy_wiener_labels' ideal_wiener_mask -- and the running sums of X.
    Returns TrainSet(X (F, NT) float32, Y (F or 1, NT) float32, mean (F, 1), std (F, 1), snr_db, frame_counts), host arrays
    in the reference's layout.  out_dir: also writes trainset_mean.npy, trainset_std.npy and CSR-1-WSJ-0_<labels>.npz with
    X_<set>, Y_<set>, snr_db and frame_counts.  output_wav_dir: also writes the wavs and the SNR pickle, as the reference does
    for its subset (:252-262, :334)."""
    from . import stft as vstft
    from . import target as vtarget
    if labels not in LABELS:
        raise ValueError("labels must be one of %s" % (LABELS,))
    Xs, Ys, all_snr, frame_counts, mom = [], [], [], [], None
    for files, s, n, x, counts, snr in _mixed_batches(file_paths, input_speech_dir, noise_audios, dataset_type, snrs, noise_types, fs,
                                                      batch_size, seed, False, device):
        Xc, fc = vstft.stft_batch(x, counts, fs, wlen_sec, hop_percent, device=device)
        Sc, _ = vstft.stft_batch(s, counts, fs, wlen_sec, hop_percent, device=device)
        NT, Fs = Xc.shape[0], Xc.shape[1]
        F = vstft.frame_geometry(counts[0], fs, wlen_sec, hop_percent)[0] // 2 + 1
        P = torch.empty(NT, Fs, dtype=torch.float32, device=Xc.device)
        check(lib().vaenmf_power_spec(_ptr(Xc), _ptr(P), NT * Fs, _stream()))
        if labels == "noisy_wiener_labels":
            Nc, _ = vstft.stft_batch(n, counts, fs, wlen_sec, hop_percent, device=device)
            Y = torch.empty(NT, Fs, dtype=torch.float32, device=Xc.device)
            check(lib().vaenmf_wiener_mask(_ptr(Sc), _ptr(Nc), NT * Fs, float(eps), _ptr(Y), _stream()))
            Y = Y[:, :F]
        elif labels == "noisy_labels":
            Y = vtarget.lorenz_labels_batch(Sc, fc, F, "ibm", quantile_fraction, quantile_weight)
        else:
            Y = vtarget.lorenz_labels_batch(Sc, fc, F, "vad", quantile_fraction, quantile_weight)[:, None]
        mom = mom or FeatureMoments(F, device)
        mom.add(P, NT)
        Xs.append(P[:, :F].t().cpu().numpy())
        Ys.append(Y.t().cpu().numpy())
        frame_counts += list(fc)
        all_snr += snr
        if output_wav_dir is not None:
            _write_wavs(files, output_wav_dir, s, n, x, counts, fs)
    if mom is None:
        raise ValueError("no files")
    X, Y = np.ascontiguousarray(np.concatenate(Xs, 1)), np.ascontiguousarray(np.concatenate(Ys, 1))
    mean, std = mom.mean_std()
    if output_wav_dir is not None:
        _write_snr(all_snr, output_wav_dir, dataset_type)
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        np.save(os.path.join(out_dir, "trainset_mean.npy"), mean)
        np.save(os.path.join(out_dir, "trainset_std.npy"), std)
        np.savez(os.path.join(out_dir, "CSR-1-WSJ-0_%s.npz" % labels), snr_db=np.asarray(all_snr), frame_counts=np.asarray(frame_counts),
                 **{"X_" + dataset_type: X, "Y_" + dataset_type: Y})
    return TrainSet(X, Y, mean, std, all_snr, frame_counts)
