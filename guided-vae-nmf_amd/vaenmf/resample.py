"""Rational-ratio resampling on the GPU (vaenmf_resample_batch): scipy.signal.resample_poly(x, up, down,
window=('kaiser', beta)) with zero padding, for ragged batches, float64 taps and sums, one rounding to float32.  It stands
where the reference calls librosa.resample (python/dataset/qut_database.py, demand_database.py: preprocess_noise) and lets
audio at another rate than the model's pass through Reconstructor / MaskEnhancer / driver.evaluate."""
import ctypes as C
import numbers

import numpy as np
import torch

from ._lib import check, lib
from .engine import _ptr, _stream

MAX_RATIO = 1024
_NOT_SUPPORTED = -3


def _rate(fs, name):
    if isinstance(fs, bool) or not isinstance(fs, (numbers.Real, np.integer, np.floating)) or fs != int(fs) or fs <= 0:
        raise ValueError("%s=%r: sampling rates are positive integers in Hz" % (name, fs))
    return int(fs)


def ratio(fs_in, fs_out):
    """(up, down) = (fs_out, fs_in) / gcd; ValueError for a rate that is no positive integer, NotImplementedError when up
    or down exceeds 1024."""
    up, down = C.c_int32(), C.c_int32()
    rc = lib().vaenmf_resample_ratio(_rate(fs_in, "fs_in"), _rate(fs_out, "fs_out"), C.byref(up), C.byref(down))
    if rc == _NOT_SUPPORTED:
        raise NotImplementedError(lib().vaenmf_last_error().decode())
    check(rc)
    return up.value, down.value


def length(n_in, up, down):
    """ceil(n_in up / down): the samples n_in samples become."""
    n = lib().vaenmf_resample_length(int(n_in), int(up), int(down))
    if n < 0:
        raise ValueError(lib().vaenmf_last_error().decode())
    return n


def taps(up, down, zeros=10, beta=5.0):
    """The 2 zeros max(up, down) + 1 filter taps (numpy float64) the library uses for up / down as given."""
    h = np.empty(2 * int(zeros) * max(int(up), int(down)) + 1, np.float64)
    rc = lib().vaenmf_resample_taps(int(up), int(down), int(zeros), float(beta), h.ctypes.data)
    if rc == _NOT_SUPPORTED:
        raise NotImplementedError(lib().vaenmf_last_error().decode())
    check(rc)
    return h


_OFFSETS = {}


def _offsets(sample_counts, up, down):
    """(in_offsets, out_offsets, counts_out) of a batch shape: host int64 arrays, kept for the shapes that repeat."""
    key = (tuple(int(t) for t in sample_counts), up, down)
    tab = _OFFSETS.get(key)
    if tab is None:
        counts_out = [length(t, up, down) for t in key[0]]
        tab = (np.concatenate([[0], np.cumsum(key[0], dtype=np.int64)]).astype(np.int64),
               np.concatenate([[0], np.cumsum(counts_out, dtype=np.int64)]).astype(np.int64), counts_out)
        if len(_OFFSETS) >= 16:
            _OFFSETS.pop(next(iter(_OFFSETS)))
        _OFFSETS[key] = tab
    return tab


def resample_batch(wav, sample_counts, fs_in, fs_out, device="cuda:0", zeros=10, beta=5.0, out=None):
    """wav: device float32 [sum T] (utterances concatenated, as stft_batch takes them) at fs_in Hz.  Returns (wav_out,
    counts_out): device float32 [sum T'] at fs_out Hz, T' = ceil(T fs_out / fs_in) per utterance.  An utterance's result
    does not depend on the batch it sits in.  out: a callable (shape, dtype) -> dense device tensor that supplies wav_out."""
    dev = torch.device(device)
    up, down = ratio(fs_in, fs_out)
    ioff, ooff, counts_out = _offsets(sample_counts, up, down)
    if wav.dtype != torch.float32 or wav.dim() != 1 or wav.shape[0] != int(ioff[-1]):
        raise ValueError("wav must be float32 [sum of sample_counts = %d], got %s %s" % (int(ioff[-1]), wav.dtype, tuple(wav.shape)))
    n_out = int(ooff[-1])
    y = torch.empty(n_out, device=dev, dtype=torch.float32) if out is None else out((n_out,), torch.float32)
    check(lib().vaenmf_resample_batch(_ptr(wav), len(counts_out), ioff.ctypes.data, ooff.ctypes.data, up, down, int(zeros),
                                      float(beta), _ptr(y), _stream()))
    return y, list(counts_out)


def resample(x, orig_sr, target_sr, zeros=10, beta=5.0, device="cuda:0"):
    """One signal, numpy or torch, 1-D; the argument order of the reference's librosa.resample(x, orig_sr, target_sr)
    calls.  A numpy input gives a numpy array of its dtype, a tensor gives a float32 tensor on its device."""
    if isinstance(x, torch.Tensor):
        if x.dim() != 1:
            raise ValueError("resample takes one 1-D signal, got shape %s" % (tuple(x.shape),))
        y, _ = resample_batch(x.to(device=device, dtype=torch.float32).contiguous(), [x.shape[0]], orig_sr, target_sr, device, zeros, beta)
        return y.to(x.device)
    a = np.asarray(x)
    if a.ndim != 1:
        raise ValueError("resample takes one 1-D signal, got shape %s" % (a.shape,))
    wav = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    y, _ = resample_batch(wav, [len(a)], orig_sr, target_sr, device, zeros, beta)
    return y.cpu().numpy().astype(a.dtype if np.issubdtype(a.dtype, np.floating) else np.float32)


def crop_batch(wav, counts, keep):
    """The first keep[u] samples of every utterance of a concatenated batch (keep[u] <= counts[u]), concatenated."""
    if list(counts) == list(keep):
        return wav
    off = np.concatenate([[0], np.cumsum(counts)])
    return torch.cat([wav[int(off[u]):int(off[u]) + int(k)] for u, k in enumerate(keep)])
