"""stft / istft with the reference's signatures and librosa's semantics (python/processing/stft.py:16-24,
66-73) running on the GPU (vaenmf_stft_batch_ex / vaenmf_istft_batch_ex) for any n_fft in [16, 4096], plus
batched device-resident variants used by the pipeline."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from .engine import _ptr, _stream


NFFT_MIN, NFFT_MAX = 16, 4096
_PAD_MODES = {"reflect": _lib.PAD_REFLECT, "constant": _lib.PAD_CONSTANT}


def _raise_from_lib():
    msg = lib().vaenmf_last_error().decode()
    if "not an integer" in msg or "shorter than n_fft" in msg:
        raise ValueError(msg)
    raise NotImplementedError(msg)


def frame_geometry(n_samples, fs, wlen_sec, hop_percent, center=True):
    """(nfft, hop, n_frames, padded_len); raises ValueError like stft.py:37-38 (and when center=False leaves
    fewer than n_fft samples), NotImplementedError for n_fft outside [16, 4096]."""
    nfft, hop, nfr, npad = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    rc = lib().vaenmf_stft_geometry(int(n_samples), float(fs), float(wlen_sec), float(hop_percent), int(bool(center)),
                                    C.byref(nfft), C.byref(hop), C.byref(nfr), C.byref(npad))
    if rc != 0:
        _raise_from_lib()
    return nfft.value, hop.value, nfr.value, npad.value


_TABLES = {}


def _remember(key, tab, limit=16):
    if len(_TABLES) >= limit:
        _TABLES.pop(next(iter(_TABLES)))
    _TABLES[key] = tab


def _check_nfft(nfft):
    if not NFFT_MIN <= nfft <= NFFT_MAX:
        raise NotImplementedError("n_fft=%d: this build takes window lengths in [%d, %d]" % (nfft, NFFT_MIN, NFFT_MAX))


def _pad_mode(pad_mode):
    if pad_mode not in _PAD_MODES:
        raise NotImplementedError("pad_mode=%r: this build pads with 'reflect' or 'constant'" % (pad_mode,))
    return _PAD_MODES[pad_mode]


def _window(win, nfft, dev):
    """None for periodic Hann (the library's own table), else a cached device float64 tensor [nfft]: a
    scipy.signal.get_window spec with fftbins=True as librosa uses, or an array of n_fft values."""
    if isinstance(win, str) and win == "hann":
        return None
    if isinstance(win, (str, tuple)):
        key = ("win", win, nfft, str(dev))
        w = None
    else:
        w = np.asarray(win, dtype=np.float64)
        if w.shape != (nfft,):
            raise ValueError("window of shape %s, expected (%d,)" % (w.shape, nfft))
        key = ("win", w.tobytes(), str(dev))
    t = _TABLES.get(key)
    if t is None:
        if w is None:
            from scipy.signal import get_window
            w = get_window(win, nfft, fftbins=True)
        t = torch.tensor(np.ascontiguousarray(w, dtype=np.float64), device=dev)
        _remember(key, t)
    return t


def _opts(nfft, hop, center, pad_mode, window):
    return _lib.StftOpts(nfft, hop, int(bool(center)), pad_mode, None if window is None else _ptr(window))


def stft_batch(wav, sample_counts, fs, wlen_sec, hop_percent, Fs=None, device="cuda:0", win="hann", center=True,
               pad_mode="reflect", out=None):
    """wav: device float32 [sum T] (utterances concatenated).  Returns (X [NT,Fs,2], frame_counts).
    out: a callable (shape, dtype) -> dense device tensor that supplies X instead of torch.empty (as BatchEngine._empty)."""
    dev = torch.device(device)
    pm = _pad_mode(pad_mode)
    key = ("stft", tuple(int(t) for t in sample_counts), fs, wlen_sec, hop_percent, bool(center), str(dev))
    tab = _TABLES.get(key)
    if tab is None:       # index tables on the device, cached per batch shape (pageable uploads make the host wait for the GPU)
        geo = [frame_geometry(t, fs, wlen_sec, hop_percent, center) for t in sample_counts]
        fc_ = [g[2] for g in geo]
        tab = (geo[0][0], geo[0][1], fc_,
               torch.tensor(np.concatenate([[0], np.cumsum(sample_counts)]), dtype=torch.int64, device=dev),
               torch.tensor(np.concatenate([[0], np.cumsum(fc_)]), dtype=torch.int32, device=dev),
               torch.repeat_interleave(torch.arange(len(fc_), dtype=torch.int32), torch.tensor(fc_)).to(dev),
               torch.tensor([g[3] for g in geo], dtype=torch.int32, device=dev))
        _remember(key, tab)
    nfft, hop, fc, soff, foff, futt, plen = tab
    fc = list(fc)
    window = _window(win, nfft, dev)
    F = nfft // 2 + 1
    Fs = Fs or (F + 15) // 16 * 16
    NT = int(sum(fc))
    X = torch.empty(NT, Fs, 2, device=dev, dtype=torch.float32) if out is None else out((NT, Fs, 2), torch.float32)
    opts = _opts(nfft, hop, center, pm, window)
    check(lib().vaenmf_stft_batch_ex(_ptr(wav), NT, _ptr(soff), _ptr(foff), _ptr(futt), _ptr(plen), C.byref(opts), Fs,
                                     _ptr(X), _stream()))
    return X, fc


def istft_batch(S, frame_counts, sample_counts, nfft, hop, device="cuda:0", win="hann", center=True):
    """S: device [NT,Fs,2] complex64 -> device float32 [sum T] (max_len = sample_counts[u])."""
    _check_nfft(nfft)
    dev = torch.device(device)
    key = ("istft", tuple(int(t) for t in sample_counts), tuple(int(t) for t in frame_counts), str(dev))
    tab = _TABLES.get(key)
    if tab is None:
        tab = (torch.tensor(np.concatenate([[0], np.cumsum(sample_counts)]), dtype=torch.int64, device=dev),
               torch.tensor(np.concatenate([[0], np.cumsum(frame_counts)]), dtype=torch.int32, device=dev))
        _remember(key, tab)
    soff, foff = tab
    window = _window(win, nfft, dev)
    NT, Fs = S.shape[0], S.shape[1]
    work = torch.empty(NT, nfft, device=dev, dtype=torch.float32)
    out = torch.empty(int(sum(sample_counts)), device=dev, dtype=torch.float32)
    opts = _opts(nfft, hop, center, _lib.PAD_REFLECT, window)
    check(lib().vaenmf_istft_batch_ex(_ptr(S), len(frame_counts), NT, _ptr(soff), _ptr(foff), C.byref(opts), Fs, _ptr(work),
                                      _ptr(out), _stream()))
    return out


def stft(x, fs=16e3, wlen_sec=50e-3, win="hann", hop_percent=0.25, center=True, pad_mode="reflect",
         pad_at_end=True, dtype="complex64"):
    """Reference signature (stft.py:16-24).  Returns numpy complex64 (n_fft//2+1, n_frames).  win: 'hann', a
    scipy.signal.get_window spec or an array of n_fft values; pad_mode 'reflect' or 'constant'."""
    if not pad_at_end:
        raise NotImplementedError("pad_at_end=False: the reference's stft() leaves its input unbound then (stft.py:48-55)")
    _pad_mode(pad_mode)
    x = np.asarray(x)
    nfft = frame_geometry(len(x), fs, wlen_sec, hop_percent, center)[0]
    wav = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    X, fc = stft_batch(wav, [len(x)], fs, wlen_sec, hop_percent, win=win, center=center, pad_mode=pad_mode)
    F = nfft // 2 + 1
    Xc = np.ascontiguousarray(X[:, :F].cpu().numpy()).view(np.complex64).reshape(fc[0], F)
    return Xc.T.astype(dtype)


def istft(Sxx, fs=16000, wlen_sec=50e-3, win="hann", hop_percent=0.25, center=True, dtype="float32", max_len=None):
    """Reference signature (stft.py:66-73).  Sxx numpy complex (F, n_frames).  Without max_len the output has
    librosa's length: hop (n_frames-1) with center, n_fft + hop (n_frames-1) without."""
    if wlen_sec * fs != int(wlen_sec * fs):
        raise ValueError("wlen_sample of iSTFT is not an integer.")
    nfft = int(wlen_sec * fs)
    hop = int(hop_percent * nfft)
    _check_nfft(nfft)
    if nfft % 2:
        # librosa infers n_fft = 2 (F - 1) from the spectrogram and rejects win_length = n_fft + 1 (stft.py:92-98)
        raise ValueError("istft: odd window length %d; librosa infers n_fft = %d from the %d bins and rejects "
                         "win_length > n_fft" % (nfft, nfft - 1, nfft // 2 + 1))
    F, nfr = Sxx.shape
    Fs = (F + 15) // 16 * 16
    S = np.zeros((nfr, Fs), np.complex64)
    S[:, :F] = np.asarray(Sxx).T
    T = int(max_len) if max_len else (hop * (nfr - 1) if center else nfft + hop * (nfr - 1))
    Sd = torch.from_numpy(S.view(np.float32).reshape(nfr, Fs, 2)).cuda()
    out = istft_batch(Sd, [nfr], [T], nfft, hop, win=win, center=center)
    return out.cpu().numpy().astype(dtype)
