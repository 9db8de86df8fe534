"""Stft: short-time analysis and windowed overlap-add synthesis on the packed real layout of Clrfft, and the two
conversions between that layout and one-sided spectra."""
import numpy as np

from ._base import _Object, _data, _pkg, _row_view, _stream_of
from ._lib import check


class Stft(_Object):
    """Short-time transforms on the packed real layout of Clrfft (extension, clfa_stft in clfft_amd.h).

    fwd=True: analyze() frames (channels, samples) float32 rows (frame f = window * x[f*hop : f*hop + size], no
    padding) into (channels, F, size/2) complex64 spectra, each what Clrfft(size, True) returns for that frame.
    fwd=False: synthesize() runs Clrfft(size, False) on every frame, multiplies by the window and overlap-adds the frames
    into rows of (F - 1) * hop + size floats, optionally divided by the window envelope sum_f w^2.
    Like the other plans the constructor does not raise: get_error() / get_log() report a failed setup."""
    _abi = "clfa_stft_"

    def __init__(self, device_id, size, hop, window=None, fwd=True):
        self.size, self.hop, self.forward = int(size), int(hop), bool(fwd)
        self.M = self.size // 2
        if window is not None:
            if hasattr(window, "detach"):
                window = window.detach().cpu().numpy()
            window = np.ascontiguousarray(window, dtype=np.float32).reshape(-1)
            if window.size != self.size:
                raise ValueError("window must hold size = %d floats" % self.size)
        self._win = window
        self._create(_pkg.lib().clfa_stft_create, int(device_id), self.size, self.hop, _data(window), int(self.forward))

    def frames(self, samples):
        """F = 0 if samples < size else 1 + (samples - size) // hop"""
        return self._get("frames", int(samples))

    def samples(self, frames):
        """L = (frames - 1) * hop + size (0 for no frames)"""
        return self._get("samples", int(frames))

    def analyze(self, x):
        """host: float32 (channels, samples) or (samples,) -> complex64 (channels, F, size/2) (leading axis kept)"""
        x = np.ascontiguousarray(x, dtype=np.float32)
        x2 = x.reshape(1, -1) if x.ndim == 1 else x
        F = self.frames(x2.shape[1])
        out = np.zeros((x2.shape[0], F, self.M), np.complex64)
        check(_pkg.lib().clfa_stft_analyze(self._h, x2.ctypes.data, x2.shape[1], x2.shape[1], x2.shape[0], out.ctypes.data),
              "Stft.analyze")
        return out[0] if x.ndim == 1 else out

    def synthesize(self, spec, normalize=False):
        """host: complex64 (channels, F, size/2) or (F, size/2) -> float32 (channels, (F - 1) * hop + size)"""
        spec = np.ascontiguousarray(spec, dtype=np.complex64)
        s3 = spec.reshape((1,) + spec.shape) if spec.ndim == 2 else spec
        if s3.ndim != 3 or s3.shape[2] != self.M:
            raise ValueError("spectra must be (channels, F, %d)" % self.M)
        L = self.samples(s3.shape[1])
        out = np.zeros((s3.shape[0], L), np.float32)
        check(_pkg.lib().clfa_stft_synthesize(self._h, s3.ctypes.data, s3.shape[1], s3.shape[0], out.ctypes.data, L,
                                         int(bool(normalize))), "Stft.synthesize")
        return out[0] if spec.ndim == 2 else out

    def analyze_device(self, signal, out, stream=None):
        """torch: signal (channels, samples) float32 (row stride taken from the tensor: padded rows work) ->
        out (channels, F, size/2) complex64, contiguous; asynchronous on `stream` (default: the current stream)"""
        p, rows, n, stride = _row_view(signal, "signal")
        if not out.is_contiguous():
            raise ValueError("spectra tensor must be contiguous")
        return _pkg.lib().clfa_stft_analyze_dev(self._h, p, stride, n, rows, out.data_ptr(), _stream_of(signal, stream))

    def synthesize_device(self, spectra, out, normalize=False, stream=None):
        """torch: spectra (channels, F, size/2) complex64, contiguous -> out (channels, >= (F - 1) * hop + size) float32,
        row stride from the tensor; asynchronous on `stream`"""
        if not spectra.is_contiguous():
            raise ValueError("spectra tensor must be contiguous")
        s3 = spectra if spectra.dim() == 3 else spectra.unsqueeze(0)
        p, rows, _, stride = _row_view(out, "signal")
        if rows != s3.shape[0]:
            raise ValueError("out has %d rows for %d channels" % (rows, s3.shape[0]))
        return _pkg.lib().clfa_stft_synthesize_dev(self._h, spectra.data_ptr(), s3.shape[1], s3.shape[0], p, stride,
                                              int(bool(normalize)), _stream_of(out, stream))


def packed_to_onesided(spec):
    """Clrfft's packed spectra (..., M) -> the M + 1 bins of np.fft.rfft / torch.stft(onesided) (numpy or torch):
    X[0] = size Re P[0], X[M] = size Im P[0], X[M/2] = (size/2) conj(P[M/2]), X[k] = (size/2) P[k] otherwise."""
    M = spec.shape[-1]
    size = 2 * M
    if hasattr(spec, "clone"):
        import torch
        X = torch.cat([spec * (size / 2), spec[..., :1].imag.to(spec.dtype) * size], dim=-1)
    else:
        X = np.concatenate([spec * (size / 2), (spec[..., :1].imag * size).astype(spec.dtype)], axis=-1)
    X[..., 0] = spec[..., 0].real * size
    X[..., M // 2] = spec[..., M // 2].conj() * (size / 2)
    return X


def onesided_to_packed(X):
    """the inverse of packed_to_onesided: (..., M + 1) one-sided bins -> (..., M) packed (Im X[0], Im X[M] dropped)"""
    M = X.shape[-1] - 1
    size = 2 * M
    P = X[..., :M] * (2.0 / size)
    if hasattr(P, "clone"):
        P = P.clone()
    else:
        P = P.copy()
    P[..., 0] = (X[..., 0].real + 1j * X[..., M].real) / size
    P[..., M // 2] = X[..., M // 2].conj() * (2.0 / size)
    return P
