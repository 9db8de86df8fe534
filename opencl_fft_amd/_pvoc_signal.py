"""Pvoc's calls with samples on one side (pvoc_signal_host.cpp): tanal (a stored signal -> frames), adsyn (frames -> samples)."""
import numpy as np

from ._base import CL_INVALID_VALUE, _data, _is_f32, _row_view, _stream_of
from ._lib import check
from ._pvoc_calls import _PvocCalls, _dense_f32


class _PvocTanal(_PvocCalls):
    """clfa_pvoc_tanal*: a stored signal -> frames at any time points (Csound's pvstanal, mincer)."""

    def tanal_kernel_name(self):
        """ "k_pvoc_tanal" ("" for a failed object)"""
        return self._text("tanal_kernel_name")

    @staticmethod
    def stretch_starts(samples, hop, factor):
        """the starts of a time stretch by `factor` (2 = twice as long) of a signal of `samples` samples: int32
        floor(g hop / factor), computed in float64, for g = 0 .. ceil(factor samples / hop) - 1.  ValueError for a factor
        that is not positive and finite"""
        factor = float(factor)
        if not (np.isfinite(factor) and factor > 0):
            raise ValueError("factor must be positive and finite")
        n = int(np.ceil(factor * int(samples) / int(hop)))
        return np.floor(np.arange(max(n, 0), dtype=np.float64) * int(hop) / factor).astype(np.int32)

    def tanal_device(self, signal, window, starts, frames_out, stream=None):
        """torch: signal float32 (channels, samples) with unit inner stride and any row stride ((samples,) for one
        channel), window float32 (size,), starts int32 (Fout,) -> frames_out (channels, Fout, size/2 + 1, 2) float32,
        contiguous (anything else: CL_INVALID_VALUE).  Frame g of every channel is the analysis of the signal under the
        window laid at starts[g] and, for the phase difference, at starts[g] - hop; samples outside the signal are zero.
        No state is read or written.  frames_out may overlap none of the inputs.  Asynchronous on `stream`."""
        if not all(hasattr(t, "data_ptr") for t in (signal, window, starts, frames_out)):
            return CL_INVALID_VALUE
        sig = signal.unsqueeze(0) if signal.dim() == 1 and self.channels == 1 else signal
        Fout = self._frames_shape(frames_out.shape)
        if (Fout is None or not _dense_f32(frames_out, frames_out.shape) or not _dense_f32(window, (self.size,))
                or str(starts.dtype) != "torch.int32" or tuple(starts.shape) != (Fout,) or not starts.is_contiguous()
                or not _is_f32(sig) or sig.dim() != 2 or sig.shape[0] != self.channels or sig.shape[1] < 1
                or (sig.shape[1] > 1 and sig.stride(1) != 1) or (self.channels > 1 and sig.stride(0) < sig.shape[1])
                or any(t.device != frames_out.device for t in (signal, window, starts))):
            return CL_INVALID_VALUE
        samples = sig.shape[1]
        return self._get("tanal_dev", sig.data_ptr(), max(sig.stride(0), samples), samples, window.data_ptr(),
                         starts.data_ptr(), frames_out.data_ptr(), Fout, _stream_of(frames_out, stream))

    def tanal(self, signal, window, starts):
        """host form of tanal_device, blocking: float32 (channels, samples) (or (samples,) for one channel), window
        (size,), integer starts (Fout,) -> the frames float32 (.., Fout, size/2 + 1, 2)"""
        signal = np.ascontiguousarray(signal, dtype=np.float32)
        window = np.ascontiguousarray(window, dtype=np.float32)
        starts = np.ascontiguousarray(starts, dtype=np.int32).reshape(-1)
        full = self._full(signal.shape, 2)
        if len(full) != 2 or full[0] != self.channels or full[1] < 1:
            raise ValueError("signal must be (%d, samples)" % self.channels)
        if window.shape != (self.size,):
            raise ValueError("window must be (%d,)" % self.size)
        out = np.zeros(signal.shape[:-1] + (starts.size, self.M + 1, 2), np.float32)
        check(self._get("tanal", signal.ctypes.data, full[1], full[1], window.ctypes.data, starts.ctypes.data,
                        out.ctypes.data, starts.size), "Pvoc.tanal")
        return out


class _PvocAdsyn(_PvocCalls):
    """clfa_pvoc_adsyn*: frames -> samples, the oscillator bank (Csound's pvsadsyn; a state of its own)."""

    def adsyn_kernel_name(self):
        """ "k_adsyn_osc" ("" for a failed object)"""
        return self._text("adsyn_kernel_name")

    def adsyn_workspace_bytes(self):
        return self._get("adsyn_workspace_bytes")

    def adsyn_tile_bins(self):
        """oscillators per LDS tile of k_adsyn_osc (fixed)"""
        return self._fn("adsyn_tile_bins")()

    def adsyn_state(self):
        """the oscillator bank's state (blocking): (P uint64 in 2^-64 turn, W int32 in 2^-32 turn per sample, A float32),
        each (channels, size/2 + 1)"""
        shape = (self.channels, self.M + 1)
        P, W, A = np.zeros(shape, np.uint64), np.zeros(shape, np.int32), np.zeros(shape, np.float32)
        check(self._get("adsyn_read_state", P.ctypes.data, W.ctypes.data, A.ctypes.data), "Pvoc.adsyn_state")
        return P, W, A

    def adsyn_device(self, frames, out, fmod=None, first_bin=0, nbins=None, step=1, gain=1.0, stream=None):
        """torch: frames (channels, F, size/2 + 1, 2) float32, contiguous -> out (channels, n >= F * hop) float32 with
        contiguous rows (one row for one channel): frame f yields the samples [f hop, (f + 1) hop), summed over the
        oscillators of the bins first_bin + i * step, i < nbins (default: all that fit), times gain.  fmod: a frequency
        multiplier, a number or a float32 device tensor (F,); None: none.  Asynchronous on `stream`."""
        F = self._device_frames(frames)
        if F is None or not _is_f32(out):
            return CL_INVALID_VALUE
        p, rows, n, stride = _row_view(out, "out")
        prep = None if rows != self.channels or n < F * self.hop else self._device_prep(F, out.device, (fmod,))
        if prep is None:
            return CL_INVALID_VALUE
        (fmod,) = prep[1]
        first_bin, nbins, step = self._selection(first_bin, nbins, step)
        return self._get("adsyn_dev", frames.data_ptr(), F, fmod, first_bin, nbins, step, float(gain), p,
                         stride if rows > 1 else n, _stream_of(out, stream))

    def adsyn(self, frames, fmod=None, first_bin=0, nbins=None, step=1, gain=1.0):
        """host form of adsyn_device, blocking: float32 (channels, F, size/2 + 1, 2) (or (F, size/2 + 1, 2)) -> float32
        (.., F * hop)"""
        frames, F, (fmod,), out = self._host_prep(frames, (fmod,), tail=(self.hop,))
        out = out.reshape(out.shape[:-2] + (F * self.hop,))
        first_bin, nbins, step = self._selection(first_bin, nbins, step)
        check(self._get("adsyn", frames.ctypes.data, F, _data(fmod), first_bin, nbins, step, float(gain), out.ctypes.data,
                        F * self.hop), "Pvoc.adsyn")
        return out
