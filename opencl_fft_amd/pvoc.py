"""Pvoc: the phase vocoder on Stft's spectra — (amp, freq) frames both ways, and the operations on such frames."""
import numpy as np

from ._base import CL_INVALID_VALUE, _Object, _is_f32, _stream_of
from ._lib import check
from ._pvoc_frames import _PvocDemix, _PvocOps, _PvocPair, _PvocShape, _PvocTrace
from ._pvoc_rows import _PvocBank, _PvocDesc, _PvocPitch
from ._pvoc_signal import _PvocAdsyn, _PvocTanal
from ._pvoc_stream import _PvocDelay, _PvocTime


class Pvoc(_Object, _PvocOps, _PvocPair, _PvocShape, _PvocTrace, _PvocDemix, _PvocTime, _PvocDelay, _PvocDesc, _PvocBank,
           _PvocPitch, _PvocTanal, _PvocAdsyn):
    """Phase vocoder on the spectra of Stft (extension, clfa_pvoc in clfft_amd.h): analyze() reads (channels, F, size/2)
    complex64 spectra as (channels, F, size/2 + 1, 2) float32 frames of (amp, freq in Hz) per bin, synthesize() turns such
    frames back into spectra.  The object carries the last spectrum (analysis) and an integer phase per bin (synthesis)
    from call to call, so a stream may be cut into calls anywhere; reset() returns both to their start.
    adsyn() is the second way back to sound: an oscillator per bin, summed straight into samples (a state of its own).
    describe() turns frames into control values: eight descriptors per frame (the previous frame's amps carried along).
    demix() takes the frames of the left and of the right channel of one recording apart by pan position.
    delay() gives every bin its own delay time and feedback (two histories of the stream carried along, after delay_setup()).
    tanal() analyses a stored signal at any time points, each frame under a window of its own: the way to another speed.
    bands() turns frames into feature vectors: the energies of a bank of bands, their log, a DCT (mel, MFCC; after bank_setup()).
    Like the other objects the constructor does not raise, and every call returns its status."""
    _abi = "clfa_pvoc_"

    def __init__(self, device_id, size, hop, sr, channels=1):
        self.size, self.hop, self.sr, self.channels = int(size), int(hop), float(sr), int(channels)
        self.M = self.size // 2
        self._create(self._fn("create"), int(device_id), self.size, self.hop, self.sr, self.channels)

    def kernel_name(self, synthesis=False):
        return self._text("kernel_name", int(bool(synthesis)))

    def scan_chunk(self):
        """frames per chunk of the synthesis' phase scan (fixed)"""
        return self._fn("scan_chunk")()

    def reset(self):
        return self._get("reset")

    def read_phase(self):
        """the synthesis state: uint32 (channels, size/2 + 1), units of 2^-32 turn (blocking)"""
        out = np.zeros((self.channels, self.M + 1), np.uint32)
        check(self._get("read_phase", out.ctypes.data), "Pvoc.read_phase")
        return out

    def read_prev(self):
        """the analysis state: complex64 (channels, size/2 + 1), z of the last frame analysed (blocking)"""
        out = np.zeros((self.channels, self.M + 1), np.complex64)
        check(self._get("read_prev", out.ctypes.data), "Pvoc.read_prev")
        return out

    # ---- spectra <-> frames ----

    def _device_call(self, name, spectra, frames, src, dst, stream):
        F = self._shapes(spectra, frames)
        if (F is None or str(spectra.dtype) != "torch.complex64" or not _is_f32(frames)
                or not spectra.is_contiguous() or not frames.is_contiguous()):
            return CL_INVALID_VALUE
        return self._get(name, src.data_ptr(), dst.data_ptr(), F, _stream_of(dst, stream))

    def analyze_device(self, spectra, frames_out, stream=None):
        """torch: spectra (channels, F, size/2) complex64 -> frames_out (channels, F, size/2 + 1, 2) float32, both
        contiguous (anything else: CL_INVALID_VALUE); asynchronous on `stream` (default: the current stream)"""
        return self._device_call("analyze_dev", spectra, frames_out, spectra, frames_out, stream)

    def synthesize_device(self, frames, spectra_out, stream=None):
        """torch: frames (channels, F, size/2 + 1, 2) float32 -> spectra_out (channels, F, size/2) complex64"""
        return self._device_call("synthesize_dev", spectra_out, frames, frames, spectra_out, stream)

    def analyze(self, spectra):
        """host: complex64 (channels, F, size/2) (or (F, size/2) for one channel) -> float32 (.., F, size/2 + 1, 2)"""
        spectra = np.ascontiguousarray(spectra, dtype=np.complex64)
        out = np.zeros(spectra.shape[:-1] + (self.M + 1, 2), np.float32)
        F = self._shapes(spectra, out)
        if F is None:
            raise ValueError("spectra must be (%d, F, %d)" % (self.channels, self.M))
        check(self._get("analyze", spectra.ctypes.data, out.ctypes.data, F), "Pvoc.analyze")
        return out

    def synthesize(self, frames):
        """host: float32 (channels, F, size/2 + 1, 2) (or (F, size/2 + 1, 2)) -> complex64 (.., F, size/2)"""
        frames, F, _, out = self._host_prep(frames, tail=(self.M,), dtype=np.complex64)
        check(self._get("synthesize", frames.ctypes.data, out.ctypes.data, F), "Pvoc.synthesize")
        return out
