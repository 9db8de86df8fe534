"""Pvoc: the phase vocoder on Stft's spectra — (amp, freq) frames both ways, and the operations on such frames."""
import numpy as np

from ._base import CL_INVALID_VALUE, _Object, _data, _is_f32, _row_view, _stream_of
from ._lib import check


def _dense_f32(t, shape):
    """a device call's tensor: float32, contiguous, of this shape"""
    return _is_f32(t) and tuple(t.shape) == tuple(shape) and t.is_contiguous()


class _PvocStereo:
    """The operations of Pvoc whose two inputs are the left and the right channel of one recording (clfa_pvoc_demix*
    in clfft_amd.h).  A base of Pvoc, which supplies the object and the shared preparation of a call: the operations
    Pvoc itself defines take one stream of frames, or two unrelated ones."""

    # ---- left and right frames -> frames by azimuth, and the azimuth profile (Csound's pvsdemix; stateless; clfft_amd.h) ----

    def demix_kernel_name(self, az=False):
        """ "k_pvoc_demix", or "k_pvoc_demix_az" for a call with the profile ("" for a failed object)"""
        return self._text("demix_kernel_name", int(bool(az)))

    def demix_device(self, left, right, out, par, points, first_bin=0, nbins=None, az_out=None, stream=None):
        """torch: the frames of the left and of the right channel of one recording, (channels, F, size/2 + 1, 2) float32,
        contiguous -> out of the same shape.  Every bin of first_bin .. first_bin + nbins - 1 (default: up to size/2) is
        placed on an azimuth axis of 2 points + 1 positions, -points hard left .. +points hard right, by the gain n / points
        of the louder side that best cancels the quieter one; the bins within width / 2 positions of pos * points keep
        the magnitude the cancellation uncovers, every other amp is +0; the freqs are the louder side's.  par: a float32
        device tensor (F, 2) of rows (pos in [-1, 1], width in [1, 2 points + 1]), shared by the channels, or a (pos, width)
        pair of numbers.  az_out: a float32 device tensor (channels, F, 2 points + 1), contiguous ((F, 2 points + 1) for one
        channel), that takes the azimuth profile: per position the summed magnitudes of the bins placed there, whatever the
        window.  out and az_out may overlap nothing; left and right may be one tensor.  Asynchronous on `stream`."""
        F = self._device_frames(left, right, out)
        if hasattr(par, "data_ptr"):
            prep = None if F is None or not _dense_f32(par, (F, 2)) else (F, [par.data_ptr()], [par])
        else:
            try:
                pos, width = par
            except (TypeError, ValueError):
                return CL_INVALID_VALUE
            prep = self._device_prep(F, out.device, (pos, width), columns=2)
        points = int(points)
        if prep is None:
            return CL_INVALID_VALUE
        (F, (rows,), _), az = prep, None
        if az_out is not None:
            if (self._full(az_out.shape, 3) != (self.channels, F, 2 * points + 1) or not _dense_f32(az_out, az_out.shape)
                    or az_out.device != out.device):
                return CL_INVALID_VALUE
            az = az_out.data_ptr()
        first_bin, nbins, _ = self._selection(first_bin, nbins, 1)
        return self._get("demix_dev", left.data_ptr(), right.data_ptr(), out.data_ptr(), rows, az, F, points, first_bin,
                         nbins, _stream_of(out, stream))

    def demix(self, left, right, pos, width, points, first_bin=0, nbins=None, az=False):
        """host form of demix_device, blocking: float32 (channels, F, size/2 + 1, 2) (or (F, size/2 + 1, 2)) twice -> the
        new frames, or (frames, profile) with the profile float32 (.., F, 2 points + 1) when az is set.  pos, width:
        numbers or (F,) arrays; a pos outside [-1, 1] or a width outside [1, 2 points + 1] raises ClError(CL_INVALID_VALUE)"""
        (left, F), (right, Fr) = self._host_frames(left), self._host_frames(right)
        if Fr != F or left.shape != right.shape:
            raise ValueError("left and right must have the same shape")
        left, F, (pos, width), out = self._host_prep(left, (pos, width))
        points = int(points)
        par = np.ascontiguousarray(np.stack([pos, width], axis=1))
        prof = np.zeros(left.shape[:-2] + (max(2 * points + 1, 0),), np.float32) if az else None
        first_bin, nbins, _ = self._selection(first_bin, nbins, 1)
        check(self._get("demix", left.ctypes.data, right.ctypes.data, out.ctypes.data, par.ctypes.data, _data(prof), F, points,
                        first_bin, nbins), "Pvoc.demix")
        return out if prof is None else (out, prof)


class _PvocDelay:
    """The operation of Pvoc that reads the stream's past through a table over the bins (clfa_pvoc_delay* in clfft_amd.h):
    the per-bin delay with feedback.  A base of Pvoc, like _PvocStereo: Pvoc supplies the object and the shared
    preparation of a call, and its own operations take their parameters per frame, not per bin."""

    # ---- frames -> frames along the stream: a delay per bin, with feedback (Csound's pvsbuffer + pvsbufread2 with a
    # ---- table of delay times; two carried histories; clfft_amd.h)

    def delay_kernel_name(self, feedback=False):
        """ "k_pvoc_delay", or "k_pvoc_delay_fb" for a call with feedback ("" for a failed object)"""
        return self._text("delay_kernel_name", int(bool(feedback)))

    def delay_setup(self, max_delay):
        """allocates and resets the two histories for delays of up to max_delay (0..4096) frames (blocking)"""
        return self._get("delay_setup", int(max_delay))

    def delay_max_frames(self):
        """max_delay of the last delay_setup, -1 before"""
        return self._get("delay_max_frames")

    def delay_state_bytes(self):
        """device memory of the two histories and the spare their commits share"""
        return self._get("delay_state_bytes")

    def delay_state(self):
        """(xhist, yhist): the last max_delay input frames and the last max_delay output frames of the stream (blocking),
        float32 (channels, max_delay, size/2 + 1, 2) each, oldest frame first"""
        out = [np.zeros((self.channels, max(self.delay_max_frames(), 0), self.M + 1, 2), np.float32) for _ in range(2)]
        for which, a in enumerate(out):
            check(self._get("delay_read_state", which, a.ctypes.data), "Pvoc.delay_state")
        return tuple(out)

    @staticmethod
    def delay_frames(seconds, sr, hop):
        """a delay time in seconds as the nearest whole number of frames of `hop` samples at the sample rate sr"""
        return int(round(float(seconds) * float(sr) / int(hop)))

    def _delay_table(self, t, dtype, device):
        """a table over the bins for a device call: a device tensor of `dtype` (size/2 + 1,), contiguous, as it is; a number
        as a tensor of size/2 + 1 copies on `device` (filled on torch's current stream, as _device_prep's are); else None"""
        import torch
        if hasattr(t, "data_ptr"):
            ok = t.dtype == dtype and tuple(t.shape) == (self.M + 1,) and t.is_contiguous() and t.device == device
            return t if ok else None
        try:
            return torch.full((self.M + 1,), int(t) if dtype == torch.int32 else float(t), dtype=dtype, device=device)
        except (TypeError, ValueError):
            return None

    def delay_device(self, frames_in, frames_out, delays, feedback=None, stream=None):
        """torch: frames (channels, F, size/2 + 1, 2) float32, contiguous -> frames_out of the same shape: bin b of frame t
        is bin b of the stream's frame t - d, d = delays[b] clamped to 0..max_delay of delay_setup; with feedback,
        y[t] = x[t - d] + g y[t - d] per bin, g = feedback[b], and an echo louder than the delayed input brings its freq
        along.  delays: an int32 device tensor (size/2 + 1,) or one int for every bin; feedback: a float32 device tensor
        (size/2 + 1,), a number, or None for none.  The frames of earlier calls are the object's two histories.
        frames_out may overlap neither frames_in nor a table.  Asynchronous on `stream`."""
        import torch
        F = self._device_frames(frames_in, frames_out)
        d = self._delay_table(delays, torch.int32, frames_out.device)
        g = None if feedback is None else self._delay_table(feedback, torch.float32, frames_out.device)
        if F is None or d is None or (feedback is not None and g is None):
            return CL_INVALID_VALUE
        return self._get("delay_dev", frames_in.data_ptr(), frames_out.data_ptr(), F, d.data_ptr(),
                         None if g is None else g.data_ptr(), _stream_of(frames_out, stream))

    def delay(self, frames, delays, feedback=None):
        """host form of delay_device, blocking: returns the new frames; delays: an int or an integer (size/2 + 1,) array,
        feedback: a number, a (size/2 + 1,) array or None.  A delay outside 0..max_delay, or a feedback that is not finite
        or above 1 in size, raises ClError(CL_INVALID_VALUE)"""
        frames, F, _, out = self._host_prep(frames)
        d = np.ascontiguousarray(np.broadcast_to(np.asarray(delays, dtype=np.int32), (self.M + 1,)))
        g = None if feedback is None else np.ascontiguousarray(np.broadcast_to(np.asarray(feedback, dtype=np.float32), (self.M + 1,)))
        check(self._get("delay", frames.ctypes.data, out.ctypes.data, F, d.ctypes.data, _data(g)), "Pvoc.delay")
        return out


class _PvocStored:
    """The operation of Pvoc that reads a stored signal, not frames (clfa_pvoc_tanal* in clfft_amd.h): the analysis at any
    time points.  A base of Pvoc, like _PvocStereo: Pvoc supplies the object and the shapes, and its own operations start
    from spectra or frames."""

    # ---- a stored signal -> frames at any time points (Csound's pvstanal, mincer; stateless; clfft_amd.h) ----

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


class _PvocBank:
    """The operation of Pvoc that turns frames into feature vectors through a bank the object is configured with
    (clfa_pvoc_bank*, clfa_pvoc_bands* in clfft_amd.h): band energies, their log, a DCT of that — the mel spectrum and the
    MFCCs.  A base of Pvoc, like _PvocStereo: Pvoc supplies the object and the shapes, and its own operations take their
    parameters per call, not from a setup."""

    # ---- frames -> band energies, log, DCT (Csound's mfb + dct; stateless apart from the bank; clfft_amd.h) ----

    BANDS_POWER, BANDS_LOG, BANDS_DCT = 1, 2, 4

    def bands_kernel_name(self):
        """ "k_pvoc_bands" ("" for a failed object)"""
        return self._text("bands_kernel_name")

    def bank_setup(self, first, count, weights):
        """sets the bank (blocking): band b covers the bins first[b] .. first[b] + count[b] - 1 of 0 .. size/2 with the
        float32 weights weights[sum(count[:b]) : sum(count[:b + 1])]; 1..256 bands, which may overlap, repeat and come in
        any order; finite weights of any sign.  Anything else is CL_INVALID_VALUE and leaves the bank as it was."""
        try:
            first = np.ascontiguousarray(first, dtype=np.int32).reshape(-1)
            count = np.ascontiguousarray(count, dtype=np.int32).reshape(-1)
            weights = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        except (TypeError, ValueError, OverflowError):
            return CL_INVALID_VALUE
        # the library reads sum(count) weights once every count is >= 1: the array has to hold them
        if first.size != count.size or ((count >= 1).all() and weights.size != int(count.astype(np.int64).sum())):
            return CL_INVALID_VALUE
        return self._get("bank_setup", int(count.size), first.ctypes.data, count.ctypes.data, weights.ctypes.data)

    def bank_bands(self):
        """the bands of the last bank_setup, -1 before"""
        return self._get("bank_bands")

    def bank_state_bytes(self):
        """device memory of the bank: bands, schedule, weights, DCT table"""
        return self._get("bank_state_bytes")

    def bank_dct(self):
        """the DCT table the device uses (blocking): float32 (B, B), D[q][b], the orthonormal DCT-II"""
        B = max(self.bank_bands(), 0)
        out = np.zeros((B, B), np.float32)
        check(self._get("bank_read_dct", out.ctypes.data), "Pvoc.bank_dct")
        return out

    def _bands_flags(self, power, log, ncoef):
        ncoef = int(ncoef)
        return ((self.BANDS_POWER if power else 0) | (self.BANDS_LOG if log else 0) | (self.BANDS_DCT if ncoef else 0)), ncoef

    def bands_device(self, frames_in, out, power=False, log=False, ncoef=0, floor=1e-10, stream=None):
        """torch: frames (channels, F, size/2 + 1, 2) float32, contiguous -> out (channels, F, N) float32, contiguous
        ((F, N) for one channel): per frame the bank's band energies, the weighted sums of the amps (power: of their
        squares), each a fixed tree of float32 additions — the same bits on every call; log: their logarithms, an energy
        below `floor` (or a NaN) taking the floor; ncoef != 0: the first ncoef coefficients of the orthonormal DCT-II of
        that vector.  N = ncoef where that is set, else the bank's bands.  out may not overlap frames_in.  Asynchronous on
        `stream`."""
        F = self._device_frames(frames_in)
        flags, ncoef = self._bands_flags(power, log, ncoef)
        shape = self._full(out.shape, 3) if hasattr(out, "data_ptr") else ()
        N = ncoef if ncoef else self.bank_bands()
        if (F is None or len(shape) != 3 or shape[:2] != (self.channels, F) or (N >= 1 and shape[2] != N)
                or not _dense_f32(out, out.shape) or out.device != frames_in.device):
            return CL_INVALID_VALUE
        return self._get("bands_dev", frames_in.data_ptr(), out.data_ptr(), F, flags, ncoef, float(floor),
                         _stream_of(out, stream))

    def bands(self, frames, power=False, log=False, ncoef=0, floor=1e-10):
        """host form of bands_device, blocking: float32 (channels, F, size/2 + 1, 2) (or (F, size/2 + 1, 2)) -> float32
        (.., F, N); a floor that is not positive and finite with log, or an ncoef outside 1..bands, raises
        ClError(CL_INVALID_VALUE)"""
        flags, ncoef = self._bands_flags(power, log, ncoef)
        N = ncoef if ncoef else self.bank_bands()
        frames, F, _, out = self._host_prep(frames, tail=(max(N, 1),))
        check(self._get("bands", frames.ctypes.data, out.ctypes.data, F, flags, ncoef, float(floor)), "Pvoc.bands")
        return out

    @staticmethod
    def mel_bank(size, sr, nbands, fmin=0.0, fmax=None):
        """(first, count, weights) of nbands HTK-mel triangles for bank_setup: mel = 2595 log10(1 + f / 700), the
        nbands + 2 edges equally spaced in mel from fmin to fmax (default sr / 2), the weights evaluated in float64 at
        the bin centres k sr / size, k = 0 .. size/2, and rounded to float32, leading and trailing zeros trimmed.  A
        band whose triangle reaches no bin centre is the one bin nearest its centre with the weight 0."""
        size, nbands, sr = int(size), int(nbands), float(sr)
        fmax = sr / 2 if fmax is None else float(fmax)
        M = size // 2
        mel = lambda f: 2595.0 * np.log10(1.0 + np.asarray(f, np.float64) / 700.0)
        edges = 700.0 * (10.0 ** (np.linspace(mel(fmin), mel(fmax), nbands + 2) / 2595.0) - 1.0)
        f = np.arange(M + 1, dtype=np.float64) * sr / size
        first, count, weights = [], [], []
        for b in range(nbands):
            lo, mid, hi = edges[b], edges[b + 1], edges[b + 2]
            w = np.maximum(0.0, np.minimum((f - lo) / (mid - lo), (hi - f) / (hi - mid))).astype(np.float32)
            nz = np.flatnonzero(w)
            if nz.size:
                k0, k1 = int(nz[0]), int(nz[-1])
            else:
                k0 = k1 = int(min(max(np.rint(mid * size / sr), 0), M))
            first.append(k0)
            count.append(k1 - k0 + 1)
            weights.append(w[k0:k1 + 1] if nz.size else np.zeros(1, np.float32))
        return np.array(first, np.int32), np.array(count, np.int32), np.concatenate(weights).astype(np.float32)


class _PvocPitch:
    """The operation of Pvoc that estimates from the frames, not reshapes them (clfa_pvoc_pitch* in clfft_amd.h): the
    fundamental frequency of every frame from its spectral peaks, and the list of those peaks.  A base of Pvoc, like
    _PvocStereo: Pvoc supplies the object and the shapes, and its own operations answer with frames, samples or the
    descriptors' sums."""

    PITCH_F0, PITCH_SAL, PITCH_CONF, PITCH_NPEAKS = range(4)
    PITCH_PEAKS_MAX = 32

    def pitch_kernel_name(self):
        """ "k_pvoc_pitch" ("" for a failed object)"""
        return self._text("pitch_kernel_name")

    def _pitch_range(self, first_bin, nbins):
        """the bins first_bin .. first_bin + nbins - 1, by default up to size/2 - 1: every bin of it has both neighbours"""
        first_bin = int(first_bin)
        return first_bin, self.M - first_bin if nbins is None else int(nbins)

    def pitch_device(self, frames_in, rows, thresh, fmin, fmax, npeaks=16, tol=0.03, decay=0.84, first_bin=1, nbins=None,
                     peaks_out=None, stream=None):
        """torch: frames (channels, F, size/2 + 1, 2) float32, contiguous -> rows (channels, F, 4) float32, contiguous
        ((F, 4) for one channel): per frame the columns PITCH_F0 (the fundamental in Hz, 0 where none is found), PITCH_SAL
        (its score: the summed amps of the peaks that lie on its harmonics, harmonic h weighted decay ** (h - 1); Csound's
        kamp), PITCH_CONF (SAL over the summed amps of all the peaks) and PITCH_NPEAKS.  The peaks are the first `npeaks`
        (1..32) local maxima of the amps of the bins first_bin .. first_bin + nbins - 1 (default: 1 .. size/2 - 1) that
        reach `thresh` and have a finite freq > 0; the candidates are their freqs over 1..8 inside fmin..fmax; a peak lies
        on harmonic h of a candidate where its freq is within tol h of h times the candidate (as a ratio).  peaks_out: a
        float32 device tensor (channels, F, npeaks, 2), contiguous ((F, npeaks, 2) for one channel), that takes the peaks'
        (amp, freq) pairs in ascending bin order, then zeros.  Asynchronous on `stream`."""
        F, npeaks = self._device_frames(frames_in), int(npeaks)
        if F is None or self._full(rows.shape, 3) != (self.channels, F, 4) or not _dense_f32(rows, rows.shape):
            return CL_INVALID_VALUE
        peaks = None
        if peaks_out is not None:
            if (self._full(peaks_out.shape, 4) != (self.channels, F, npeaks, 2) or not _dense_f32(peaks_out, peaks_out.shape)
                    or peaks_out.device != rows.device):
                return CL_INVALID_VALUE
            peaks = peaks_out.data_ptr()
        first_bin, nbins = self._pitch_range(first_bin, nbins)
        return self._get("pitch_dev", frames_in.data_ptr(), rows.data_ptr(), peaks, F, first_bin, nbins, npeaks, float(thresh),
                         float(fmin), float(fmax), float(tol), float(decay), _stream_of(rows, stream))

    def pitch(self, frames, thresh, fmin, fmax, npeaks=16, tol=0.03, decay=0.84, first_bin=1, nbins=None, peaks=False):
        """host form of pitch_device, blocking: float32 (channels, F, size/2 + 1, 2) (or (F, size/2 + 1, 2)) -> the rows,
        float32 (.., F, 4), or (rows, list) with the list float32 (.., F, npeaks, 2) when `peaks` is set"""
        frames, F, _, out = self._host_prep(frames, tail=(4,))
        npeaks = int(npeaks)
        lst = np.zeros(frames.shape[:-2] + (max(npeaks, 0), 2), np.float32) if peaks else None
        first_bin, nbins = self._pitch_range(first_bin, nbins)
        check(self._get("pitch", frames.ctypes.data, out.ctypes.data, _data(lst), F, first_bin, nbins, npeaks, float(thresh),
                        float(fmin), float(fmax), float(tol), float(decay)), "Pvoc.pitch")
        return out if lst is None else (out, lst)


class Pvoc(_Object, _PvocStereo, _PvocDelay, _PvocStored, _PvocBank, _PvocPitch):
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

    # ---- what the calls share: shapes, then the preparation of a host call and of a device call ----

    def _full(self, shape, rank):
        """`shape` as a tuple of `rank` axes, the channel axis first: for one channel it may be left out"""
        s = tuple(shape)
        return (1,) + s if len(s) == rank - 1 and self.channels == 1 else s

    def _frames_shape(self, shape):
        """F of a (channels, F, M + 1, 2) shape (or (F, M + 1, 2) for one channel), else None"""
        f = self._full(shape, 4)
        return f[1] if len(f) == 4 and f[0] == self.channels and f[2:] == (self.M + 1, 2) else None

    def _shapes(self, spectra, frames):
        """F if `spectra` is (channels, F, M) (or (F, M) for one channel) and `frames` the matching (.., F, M + 1, 2), else None"""
        F = self._frames_shape(frames.shape)
        return F if F is not None and self._full(spectra.shape, 3) == (self.channels, F, self.M) else None

    def _host_frames(self, frames):
        """(the frames as a contiguous float32 array, F); ValueError for another shape"""
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        F = self._frames_shape(frames.shape)
        if F is None:
            raise ValueError("frames must be (%d, F, %d, 2)" % (self.channels, self.M + 1))
        return frames, F

    def _host_prep(self, frames, pars=(), rows=None, tail=None, dtype=np.float32):
        """A host call's preparation: (the frames as a contiguous float32 array, F, the per-frame values `pars` — numbers
        or arrays, None stays None — as contiguous float32 (rows,) arrays, the zeroed output (.., rows) + tail).  rows: F
        unless given; tail: (M + 1, 2), the output being frames, unless given.  ValueError for frames of another shape."""
        frames, F = self._host_frames(frames)
        rows = F if rows is None else rows
        pars = [None if par is None else np.ascontiguousarray(np.broadcast_to(np.asarray(par, dtype=np.float32), (rows,)))
                for par in pars]
        return frames, F, pars, np.zeros(frames.shape[:-3] + (rows,) + ((self.M + 1, 2) if tail is None else tail), dtype)

    def _device_frames(self, *tensors):
        """F if every tensor holds F frames for a device call ((channels, F, M + 1, 2), or (F, M + 1, 2) for one channel,
        float32, contiguous), else None"""
        F = self._frames_shape(tensors[0].shape)
        ok = F is not None and all(self._frames_shape(t.shape) == F and _dense_f32(t, t.shape) for t in tensors)
        return F if ok else None

    def _device_prep(self, F, device, pars, columns=0):
        """The rest of a device call's preparation, F being _device_frames() of its frame tensors: (F, the pointers of the
        per-frame values `pars`, the tensors to keep until the call is made), or None for a call to refuse: F is None,
        or a value is a tensor that is not float32 (F,), contiguous.  A plain number becomes a tensor of F copies on
        `device`, None a NULL.  columns: the values become the columns of the one (F, columns) tensor of rows that the
        shaping ops read instead."""
        if F is None:
            return None
        pars = [par if par is None or hasattr(par, "data_ptr") else float(par) for par in pars]
        if any(hasattr(par, "data_ptr") and not _dense_f32(par, (F,)) for par in pars):
            return None
        # Known ordering problem, left as it was: the tensors made here are filled on torch's current stream, while the
        # library call that reads them runs on the caller's `stream`.  When the two differ nothing orders the fill before
        # the kernel, and the tensors are released when the caller returns.  A fix belongs here and nowhere else.
        import torch
        made = dict(dtype=torch.float32, device=device)
        if columns:
            rows = torch.zeros((F, columns), **made)
            for i, par in enumerate(pars):
                rows[:, i] = par
            pars = [rows]
        else:
            pars = [torch.full((F,), par, **made) if isinstance(par, float) else par for par in pars]
        return F, [None if t is None else t.data_ptr() for t in pars], pars

    @staticmethod
    def _op_code(ops, op):
        """an op given by its name or its code, as the code (-1 for an unknown name)"""
        return ops.get(op, -1) if isinstance(op, str) else int(op)

    def _selection(self, first_bin, nbins, step):
        first_bin, step = int(first_bin), int(step)
        if nbins is None:      # every bin from first_bin up that the step reaches
            nbins = (self.M - first_bin) // step + 1 if step >= 1 and 0 <= first_bin <= self.M else 0
        return first_bin, int(nbins), step

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

    # ---- frames -> frames: pitch scale, frequency shift, timed read (stateless; clfft_amd.h) ----

    def ops_kernel_name(self, op, keepform=False):
        """op "scale", "shift" or "read" -> "k_pvoc_map" / "k_pvoc_formant" (keepform) / "k_pvoc_read" ("" for a failed object)"""
        return self._text("ops_kernel_name", {"scale": 0, "shift": 1, "read": 2}.get(op, -1), int(bool(keepform)))

    def scale_device(self, frames_in, frames_out, scale, keepform=False, gain=1.0, coefs=80, stream=None):
        """pitch scale (Csound's pvscale): torch frames (channels, F, size/2 + 1, 2) float32 -> frames_out of the same
        shape; scale: a number or a float32 device tensor (F,), each in [0.25, 4]; keepform: the formants (the
        cepstral envelope of `coefs` coefficients) stay where they are.  Asynchronous on `stream`."""
        prep = self._device_prep(self._device_frames(frames_in, frames_out), frames_out.device, (scale,))
        if prep is None:
            return CL_INVALID_VALUE
        F, (par,), _ = prep
        return self._get("scale_dev", frames_in.data_ptr(), frames_out.data_ptr(), F, par, int(bool(keepform)),
                         float(gain), int(coefs), _stream_of(frames_out, stream))

    def shift_device(self, frames_in, frames_out, shift, lowest_bin=1, keepform=False, gain=1.0, coefs=80, stream=None):
        """frequency shift (Csound's pvshift): the bins from lowest_bin up move by shift Hz (a number or a float32
        device tensor (F,)), rounded to whole bins; the bins below are copied"""
        prep = self._device_prep(self._device_frames(frames_in, frames_out), frames_out.device, (shift,))
        if prep is None:
            return CL_INVALID_VALUE
        F, (par,), _ = prep
        return self._get("shift_dev", frames_in.data_ptr(), frames_out.data_ptr(), F, par, int(lowest_bin),
                         int(bool(keepform)), float(gain), int(coefs), _stream_of(frames_out, stream))

    def read_device(self, frames_in, pos, frames_out, stream=None):
        """timed read (Csound's pvsbufread): frames_out[:, g] = frames_in read at the position pos[g] in frames (float32
        device tensor (Fout,)), clamped to the ends and interpolated linearly between neighbouring frames"""
        Fin = self._device_frames(frames_in)
        prep = None if Fin is None else self._device_prep(self._device_frames(frames_out), frames_out.device, (pos,))
        if prep is None or not hasattr(pos, "data_ptr"):
            return CL_INVALID_VALUE
        Fout, (par,), _ = prep
        return self._get("read_dev", frames_in.data_ptr(), Fin, par, frames_out.data_ptr(), Fout,
                         _stream_of(frames_out, stream))

    def scale(self, frames, scale, keepform=False, gain=1.0, coefs=80):
        """host form of scale_device, blocking: returns the new frames; a value of `scale` outside [0.25, 4] raises
        ClError(CL_INVALID_VALUE)"""
        frames, F, (par,), out = self._host_prep(frames, (scale,))
        check(self._get("scale", frames.ctypes.data, out.ctypes.data, F, par.ctypes.data, int(bool(keepform)), float(gain),
                        int(coefs)), "Pvoc.scale")
        return out

    def shift(self, frames, shift, lowest_bin=1, keepform=False, gain=1.0, coefs=80):
        """host form of shift_device, blocking"""
        frames, F, (par,), out = self._host_prep(frames, (shift,))
        check(self._get("shift", frames.ctypes.data, out.ctypes.data, F, par.ctypes.data, int(lowest_bin),
                        int(bool(keepform)), float(gain), int(coefs)), "Pvoc.shift")
        return out

    def read(self, frames, pos):
        """host form of read_device, blocking: pos float32 (Fout,) -> frames (.., Fout, size/2 + 1, 2)"""
        pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1)
        frames, Fin, (par,), out = self._host_prep(frames, (pos,), rows=pos.size)
        check(self._get("read", frames.ctypes.data, Fin, par.ctypes.data, out.ctypes.data, pos.size), "Pvoc.read")
        return out

    # ---- two streams of frames -> frames: cross, morph, filter, mix, vocode (stateless; clfft_amd.h) ----

    _PAIR_OPS = {"cross": 0, "morph": 1, "filter": 2, "mix": 3, "vocode": 4}

    def pair_kernel_name(self, op):
        """op "cross", "morph", "filter", "mix" (or 0..3) -> "k_pvoc_pair", "vocode" (4) -> "k_pvoc_vocode" ("" for a failed
        object or an unknown op)"""
        return self._text("pair_kernel_name", self._op_code(self._PAIR_OPS, op))

    def _pair_device(self, op, a, b, out, p, q, coefs, stream):
        """one two-input device call; p, q: numbers or float32 device tensors (F,), None for mix"""
        prep = self._device_prep(self._device_frames(out, a, b), out.device, (p, q))
        if prep is None:
            return CL_INVALID_VALUE
        F, (p, q), _ = prep
        return self._get("pair_dev", op, a.data_ptr(), b.data_ptr(), out.data_ptr(), F, p, q, int(coefs),
                         _stream_of(out, stream))

    def cross_device(self, a, b, out, amp_a=1.0, amp_b=1.0, stream=None):
        """cross-synthesis (Csound's pvscross): torch frames a, b (channels, F, size/2 + 1, 2) float32 -> out of the same
        shape with amp = a.amp amp_a + b.amp amp_b and the freqs of a; amp_a, amp_b: numbers or float32 device tensors
        (F,).  out may overlap neither input; a and b may be the same tensor.  Asynchronous on `stream`."""
        return self._pair_device(0, a, b, out, amp_a, amp_b, 1, stream)

    def morph_device(self, a, b, out, amp=0.5, freq=0.5, stream=None):
        """morph (Csound's pvsmorph): amps and freqs interpolated from a (weight 0) to b (weight 1); amp, freq: the two
        weights, numbers or float32 device tensors (F,), clamped to [0, 1]"""
        return self._pair_device(1, a, b, out, amp, freq, 1, stream)

    def filter_device(self, a, b, out, depth=1.0, gain=1.0, stream=None):
        """spectral filter (Csound's pvsfilter): the amps of a times (1 - depth) + depth b.amp, times gain; the freqs of a"""
        return self._pair_device(2, a, b, out, depth, gain, 1, stream)

    def mix_device(self, a, b, out, stream=None):
        """spectral maximum (Csound's pvsmix): per bin the (amp, freq) pair of the input with the larger amp"""
        return self._pair_device(3, a, b, out, None, None, 1, stream)

    def vocode_device(self, a, b, out, depth=1.0, gain=1.0, coefs=80, stream=None):
        """channel vocoder (Csound's pvsvoc): the excitation b takes the formants of a — its amps are multiplied by
        (1 - depth) + depth envA / envB, the cepstral envelopes of `coefs` coefficients, and by gain; the freqs of b"""
        return self._pair_device(4, a, b, out, depth, gain, coefs, stream)

    def _pair_host(self, op, a, b, p, q, coefs, what):
        (a, F), (b, Fb) = self._host_frames(a), self._host_frames(b)
        if Fb != F or a.shape != b.shape:
            raise ValueError("a and b must have the same shape")
        a, F, (p, q), out = self._host_prep(a, (p, q))
        check(self._get("pair", op, a.ctypes.data, b.ctypes.data, out.ctypes.data, F, _data(p), _data(q), int(coefs)), what)
        return out

    def cross(self, a, b, amp_a=1.0, amp_b=1.0):
        """host form of cross_device, blocking: returns the new frames"""
        return self._pair_host(0, a, b, amp_a, amp_b, 1, "Pvoc.cross")

    def morph(self, a, b, amp=0.5, freq=0.5):
        """host form of morph_device, blocking; a weight outside [0, 1] raises ClError(CL_INVALID_VALUE)"""
        return self._pair_host(1, a, b, amp, freq, 1, "Pvoc.morph")

    def filter(self, a, b, depth=1.0, gain=1.0):
        """host form of filter_device, blocking; a depth outside [0, 1] raises ClError(CL_INVALID_VALUE)"""
        return self._pair_host(2, a, b, depth, gain, 1, "Pvoc.filter")

    def mix(self, a, b):
        """host form of mix_device, blocking"""
        return self._pair_host(3, a, b, None, None, 1, "Pvoc.mix")

    def vocode(self, a, b, depth=1.0, gain=1.0, coefs=80):
        """host form of vocode_device, blocking; a depth outside [0, 1] raises ClError(CL_INVALID_VALUE)"""
        return self._pair_host(4, a, b, depth, gain, coefs, "Pvoc.vocode")

    # ---- one stream of frames -> frames, along the bins: band, mask, stencil, arp, lock, warp (stateless; clfft_amd.h) ----

    _SHAPE_OPS = {"band": 0, "mask": 1, "stencil": 2, "arp": 3, "lock": 4, "warp": 5}

    def shape_kernel_name(self, op):
        """op "band", "mask", "stencil", "arp" (or 0..3) -> "k_pvoc_shape", "lock" (4) -> "k_pvoc_lock", "warp" (5) ->
        "k_pvoc_warp" ("" for a failed object or an unknown op)"""
        return self._text("shape_kernel_name", self._op_code(self._SHAPE_OPS, op))

    def _shape_device(self, op, frames_in, frames_out, cols, table, flags, lowest_bin, coefs, stream):
        """one shaping device call; cols: the op's per-frame values (numbers or float32 device tensors (F,)), stacked
        into the (F, 4) rows the library reads; table: None or a float32 device tensor (size/2 + 1,)"""
        prep = self._device_prep(self._device_frames(frames_out, frames_in), frames_out.device, cols, columns=4)
        if prep is None or (table is not None and not (hasattr(table, "data_ptr") and _dense_f32(table, (self.M + 1,)))):
            return CL_INVALID_VALUE
        F, (rows,), _ = prep
        return self._get("shape_dev", op, frames_in.data_ptr(), frames_out.data_ptr(), F, rows,
                         None if table is None else table.data_ptr(), int(flags), int(lowest_bin), int(coefs),
                         _stream_of(frames_out, stream))

    def band_device(self, frames_in, frames_out, lowcut, lowfull, highfull, highcut, reject=False, stream=None):
        """band pass (Csound's pvsbandp; reject: the band reject pvsbandr): torch frames (channels, F, size/2 + 1, 2)
        float32 -> frames_out of the same shape, the amps times a gain that rises from 0 at lowcut to 1 at lowfull, stays
        1 up to highfull and falls to 0 at highcut (Hz, against each bin's |freq|; numbers or float32 device tensors
        (F,)).  frames_out may not overlap frames_in.  Asynchronous on `stream`."""
        return self._shape_device(0, frames_in, frames_out, (lowcut, lowfull, highfull, highcut), None,
                                  int(bool(reject)), 1, 1, stream)

    def mask_device(self, frames_in, frames_out, table, depth=1.0, stream=None):
        """table mask (Csound's pvsmaska): the amps times (1 - depth) + depth table[k]; table: float32 device tensor
        (size/2 + 1,), depth clamped to [0, 1]"""
        return self._shape_device(1, frames_in, frames_out, (depth,), table, 0, 1, 1, stream)

    def stencil_device(self, frames_in, frames_out, table, gain=0.0, level=1.0, stream=None):
        """stencil (Csound's pvstencil): the amps below table[k] level are multiplied by gain, the others kept"""
        return self._shape_device(2, frames_in, frames_out, (gain, level), table, 0, 1, 1, stream)

    def arp_device(self, frames_in, frames_out, pos, depth=1.0, gain=1.0, stream=None):
        """spectral arpeggiator (Csound's pvsarp): the bin at pos (0..1 of the bins 0..size/2) is multiplied by gain,
        every other bin by 1 - depth"""
        return self._shape_device(3, frames_in, frames_out, (pos, depth, gain), None, 0, 1, 1, stream)

    def lock_device(self, frames_in, frames_out, lock=1.0, tol=0.01, stream=None):
        """peak frequency lock (Csound's pvslock): in a frame with lock != 0, the bins next to a spectral peak take the
        peak's freq where theirs lies within tol |freq| of it"""
        return self._shape_device(4, frames_in, frames_out, (lock, tol), None, 0, 1, 1, stream)

    def warp_device(self, frames_in, frames_out, scale, shift=0.0, lowest_bin=1, gain=1.0, coefs=80, stream=None):
        """envelope warp (Csound's pvswarp): the spectral envelope (cepstral, `coefs` coefficients) of the bins from
        lowest_bin up is scaled by `scale` (in [0.25, 4]) and shifted by `shift` Hz, the partials stay where they are"""
        return self._shape_device(5, frames_in, frames_out, (scale, shift, gain), None, 0, lowest_bin, coefs, stream)

    def _shape_host(self, op, frames, cols, table, flags, lowest_bin, coefs, what):
        frames, F, cols, out = self._host_prep(frames, cols)
        rows = np.zeros((F, 4), np.float32)
        rows[:, :len(cols)] = np.stack(cols, axis=1)
        if table is not None:
            table = np.ascontiguousarray(table, dtype=np.float32)
            if table.shape != (self.M + 1,):
                raise ValueError("table must be (%d,)" % (self.M + 1))
        check(self._get("shape", op, frames.ctypes.data, out.ctypes.data, F, rows.ctypes.data, _data(table), int(flags),
                        int(lowest_bin), int(coefs)), what)
        return out

    def band(self, frames, lowcut, lowfull, highfull, highcut, reject=False):
        """host form of band_device, blocking: returns the new frames; edges that are not finite or not in the order
        0 <= lowcut <= lowfull <= highfull <= highcut raise ClError(CL_INVALID_VALUE)"""
        return self._shape_host(0, frames, (lowcut, lowfull, highfull, highcut), None, int(bool(reject)), 1, 1, "Pvoc.band")

    def mask(self, frames, table, depth=1.0):
        """host form of mask_device, blocking; a depth outside [0, 1] raises ClError(CL_INVALID_VALUE)"""
        return self._shape_host(1, frames, (depth,), table, 0, 1, 1, "Pvoc.mask")

    def stencil(self, frames, table, gain=0.0, level=1.0):
        """host form of stencil_device, blocking"""
        return self._shape_host(2, frames, (gain, level), table, 0, 1, 1, "Pvoc.stencil")

    def arp(self, frames, pos, depth=1.0, gain=1.0):
        """host form of arp_device, blocking; a pos or depth outside [0, 1] raises ClError(CL_INVALID_VALUE)"""
        return self._shape_host(3, frames, (pos, depth, gain), None, 0, 1, 1, "Pvoc.arp")

    def lock(self, frames, lock=1.0, tol=0.01):
        """host form of lock_device, blocking; a negative tol raises ClError(CL_INVALID_VALUE)"""
        return self._shape_host(4, frames, (lock, tol), None, 0, 1, 1, "Pvoc.lock")

    def warp(self, frames, scale, shift=0.0, lowest_bin=1, gain=1.0, coefs=80):
        """host form of warp_device, blocking; a scale outside [0.25, 4] raises ClError(CL_INVALID_VALUE)"""
        return self._shape_host(5, frames, (scale, shift, gain), None, 0, lowest_bin, coefs, "Pvoc.warp")

    # ---- frames -> frames along the stream: blur, smooth, freeze (a carried state each; clfft_amd.h) ----

    _TIME_OPS = {"blur": 0, "smooth": 1, "freeze": 2}

    def time_kernel_name(self, op):
        """op "blur", "smooth", "freeze" (or 0..2) -> "k_pvoc_blur", "k_pvoc_smooth", "k_pvoc_freeze" ("" for a failed
        object or an unknown op)"""
        return self._text("time_kernel_name", self._op_code(self._TIME_OPS, op))

    def time_state_bytes(self):
        """device memory of the three carried states, the blur's spare included"""
        return self._get("time_state_bytes")

    def blur_setup(self, max_frames):
        """allocates and resets the blur's history for windows of up to max_frames (1..4096) frames (blocking)"""
        return self._get("blur_setup", int(max_frames))

    def blur_max_frames(self):
        """max_frames of the last blur_setup, 0 before"""
        return self._get("blur_max_frames")

    def time_state(self, op):
        """the carried state of op "blur", "smooth" or "freeze" (blocking), float32: the blur's history (channels,
        max_frames - 1, size/2 + 1, 2), oldest frame first; the smoothing's y and the freeze's held (channels, size/2 + 1, 2)"""
        code = self._op_code(self._TIME_OPS, op)
        shape = (self.channels, max(self.blur_max_frames() - 1, 0)) if code == 0 else (self.channels,)
        out = np.zeros(shape + (self.M + 1, 2), np.float32)
        check(self._get("time_read_state", code, out.ctypes.data), "Pvoc.time_state")
        return out

    def _time_device(self, op, frames_in, frames_out, p, q, stream):
        """one device call along the frames; p, q: numbers or float32 device tensors (F,), q None for blur"""
        prep = self._device_prep(self._device_frames(frames_out, frames_in), frames_out.device, (p, q))
        if prep is None:
            return CL_INVALID_VALUE
        F, (p, q), _ = prep
        return self._get("time_dev", op, frames_in.data_ptr(), frames_out.data_ptr(), F, p, q,
                         _stream_of(frames_out, stream))

    def blur_device(self, frames_in, frames_out, length, stream=None):
        """moving average along the frames (Csound's pvsblur): torch frames (channels, F, size/2 + 1, 2) float32 ->
        frames_out of the same shape, each frame the mean of the stream's last n frames, n = length (a number or a
        float32 device tensor (F,)) cut to whole frames, 1..max_frames of blur_setup.  The frames of earlier calls are
        the object's history.  Asynchronous on `stream`."""
        return self._time_device(0, frames_in, frames_out, length, None, stream)

    def smooth_device(self, frames_in, frames_out, amp=0.5, freq=0.5, stream=None):
        """one-pole low-pass along the frames (Csound's pvsmooth): y += w (x - y) per bin, for the amps with the weight
        `amp`, for the freqs with `freq` (numbers or float32 device tensors (F,), clamped to [0, 1]; smooth_weight maps
        Csound's cutoff to a weight).  y is carried from call to call."""
        return self._time_device(1, frames_in, frames_out, amp, freq, stream)

    def freeze_device(self, frames_in, frames_out, amp=0.0, freq=0.0, stream=None):
        """freeze (Csound's pvsfreeze): where amp (freq) is not 0 in a frame, the amps (freqs) of the last frame of the
        stream where it was 0 are held; numbers or float32 device tensors (F,)"""
        return self._time_device(2, frames_in, frames_out, amp, freq, stream)

    def _time_host(self, op, frames, p, q, what):
        frames, F, (p, q), out = self._host_prep(frames, (p, q))
        check(self._get("time", op, frames.ctypes.data, out.ctypes.data, F, p.ctypes.data, _data(q)), what)
        return out

    def blur(self, frames, length):
        """host form of blur_device, blocking: returns the new frames; a length outside 1..max_frames raises
        ClError(CL_INVALID_VALUE)"""
        return self._time_host(0, frames, length, None, "Pvoc.blur")

    def smooth(self, frames, amp=0.5, freq=0.5):
        """host form of smooth_device, blocking; a weight outside [0, 1] raises ClError(CL_INVALID_VALUE)"""
        return self._time_host(1, frames, amp, freq, "Pvoc.smooth")

    def freeze(self, frames, amp=0.0, freq=0.0):
        """host form of freeze_device, blocking"""
        return self._time_host(2, frames, amp, freq, "Pvoc.freeze")

    @staticmethod
    def smooth_weight(cutoff):
        """Csound's pvsmooth cutoff (a fraction of half the frame rate) as the weight of smooth, in float64:
        g = 2 - cos(pi cutoff), c = 1 + sqrt(g g - 1) - g"""
        g = 2.0 - np.cos(np.pi * float(cutoff))
        return float(1.0 + np.sqrt(g * g - 1.0) - g)

    # ---- frames -> eight descriptors per frame (Csound's pvscent and kin; a state of its own; clfft_amd.h) ----

    DESC_MAG, DESC_POW, DESC_MOM, DESC_CENT, DESC_FLUX, DESC_PEAK_AMP, DESC_PEAK_FREQ, DESC_PEAK_BIN = range(8)

    def desc_kernel_name(self):
        """ "k_pvoc_desc" ("" for a failed object)"""
        return self._text("desc_kernel_name")

    def desc_state_bytes(self):
        """device memory of the descriptors' carried state"""
        return self._get("desc_state_bytes")

    def desc_state(self):
        """the descriptors' carried state (blocking): float32 (channels, size/2 + 1), the amps of the stream's last frame"""
        out = np.zeros((self.channels, self.M + 1), np.float32)
        check(self._get("desc_read_state", out.ctypes.data), "Pvoc.desc_state")
        return out

    def describe_device(self, frames_in, out, first_bin=0, nbins=None, rectify=False, stream=None):
        """torch: frames (channels, F, size/2 + 1, 2) float32, contiguous -> out (channels, F, 8) float32, contiguous
        ((F, 8) for one channel): per frame the columns DESC_MAG (sum of the amps), DESC_POW (of their squares), DESC_MOM
        (of amp times bin centre), DESC_CENT (MOM / MAG, Csound's pvscent), DESC_FLUX (the sum of the squared amp
        differences to the stream's previous frame; rectify: rises only), DESC_PEAK_AMP, DESC_PEAK_FREQ and DESC_PEAK_BIN,
        over the bins first_bin .. first_bin + nbins - 1 (default: up to size/2).  The sums are a fixed tree of float32
        additions: the same bits on every call.  The last frame's amps are carried to the next call.  Asynchronous on
        `stream`."""
        F = self._device_frames(frames_in)
        if F is None or self._full(out.shape, 3) != (self.channels, F, 8) or not _dense_f32(out, out.shape):
            return CL_INVALID_VALUE
        first_bin, nbins, _ = self._selection(first_bin, nbins, 1)
        return self._get("desc_dev", frames_in.data_ptr(), out.data_ptr(), F, first_bin, nbins, int(bool(rectify)),
                         _stream_of(out, stream))

    def describe(self, frames, first_bin=0, nbins=None, rectify=False):
        """host form of describe_device, blocking: float32 (channels, F, size/2 + 1, 2) (or (F, size/2 + 1, 2)) -> float32
        (.., F, 8)"""
        frames, F, _, out = self._host_prep(frames, tail=(8,))
        first_bin, nbins, _ = self._selection(first_bin, nbins, 1)
        check(self._get("desc", frames.ctypes.data, out.ctypes.data, F, first_bin, nbins, int(bool(rectify))), "Pvoc.describe")
        return out

    # ---- frames -> frames: the N loudest bins of every frame (Csound's pvstrace; stateless; clfft_amd.h) ----

    TRACE_RESIDUAL = 1

    def trace_kernel_name(self):
        """ "k_pvoc_trace" ("" for a failed object)"""
        return self._text("trace_kernel_name")

    def trace_device(self, frames_in, frames_out, n, first_bin=0, nbins=None, residual=False, bins_out=None, stream=None):
        """torch: frames (channels, F, size/2 + 1, 2) float32, contiguous -> frames_out of the same shape: of the bins
        first_bin .. first_bin + nbins - 1 (default: up to size/2) of every frame the floor(n) loudest keep their amp and the
        others get +0; residual: the other way round.  Equal amps: the lower bin is the louder one, so exactly floor(n) bins
        are selected (Csound's pvstrace keeps all ties); a NaN amp is never selected.  n: a number or a float32 device tensor
        (F,), shared by the channels.  bins_out: an int32 device tensor (channels, F, L), contiguous ((F, L) for one
        channel), that takes the selected bins in ascending order, the first L of them, then -1.  Asynchronous on `stream`."""
        prep = self._device_prep(self._device_frames(frames_in, frames_out), frames_out.device, (n,))
        if prep is None:
            return CL_INVALID_VALUE
        (F, (n,), _), bins, L = prep, None, 0
        if bins_out is not None:
            b = self._full(bins_out.shape, 3)
            if (len(b) != 3 or b[:2] != (self.channels, F) or b[2] < 1 or str(bins_out.dtype) != "torch.int32"
                    or not bins_out.is_contiguous() or bins_out.device != frames_out.device):
                return CL_INVALID_VALUE
            bins, L = bins_out.data_ptr(), b[2]
        first_bin, nbins, _ = self._selection(first_bin, nbins, 1)
        return self._get("trace_dev", frames_in.data_ptr(), frames_out.data_ptr(), n, bins, L, F, first_bin, nbins,
                         self.TRACE_RESIDUAL if residual else 0, _stream_of(frames_out, stream))

    def trace(self, frames, n, first_bin=0, nbins=None, residual=False, list_n=0):
        """host form of trace_device, blocking: float32 (channels, F, size/2 + 1, 2) (or (F, size/2 + 1, 2)) -> the new
        frames, or (frames, bins) with bins int32 (.., F, list_n) when list_n > 0"""
        frames, F, (n,), out = self._host_prep(frames, (n,))
        list_n = int(list_n)
        bins = np.full(frames.shape[:-2] + (list_n,), -1, np.int32) if list_n > 0 else None
        first_bin, nbins, _ = self._selection(first_bin, nbins, 1)
        check(self._get("trace", frames.ctypes.data, out.ctypes.data, n.ctypes.data, _data(bins), list_n, F, first_bin, nbins,
                        self.TRACE_RESIDUAL if residual else 0), "Pvoc.trace")
        return out if bins is None else (out, bins)

    # ---- frames -> samples: the oscillator bank (Csound's pvsadsyn; a state of its own; clfft_amd.h) ----

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
