"""Pvoc's calls from frames to rows of values per frame (pvoc_rows_host.cpp): describe, bands (with the bank), pitch."""
import numpy as np

from ._base import CL_INVALID_VALUE, _data, _stream_of
from ._lib import check
from ._pvoc_calls import _PvocCalls, _dense_f32


class _PvocDesc(_PvocCalls):
    """clfa_pvoc_desc*: eight descriptors per frame (Csound's pvscent and kin), the previous frame's amps carried along."""

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


class _PvocBank(_PvocCalls):
    """clfa_pvoc_bank*, clfa_pvoc_bands*: band energies, their log, a DCT of that (Csound's mfb + dct; mel, MFCC)."""

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


class _PvocPitch(_PvocCalls):
    """clfa_pvoc_pitch*: the fundamental of every frame from its spectral peaks, and the list of those peaks."""

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
