"""Pvoc's stateless calls from frames to frames (pvoc_frames_host.cpp): ops, pair, shape, trace, demix."""
import numpy as np

from ._base import CL_INVALID_VALUE, _data, _stream_of
from ._lib import check
from ._pvoc_calls import _PvocCalls, _dense_f32


class _PvocOps(_PvocCalls):
    """clfa_pvoc_scale*, clfa_pvoc_shift*, clfa_pvoc_read*: pitch scale, frequency shift, timed read."""

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


class _PvocPair(_PvocCalls):
    """clfa_pvoc_pair*: two streams of frames -> frames (cross, morph, filter, mix, vocode)."""

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


class _PvocShape(_PvocCalls):
    """clfa_pvoc_shape*: one stream of frames -> frames, along the bins (band, mask, stencil, arp, lock, warp)."""

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


class _PvocTrace(_PvocCalls):
    """clfa_pvoc_trace*: the N loudest bins of every frame (Csound's pvstrace)."""

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


class _PvocDemix(_PvocCalls):
    """clfa_pvoc_demix*: left and right frames -> frames by azimuth, and the azimuth profile (Csound's pvsdemix)."""

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
