"""Pvoc's calls from frames to frames along the stream, each with a carried history and a set-up (pvoc_stream_host.cpp):
time (blur, smooth, freeze) and the per-bin delay."""
import numpy as np

from ._base import CL_INVALID_VALUE, _data, _stream_of
from ._lib import check
from ._pvoc_calls import _PvocCalls


class _PvocTime(_PvocCalls):
    """clfa_pvoc_time*, clfa_pvoc_blur_*: blur, smooth, freeze (Csound's pvsblur, pvsmooth, pvsfreeze)."""

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


class _PvocDelay(_PvocCalls):
    """clfa_pvoc_delay*: a delay per bin, with feedback (Csound's pvsbuffer + pvsbufread2 with a table of delay times)."""

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
