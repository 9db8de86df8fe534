"""What the calls of Pvoc share: the shapes, then the preparation of a host call and of a device call."""
import numpy as np

from ._base import _is_f32


def _dense_f32(t, shape):
    """a device call's tensor: float32, contiguous, of this shape"""
    return _is_f32(t) and tuple(t.shape) == tuple(shape) and t.is_contiguous()


class _PvocCalls:
    """The base of every family of Pvoc's calls (_pvoc_frames.py, _pvoc_stream.py, _pvoc_rows.py, _pvoc_signal.py); it
    needs the object's channels and M."""

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
