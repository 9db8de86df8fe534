"""What the modules of the package share: the status constants, the owner of one object of the C ABI, and the checks
of device tensors and host arrays.  PyTorch is never imported here: tensors are only asked for what they carry."""
import ctypes as C
import sys

import numpy as np

# The package itself: every module reaches the library as _pkg.lib(), looked up at the time of the call, so that a
# stand-in library put in place of opencl_fft_amd.lib (tests/test_dist_cpu.py) is the one all of them call.
_pkg = sys.modules[__package__]

CL_SUCCESS = 0
CL_INVALID_VALUE = -30


def _is_f32(t):
    """is the torch tensor `t` of float32 (asked of its dtype's name: torch is not imported for it)"""
    return str(t.dtype) == "torch.float32"


def _stream_of(tensor, stream):
    """`stream` if it was given, else the HIP handle of the current torch stream on the tensor's device"""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream(tensor.device).cuda_stream
    return stream


def _ptr_stream(obj, stream):
    """(device pointer, hip stream handle) from a torch tensor or a raw int pointer"""
    if hasattr(obj, "data_ptr"):
        if not obj.is_contiguous():
            raise ValueError("device tensor must be contiguous")
        return obj.data_ptr(), _stream_of(obj, stream)
    return int(obj), stream


def _host(a, dtype):
    if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.flags.c_contiguous and a.flags.writeable):
        raise ValueError("expected a writable C-contiguous numpy array of %s" % np.dtype(dtype).name)
    return a


def _data(a):
    """the address of a host array, NULL for None"""
    return None if a is None else a.ctypes.data


def _row_view(t, what):
    """(pointer, rows, row length, row stride) of a (rows, n) or (n,) torch tensor whose rows are contiguous"""
    if t.dim() == 1:
        t = t.unsqueeze(0)
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError("%s: expected (channels, n) with contiguous rows" % what)
    return t.data_ptr(), t.shape[0], t.shape[1], t.stride(0)


def _block_rows(t, nrows, what, allow_1d):
    """(row length, row stride) of a float32 device tensor of `nrows` rows whose samples are contiguous; a 1-D tensor
    stands for one row where allow_1d.  The stride of a single row is never below its length."""
    if _is_f32(t):
        if t.dim() == 1 and allow_1d and nrows == 1:
            return t.shape[0], max(t.shape[0], 1)
        if t.dim() == 2 and t.shape[0] == nrows and (t.shape[1] <= 1 or t.stride(1) == 1):
            return t.shape[1], t.stride(0) if nrows > 1 else max(t.stride(0), t.shape[1])
    raise ValueError("expected a (%s, L) float32 tensor with stride(1) == 1" % what)


class _Handle:
    """owner of one object of the C ABI: `_h`, made, asked and released through the functions `_abi` + name of the
    library (`_abi`: the subclass's prefix, "clfa_stft_", "clfa_pvoc_", ...)"""
    _h = None
    _abi = None

    def _create(self, create, *args):
        """`_h` from a create function of the library; its status"""
        self._h = C.c_void_p()
        return create(C.byref(self._h), *args)

    def _fn(self, name):
        return getattr(_pkg.lib(), self._abi + name)

    def _get(self, name, *args):
        """what the object's function `name` answers"""
        return self._fn(name)(self._h, *args)

    def _text(self, name, *args):
        return self._get(name, *args).decode()

    def __del__(self):
        h, self._h = self._h, None
        if h and _pkg is not None:      # module globals are already gone at interpreter shutdown
            self._fn("destroy")(h)


class _Object(_Handle):
    """an object with the library's four status getters: its error, its log, its device workspace, its kernel"""

    def get_error(self):
        return self._get("get_error")

    def get_log(self):
        return self._text("get_log")

    def kernel_name(self):
        return self._text("kernel_name")

    def workspace_bytes(self):
        return self._get("workspace_bytes")
