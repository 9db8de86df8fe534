"""The plans of the reference's cl_fft.h, Clcfft and Clrfft, and the library's functions that belong to no object:
devices, error strings, the reference's tables, the reorder kernel and the bandwidth yardsticks."""
import ctypes as C

import numpy as np

from ._base import CL_INVALID_VALUE, CL_SUCCESS, _Object, _host, _pkg, _ptr_stream
from ._lib import check

PI = 3.141592653589793  # cl_fft.h:24
# one workgroup's record of the resident n = 65536 kernel (clfa_fft_balance_read)
BALANCE_RECORD = np.dtype([("count", np.uint32), ("xcd", np.uint32), ("stamp", np.uint64)])


def cl_error_string(err):
    """cl_fft::cl_error_string (cl_fft.cpp:298-395)"""
    return _pkg.lib().clfa_error_string(int(err)).decode()


def device_count():
    """number of devices, as clGetDeviceIDs would report (test_cfft.cpp:31)"""
    n = C.c_int(0)
    _pkg.lib().clfa_device_count(C.byref(n))
    return n.value


def device_name(device=0):
    """clGetDeviceInfo(CL_DEVICE_NAME) (test_cfft.cpp:37)"""
    buf = C.create_string_buffer(256)
    check(_pkg.lib().clfa_device_name(device, buf, 256), "device_name")
    return buf.value.decode()


def bitrev_table(n):
    """cl_fft.cpp:96-101"""
    out = np.empty(n, dtype=np.int32)
    check(_pkg.lib().clfa_bitrev_table(n, out.ctypes.data_as(C.POINTER(C.c_int))), "bitrev_table")
    return out


def twiddle_table(n, forward=True):
    """cl_fft.cpp:86-91"""
    out = np.empty(2 * n, dtype=np.float32)
    check(_pkg.lib().clfa_twiddle_table(n, int(forward), out.ctypes.data_as(C.POINTER(C.c_float))), "twiddle_table")
    return out.view(np.complex64)


def r2c_twiddle_table(m, forward=True):
    """cl_fft.cpp:233-238"""
    out = np.empty(2 * m, dtype=np.float32)
    check(_pkg.lib().clfa_r2c_twiddle_table(m, int(forward), out.ctypes.data_as(C.POINTER(C.c_float))),
          "r2c_twiddle_table")
    return out.view(np.complex64)


def reorder_device(device, out, inp, n, batch, stream=None):
    """the reference's reorder kernel (cl_fft.cpp:24-27) as an op on device memory"""
    po, stream = _ptr_stream(out, stream)
    pi, _ = _ptr_stream(inp, stream)
    return _pkg.lib().clfa_reorder_dev(device, po, pi, n, batch, stream)


class _Plan(_Object):
    _abi = "clfa_fft_"

    def get_error(self):
        """cl_fft.h:65"""
        return self._get("get_error")

    def get_log(self):
        """cl_fft.h:69"""
        return self._text("get_log")

    def alloc_host(self, shape, dtype):
        """extension (clfa_fft_host_alloc): a numpy array over page-locked host memory of the plan; transform() calls on it
        (or on contiguous slices of it) run on that memory directly, without staging copies.  The array must not outlive the
        plan; free_host(array) releases it earlier."""
        dt = np.dtype(dtype)
        n = int(np.prod(shape))
        ptr = C.c_void_p()
        e = _pkg.lib().clfa_fft_host_alloc(self._h, n * dt.itemsize, C.byref(ptr))
        if e != CL_SUCCESS:
            return None
        buf = (C.c_char * (n * dt.itemsize)).from_address(ptr.value)
        return np.frombuffer(buf, dtype=dt, count=n).reshape(shape)

    def free_host(self, array):
        return _pkg.lib().clfa_fft_host_free(self._h, array.ctypes.data)

    def exec_device(self, data, batch, stream=None):
        """in place on device memory, asynchronous on `stream` (Clcfft::fft(), cl_fft.cpp:138-151)"""
        p, stream = _ptr_stream(data, stream)
        return _pkg.lib().clfa_fft_exec_dev(self._h, p, batch, stream)

    def exec_device_oop(self, src, dst, batch, stream=None):
        """src -> dst on device memory (extension; the reference's device side is out of place too: data1 -> data2,
        cl_fft.cpp:138-151); src is left untouched"""
        ps, stream = _ptr_stream(src, stream)
        pd, _ = _ptr_stream(dst, stream)
        return _pkg.lib().clfa_fft_exec_dev_oop(self._h, ps, pd, batch, stream)

    def balance_record(self, on=True):
        """measurement aid (complex n = 65536 plans): let every later launch of the resident kernel leave one record
        per workgroup (clfa_fft_balance_record); blocks"""
        return _pkg.lib().clfa_fft_balance_record(self._h, int(bool(on)))

    def balance_read(self):
        """the records of the plan's last launch, in workgroup order (workgroup i runs on XCD i % 8): a structured array
        with the fields count (transforms processed), xcd (workgroup index % 8) and stamp (100 MHz wall clock at
        exit); waits for the device.  None if nothing is being recorded."""
        out = np.zeros(4096, dtype=BALANCE_RECORD)
        n = C.c_int(0)
        if _pkg.lib().clfa_fft_balance_read(self._h, out.ctypes.data, len(out), C.byref(n)) != CL_SUCCESS:
            return None
        return out[:n.value].copy()

    def balance_counters(self):
        """test aid (complex n = 65536 plans): (guard line before, the nine counter lines as a (9, 32) array, guard line
        after) of the shared assignment's counters in the plan's workspace, uint32 words (clfa_fft_balance_counters);
        waits for the device.  None for any other plan."""
        out = np.zeros(352, dtype=np.uint32)
        n = C.c_int(0)
        if _pkg.lib().clfa_fft_balance_counters(self._h, out.ctypes.data, len(out), C.byref(n)) != CL_SUCCESS or n.value != len(out):
            return None
        return out[:32].copy(), out[32:320].reshape(9, 32).copy(), out[320:].copy()


class Clcfft(_Plan):
    """cl_fft::Clcfft(device_id, size, fwd=true) (cl_fft.h:29-70, cl_fft.cpp:44-161)"""

    def __init__(self, device_id, size, fwd=True):
        self.N = int(size)
        self.forward = bool(fwd)
        self._create(_pkg.lib().clfa_cfft_create, int(device_id), int(size), int(bool(fwd)))

    def transform(self, c):
        """in place on complex64[..., N]; leading axes are batches (cl_fft.cpp:153-161)"""
        c = _host(c, np.complex64)
        if c.shape[-1] != self.N:
            return CL_INVALID_VALUE
        return _pkg.lib().clfa_cfft_transform(self._h, c.ctypes.data, c.size // self.N)


class Clrfft(_Plan):
    """cl_fft::Clrfft(device_id, size, fwd) (cl_fft.h:74-111, cl_fft.cpp:208-296)"""

    def __init__(self, device_id, size, fwd):
        self.size = int(size)
        self.N = self.size // 2          # the inherited member N is size/2 (cl_fft.cpp:210)
        self.forward = bool(fwd)
        self._create(_pkg.lib().clfa_rfft_create, int(device_id), int(size), int(bool(fwd)))

    def transform(self, c, r=None):
        """transform(c, r): forward reads r (float32[..., size]) and writes c
        (complex64[..., size/2]); inverse reads c and writes r.  transform(c) is
        the in-place form (cl_fft.h:104-109)."""
        c = _host(c, np.complex64)
        if c.shape[-1] != self.N:
            return CL_INVALID_VALUE
        if r is None:
            rp = c.ctypes.data
        else:
            r = _host(r, np.float32)
            if r.shape[-1] != self.size or r.size // self.size != c.size // self.N:
                return CL_INVALID_VALUE
            rp = r.ctypes.data
        return _pkg.lib().clfa_rfft_transform(self._h, c.ctypes.data, rp, c.size // self.N)


def bandwidth_probe(device_id=0, nbytes=1 << 30, launches=100):
    """sustained device-memory bandwidth in TB/s: {"read", "write", "copy", "copy_colblock"} — the
    yardsticks for the roofline fractions (clfa_bandwidth_probe in clfft_amd.h)"""
    out = {}
    for what, name in enumerate(("read", "write", "copy", "copy_colblock")):
        v = C.c_double(0.0)
        e = _pkg.lib().clfa_bandwidth_probe(int(device_id), what, int(nbytes), int(launches), C.byref(v))
        if e != CL_SUCCESS:
            raise RuntimeError("bandwidth probe: " + cl_error_string(e))
        out[name] = v.value
    return out
