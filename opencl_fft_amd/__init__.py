"""opencl_fft_amd — MI355X-native drop-in for the hot path of vlazzarini/opencl_fft.

Host-side mirror of the reference's class surface (same names, argument
meaning and integer OpenCL status codes), over the C ABI of libclfft_amd.so:

    Clcfft   cl_fft.h:29-70     complex FFT, forward scaled 1/N, inverse unscaled
    Clrfft   cl_fft.h:74-111    packed real FFT
    Clpconv  cl_conv.h:124-188  uniformly partitioned overlap-add convolution
    Cldconv  cl_dconv.h:17-66   direct convolution
    Stft     (extension)        short-time analysis / windowed overlap-add synthesis on the Clrfft layout
    PconvMatrix (extension)     convolution matrix: many inputs mixed into many outputs
    Pvoc     (extension)        phase vocoder on Stft's spectra: (amp, freq) frames both ways

Like the reference, constructors never raise: a failed setup is read back with
``get_error()`` / ``get_cl_err()`` and every method returns the status code.
Extensions the reference does not have: batches (leading array axes), many
independent channels per Clpconv object, and ``*_device`` methods that work in
place on device memory (raw pointers or torch tensors) on a given HIP stream.

PyTorch is only used by callers for device memory and streams; nothing here
imports it.
"""
import ctypes as C

import numpy as np

from ._lib import ClError, check, lib

__all__ = ["Clcfft", "Clrfft", "Clpconv", "Cldconv", "ClError", "cl_error_string", "device_count",
           "device_name", "bitrev_table", "twiddle_table", "r2c_twiddle_table", "reorder_device", "PI",
           "Stft", "packed_to_onesided", "onesided_to_packed", "PconvMatrix", "Pvoc"]

PI = 3.141592653589793  # cl_fft.h:24
CL_SUCCESS = 0
CL_INVALID_VALUE = -30


def cl_error_string(err):
    """cl_fft::cl_error_string (cl_fft.cpp:298-395)"""
    return lib().clfa_error_string(int(err)).decode()


def device_count():
    """number of devices, as clGetDeviceIDs would report (test_cfft.cpp:31)"""
    n = C.c_int(0)
    lib().clfa_device_count(C.byref(n))
    return n.value


def device_name(device=0):
    """clGetDeviceInfo(CL_DEVICE_NAME) (test_cfft.cpp:37)"""
    buf = C.create_string_buffer(256)
    check(lib().clfa_device_name(device, buf, 256), "device_name")
    return buf.value.decode()


def bitrev_table(n):
    """cl_fft.cpp:96-101"""
    out = np.empty(n, dtype=np.int32)
    check(lib().clfa_bitrev_table(n, out.ctypes.data_as(C.POINTER(C.c_int))), "bitrev_table")
    return out


def twiddle_table(n, forward=True):
    """cl_fft.cpp:86-91"""
    out = np.empty(2 * n, dtype=np.float32)
    check(lib().clfa_twiddle_table(n, int(forward), out.ctypes.data_as(C.POINTER(C.c_float))), "twiddle_table")
    return out.view(np.complex64)


def r2c_twiddle_table(m, forward=True):
    """cl_fft.cpp:233-238"""
    out = np.empty(2 * m, dtype=np.float32)
    check(lib().clfa_r2c_twiddle_table(m, int(forward), out.ctypes.data_as(C.POINTER(C.c_float))),
          "r2c_twiddle_table")
    return out.view(np.complex64)


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


def reorder_device(device, out, inp, n, batch, stream=None):
    """the reference's reorder kernel (cl_fft.cpp:24-27) as an op on device memory"""
    po, stream = _ptr_stream(out, stream)
    pi, _ = _ptr_stream(inp, stream)
    return lib().clfa_reorder_dev(device, po, pi, n, batch, stream)


class _Handle:
    """owner of one object of the C ABI: `_h`, released with the function the subclass names in `_destroy`"""
    _h = None
    _destroy = None

    def __del__(self):
        h, self._h = self._h, None
        if h and lib is not None:      # module globals are already gone at interpreter shutdown
            getattr(lib(), self._destroy)(h)


class _Plan(_Handle):
    _destroy = "clfa_fft_destroy"

    def get_error(self):
        """cl_fft.h:65"""
        return lib().clfa_fft_get_error(self._h)

    def get_log(self):
        """cl_fft.h:69"""
        return lib().clfa_fft_get_log(self._h).decode()

    def workspace_bytes(self):
        return lib().clfa_fft_workspace_bytes(self._h)

    def kernel_name(self):
        return lib().clfa_fft_kernel_name(self._h).decode()

    def alloc_host(self, shape, dtype):
        """extension (clfa_fft_host_alloc): a numpy array over page-locked host memory of the plan; transform() calls on it
        (or on contiguous slices of it) run on that memory directly, without staging copies.  The array must not outlive the
        plan; free_host(array) releases it earlier."""
        dt = np.dtype(dtype)
        n = int(np.prod(shape))
        ptr = C.c_void_p()
        e = lib().clfa_fft_host_alloc(self._h, n * dt.itemsize, C.byref(ptr))
        if e != CL_SUCCESS:
            return None
        buf = (C.c_char * (n * dt.itemsize)).from_address(ptr.value)
        return np.frombuffer(buf, dtype=dt, count=n).reshape(shape)

    def free_host(self, array):
        return lib().clfa_fft_host_free(self._h, array.ctypes.data)

    def exec_device(self, data, batch, stream=None):
        """in place on device memory, asynchronous on `stream` (Clcfft::fft(), cl_fft.cpp:138-151)"""
        p, stream = _ptr_stream(data, stream)
        return lib().clfa_fft_exec_dev(self._h, p, batch, stream)

    def exec_device_oop(self, src, dst, batch, stream=None):
        """src -> dst on device memory (extension; the reference's device side is out of place too: data1 -> data2,
        cl_fft.cpp:138-151); src is left untouched"""
        ps, stream = _ptr_stream(src, stream)
        pd, _ = _ptr_stream(dst, stream)
        return lib().clfa_fft_exec_dev_oop(self._h, ps, pd, batch, stream)


class Clcfft(_Plan):
    """cl_fft::Clcfft(device_id, size, fwd=true) (cl_fft.h:29-70, cl_fft.cpp:44-161)"""

    def __init__(self, device_id, size, fwd=True):
        self.N = int(size)
        self.forward = bool(fwd)
        h = C.c_void_p()
        lib().clfa_cfft_create(C.byref(h), int(device_id), int(size), int(bool(fwd)))
        self._h = h

    def transform(self, c):
        """in place on complex64[..., N]; leading axes are batches (cl_fft.cpp:153-161)"""
        c = _host(c, np.complex64)
        if c.shape[-1] != self.N:
            return CL_INVALID_VALUE
        return lib().clfa_cfft_transform(self._h, c.ctypes.data, c.size // self.N)


class Clrfft(_Plan):
    """cl_fft::Clrfft(device_id, size, fwd) (cl_fft.h:74-111, cl_fft.cpp:208-296)"""

    def __init__(self, device_id, size, fwd):
        self.size = int(size)
        self.N = self.size // 2          # the inherited member N is size/2 (cl_fft.cpp:210)
        self.forward = bool(fwd)
        h = C.c_void_p()
        lib().clfa_rfft_create(C.byref(h), int(device_id), int(size), int(bool(fwd)))
        self._h = h

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
        return lib().clfa_rfft_transform(self._h, c.ctypes.data, rp, c.size // self.N)


def _row_view(t, what):
    """(pointer, rows, row length, row stride) of a (rows, n) or (n,) torch tensor whose rows are contiguous"""
    if t.dim() == 1:
        t = t.unsqueeze(0)
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError("%s: expected (channels, n) with contiguous rows" % what)
    return t.data_ptr(), t.shape[0], t.shape[1], t.stride(0)


class Stft(_Handle):
    """Short-time transforms on the packed real layout of Clrfft (extension, clfa_stft in clfft_amd.h).

    fwd=True: analyze() frames (channels, samples) float32 rows (frame f = window * x[f*hop : f*hop + size], no
    padding) into (channels, F, size/2) complex64 spectra, each what Clrfft(size, True) returns for that frame.
    fwd=False: synthesize() runs Clrfft(size, False) on every frame, multiplies by the window and overlap-adds the frames
    into rows of (F - 1) * hop + size floats, optionally divided by the window envelope sum_f w^2.
    Like the other plans the constructor does not raise: get_error() / get_log() report a failed setup."""
    _destroy = "clfa_stft_destroy"

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
        h = C.c_void_p()
        lib().clfa_stft_create(C.byref(h), int(device_id), self.size, self.hop,
                               None if window is None else window.ctypes.data, int(self.forward))
        self._h = h

    def get_error(self):
        return lib().clfa_stft_get_error(self._h)

    def get_log(self):
        return lib().clfa_stft_get_log(self._h).decode()

    def kernel_name(self):
        return lib().clfa_stft_kernel_name(self._h).decode()

    def workspace_bytes(self):
        return lib().clfa_stft_workspace_bytes(self._h)

    def frames(self, samples):
        """F = 0 if samples < size else 1 + (samples - size) // hop"""
        return lib().clfa_stft_frames(self._h, int(samples))

    def samples(self, frames):
        """L = (frames - 1) * hop + size (0 for no frames)"""
        return lib().clfa_stft_samples(self._h, int(frames))

    def analyze(self, x):
        """host: float32 (channels, samples) or (samples,) -> complex64 (channels, F, size/2) (leading axis kept)"""
        x = np.ascontiguousarray(x, dtype=np.float32)
        x2 = x.reshape(1, -1) if x.ndim == 1 else x
        F = self.frames(x2.shape[1])
        out = np.zeros((x2.shape[0], F, self.M), np.complex64)
        check(lib().clfa_stft_analyze(self._h, x2.ctypes.data, x2.shape[1], x2.shape[1], x2.shape[0], out.ctypes.data),
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
        check(lib().clfa_stft_synthesize(self._h, s3.ctypes.data, s3.shape[1], s3.shape[0], out.ctypes.data, L,
                                         int(bool(normalize))), "Stft.synthesize")
        return out[0] if spec.ndim == 2 else out

    def analyze_device(self, signal, out, stream=None):
        """torch: signal (channels, samples) float32 (row stride taken from the tensor: padded rows work) ->
        out (channels, F, size/2) complex64, contiguous; asynchronous on `stream` (default: the current stream)"""
        p, rows, n, stride = _row_view(signal, "signal")
        if not out.is_contiguous():
            raise ValueError("spectra tensor must be contiguous")
        return lib().clfa_stft_analyze_dev(self._h, p, stride, n, rows, out.data_ptr(), _stream_of(signal, stream))

    def synthesize_device(self, spectra, out, normalize=False, stream=None):
        """torch: spectra (channels, F, size/2) complex64, contiguous -> out (channels, >= (F - 1) * hop + size) float32,
        row stride from the tensor; asynchronous on `stream`"""
        if not spectra.is_contiguous():
            raise ValueError("spectra tensor must be contiguous")
        s3 = spectra if spectra.dim() == 3 else spectra.unsqueeze(0)
        p, rows, _, stride = _row_view(out, "signal")
        if rows != s3.shape[0]:
            raise ValueError("out has %d rows for %d channels" % (rows, s3.shape[0]))
        return lib().clfa_stft_synthesize_dev(self._h, spectra.data_ptr(), s3.shape[1], s3.shape[0], p, stride,
                                              int(bool(normalize)), _stream_of(out, stream))


class Pvoc(_Handle):
    """Phase vocoder on the spectra of Stft (extension, clfa_pvoc in clfft_amd.h): analyze() reads (channels, F, size/2)
    complex64 spectra as (channels, F, size/2 + 1, 2) float32 frames of (amp, freq in Hz) per bin, synthesize() turns such
    frames back into spectra.  The object carries the last spectrum (analysis) and an integer phase per bin (synthesis)
    from call to call, so a stream may be cut into calls anywhere; reset() returns both to their start.
    adsyn() is the second way back to sound: an oscillator per bin, summed straight into samples (a state of its own).
    describe() turns frames into control values: eight descriptors per frame (the previous frame's amps carried along).
    Like the other objects the constructor does not raise, and every call returns its status."""
    _destroy = "clfa_pvoc_destroy"

    def __init__(self, device_id, size, hop, sr, channels=1):
        self.size, self.hop, self.sr, self.channels = int(size), int(hop), float(sr), int(channels)
        self.M = self.size // 2
        h = C.c_void_p()
        lib().clfa_pvoc_create(C.byref(h), int(device_id), self.size, self.hop, self.sr, self.channels)
        self._h = h

    def get_error(self):
        return lib().clfa_pvoc_get_error(self._h)

    def get_log(self):
        return lib().clfa_pvoc_get_log(self._h).decode()

    def kernel_name(self, synthesis=False):
        return lib().clfa_pvoc_kernel_name(self._h, int(bool(synthesis))).decode()

    def workspace_bytes(self):
        return lib().clfa_pvoc_workspace_bytes(self._h)

    def scan_chunk(self):
        """frames per chunk of the synthesis' phase scan (fixed)"""
        return lib().clfa_pvoc_scan_chunk()

    def reset(self):
        return lib().clfa_pvoc_reset(self._h)

    def read_phase(self):
        """the synthesis state: uint32 (channels, size/2 + 1), units of 2^-32 turn (blocking)"""
        out = np.zeros((self.channels, self.M + 1), np.uint32)
        check(lib().clfa_pvoc_read_phase(self._h, out.ctypes.data), "Pvoc.read_phase")
        return out

    def read_prev(self):
        """the analysis state: complex64 (channels, size/2 + 1), z of the last frame analysed (blocking)"""
        out = np.zeros((self.channels, self.M + 1), np.complex64)
        check(lib().clfa_pvoc_read_prev(self._h, out.ctypes.data), "Pvoc.read_prev")
        return out

    def _shapes(self, spectra, frames):
        """F if `spectra` is (channels, F, M) (or (F, M) for one channel) and `frames` the matching (.., F, M + 1, 2), else None"""
        s, F = tuple(spectra.shape), self._frames_shape(frames.shape)
        if len(s) == 2 and self.channels == 1:
            s = (1,) + s
        return F if F is not None and s == (self.channels, F, self.M) else None

    def _device_call(self, fn, spectra, frames, src, dst, stream):
        import torch
        F = self._shapes(spectra, frames)
        if (F is None or spectra.dtype != torch.complex64 or frames.dtype != torch.float32
                or not spectra.is_contiguous() or not frames.is_contiguous()):
            return CL_INVALID_VALUE
        return fn(self._h, src.data_ptr(), dst.data_ptr(), F, _stream_of(dst, stream))

    def analyze_device(self, spectra, frames_out, stream=None):
        """torch: spectra (channels, F, size/2) complex64 -> frames_out (channels, F, size/2 + 1, 2) float32, both
        contiguous (anything else: CL_INVALID_VALUE); asynchronous on `stream` (default: the current stream)"""
        return self._device_call(lib().clfa_pvoc_analyze_dev, spectra, frames_out, spectra, frames_out, stream)

    def synthesize_device(self, frames, spectra_out, stream=None):
        """torch: frames (channels, F, size/2 + 1, 2) float32 -> spectra_out (channels, F, size/2) complex64"""
        return self._device_call(lib().clfa_pvoc_synthesize_dev, spectra_out, frames, frames, spectra_out, stream)

    def analyze(self, spectra):
        """host: complex64 (channels, F, size/2) (or (F, size/2) for one channel) -> float32 (.., F, size/2 + 1, 2)"""
        spectra = np.ascontiguousarray(spectra, dtype=np.complex64)
        out = np.zeros(spectra.shape[:-1] + (self.M + 1, 2), np.float32)
        F = self._shapes(spectra, out)
        if F is None:
            raise ValueError("spectra must be (%d, F, %d)" % (self.channels, self.M))
        check(lib().clfa_pvoc_analyze(self._h, spectra.ctypes.data, out.ctypes.data, F), "Pvoc.analyze")
        return out

    def synthesize(self, frames):
        """host: float32 (channels, F, size/2 + 1, 2) (or (F, size/2 + 1, 2)) -> complex64 (.., F, size/2)"""
        frames, F = self._host_frames(frames)
        out = np.zeros(frames.shape[:-2] + (self.M,), np.complex64)
        check(lib().clfa_pvoc_synthesize(self._h, frames.ctypes.data, out.ctypes.data, F), "Pvoc.synthesize")
        return out

    # ---- frames -> frames: pitch scale, frequency shift, timed read (stateless; clfft_amd.h) ----

    def ops_kernel_name(self, op, keepform=False):
        """op "scale", "shift" or "read" -> "k_pvoc_map" / "k_pvoc_formant" (keepform) / "k_pvoc_read" ("" for a failed object)"""
        return lib().clfa_pvoc_ops_kernel_name(self._h, {"scale": 0, "shift": 1, "read": 2}.get(op, -1),
                                               int(bool(keepform))).decode()

    def _frames_shape(self, shape):
        """F of a (channels, F, M + 1, 2) shape (or (F, M + 1, 2) for one channel), else None"""
        f = tuple(shape)
        if len(f) == 3 and self.channels == 1:
            f = (1,) + f
        if len(f) != 4 or f[0] != self.channels or f[2:] != (self.M + 1, 2):
            return None
        return f[1]

    def _host_frames(self, frames):
        """(the frames as a contiguous float32 array, F); ValueError for another shape"""
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        F = self._frames_shape(frames.shape)
        if F is None:
            raise ValueError("frames must be (%d, F, %d, 2)" % (self.channels, self.M + 1))
        return frames, F

    @staticmethod
    def _is_f32(t, shape):
        """a device call's tensor: float32, contiguous, of this shape"""
        import torch
        return t.dtype == torch.float32 and tuple(t.shape) == tuple(shape) and t.is_contiguous()

    def _device_frames(self, *tensors):
        """F if every tensor holds F frames for a device call ((channels, F, M + 1, 2), or (F, M + 1, 2) for one channel,
        float32, contiguous), else None"""
        F = self._frames_shape(tensors[0].shape)
        ok = F is not None and all(self._frames_shape(t.shape) == F and self._is_f32(t, t.shape) for t in tensors)
        return F if ok else None

    def _per_frame(self, par, F, device):
        """a per-frame value of a device call as a float32 (F,) tensor: a plain number becomes F copies on `device`;
        None for a tensor of another kind"""
        import torch
        if not hasattr(par, "data_ptr"):
            par = torch.full((F,), float(par), dtype=torch.float32, device=device)
        return par if self._is_f32(par, (F,)) else None

    def _per_frame_ptrs(self, pars, F, device):
        """the per-frame parameters of a device call as (their pointers, the tensors to keep until the call is made): a
        number becomes a tensor of F copies, None a NULL; (None, None) if one is a tensor of another kind"""
        keep = [None if par is None else self._per_frame(par, F, device) for par in pars]
        if any(t is None and par is not None for t, par in zip(keep, pars)):
            return None, None
        return [None if t is None else t.data_ptr() for t in keep], keep

    def _per_frame_host(self, par, F):
        """a per-frame value of a host call (a number or an array of F) as a contiguous float32 (F,) array"""
        return np.ascontiguousarray(np.broadcast_to(np.asarray(par, dtype=np.float32), (F,)))

    @staticmethod
    def _op_code(ops, op):
        """an op given by its name or its code, as the code (-1 for an unknown name)"""
        return ops.get(op, -1) if isinstance(op, str) else int(op)

    def _ops_device(self, frames_in, frames_out, par, stream):
        """(Fin, Fout, the per-frame pointer, stream, what to keep) of a device call, None for bad tensors; a plain number
        becomes a tensor of Fout copies"""
        Fin, Fout = self._device_frames(frames_in), self._device_frames(frames_out)
        if Fin is None or Fout is None:
            return None
        ptrs, keep = self._per_frame_ptrs((par,), Fout, frames_out.device)
        return None if ptrs is None else (Fin, Fout, ptrs[0], _stream_of(frames_out, stream), keep)

    def scale_device(self, frames_in, frames_out, scale, keepform=False, gain=1.0, coefs=80, stream=None):
        """pitch scale (Csound's pvscale): torch frames (channels, F, size/2 + 1, 2) float32 -> frames_out of the same
        shape; scale: a number or a float32 device tensor (F,), each in [0.25, 4]; keepform: the formants (the
        cepstral envelope of `coefs` coefficients) stay where they are.  Asynchronous on `stream`."""
        a = self._ops_device(frames_in, frames_out, scale, stream)
        if a is None or a[0] != a[1]:
            return CL_INVALID_VALUE
        return lib().clfa_pvoc_scale_dev(self._h, frames_in.data_ptr(), frames_out.data_ptr(), a[1], a[2],
                                         int(bool(keepform)), float(gain), int(coefs), a[3])

    def shift_device(self, frames_in, frames_out, shift, lowest_bin=1, keepform=False, gain=1.0, coefs=80, stream=None):
        """frequency shift (Csound's pvshift): the bins from lowest_bin up move by shift Hz (a number or a float32
        device tensor (F,)), rounded to whole bins; the bins below are copied"""
        a = self._ops_device(frames_in, frames_out, shift, stream)
        if a is None or a[0] != a[1]:
            return CL_INVALID_VALUE
        return lib().clfa_pvoc_shift_dev(self._h, frames_in.data_ptr(), frames_out.data_ptr(), a[1], a[2],
                                         int(lowest_bin), int(bool(keepform)), float(gain), int(coefs), a[3])

    def read_device(self, frames_in, pos, frames_out, stream=None):
        """timed read (Csound's pvsbufread): frames_out[:, g] = frames_in read at the position pos[g] in frames (float32
        device tensor (Fout,)), clamped to the ends and interpolated linearly between neighbouring frames"""
        a = self._ops_device(frames_in, frames_out, pos, stream)
        if a is None or not hasattr(pos, "data_ptr"):
            return CL_INVALID_VALUE
        return lib().clfa_pvoc_read_dev(self._h, frames_in.data_ptr(), a[0], a[2], frames_out.data_ptr(),
                                        a[1], a[3])

    def _ops_host(self, frames, par, Fout=None):
        frames, Fin = self._host_frames(frames)
        Fout = Fin if Fout is None else Fout
        return frames, Fin, self._per_frame_host(par, Fout), np.zeros(frames.shape[:-3] + (Fout, self.M + 1, 2), np.float32)

    def scale(self, frames, scale, keepform=False, gain=1.0, coefs=80):
        """host form of scale_device, blocking: returns the new frames; a value of `scale` outside [0.25, 4] raises
        ClError(CL_INVALID_VALUE)"""
        frames, F, par, out = self._ops_host(frames, scale)
        check(lib().clfa_pvoc_scale(self._h, frames.ctypes.data, out.ctypes.data, F, par.ctypes.data, int(bool(keepform)),
                                    float(gain), int(coefs)), "Pvoc.scale")
        return out

    def shift(self, frames, shift, lowest_bin=1, keepform=False, gain=1.0, coefs=80):
        """host form of shift_device, blocking"""
        frames, F, par, out = self._ops_host(frames, shift)
        check(lib().clfa_pvoc_shift(self._h, frames.ctypes.data, out.ctypes.data, F, par.ctypes.data, int(lowest_bin),
                                    int(bool(keepform)), float(gain), int(coefs)), "Pvoc.shift")
        return out

    def read(self, frames, pos):
        """host form of read_device, blocking: pos float32 (Fout,) -> frames (.., Fout, size/2 + 1, 2)"""
        pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1)
        frames, Fin, par, out = self._ops_host(frames, pos, pos.size)
        check(lib().clfa_pvoc_read(self._h, frames.ctypes.data, Fin, par.ctypes.data, out.ctypes.data, pos.size), "Pvoc.read")
        return out

    # ---- two streams of frames -> frames: cross, morph, filter, mix, vocode (stateless; clfft_amd.h) ----

    _PAIR_OPS = {"cross": 0, "morph": 1, "filter": 2, "mix": 3, "vocode": 4}

    def pair_kernel_name(self, op):
        """op "cross", "morph", "filter", "mix" (or 0..3) -> "k_pvoc_pair", "vocode" (4) -> "k_pvoc_vocode" ("" for a failed
        object or an unknown op)"""
        return lib().clfa_pvoc_pair_kernel_name(self._h, self._op_code(self._PAIR_OPS, op)).decode()

    def _pair_device(self, op, a, b, out, p, q, coefs, stream):
        """one two-input device call; p, q: numbers or float32 device tensors (F,), None for mix"""
        F = self._device_frames(out, a, b)
        ptrs, keep = (None, None) if F is None else self._per_frame_ptrs((p, q), F, out.device)
        if ptrs is None:
            return CL_INVALID_VALUE
        return lib().clfa_pvoc_pair_dev(self._h, op, a.data_ptr(), b.data_ptr(), out.data_ptr(), F, ptrs[0], ptrs[1],
                                        int(coefs), _stream_of(out, stream))

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
        a, F = self._host_frames(a)
        b, Fb = self._host_frames(b)
        if Fb != F or a.shape != b.shape:
            raise ValueError("a and b must have the same shape")
        out = np.zeros(a.shape, np.float32)
        p, q = (None if x is None else self._per_frame_host(x, F) for x in (p, q))
        check(lib().clfa_pvoc_pair(self._h, op, a.ctypes.data, b.ctypes.data, out.ctypes.data, F,
                                   None if p is None else p.ctypes.data, None if q is None else q.ctypes.data, int(coefs)), what)
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
        return lib().clfa_pvoc_shape_kernel_name(self._h, self._op_code(self._SHAPE_OPS, op)).decode()

    def _shape_device(self, op, frames_in, frames_out, cols, table, flags, lowest_bin, coefs, stream):
        """one shaping device call; cols: the op's per-frame values (numbers or float32 device tensors (F,)), stacked
        into the (F, 4) rows the library reads; table: None or a float32 device tensor (size/2 + 1,)"""
        import torch
        F = self._device_frames(frames_out, frames_in)
        if F is None:
            return CL_INVALID_VALUE
        rows = torch.zeros((F, 4), dtype=torch.float32, device=frames_out.device)
        for i, par in enumerate(cols):
            if hasattr(par, "data_ptr"):
                par = self._per_frame(par, F, frames_out.device)
                if par is None:
                    return CL_INVALID_VALUE
                rows[:, i] = par
            else:
                rows[:, i] = float(par)
        if table is not None and not (hasattr(table, "data_ptr") and self._is_f32(table, (self.M + 1,))):
            return CL_INVALID_VALUE
        return lib().clfa_pvoc_shape_dev(self._h, op, frames_in.data_ptr(), frames_out.data_ptr(), F, rows.data_ptr(),
                                         None if table is None else table.data_ptr(), int(flags), int(lowest_bin),
                                         int(coefs), _stream_of(frames_out, stream))

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
        frames, F = self._host_frames(frames)
        out = np.zeros(frames.shape, np.float32)
        rows = np.zeros((F, 4), np.float32)
        for i, par in enumerate(cols):
            rows[:, i] = self._per_frame_host(par, F)
        if table is not None:
            table = np.ascontiguousarray(table, dtype=np.float32)
            if table.shape != (self.M + 1,):
                raise ValueError("table must be (%d,)" % (self.M + 1))
        check(lib().clfa_pvoc_shape(self._h, op, frames.ctypes.data, out.ctypes.data, F, rows.ctypes.data,
                                    None if table is None else table.ctypes.data, int(flags), int(lowest_bin),
                                    int(coefs)), what)
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
        return lib().clfa_pvoc_time_kernel_name(self._h, self._op_code(self._TIME_OPS, op)).decode()

    def time_state_bytes(self):
        """device memory of the three carried states, the blur's spare included"""
        return lib().clfa_pvoc_time_state_bytes(self._h)

    def blur_setup(self, max_frames):
        """allocates and resets the blur's history for windows of up to max_frames (1..4096) frames (blocking)"""
        return lib().clfa_pvoc_blur_setup(self._h, int(max_frames))

    def blur_max_frames(self):
        """max_frames of the last blur_setup, 0 before"""
        return lib().clfa_pvoc_blur_max_frames(self._h)

    def time_state(self, op):
        """the carried state of op "blur", "smooth" or "freeze" (blocking), float32: the blur's history (channels,
        max_frames - 1, size/2 + 1, 2), oldest frame first; the smoothing's y and the freeze's held (channels, size/2 + 1, 2)"""
        code = self._op_code(self._TIME_OPS, op)
        shape = (self.channels, max(self.blur_max_frames() - 1, 0)) if code == 0 else (self.channels,)
        out = np.zeros(shape + (self.M + 1, 2), np.float32)
        check(lib().clfa_pvoc_time_read_state(self._h, code, out.ctypes.data), "Pvoc.time_state")
        return out

    def _time_device(self, op, frames_in, frames_out, p, q, stream):
        """one device call along the frames; p, q: numbers or float32 device tensors (F,), q None for blur"""
        F = self._device_frames(frames_out, frames_in)
        ptrs, keep = (None, None) if F is None else self._per_frame_ptrs((p, q), F, frames_out.device)
        if ptrs is None:
            return CL_INVALID_VALUE
        return lib().clfa_pvoc_time_dev(self._h, op, frames_in.data_ptr(), frames_out.data_ptr(), F, ptrs[0], ptrs[1],
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
        frames, F = self._host_frames(frames)
        out = np.zeros(frames.shape, np.float32)
        p, q = (None if x is None else self._per_frame_host(x, F) for x in (p, q))
        check(lib().clfa_pvoc_time(self._h, op, frames.ctypes.data, out.ctypes.data, F, p.ctypes.data,
                                   None if q is None else q.ctypes.data), what)
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
        return lib().clfa_pvoc_desc_kernel_name(self._h).decode()

    def desc_state_bytes(self):
        """device memory of the descriptors' carried state"""
        return lib().clfa_pvoc_desc_state_bytes(self._h)

    def desc_state(self):
        """the descriptors' carried state (blocking): float32 (channels, size/2 + 1), the amps of the stream's last frame"""
        out = np.zeros((self.channels, self.M + 1), np.float32)
        check(lib().clfa_pvoc_desc_read_state(self._h, out.ctypes.data), "Pvoc.desc_state")
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
        o = tuple(out.shape)
        if len(o) == 2 and self.channels == 1:
            o = (1,) + o
        if F is None or o != (self.channels, F, 8) or not self._is_f32(out, out.shape):
            return CL_INVALID_VALUE
        first_bin, nbins, _ = self._selection(first_bin, nbins, 1)
        return lib().clfa_pvoc_desc_dev(self._h, frames_in.data_ptr(), out.data_ptr(), F, first_bin, nbins,
                                        int(bool(rectify)), _stream_of(out, stream))

    def describe(self, frames, first_bin=0, nbins=None, rectify=False):
        """host form of describe_device, blocking: float32 (channels, F, size/2 + 1, 2) (or (F, size/2 + 1, 2)) -> float32
        (.., F, 8)"""
        frames, F = self._host_frames(frames)
        out = np.zeros(frames.shape[:-2] + (8,), np.float32)
        first_bin, nbins, _ = self._selection(first_bin, nbins, 1)
        check(lib().clfa_pvoc_desc(self._h, frames.ctypes.data, out.ctypes.data, F, first_bin, nbins, int(bool(rectify))),
              "Pvoc.describe")
        return out

    # ---- frames -> frames: the N loudest bins of every frame (Csound's pvstrace; stateless; clfft_amd.h) ----

    TRACE_RESIDUAL = 1

    def trace_kernel_name(self):
        """ "k_pvoc_trace" ("" for a failed object)"""
        return lib().clfa_pvoc_trace_kernel_name(self._h).decode()

    def trace_device(self, frames_in, frames_out, n, first_bin=0, nbins=None, residual=False, bins_out=None, stream=None):
        """torch: frames (channels, F, size/2 + 1, 2) float32, contiguous -> frames_out of the same shape: of the bins
        first_bin .. first_bin + nbins - 1 (default: up to size/2) of every frame the floor(n) loudest keep their amp and the
        others get +0; residual: the other way round.  Equal amps: the lower bin is the louder one, so exactly floor(n) bins
        are selected (Csound's pvstrace keeps all ties); a NaN amp is never selected.  n: a number or a float32 device tensor
        (F,), shared by the channels.  bins_out: an int32 device tensor (channels, F, L), contiguous ((F, L) for one
        channel), that takes the selected bins in ascending order, the first L of them, then -1.  Asynchronous on `stream`."""
        import torch
        F = self._device_frames(frames_in, frames_out)
        if F is None:
            return CL_INVALID_VALUE
        ptrs, keep = self._per_frame_ptrs((n,), F, frames_out.device)
        if ptrs is None:
            return CL_INVALID_VALUE
        bins, L = None, 0
        if bins_out is not None:
            b = tuple(bins_out.shape)
            if len(b) == 2 and self.channels == 1:
                b = (1,) + b
            if (len(b) != 3 or b[:2] != (self.channels, F) or b[2] < 1 or bins_out.dtype != torch.int32
                    or not bins_out.is_contiguous() or bins_out.device != frames_out.device):
                return CL_INVALID_VALUE
            bins, L = bins_out.data_ptr(), b[2]
        first_bin, nbins, _ = self._selection(first_bin, nbins, 1)
        return lib().clfa_pvoc_trace_dev(self._h, frames_in.data_ptr(), frames_out.data_ptr(), ptrs[0], bins, L, F, first_bin,
                                         nbins, self.TRACE_RESIDUAL if residual else 0, _stream_of(frames_out, stream))

    def trace(self, frames, n, first_bin=0, nbins=None, residual=False, list_n=0):
        """host form of trace_device, blocking: float32 (channels, F, size/2 + 1, 2) (or (F, size/2 + 1, 2)) -> the new
        frames, or (frames, bins) with bins int32 (.., F, list_n) when list_n > 0"""
        frames, F = self._host_frames(frames)
        n = self._per_frame_host(n, F)
        out = np.zeros_like(frames)
        list_n = int(list_n)
        bins = np.full(frames.shape[:-2] + (list_n,), -1, np.int32) if list_n > 0 else None
        first_bin, nbins, _ = self._selection(first_bin, nbins, 1)
        check(lib().clfa_pvoc_trace(self._h, frames.ctypes.data, out.ctypes.data, n.ctypes.data,
                                    None if bins is None else bins.ctypes.data, list_n, F, first_bin, nbins,
                                    self.TRACE_RESIDUAL if residual else 0), "Pvoc.trace")
        return out if bins is None else (out, bins)

    # ---- frames -> samples: the oscillator bank (Csound's pvsadsyn; a state of its own; clfft_amd.h) ----

    def adsyn_kernel_name(self):
        """ "k_adsyn_osc" ("" for a failed object)"""
        return lib().clfa_pvoc_adsyn_kernel_name(self._h).decode()

    def adsyn_workspace_bytes(self):
        return lib().clfa_pvoc_adsyn_workspace_bytes(self._h)

    def adsyn_tile_bins(self):
        """oscillators per LDS tile of k_adsyn_osc (fixed)"""
        return lib().clfa_pvoc_adsyn_tile_bins()

    def adsyn_state(self):
        """the oscillator bank's state (blocking): (P uint64 in 2^-64 turn, W int32 in 2^-32 turn per sample, A float32),
        each (channels, size/2 + 1)"""
        shape = (self.channels, self.M + 1)
        P, W, A = np.zeros(shape, np.uint64), np.zeros(shape, np.int32), np.zeros(shape, np.float32)
        check(lib().clfa_pvoc_adsyn_read_state(self._h, P.ctypes.data, W.ctypes.data, A.ctypes.data), "Pvoc.adsyn_state")
        return P, W, A

    def _selection(self, first_bin, nbins, step):
        first_bin, step = int(first_bin), int(step)
        if nbins is None:      # every bin from first_bin up that the step reaches
            nbins = (self.M - first_bin) // step + 1 if step >= 1 and 0 <= first_bin <= self.M else 0
        return first_bin, int(nbins), step

    def adsyn_device(self, frames, out, fmod=None, first_bin=0, nbins=None, step=1, gain=1.0, stream=None):
        """torch: frames (channels, F, size/2 + 1, 2) float32, contiguous -> out (channels, n >= F * hop) float32 with
        contiguous rows (one row for one channel): frame f yields the samples [f hop, (f + 1) hop), summed over the
        oscillators of the bins first_bin + i * step, i < nbins (default: all that fit), times gain.  fmod: a frequency
        multiplier, a number or a float32 device tensor (F,); None: none.  Asynchronous on `stream`."""
        import torch
        F = self._device_frames(frames)
        if F is None or out.dtype != torch.float32:
            return CL_INVALID_VALUE
        p, rows, n, stride = _row_view(out, "out")
        if rows != self.channels or n < F * self.hop:
            return CL_INVALID_VALUE
        ptrs, keep = self._per_frame_ptrs((fmod,), F, out.device)
        if ptrs is None:
            return CL_INVALID_VALUE
        first_bin, nbins, step = self._selection(first_bin, nbins, step)
        return lib().clfa_pvoc_adsyn_dev(self._h, frames.data_ptr(), F, ptrs[0], first_bin, nbins, step, float(gain), p,
                                         stride if rows > 1 else n, _stream_of(out, stream))

    def adsyn(self, frames, fmod=None, first_bin=0, nbins=None, step=1, gain=1.0):
        """host form of adsyn_device, blocking: float32 (channels, F, size/2 + 1, 2) (or (F, size/2 + 1, 2)) -> float32
        (.., F * hop)"""
        frames, F = self._host_frames(frames)
        if fmod is not None:
            fmod = self._per_frame_host(fmod, F)
        out = np.zeros(frames.shape[:-3] + (F * self.hop,), np.float32)
        first_bin, nbins, step = self._selection(first_bin, nbins, step)
        check(lib().clfa_pvoc_adsyn(self._h, frames.ctypes.data, F, None if fmod is None else fmod.ctypes.data, first_bin,
                                    nbins, step, float(gain), out.ctypes.data, F * self.hop), "Pvoc.adsyn")
        return out


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


def bandwidth_probe(device_id=0, nbytes=1 << 30, launches=100):
    """sustained device-memory bandwidth in TB/s: {"read", "write", "copy", "copy_colblock"} — the
    yardsticks for the roofline fractions (clfa_bandwidth_probe in clfft_amd.h)"""
    out = {}
    for what, name in enumerate(("read", "write", "copy", "copy_colblock")):
        v = C.c_double(0.0)
        e = lib().clfa_bandwidth_probe(int(device_id), what, int(nbytes), int(launches), C.byref(v))
        if e != CL_SUCCESS:
            raise RuntimeError("bandwidth probe: " + cl_error_string(e))
        out[name] = v.value
    return out


def _block_rows(t, nrows, what, allow_1d):
    """(row length, row stride) of a float32 device tensor of `nrows` rows whose samples are contiguous; a 1-D tensor
    stands for one row where allow_1d.  The stride of a single row is never below its length."""
    if str(t.dtype) == "torch.float32":
        if t.dim() == 1 and allow_1d and nrows == 1:
            return t.shape[0], max(t.shape[0], 1)
        if t.dim() == 2 and t.shape[0] == nrows and (t.shape[1] <= 1 or t.stride(1) == 1):
            return t.shape[1], t.stride(0) if nrows > 1 else max(t.stride(0), t.shape[1])
    raise ValueError("expected a (%s, L) float32 tensor with stride(1) == 1" % what)


class _BlockConv(_Handle):
    """What Clpconv and Cldconv share: blocks of float32[channels, block length] through the C ABI functions
    `_abi` + name, the block length being the attribute `_block` names (pts / vsize)."""
    _abi = None
    _block = None

    def _fn(self, name):
        return getattr(lib(), self._abi + name)

    def _report(self, e):
        # error callback by value, default prints unless user data is given (cl_conv.h:142-145)
        msg = cl_error_string(e)
        if self._errs is not None:
            self._errs(msg, self._udata)
        elif self._udata is None:
            print(msg)

    def cl_error_string(self, err):
        return cl_error_string(err)

    def convolution(self, output, input1, input2=None):
        """convolution(out, in) (cl_conv.cpp:393-458, cl_dconv.cpp:109-133) or the time-varying
        convolution(out, in1, in2) (cl_conv.cpp:460-548, cl_dconv.cpp:134-148); float32[channels, block length]"""
        output = _host(output, np.float32)
        a = np.ascontiguousarray(input1, dtype=np.float32)
        n = self.channels * getattr(self, self._block)
        if output.size != n or a.size != n:
            return CL_INVALID_VALUE
        if input2 is None:
            return self._fn("convolution")(self._h, output.ctypes.data, a.ctypes.data)
        b = np.ascontiguousarray(input2, dtype=np.float32)
        if b.size != n:
            return CL_INVALID_VALUE
        return self._fn("convolution_tv")(self._h, output.ctypes.data, a.ctypes.data, b.ctypes.data)

    # ---- many blocks per call (extension): clfa_pconv_ / clfa_dconv_process_blocks_dev, include/clfft_amd.h
    def blocks_workspace_bytes(self):
        return self._fn("blocks_workspace_bytes")(self._h)

    def convolution_blocks(self, output, input1, input2=None):
        """whole signals: float32[channels, nblocks * block length] (or 1-D for one channel); equals nblocks calls of
        convolution(), blocking"""
        blk = getattr(self, self._block)
        output = _host(output, np.float32)
        a = np.ascontiguousarray(input1, dtype=np.float32)
        if a.ndim == 1:
            a = a[None, :]
        if a.ndim != 2 or a.shape[0] != self.channels or a.shape[1] % blk or output.size != a.size:
            return CL_INVALID_VALUE
        b = None
        if input2 is not None:
            b = np.ascontiguousarray(input2, dtype=np.float32)
            if b.size != a.size:
                return CL_INVALID_VALUE
        return self._fn("convolution_blocks")(self._h, output.ctypes.data, a.ctypes.data,
                                              None if b is None else b.ctypes.data, a.shape[1] // blk)

    def process_blocks_device(self, out, in1, in2=None, stream=None):
        """device tensors (channels, L) of float32 (1-D for one channel), stride(1) == 1, L a multiple of the block
        length; the row stride of each is its stride(0) (views into longer rows are fine).  Asynchronous on `stream`."""
        blk = getattr(self, self._block)
        (lo, so), (l1, s1) = (_block_rows(t, self.channels, "channels", True) for t in (out, in1))
        l2, s2 = _block_rows(in2, self.channels, "channels", True) if in2 is not None else (l1, s1)
        if lo != l1 or l2 != l1 or l1 % blk:
            return CL_INVALID_VALUE
        if s2 != s1:
            return CL_INVALID_VALUE   # one stride for both inputs (the ABI's in_stride)
        return self._fn("process_blocks_dev")(self._h, out.data_ptr(), so, in1.data_ptr(),
                                              in2.data_ptr() if in2 is not None else None, s1, l1 // blk,
                                              _stream_of(in1, stream))


class Clpconv(_BlockConv):
    """cl_conv::Clpconv(device_id, cvs, pts, errs=NULL, uData=NULL, ...) (cl_conv.h:124-188)

    `channels` (extension) runs that many independent instances in one object;
    arrays then carry a leading channel axis."""
    _destroy, _abi, _block = "clfa_pconv_destroy", "clfa_pconv_", "pts"

    def __init__(self, device_id, cvs, pts, errs=None, uData=None, channels=1):
        self.pts = int(pts)
        self.channels = int(channels)
        self._errs, self._udata = errs, uData
        h = C.c_void_p()
        e = lib().clfa_pconv_create(C.byref(h), int(device_id), int(cvs), int(pts), int(channels))
        self._h = h
        if e != CL_SUCCESS:
            self._report(e)

    def get_cl_err(self):
        """cl_conv.h:187"""
        return lib().clfa_pconv_get_error(self._h)

    nparts = property(lambda s: lib().clfa_pconv_nparts(s._h))
    wp = property(lambda s: lib().clfa_pconv_wp(s._h))
    wp2 = property(lambda s: lib().clfa_pconv_wp2(s._h))

    def state_bytes(self):
        return lib().clfa_pconv_state_bytes(self._h)

    def kernel_name(self):
        return lib().clfa_pconv_kernel_name(self._h).decode()

    def push_ir(self, ir):
        """cl_conv.cpp:353-388; ir: float32[channels, nparts*pts] (or 1-D for one channel)"""
        ir = np.ascontiguousarray(ir, dtype=np.float32)
        need = self.nparts * self.pts
        if ir.ndim == 1:
            ir = ir[None, :]
        if ir.shape[0] != self.channels or ir.shape[1] < need:
            return CL_INVALID_VALUE
        ir = np.ascontiguousarray(ir[:, :need])
        return lib().clfa_pconv_push_ir(self._h, ir.ctypes.data)

    def push_ir_device(self, ir, stream=None):
        """ir: device tensor (channels, >= nparts*pts) of float32, rows contiguous; a (channels, cvs)
        tensor with cvs not a multiple of pts is fine (the remainder of every row is ignored, like the
        reference's floor(cvs / pts), cl_conv.cpp:143)"""
        need = self.nparts * self.pts
        shape, strides = tuple(ir.shape), tuple(ir.stride())
        if ir.dim() == 1:
            shape, strides = (1,) + shape, (shape[0],) + strides
        if (len(shape) != 2 or shape[0] != self.channels or shape[1] < need or strides[1] != 1
                or (shape[0] > 1 and strides[0] < need) or str(ir.dtype) != "torch.float32"):
            return -30   # CL_INVALID_VALUE
        p, stream = _ptr_stream(ir, stream)
        return lib().clfa_pconv_push_ir_dev(self._h, p, strides[0], stream)

    def process_device(self, out, in1, in2=None, stream=None):
        po, stream = _ptr_stream(out, stream)
        p1, _ = _ptr_stream(in1, stream)
        p2 = _ptr_stream(in2, stream)[0] if in2 is not None else None
        return lib().clfa_pconv_process_dev(self._h, po, p1, p2, stream)

    def blocks_kernel_name(self):
        """"k_pconvb_mac" (partitions of 32..4096 samples) or "loop" (the single-block route once per block)"""
        return lib().clfa_pconv_blocks_kernel_name(self._h).decode()


class PconvMatrix(_Handle):
    """Convolution matrix (extension, clfa_pconv_matrix in clfft_amd.h): `inputs` signals mixed into `outputs` signals,
    y_o = sum_i x_i * h_{o,i}, by uniformly partitioned overlap-add convolution with static responses.  Block j of output
    o is the sum over i of what Clpconv(device_id, cvs, pts) holding h_{o,i} returns for block j of input i.  pts is a
    power of two, 32..4096.  Like the other objects the constructor does not raise: get_error() / get_log() report a
    failed setup."""
    _destroy = "clfa_pconv_matrix_destroy"

    def __init__(self, device_id, cvs, pts, inputs, outputs):
        self.cvs, self.pts, self.inputs, self.outputs = int(cvs), int(pts), int(inputs), int(outputs)
        h = C.c_void_p()
        lib().clfa_pconv_matrix_create(C.byref(h), int(device_id), self.cvs, self.pts, self.inputs, self.outputs)
        self._h = h

    def get_error(self):
        return lib().clfa_pconv_matrix_get_error(self._h)

    def get_log(self):
        return lib().clfa_pconv_matrix_get_log(self._h).decode()

    nparts = property(lambda s: lib().clfa_pconv_matrix_nparts(s._h))

    def state_bytes(self):
        return lib().clfa_pconv_matrix_state_bytes(self._h)

    def workspace_bytes(self):
        return lib().clfa_pconv_matrix_workspace_bytes(self._h)

    def kernel_name(self):
        return lib().clfa_pconv_matrix_kernel_name(self._h).decode()

    def _host_rows(self, ir):
        ir = np.asarray(ir, dtype=np.float32)
        need = self.nparts * self.pts
        if ir.ndim != 3 or ir.shape[:2] != (self.outputs, self.inputs) or ir.shape[2] < need:
            return None
        return np.ascontiguousarray(ir[:, :, :need])

    def _device_rows(self, ir, stream):
        """(row stride, stream) of a device tensor of responses, None for a bad one"""
        need = self.nparts * self.pts
        if (ir.dim() != 3 or tuple(ir.shape[:2]) != (self.outputs, self.inputs) or ir.shape[2] < need
                or str(ir.dtype) != "torch.float32" or ir.stride(2) != 1):
            return None
        rs = ir.stride(1) if self.inputs > 1 else (ir.stride(0) if self.outputs > 1 else max(ir.stride(1), need))
        if self.outputs > 1 and ir.stride(0) != self.inputs * rs:
            return None
        return rs, _stream_of(ir, stream)

    def push_ir(self, ir):
        """ir: float32 (outputs, inputs, >= nparts*pts), e.g. rows of cvs samples (the remainder is ignored)"""
        ir = self._host_rows(ir)
        if ir is None:
            return CL_INVALID_VALUE
        return lib().clfa_pconv_matrix_push_ir(self._h, ir.ctypes.data)

    def push_ir_device(self, ir, stream=None):
        """ir: device tensor (outputs, inputs, >= nparts*pts) of float32 whose rows are contiguous and evenly spaced
        (stride(0) == inputs * stride(1)); the row stride is stride(1).  Asynchronous on `stream`."""
        rows = self._device_rows(ir, stream)
        if rows is None:
            return CL_INVALID_VALUE
        return lib().clfa_pconv_matrix_push_ir_dev(self._h, ir.data_ptr(), rows[0], rows[1])

    def push_ir_fade(self, ir, fade_blocks):
        """push_ir as a crossfade: over the next fade_blocks blocks the output moves linearly, sample by sample, from
        what the responses in force give to what `ir` gives on the same input history (clfft_amd.h); blocking"""
        ir = self._host_rows(ir)
        if ir is None:
            return CL_INVALID_VALUE
        return lib().clfa_pconv_matrix_push_ir_fade(self._h, ir.ctypes.data, int(fade_blocks))

    def push_ir_fade_device(self, ir, fade_blocks, stream=None):
        """push_ir_device as a crossfade over the next fade_blocks blocks.  Asynchronous on `stream`; not under graph
        capture, and no other push while fade_remaining() > 0 (CL_INVALID_OPERATION)."""
        rows = self._device_rows(ir, stream)
        if rows is None:
            return CL_INVALID_VALUE
        return lib().clfa_pconv_matrix_push_ir_fade_dev(self._h, ir.data_ptr(), rows[0], int(fade_blocks), rows[1])

    def fade_remaining(self):
        """blocks of a pending crossfade that have not been processed yet; 0: none"""
        return lib().clfa_pconv_matrix_fade_remaining(self._h)

    def convolution(self, output, input):
        """whole signals on the host: float32 (inputs, L) -> (outputs, L), L a multiple of pts; blocking"""
        output = _host(output, np.float32)
        a = np.ascontiguousarray(input, dtype=np.float32)
        if (a.ndim != 2 or a.shape[0] != self.inputs or a.shape[1] % self.pts
                or output.shape != (self.outputs, a.shape[1])):
            return CL_INVALID_VALUE
        return lib().clfa_pconv_matrix_convolution(self._h, output.ctypes.data, a.ctypes.data, a.shape[1] // self.pts)

    def process_device(self, out, x, stream=None):
        """device tensors: x (inputs, L), out (outputs, L) of float32, stride(1) == 1, L % pts == 0; the row stride of
        each is its stride(0) (views into longer rows are fine).  Asynchronous on `stream`."""
        lo, so = _block_rows(out, self.outputs, self.outputs, False)
        li, si = _block_rows(x, self.inputs, self.inputs, False)
        if lo != li or li % self.pts:
            return CL_INVALID_VALUE
        return lib().clfa_pconv_matrix_process_dev(self._h, out.data_ptr(), so, x.data_ptr(), si, li // self.pts,
                                                   _stream_of(x, stream))


class Cldconv(_BlockConv):
    """cl_conv::Cldconv(device_id, cvs, vsize, errs=NULL, uData=NULL) (cl_dconv.h:17-66); channels > 1 (extension): that
    many independent instances in one object, blocks of float32[channels, vsize]"""
    _destroy, _abi, _block = "clfa_dconv_destroy", "clfa_dconv_", "vsize"

    def __init__(self, device_id, cvs, vsize, errs=None, uData=None, channels=1):
        self.irsize, self.vsize, self.channels = int(cvs), int(vsize), int(channels)
        self._errs, self._udata = errs, uData
        h = C.c_void_p()
        e = lib().clfa_dconv_create_channels(C.byref(h), int(device_id), int(cvs), int(vsize), int(channels))
        self._h = h
        if e != CL_SUCCESS:
            self._report(e)

    def get_cl_err(self):
        return lib().clfa_dconv_get_error(self._h)

    wp = property(lambda s: lib().clfa_dconv_wp(s._h))

    def state_bytes(self):
        return lib().clfa_dconv_state_bytes(self._h)

    def push_ir(self, ir):
        """cl_dconv.cpp:150-153; channels > 1: float32 (channels, >= irsize)"""
        ir = np.asarray(ir, dtype=np.float32)
        if self.channels > 1:
            if ir.ndim != 2 or ir.shape[0] != self.channels or ir.shape[1] < self.irsize:
                return CL_INVALID_VALUE
            ir = np.ascontiguousarray(ir[:, :self.irsize])
            return lib().clfa_dconv_push_ir(self._h, ir.ctypes.data)
        ir = np.ascontiguousarray(ir)
        if ir.size < self.irsize:
            return CL_INVALID_VALUE
        return lib().clfa_dconv_push_ir(self._h, ir.ctypes.data)

    def push_ir_device(self, ir, stream=None):
        """ir: device tensor (channels, >= irsize) of float32 (1-D for one channel), rows contiguous; asynchronous on
        `stream`"""
        shape, strides = tuple(ir.shape), tuple(ir.stride())
        if ir.dim() == 1:
            shape, strides = (1,) + shape, (shape[0],) + strides
        if (len(shape) != 2 or shape[0] != self.channels or shape[1] < self.irsize or (shape[1] > 1 and strides[1] != 1)
                or (shape[0] > 1 and strides[0] < self.irsize) or str(ir.dtype) != "torch.float32"):
            return CL_INVALID_VALUE
        return lib().clfa_dconv_push_ir_dev(self._h, ir.data_ptr(), max(strides[0], self.irsize), _stream_of(ir, stream))

    def convolution(self, out, in1, in2=None):
        """cl_dconv.cpp:109-148; float32[channels, vsize]"""
        return _BlockConv.convolution(self, out, in1, in2)   # (the reference's argument names, cl_dconv.h:59-61)

    def process_device(self, out, in1, in2=None, stream=None):
        """device-resident block (extension): channels x vsize float32 each, asynchronous on `stream`; out must not
        overlap an input"""
        n = self.vsize * self.channels
        for t in (out, in1) + ((in2,) if in2 is not None else ()):
            if hasattr(t, "numel") and (t.numel() != n or not t.is_contiguous() or str(t.dtype) != "torch.float32"):
                return CL_INVALID_VALUE
        po, stream = _ptr_stream(out, stream)
        p1, _ = _ptr_stream(in1, stream)
        p2 = _ptr_stream(in2, stream)[0] if in2 is not None else None
        return lib().clfa_dconv_process_dev(self._h, po, p1, p2, stream)

    def blocks_kernel_name(self, time_varying=False):
        """"k_dconvb_fir" (static form) or "loop" (two inputs: the single-block kernel once per block and channel)"""
        return lib().clfa_dconv_blocks_kernel_name(self._h, int(bool(time_varying))).decode()
