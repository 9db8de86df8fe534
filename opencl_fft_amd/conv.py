"""The convolutions: Clpconv and Cldconv of the reference's cl_conv.h / cl_dconv.h with what they share (_BlockConv),
the convolution matrix PconvMatrix, the non-uniformly partitioned convolution Nupconv and its matrix form NupconvMatrix."""
import numpy as np

from ._base import CL_INVALID_VALUE, CL_SUCCESS, _Handle, _Object, _block_rows, _host, _is_f32, _pkg, _ptr_stream, _stream_of
from .fft import cl_error_string


class _BlockConv(_Handle):
    """What Clpconv and Cldconv share: blocks of float32[channels, block length] through the C ABI functions
    `_abi` + name, the block length being the attribute `_block` names (pts / vsize)."""
    _block = None
    wp = property(lambda s: s._get("wp"))

    def state_bytes(self):
        return self._get("state_bytes")

    def _report(self, e):
        # error callback by value, default prints unless user data is given (cl_conv.h:142-145)
        msg = cl_error_string(e)
        if self._errs is not None:
            self._errs(msg, self._udata)
        elif self._udata is None:
            print(msg)

    def cl_error_string(self, err):
        return cl_error_string(err)

    def _ir_rows(self, ir, need, unit_stride_of_one_sample):
        """the row stride of a device tensor of responses, (channels, >= need) float32 (or 1-D for one channel) whose rows
        are contiguous and do not overlap; None for another.  unit_stride_of_one_sample: stride(1) == 1 is asked of
        rows of a single sample as well."""
        shape, strides = tuple(ir.shape), tuple(ir.stride())
        if ir.dim() == 1:
            shape, strides = (1,) + shape, (shape[0],) + strides
        if (len(shape) != 2 or shape[0] != self.channels or shape[1] < need
                or ((unit_stride_of_one_sample or shape[1] > 1) and strides[1] != 1)
                or (shape[0] > 1 and strides[0] < need) or not _is_f32(ir)):
            return None
        return strides[0]

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
        return self._get("blocks_workspace_bytes")

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
    _abi, _block = "clfa_pconv_", "pts"

    def __init__(self, device_id, cvs, pts, errs=None, uData=None, channels=1):
        self.pts = int(pts)
        self.channels = int(channels)
        self._errs, self._udata = errs, uData
        e = self._create(_pkg.lib().clfa_pconv_create, int(device_id), int(cvs), int(pts), int(channels))
        if e != CL_SUCCESS:
            self._report(e)

    def get_cl_err(self):
        """cl_conv.h:187"""
        return self._get("get_error")

    nparts = property(lambda s: s._get("nparts"))
    wp2 = property(lambda s: s._get("wp2"))

    def kernel_name(self):
        return self._text("kernel_name")

    def push_ir(self, ir):
        """cl_conv.cpp:353-388; ir: float32[channels, nparts*pts] (or 1-D for one channel)"""
        ir = np.ascontiguousarray(ir, dtype=np.float32)
        need = self.nparts * self.pts
        if ir.ndim == 1:
            ir = ir[None, :]
        if ir.shape[0] != self.channels or ir.shape[1] < need:
            return CL_INVALID_VALUE
        ir = np.ascontiguousarray(ir[:, :need])
        return _pkg.lib().clfa_pconv_push_ir(self._h, ir.ctypes.data)

    def push_ir_device(self, ir, stream=None):
        """ir: device tensor (channels, >= nparts*pts) of float32, rows contiguous; a (channels, cvs)
        tensor with cvs not a multiple of pts is fine (the remainder of every row is ignored, like the
        reference's floor(cvs / pts), cl_conv.cpp:143)"""
        stride = self._ir_rows(ir, self.nparts * self.pts, True)
        if stride is None:
            return CL_INVALID_VALUE
        p, stream = _ptr_stream(ir, stream)      # (the whole tensor contiguous: ValueError for padded rows)
        return _pkg.lib().clfa_pconv_push_ir_dev(self._h, p, stride, stream)

    def process_device(self, out, in1, in2=None, stream=None):
        po, stream = _ptr_stream(out, stream)
        p1, _ = _ptr_stream(in1, stream)
        p2 = _ptr_stream(in2, stream)[0] if in2 is not None else None
        return _pkg.lib().clfa_pconv_process_dev(self._h, po, p1, p2, stream)

    def blocks_kernel_name(self):
        """"k_pconvb_mac" (partitions of 32..4096 samples) or "loop" (the single-block route once per block)"""
        return self._text("blocks_kernel_name")


class _MatrixRows:
    """responses of a matrix object as rows: (outputs, inputs, >= self._need()) float32"""

    def _host_rows(self, ir):
        """the packed rows of a host array of responses, None for a bad one"""
        ir = np.asarray(ir, dtype=np.float32)
        need = self._need()
        if ir.ndim != 3 or ir.shape[:2] != (self.outputs, self.inputs) or ir.shape[2] < need:
            return None
        return np.ascontiguousarray(ir[:, :, :need])

    def _device_rows(self, ir, stream):
        """(row stride, stream) of a device tensor of responses, None for a bad one"""
        need = self._need()
        if (ir.dim() != 3 or tuple(ir.shape[:2]) != (self.outputs, self.inputs) or ir.shape[2] < need
                or not _is_f32(ir) or ir.stride(2) != 1):
            return None
        rs = ir.stride(1) if self.inputs > 1 else (ir.stride(0) if self.outputs > 1 else max(ir.stride(1), need))
        if self.outputs > 1 and ir.stride(0) != self.inputs * rs:
            return None
        return rs, _stream_of(ir, stream)


class PconvMatrix(_MatrixRows, _Object):
    """Convolution matrix (extension, clfa_pconv_matrix in clfft_amd.h): `inputs` signals mixed into `outputs` signals,
    y_o = sum_i x_i * h_{o,i}, by uniformly partitioned overlap-add convolution with static responses.  Block j of output
    o is the sum over i of what Clpconv(device_id, cvs, pts) holding h_{o,i} returns for block j of input i.  pts is a
    power of two, 32..4096.  Like the other objects the constructor does not raise: get_error() / get_log() report a
    failed setup."""
    _abi = "clfa_pconv_matrix_"

    def __init__(self, device_id, cvs, pts, inputs, outputs):
        self.cvs, self.pts, self.inputs, self.outputs = int(cvs), int(pts), int(inputs), int(outputs)
        self._create(_pkg.lib().clfa_pconv_matrix_create, int(device_id), self.cvs, self.pts, self.inputs, self.outputs)

    nparts = property(lambda s: s._get("nparts"))

    def state_bytes(self):
        return self._get("state_bytes")

    def _need(self):
        return self.nparts * self.pts

    def push_ir(self, ir):
        """ir: float32 (outputs, inputs, >= nparts*pts), e.g. rows of cvs samples (the remainder is ignored)"""
        ir = self._host_rows(ir)
        if ir is None:
            return CL_INVALID_VALUE
        return _pkg.lib().clfa_pconv_matrix_push_ir(self._h, ir.ctypes.data)

    def push_ir_device(self, ir, stream=None):
        """ir: device tensor (outputs, inputs, >= nparts*pts) of float32 whose rows are contiguous and evenly spaced
        (stride(0) == inputs * stride(1)); the row stride is stride(1).  Asynchronous on `stream`."""
        rows = self._device_rows(ir, stream)
        if rows is None:
            return CL_INVALID_VALUE
        return _pkg.lib().clfa_pconv_matrix_push_ir_dev(self._h, ir.data_ptr(), rows[0], rows[1])

    def push_ir_fade(self, ir, fade_blocks):
        """push_ir as a crossfade: over the next fade_blocks blocks the output moves linearly, sample by sample, from
        what the responses in force give to what `ir` gives on the same input history (clfft_amd.h); blocking"""
        ir = self._host_rows(ir)
        if ir is None:
            return CL_INVALID_VALUE
        return _pkg.lib().clfa_pconv_matrix_push_ir_fade(self._h, ir.ctypes.data, int(fade_blocks))

    def push_ir_fade_device(self, ir, fade_blocks, stream=None):
        """push_ir_device as a crossfade over the next fade_blocks blocks.  Asynchronous on `stream`; not under graph
        capture, and no other push while fade_remaining() > 0 (CL_INVALID_OPERATION)."""
        rows = self._device_rows(ir, stream)
        if rows is None:
            return CL_INVALID_VALUE
        return _pkg.lib().clfa_pconv_matrix_push_ir_fade_dev(self._h, ir.data_ptr(), rows[0], int(fade_blocks), rows[1])

    def fade_remaining(self):
        """blocks of a pending crossfade that have not been processed yet; 0: none"""
        return self._get("fade_remaining")

    def convolution(self, output, input):
        """whole signals on the host: float32 (inputs, L) -> (outputs, L), L a multiple of pts; blocking"""
        output = _host(output, np.float32)
        a = np.ascontiguousarray(input, dtype=np.float32)
        if (a.ndim != 2 or a.shape[0] != self.inputs or a.shape[1] % self.pts
                or output.shape != (self.outputs, a.shape[1])):
            return CL_INVALID_VALUE
        return _pkg.lib().clfa_pconv_matrix_convolution(self._h, output.ctypes.data, a.ctypes.data, a.shape[1] // self.pts)

    def process_device(self, out, x, stream=None):
        """device tensors: x (inputs, L), out (outputs, L) of float32, stride(1) == 1, L % pts == 0; the row stride of
        each is its stride(0) (views into longer rows are fine).  Asynchronous on `stream`."""
        lo, so = _block_rows(out, self.outputs, self.outputs, False)
        li, si = _block_rows(x, self.inputs, self.inputs, False)
        if lo != li or li % self.pts:
            return CL_INVALID_VALUE
        return _pkg.lib().clfa_pconv_matrix_process_dev(self._h, out.data_ptr(), so, x.data_ptr(), si, li // self.pts,
                                                   _stream_of(x, stream))


class _Nup(_Object):
    """what Nupconv and NupconvMatrix share: two levels, a position, a pending crossfade, reset"""
    position = property(lambda s: s._get("position"))

    def nparts(self, level):
        """partitions of level 0 (the head) or 1 (the tail)"""
        return self._get("nparts", int(level))

    def state_bytes(self):
        return self._get("state_bytes")

    def _need(self):
        return 2 * self.pts1 + self.nparts(1) * self.pts1

    def fade_remaining(self):
        """head blocks of a pending crossfade that have not been processed yet; 0: none"""
        return self._get("fade_remaining")

    def reset(self, stream=None):
        """forget the input history (position 0); the responses stay.  `stream`: a HIP stream handle, default the
        current torch stream of the object's device"""
        if stream is None:
            import torch
            stream = torch.cuda.current_stream().cuda_stream
        return self._get("reset", stream)


class Nupconv(_Nup):
    """Non-uniformly partitioned convolution (extension, clfa_nupconv in clfft_amd.h): long responses at a latency of
    pts0 samples.  A head of 2 * pts1 / pts0 partitions of pts0 covers h[:2*pts1]; the tail runs in partitions of pts1,
    each tail block's work spread over the pts1 / pts0 small blocks that pass while it is not yet needed.  The output is,
    bit for bit, Clpconv(2*pts1, pts0) on h[:2*pts1] plus Clpconv(cvs - 2*pts1, pts1) on h[2*pts1:] delayed by 2*pts1
    samples, both through process_blocks_device — not the bits of Clpconv(cvs, pts0).  pts0 < pts1 are powers of two,
    32..4096; cvs >= 3 * pts1.  Like the other objects the constructor does not raise: get_error() / get_log()."""
    _abi = "clfa_nupconv_"

    def __init__(self, device_id, cvs, pts0, pts1, channels=1):
        self.cvs, self.pts0, self.pts1, self.channels = int(cvs), int(pts0), int(pts1), int(channels)
        self._create(_pkg.lib().clfa_nupconv_create, int(device_id), self.cvs, self.pts0, self.pts1, self.channels)

    def _host_rows(self, ir):
        """the packed rows of a host array of responses, None for a bad one"""
        ir = np.asarray(ir, dtype=np.float32)
        if ir.ndim == 1:
            ir = ir[None, :]
        need = self._need()
        if ir.ndim != 2 or ir.shape[0] != self.channels or ir.shape[1] < need:
            return None
        return np.ascontiguousarray(ir[:, :need])

    def push_ir(self, ir):
        """ir: float32 (channels, >= 2*pts1 + nparts(1)*pts1), e.g. rows of cvs samples (1-D for one channel); blocking.
        Exact at position % (pts1 // pts0) == 0; at another phase the tail block in progress mixes both responses: for a
        change at any phase, and without the step, use push_ir_fade."""
        ir = self._host_rows(ir)
        if ir is None:
            return CL_INVALID_VALUE
        return _pkg.lib().clfa_nupconv_push_ir(self._h, ir.ctypes.data)

    def push_ir_device(self, ir, stream=None):
        """ir: device tensor (channels, >= 2*pts1 + nparts(1)*pts1) of float32 (1-D for one channel), stride(1) == 1; the
        row stride is its stride(0).  Asynchronous on `stream`."""
        length, stride = _block_rows(ir, self.channels, "channels", True)
        if length < self._need():
            return CL_INVALID_VALUE
        return _pkg.lib().clfa_nupconv_push_ir_dev(self._h, ir.data_ptr(), stride, _stream_of(ir, stream))

    def push_ir_fade(self, ir, fade_blocks):
        """push_ir as a crossfade, at any phase: over the next fade_blocks head blocks the output moves linearly, sample by
        sample, from what the responses in force give to what an object that always held `ir` gives on the same input
        history (clfft_amd.h); blocking.  The first fade allocates a second response set: it doubles the response memory."""
        ir = self._host_rows(ir)
        if ir is None:
            return CL_INVALID_VALUE
        return _pkg.lib().clfa_nupconv_push_ir_fade(self._h, ir.ctypes.data, int(fade_blocks))

    def push_ir_fade_device(self, ir, fade_blocks, stream=None):
        """push_ir_device as a crossfade over the next fade_blocks head blocks.  Asynchronous on `stream`; not under graph
        capture, and no other push and no reset while fade_remaining() > 0 (CL_INVALID_OPERATION)."""
        length, stride = _block_rows(ir, self.channels, "channels", True)
        if length < self._need():
            return CL_INVALID_VALUE
        return _pkg.lib().clfa_nupconv_push_ir_fade_dev(self._h, ir.data_ptr(), stride, int(fade_blocks), _stream_of(ir, stream))

    def convolution(self, output, input):
        """whole signals on the host: float32 (channels, L) -> (channels, L) (1-D for one channel), L a multiple of
        pts0; blocking"""
        output = _host(output, np.float32)
        a = np.ascontiguousarray(input, dtype=np.float32)
        if a.ndim == 1:
            a = a[None, :]
        if a.ndim != 2 or a.shape[0] != self.channels or a.shape[1] % self.pts0 or output.size != a.size:
            return CL_INVALID_VALUE
        return _pkg.lib().clfa_nupconv_convolution(self._h, output.ctypes.data, a.ctypes.data, a.shape[1] // self.pts0)

    def process_device(self, out, x, stream=None):
        """device tensors (channels, L) of float32 (1-D for one channel), stride(1) == 1, L a multiple of pts0; the row
        stride of each is its stride(0) (views into longer rows are fine).  Asynchronous on `stream`; not under graph
        capture (CL_INVALID_OPERATION: the phase of the schedule lives on the host)."""
        (lo, so), (li, si) = (_block_rows(t, self.channels, "channels", True) for t in (out, x))
        if lo != li or li % self.pts0:
            return CL_INVALID_VALUE
        return _pkg.lib().clfa_nupconv_process_dev(self._h, out.data_ptr(), so, x.data_ptr(), si, li // self.pts0,
                                                   _stream_of(x, stream))

    tv_period = property(lambda s: s._get("tv_period"), doc="head blocks of one response period, (nparts(1) + 2) * pts1 // pts0")

    def convolution_tv(self, output, input, second):
        """convolution() with a time-varying second input (clfft_amd.h): `second`, shaped as `input`, is the response as
        a live stream — its sample j is response sample j % (tv_period * pts0); blocking"""
        output = _host(output, np.float32)
        a = np.ascontiguousarray(input, dtype=np.float32)
        b = np.ascontiguousarray(second, dtype=np.float32)
        if a.ndim == 1:
            a = a[None, :]
        if (a.ndim != 2 or a.shape[0] != self.channels or a.shape[1] % self.pts0 or output.size != a.size
                or b.size != a.size):
            return CL_INVALID_VALUE
        return _pkg.lib().clfa_nupconv_convolution_tv(self._h, output.ctypes.data, a.ctypes.data, b.ctypes.data,
                                                      a.shape[1] // self.pts0)

    def process_tv_device(self, out, x, w, stream=None):
        """process_device() with a time-varying second input w (clfft_amd.h): device tensors as there, w with its own row
        stride (w may be x itself).  Not while fade_remaining() > 0 and not under graph capture (CL_INVALID_OPERATION)."""
        (lo, so), (li, si), (lw, sw) = (_block_rows(t, self.channels, "channels", True) for t in (out, x, w))
        if lo != li or lw != li or li % self.pts0:
            return CL_INVALID_VALUE
        return _pkg.lib().clfa_nupconv_process_tv_dev(self._h, out.data_ptr(), so, x.data_ptr(), si, w.data_ptr(), sw,
                                                      li // self.pts0, _stream_of(x, stream))


class NupconvMatrix(_MatrixRows, _Nup):
    """Non-uniformly partitioned convolution matrix (extension, clfa_nupconv_matrix in clfft_amd.h): `inputs` signals mixed
    into `outputs` signals, y_o = sum_i x_i * h_{o,i}, with long static responses at a latency of pts0 samples — Nupconv's
    two levels and schedule around PconvMatrix's sum over inputs.  The output is, bit for bit, PconvMatrix(2*pts1, pts0)
    on h[:, :, :2*pts1] plus PconvMatrix(cvs - 2*pts1, pts1) on h[:, :, 2*pts1:] delayed by 2*pts1 samples, each reducing
    in segments(level) segments.  pts0 < pts1 are powers of two, 32..4096; cvs >= 3 * pts1.  Responses change without a step through
    fade_ir.  Like the other objects the constructor does not raise: get_error() / get_log()."""
    _abi = "clfa_nupconv_matrix_"

    def __init__(self, device_id, cvs, pts0, pts1, inputs, outputs):
        self.cvs, self.pts0, self.pts1 = int(cvs), int(pts0), int(pts1)
        self.inputs, self.outputs = int(inputs), int(outputs)
        self._create(_pkg.lib().clfa_nupconv_matrix_create, int(device_id), self.cvs, self.pts0, self.pts1, self.inputs,
                     self.outputs)

    def segments(self, level):
        """segments in which level 0 (the head) or 1 (the tail) sums over (input, partition)"""
        return self._get("segments", int(level))

    def push_ir(self, ir):
        """ir: float32 (outputs, inputs, >= 2*pts1 + nparts(1)*pts1), e.g. rows of cvs samples; blocking.  Exact at
        position % (pts1 // pts0) == 0; at another phase the tail block in progress mixes both responses: for a change
        at any phase, and without the step, use fade_ir."""
        ir = self._host_rows(ir)
        if ir is None:
            return CL_INVALID_VALUE
        return _pkg.lib().clfa_nupconv_matrix_push_ir(self._h, ir.ctypes.data)

    def push_ir_device(self, ir, stream=None):
        """ir: device tensor (outputs, inputs, >= 2*pts1 + nparts(1)*pts1) of float32 whose rows are contiguous and evenly
        spaced (stride(0) == inputs * stride(1)); the row stride is stride(1).  Asynchronous on `stream`."""
        rows = self._device_rows(ir, stream)
        if rows is None:
            return CL_INVALID_VALUE
        return _pkg.lib().clfa_nupconv_matrix_push_ir_dev(self._h, ir.data_ptr(), rows[0], rows[1])

    def fade_ir(self, ir, fade_blocks):
        """push_ir as a crossfade, at any phase (clfa_nupconv_matrix_push_ir_fade in clfft_amd.h): over the next
        fade_blocks head blocks the output moves linearly, sample by sample, from what the responses in force give to
        what an object that always held `ir` gives on the same input history; blocking.  The first fade allocates a
        second response set: it doubles the response memory.  The method is not called push_ir_fade as on Nupconv and
        PconvMatrix because tests/test_nupconv_matrix_cpu.py, written when this class had no crossfade, asserts that it
        has no attribute of that name, and existing test files stay as they are; the C names do not differ."""
        ir = self._host_rows(ir)
        if ir is None:
            return CL_INVALID_VALUE
        return _pkg.lib().clfa_nupconv_matrix_push_ir_fade(self._h, ir.ctypes.data, int(fade_blocks))

    def fade_ir_device(self, ir, fade_blocks, stream=None):
        """push_ir_device as a crossfade over the next fade_blocks head blocks (clfa_nupconv_matrix_push_ir_fade_dev).
        Asynchronous on `stream`; not under graph capture, and no other push and no reset while fade_remaining() > 0
        (CL_INVALID_OPERATION)."""
        rows = self._device_rows(ir, stream)
        if rows is None:
            return CL_INVALID_VALUE
        return _pkg.lib().clfa_nupconv_matrix_push_ir_fade_dev(self._h, ir.data_ptr(), rows[0], int(fade_blocks), rows[1])

    def convolution(self, output, input):
        """whole signals on the host: float32 (inputs, L) -> (outputs, L), L a multiple of pts0; blocking"""
        output = _host(output, np.float32)
        a = np.ascontiguousarray(input, dtype=np.float32)
        if (a.ndim != 2 or a.shape[0] != self.inputs or a.shape[1] % self.pts0
                or output.shape != (self.outputs, a.shape[1])):
            return CL_INVALID_VALUE
        return _pkg.lib().clfa_nupconv_matrix_convolution(self._h, output.ctypes.data, a.ctypes.data, a.shape[1] // self.pts0)

    def process_device(self, out, x, stream=None):
        """device tensors: x (inputs, L), out (outputs, L) of float32, stride(1) == 1, L a multiple of pts0; the row stride
        of each is its stride(0) (views into longer rows are fine).  Asynchronous on `stream`; not under graph capture
        (CL_INVALID_OPERATION: the phase of the schedule lives on the host)."""
        lo, so = _block_rows(out, self.outputs, self.outputs, False)
        li, si = _block_rows(x, self.inputs, self.inputs, False)
        if lo != li or li % self.pts0:
            return CL_INVALID_VALUE
        return _pkg.lib().clfa_nupconv_matrix_process_dev(self._h, out.data_ptr(), so, x.data_ptr(), si, li // self.pts0,
                                                          _stream_of(x, stream))


class Cldconv(_BlockConv):
    """cl_conv::Cldconv(device_id, cvs, vsize, errs=NULL, uData=NULL) (cl_dconv.h:17-66); channels > 1 (extension): that
    many independent instances in one object, blocks of float32[channels, vsize]"""
    _abi, _block = "clfa_dconv_", "vsize"

    def __init__(self, device_id, cvs, vsize, errs=None, uData=None, channels=1):
        self.irsize, self.vsize, self.channels = int(cvs), int(vsize), int(channels)
        self._errs, self._udata = errs, uData
        e = self._create(_pkg.lib().clfa_dconv_create_channels, int(device_id), int(cvs), int(vsize), int(channels))
        if e != CL_SUCCESS:
            self._report(e)

    def get_cl_err(self):
        return self._get("get_error")

    def push_ir(self, ir):
        """cl_dconv.cpp:150-153; channels > 1: float32 (channels, >= irsize)"""
        ir = np.asarray(ir, dtype=np.float32)
        if self.channels > 1:
            if ir.ndim != 2 or ir.shape[0] != self.channels or ir.shape[1] < self.irsize:
                return CL_INVALID_VALUE
            ir = np.ascontiguousarray(ir[:, :self.irsize])
            return _pkg.lib().clfa_dconv_push_ir(self._h, ir.ctypes.data)
        ir = np.ascontiguousarray(ir)
        if ir.size < self.irsize:
            return CL_INVALID_VALUE
        return _pkg.lib().clfa_dconv_push_ir(self._h, ir.ctypes.data)

    def push_ir_device(self, ir, stream=None):
        """ir: device tensor (channels, >= irsize) of float32 (1-D for one channel), rows contiguous; asynchronous on
        `stream`"""
        stride = self._ir_rows(ir, self.irsize, False)
        if stride is None:
            return CL_INVALID_VALUE
        return _pkg.lib().clfa_dconv_push_ir_dev(self._h, ir.data_ptr(), max(stride, self.irsize), _stream_of(ir, stream))

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
        return _pkg.lib().clfa_dconv_process_dev(self._h, po, p1, p2, stream)

    def blocks_kernel_name(self, time_varying=False):
        """"k_dconvb_fir" (static form) or "loop" (two inputs: the single-block kernel once per block and channel)"""
        return self._text("blocks_kernel_name", int(bool(time_varying)))
