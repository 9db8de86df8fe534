"""opencl_fft_amd — MI355X-native drop-in for the hot path of vlazzarini/opencl_fft.

Host-side mirror of the reference's class surface (same names, argument
meaning and integer OpenCL status codes), over the C ABI of libclfft_amd.so:

    Clcfft   cl_fft.h:29-70     complex FFT, forward scaled 1/N, inverse unscaled
    Clrfft   cl_fft.h:74-111    packed real FFT
    Clpconv  cl_conv.h:124-188  uniformly partitioned overlap-add convolution
    Cldconv  cl_dconv.h:17-66   direct convolution
    Stft     (extension)        short-time analysis / windowed overlap-add synthesis on the Clrfft layout
    PconvMatrix (extension)     convolution matrix: many inputs mixed into many outputs
    Nupconv  (extension)        non-uniformly partitioned convolution: long responses at low latency
    NupconvMatrix (extension)   ... many inputs mixed into many outputs, long responses at low latency
    Pvoc     (extension)        phase vocoder on Stft's spectra: (amp, freq) frames both ways

Like the reference, constructors never raise: a failed setup is read back with
``get_error()`` / ``get_cl_err()`` and every method returns the status code.
Extensions the reference does not have: batches (leading array axes), many
independent channels per Clpconv object, and ``*_device`` methods that work in
place on device memory (raw pointers or torch tensors) on a given HIP stream.

PyTorch is only used by callers for device memory and streams; nothing here
imports it.
"""
from . import _lib  # noqa: F401
from ._base import (CL_INVALID_VALUE, CL_SUCCESS, _block_rows, _Handle, _host, _ptr_stream, _row_view,  # noqa: F401
                    _stream_of)
from ._lib import ClError, check, lib  # noqa: F401  (`lib` here is the one every module calls: _base._pkg)
from .conv import Cldconv, Clpconv, Nupconv, NupconvMatrix, PconvMatrix, _BlockConv  # noqa: F401
from .fft import (PI, Clcfft, Clrfft, _Plan, bandwidth_probe, bitrev_table, cl_error_string, device_count,  # noqa: F401
                  device_name, r2c_twiddle_table, reorder_device, twiddle_table)
from .pvoc import Pvoc
from .stft import Stft, onesided_to_packed, packed_to_onesided

__all__ = ["Clcfft", "Clrfft", "Clpconv", "Cldconv", "ClError", "cl_error_string", "device_count",
           "device_name", "bitrev_table", "twiddle_table", "r2c_twiddle_table", "reorder_device", "PI",
           "Stft", "packed_to_onesided", "onesided_to_packed", "PconvMatrix", "Nupconv", "NupconvMatrix", "Pvoc"]
