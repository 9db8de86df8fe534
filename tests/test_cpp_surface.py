"""The reference's C++ class surface (include/cl_fft.h, cl_conv.h, cl_dconv.h -> libcl_fft.so):
programs written like the reference's own callers (clGetDeviceIDs, Clcfft(device, N, fwd),
get_error(), transform(), cl_error_string()) compile against the drop-in headers and, on a GPU,
produce the reference's known answers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
PROGS = ["test_cfft", "test_rfft", "test_conv", "test_opcodes", "test_subclass"]


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "opencl_fft_amd", "csrc")], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", CPP], stdout=subprocess.DEVNULL)
    return os.path.join(CPP, "build")


def test_class_library_exports_reference_symbols(built):
    out = subprocess.check_output(["nm", "-DC", "--defined-only", os.path.join(ROOT, "opencl_fft_amd", "libcl_fft.so")]).decode()
    for sym in ["cl_fft::Clcfft::Clcfft(_cl_device_id*, int, bool)", "cl_fft::Clcfft::transform(std::complex<float>*)",
                "cl_fft::Clrfft::Clrfft(_cl_device_id*, int, bool)", "cl_fft::Clrfft::transform(std::complex<float>*, float*)",
                "cl_fft::cl_error_string(int)", "cl_conv::Clpconv::push_ir(float*)",
                "cl_conv::Clpconv::convolution(float*, float*)", "cl_conv::Clpconv::convolution(float*, float*, float*)",
                "cl_conv::Cldconv::convolution(float*, float*)", "cl_conv::Cldconv::push_ir(float*)"]:
        assert sym in out, sym


@pytest.mark.parametrize("prog", PROGS)
def test_programs_fail_loudly_without_device(built, prog):
    import opencl_fft_amd as fa
    if fa.device_count() > 0:
        pytest.skip("a HIP device is present")
    r = subprocess.run([os.path.join(built, prog)], capture_output=True, text=True)
    assert r.returncode == 2


@pytest.mark.gpu
@pytest.mark.parametrize("prog", PROGS)
def test_programs_on_gpu(built, prog):
    r = subprocess.run([os.path.join(built, prog)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("OK"), r.stdout

