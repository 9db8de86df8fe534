"""tests/cpp/test_dconv_blocks.cpp: the extension members of cl_conv::Cldconv (channels, whole signals per call)
through the C++ class surface, built by the C++ harness's pattern rule."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
PROG = "test_dconv_blocks"


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "opencl_fft_amd", "csrc")], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", CPP, "build/" + PROG], stdout=subprocess.DEVNULL)
    return os.path.join(CPP, "build", PROG)


def test_class_library_exports_the_extension_members(built):
    out = subprocess.check_output(["nm", "-DC", "--defined-only", os.path.join(ROOT, "opencl_fft_amd", "libcl_fft.so")]).decode()
    for sym in ["cl_conv::Cldconv::convolution_blocks(float*, float*, float*, long)",
                "cl_conv::Cldconv::convolution_blocks_device(void*, long, void const*, void const*, long, long, void*)",
                "cl_conv::Cldconv::push_ir_device(void const*, long, void*)", "cl_conv::Cldconv::blocks_kernel_name(bool)",
                "cl_conv::Cldconv::convolution(float*, float*)"]:
        assert sym in out, sym


@pytest.mark.gpu
def test_program_on_gpu(built):
    r = subprocess.run([built], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("OK"), r.stdout
