"""What a header edit rebuilds, asked of make (opencl_fft_amd/csrc/Makefile): the objects' dependencies are the
compiler's own lists (build/<stem>.d, written by -MMD -MP), and the objects are every *.hip of the directory plus the
host sources.  For a header H the sources recompiled after an edit are the `-c <source>` of `make -n -W H` minus those of
plain `make -n`; no file is touched.  The launch headers are per kernel family, so an edit of one family's header or of
the FFT engine leaves the other families' objects alone, and a new kernel file cannot be left out of the link."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opencl_fft_amd", "csrc")
CONV_HOST = ["pconv_host.cpp", "dconv_host.cpp", "pconv_matrix_host.cpp", "nupconv_host.cpp"]
PVOC_HOST = ["pvoc_host.cpp", "pvoc_frames_host.cpp", "pvoc_stream_host.cpp", "pvoc_rows_host.cpp", "pvoc_signal_host.cpp"]
HOST = ["clfft_amd.cpp"] + CONV_HOST + ["stft_host.cpp"] + PVOC_HOST
PVOC = ["pvoc_kernels.hip", "pvoc_ops.hip", "pvoc_pair.hip", "pvoc_time.hip", "pvoc_delay.hip", "pvoc_shape.hip",
        "pvoc_desc.hip", "pvoc_trace.hip", "pvoc_demix.hip", "pvoc_adsyn.hip"]
# the units that use nothing of the FFT engine (fft_device.hpp)
NO_ENGINE = ["pvoc_kernels.hip", "pvoc_time.hip", "pvoc_delay.hip", "pvoc_desc.hip", "pvoc_trace.hip", "pvoc_demix.hip",
             "pvoc_adsyn.hip", "dconv_block.hip", "bandwidth_probe.hip"] + PVOC_HOST


def units():
    return sorted(os.path.basename(f) for f in glob.glob(os.path.join(CSRC, "*.hip"))) + HOST


def make_n(*args):
    """the command lines `make -n` would run"""
    return subprocess.check_output(["make", "-n", "-C", CSRC] + list(args), stderr=subprocess.STDOUT).decode().splitlines()


def compiled(lines):
    return {m.group(1) for ln in lines for m in [re.search(r"\s-c (\S+)", ln)] if m}


@pytest.fixture(scope="module")
def up_to_date():
    """the sources plain `make -n` would compile (none after a build), once the compiler's lists are there"""
    missing = [u for u in units() if not os.path.exists(os.path.join(CSRC, "build", os.path.splitext(u)[0] + ".d"))]
    assert not missing, "no build/*.d for %s: build the library first" % missing
    return compiled(make_n())


def recompiled(header, base):
    assert os.path.exists(os.path.join(CSRC, header)), header
    return compiled(make_n("-W", header)) - base


def test_units_are_every_kernel_file():
    assert set(PVOC) == {u for u in units() if u.startswith("pvoc_") and u.endswith(".hip")}
    assert set(NO_ENGINE) < set(units())


@pytest.mark.parametrize("header, unit", [("fft_res_regs.inc", "fft_resident.hip"), ("pconv_fused.inc", "pconv_chain.hip")])
def test_inc_file_belongs_to_one_unit(up_to_date, header, unit):
    assert recompiled(header, up_to_date) == {unit}


def test_pvoc_launch_header_is_pvoc_only(up_to_date):
    assert recompiled("pvoc_launch.hpp", up_to_date) == set(PVOC) | set(PVOC_HOST)


@pytest.mark.parametrize("header, units", [("bank_launch.hpp", {"bank_kernels.hip", "pvoc_rows_host.cpp"}),
                                           ("pitch_launch.hpp", {"pitch_kernels.hip", "pvoc_rows_host.cpp"}),
                                           ("tanal_launch.hpp", {"tanal_kernels.hip", "pvoc_signal_host.cpp"})])
def test_family_launch_header_is_its_kernel_file_and_one_host_source(up_to_date, header, units):
    assert recompiled(header, up_to_date) == units


def test_pvoc_host_header_is_the_pvoc_hosts(up_to_date):
    assert recompiled("pvoc_host.hpp", up_to_date) == set(PVOC_HOST)


def test_dconv_launch_header_is_dconv_only(up_to_date):
    assert recompiled("dconv_launch.hpp", up_to_date) == {"dconv_block.hip", "dconv_blocks.hip", "dconv_host.cpp"}


def test_conv_host_header_is_the_convolution_hosts(up_to_date):
    assert recompiled("conv_host.hpp", up_to_date) == set(CONV_HOST)


def test_fft_engine_leaves_other_families_alone(up_to_date):
    got = recompiled("fft_device.hpp", up_to_date)
    assert {"fft_kernels.hip", "fft_resident.hip"} <= got
    assert not got & set(NO_ENGINE), sorted(got & set(NO_ENGINE))


def test_complex_type_reaches_every_unit_but_the_probe(up_to_date):
    assert recompiled("cpx.hpp", up_to_date) == set(units()) - {"bandwidth_probe.hip"}


def test_link_line_holds_every_unit(up_to_date):
    link = [ln for ln in make_n("-W", "clfft_amd.cpp") if " -shared " in ln and "libclfft_amd.so" in ln]
    assert len(link) == 1, link
    objs = [t for t in link[0].split() if t.endswith(".o")]
    assert sorted(objs) == sorted("build/%s.o" % os.path.splitext(u)[0] for u in units())
