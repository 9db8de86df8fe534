"""Multi-block, multi-channel direct convolution without a GPU: the contract's three definitions (static form,
time-varying form, state) as a numpy model against oracle.Dconv driven block by block, the new ABI symbols, and the
answers that need no device."""
import ctypes as C

import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd import _lib
from opencl_fft_amd._lib import lib
from oracle import oracle
from tests.dconv_blocks_model import DconvBlocksModel

CL_INVALID_VALUE, CL_DEVICE_NOT_FOUND = -30, -1
NAMES = ["clfa_dconv_create_channels", "clfa_dconv_push_ir_dev", "clfa_dconv_process_blocks_dev",
         "clfa_dconv_convolution_blocks", "clfa_dconv_channels", "clfa_dconv_wp", "clfa_dconv_state_bytes",
         "clfa_dconv_blocks_workspace_bytes", "clfa_dconv_blocks_kernel_name"]
GEOMETRIES = [(1, 1), (7, 3), (16, 8), (5, 8), (65, 7), (1000, 64)]


@pytest.mark.parametrize("name", NAMES)
def test_symbol_exported_and_bound(name):
    assert hasattr(lib(), name)
    assert name in [s[0] for s in _lib.SYMBOLS]


def _oracle_blocks(orc, x1, x2, vsize):
    n = x1.size // vsize
    return np.concatenate([orc.convolution(x1[j * vsize:(j + 1) * vsize], None if x2 is None else x2[j * vsize:(j + 1) * vsize])
                           for j in range(n)]) if n else np.zeros(0, np.float32)


@pytest.mark.parametrize("tv", [False, True], ids=["static", "tv"])
@pytest.mark.parametrize("irsize,vsize", GEOMETRIES)
def test_model_matches_the_oracle_block_by_block(irsize, vsize, tv):
    """calls of 1 + 5 + 0 + 3 blocks (more where the ring is long, so that it wraps): wp0 != 0 from the second call on;
    a push_ir between two calls; several channels.  float32 rounding of irsize products: the oracle is float32, the
    model float64 — bound 2 sqrt(irsize) 2^-24 + 1e-6, relative to the largest expected sample."""
    channels = 3 if irsize < 1000 else 2
    rng = np.random.default_rng(irsize * 100 + vsize + tv)
    m = DconvBlocksModel(irsize, vsize, channels)
    orcs = [oracle.Dconv(irsize, vsize) for _ in range(channels)]
    ir = (rng.random((channels, irsize), dtype=np.float32) - 0.5)
    m.push_ir(ir)
    for c in range(channels):
        orcs[c].push_ir(ir[c])
    cycle = (irsize + vsize + vsize - 1) // vsize
    counts = [1, 5, 0, 3] if irsize < 1000 else [1, 5, 0, cycle + 1]
    if irsize == 65:
        counts = [1, 5, 0, 2 * cycle + 3]
    tol = 2 * np.sqrt(irsize) * 2.0 ** -24 + 1e-6
    wp = 0
    for call, nb in enumerate(counts):
        if call == 3:
            ir = (rng.random((channels, irsize), dtype=np.float32) - 0.5)
            m.push_ir(ir)
            for c in range(channels):
                orcs[c].push_ir(ir[c])
        x1 = rng.random((channels, nb * vsize), dtype=np.float32) - 0.5
        x2 = rng.random((channels, nb * vsize), dtype=np.float32) - 0.5 if tv else None
        assert m.wp == wp
        got = m.blocks(x1, x2)
        wp = (wp + nb * vsize) % (irsize + vsize)
        assert m.wp == wp
        for c in range(channels):
            want = _oracle_blocks(orcs[c], x1[c], None if x2 is None else x2[c], vsize)
            if nb:
                err = np.max(np.abs(got[c] - want)) / max(np.max(np.abs(want)), 1e-30)
                assert err <= tol, (call, nb, c, err)
    # the state: three more single blocks through the model equal the oracle's
    for j in range(3):
        x1 = rng.random((channels, vsize), dtype=np.float32) - 0.5
        x2 = rng.random((channels, vsize), dtype=np.float32) - 0.5 if tv else None
        got = m.blocks(x1, x2)
        for c in range(channels):
            want = orcs[c].convolution(x1[c], None if x2 is None else x2[c])
            assert np.max(np.abs(got[c] - want)) <= tol * max(np.max(np.abs(want)), 1e-3), (j, c)


def test_argument_errors_need_no_device():
    """a NULL object is an invalid value for every new entry point; the Python surface refuses shapes that do not fit
    before anything reaches the device"""
    L = C.c_long
    f = lib()
    assert f.clfa_dconv_process_blocks_dev(None, None, L(8), None, None, L(8), L(1), None) == CL_INVALID_VALUE
    assert f.clfa_dconv_convolution_blocks(None, None, None, None, L(1)) == CL_INVALID_VALUE
    assert f.clfa_dconv_push_ir_dev(None, None, L(8), None) == CL_INVALID_VALUE
    assert f.clfa_dconv_create_channels(None, 0, 16, 8, 2) == CL_INVALID_VALUE
    assert f.clfa_dconv_channels(None) == 0 and f.clfa_dconv_wp(None) == -1
    assert f.clfa_dconv_state_bytes(None) == 0 and f.clfa_dconv_blocks_workspace_bytes(None) == 0
    assert f.clfa_dconv_blocks_kernel_name(None, 0) == b""
    msgs = []
    d = fa.Cldconv(0, 16, 8, errs=lambda s, u: msgs.append(s), channels=3)
    assert d.channels == 3
    x = np.zeros((3, 24), np.float32)
    assert d.convolution_blocks(np.zeros((3, 24), np.float32), x[:2]) == CL_INVALID_VALUE            # channels
    assert d.convolution_blocks(np.zeros((3, 24), np.float32), x[:, :23]) == CL_INVALID_VALUE        # not whole blocks
    assert d.convolution_blocks(np.zeros((3, 16), np.float32), x) == CL_INVALID_VALUE                # out size
    assert d.convolution_blocks(np.zeros((3, 24), np.float32), x, x[:, :16]) == CL_INVALID_VALUE     # in2 size
    assert d.push_ir(np.zeros(16, np.float32)) == CL_INVALID_VALUE                                   # one row for three
    assert d.push_ir(np.zeros((3, 15), np.float32)) == CL_INVALID_VALUE
    assert d.convolution(np.zeros((3, 8), np.float32), np.zeros(8, np.float32)) == CL_INVALID_VALUE  # one block of one channel
    import torch
    t = torch.zeros((3, 24))
    assert d.process_blocks_device(torch.zeros((3, 16)), t, stream=0) == CL_INVALID_VALUE
    assert d.push_ir_device(torch.zeros((2, 16)), stream=0) == CL_INVALID_VALUE
    with pytest.raises(ValueError):
        d.process_blocks_device(torch.zeros(24), torch.zeros(24), stream=0)   # 1-D needs channels == 1
    # a bad geometry or no device: the object keeps its creation error and every call returns it
    bad = fa.Cldconv(0, 16, 8, errs=lambda s, u: None, channels=0)
    e = bad.get_cl_err()
    assert e in (CL_INVALID_VALUE, CL_DEVICE_NOT_FOUND) and e != 0
    if fa.device_count() == 0:
        assert d.get_cl_err() == CL_DEVICE_NOT_FOUND and len(msgs) == 1
        assert d.convolution_blocks(np.zeros_like(x), x) == CL_DEVICE_NOT_FOUND
        assert d.process_blocks_device(torch.zeros_like(t), t, stream=0) == CL_DEVICE_NOT_FOUND
        assert d.blocks_kernel_name() == "" and d.blocks_workspace_bytes() == 0
