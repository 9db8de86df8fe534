"""The batch thresholds between an FFT plan's routes (opencl_fft_amd/csrc/fft_route.hpp), pinned on the device: the four
plans that change kernels with the batch, at the last batch of the few-transform route and the first of the fused one."""
import numpy as np
import pytest

import opencl_fft_amd as fa
from tests.util import assert_parity

pytestmark = pytest.mark.gpu


def _pack(x):
    """Clrfft forward in float64: amplitude scaling, DC / Nyquist in bin 0, bin M/2 left un-conjugated"""
    size = x.shape[-1]
    m = size // 2
    X = np.fft.fft(x.astype(np.float64), axis=-1)
    p = np.empty(x.shape[:-1] + (m,), np.complex128)
    p[..., 0] = X[..., 0].real / size + 1j * X[..., m].real / size
    p[..., 1:] = 2 * X[..., 1:m] / size
    p[..., m // 2] = np.conj(p[..., m // 2])
    return p


def _unpack(p):
    """Clrfft inverse in float64: the map above undone, then the real inverse transform"""
    m = p.shape[-1]
    size = 2 * m
    p = p.astype(np.complex128)
    X = np.empty(p.shape[:-1] + (m + 1,), np.complex128)
    X[..., 1:m] = p[..., 1:] * (size / 2)
    X[..., m // 2] = np.conj(X[..., m // 2])
    X[..., 0] = p[..., 0].real * size
    X[..., m] = p[..., 0].imag * size
    return np.fft.irfft(X, n=size, axis=-1)


# (real, size, the batch up to which the few-transform route runs, as a fraction of the CUs): complex 16384 and real 131072
# change at batch * 4 > CUs, real 32768 / 65536 at batch > CUs / 8
PLANS = [(False, 16384, 4), (True, 32768, 8), (True, 65536, 8), (True, 131072, 4)]


@pytest.mark.parametrize("fwd", [True, False], ids=["fwd", "inv"])
@pytest.mark.parametrize("real,size,div", PLANS, ids=["%s-%d" % ("real" if p[0] else "c2c", p[1]) for p in PLANS])
def test_route_boundaries(real, size, div, fwd):
    """batches 3, T, T + 1 and T + 6 of fixed-seed noise, T = the plan's threshold batch on this device: every transform
    against float64, transform 0 of batch T with the bits of batch 3's (both on the few-transform route) and transform 0
    of batch T + 1 with the bits of batch T + 6's (both on the fused kernel)"""
    import torch
    T = torch.cuda.get_device_properties(0).multi_processor_count // div
    assert T >= 3
    rng = np.random.default_rng(size + fwd)
    if real:
        r = rng.uniform(-1, 1, (T + 6, size)).astype(np.float32)
        x = r if fwd else np.ascontiguousarray(_pack(r).astype(np.complex64)).view(np.float32)
        want = _pack(x) if fwd else _unpack(x.view(np.complex64))
    else:
        x = rng.uniform(-1, 1, (T + 6, size, 2)).astype(np.float32)
        z = x.view(np.complex64).reshape(T + 6, size).astype(np.complex128)
        want = np.fft.fft(z, axis=-1) / size if fwd else np.fft.ifft(z, axis=-1) * size
    plan = (fa.Clrfft if real else fa.Clcfft)(0, size, fwd)
    assert plan.get_error() == 0, plan.get_log()
    first = {}
    for batch in (3, T, T + 1, T + 6):
        d = torch.from_numpy(x[:batch]).cuda()
        assert plan.exec_device(d, batch) == 0
        torch.cuda.synchronize()
        y = d.cpu().numpy().reshape(batch, -1)
        if fwd or not real:
            y = y.view(np.complex64)
        assert_parity(y, want[:batch], what="size %d batch %d" % (size, batch))
        first[batch] = y[0].copy().view(np.uint32)
    assert np.array_equal(first[T], first[3]), "batch T = %d left the few-transform route" % T
    assert np.array_equal(first[T + 1], first[T + 6]), "batch T + 1 = %d is not on the fused kernel" % (T + 1)
