"""CPU tests of tests/fft_exact.py: the float64 impulse helpers against numpy's FFT, and the oracle (the reference's
arithmetic in float32) against the helpers on the impulse families — "the reference alone stays within the per-bin bar",
which is what entitles tests/test_gpu_fft_impulses.py to hold the HIP kernels to TOL per bin."""
import numpy as np
import pytest

from oracle import oracle
from tests import fft_exact as fx
from tests.util import TOL, assert_parity, rel_err

AMP = 1 - 0.5j


# ---- the helpers are the DFT (linearity: dense input = a sum of deltas) -------------------------------------------------

@pytest.mark.parametrize("n", [2, 3, 16, 100, 256, 1000])
def test_cfft_impulses_equal_numpy(n):
    rng = np.random.default_rng(n)
    x = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
    js = np.arange(n)
    assert np.allclose(x @ fx.cfft_impulses(n, js, True), np.fft.fft(x) / n, rtol=0, atol=1e-13)
    assert np.allclose(x @ fx.cfft_impulses(n, js, False), np.fft.ifft(x) * n, rtol=0, atol=1e-13 * n)
    assert np.allclose(fx.cfft_impulses(n, js[:2], True, AMP), AMP * fx.cfft_impulses(n, js[:2], True), rtol=0, atol=1e-15)


def test_cfft_impulses_large_index_and_chunks(monkeypatch):
    """j k beyond 2^31 (int64 index), and the chunked generator against the one-piece result"""
    n = 1 << 17
    js = np.array([n - 1, n // 2 + 1, 65537])
    got = fx.cfft_impulses(n, js, True)
    x = np.zeros((3, n))
    x[np.arange(3), js] = 1
    assert np.allclose(got, np.fft.fft(x, axis=-1) / n, rtol=0, atol=1e-15)
    monkeypatch.setattr(fx, "CHUNK_BYTES", 16 * n)       # one row per chunk
    parts = list(fx.cfft_impulse_chunks(n, js, True))
    assert [(lo, hi) for lo, hi, _ in parts] == [(0, 1), (1, 2), (2, 3)]
    assert np.array_equal(np.concatenate([b for _, _, b in parts]), got)


def _pack64(x):
    """the packing rules of test_rfft_any_length on a float64 FFT"""
    size = x.shape[-1]
    m = size // 2
    X = np.fft.fft(x, axis=-1)
    want = np.empty(x.shape[:-1] + (m,), np.complex128)
    want[..., 0] = X[..., 0].real / size + 1j * X[..., m].real / size
    want[..., 1:] = 2 * X[..., 1:m] / size
    want[..., m // 2] = np.conj(want[..., m // 2])
    return want


@pytest.mark.parametrize("size", [4, 8, 12, 64, 1000])
def test_rfft_impulses_equal_numpy(size):
    x = np.random.default_rng(size).uniform(-1, 1, size)
    assert np.allclose(x @ fx.rfft_impulses(size, np.arange(size)), _pack64(x), rtol=0, atol=1e-13)


@pytest.mark.parametrize("size", [4, 8, 12, 64, 1000])
def test_irfft_single_bins_equal_numpy(size):
    """a dense packed spectrum is a real-linear sum of single bins with values 1 and i; numpy's irfft of the unpacked
    one-sided spectrum is the independent formula (bin 0 carries DC and Nyquist, bin M/2 is conjugated)"""
    m = size // 2
    rng = np.random.default_rng(size)
    p = rng.uniform(-1, 1, m) + 1j * rng.uniform(-1, 1, m)
    ks = np.arange(m)
    got = p.real @ fx.irfft_single_bins(size, ks, 1.0) + p.imag @ fx.irfft_single_bins(size, ks, 1j)
    X = np.empty(m + 1, np.complex128)
    X[:m] = p * (size / 2)
    X[0], X[m] = p[0].real * size, p[0].imag * size
    X[m // 2] = np.conj(p[m // 2]) * (size / 2)
    assert np.allclose(got, np.fft.irfft(X, n=size), rtol=0, atol=1e-12)
    assert np.allclose(fx.irfft_single_bins(size, ks, AMP), fx.irfft_single_bins(size, ks, 1.0) - 0.5 * fx.irfft_single_bins(size, ks, 1j),
                       rtol=0, atol=1e-15)


def test_impulse_positions():
    assert np.array_equal(fx.impulse_positions(1024), np.arange(1024))
    js = fx.impulse_positions(65536)
    assert js.size == 513 and {0, 255, 256, 256 * 255, 32769, 65535} <= set(js.tolist())
    js = fx.impulse_positions(4096)
    assert js.size == 256 + 15 + 2 and js.max() == 4095
    for n, cap in ((1000, 300), (65536, 72), (8192, 100)):
        js = fx.impulse_positions(n, cap)
        assert js.size <= cap and {0, 1, n // 2 + 1, n - 1} <= set(js.tolist()) and np.all(np.diff(js) > 0)
    ks = fx.real_bins(131072)
    assert ks.max() < 65536 and {0, 32768, 65535} <= set(ks.tolist())


# ---- the oracle on the impulse families: worst bin within TOL ---------------------------------------------------------------

def _delta_batch(n, js, amp, dtype):
    x = np.zeros((len(js), n), dtype)
    x[np.arange(len(js)), js] = amp
    return x


@pytest.mark.parametrize("n", [1 << k for k in range(1, 17)])
def test_oracle_cfft_impulses_within_tol(n):
    js = fx.impulse_positions(n)
    for fwd in (True, False):
        worst = 0.0
        for lo, hi, want in fx.cfft_impulse_chunks(n, js, fwd, AMP):
            got = oracle.cfft(_delta_batch(n, js[lo:hi], AMP, np.complex64), fwd)
            worst = max(worst, assert_parity(got, want, what="oracle c2c n=%d fwd=%s rows %d.." % (n, fwd, lo))[1])
        print("ORACLE c2c n=%d %s worst-bin %.3g" % (n, "fwd" if fwd else "inv", worst))


@pytest.mark.parametrize("size", [1 << k for k in range(2, 18)])
def test_oracle_rfft_impulses_within_tol(size):
    js = fx.real_positions(size)
    worst = 0.0
    for lo, hi, want in fx.rfft_impulse_chunks(size, js, 0.75):
        got = oracle.rfft_forward(_delta_batch(size, js[lo:hi], 0.75, np.float32))
        worst = max(worst, assert_parity(got, want, what="oracle r2c size=%d rows %d.." % (size, lo))[1])
    ks = fx.real_bins(size)
    worst_i = 0.0
    for lo, hi, want in fx.irfft_single_bin_chunks(size, ks, AMP):
        got = oracle.rfft_inverse(_delta_batch(size // 2, ks[lo:hi], AMP, np.complex64))
        worst_i = max(worst_i, assert_parity(got, want, what="oracle c2r size=%d rows %d.." % (size, lo))[1])
    print("ORACLE real size=%d fwd worst-bin %.3g inv worst-sample %.3g" % (size, worst, worst_i))


@pytest.mark.parametrize("n", [3, 100, 1000, 4095])
def test_bluestein_model_within_tol(n):
    js = fx.impulse_positions(n, 300)
    for fwd in (True, False):
        got = fx.bluestein_f32(_delta_batch(n, js, AMP, np.complex64), n, fwd)
        _, mx = assert_parity(got, fx.cfft_impulses(n, js, fwd, AMP), what="bluestein model n=%d fwd=%s" % (n, fwd))
        print("MODEL bluestein n=%d %s worst-bin %.3g" % (n, "fwd" if fwd else "inv", mx))
    rng = np.random.default_rng(n)
    x = (rng.uniform(-1, 1, (2, n)) + 1j * rng.uniform(-1, 1, (2, n))).astype(np.complex64)
    assert rel_err(fx.bluestein_f32(x, n, True), np.fft.fft(x.astype(np.complex128), axis=-1) / n)[0] < TOL


# ---- the oracle refuses what the reference cannot compute ---------------------------------------------------------------------

def test_oracle_refuses_lengths_outside_the_reference_range():
    """above n = 65536 the reference's stage index g * n2 overflows int32 (cl_fft.cpp:32); the C restatement used to follow it
    out of the array (glibc: "corrupted size vs. prev_size") and now answers CL_INVALID_VALUE, the wrappers ValueError"""
    for n in (1, 3, 100, 1 << 17, 1 << 20):
        with pytest.raises(ValueError):
            oracle.cfft(np.zeros(n, np.complex64), True)
    for size in (2, 6, 1000, 1 << 18, 1 << 21):
        with pytest.raises(ValueError):
            oracle.rfft_forward(np.zeros(size, np.float32))
        with pytest.raises(ValueError):
            oracle.rfft_inverse(np.zeros(size // 2, np.complex64))
    import ctypes as C
    buf = np.zeros(2 << 17, np.float32)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    L = oracle.lib()
    assert L.orc_cfft(fp, 1 << 17, 1) == -30 and L.orc_cfft_batched(fp, 1 << 17, 1, 1, 1) == -30
    assert L.orc_rfft(fp, 1 << 18, 1) == -30 and L.orc_rfft_batched(fp, 1 << 18, 1, 0, 1) == -30
    assert not buf.any()
    # the ends of the range still run
    assert oracle.cfft(np.ones(65536, np.complex64), True)[0] == pytest.approx(1.0)
    assert oracle.rfft_forward(np.ones(131072, np.float32))[0].real == pytest.approx(1.0)
