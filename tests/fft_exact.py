"""Exact (float64) transforms of impulses under the reference's conventions, and a float32 model of Bluestein's algorithm.

A delta of amplitude a at position j transforms to a w^(jk) (/ n forward): every bin has the same magnitude, so the
criterion max|err| / max|ref| of tests/util.py is the worst SINGLE bin, and each bin is one product of twiddle-table
entries of the kernel under test.  Everything here runs on the CPU in float64; the tests that use it are
tests/test_fft_exact_cpu.py (the oracle against these helpers) and tests/test_gpu_fft_impulses.py (the HIP kernels).

Conventions (cl_fft.cpp:29-41, 178-205): complex forward scaled by 1 / n with exp(-i ...), inverse unscaled with exp(+i ...);
packed real spectra P[0] = (DC, Nyquist) / size, P[k] = 2 X[k] / size, P[M/2] left un-conjugated.
"""
import numpy as np

CHUNK_BYTES = 64 << 20      # live float64 result per chunk of the *_chunks generators (at least one row)


def impulse_positions(n, cap=None):
    """The delta positions whose transforms touch every entry of the per-stage twiddle tables: all of them for n <= 1024
    (the batch is the identity, the output the whole DFT matrix); above, every j < 256 (the low digit of every radix-16 /
    radix-256 split), every multiple of 256 up to 256 * 255 below n (the high digit), n - 1 and n / 2 + 1.  cap: at most that
    many, spread evenly over the family, with 0, 1, n / 2 + 1 and n - 1 kept."""
    if n <= 1024:
        js = np.arange(n, dtype=np.int64)
    else:
        hi = np.arange(0, 256 * 256, 256, dtype=np.int64)
        js = np.unique(np.concatenate([np.arange(256, dtype=np.int64), hi[hi < n], [n - 1, n // 2 + 1]]))
    if cap is not None and js.size > cap:
        keep = np.array([j for j in (0, 1, n // 2 + 1, n - 1) if 0 <= j < n], dtype=np.int64)
        rest = js[np.round(np.linspace(0, js.size - 1, max(cap - keep.size, 0))).astype(np.int64)]
        js = np.unique(np.concatenate([keep, rest]))
    return js


def real_positions(size, cap=None):
    """impulse_positions for packed real plans: j < 256, the multiples of 256 (up to 256 * 255), size / 2 +- 1, size - 1"""
    hi = np.arange(0, 256 * 256, 256, dtype=np.int64)
    js = np.concatenate([np.arange(min(256, size), dtype=np.int64), hi[hi < size], [size // 2 - 1, size // 2 + 1, size - 1]])
    js = np.unique(js[(js >= 0) & (js < size)])
    if cap is not None and js.size > cap:
        keep = np.array([0, 1, size // 2 - 1, size // 2 + 1, size - 1], dtype=np.int64)
        rest = js[np.round(np.linspace(0, js.size - 1, max(cap - keep.size, 0))).astype(np.int64)]
        js = np.unique(np.concatenate([keep, rest]))
    return js


def real_bins(size, cap=None):
    """the same index set taken as bins of the packed spectrum (those below M = size / 2), plus bin 0 and bin M / 2"""
    m = size // 2
    js = real_positions(size, cap)
    return np.unique(np.concatenate([js[js < m], [0, m // 2]]))


def _table(n, sign):
    """E[t] = exp(sign 2 pi i t / n), t < n, float64"""
    a = np.arange(n, dtype=np.float64) * (2.0 * np.pi / n)
    return np.cos(a) + (1j * sign) * np.sin(a)


def _row_chunks(rows, n):
    step = max(1, CHUNK_BYTES // (16 * n))
    for lo in range(0, rows, step):
        yield lo, min(rows, lo + step)


def cfft_impulse_chunks(n, js, fwd, amp=1.0):
    """yields (lo, hi, complex128[hi - lo, n]): rows lo..hi of cfft_impulses(), at most CHUNK_BYTES each (one row at least)"""
    js = np.asarray(js, dtype=np.int64).reshape(-1)
    E = _table(n, -1.0 if fwd else 1.0) * (complex(amp) / n if fwd else complex(amp))
    k = np.arange(n, dtype=np.int64)
    for lo, hi in _row_chunks(js.size, n):
        yield lo, hi, E[(js[lo:hi, None] * k[None, :]) % n]        # int64: j k < 2^48


def cfft_impulses(n, js, fwd, amp=1.0):
    """complex128[len(js), n]: row r = Clcfft(n, fwd) of amp * delta(. - js[r])"""
    js = np.asarray(js, dtype=np.int64).reshape(-1)
    out = np.empty((js.size, n), np.complex128)
    for lo, hi, blk in cfft_impulse_chunks(n, js, fwd, amp):
        out[lo:hi] = blk
    return out


def rfft_impulse_chunks(size, js, amp=1.0):
    js = np.asarray(js, dtype=np.int64).reshape(-1)
    m = size // 2
    E = _table(size, -1.0) * (2.0 * amp / size)
    k = np.arange(m, dtype=np.int64)
    for lo, hi in _row_chunks(js.size, m):
        j = js[lo:hi]
        blk = E[(j[:, None] * k[None, :]) % size]                  # 2 X[k] / size
        blk[:, 0] = (amp / size) * (1.0 + 1j * np.where(j & 1, -1.0, 1.0))     # X[0] = a, X[M] = a (-1)^j
        blk[:, m // 2] = np.conj(blk[:, m // 2])
        yield lo, hi, blk


def rfft_impulses(size, js, amp=1.0):
    """complex128[len(js), size / 2]: the packed spectrum Clrfft(size, forward) gives for the real signal amp * delta(. - js[r])
    (amplitude scaling, bin 0 = (DC, Nyquist), bin M/2 left un-conjugated: the formula of test_rfft_any_length)"""
    js = np.asarray(js, dtype=np.int64).reshape(-1)
    out = np.empty((js.size, size // 2), np.complex128)
    for lo, hi, blk in rfft_impulse_chunks(size, js, amp):
        out[lo:hi] = blk
    return out


def irfft_single_bin_chunks(size, ks, value):
    """The reference's inverse map (cl_fft.cpp:192-205) on a spectrum with P[k] = value alone: bin 0 -> c[0] = (re + im, re - im);
    bin M/2 untouched; a bin 0 < k < M, k != M/2, lands in c[k] and c[M - k]; then the unscaled M-point inverse, whose real and
    imaginary parts are the even and odd samples."""
    ks = np.asarray(ks, dtype=np.int64).reshape(-1)
    m = size // 2
    v = complex(value)
    E = _table(m, 1.0)
    W = _table(size, 1.0)                                           # w2[i] = exp(+ i pi i / M)
    t = np.arange(m, dtype=np.int64)
    for lo, hi in _row_chunks(ks.size, 2 * m):
        k = ks[lo:hi]
        own = k < m // 2
        i = np.where(own, k, m - k) % m                             # the pair (i, j = M - i) bin k belongs to
        ci, cj = np.where(own, v, 0j), np.where(own, 0j, np.conj(v))   # c[i], conj(c[j])
        e, o = 0.5 * (ci + cj), 0.5j * (ci - cj)
        p = W[i] * o
        z = (e + p)[:, None] * E[(i[:, None] * t) % m] + np.conj(e - p)[:, None] * E[((m - i)[:, None] * t) % m]
        z[k == 0] = complex(v.real + v.imag, v.real - v.imag)
        if np.any(k == m // 2):
            z[k == m // 2] = v * E[((m // 2) * t) % m]
        out = np.empty((hi - lo, size), np.float64)
        out[:, 0::2], out[:, 1::2] = z.real, z.imag
        yield lo, hi, out


def irfft_single_bins(size, ks, value=1.0):
    """float64[len(ks), size]: Clrfft(size, inverse) of the packed spectrum whose only non-zero bin is P[ks[r]] = value"""
    ks = np.asarray(ks, dtype=np.int64).reshape(-1)
    out = np.empty((ks.size, size), np.float64)
    for lo, hi, blk in irfft_single_bin_chunks(size, ks, value):
        out[lo:hi] = blk
    return out


def bluestein_f32(x, n, fwd):
    """float32 model of the lengths the reference does not have: Bluestein's algorithm with the chirp w[k] = exp(-+ i pi k^2 / n)
    evaluated in float64 and rounded once to complex64, the products in complex64, and the two convolution transforms of length
    m = the next power of two >= 2 n - 1 run by the oracle's plans (the filter's spectrum, a table, is rounded once from float64).
    complex64[..., n] -> complex64[..., n], forward divided by n.  Valid for m <= 65536 (the oracle's range)."""
    from oracle import oracle
    x = np.asarray(x, dtype=np.complex64)
    m = 1 << int(np.ceil(np.log2(max(2 * n - 1, 2))))
    k = np.arange(n, dtype=np.int64)
    ang = ((k * k) % (2 * n)).astype(np.float64) * (np.pi / n)
    w64 = np.cos(ang) + (-1j if fwd else 1j) * np.sin(ang)
    w = w64.astype(np.complex64)
    b = np.zeros(m, np.complex128)
    b[:n] = np.conj(w64)
    b[m - n + 1:] = np.conj(w64[1:][::-1])
    B = np.fft.fft(b).astype(np.complex64)
    a = np.zeros(x.shape[:-1] + (m,), np.complex64)
    a[..., :n] = x * w
    A = oracle.cfft(a, True)                                        # FFT(a) / m
    y = oracle.cfft((A * B).astype(np.complex64), False)            # (a conv b) / m ... times m from the unscaled inverse
    y = y[..., :n] * w
    return (y * np.float32(1.0 / n) if fwd else y).astype(np.complex64)
