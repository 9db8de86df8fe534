"""numpy restatement of the operations that reshape one stream of (amp, freq) frames of clfa_pvoc along the bins
(include/clfft_amd.h): band, mask, stencil, arp, lock and warp — in float32, operation by operation (what the device
results are compared with bit for bit; the warp's envelope goes through the device's logf / expf and transforms, which
are not numpy's), and the warp's amplitudes once more in float64 (the truth they are measured against).  Frames are
(channels, F, M + 1, 2) float32; the per-frame values are numbers or (F,) arrays, stacked into (F, 4) rows by rows()."""
import numpy as np

from tests import pvoc_ops_model as om
from tests.pvoc_pair_model import clamp

f32 = np.float32
BAND, MASK, STENCIL, ARP, LOCK, WARP = range(6)
COLS = {BAND: 4, MASK: 1, STENCIL: 2, ARP: 3, LOCK: 2, WARP: 3}


def rows(F, *cols):
    """the (F, 4) float32 rows of a call: one column per value (a number or an (F,) array), zeros in the rest"""
    r = np.zeros((F, 4), f32)
    for i, c in enumerate(cols):
        r[:, i] = np.broadcast_to(np.asarray(c, f32), (F,))
    return r


def _col(r, i):
    """column i of the rows as (1, F, 1)"""
    return np.ascontiguousarray(r[:, i]).reshape(1, -1, 1)


def _pick(cond, src, other):
    """the bits of src where cond, else other"""
    out = np.ascontiguousarray(np.broadcast_to(other, src.shape), f32).copy()
    cond = np.broadcast_to(cond, src.shape)
    out.view(np.uint32)[cond] = np.ascontiguousarray(src).view(np.uint32)[cond]
    return out


def band_gain(x, lc, lf, hf, hc, reject=False):
    """the band's gain at x = |freq|, float32 step by step; the arguments broadcast"""
    x, lc, lf, hf, hc = (np.asarray(v, f32) for v in (x, lc, lf, hf, hc))
    with np.errstate(all="ignore"):
        inside = (lc <= lf) & (lf <= hf) & (hf <= hc) & (x >= lc) & (x <= hc)      # a comparison with a NaN is false
        up = (x - lc) / (lf - lc)
        down = (hc - x) / (hc - hf)
        g = np.where(x < lf, up, np.where(x <= hf, f32(1), down))
        g = np.where(inside, g, f32(0)).astype(f32)
        if reject:
            g = f32(1) - g
    assert g.dtype == f32
    return g


def peaks(amp):
    """bin c is a peak: 2 <= c <= M-2 and amp[c] strictly above amp[c-2], amp[c-1], amp[c+1], amp[c+2] (a NaN: false)"""
    a = np.asarray(amp, f32)
    M = a.shape[-1] - 1
    p = np.zeros(a.shape, bool)
    with np.errstate(invalid="ignore"):
        c = a[..., 2:M - 1]
        p[..., 2:M - 1] = (c > a[..., 0:M - 3]) & (c > a[..., 1:M - 2]) & (c > a[..., 3:M]) & (c > a[..., 4:M + 1])
    return p


def lock_gather(frames, lock, tol):
    """the lock as the kernels compute it: every output bin looks for the peak next to it"""
    fr = np.ascontiguousarray(frames, f32)
    C, F, B, _ = fr.shape
    M = B - 1
    lock, tol = (np.broadcast_to(np.asarray(v, f32), (F,)) for v in (lock, tol))
    amp, freq = fr[..., 0], fr[..., 1]
    pk = peaks(amp)
    j = np.arange(1, M)
    up, down = pk[..., j + 1], pk[..., j - 1]
    cand = np.where(up, j + 1, np.where(down, j - 1, 0))
    with np.errstate(all="ignore"):
        Fc = np.take_along_axis(freq, cand, axis=-1)
        d = tol.reshape(1, F, 1) * np.abs(Fc)
        e = freq[..., 1:M] - Fc
        take = (up | down) & (np.abs(e) < d) & (lock != 0).reshape(1, F, 1)
    out = fr.copy()
    of = np.ascontiguousarray(out[..., 1])
    of[..., 1:M] = _pick(take, Fc, freq[..., 1:M])
    out.view(np.uint32)[..., 1] = of.view(np.uint32)
    return out


def warp_map(M, s, shift, lowest, bpf):
    """src[j] of the warp: k, om.EMPTY (the plain gain) or om.COPY; from the serial definition of the pitch scale's map"""
    src = np.full(M + 1, om.EMPTY, np.int64)
    src[0] = src[M] = om.COPY
    src[1:lowest] = om.COPY
    s = f32(s)
    with np.errstate(invalid="ignore", over="ignore"):
        t = f32(shift) * f32(bpf)
    if not (s >= f32(0.25) and s <= f32(4)) or not abs(t) <= f32(M):
        return src
    d = int(np.rint(t))
    smap = om.scale_map_serial(M, s)
    for j in range(lowest, M):
        jj = j - d
        if 1 <= jj <= M - 1 and smap[jj] >= 0:
            src[j] = smap[jj]
    return src


def _warp_amps(fr, r, size, sr, lowest, env, dtype):
    C, F, B, _ = fr.shape
    M = B - 1
    amp = fr[..., 0].astype(dtype)
    out = amp.copy()
    with np.errstate(all="ignore"):
        for f in range(F):
            src = warp_map(M, r[f, 0], r[f, 1], lowest, om.bpf_of(size, sr))
            gain = dtype(f32(r[f, 2]))
            j = np.nonzero(src != om.COPY)[0]
            g = gain * amp[:, f, j]
            k = src[j]
            moved = k >= 0
            kk = np.where(moved, k, j)
            w = g / env[:, f, j]
            x = w * env[:, f, kk]
            a = np.where(moved, x, g)
            assert a.dtype == dtype
            out[:, f, j] = a
    return out


def env_of(amp, coefs, dtype):
    """the cepstral envelope by the float32 or float64 model of tests/pvoc_ops_model.py"""
    if dtype == f32:
        return om.env32(amp, coefs)
    size = 2 * (amp.shape[-1] - 1)
    return om.env64(amp, coefs) if size * coefs <= 1 << 20 else om.env64_fft(amp, coefs)


def warp64_amps(frames, r, size, sr, lowest=1, coefs=1):
    """float64 amplitudes of the warp (the row's values as the float32 the call passes)"""
    fr = np.ascontiguousarray(frames, f32)
    return _warp_amps(fr, np.asarray(r, f32), size, sr, lowest, env_of(fr[..., 0], coefs, np.float64), np.float64)


def shape32(op, frames, r, size, sr, table=None, reject=False, lowest=1, coefs=1):
    """float32 model of op 0..5 -> frames (C, F, M + 1, 2) float32; r: the (F, 4) rows (rows())"""
    fr = np.ascontiguousarray(frames, f32)
    C, F, B, _ = fr.shape
    M = B - 1
    assert B == size // 2 + 1
    r = np.asarray(r, f32)
    assert r.shape == (F, 4)
    if op == LOCK:
        return lock_gather(fr, r[:, 0], r[:, 1])
    amp = fr[..., 0]
    tab = None if table is None else np.asarray(table, f32).reshape(1, 1, B)
    with np.errstate(all="ignore"):
        if op == BAND:
            g = band_gain(np.abs(fr[..., 1]), _col(r, 0), _col(r, 1), _col(r, 2), _col(r, 3), reject)
            a = _pick(g == 1, amp, np.where(g == 0, f32(0), amp * g))
        elif op == MASK:
            d = clamp(_col(r, 0))
            u, w = f32(1) - d, d * tab
            m = u + w
            a = _pick(d == 0, amp, amp * m)
        elif op == STENCIL:
            thr = tab * _col(r, 1)
            a = _pick(~(amp < thr), amp, amp * _col(r, 0))
        elif op == ARP:
            t = np.floor(clamp(_col(r, 0)) * f32(M)).astype(np.int64)
            m = f32(1) - clamp(_col(r, 1))
            a = _pick(m == 1, amp, amp * m)
            at = np.arange(B).reshape(1, 1, B) == t
            a = np.where(at, amp * _col(r, 2), a)
        elif op == WARP:
            a = _warp_amps(fr, r, size, sr, lowest, env_of(amp, coefs, f32), f32)
            a = _pick(np.isin(np.arange(B), np.r_[0:lowest, M]), amp, a)
        else:
            raise ValueError(op)
    assert a.dtype == f32
    out = fr.copy()
    out.view(np.uint32)[..., 0] = np.ascontiguousarray(a).view(np.uint32)
    return out
