"""numpy restatement of the two-input operations on (amp, freq) frames of clfa_pvoc (include/clfft_amd.h): cross, morph,
filter, mix and vocode — in float32, operation by operation (what the device results of ops 0..3 are compared with bit
for bit; the vocoder's envelopes go through the device's logf / expf and transforms, which are not numpy's), and the
vocoder's amplitudes once more in float64 (the truth they are measured against).  Frames are (channels, F, M + 1, 2)
float32; p and q are numbers or (F,) arrays."""
import numpy as np

from tests import pvoc_ops_model as om

f32 = np.float32
CROSS, MORPH, FILTER, MIX, VOCODE = range(5)


def clamp(x):
    """fminf(fmaxf(x, 0), 1): a NaN gives 0"""
    return np.fmin(np.fmax(np.asarray(x, f32), f32(0)), f32(1))


def _per_frame(x, F):
    """(1, F, 1) float32 of a number or an (F,) array; None stays None"""
    return None if x is None else np.broadcast_to(np.asarray(x, f32), (F,)).reshape(1, F, 1)


def _select(w, x0, x1, mid):
    """x0 (bits) where w == 0, x1 (bits) where w == 1, else mid"""
    out = np.ascontiguousarray(mid, f32).copy()
    w = np.broadcast_to(w, out.shape)
    u, u0, u1 = out.view(np.uint32), np.ascontiguousarray(x0).view(np.uint32), np.ascontiguousarray(x1).view(np.uint32)
    u[w == 0] = u0[w == 0]
    u[w == 1] = u1[w == 1]
    return out


def _morph(x0, x1, w):
    d = x1 - x0
    s = w * d
    return _select(w, x0, x1, x0 + s)


def pair32(op, a, b, p, q, size, sr, coefs=1):
    """float32 model of op 0..4 -> frames (C, F, M + 1, 2) float32; size and sr belong to the object (no rule uses them)"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    assert a.shape == b.shape and a.shape[2] == size // 2 + 1
    F = a.shape[1]
    P, Q = _per_frame(p, F), _per_frame(q, F)
    aa, af, ba, bf = a[..., 0], a[..., 1], b[..., 0], b[..., 1]
    out = np.empty_like(a)
    with np.errstate(all="ignore"):
        if op == CROSS:
            x, y = aa * P, ba * Q
            out[..., 0], out[..., 1] = x + y, af
        elif op == MORPH:
            out[..., 0], out[..., 1] = _morph(aa, ba, clamp(P)), _morph(af, bf, clamp(Q))
        elif op == FILTER:
            d = clamp(P)
            u, w = f32(1) - d, d * ba
            m = np.where(np.broadcast_to(d, aa.shape) == 0, f32(1), u + w)
            x = aa * m
            out[..., 0], out[..., 1] = Q * x, af
        elif op == MIX:
            take_b = (ba > aa)[..., None]           # a comparison with a NaN is false
            out = np.where(take_b, b.view(np.uint32), a.view(np.uint32)).view(f32)
        elif op == VOCODE:
            ea, eb = om.env32(aa, coefs), om.env32(ba, coefs)
            d = clamp(P)
            r = ea / eb
            u, w = f32(1) - d, d * r
            m = u + w
            x = ba * m
            out[..., 0], out[..., 1] = Q * x, bf
        else:
            raise ValueError(op)
    assert out.dtype == f32
    # the columns that are copies are copies of the bits
    if op in (CROSS, FILTER):
        out.view(np.uint32)[..., 1] = a.view(np.uint32)[..., 1]
    if op == VOCODE:
        out.view(np.uint32)[..., 1] = b.view(np.uint32)[..., 1]
    return out


def vocode64_amps(a, b, p, q, size, sr, coefs):
    """float64 amplitudes of the vocoder (p and q as the float32 values the call passes)"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    F = a.shape[1]
    d = clamp(_per_frame(p, F)).astype(np.float64)
    Q = _per_frame(q, F).astype(np.float64)
    with np.errstate(all="ignore"):
        r = om.env64(a[..., 0], coefs) / om.env64(b[..., 0], coefs)
        return Q * (b[..., 0].astype(np.float64) * ((1.0 - d) + d * r))
