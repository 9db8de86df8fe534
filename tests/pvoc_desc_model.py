"""numpy restatement of the per-frame descriptors of clfa_pvoc (include/clfft_amd.h, clfa_pvoc_desc_dev): magnitude, power,
moment, centroid, flux and peak of a range of bins — in float32, operation by operation (what the device results are
compared with bit for bit), and the sums once more in float64.  Frames are (channels, F, M + 1, 2) float32; a row of the
result is the eight columns MAG .. PEAK_BIN.  The sums follow the header's TREE SUM: never np.sum, which pairs differently.

`mutant` names one deliberate departure from the definition (tests/test_pvoc_desc_cpu.py shows that the compared values
notice each of them); None is the definition."""
import numpy as np

f32 = np.float32
MAG, POW, MOM, CENT, FLUX, PEAK_AMP, PEAK_FREQ, PEAK_BIN = range(8)
MUTANTS = ("serial", "halving", "nyquist_first", "w64", "fma", "tie_high", "state_range")
LANES = 256   # W = min(M, LANES)


def lanes(M, mutant=None):
    return min(M, 64 if mutant == "w64" else LANES)


def tree_sum(t, mutant=None, xy=None):
    """T(t) along the last axis (M + 1 float32 terms, those outside the range already +0).
    1. W = min(M, 256); p[j] = t[j], then t[j + W], t[j + 2W], ... (indices < M) are added in ascending order;
    2. while more than one value is left, s[i] = fl(s[2i] + s[2i+1]);
    3. T = fl(s[0] + t[M]).
    xy: the two factors of the terms, used by the "fma" mutant only (the product is then not rounded on its own)."""
    t = np.asarray(t, f32)
    M = t.shape[-1] - 1
    assert M >= 2 and M & (M - 1) == 0

    def add(acc, k):   # acc + t[k], k an index or a slice
        if mutant == "fma" and xy is not None:
            return (acc.astype(np.float64) + xy[0][..., k].astype(np.float64) * xy[1][..., k].astype(np.float64)).astype(f32)
        return acc + t[..., k]

    with np.errstate(all="ignore"):
        if mutant == "serial":
            acc = t[..., 0].copy()
            for k in range(1, M + 1):
                acc = add(acc, k)
            return acc
        W = lanes(M, mutant)
        p = t[..., :W].copy()
        if mutant == "nyquist_first":
            p[..., 0] = t[..., M] + t[..., 0]
        for r in range(1, M // W):
            p = add(p, slice(r * W, (r + 1) * W))
        while p.shape[-1] > 1:
            h = p.shape[-1] // 2
            p = p[..., :h] + p[..., h:] if mutant == "halving" else p[..., 0::2] + p[..., 1::2]
        T = p[..., 0] if mutant == "nyquist_first" else add(p[..., 0], M)
    assert T.dtype == f32
    return T


def bin_freqs(size, sr):
    """w[k] = fl((float)k cf), cf = (float)(sr / size): the EMPTY bin's freq"""
    return np.arange(size // 2 + 1, dtype=f32) * f32(sr / size)


def selection(M, first_bin=0, nbins=None):
    nbins = M + 1 - first_bin if nbins is None else nbins
    lo, hi = first_bin, first_bin + nbins - 1
    assert 0 <= lo <= hi <= M
    return lo, hi


def describe32(frames, last, size, sr, first_bin=0, nbins=None, rectify=False, mutant=None):
    """last: (C, M + 1) float32, the amps of the stream's previous frame -> (desc (C, F, 8), the new last)"""
    frames, last = np.ascontiguousarray(frames, f32), np.ascontiguousarray(last, f32)
    C, F, B, _ = frames.shape
    M = B - 1
    assert size == 2 * M and last.shape == (C, B)
    lo, hi = selection(M, first_bin, nbins)
    k = np.arange(B)
    sel = (k >= lo) & (k <= hi)
    zero = f32(0)
    a, fr = frames[..., 0], frames[..., 1]
    w = np.broadcast_to(bin_freqs(size, sr), a.shape)
    prev = np.concatenate([last[:, None], a[:, :F - 1]], axis=1) if F else a
    desc = np.zeros((C, F, 8), f32)
    with np.errstate(all="ignore"):
        am, wm = np.where(sel, a, zero), np.where(sel, w, zero)
        d = a - prev
        if rectify:
            d = np.where(d > 0, d, zero)       # a NaN is dropped
        dm = np.where(sel, d, zero)
        mag = tree_sum(am, mutant)
        mom = tree_sum(np.where(sel, a * w, zero), mutant, (am, wm))
        desc[..., MAG] = mag
        desc[..., POW] = tree_sum(np.where(sel, a * a, zero), mutant, (am, am))
        desc[..., MOM] = mom
        desc[..., CENT] = np.where(mag == 0, zero, mom / mag)
        desc[..., FLUX] = tree_sum(np.where(sel, d * d, zero), mutant, (dm, dm))
        # the peak: the lowest bin of the range whose amp is no NaN and >= every amp of the range that is no NaN
        valid = sel & ~np.isnan(a)
        top = np.max(np.where(valid, a, -np.inf), axis=-1, keepdims=True)
        cand = valid & (a == top)                                   # -0 == +0
        kp = (B - 1 - np.argmax(cand[..., ::-1], axis=-1)) if mutant == "tie_high" else np.argmax(cand, axis=-1)
        some = valid.any(axis=-1)
        pick = lambda x: np.take_along_axis(x, kp[..., None], axis=-1)[..., 0]
        desc[..., PEAK_AMP] = np.where(some, pick(a), zero)
        desc[..., PEAK_FREQ] = np.where(some, pick(fr), zero)
        desc[..., PEAK_BIN] = np.where(some, kp.astype(f32), f32(-1))
    if F:
        new = a[:, F - 1].copy()
        if mutant == "state_range":
            new = np.where(sel, new, last)
    else:
        new = last.copy()
    return desc, np.ascontiguousarray(new)


def sums64(frames, last, size, sr, first_bin=0, nbins=None, rectify=False):
    """(the sums MAG, POW, MOM, FLUX in float64 of the float32 terms, their sums of |term|): (C, F, 4) each — what the
    model's error bound is stated against"""
    frames, last = np.ascontiguousarray(frames, f32), np.ascontiguousarray(last, f32)
    C, F, B, _ = frames.shape
    lo, hi = selection(B - 1, first_bin, nbins)
    a = frames[..., 0]
    w = np.broadcast_to(bin_freqs(size, sr), a.shape)
    prev = np.concatenate([last[:, None], a[:, :F - 1]], axis=1)
    with np.errstate(all="ignore"):
        d = a - prev
        if rectify:
            d = np.where(d > 0, d, f32(0))
        terms = np.stack([a, a * a, a * w, d * d], axis=-2)[..., lo:hi + 1].astype(np.float64)
    return terms.sum(axis=-1), np.abs(terms).sum(axis=-1)


class Stream:
    """the descriptor state of one clfa_pvoc, and the call that advances it"""

    def __init__(self, channels, size, sr, mutant=None):
        self.channels, self.size, self.sr, self.mutant = channels, size, sr, mutant
        self.reset()

    def reset(self):
        self.last = np.zeros((self.channels, self.size // 2 + 1), f32)

    def run(self, frames, first_bin=0, nbins=None, rectify=False):
        desc, self.last = describe32(frames, self.last, self.size, self.sr, first_bin, nbins, rectify, self.mutant)
        return desc
