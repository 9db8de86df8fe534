"""numpy restatement of the stereo demix by azimuth of clfa_pvoc (include/clfft_amd.h, clfa_pvoc_demix_dev): the side, the
scan over the P + 1 gains done literally, the signed azimuth, the window of a frame, the output frames and the azimuth
profile.  Every float32 operation is a numpy float32 operation, rounded on its own, so everything a test compares is bits.
The profile's sums are the descriptors' TREE SUM, taken from tests/pvoc_desc_model.py unchanged.

`mutant` names one deliberate departure from the definition (tests/test_pvoc_demix_cpu.py shows that the inputs of the GPU
test notice each of them).  The file also holds the input recipes of the demix tests (panned, pair) and their rows of
(pos, width); numpy only, so the tests without a device use them too."""
import numpy as np

from tests.pvoc_desc_model import selection, tree_sum
from tests.pvoc_inputs import SR, raw, raw_freq_first

f32 = np.float32
MUTANTS = ("tie_high", "side_ge", "h_plus", "h_minus", "c_trunc", "mag_mx", "freq_left", "nan_kept", "range_amps",
           "range_profile", "profile_serial", "g_recip")
POINTS_MAX = 1024


def gains(P, mutant=None):
    """g[n] = fl((float)n / (float)P), n = 0..P"""
    n = np.arange(P + 1, dtype=f32)
    g = n * (f32(1) / f32(P)) if mutant == "g_recip" else n / f32(P)
    assert g.dtype == f32
    return g


def scan(L, R, P, mutant=None):
    """the per-bin part, L and R float32 of any one shape: (left, placed, u, mag)"""
    L, R = np.asarray(L, f32), np.asarray(R, f32)
    g = gains(P, mutant)
    with np.errstate(all="ignore"):
        left = L >= R if mutant == "side_ge" else L > R        # a tie or a NaN is RIGHT
        loud, quiet = np.where(left, L, R), np.where(left, R, L)
        d = np.abs(quiet[..., None] - g * loud[..., None])      # (.., P + 1): a product and a difference, each rounded
        assert d.dtype == f32
        nan = np.isnan(d).any(-1)
        if mutant == "tie_high":
            nmin = P - np.argmin(d[..., ::-1], axis=-1)
        else:
            nmin = np.argmin(d, axis=-1)                        # the lowest n of the smallest d
        m, mx = d.min(-1), d.max(-1)
        mag = mx if mutant == "mag_mx" else mx - m
        placed = ~(mag <= 0) if mutant == "nan_kept" else ~nan & (mag > 0)
    u = np.where(left, nmin - P, P - nmin)
    return left, placed, u, mag


def window(par, P, mutant=None):
    """par (F, 2) rows of (pos, width) -> (c, H) per frame, the device form's clamps"""
    par = np.asarray(par, f32).reshape(-1, 2)
    pc = np.fmin(np.fmax(par[:, 0], f32(-1)), f32(1))           # fmaxf, fminf: a NaN gives -1
    t = pc * f32(P)
    c = (np.trunc(t) if mutant == "c_trunc" else np.rint(t)).astype(np.int64)
    w = np.fmin(np.fmax(par[:, 1], f32(1)), f32(2 * P + 1))     # a NaN gives 1
    H = w.astype(np.int64) // 2 + {"h_plus": 1, "h_minus": -1}.get(mutant, 0)
    return c, H


def values_ok(par, P):
    """what the blocking form accepts: pos finite in [-1, 1], width finite in [1, 2P + 1]"""
    par = np.asarray(par, f32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        return bool(np.all(np.isfinite(par)) and np.all((par[:, 0] >= -1) & (par[:, 0] <= 1))
                    and np.all((par[:, 1] >= 1) & (par[:, 1] <= 2 * P + 1)))


def demix(left, right, par, P, first_bin=0, nbins=None, az=True, mutant=None):
    """left, right (C, F, M + 1, 2) float32, par (F, 2) -> (frames, profile (C, F, 2P + 1) or None)"""
    left, right = np.ascontiguousarray(left, f32), np.ascontiguousarray(right, f32)
    C, F, B, _ = left.shape
    assert right.shape == left.shape and 1 <= P <= POINTS_MAX
    lo, hi = selection(B - 1, first_bin, nbins)
    k = np.arange(B)
    sel = (k >= lo) & (k <= hi)
    c, H = window(par, P, mutant)
    assert c.shape == (F,)
    out = np.zeros((C, F, B, 2), f32)
    prof = np.zeros((C, F, 2 * P + 1), f32) if az else None
    zero = f32(0)
    for ch in range(C):                                         # a channel at a time: the scan is (F, B, P + 1) floats
        isleft, placed, u, mag = scan(left[ch, ..., 0], right[ch, ..., 0], P, mutant)
        if mutant == "freq_left":
            isleft_f = np.ones_like(isleft)
        else:
            isleft_f = isleft
        out[ch, ..., 1].view(np.uint32)[:] = np.where(isleft_f, left[ch, ..., 1].view(np.uint32), right[ch, ..., 1].view(np.uint32))
        inr = np.ones_like(sel) if mutant == "range_amps" else sel
        kept = placed & inr & (np.abs(u - c[:, None]) <= H[:, None])
        out[ch, ..., 0] = np.where(kept, mag, zero)
        if az:
            inp = placed if mutant == "range_profile" else placed & sel
            for j in range(2 * P + 1):
                t = np.where(inp & (u == j - P), mag, zero)
                prof[ch, :, j] = tree_sum(t, "serial" if mutant == "profile_serial" else None)
    return out, prof


# ---- the inputs ----------------------------------------------------------------------------------------------------

POSITIONS = (-1.0, -0.0, 0.37, 1.0)


def par_rows(F, P, turn=0):
    """rows of (pos, width) that walk the widths 1, 4, 2P + 1 and the positions -1, -0.0, 0.37, 1: frame f takes
    combination f + turn, so 12 frames see all of them"""
    widths = (1.0, 4.0, 2.0 * P + 1)
    i = np.arange(F) + turn
    return np.stack([np.array(POSITIONS, f32)[i % 4], np.array(widths, f32)[(i // 4) % 3]], axis=1).astype(f32)


def edge_rows(F, P):
    """the device form's edge values: a NaN, infinities and values outside [-1, 1] and [1, 2P + 1], each of which the
    kernel clamps"""
    vals = np.array([[np.nan, 3], [0.5, np.nan], [-7, 0], [7, -5], [np.inf, np.inf], [-np.inf, -np.inf], [0.1, 1e9],
                     [-0.0, 0.5], [0.37, 2 * P + 2], [1, 2.9]], f32)
    return vals[np.arange(F) % len(vals)]


def _freqs(rng, shape):
    return rng.uniform(-SR, SR, shape).astype(f32)


def panned(size, C, F, P, seed, pans=None):
    """Stereo frames whose bins are sources at planted pans: bin k has a loud amp on one side and quiet = fl(g[n] loud) on
    the other, so its d[n] is exactly 0.  pans: a list of (side, n), side -1 (LEFT) or +1 (RIGHT), dealt over the bins at
    random; None: every n of either side.  A sixth of the bins are instead at no gain of the grid (quiet = loud times a
    random factor), and with P a power of two some bins are exactly tied between n and n + 1 (loud a power of two,
    quiet = loud (n + 0.5) / P), some have L == R.  Frame 0 carries the odd bins: both amps 0, one amp 0, a negative amp on
    either side, both negative, an infinity and a NaN on either side.  Returns (left, right, source), source (C, F, B) the
    index into pans of the bin's planted source or -1 (read-only, the draws in this order)."""
    rng = np.random.default_rng(seed)
    B = size // 2 + 1
    g = gains(P)
    if pans is None:
        plain = False
        pans = [(-1, n) for n in range(P + 1)] + [(1, n) for n in range(P + 1)]
    else:
        plain = True
    src = rng.integers(0, len(pans), (C, F, B))
    side = np.array([p[0] for p in pans])[src]
    n = np.array([p[1] for p in pans])[src]
    loud = (2.0 ** rng.uniform(-6, 6, (C, F, B))).astype(f32)
    quiet = g[n] * loud
    if not plain:
        off = rng.random((C, F, B)) < 1 / 6
        quiet = np.where(off, (loud * rng.random((C, F, B)).astype(f32)).astype(f32), quiet)
        src = np.where(off, -1, src)
        if P & (P - 1) == 0:
            tie = rng.random((C, F, B)) < 1 / 8
            tl = (2.0 ** rng.integers(-3, 4, (C, F, B))).astype(f32)
            tq = (tl * ((rng.integers(0, P, (C, F, B)) + 0.5) / P)).astype(f32)      # exact: P and tl are powers of two
            loud, quiet, src = np.where(tie, tl, loud), np.where(tie, tq, quiet), np.where(tie, -1, src)
        same = rng.random((C, F, B)) < 1 / 16
        quiet, src = np.where(same, loud, quiet), np.where(same, -1, src)
    L = np.where(side < 0, loud, quiet).astype(f32)
    R = np.where(side < 0, quiet, loud).astype(f32)
    if not plain:
        odd = [(0, 0), (0, 1.5), (2.5, 0), (-1, 0.5), (0.5, -1), (-2, -1), (-1, -2), (np.inf, 1), (1, np.inf), (np.inf, np.inf),
               (-np.inf, 1), (np.nan, 1), (1, np.nan), (np.nan, np.nan), (-0.0, 0.0), (3e38, -3e38), (1e-45, 1e-40)]
        at = 5 + np.arange(len(odd)) % (B - 6)
        for ch in range(C):
            for i, (a, b) in enumerate(odd):
                L[ch, 0, at[i]], R[ch, 0, at[i]] = a, b
                src[ch, 0, at[i]] = -1
    left = np.stack([L, _freqs(rng, L.shape)], axis=-1)
    right = np.stack([R, _freqs(rng, R.shape)], axis=-1)
    for a in (left, right, src):
        a.setflags(write=False)
    return left, right, src


def pair(size, C, F, seed):
    """two unrelated streams as the two sides: tests/pvoc_inputs.py's raw frames against its raw frames with NaN amps and
    freqs"""
    return raw(size, C, F, seed), raw_freq_first(size, C, F, seed + 1)
