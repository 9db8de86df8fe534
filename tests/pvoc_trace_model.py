"""numpy restatement of the N loudest bins of clfa_pvoc (include/clfft_amd.h, clfa_pvoc_trace_dev): the count, the order
with its tie rule, the selection, the frames with and without RESIDUAL and the bin list.  There is no arithmetic on the
values in the definition, so everything a test compares is bits.

`mutant` names one deliberate departure from the definition (tests/test_pvoc_trace_cpu.py shows that the inputs of the GPU
test notice each of them).  The file also holds the input recipes of the trace tests that tests/pvoc_inputs.py does not
have (levels, near_keys), their n rows and their ranges; numpy only, so the tests without a device use them too."""
import numpy as np

from tests.pvoc_inputs import SR

f32 = np.float32
MUTANTS = ("tie_high", "ties_kept", "nan_loudest", "neg_zero_low", "raw_bits", "abs", "range_ignored", "n_rounded")
LEVELS = np.array([0.0, -0.0, 1e-40, 0.25, 0.25, 1.0, 1.0, 3.0, -2.0, np.inf], f32)


def counts(n, nbins, mutant=None):
    """N per frame: 0 where n >= 0 does not hold, else (int)floorf(fminf(n, (float)nbins))"""
    n = np.asarray(n, f32)
    ok = n >= 0                                   # False for a NaN
    m = np.minimum(np.where(ok, n, f32(0)), f32(nbins))
    m = np.rint(m) if mutant == "n_rounded" else np.floor(m)
    return np.where(ok, m, 0).astype(np.int64)


def selected(amp, n, first_bin=0, nbins=None, mutant=None):
    """the SELECTED bins of amp (C, F, B) as a bool array"""
    C, F, B = amp.shape
    nbins = B - first_bin if nbins is None else nbins
    N = counts(n, nbins, mutant)
    lo, hi = (0, B - 1) if mutant == "range_ignored" else (first_bin, first_bin + nbins - 1)
    inr = np.zeros(B, bool)
    inr[lo:hi + 1] = True
    nan = np.isnan(amp)
    cand = inr & (np.ones_like(nan) if mutant == "nan_loudest" else ~nan)
    # the sort value: ascending = louder first.  float64 holds every float32 and leaves room below -0
    if mutant == "raw_bits":
        v = -amp.view(np.uint32).astype(np.float64)
    elif mutant == "abs":
        v = -np.abs(amp).astype(np.float64)
    else:
        v = -amp.astype(np.float64)               # -0 == +0
        if mutant == "neg_zero_low":
            v[(amp == 0) & np.signbit(amp)] = 1e-300
    v = np.where(nan, -np.inf, v)                 # only the mutant has them among the candidates
    keys = (v, ~nan, ~cand)                       # lexsort: the last key first; it is stable, so the lower bin wins a tie
    if mutant == "tie_high":
        order = B - 1 - np.lexsort(tuple(k[..., ::-1] for k in keys), axis=-1)
    else:
        order = np.lexsort(keys, axis=-1)
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(B), order.shape), axis=-1)
    sel = cand & (rank < N[None, :, None])
    if mutant == "ties_kept":                     # Csound's rule: everything >= the N-th loudest amp
        ncand = cand.sum(-1)
        k = np.clip(np.minimum(N[None, :], ncand) - 1, 0, B - 1)
        thr = np.take_along_axis(amp, np.take_along_axis(order, k[..., None], -1), -1)
        sel = cand & (amp >= thr) & (np.minimum(N[None, :], ncand) > 0)[..., None]
    return sel


def trace(x, n, first_bin=0, nbins=None, residual=False, list_n=0, mutant=None):
    """x (C, F, B, 2) float32, n (F,) -> (frames, bins); bins (C, F, list_n) int32, or None for list_n == 0"""
    x = np.ascontiguousarray(x, dtype=f32)
    C, F, B, _ = x.shape
    nbins = B - first_bin if nbins is None else nbins
    sel = selected(x[..., 0], n, first_bin, nbins, mutant)
    lo, hi = (0, B - 1) if mutant == "range_ignored" else (first_bin, first_bin + nbins - 1)
    inr = np.zeros(B, bool)
    inr[lo:hi + 1] = True
    out = x.copy().view(np.uint32)
    keep = ~inr | (sel != bool(residual))
    out[..., 0] = np.where(keep, out[..., 0], np.uint32(0))
    bins = None
    if list_n > 0:
        bins = np.full((C, F, list_n), -1, np.int32)
        pos = np.cumsum(sel, axis=-1) - 1
        c, f, k = np.nonzero(sel & (pos < list_n))
        bins[c, f, pos[c, f, k]] = k
    return out.view(f32), bins


def brute_selected(amp, n, first_bin, nbins):
    """the definition word for word, one frame at a time: a candidate is selected iff fewer than N candidates are louder"""
    C, F, B = amp.shape
    N = counts(n, nbins)
    sel = np.zeros(amp.shape, bool)
    ks = np.arange(first_bin, first_bin + nbins)
    for c in range(C):
        for f in range(F):
            a = amp[c, f, ks]
            cand = ~np.isnan(a)
            with np.errstate(invalid="ignore"):
                louder = (a[:, None] > a[None, :]) | ((a[:, None] == a[None, :]) & (ks[:, None] < ks[None, :]))
            louder &= cand[:, None]               # louder[j, k]: candidate j is louder than k
            sel[c, f, ks] = cand & (louder.sum(0) < N[f])
    return sel


# ---- inputs ----

def _freqs(rng, C, F, B):
    freq = rng.uniform(-SR, SR, (C, F, B)).astype(f32)
    freq[rng.random((C, F, B)) < 0.01] = np.nan
    return freq


def levels(size, C, F, seed):
    """every amp one of LEVELS, 3 % NaN; frame 0 all 1, frame 1 all NaN, frame 2 a random mix of +0 and -0: nearly every
    cut falls inside a run of ties"""
    rng = np.random.default_rng(seed)
    B = size // 2 + 1
    amp = LEVELS[rng.integers(0, len(LEVELS), (C, F, B))]
    amp[rng.random((C, F, B)) < 0.03] = np.nan
    amp[:, 0] = 1
    if F > 1:
        amp[:, 1] = np.nan
    if F > 2:
        amp[:, 2] = np.where(rng.random((C, B)) < 0.5, f32(0.0), f32(-0.0))
    return np.stack([amp, _freqs(rng, C, F, B)], axis=-1)


def near_keys(size, C, F, seed, exponents=False):
    """amps 1 + j 2^-23 for a shuffled j (only the last digit or bit of the key decides); exponents: 2^e for a shuffled e in
    -100 .. 100 (only the top one does; the values repeat every 201 bins)"""
    rng = np.random.default_rng(seed)
    B = size // 2 + 1
    j = np.stack([[rng.permutation(B) for _ in range(F)] for _ in range(C)])
    amp = np.ldexp(1.0, j % 201 - 100).astype(f32) if exponents else (1.0 + j * 2.0 ** -23).astype(f32)
    return np.stack([amp, _freqs(rng, C, F, B)], axis=-1)


PLANTED = (0.0, 1.0, None, None, np.nan, -1.0, 2.5, 3.5)     # None: nbins, nbins + 5


def n_row(F, nbins, seed):
    """n per frame: uniform in [0, nbins], with 0, 1, nbins, nbins + 5, NaN, -1, 2.5 and 3.5 in the first frames"""
    n = np.random.default_rng(seed).uniform(0, nbins, F).astype(f32)
    planted = [nbins if v is None and i == 2 else (nbins + 5 if v is None else v) for i, v in enumerate(PLANTED)]
    n[:len(planted)] = np.array(planted, f32)[:F]
    return n


def ranges(B):
    """(first_bin, nbins): everything, all but bin 0, an inner range, the last two bins"""
    return ((0, B), (1, B - 1), (3, B - 5), (B - 2, 2))
