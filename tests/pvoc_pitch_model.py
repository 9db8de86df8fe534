"""The pitch of every frame of clfa_pvoc (include/clfft_amd.h, clfa_pvoc_pitch_dev) restated in numpy float32, and the
planted frames that pin the definition.  numpy only: the CPU and the GPU tests share it.

Every float32 operation is rounded on its own; fl() marks a rounding; divisions are numpy's float32 divisions, which are
correctly rounded.  Per channel and frame, with a[k] the amp and q[k] the freq of bin k, lo = first_bin, hi = first_bin +
nbins - 1, 1 <= lo <= hi <= M - 1:

  PEAK        bin k of lo..hi is a peak iff a[k] > a[k-1] and a[k] >= a[k+1] (the neighbours are read from the frame even
              when they lie outside lo..hi), a[k] >= thresh, and q[k] is finite and q[k] > 0.  A NaN makes its comparison
              false.  Of a plateau only the lowest bin is a peak.
  LIST        the first npeaks peaks in ascending bin order, L of them; (A[i], Q[i]) = (a, q) of list entry i, as bits.
              The list output holds the pairs and (+0, +0) in the entries from L on.
  CANDIDATES  for every list entry i and every m = 1..8, c = fl(Q[i] / (float)m); a candidate iff fmin <= c <= fmax.
  SCORE       s(c) starts at +0 and takes the list entries j = 0..L-1 in that order.  With w[h-1] =
              (float)pow((double)decay, h - 1): r = fl(Q[j] / c), h = rintf(r); entry j counts iff 1 <= h <= 32 and
              fl(fl(|fl(r - h)|) / h) <= tol; if it counts, s = fl(s + fl(A[j] w[h-1])).  A candidate whose score is a NaN
              is dropped.
  BEST        the candidate that no other candidate beats: d beats c iff s(d) > s(c), or s(d) == s(c) and d > c.  Two
              candidates equal in both give the same outputs.
  ROW         F0 = the bits of the best c; SAL = its score; CONF = fl(SAL / TOTAL), TOTAL the serial sum of A[0..L-1] in
              list order from +0, CONF = +0 where TOTAL == 0; NPEAKS = (float)L.  With no candidate F0, SAL, CONF = +0.

pitch() is vectorised over the frames and the candidates and serial over the at most 32 list entries.  MUTANTS are
seven wrong readings of the definition; tests/test_pvoc_pitch_cpu.py shows that the planted cases tell each from the
model."""
import numpy as np

SR = 48000.0
f32 = np.float32
DIV, HARM, PEAKS_MAX = 8, 32, 32
F0, SAL, CONF, NPEAKS = range(4)
MUTANTS = ("right_gt", "tie_low", "loudest", "w_h", "no_div_h", "reverse", "lt_tol")
DEFAULTS = dict(npeaks=16, tol=0.03, decay=0.84, first_bin=1, nbins=None)


def weights(decay, count=HARM):
    """w[h - 1] = (float)pow((double)decay, h - 1), decay a float32: Python's float power is the C library's pow"""
    d = float(f32(decay))
    return np.array([d ** h for h in range(count)], np.float64).astype(f32)


def peak_mask(x, first_bin, nbins, thresh, mutant=None):
    """(channels, F, nbins) bool: which bins of the range are peaks; thresh: a number, or an array that broadcasts
    against (channels, F, 1)"""
    a, q = x[..., 0], x[..., 1]
    k = np.arange(first_bin, first_bin + nbins)
    thresh = np.asarray(thresh, f32)
    with np.errstate(invalid="ignore"):
        right = a[..., k] > a[..., k + 1] if mutant == "right_gt" else a[..., k] >= a[..., k + 1]
        return (a[..., k] > a[..., k - 1]) & right & (a[..., k] >= thresh) & np.isfinite(q[..., k]) & (q[..., k] > 0)


def peak_list(x, first_bin, nbins, npeaks, thresh, mutant=None):
    """(A, Q, L): the list's amps and freqs, (channels, F, npeaks) float32 with +0 from L on, and L (channels, F)"""
    pk = peak_mask(x, first_bin, nbins, thresh, mutant)
    if mutant == "loudest":     # the npeaks loudest peaks (of equal amps the lower bin), in ascending bin order
        amp = np.where(pk, x[..., first_bin:first_bin + nbins, 0], -np.inf)
        rank = np.argsort(np.argsort(-amp, axis=-1, kind="stable"), axis=-1, kind="stable")
        pk = pk & (rank < npeaks)
    place = np.cumsum(pk, axis=-1) - 1
    sel = pk & (place < npeaks)
    A, Q = np.zeros(x.shape[:2] + (npeaks,), f32), np.zeros(x.shape[:2] + (npeaks,), f32)
    c, f, i = np.nonzero(sel)
    A[c, f, place[c, f, i]] = x[c, f, first_bin + i, 0]
    Q[c, f, place[c, f, i]] = x[c, f, first_bin + i, 1]
    return A, Q, np.minimum(pk.sum(axis=-1), npeaks)


def pitch(x, thresh, fmin, fmax, npeaks=16, tol=0.03, decay=0.84, first_bin=1, nbins=None, mutant=None):
    """x (channels, F, M + 1, 2) float32 -> (rows (channels, F, 4), list (channels, F, npeaks, 2)) float32"""
    x = np.asarray(x, f32)
    C, F, B = x.shape[:3]
    M = B - 1
    nbins = M - first_bin if nbins is None else nbins
    assert 1 <= first_bin and 1 <= nbins and first_bin + nbins <= M and 1 <= npeaks <= PEAKS_MAX
    fmin, fmax, tol = f32(fmin), f32(fmax), f32(tol)
    A, Q, L = peak_list(x, first_bin, nbins, npeaks, thresh, mutant)
    have = np.arange(npeaks) < L[..., None]                       # (C, F, npeaks): the entries of the list
    w = weights(decay, HARM + 1)
    with np.errstate(all="ignore"):
        c = Q[..., None] / np.arange(1, DIV + 1, dtype=f32)       # (C, F, npeaks, 8)
        cand = have[..., None] & (c >= fmin) & (c <= fmax)
        s = np.zeros(c.shape, f32)
        for j in (range(npeaks - 1, -1, -1) if mutant == "reverse" else range(npeaks)):
            r = Q[..., j, None, None] / c
            h = np.rint(r)
            d = np.abs(r - h)
            e = d if mutant == "no_div_h" else d / h
            near = e < tol if mutant == "lt_tol" else e <= tol
            counts = have[..., j, None, None] & (h >= 1) & (h <= HARM) & near
            hi = np.where(counts, h, 1).astype(np.int64)
            t = A[..., j, None, None] * w[hi if mutant == "w_h" else hi - 1]
            assert r.dtype == f32 and e.dtype == f32 and t.dtype == f32
            s = np.where(counts, s + t, s)
        cand = cand & ~np.isnan(s)
        flat_s, flat_c, flat = s.reshape(C, F, -1), c.reshape(C, F, -1), cand.reshape(C, F, -1)
        any_ = flat.any(axis=-1)
        smax = np.where(flat, flat_s, f32(-1)).max(axis=-1)
        tie = flat & (flat_s == smax[..., None])
        cbest = np.where(tie, flat_c, f32(np.inf) if mutant == "tie_low" else f32(0))
        cbest = cbest.min(axis=-1) if mutant == "tie_low" else cbest.max(axis=-1)
        total = np.zeros((C, F), f32)
        for j in range(npeaks):
            total = np.where(have[..., j], total + A[..., j], total)
        conf = smax / total
    rows = np.zeros((C, F, 4), f32)
    rows[..., F0] = np.where(any_, cbest, f32(0))
    rows[..., SAL] = np.where(any_, smax, f32(0))
    rows[..., CONF] = np.where(any_ & (total != 0), conf, f32(0))
    rows[..., NPEAKS] = L
    return rows, np.stack([A, Q], axis=-1)


# ---- the planted frames ----

def silent(size, C, F):
    """frames without a peak: every amp +0, every freq its bin centre"""
    x = np.zeros((C, F, size // 2 + 1, 2), f32)
    x[..., 1] = (np.arange(size // 2 + 1) * (SR / size)).astype(f32)
    return x


def offset(size, c, f, span=26):
    """where the pattern of frame (c, f) starts: the patterns are `span` bins long at most and move with the frame, so
    that at the large sizes they lie in many rows of the kernel's walk"""
    return ((c * 7 + f) * 37) % (size // 2 - span)


def planted(size, C, F):
    """[(name, frames, arguments of pitch())]: the cases of the issue, each on frames of (C, F).  The patterns move with
    the frame (offset()), the planted freqs do not depend on the bin."""
    M = size // 2
    inf, nan = f32(np.inf), f32(np.nan)
    cases = []

    def case(name, plant, **args):
        x = silent(size, C, F)
        for c in range(C):
            for f in range(F):
                plant(x[c, f], 1 + offset(size, c, f), c, f)
        cases.append((name, x, args))

    # a plateau: only its lowest bin is a peak; with `>` on the right there is none
    def plateau(fr, o, c, f):
        fr[o + 3:o + 6, 0] = 1.0
        fr[o + 3:o + 6, 1] = (300.0, 310.0, 320.0)
        fr[o + 10, 0], fr[o + 10, 1] = 0.5, 600.0
    case("plateau", plateau, thresh=0.1, fmin=50.0, fmax=1000.0)

    # a NaN amp as a neighbour on either side and as a centre: none of the three bins is a peak
    def nan_amps(fr, o, c, f):
        fr[o + 2, 0], fr[o + 3, 0] = nan, 1.0            # o + 3: its left neighbour is a NaN
        fr[o + 7, 0], fr[o + 8, 0] = 1.0, nan            # o + 7: its right neighbour is a NaN; o + 8: a NaN itself
        fr[o + 12, 0], fr[o + 12, 1] = 0.25, 440.0       # a peak that stays
        fr[o + 16, 0], fr[o + 16, 1] = 0.125, 880.0
    case("NaN amps", nan_amps, thresh=0.01, fmin=50.0, fmax=1000.0)

    # a NaN, negative, zero or infinite freq at a peak: no peak; the frames take turns in which comes first
    def bad_freqs(fr, o, c, f):
        bad = np.roll(np.array([nan, -220.0, 0.0, -0.0, inf, -inf], f32), c + f)
        for i, q in enumerate(bad):
            fr[o + 2 + 2 * i, 0], fr[o + 2 + 2 * i, 1] = 2.0 + i, q
        fr[o + 16, 0], fr[o + 16, 1] = 0.5, 220.0
        fr[o + 20, 0], fr[o + 20, 1] = 0.25, 441.0
    case("bad freqs", bad_freqs, thresh=0.01, fmin=50.0, fmax=1000.0)

    # a louder neighbour just outside lo..hi at either end (the range is the call's, so this pattern does not move)
    lo, hi = M // 2 - 4, M // 2 + 4

    def outside(fr, o, c, f):
        fr[lo - 1, 0], fr[lo, 0], fr[lo, 1] = 2.0, 1.0, 500.0       # not a peak: a[lo - 1] is louder
        fr[hi + 1, 0], fr[hi, 0], fr[hi, 1] = 2.0, 1.0, 900.0       # not a peak: a[hi + 1] is louder
        fr[lo + 4, 0], fr[lo + 4, 1] = 0.5, 700.0 + c + f
    case("louder outside", outside, thresh=0.01, fmin=50.0, fmax=2000.0, first_bin=lo, nbins=hi - lo + 1)

    # more peaks than npeaks, the loudest last: the list is the lowest
    def many(fr, o, c, f):
        for i in range(12):
            fr[o + 1 + 2 * i, 0], fr[o + 1 + 2 * i, 1] = 1.0 + i, 110.0 * (i + 1)
    case("more peaks than npeaks", many, thresh=0.5, fmin=50.0, fmax=2000.0, npeaks=5)
    case("as many peaks as npeaks", many, thresh=0.5, fmin=50.0, fmax=2000.0, npeaks=12)

    # no peak: the zero row
    case("no peak", lambda fr, o, c, f: None, thresh=0.0, fmin=50.0, fmax=2000.0)

    # peaks, and no candidate inside fmin..fmax
    def out_of_band(fr, o, c, f):
        fr[o + 3, 0], fr[o + 3, 1] = 1.0, 3000.0
        fr[o + 9, 0], fr[o + 9, 1] = 0.5, 4000.0
    case("no candidate", out_of_band, thresh=0.1, fmin=2.0, fmax=300.0)

    # a harmonic series whose candidates c = 200 and c / 2 = 100 reach equal scores (decay 1): the higher wins
    def series(fr, o, c, f):
        for i, q in enumerate((200.0, 400.0, 600.0)):
            fr[o + 2 + 4 * i, 0], fr[o + 2 + 4 * i, 1] = 1.0 / (i + 1 + f), q
    case("equal scores", series, thresh=0.0, fmin=90.0, fmax=250.0, decay=1.0)

    # the same series with the decay: the weights show (w[h] for w[h-1])
    case("decay", series, thresh=0.0, fmin=90.0, fmax=700.0, decay=0.84)

    # harmonic 3 off by 0.06: inside tol = 0.03 only once the deviation is divided by h; 100 is the one candidate
    def third(fr, o, c, f):
        fr[o + 2, 0], fr[o + 2, 1] = 1.0, 100.0
        fr[o + 9, 0], fr[o + 9, 1] = 0.5, 306.0
    case("deviation over h", third, thresh=0.1, fmin=90.0, fmax=101.0)

    # a deviation equal to tol: 132 / 128 = 1.03125 exactly, tol = 2^-5; 128 is the one candidate
    def at_tol(fr, o, c, f):
        fr[o + 2, 0], fr[o + 2, 1] = 1.0, 128.0
        fr[o + 5, 0], fr[o + 5, 1] = 0.5, 132.0
    case("deviation equal to tol", at_tol, thresh=0.1, fmin=100.0, fmax=130.0, tol=0.03125)

    # the order of the sum: 1 + 2^-24 + 2^-24 is 1 from the left and 1 + 2^-23 from the right
    def order(fr, o, c, f):
        for i, a in enumerate((1.0, 2.0 ** -24, 2.0 ** -24)):
            fr[o + 2 + 3 * i, 0], fr[o + 2 + 3 * i, 1] = a, 100.0 * (i + 1)
    case("order of the sum", order, thresh=0.0, fmin=90.0, fmax=110.0, decay=1.0)

    # an inf amp: SAL and TOTAL are inf and CONF is a NaN; with a weight that has underflowed to 0 the score of a
    # candidate that meets it at that harmonic is a NaN, and the candidate is dropped
    def inf_amp(fr, o, c, f):
        fr[o + 2, 0], fr[o + 2, 1] = 1.0, 150.0
        fr[o + 8, 0], fr[o + 8, 1] = inf, 450.0
    case("inf amp", inf_amp, thresh=0.1, fmin=100.0, fmax=500.0)
    case("inf amp times a zero weight", inf_amp, thresh=0.1, fmin=100.0, fmax=500.0, decay=1e-30)
    return cases


def tones(size, C, F, seed):
    """frames with a harmonic series planted straight into them, a new one per frame: 3..14 partials of a random f0 at
    random bins in ascending order, the freqs a little off their harmonics; the other bins low noise"""
    rng = np.random.default_rng(seed)
    M = size // 2
    x = silent(size, C, F)
    x[..., 0] = rng.uniform(0, 1e-3, x.shape[:3]).astype(f32)
    for c in range(C):
        for f in range(F):
            n = int(rng.integers(3, min(15, (M - 2) // 2 + 1)))
            bins = np.sort(rng.choice(np.arange(1, (M - 1) // 2 + 1), n, replace=False)) * 2
            f0 = rng.uniform(60.0, 900.0)
            x[c, f, bins, 0] = (rng.uniform(0.2, 1.0, n) / np.arange(1, n + 1)).astype(f32)
            x[c, f, bins, 1] = (f0 * np.arange(1, n + 1) * (1 + rng.uniform(-0.01, 0.01, n))).astype(f32)
    return x
