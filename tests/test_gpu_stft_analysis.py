"""Every size and load route of the short-time analysis (k_stft_analyze, stft_kernels.hip), checked per frame and per bin.

The sparse probe.  Channels 0 and 2 hold integers from {+-1, +-2, +-3} at the positions o_c + m (size + 1) and zeros
elsewhere, o_0 = 0 and o_2 = size - 1; the window holds the integers 1..31 (int_window of the synthesis tests).  Deltas
size + 1 apart leave at most one non-zero sample in any frame, at d = j - f hop, of the exact float32 value w[d] x[j]: the
frame's packed spectrum is fft_exact.rfft_impulses(size, [d], w[d] x[j]), one twiddle product per bin and all bins of one
magnitude.  Every frame of the real channels is compared on its own, max_k |got - want| <= TOL max_k |want| with
TOL = util.TOL = 1e-6, the project's parity bar, against float64; a frame without a delta must be zero in every bin.  The
unmarked cases run the same probe through the oracle first (worst frame 4.8e-7, at size 16384 hop 2, over all nine sizes
and hops 2, 3, size/4, size/4 + 1, size), so the probe is proven before a device sees it.  A frame taken from a wrong
offset, a neighbour's sample or a wrong window value moves d or the amplitude; a failure names (channel, frame, d, bin).

The exact probe.  w[0] = 31 and zero elsewhere, distinct small integers per sample: every frame is a delta at complex
index 0, every pass multiplies by table entry 0 = (1, 0), 1 / N is a power of two and the difference term of r2c_pair is
exactly zero, so bin k >= 1 is 2 v / size and bin 0 is (v / size, v / size), v = 31 x[c, f hop], with no rounding at all.
The device must equal that as numbers (the conjugate leaves a -0.0).

Isolation.  Three channels, the middle one all NaN; the hop - 1 samples behind the last frame, the pad between the rows
and the floats around the signal are NaN as well: channels 0 and 2 must be finite, so no frame takes anything from a
neighbour's row or from behind the last frame.  The spectra go into a buffer prefilled with a canary, 1024 complex
values of it before and after, which must survive, and none may be left inside.

Shape.  F is the smallest frame count that gives at least seven full groups of FPW frames and a ragged eighth
(3 F // FPW >= 7, 3 F % FPW != 0) with F % FPW != 0, so groups straddle a channel boundary and the last group takes the
guarded store path; from 299 frames at size 64 down to 3 at 8192 and 16384 (FPW = 1: nine groups).  Every case runs free
and with CLFA_STFT_GRID_MAX=2 at plan creation (four or more strides per workgroup, three or more prefetches), and the
two results must be bit-identical.  Routes: the three reasons of the aligned8 predicate of clfa_stft_analyze_dev, each the
sole one (odd hop, odd row stride, a base 4 bytes into an 8-byte aligned buffer), and the 8-byte form at hop size / 4, 2
and size."""
import numpy as np
import pytest
import torch

import opencl_fft_amd as fa
from opencl_fft_amd import _lib
from oracle import oracle
from tests import fft_exact, util
from tests import gpu_guard
from tests import stft_model as sm
from tests.gpu_guard import DEV
from tests.test_gpu_stft_synth import int_window

gpu = pytest.mark.gpu
GUARD = 1024            # complex canaries around the spectra; NaN floats around the signal
TOL = util.TOL
SIZES = [64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384]
CH, REAL = 3, [0, 2]

# id: (hop of the size, odd row stride, floats the base is shifted by, aligned8)
ROUTES = {
    "a8": (lambda s: s // 4, False, 0, True),
    "a8-hop2": (lambda s: 2, False, 0, True),
    "a8-full": (lambda s: s, False, 0, True),
    "a4-hop3": (lambda s: 3, False, 0, False),
    "a4-hopq1": (lambda s: s // 4 + 1, False, 0, False),
    "a4-stride": (lambda s: s // 4, True, 0, False),
    "a4-base": (lambda s: s // 4, False, 1, False),
}
SIZE_HOPS = sorted({(s, r[0](s)) for s in SIZES for r in ROUTES.values()})


def frames_for(size):
    """the smallest F with seven full groups and a ragged one over the 3 F frames, and a channel boundary inside a group"""
    fpw = sm.fpw(size)
    F = 1
    while not (3 * F // fpw >= 7 and (fpw == 1 or ((3 * F) % fpw and F % fpw))):
        F += 1
    return F


def assert_shape(size, F):
    """the facts the cases rest on, from the mirror of LdsGeom::FPW"""
    fpw = sm.fpw(size)
    assert -(-(CH * F) // fpw) >= 7, "two workgroups: the second makes three strides at least and prefetches twice"
    if fpw > 1:
        assert (CH * F) % fpw, "no ragged last group"
        assert F % fpw, "no group straddles a channel boundary"


def test_frame_counts():
    assert [frames_for(s) for s in SIZES] == [299, 150, 75, 38, 19, 10, 5, 3, 3]
    for s in SIZES:
        assert_shape(s, frames_for(s))


def nan_tail(x, size, hop, F):
    """channel 1 and the hop - 1 samples no frame covers: NaN"""
    x[1] = np.nan
    x[:, size + (F - 1) * hop:] = np.nan
    return x


# ---- the sparse probe ------------------------------------------------------------------------------------------------
_PROBES = {}


def probe(size, hop):
    """(x (3, samples), w, d (2, F) or -1, want (2, F, M) complex128) of the sparse probe: made once, never written to"""
    if (size, hop) not in _PROBES:
        F = frames_for(size)
        covered = size + (F - 1) * hop
        samples = covered + hop - 1
        rng = np.random.default_rng(size * 31 + hop)
        x = np.zeros((CH, samples), np.float32)
        for c, o in ((0, 0), (2, size - 1)):
            pos = np.arange(o, covered, size + 1)
            x[c, pos] = rng.choice(np.array([-3, -2, -1, 1, 2, 3], np.float32), pos.size)
        nan_tail(x, size, hop, F)
        w = int_window(size)
        fr = sm.frame_view(x[REAL], size, hop)
        assert fr.shape == (2, F, size) and np.all(np.isfinite(fr)), "a frame covers a NaN"
        nz = fr != 0
        assert nz.sum(-1).max() <= 1, "more than one non-zero sample in a frame"
        d = np.where(nz.any(-1), nz.argmax(-1), -1)
        has = d >= 0
        amp = np.zeros(d.shape, np.float32)
        amp[has] = (w[d[has]] * fr[has, d[has]]).astype(np.float32)      # exact: |w x| <= 93
        assert d[0, 0] == 0 and d[1, 0] == size - 1, "d = 0 and d = size - 1 occur in frame 0"
        assert np.any(d[has] & 1) and not np.all(d[has] & 1), "both parities of d occur"
        want = np.zeros((2, F, size // 2), np.complex128)
        want[has] = fft_exact.rfft_impulses(size, d[has]) * amp[has].astype(np.float64)[:, None]
        for a in (x, w, d, want):
            a.setflags(write=False)
        _PROBES[(size, hop)] = (x, w, d, want)
    return _PROBES[(size, hop)]


def frame_errors(got, d, want, chans=REAL):
    """per-frame check of (2, F, M) spectra: (the worst max_k |got - want| / max_k |want| over the frames with a delta, the
    first failing frame as text or None)"""
    g = got.astype(np.complex128)
    with np.errstate(invalid="ignore"):
        err = np.abs(g - want)
    err[~np.isfinite(err)] = np.inf
    e, ref = err.max(-1), np.abs(want).max(-1)
    has = d >= 0
    bad = np.where(has, ~(e <= TOL * ref), ~np.all(g == 0, axis=-1))
    worst = float((e[has] / ref[has]).max()) if has.any() else 0.0
    msg = None
    if bad.any():
        i, f = (int(v[0]) for v in np.nonzero(bad))
        k = int(err[i, f].argmax())
        msg = ("%d frames outside %.1g; first: channel %d frame %d d %d: worst bin %d expected %r received %r, frame error "
               "%.3g" % (bad.sum(), TOL, chans[i], f, d[i, f], k, want[i, f, k], got[i, f, k],
                         e[i, f] / ref[i, f] if ref[i, f] else e[i, f]))
    return worst, msg


@pytest.mark.parametrize("size,hop", SIZE_HOPS)
def test_oracle_passes_the_sparse_probe(size, hop):
    x, w, d, want = probe(size, hop)
    F = frames_for(size)
    got = oracle.rfft_forward(sm.windowed_frames_f32(x[REAL], size, hop, w).reshape(-1, size)).reshape(2, F, size // 2)
    worst, msg = frame_errors(got, d, want)
    print("STFTANA-ORACLE %d %d: worst frame %.3g" % (size, hop, worst))
    assert msg is None, msg


# ---- the device, behind guard bands ----------------------------------------------------------------------------------
def signal_rows(x, odd_stride, shift):
    """x in rows of a device buffer whose pads and surroundings are NaN; the view handed to analyze_device"""
    C_, samples = x.shape
    stride = samples + 5
    stride += (stride & 1) != int(odd_stride)
    host = np.full(GUARD + shift + C_ * stride + GUARD, np.nan, np.float32)
    host[GUARD + shift:GUARD + shift + C_ * stride].reshape(C_, stride)[:, :samples] = x
    buf = torch.from_numpy(host).to(DEV)
    assert buf.data_ptr() % 8 == 0
    rows = buf[GUARD + shift:GUARD + shift + C_ * stride].view(C_, stride)[:, :samples]
    assert rows.stride(0) == stride and rows.data_ptr() % 8 == 4 * shift
    return rows


def analyze_guarded(size, hop, x, w, route, grid_max=None, monkeypatch=None):
    """device analysis of x laid out for `route`, into spectra between guard bands; (C, F, M) after checking every canary"""
    _, odd_stride, shift, a8 = ROUTES[route]
    if grid_max is not None:
        monkeypatch.setenv("CLFA_STFT_GRID_MAX", str(grid_max))
    st = fa.Stft(0, size, hop, window=w, fwd=True)
    if grid_max is not None:
        monkeypatch.delenv("CLFA_STFT_GRID_MAX")
    assert st.get_error() == 0, st.get_log()
    rows = signal_rows(x, odd_stride, shift)
    # the predicate of clfa_stft_analyze_dev: the route takes the load form it is named after
    assert (rows.data_ptr() % 8 == 0 and hop % 2 == 0 and rows.stride(0) % 2 == 0) == a8
    C_, F, M = x.shape[0], st.frames(x.shape[1]), size // 2
    g = gpu_guard.flat((C_, F, M), torch.complex64, misalign=0, before=2 * GUARD, after=2 * GUARD)
    assert st.analyze_device(rows, g.data) == 0
    torch.cuda.synchronize()
    g.check_sides("the spectra")
    assert not g.unwritten(), "%d floats of the spectra were not written" % g.unwritten()
    return g.data.cpu().numpy()


def assert_isolated(spec):
    assert np.all(np.isnan(spec[1].real) & np.isnan(spec[1].imag)), "the NaN channel's spectra are not all NaN"
    assert np.all(np.isfinite(spec[REAL].view(np.float32))), "a real channel took something from a NaN"


def free_and_capped(size, hop, x, w, route, monkeypatch):
    assert_shape(size, frames_for(size))
    free = analyze_guarded(size, hop, x, w, route)
    assert free.shape == (CH, frames_for(size), size // 2)
    capped = analyze_guarded(size, hop, x, w, route, grid_max=2, monkeypatch=monkeypatch)
    return free, capped


def assert_same_bits(a, b, what):
    assert np.array_equal(a[REAL].view(np.uint32), b[REAL].view(np.uint32)), what


@gpu
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("size", SIZES)
def test_sparse_probe_per_frame(size, route, monkeypatch):
    hop = ROUTES[route][0](size)
    x, w, d, want = probe(size, hop)
    free, capped = free_and_capped(size, hop, x, w, route, monkeypatch)
    checks = [frame_errors(got[REAL], d, want) for got in (free, capped)]
    print("STFTANA %d %d %s: worst frame %.3g" % (size, hop, route, max(worst for worst, _ in checks)))
    for got, (_, msg) in zip((free, capped), checks):
        assert_isolated(got)
        assert msg is None, msg
    assert_same_bits(free, capped, "the capped grid changes bits")


# ---- the load form changes no bit ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("size", SIZES)
def test_load_form_changes_no_bit(size):
    hop, F = size // 4, frames_for(size)
    rng = np.random.default_rng(size + 5)
    x = nan_tail(rng.random((CH, size + (F - 1) * hop + hop - 1), dtype=np.float32) * 2 - 1, size, hop, F)
    w = (rng.random(size, dtype=np.float32) + 0.25).astype(np.float32)
    a8 = analyze_guarded(size, hop, x, w, "a8")
    assert_isolated(a8)
    for route in ("a4-stride", "a4-base"):
        assert_same_bits(analyze_guarded(size, hop, x, w, route), a8, "%s differs from a8" % route)


# ---- the exact probe -------------------------------------------------------------------------------------------------
def exact_probe(size, hop):
    """(x, w, want (2, F, M) complex64): w[0] = 31 alone, small distinct integers per sample"""
    F = frames_for(size)
    samples = size + (F - 1) * hop + hop - 1
    j = np.arange(samples, dtype=np.int64)
    x = np.stack([(((j * 40503 + 977 * c) >> 4) % 61 - 30) for c in range(CH)]).astype(np.float32)
    assert np.all(x[REAL][:, 1:] != x[REAL][:, :-1]), "neighbouring samples differ"
    nan_tail(x, size, hop, F)
    w = np.zeros(size, np.float32)
    w[0] = 31
    v = 31.0 * x[REAL][:, np.arange(F) * hop].astype(np.float64)
    want = np.empty((2, F, size // 2), np.complex128)
    want[:] = (2 * v / size)[:, :, None]
    want[:, :, 0] = v / size * (1 + 1j)
    assert np.array_equal(want.astype(np.complex64).astype(np.complex128), want)
    return x, w, want.astype(np.complex64)


def assert_exact(got, want, hop, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d bins differ; first: channel %d frame %d (sample %d) bin %d expected %r received %r" % (
        what, len(bad), REAL[bad[0][0]], bad[0][1], bad[0][1] * hop, bad[0][2], want[tuple(bad[0])], got[tuple(bad[0])])
    assert np.array_equal(got, want)


EXACT = [(s, r) for s in SIZES for r in ("a4-hop3", "a8")]


@pytest.mark.parametrize("size,route", EXACT)
def test_oracle_passes_the_exact_probe(size, route):
    hop = ROUTES[route][0](size)
    x, w, want = exact_probe(size, hop)
    got = oracle.rfft_forward(sm.windowed_frames_f32(x[REAL], size, hop, w).reshape(-1, size)).reshape(want.shape)
    assert_exact(got, want, hop, "oracle")


@gpu
@pytest.mark.parametrize("size,route", EXACT)
def test_exact_probe_every_bin_of_every_frame(size, route, monkeypatch):
    hop = ROUTES[route][0](size)
    x, w, want = exact_probe(size, hop)
    for name, got in zip(("free", "capped"), free_and_capped(size, hop, x, w, route, monkeypatch)):
        assert_isolated(got)
        assert_exact(got[REAL], want, hop, name)


# ---- the host form with padded rows ----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("size,hop", [(256, 64), (2048, 3)])
def test_host_form_packs_padded_rows(size, hop):
    """signal_stride > samples: the rows are packed on the way in, and the NaN pads never reach the device's frames"""
    F = frames_for(size)
    samples = size + (F - 1) * hop + hop - 1
    rng = np.random.default_rng(size * 3 + hop)
    x = (rng.random((CH, samples), dtype=np.float32) * 2 - 1)
    w = (rng.random(size, dtype=np.float32) + 0.25).astype(np.float32)
    st = fa.Stft(0, size, hop, window=w)
    assert st.get_error() == 0, st.get_log()
    packed = st.analyze(x)
    padded = np.full((CH, samples + 5), np.nan, np.float32)
    padded[:, :samples] = x
    out = np.full((CH, F, size // 2), np.nan + 1j * np.nan, np.complex64)
    assert _lib.lib().clfa_stft_analyze(st._h, padded.ctypes.data, samples + 5, samples, CH, out.ctypes.data) == 0
    assert packed.shape == out.shape and np.all(np.isfinite(out.view(np.float32)))
    assert np.array_equal(out.view(np.uint32), packed.view(np.uint32))
