"""The frame operations of clfa_pvoc (pitch scale, frequency shift, timed read) without a GPU: properties of the numpy
model of their definitions (tests/pvoc_ops_model.py), and the library's new symbols and argument checks — which come
before any device lookup, so they answer on a machine without a device too."""
import ctypes

import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd import _lib
from tests import pvoc_env_probe as ep
from tests import pvoc_ops_model as om

CL_INVALID_VALUE = -30
SR = 48000.0
f32 = np.float32


def _frames(rng, C, F, size):
    B = size // 2 + 1
    amp = np.abs(rng.standard_normal((C, F, B))).astype(f32) + f32(0.01)
    freq = (np.arange(B) * (SR / size) + rng.standard_normal((C, F, B)) * SR / size / 4).astype(f32)
    return np.stack([amp, freq], axis=-1)


def test_scale_one_is_the_identity():
    size = 64
    fr = _frames(np.random.default_rng(1), 2, 3, size)
    out = om.op32("scale", fr, 1.0, size, SR)
    assert np.array_equal(out.view(np.uint32), fr.view(np.uint32))


@pytest.mark.parametrize("s", [0.5, 0.75, 1.5, 2.0])
def test_a_single_peak_moves_to_its_scaled_bin(s):
    """k0 = 36 is the LAST k that reaches its bin for each of these s (below 1 two sources can share a bin, and the later
    one wins: 37 would lose bin 19 to 38 at s = 0.5)"""
    size, k0 = 256, 36
    M = size // 2
    fr = np.zeros((1, 1, M + 1, 2), f32)
    fr[0, 0, :, 1] = np.arange(M + 1, dtype=f32) * om.cf_of(size, SR)
    fr[0, 0, k0] = (0.8, 36.3 * SR / size)
    out = om.op32("scale", fr, s, size, SR)
    j0 = int(np.floor(f32(k0) * f32(s) + f32(0.5)))
    assert np.flatnonzero(out[0, 0, :, 0]).tolist() == [j0]
    assert out[0, 0, j0, 0] == f32(0.8) and out[0, 0, j0, 1] == f32(36.3 * SR / size) * f32(s)
    # every bin without a source is silent at its centre
    rest = [j for j in range(1, M) if om.scale_map_serial(M, s)[j] == om.EMPTY]
    assert np.array_equal(out[0, 0, rest, 1], np.arange(M + 1, dtype=f32)[rest] * om.cf_of(size, SR))


@pytest.mark.parametrize("M", [32, 512])
def test_serial_map_equals_the_gather(M):
    rng = np.random.default_rng(M)
    ss = np.concatenate([[0.25, 4.0, 1.0, 0.5, 2.0], rng.uniform(0.25, 4.0, 195)]).astype(f32)
    for s in ss:
        assert np.array_equal(om.scale_map_serial(M, s), om.scale_map_gather(M, s)), s
    for s in (0.2, 4.5, np.nan, np.inf):
        m = om.scale_map_serial(M, s)
        assert m[0] == m[M] == om.COPY and (m[1:M] == om.EMPTY).all()


def test_shift_there_and_back_restores_the_bins_that_stayed_in_range():
    size, lowest, d = 128, 3, 5
    M = size // 2
    fr = _frames(np.random.default_rng(2), 2, 4, size)
    hz = f32(d * SR / size)
    there = om.op32("shift", fr, hz, size, SR, lowest=lowest)
    back = om.op32("shift", there, -hz, size, SR, lowest=lowest)
    keep = np.arange(lowest, M - d)       # bins whose image j + d stayed below M
    assert np.array_equal(back[:, :, keep, 0], fr[:, :, keep, 0])
    assert np.allclose(back[:, :, keep, 1], fr[:, :, keep, 1], rtol=1e-6)
    low = np.arange(0, lowest)
    assert np.array_equal(there[:, :, low], fr[:, :, low]) and np.array_equal(there[:, :, M], fr[:, :, M])
    assert not there[:, :, lowest:lowest + d, 0].any() and not back[:, :, M - d:M, 0].any()


def test_read_at_integer_positions_copies_frames():
    fr = _frames(np.random.default_rng(3), 2, 6, 64)
    fr[0, 2, 5, 0] = np.nan
    pos = np.array([3, 0, 5, 5, 1, -2, 99, np.nan], f32)
    out = om.read32(fr, pos)
    for g, i in enumerate([3, 0, 5, 5, 1, 0, 5, 0]):
        assert np.array_equal(out[:, g].view(np.uint32), fr[:, i].view(np.uint32)), g
    assert not np.isnan(out).any()        # frame 2 was never read, neither as frame i nor with weight 0


def test_read_of_a_linear_ramp_at_half_positions_is_exact():
    Fin, B = 9, 33
    ramp = np.arange(Fin, dtype=f32)[None, :, None, None] * f32(4) + np.arange(B, dtype=f32)[None, None, :, None]
    fr = np.broadcast_to(ramp, (1, Fin, B, 2)).copy()
    pos = (np.arange(2 * Fin - 1) / 2).astype(f32)
    out = om.read32(fr, pos)
    want = pos[None, :, None, None] * f32(4) + np.arange(B, dtype=f32)[None, None, :, None]
    assert np.array_equal(out, np.broadcast_to(want, out.shape))


@pytest.mark.parametrize("op,par", [("scale", 1.31), ("scale", 0.6), ("shift", 700.0)])
def test_formant_keeps_a_cosine_series_envelope(op, par):
    """log amp = an exact cosine series of order <= coefs: env = amp, so every bin with a source comes out with the
    amplitude its own position has in the input.  The exact series is float64 data: rounded to float32 it would be a
    cosine series only to 6e-8, so the float64 model takes it as it is.  The float32 model then sees the rounded frame."""
    size, coefs = 256, 12
    M = size // 2
    rng = np.random.default_rng(4)
    k = np.arange(M + 1)
    logA = 0.3 + sum(rng.uniform(-0.5, 0.5) * np.cos(2 * np.pi * k * q / size) for q in range(1, coefs + 1))
    fr = np.zeros((1, 2, M + 1, 2), np.float64)
    fr[..., 0] = np.exp(logA)
    fr[..., 1] = (k * SR / size).astype(f32)
    env = om.env64(fr[..., 0], coefs)
    assert np.abs(env / fr[..., 0] - 1).max() < 1e-9
    amps = om.op64_amps(op, fr, par, size, SR, lowest=2, keepform=True, coefs=coefs)
    src = om.maps(op, M, [par], 2, om.bpf_of(size, SR))[0]
    has = np.flatnonzero(src >= 0)
    assert has.size > M // 3
    assert np.abs(amps[0, :, has] / fr[0, :, has, 0] - 1).max() < 1e-9
    # and the float32 model agrees with the float64 one, on the frame rounded to float32, to float32 accuracy
    fr32 = fr.astype(f32)
    a32 = om.op32(op, fr32, par, size, SR, lowest=2, keepform=True, coefs=coefs)[..., 0]
    assert om.rel_l2(a32, om.op64_amps(op, fr32, par, size, SR, lowest=2, keepform=True, coefs=coefs)) < 1e-5


def test_library_exports_the_ops_symbols():
    names = ["clfa_pvoc_scale_dev", "clfa_pvoc_scale", "clfa_pvoc_shift_dev", "clfa_pvoc_shift", "clfa_pvoc_read_dev",
             "clfa_pvoc_read", "clfa_pvoc_ops_kernel_name"]
    L = ctypes.CDLL(_lib.LIB_PATH)
    bound = [s[0] for s in _lib.SYMBOLS]
    for n in names:
        assert hasattr(L, n) and n in bound, n
    assert fa.Pvoc(0, 48, 16, SR).ops_kernel_name("scale") == ""


def test_argument_errors_come_before_the_device_lookup():
    size, C, F = 64, 2, 3
    M = size // 2
    pv = fa.Pvoc(0, size, 16, SR, C)
    good = pv.get_error()                  # 0 with a device, "Device not found" without: what a good call returns
    assert good == (0 if fa.device_count() > 0 else -1)
    L = _lib.lib()
    fr = _frames(np.random.default_rng(5), C, F, size)
    out = np.full_like(fr, 7.0)
    par = np.full(F, 1.5, f32)
    p = lambda a: a.ctypes.data

    def scale(par=par, keepform=0, coefs=10, i=fr, o=out, F=F):
        return L.clfa_pvoc_scale(pv._h, p(i), p(o), F, p(par), keepform, 1.0, coefs)

    def shift(par=par, lowest=1, keepform=0, coefs=10, o=out):
        return L.clfa_pvoc_shift(pv._h, p(fr), p(o), F, p(par), lowest, keepform, 1.0, coefs)

    def read(Fin=F, Fout=F, o=out):
        return L.clfa_pvoc_read(pv._h, p(fr), Fin, p(par), p(o), Fout)

    assert scale() == good and shift() == good and read() == good
    assert scale(F=0) == good and read(Fout=0) == good
    for bad in (0.2, 4.5, np.nan, np.inf):
        assert scale(par=np.array([1.0, bad, 1.0], f32)) == CL_INVALID_VALUE, bad
    for bad in (np.nan, -np.inf):
        assert shift(par=np.array([0.0, 10.0, bad], f32)) == CL_INVALID_VALUE, bad
    assert scale(keepform=1, coefs=0) == CL_INVALID_VALUE and scale(keepform=1, coefs=M) == CL_INVALID_VALUE
    assert scale(keepform=0, coefs=0) == good and scale(keepform=1, coefs=M - 1) == good
    assert shift(lowest=0) == CL_INVALID_VALUE and shift(lowest=M) == CL_INVALID_VALUE and shift(lowest=M - 1) == good
    assert shift(keepform=1, coefs=M) == CL_INVALID_VALUE
    assert read(Fin=0) == CL_INVALID_VALUE and read(Fin=2 ** 24 + 1) == CL_INVALID_VALUE
    assert scale(F=-1) == CL_INVALID_VALUE and read(Fout=-1) == CL_INVALID_VALUE
    # an output that overlaps the frames or the per-frame array, even partly
    flat = fr.reshape(-1)
    assert scale(o=flat[2:]) == CL_INVALID_VALUE and scale(o=fr) == CL_INVALID_VALUE
    both = np.zeros(fr.size + F, f32)
    assert scale(par=both[fr.size - 1:fr.size - 1 + F], o=both[:fr.size]) == CL_INVALID_VALUE
    assert L.clfa_pvoc_scale(pv._h, None, p(out), F, p(par), 0, 1.0, 10) == CL_INVALID_VALUE
    assert L.clfa_pvoc_scale(None, p(fr), p(out), F, p(par), 0, 1.0, 10) == CL_INVALID_VALUE
    if good != 0:
        assert (out == 7.0).all()          # nothing was computed anywhere
    # an object whose creation arguments were bad keeps answering with that error
    bad_pv = fa.Pvoc(0, 48, 16, SR)
    assert L.clfa_pvoc_scale(bad_pv._h, p(fr), p(out), F, p(par), 0, 1.0, 10) == CL_INVALID_VALUE
    # the Python forms: a plain number for the per-frame array; the status raised as ClError
    if good != 0:
        with pytest.raises(fa.ClError):
            pv.scale(fr, 1.5)
    with pytest.raises(fa.ClError) as e:
        pv.scale(fr, 5.0)
    assert e.value.code == CL_INVALID_VALUE


# ---- the probe frames of the per-bin envelope tests (tests/pvoc_env_probe.py, tests/test_gpu_pvoc_env.py) ----

def _log_env(env):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(env, np.float64))


@pytest.mark.parametrize("size", [64, 256, 1024])
def test_env64_fft_is_env64_on_the_probes(size):
    """env64 (the cosine sums of the definition) stays the definition; env64_fft is what reaches size 16384"""
    amp = ep.probe_for(size)[..., 0]
    for coefs in ep.coefs_for(size):
        d = np.abs(_log_env(om.env64_fft(amp, coefs)) - _log_env(om.env64(amp, coefs))).max()
        assert d < 1e-11, (size, coefs, d)


@pytest.mark.parametrize("size", ep.SIZES)
def test_the_probes_are_as_specified(size):
    M, T, w = size // 2, ep.lanes(size), ep.fpw(size)
    C = ep.channels_for(size)
    F = ep.frames_for(size, C)
    fr = ep.probe(size, C, F)
    assert fr.shape == (C, F, M + 1, 2) and fr.dtype == f32 and not fr.flags.writeable
    assert F >= 40 and C * F >= 3 * w and (w == 1 or (C * F) % w != 0), "three full groups and a ragged one"
    assert w == 1 or F % w != 0, "a group straddles the channel boundary"
    assert ep.frames_for(64, 2) == 193 and ep.frames_for(16384, 2) == 40
    assert np.isfinite(fr).all()
    flat = fr.reshape(C * F, M + 1, 2)[..., 0]
    # odd frames: the two constants alternately
    assert all((flat[b] == (ep.HI if (b // 2) % 2 == 0 else ep.LO)).all() for b in range(1, C * F, 2))
    # even frames: ones and one bin of 256, 1 / 256 or 0; every k0 of the list occurs, and every A
    seen, amps = [], set()
    for b in range(0, C * F, 2):
        k = np.flatnonzero(flat[b] != 1)
        assert k.size == 1
        seen.append(int(k[0]))
        amps.add(float(flat[b, k[0]]))
    want = [0, 1, 2, 3, T - 1, T, T + 1, 15, 16, 17, M // 2 - 1, M // 2, M // 2 + 1, M - 3, M - 2, M - 1, M]
    assert set(min(max(k, 0), M) for k in want) <= set(seen[:len(ep.k0_list(size))])
    assert amps == {256.0, 1 / 256, 0.0}
    cs = ep.coefs_for(size)
    assert set(cs) == set(min(max(c, 1), M - 1) for c in [1, 2, T - 1, T, T + 1, M // 2 - 1, M // 2, M // 2 + 1, M - 2, M - 1])
    assert len(cs) == len(set(cs))
    for coefs in cs:
        assert np.isfinite(om.env64_fft(flat, coefs)).all() and np.isfinite(om.env32(flat, coefs)).all(), coefs


@pytest.mark.parametrize("size", ep.SIZES)
def test_env32_of_an_all_ones_frame_is_exactly_one(size):
    """log 1 = 0, the transforms of zeros are zeros, exp 0 = 1: what lets the device tests ask for 1.0 bits"""
    ones = np.ones((2, size // 2 + 1), f32)
    for coefs in ep.coefs_for(size):
        assert np.array_equal(om.env32(ones, coefs).view(np.uint32), ones.view(np.uint32)), coefs


@pytest.mark.parametrize("size", ep.SIZES)
def test_the_probes_localise_a_misplaced_bin(size):
    """An impulse of 256 moved by one bin changes log E by more than 1 somewhere as soon as coefs >= M / 2 - 1 (measured
    on the float32 model: 1.7 .. 1.8 at M / 2 - 1, 5.2 .. 5.5 at M - 1, at every size), five orders above the per-bin
    tolerance of the device tests.  The LOW coefs do not localise: at coefs 1 a move between inner bins changes log E by 6e-7 at size 16384, so
    they pin the smooth part of the envelope only.  The high values of coefs_for are therefore the ones that find a bin
    handled as its neighbour: do not trim them to save time."""
    M = size // 2
    ks = ep.k0_list(size)
    here, moved = np.ones((len(ks), M + 1), f32), np.ones((len(ks), M + 1), f32)
    for i, k in enumerate(ks):
        here[i, k] = 256
        moved[i, k + 1 if k < M else k - 1] = 256
    for coefs in sorted(c for c in ep.coefs_for(size) if c >= M // 2 - 1):
        d = np.abs(_log_env(om.env32(here, coefs)) - _log_env(om.env32(moved, coefs))).max(axis=-1)
        assert d.min() > 1, (size, coefs, d.min())
    if size == 16384:
        inner = [i for i, k in enumerate(ks) if 1 <= k < M - 1]      # (a move across bin 0 or M changes the mean: 1e-3)
        d = np.abs(_log_env(om.env32(here[inner], 1)) - _log_env(om.env32(moved[inner], 1))).max()
        assert d < 1e-5, d
