"""The cases of the Nupconv / NupconvMatrix tests, in one place: the geometries, the push positions and fade lengths, the
cached signals, the object makers, the compositions that define the objects' bits, and the three drivers (run, run_aligned,
faded) that put an object through calls on guarded rows.  pytest does not collect this file; tests/test_nupconv_cases_cpu.py
runs the drivers on CPU tensors against a fake object, and shows that each of their assertions can fail.

A geometry of four numbers is Nupconv's, (pts0, pts1, n1, channels); one of five is NupconvMatrix's, (pts0, pts1, n1,
inputs, outputs).  The drivers know an object through a Form: the attributes that hold its row counts on either side and
the names of its two fade pushes.

Every signal recipe draws from its generator in a fixed order (the responses, then the streams): the order of the draws
and the seeds are part of each recipe."""
import collections
import functools

import numpy as np
import pytest
import torch

import opencl_fft_amd as fa
from tests import gpu_guard as gg
from tests import nupconv_definitions as definitions

SEGS_ENV = "CLFA_PCONV_MATRIX_SEGS"
Form = collections.namedtuple("Form", "rows_in rows_out fade fade_device")
NUPCONV = Form("channels", "channels", "push_ir_fade", "push_ir_fade_device")
MATRIX = Form("inputs", "outputs", "fade_ir", "fade_ir_device")

# ---- the float64 models' geometries (pts0, pts1, n1): the CPU tests
MODEL_GEOMS = [(4, 8, 1), (4, 16, 3), (8, 64, 2)]
TV_MODEL_GEOMS = [(32, 64, 1), (32, 256, 3)]

# ---- Nupconv on the device: pts0, pts1, n1
GEOMS = [(32, 64, 1), (32, 256, 3), (64, 4096, 2)]
# m = 2 at every transform size of the blocks route: with (32, 64, 1) above each size 32 .. 4096 is once the head's and once
# the tail's (k_pconvb_fwd / k_pconvb_inv, one instantiation per size; k_nupc_fwd, the forward transform with the stage copy
# folded in, for the time-varying calls)
SIZE_GEOMS = [(64, 128, 2), (128, 256, 3), (256, 512, 1), (512, 1024, 2), (1024, 2048, 3), (2048, 4096, 1)]
# tails on both sides of k_nupc_mac's prefetch depth of 16 partitions: one short of a pass, a whole pass, one and two whole
# passes and a partial one after them
DEPTH_GEOMS = [(32, 64, 15), (32, 64, 16), (32, 64, 17), (32, 64, 33), (32, 256, 17)]
ALL_GEOMS = GEOMS + SIZE_GEOMS + DEPTH_GEOMS
# the main fade test also at the head and tail sizes no other geometry has (128, 2048), and with tails past the prefetch
# depth of k_nupc_mac, whose block is the four-job launch during a fade
FADE_GEOMS = GEOMS + [(128, 256, 3), (1024, 2048, 3), (32, 64, 17), (32, 64, 33)]

# ---- NupconvMatrix on the device: pts0, pts1, n1, inputs, outputs
MATRIX_GEOMS = [(32, 64, 1, 2, 3),       # m = 2: the tail's forward and inverse in consecutive calls; 16-item slices share waves
                (32, 256, 11, 3, 2),     # both levels segmented (3 and 2 on 256 CUs), on both sides of the prefetch depth
                (64, 4096, 2, 2, 2),     # the largest pts1, a head chain of 128 partitions x 2 inputs
                (32, 256, 3, 1, 4),      # one input
                (32, 256, 3, 4, 1)]      # one output
# the transform sizes 128 and 2048, which no geometry above has, as head and as tail (the two parametrised tests of
# tests/test_gpu_nupconv_matrix.py; tests/test_gpu_nupconv_matrix_fade.py keeps MATRIX_GEOMS)
MATRIX_SIZE_GEOMS = [(128, 512, 2, 2, 2), (512, 2048, 1, 2, 3)]
SEGMENTED = (32, 256, 11, 3, 2)
BIG = (64, 4096, 2, 2, 2)          # the largest pts1 and a head chain of 256 terms: two cases only
SMALL = [g for g in MATRIX_GEOMS if g != BIG]
assert BIG in MATRIX_GEOMS and SEGMENTED in SMALL and len(SMALL) == 4

# (push position, fade length, calls): indices into positions() and fades().  Every position, with every fade length and
# every cut of the stream met several times over the two tables and the geometries
TABLES = {
    1: [(0, 1, "odd"), (1, 0, "singles"), (2, 2, "one"), (3, 1, "singles"), (4, 2, "odd"), (5, 0, "one")],
    3: [(0, 2, "singles"), (1, 1, "odd"), (2, 0, "one"), (3, 2, "odd"), (4, 0, "singles"), (5, 1, "one"), (5, 2, "singles")],
}
# the big geometry's cases, as TABLES': indices of the push position and the fade length, the calls
BIG_CASES = [(3, 1, "one"), (5, 2, "odd")]


def cvs(pts1, n1, rest=5):
    return 2 * pts1 + n1 * pts1 + rest   # a remainder, dropped


def positions(m, n1):
    """the push positions: c = 0; c = 1, in the first period; P = 1 with s = 0 and s = 1; P = 2 with s = m - 1; P = n1 + 3
    with s = 1, where the tail's ring has wrapped"""
    return [0, 1, m, m + 1, 2 * m + m - 1, (n1 + 3) * m + 1]


def fades(m):
    return [1, m + 1, 2 * m + 3]


def nblocks(m, n1):
    """the latest push, the longest fade and n1 + 4 periods after it"""
    return positions(m, n1)[-1] + fades(m)[-1] + (n1 + 4) * m


def splits(style, fade, rest):
    """the calls after the push: one; single blocks; an odd split whose second call starts inside the fade and ends after it"""
    if style == "one":
        return [rest]
    if style == "singles":
        return [1] * rest
    assert fade >= 2
    first, second = fade // 2, fade - fade // 2 + 2
    return [first, second, rest - first - second]


def cutting(I, nparts):
    """a segment count whose cuts fall inside an input's partitions (not all on multiples of nparts); with one
    partition per input there is no inside: the inputs are cut apart"""
    total = I * nparts
    if nparts == 1:
        return min(2, total)
    for segs in range(2, total + 1):
        if any((total * s // segs) % nparts for s in range(1, segs)):
            return segs
    raise AssertionError("no segment count cuts inside an input's partitions")


def model_grid(pts0, pts1, n1):
    """(period, phase, fade length) of every push the float64 fade models are held to"""
    m = pts1 // pts0
    return [(P, s, fade) for P in range(n1 + 5) for s in sorted({0, 1, m - 1}) for fade in sorted({1, m - 1, m + 1, 2 * m + 3})]


def model_calls(model, x, splits, w=None, plain=()):
    """a float64 model through calls of `splits` blocks each; with a second input w, the calls whose index is in `plain`
    go without it"""
    out, j, n = [], 0, model.pts0
    for i, k in enumerate(splits):
        a, b = j * n, (j + k) * n
        out.append(model.process(x[:, a:b]) if w is None or i in plain else model.process(x[:, a:b], w[:, a:b]))
        j += k
    assert j * n == x.shape[1] and model.position == j
    return np.concatenate(out, axis=1)


def model_faded(model, hA, hB, x, c, fade, nblocks):
    """a float64 model that holds hA, pushed hB at position c: its output over nblocks blocks, fade_remaining() checked
    block by block"""
    pts0 = model.pts0
    model.push_ir(hA)
    out = [model.process(x[:, :c * pts0])]
    assert model.position == c
    model.push_ir_fade(hB, fade)
    for j in range(c, nblocks):
        assert model.fade_remaining() == max(0, fade - (j - c))
        out.append(model.process(x[:, j * pts0:(j + 1) * pts0]))
    assert model.fade_remaining() == 0
    return np.concatenate(out, axis=1)


# The float64 fade models of both objects against the definition.  case = (hA, hB, hC, x, yA, yB, yC): three response sets,
# a signal long enough for every push of the grid (model_blocks), and what the definition gives for the objects that always
# held A, B, C; new_model(extra=2) makes a fresh model with a tail ring of n1 + extra frames.

def model_blocks(m, n1):
    """the latest push of model_grid, the longest fade, n1 + 4 periods"""
    return (n1 + 4) * m + (m - 1) + (2 * m + 3) + (n1 + 4) * m


def check_model_grid(new_model, case, geom, what=""):
    pts0, pts1, n1 = geom
    m = pts1 // pts0
    hA, hB, _, x, yA, yB, _ = case
    peak = np.max(np.abs(yA))
    for P, s, fade in model_grid(pts0, pts1, n1):
        c = P * m + s
        nblocks = c + fade + (n1 + 4) * m       # n1 + 4 periods past the fade's end: a wrong exchange shows
        assert nblocks * pts0 <= x.shape[1]
        L = nblocks * pts0
        want = definitions.mixed(yA[:, :L], yB[:, :L], c, fade, pts0)
        got = model_faded(new_model(), hA, hB, x, c, fade, nblocks)
        err = np.max(np.abs(got - want)) / peak
        assert err < 1e-12, (what, "P %d s %d fade %d" % (P, s, fade), err)
        # the fade is audible: the two ends differ after it
        after = (c + fade) * pts0
        assert np.max(np.abs(yA[:, after:L] - yB[:, after:L])) > 1e-3 * peak


def check_a_short_ring(new_model, case):
    """geometry (4, 8, 1): at phase s > 0 of period P tail block P - 3 reads input block P - 2 - n1, which a ring of n1 + 1
    frames has lost"""
    pts0, n1, m, P, s, fade = 4, 1, 2, 3, 1, 3
    hA, hB, _, x, yA, yB, _ = case
    c = P * m + s
    nblocks = c + fade + (n1 + 4) * m
    L = nblocks * pts0
    want = definitions.mixed(yA[:, :L], yB[:, :L], c, fade, pts0)
    peak = np.max(np.abs(yA))
    assert np.max(np.abs(model_faded(new_model(extra=1), hA, hB, x, c, fade, nblocks) - want)) > 1e-3 * peak
    assert np.max(np.abs(model_faded(new_model(extra=2), hA, hB, x, c, fade, nblocks) - want)) < 1e-12 * peak


def check_a_to_a(new_model, case, geom):
    pts0, pts1, n1 = geom
    m = pts1 // pts0
    hA, _, _, x, yA, _, _ = case
    peak = np.max(np.abs(yA))
    for c, fade in ((0, 1), (1, m + 1), (2 * m + m - 1, 2 * m + 3), ((n1 + 3) * m + 1, m + 1)):
        nblocks = c + fade + (n1 + 4) * m
        got = model_faded(new_model(), hA, hA, x, c, fade, nblocks)
        assert np.max(np.abs(got - yA[:, :nblocks * pts0])) < 1e-12 * peak, (c, fade)


def check_a_second_fade(new_model, case, geom):
    pts0, pts1, n1 = geom
    m = pts1 // pts0
    hA, hB, hC, x, yA, yB, yC = case
    c1, f1, f2 = 2 * m + 1, m + 1, 2 * m + 3
    c2 = c1 + f1 + m + 2                          # inside a period, a few blocks after the first fade's end
    nblocks = c2 + f2 + (n1 + 4) * m
    L = nblocks * pts0
    model = new_model()
    model.push_ir(hA)
    out = [model.process(x[:, :c1 * pts0])]
    model.push_ir_fade(hB, f1)
    with pytest.raises(AssertionError):
        model.push_ir_fade(hC, f2)                # one fade at a time
    with pytest.raises(AssertionError):
        model.push_ir(hC)
    out.append(model.process(x[:, c1 * pts0:c2 * pts0]))
    assert model.fade_remaining() == 0
    model.push_ir_fade(hC, f2)
    out.append(model.process(x[:, c2 * pts0:L]))
    got = np.concatenate(out, axis=1)
    want = definitions.mixed(definitions.mixed(yA[:, :L], yB[:, :L], c1, f1, pts0), yC[:, :L], c2, f2, pts0)
    peak = np.max(np.abs(yA))
    assert np.max(np.abs(got - want)) < 1e-12 * peak
    assert np.max(np.abs(yB[:, (c2 + f2) * pts0:L] - yC[:, (c2 + f2) * pts0:L])) > 1e-3 * peak


def mixed(a, b, c, fade, pts0):
    """the fade's definition on the host in float32: a before the fade, a + g * (b - a) inside it, b after it"""
    n0, N = c * pts0, fade * pts0
    g = np.arange(N).astype(np.float32) / np.float32(N)
    want = np.array(a)
    sa, sb = a[:, n0:n0 + N], b[:, n0:n0 + N]
    want[:, n0:n0 + N] = sa + g * (sb - sa)
    want[:, n0 + N:] = b[:, n0 + N:]
    assert want.dtype == np.float32
    return want


# kind: (added to the seed, a factor of pts0 added to it, responses, streams, head blocks of a stream)
_RECIPES = {
    # one response set and a signal of (n1 + 3) m + 3 head blocks: the tail's ring of n1 + 2 frames wraps
    "plain": (0, 0, 1, 1, lambda m, n1: (n1 + 3) * m + 3),
    # hA, hB, hC and a signal long enough for every case of the tables
    "fade": (0, 6, 3, 1, nblocks),
    # h, x and the second input w of R0 + 3m + 3 blocks: every partition of both levels is rewritten, the first head ones twice
    "tv": (1, 0, 1, 2, lambda m, n1: (n1 + 2) * m + 3 * m + 3),
}


@functools.lru_cache(maxsize=None)
def signals(kind, geom):
    """the responses of cvs samples, then the streams, float32, uniform in [-0.5, 0.5), read-only: (h, x), (hA, hB, hC, x) or
    (h, x, w)"""
    pts0, pts1, n1, rows = geom[0], geom[1], geom[2], geom[3:]
    plus, times, responses, streams, blocks = _RECIPES[kind]
    seed = pts0 + pts1 + 10 * n1 + (rows[0] if len(rows) == 1 else 100 * rows[0] + rows[1]) + plus + times * pts0
    rng = np.random.default_rng(seed)
    out = [rng.random(rows[::-1] + (cvs(pts1, n1),), dtype=np.float32) - 0.5 for _ in range(responses)]
    L = blocks(pts1 // pts0, n1) * pts0
    out += [rng.random((rows[0], L), dtype=np.float32) - 0.5 for _ in range(streams)]
    for a in out:
        a.setflags(write=False)
    return tuple(out)


def device_rows(h, need, device=gg.DEV):
    """response rows at a longer stride, one float off the 8-byte grid: (the guarded rows, their view in h's shape)"""
    lead = h.shape[:-1]
    rows = gg.rows(int(np.prod(lead)), need, need + 3, misalign=1, device=device)
    rows.fill(np.array(h[..., :need]).reshape(-1, need))   # (a copy: the cached rows are read-only)
    return rows, rows.data.unflatten(0, lead)


def make(geom, h=None, monkeypatch=None, env=None):
    """the object of a geometry, checked as created, holding h; env: CLFA_PCONV_MATRIX_SEGS at a matrix's creation"""
    pts0, pts1, n1 = geom[:3]
    if len(geom) == 4:
        p = fa.Nupconv(0, cvs(pts1, n1), pts0, pts1, channels=geom[3])
        assert p.get_error() == 0, p.get_log()
        assert p.nparts(0) == 2 * pts1 // pts0 and p.nparts(1) == n1 and p.kernel_name() == "k_nupc_mac"
        assert p.tv_period == (n1 + 2) * (pts1 // pts0)
    else:
        if env is None:
            monkeypatch.delenv(SEGS_ENV, raising=False)
        else:
            monkeypatch.setenv(SEGS_ENV, str(env))
        p = fa.NupconvMatrix(0, cvs(pts1, n1), pts0, pts1, geom[3], geom[4])
        monkeypatch.delenv(SEGS_ENV, raising=False)
        assert p.get_error() == 0, p.get_log()
        assert p.nparts(0) == 2 * pts1 // pts0 and p.nparts(1) == n1 and p.kernel_name() == "k_nupm_mac"
        assert p.segments(0) >= 1 and p.segments(1) >= 1 and p.segments(2) == 0
        if env is not None:
            assert p.segments(0) == env and p.segments(1) == env
    assert p.position == 0 and p.state_bytes() > 0
    if h is not None:
        assert p.push_ir(h) == 0
    return p


def form(geom):
    return NUPCONV if len(geom) == 4 else MATRIX


def segs(p):
    """a matrix's segment counts on both levels; None for a Nupconv"""
    return (p.segments(0), p.segments(1)) if hasattr(p, "segments") else None


# ---- the compositions that define the bits: two Clpconv objects for Nupconv, two PconvMatrix objects for NupconvMatrix

def levels(geom, h, monkeypatch=None, segments=None):
    """the two objects of the definition, holding h; a matrix's are created with the object's segment counts"""
    pts0, pts1, n1 = geom[:3]
    sizes = ((2 * pts1, pts0), (cvs(pts1, n1) - 2 * pts1, pts1))
    if len(geom) == 4:
        head, tail = (fa.Clpconv(0, c, pts, channels=geom[3]) for c, pts in sizes)
        assert head.get_cl_err() == 0 and tail.get_cl_err() == 0
        assert head.blocks_kernel_name() == "k_pconvb_mac" and tail.blocks_kernel_name() == "k_pconvb_mac"
    else:
        made = []
        for (c, pts), s in zip(sizes, segments):
            monkeypatch.setenv(SEGS_ENV, str(s))
            made.append(fa.PconvMatrix(0, c, pts, geom[3], geom[4]))
            monkeypatch.delenv(SEGS_ENV, raising=False)
            assert made[-1].get_error() == 0, made[-1].get_log()
        head, tail = made
    assert head.nparts == 2 * pts1 // pts0 and tail.nparts == n1
    assert head.push_ir(h[..., :2 * pts1]) == 0 and tail.push_ir(h[..., 2 * pts1:]) == 0
    return head, tail


def _whole_signal(obj):
    """the call of a definition's object that takes any number of blocks"""
    return obj.process_device if hasattr(obj, "outputs") else obj.process_blocks_device


def compose(head, tail, xd, pts1, push=None):
    """yh + yt delayed by 2 * pts1: both objects over the whole signal, the shifted concatenation and one torch addition.
    push = (h2, head blocks before it, tail blocks before it)"""
    rows, L = getattr(head, "outputs", xd.shape[0]), xd.shape[1]
    Lt = L // pts1 * pts1
    yh, yt = torch.empty((rows, L), device=xd.device), torch.empty((rows, Lt), device=xd.device)
    cuts = [(0, L, 0, Lt)]
    if push is not None:
        h2, cb, tb = push
        a, b = cb * head.pts, tb * pts1
        cuts = [(0, a, 0, b), (a, L, b, Lt)]
    for k, (a0, a1, b0, b1) in enumerate(cuts):
        if k:
            torch.cuda.synchronize()
            assert head.push_ir(h2[..., :2 * pts1]) == 0 and tail.push_ir(h2[..., 2 * pts1:]) == 0
        if a1 > a0:
            assert _whole_signal(head)(yh[:, a0:a1], xd[:, a0:a1]) == 0
        if b1 > b0:
            assert _whole_signal(tail)(yt[:, b0:b1], xd[:, b0:b1]) == 0
    shifted = torch.cat([torch.zeros((rows, 2 * pts1), device=xd.device), yt], dim=1)[:, :L]
    want = yh + shifted
    torch.cuda.synchronize()
    return want.cpu().numpy()


_compositions = {}


def composition(geom, monkeypatch=None, segments=None):
    """the composition's output for the cached plain signals (at these segment counts), computed once, read-only"""
    key = (geom, segments)
    if key not in _compositions:
        h, x = signals("plain", geom)
        want = compose(*levels(geom, h, monkeypatch, segments), gg.dev(x), geom[1])
        want.setflags(write=False)
        _compositions[key] = want
    return _compositions[key]


def head_only(geom, monkeypatch=None, segments=None):
    """what the head level alone returns for the cached plain signals"""
    h, x = signals("plain", geom)
    head, _ = levels(geom, h, monkeypatch, segments)
    yh = torch.empty((geom[-1], x.shape[1]), device=gg.DEV)
    assert _whole_signal(head)(yh, gg.dev(x)) == 0
    torch.cuda.synchronize()
    return yh.cpu().numpy()


_plains = {}


def plain(geom, which, monkeypatch=None, env=None):
    """(what a plain object that holds response set `which` (0, 1, 2) of the fade signals since its creation returns for
    the whole signal in one call, its segments); computed once, read-only"""
    key = (geom, which, env)
    if key not in _plains:
        sig = signals("fade", geom)
        p = make(geom, sig[which], monkeypatch, env)
        out = run(form(geom), p, sig[3], [sig[3].shape[1] // geom[0]])
        out.setflags(write=False)
        _plains[key] = (out, segs(p))
    return _plains[key]


# ---- the drivers

def _sync(t):
    if t.is_cuda:
        torch.cuda.synchronize()


def run(form, p, x, splits, w=None, plain=(), device=gg.DEV):
    """the calls of `splits` blocks each on guarded rows: out at a longer stride, 4 bytes past a 16-byte boundary; the
    input at a longer stride, unchanged afterwards; nothing written outside out, every element of it written.  With a
    second input w the calls go through process_tv_device, except those whose index is in `plain`: w at a third stride,
    8 bytes past a 16-byte boundary, unchanged afterwards"""
    L = x.shape[1]
    xin = gg.rows(getattr(p, form.rows_in), L, L + 4, device=device).fill(np.array(x))   # (a copy: the cached signals are read-only)
    win = None if w is None else gg.rows(getattr(p, form.rows_in), L, L + 7, misalign=2, device=device).fill(np.array(w))
    out = gg.rows(getattr(p, form.rows_out), L, L + 9, misalign=1, device=device)
    j, start = 0, p.position
    for i, n in enumerate(splits):
        a, b = j * p.pts0, (j + n) * p.pts0
        if win is None or i in plain:
            assert p.process_device(out.data[:, a:b], xin.data[:, a:b]) == 0
        else:
            assert p.process_tv_device(out.data[:, a:b], xin.data[:, a:b], win.data[:, a:b]) == 0
        j += n
        assert p.position == start + j, "the position after a call"
    _sync(out.buf)
    assert j * p.pts0 == L
    out.check_sides("the output rows")
    assert not out.unwritten(), "an output element was not written"
    assert xin.unchanged(), "the input changed"
    assert win is None or win.unchanged(), "the second input changed"
    return out.host()


def run_aligned(form, p, x, splits, device=gg.DEV):
    """as run on packed rows: every row of every call starts on a 16-byte boundary (the kernels' 16-byte row forms)"""
    xd = gg.dev(x, device=device)
    out = torch.full((getattr(p, form.rows_out), x.shape[1]), float("nan"), device=device)
    j = 0
    for n in splits:
        a, b = j * p.pts0, (j + n) * p.pts0
        assert out[:, a:b].data_ptr() % 16 == 0 and out.stride(0) % 4 == 0
        assert p.process_device(out[:, a:b], xd[:, a:b]) == 0
        j += n
    _sync(out)
    assert j * p.pts0 == x.shape[1]
    return out.cpu().numpy()


def faded(form, p, x, c, h2, fade, style, nblocks, host=False, run=run, device=gg.DEV):
    """p at position `start` <= c: the blocks up to c, the fade push, the blocks up to nblocks; fade_remaining() on the way"""
    pts0, start = p.pts0, p.position
    parts = []
    if c > start:
        parts.append(run(form, p, x[:, start * pts0:c * pts0], [c - start], device=device))
    need = 2 * p.pts1 + p.nparts(1) * p.pts1
    if host:
        assert getattr(p, form.fade)(h2, fade) == 0
    else:
        rows, view = device_rows(h2, need, device=device)
        assert getattr(p, form.fade_device)(view, fade) == 0
    assert p.fade_remaining() == fade and p.position == c
    j = c
    for n in splits(style, fade, nblocks - c):
        parts.append(run(form, p, x[:, j * pts0:(j + n) * pts0], [n], device=device))
        j += n
        assert p.fade_remaining() == max(0, fade - (j - c)) and p.position == j, "fade_remaining() and the position after a call"
    assert p.fade_remaining() == 0
    if not host:
        assert rows.unchanged(), "the response rows changed"
    return np.concatenate(parts, axis=1)


# ---- the fade tests whose bodies are the same for both objects

def ends(geom, p, a=0, b=1, monkeypatch=None, env=None):
    """yA, yB of the fade's definition: plain objects at the faded object's segments"""
    (ya, sa), (yb, sb) = plain(geom, a, monkeypatch, env), plain(geom, b, monkeypatch, env)
    assert sa == segs(p) and sb == segs(p), (sa, sb, segs(p))
    return ya, yb


def check_fade_bits(geom, cases, monkeypatch=None, env=None):
    """the bits of mixed(yA, yB) before, inside and after the fade; cases: (index of the push position, index of the fade
    length, calls), as TABLES'"""
    pts0, pts1, n1 = geom[:3]
    hA, hB, _, x = signals("fade", geom)
    m = pts1 // pts0
    for ip, jf, style in cases:
        c, fade = positions(m, n1)[ip], fades(m)[jf]
        nblocks = c + fade + (n1 + 4) * m
        L = nblocks * pts0
        assert L <= x.shape[1]
        p = make(geom, hA, monkeypatch, env)
        if geom == SEGMENTED and env is None:
            assert p.segments(0) > 1 and p.segments(1) > 1, segs(p)
        yA, yB = ends(geom, p, monkeypatch=monkeypatch, env=env)
        want = mixed(yA[:, :L], yB[:, :L], c, fade, pts0)
        got = faded(form(geom), p, x, c, hB, fade, style, nblocks)
        what = "%s, segments %s, push at %d, %d fade blocks, calls: %s" % (geom, segs(p), c, fade, style)
        gg.same(got[:, :c * pts0], want[:, :c * pts0], what + " (before the fade)")
        gg.same(got[:, c * pts0:(c + fade) * pts0], want[:, c * pts0:(c + fade) * pts0], what + " (the fade)")
        gg.same(got[:, (c + fade) * pts0:], want[:, (c + fade) * pts0:], what + " (after the fade)")
        # the fade is audible
        assert not np.array_equal(yA[:, (c + fade) * pts0:L], yB[:, (c + fade) * pts0:L])


def check_a_to_a_bits(geom, monkeypatch=None):
    """a fade from A to A gives the bits of no push"""
    pts0, pts1, n1 = geom[:3]
    hA, _, _, x = signals("fade", geom)
    m = pts1 // pts0
    c, fade = positions(m, n1)[5], 2 * m + 3
    nblocks = c + fade + (n1 + 4) * m
    p = make(geom, hA, monkeypatch)
    yA, _ = ends(geom, p, 0, 0, monkeypatch)
    got = faded(form(geom), p, x, c, hA, fade, "odd", nblocks)
    gg.same(got, yA[:, :nblocks * pts0], "a fade from A to A")


def check_a_plain_push_after_the_fade(geom, monkeypatch=None):
    """the exchange: the faded object pushed at phase 0 after its fade equals the object that always held B, pushed at the
    same block"""
    pts0, pts1, n1 = geom[:3]
    hA, hB, hC, x = signals("fade", geom)
    f, m = form(geom), pts1 // pts0
    c, fade = 2 * m + 1, m + 1
    c2 = 5 * m                                   # phase 0, after the fade's end
    nblocks = c2 + (n1 + 4) * m
    assert c + fade < c2 and nblocks * pts0 <= x.shape[1]
    ref = make(geom, hB, monkeypatch)
    want = [run(f, ref, x[:, :c2 * pts0], [c2])]
    assert ref.push_ir(hC) == 0
    want.append(run(f, ref, x[:, c2 * pts0:nblocks * pts0], [nblocks - c2]))
    want = np.concatenate(want, axis=1)
    assert not np.array_equal(want[:, c2 * pts0:], plain(geom, 1, monkeypatch)[0][:, c2 * pts0:nblocks * pts0])
    p = make(geom, hA, monkeypatch)
    assert segs(p) == segs(ref)
    got = [faded(f, p, x, c, hB, fade, "singles", c2)]
    assert p.position == c2 and p.position % m == 0
    assert p.push_ir(hC) == 0
    got.append(run(f, p, x[:, c2 * pts0:nblocks * pts0], [3, nblocks - c2 - 3]))
    got = np.concatenate(got, axis=1)
    gg.same(got[:, (c + fade) * pts0:], want[:, (c + fade) * pts0:], "a plain push after the fade")
