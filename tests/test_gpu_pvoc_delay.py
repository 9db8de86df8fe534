"""The per-bin delay with feedback of clfa_pvoc on the device (pvoc_delay.hip: k_pvoc_delay, k_pvoc_delay_fb) against the
numpy restatement of its definition (tests/pvoc_delay_model.py).

Everything is compared bit for bit with the float32 model: an output value is a fixed sequence of single correctly rounded
float32 operations on the stream's values, so there is no tolerance to choose.  Where the model gives a NaN the device gives
a NaN; payloads are not compared.  The frames are tests/pvoc_inputs.py's analysed() and raw(), the guard bands those of
tests/gpu_guard.py.  The tables are made from L = max_delay, so that no case depends on L being large enough."""
import numpy as np
import pytest
import torch

import opencl_fft_amd as fa
from opencl_fft_amd import _lib
from tests import pvoc_delay_model as dm
from tests.gpu_guard import CANARY, DEV, bits, dev, flat, run, same
from tests.pvoc_inputs import SR, analysed, make_pvoc, raw

pytestmark = pytest.mark.gpu
CL_INVALID_VALUE = -30
CL_INVALID_OPERATION = -59
f32 = np.float32
MAX_DELAY = (0, 1, 6, 39)
ROUTES = (False, True)          # without and with feedback
NAMES = {False: "k_pvoc_delay", True: "k_pvoc_delay_fb"}


def make(size, channels=1, max_delay=None, grid_max=None, monkeypatch=None):
    pv = make_pvoc(size, size // 4, channels, env={"CLFA_PVOC_OPS_GRID_MAX": grid_max}, monkeypatch=monkeypatch)
    assert [pv.delay_kernel_name(fb) for fb in ROUTES] == [NAMES[False], NAMES[True]]
    if max_delay is not None:
        assert pv.delay_setup(max_delay) == 0 and pv.delay_max_frames() == max_delay
    return pv


def frames_of(kind, size, C, F, seed=3):
    return analysed(size, C, F, seed) if kind == "analysed" else raw(size, C, F, seed + 1)


def tables(B, L, F, seed=0):
    """(delays int32 (B,), feedback float32 (B,)) for the device form.  Delays, as far as L allows: 0, 1 and L, the values
    below the group of 8 frames and above it, values above F (every tap in the history) and below F (taps the same launch
    wrote), the out-of-range pair -3 and L + 5 (the clamp), then a ramp 0..L over the remaining bins.  Feedback: 0, -0, 1,
    -1, 0.5, -0.7, 2^-20, a NaN and 1.5, once ascending and once descending over the first bins, so that each meets
    several delays; then uniform values in [-1, 1]"""
    rng = np.random.default_rng(100 * L + F + seed)
    want = [0, 1, L, 2, 3, 4, 5, 6, 7, 8, 9, 13, F + 2, F + 1, max(F - 1, 0), max(F - 3, 0), F // 2]
    pool = [v for v in want if v <= L] + [-3, L + 5]
    rest = B - len(pool)
    assert rest > 1
    d = np.concatenate([pool, (np.arange(rest) * L) // (rest - 1)]).astype(np.int32)
    g = rng.uniform(-1, 1, B).astype(f32)
    special = np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.7, 2.0 ** -20, np.nan, 1.5], f32)
    g[:special.size] = special
    g[special.size:2 * special.size] = special[::-1]
    g[B - special.size:] = special           # the end of the ramp: the longest delays
    return d, g


def call(pv, x, o, d, g, stream=None):
    return pv.delay_device(x, o, d, g, stream=stream)


def run_guarded(pv, x, d, g):
    """one device call into a guarded output: the result as numpy, the guard bands checked, every element written"""
    dx, dd, dg = dev(x), dev(d), None if g is None else dev(g)
    return run(lambda o: call(pv, dx, o, dd, dg), x.shape)


def run_cut(pv, x, d, g_of_piece, cut, stream=None):
    """the stream in calls of `cut` frames (the last one shorter), piece i with the feedback g_of_piece(i): the outputs put
    together"""
    F = x.shape[1]
    out = torch.zeros(x.shape, device=DEV)
    dx, dd = dev(x), dev(d)
    for i, a in enumerate(range(0, F, cut)):
        b = min(a + cut, F)
        o = torch.zeros((x.shape[0], b - a) + x.shape[2:], device=DEV)
        g = g_of_piece(i)
        assert call(pv, dx[:, a:b].contiguous(), o, dd, None if g is None else dev(g), stream=stream) == 0
        out[:, a:b] = o
    torch.cuda.synchronize()
    return out.cpu().numpy()


def same_state(pv, model, what):
    for name, got, want in zip(("xhist", "yhist"), pv.delay_state(), model.state()):
        same(got, want, "%s: %s" % (what, name))


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size", [64, 1024])
def test_one_call_is_the_models_bits(size, channels):
    B = size // 2 + 1
    pv = make(size, channels)
    time_bytes = pv.time_state_bytes()
    assert time_bytes == 2 * channels * B * 8 and pv.delay_state_bytes() == 0
    for F in (1, 5, 37, 200):
        for kind in ("analysed", "raw"):
            x = frames_of(kind, size, channels, F)
            for L in MAX_DELAY:
                d, g = tables(B, L, F)
                for fb in ROUTES:
                    what = "size %d ch %d F %d %s max_delay %d %s" % (size, channels, F, kind, L, NAMES[fb])
                    assert pv.delay_setup(L) == 0 and pv.delay_kernel_name(fb) == NAMES[fb]
                    assert pv.delay_state_bytes() == 3 * channels * L * B * 8
                    model = dm.Stream(channels, size, SR, L)
                    same(run_guarded(pv, x, d, g if fb else None), model.run(x, d, g if fb else None), what)
                    same_state(pv, model, what)
                    # a second call goes on from the first one's state; plain numbers as the tables
                    num = (3, 0.5 if fb else None)
                    o = flat(x.shape)
                    assert call(pv, dev(x), o.data, *num) == 0
                    torch.cuda.synchronize()
                    assert o.intact() and not o.unwritten()
                    same(o.data.cpu().numpy(), model.run(x, *num), what + ": second call")
                    same_state(pv, model, what + ": after the second call")
    assert pv.time_state_bytes() == time_bytes


@pytest.mark.parametrize("grid_max", [None, 1, 3])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size", [64, 1024])
def test_the_bits_do_not_depend_on_how_the_stream_is_cut(size, channels, grid_max, monkeypatch):
    """One call against cuts of 1, 2, 5 and F - 8 frames, on either route.  Then the routes alternating between the cuts:
    a piece without feedback is another function of the stream than a piece with it, so that run is compared with the
    model called the same way — whose own bits do not depend on the cuts (tests/test_pvoc_delay_cpu.py).  It shows that the
    histories a route leaves are those the other route goes on from."""
    F, B = 37, size // 2 + 1
    pv = make(size, channels, grid_max=grid_max, monkeypatch=monkeypatch)
    x = frames_of("raw" if channels == 1 else "analysed", size, channels, F)
    for L in MAX_DELAY:
        d, g = tables(B, L, F)
        what = "size %d ch %d grid %s max_delay %d" % (size, channels, grid_max, L)
        for fb in ROUTES:
            model = dm.Stream(channels, size, SR, L)
            want = model.run(x, d, g if fb else None)
            for cut in (F, 1, 2, 5, F - 8):
                assert pv.delay_setup(L) == 0
                same(run_cut(pv, x, d, lambda i: g if fb else None, cut), want, "%s %s cut %d" % (what, NAMES[fb], cut))
                same_state(pv, model, "%s %s cut %d" % (what, NAMES[fb], cut))
        for cut in (1, 2, 5, F - 8):
            for first in ROUTES:
                route = lambda i: g if (i % 2 == 0) == first else None
                model = dm.Stream(channels, size, SR, L)
                want = np.concatenate([model.run(x[:, a:a + cut], d, route(i)) for i, a in enumerate(range(0, F, cut))], axis=1)
                assert pv.delay_setup(L) == 0
                same(run_cut(pv, x, d, route, cut), want, "%s alternating from %s cut %d" % (what, NAMES[first], cut))
                same_state(pv, model, "%s alternating from %s cut %d" % (what, NAMES[first], cut))


def test_a_call_on_another_stream_goes_on_from_the_first():
    size, C, F, L = 1024, 3, 11, 6
    B = size // 2 + 1
    pv = make(size, C, max_delay=L)
    x = frames_of("analysed", size, C, 2 * F)
    d, g = tables(B, L, F)
    side = torch.cuda.Stream()
    for fb in ROUTES:
        assert pv.delay_setup(L) == 0
        model = dm.Stream(C, size, SR, L)
        want = model.run(x, d, g if fb else None)
        first = run_cut(pv, x[:, :F], d, lambda i: g if fb else None, F)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            second = run_cut(pv, x[:, F:], d, lambda i: g if fb else None, F)
        same(np.concatenate([first, second], axis=1), want, NAMES[fb])
        same_state(pv, model, NAMES[fb])


@pytest.mark.parametrize("fb", ROUTES)
def test_a_graph_replay_advances_the_state(fb):
    size, C, F, L = 1024, 2, 3, 6
    B = size // 2 + 1
    pv = make(size, C, max_delay=L)
    x = frames_of("analysed", size, C, F)
    d, g = tables(B, L, F, seed=5)
    dx, dd, dg = dev(x), dev(d), dev(g) if fb else None
    out = torch.zeros(x.shape, device=DEV)
    model = dm.Stream(C, size, SR, L)
    # the warm-up, on a side stream as torch's notes on graphs ask
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert call(pv, dx, out, dd, dg) == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    same(out.cpu().numpy(), model.run(x, d, g if fb else None), "warm-up")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert call(pv, dx, out, dd, dg) == 0
    torch.cuda.synchronize()
    same_state(pv, model, "the capture itself ran nothing")
    for i in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        same(out.cpu().numpy(), model.run(x, d, g if fb else None), "replay %d" % i)     # the model run three times in all
        same_state(pv, model, "after replay %d" % i)
    # the setup is refused while the object's stream is being captured
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        assert call(pv, dx, out, dd, dg) == 0
        assert pv.delay_setup(9) == CL_INVALID_OPERATION
    assert pv.delay_max_frames() == L


def test_the_tables_may_change_between_two_calls():
    size, C, F, L = 1024, 3, 21, 17
    B = size // 2 + 1
    pv = make(size, C, max_delay=L)
    x = frames_of("raw", size, C, 3 * F)
    model = dm.Stream(C, size, SR, L)
    d1, g1 = tables(B, L, F)
    d2, g2 = d1[::-1].copy(), np.roll(g1, 7)
    for i, (d, g) in enumerate(((d1, g1), (d2, g2), (d2, None), (d1, g2), (0, g1), (L, -1.0))):
        piece = x[:, (i % 3) * F:(i % 3 + 1) * F]
        same(run_guarded(pv, piece, np.broadcast_to(np.asarray(d, np.int32), (B,)),
                         None if g is None else np.broadcast_to(np.asarray(g, f32), (B,))), model.run(piece, d, g), "call %d" % i)
        same_state(pv, model, "call %d" % i)


def test_failed_calls_reset_and_the_other_states():
    size, C, F, L = 64, 2, 9, 5
    B = size // 2 + 1
    pv = make(size, C)
    x = frames_of("analysed", size, C, F)
    d, g = tables(B, L, F)
    time_bytes = pv.time_state_bytes()
    others = [pv.time_state(op) for op in ("smooth", "freeze")] + [pv.read_prev(), pv.read_phase(), pv.desc_state()]
    # a call before the setup: refused, nothing written
    guard = flat(x.shape)
    for fb in ROUTES:
        assert call(pv, dev(x), guard.data, dev(d), dev(g) if fb else None) == CL_INVALID_OPERATION
    torch.cuda.synchronize()
    assert guard.untouched()
    with pytest.raises(fa.ClError) as err:
        pv.delay_state()
    assert err.value.code == CL_INVALID_OPERATION
    assert pv.delay_setup(L) == 0 and pv.time_state_bytes() == time_bytes
    model = dm.Stream(C, size, SR, L)
    same_state(pv, model, "EMPTY after the setup")
    for fb in ROUTES:
        same(run_guarded(pv, x, d, g if fb else None), model.run(x, d, g if fb else None), NAMES[fb])
    states = pv.delay_state()
    same_state(pv, model, "before the failures")

    def unchanged(what):
        for a, b in zip(pv.delay_state(), states):
            assert np.array_equal(bits(a), bits(b)), what

    # an output that overlaps the input by one pair, or is it; an input of another length
    n = x.size
    buf = torch.full((2 * n + 2 * B,), CANARY, dtype=torch.int32, device=DEV)
    fbuf = buf.view(torch.float32)
    lo, hi = fbuf[:n].view(*x.shape), fbuf[n - 2:2 * n - 2].view(*x.shape)
    dd, dg = dev(d), dev(g)
    for fb in (None, dg):
        assert call(pv, lo, hi, dd, fb) == CL_INVALID_VALUE and call(pv, hi, lo, dd, fb) == CL_INVALID_VALUE
        assert call(pv, lo, lo, dd, fb) == CL_INVALID_VALUE
        assert call(pv, dev(x)[:, :4].contiguous(), hi, dd, fb) == CL_INVALID_VALUE
    # an output that overlaps a table by one element
    tail_i, tail_f = buf[n - 1:n - 1 + B], fbuf[n - 1:n - 1 + B]
    assert call(pv, dev(x), lo, tail_i, dg) == CL_INVALID_VALUE and call(pv, dev(x), lo, tail_i, None) == CL_INVALID_VALUE
    assert call(pv, dev(x), lo, dd, tail_f) == CL_INVALID_VALUE
    # tables of another shape or type
    assert call(pv, dev(x), hi, dd[:B - 1].contiguous(), dg) == CL_INVALID_VALUE
    assert call(pv, dev(x), hi, dd.float(), dg) == CL_INVALID_VALUE and call(pv, dev(x), hi, dd, dg.double()) == CL_INVALID_VALUE
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all())
    unchanged("a refused device call")
    # a blocking call with a bad table: the code, the output untouched, the histories as they were
    L_ = _lib.lib()
    host_out = np.full(x.shape, 7.0, f32)
    xs = np.ascontiguousarray(x)
    for bad_d, bad_g in ((L + 1, 0.5), (-1, 0.5), (1, 1.5), (1, np.nan), (1, -np.inf)):
        td, tg = np.clip(d, 0, L).astype(np.int32), np.clip(np.nan_to_num(g), -1, 1).astype(f32)
        td[B // 2], tg[B // 3] = bad_d, bad_g
        assert L_.clfa_pvoc_delay(pv._h, xs.ctypes.data, host_out.ctypes.data, F, td.ctypes.data, tg.ctypes.data) == CL_INVALID_VALUE
    assert (host_out == 7.0).all()
    with pytest.raises(fa.ClError) as err:
        pv.delay(x, L + 1)
    assert err.value.code == CL_INVALID_VALUE
    unchanged("a refused blocking call")
    # the blocking form is the device form
    td, tg = np.clip(d, 0, L).astype(np.int32), np.clip(np.nan_to_num(g), -1, 1).astype(f32)
    same(pv.delay(x, td, tg), model.run(x, td, tg), "host form with feedback")
    same(pv.delay(x, td), model.run(x, td), "host form without")
    same(pv.delay(x, 2, -0.7), model.run(x, 2, f32(-0.7)), "host form, numbers")
    same_state(pv, model, "after the host forms")
    # F == 0: success, nothing happens
    states = pv.delay_state()
    e = torch.zeros((C, 0, B, 2), device=DEV)
    assert call(pv, e, e.clone(), dd, dg) == 0 and call(pv, e, e.clone(), dd, None) == 0
    unchanged("F == 0")
    # reset, and a second setup: EMPTY histories; the other states were never touched
    assert pv.reset() == 0
    model.reset()
    same_state(pv, model, "reset")
    assert not np.isnan(pv.delay_state()[0]).any() and pv.delay_max_frames() == L
    same(run_guarded(pv, x, d, g), model.run(x, d, g), "after the reset")
    assert pv.delay_setup(L + 2) == 0
    model = dm.Stream(C, size, SR, L + 2)
    same_state(pv, model, "the second setup")
    assert pv.delay_state()[1].shape == (C, L + 2, B, 2) and pv.delay_state_bytes() == 3 * C * (L + 2) * B * 8
    assert pv.time_state_bytes() == time_bytes
    now = [pv.time_state(op) for op in ("smooth", "freeze")] + [pv.read_prev(), pv.read_phase(), pv.desc_state()]
    for a, b in zip(now, others):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
