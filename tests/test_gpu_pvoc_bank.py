"""The filter bank of clfa_pvoc on the device (bank_kernels.hip: k_pvoc_bands) against the numpy restatement of its definition
(tests/pvoc_bank_model.py), at sizes 64, 512, 2048, 4096 and 16384 (runs of 8, 8, 4, 2 and 1 frames: every instance of the kernel), 2 channels x 9 frames (a ragged run, and
runs on both sides of the channel boundary), on the 40-band mel bank, 256 random overlapping bands, one band, and seventeen
hand-made ones.  Every call goes through tests/gpu_guard.run into a guarded output, once on a free object and once on one
whose launches have at most 2 workgroups: bit-identical.

Band energies, plain and POWER: bit for bit the float32 model (a NaN where it has one).  DCT: bit for bit the model's DCT
of THE DEVICE'S OWN v (the same call without the DCT flag) with the table of bank_dct().  tests/test_pvoc_bank_cpu.py
shows that these inputs notice six mutants of the model.

LOG is the device's logf, judged as tests/test_gpu_pvoc_env.py judges its logs: |L_dev - log64(max(E, floor))| at every
band, E the model's exact bits, against MARGIN x max(e32, ulp32(Lmax)) — e32 the numpy float32 model's own worst error
against the same truth (never the device's), ulp32(Lmax) one float32 ulp at the case's largest |L|.  Where the truth is
infinite (an infinite amp) the device gives that infinity.
MARGIN.  The rule: the smallest of 2, 4, 8 that clears the largest ratio measured over every case of this file by a factor
1.5.  Every case prints its ratio (`PVOCBANK ...` lines, pytest -s); profiles/pvoc_bank.txt holds a device run's.
MEASURED on an MI355X (32 cases: every bank at sizes 64, 512 and 16384, the mel and the hand-made bank at 2048 and 4096,
plain and odd frames): the ratios lie between 1.00 and 1.81.  The largest, 1.81, is size 64, one band, plain frames:
1.72e-6 against an ulp of 9.54e-7 (the float32 model 4.7e-7).  In 25 of the 32 cases the worst band is one at the floor and
the ratio 1.67: logf(1e-10) = -23.0258... comes out 3.19e-6 off, where one float32 ulp is 1.91e-6 and numpy's float32 log
is within 1.0e-6; the other cases have 1.00 .. 1.28 (sizes 2048 and 4096, mel, plain: 1.18 and 1.28).
1.81 x 1.5 = 2.7 rules out 2, so MARGIN is 4.  No case came near 8 / 1.5.
"""
import numpy as np
import pytest
import torch

import opencl_fft_amd as fa
from tests import pvoc_bank_model as bm
from tests.gpu_guard import CANARY, DEV, bits, dev, flat, run, same
from tests.pvoc_inputs import SR, make_pvoc

pytestmark = pytest.mark.gpu
INVALID, INVALID_OPERATION = -30, -59
MARGIN = 4.0            # see the docstring: the largest ratio measured is 1.81
FLOOR = 1e-10
SIZES = (64, 512, 2048, 4096, 16384)      # runs of 8, 8, 4, 2 and 1 frames: every k_pvoc_bands<R>
BANKS = ("mel", "random256", "one", "hand17")
# every bank at the sizes of the runs of 8 and of 1; the mel and the hand-made bank at the sizes of the runs of 4 and 2
CASES = [(size, name) for size in (64, 512, 16384) for name in BANKS] + [(size, name) for size in (2048, 4096) for name in ("mel", "hand17")]
f32 = np.float32
RATIO = {"max": 0.0, "case": ""}
_REF = {}


def make(size, grid_max=None, monkeypatch=None, channels=2):
    pv = make_pvoc(size, size // 4, channels, env={"CLFA_PVOC_OPS_GRID_MAX": grid_max}, monkeypatch=monkeypatch)
    assert pv.bands_kernel_name() == "k_pvoc_bands"
    return pv


def both(size, bank, monkeypatch):
    """(a free object, one whose launches have at most 2 workgroups), the bank set up in both"""
    pvs = make(size), make(size, grid_max=2, monkeypatch=monkeypatch)
    for pv in pvs:
        assert pv.bank_bands() == -1 and pv.bank_setup(*bank.args()) == 0 and pv.bank_bands() == bank.B
    return pvs


def run_both(pvs, dx, N, what, **kw):
    """the call on the free and on the capped object: one result, bit-identical"""
    free, capped = (run(lambda o: pv.bands_device(dx, o, **kw), tuple(dx.shape[:2]) + (N,)) for pv in pvs)
    assert np.array_equal(bits(free), bits(capped)), what + ": the grid cap changed the result"
    return free


def ref(size, name, odd, power):
    """the model's band energies of a case (computed once, read-only)"""
    key = (size, name, odd, power)
    if key not in _REF:
        e = bm.bands32(bm.frames(size)[odd][..., 0], bm.banks(size)[name], power)
        e.setflags(write=False)
        _REF[key] = e
    return _REF[key]


@pytest.mark.parametrize("size, name", CASES)
def test_bands_log_and_dct(size, name, monkeypatch):
    bank = bm.banks(size)[name]
    B = bank.B
    pvs = both(size, bank, monkeypatch)
    D = pvs[0].bank_dct()
    assert np.array_equal(bits(D), bits(pvs[1].bank_dct()))
    lfloor = np.log(f32(FLOOR))
    for odd in (0, 1):
        x = bm.frames(size)[odd]
        dx = dev(x)
        what = "size %d %s %s" % (size, name, "odd" if odd else "plain")
        # bands, plain and POWER: the model's bits
        E = {}
        for power in (False, True):
            E[power] = run_both(pvs, dx, B, what, power=power)
            same(E[power], ref(size, name, odd, power), "%s power %d" % (what, power))
        # LOG against float64
        Em = ref(size, name, odd, True)
        L = run_both(pvs, dx, B, what, power=True, log=True, floor=FLOOR)
        truth = bm.log64(Em, FLOOR)
        m32 = bm.log32(Em, FLOOR)
        fin = np.isfinite(truth)
        assert np.array_equal(L[~fin], truth[~fin].astype(f32)), what + ": an infinite energy"
        ulp = float(np.spacing(f32(np.abs(truth[fin]).max())))
        e_dev, e_f32 = float(np.abs(L[fin] - truth[fin]).max()), float(np.abs(m32[fin].astype(np.float64) - truth[fin]).max())
        bound = max(e_f32, ulp)
        ratio = e_dev / bound
        if ratio > RATIO["max"]:
            RATIO["max"], RATIO["case"] = ratio, what
        print("PVOCBANK %s: worst |dL| %.3g (float32 model %.3g, ulp %.3g, ratio %.2f; largest so far %.2f, %s)"
              % (what, e_dev, e_f32, ulp, ratio, RATIO["max"], RATIO["case"]))
        assert e_dev <= MARGIN * bound, "%s: %.3g against %.3g" % (what, e_dev, bound)
        # a NaN band and a band below the floor give logf(floor)
        low = np.isnan(Em) | (Em < f32(FLOOR))
        if odd or (name == "mel" and size == 64) or name in ("random256", "hand17"):
            assert low.any(), what + ": no band at the floor"
        assert (np.abs(L[low].astype(np.float64) - float(lfloor)) <= MARGIN * bound).all(), what + ": the floor"
        if odd:
            assert np.isnan(Em).any(), what + ": no NaN band"
        # DCT of the device's own v, with and without LOG
        for log, v in ((False, E[True]), (True, L)):
            for ncoef in sorted({1, B, min(13, B)}):
                C = run_both(pvs, dx, ncoef, what, power=True, log=log, ncoef=ncoef, floor=FLOOR)
                same(C, bm.dct32(v, D, ncoef), "%s dct log %d ncoef %d" % (what, log, ncoef))


@pytest.mark.parametrize("B", [1, 17, 40, 256])
def test_the_table(B):
    pv = make(64)
    rng = np.random.default_rng(B)
    assert pv.bank_setup(rng.integers(0, 33, B), np.ones(B, np.int32), np.ones(B, f32)) == 0
    D = pv.bank_dct()
    want = bm.dct_table(B)
    assert D.shape == (B, B) and (np.abs(D - want) <= np.spacing(np.abs(want).astype(f32))).all()
    assert np.abs(D.astype(np.float64) @ D.astype(np.float64).T - np.eye(B)).max() <= B * 2.0 ** -23


@pytest.mark.parametrize("size", SIZES)
def test_cutting_the_stream_and_a_side_stream(size, monkeypatch):
    """9 frames as 1 + 3 + 5: with runs of 8, 4, 2 and 1 frames the calls' runs fall differently from the whole stream's"""
    bank = bm.mel(size)
    pvs = both(size, bank, monkeypatch)
    x = bm.frames(size)[1]
    dx = dev(x)
    kw = dict(power=True, log=True, ncoef=13, floor=FLOOR)
    whole = run_both(pvs, dx, 13, "size %d whole" % size, **kw)
    v = run_both(pvs, dx, 40, "size %d v" % size, power=True, log=True, floor=FLOOR)
    same(whole, bm.dct32(v, pvs[0].bank_dct(), 13), "size %d: the whole stream" % size)
    parts = [run_both(pvs, dx[:, a:b].contiguous(), 13, "size %d frames %d..%d" % (size, a, b), **kw) for a, b in ((0, 1), (1, 4), (4, 9))]
    assert np.array_equal(bits(np.concatenate(parts, axis=1)), bits(whole)), "1 + 3 + 5 frames"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = run_both(pvs, dx, 13, "size %d side stream" % size, **kw)
    assert np.array_equal(bits(again), bits(whole)), "another stream"
    # the blocking form is the device form
    for pv in pvs:
        assert np.array_equal(bits(pv.bands(x, **kw)), bits(whole))
    one = make(size, channels=1)
    assert one.bank_setup(*bank.args()) == 0
    assert np.array_equal(bits(one.bands(x[1], **kw)), bits(whole[1])), "one channel, no axis"


@pytest.mark.parametrize("grid_max", [None, 2])
@pytest.mark.parametrize("size", [512, 2048])
def test_a_graph_replay_gives_the_same_bits(size, grid_max, monkeypatch):
    """A captured call has one output address for the capture and every replay, so gpu_guard.run (a fresh buffer per
    call) does not fit: the output is one guarded buffer, refilled with the canary before each replay and checked after."""
    bank = bm.mel(size)
    pv = make(size, grid_max=grid_max, monkeypatch=monkeypatch)
    assert pv.bank_setup(*bank.args()) == 0
    dx = dev(bm.frames(size)[0])
    g_out = flat((2, 9, 13))
    out = g_out.data
    kw = dict(power=True, log=True, ncoef=13, floor=FLOOR)
    # the warm-up, on a side stream as torch's notes on graphs ask
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert pv.bands_device(dx, out, **kw) == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    want = out.cpu().numpy()
    v = run(lambda o: pv.bands_device(dx, o, power=True, log=True, floor=FLOOR), (2, 9, 40))
    same(want, bm.dct32(v, pv.bank_dct(), 13), "the warm-up")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert pv.bands_device(dx, out, **kw) == 0
        assert pv.bank_setup(*bank.args()) == INVALID_OPERATION, "a setup while the object's stream is captured"
    torch.cuda.synchronize()
    for i in range(2):
        g_out.buf.fill_(CANARY)
        g.replay()
        torch.cuda.synchronize()
        assert g_out.intact() and not g_out.unwritten(), "replay %d: the guard bands" % i
        assert np.array_equal(bits(out.cpu().numpy()), bits(want)), "replay %d" % i


@pytest.mark.parametrize("grid_max", [None, 2])
def test_refused_calls_and_a_repeated_setup(grid_max, monkeypatch):
    size, C, F = 64, 2, 9
    M = size // 2
    pv = make(size, grid_max=grid_max, monkeypatch=monkeypatch)
    x = bm.frames(size)[0]
    g_in = flat(x.shape).fill(np.array(x))
    g = flat((C, F, 40))
    call = lambda **kw: pv.bands_device(g_in.data, g.data, **kw)
    # before the setup: an invalid operation, and a bad argument an invalid value ahead of it
    assert pv.bank_bands() == -1 and pv.bank_state_bytes() == 0
    assert call() == INVALID_OPERATION and call(log=True, floor=0.0) == INVALID
    with pytest.raises(fa.ClError):
        pv.bank_dct()
    with pytest.raises(fa.ClError):
        pv.bands(x)
    mel = bm.mel(size)
    assert pv.bank_setup(*mel.args()) == 0 and pv.bank_bands() == 40
    bytes40 = pv.bank_state_bytes()
    assert bytes40 >= 40 * 40 * 4 + mel.weights.size * 4 + 40 * 16
    before = run(lambda o: pv.bands_device(g_in.data, o, power=True), (C, F, 40))
    lib = fa.lib()
    raw = lambda flags, ncoef, floor=FLOOR, out=g.data: lib.clfa_pvoc_bands_dev(
        pv._h, g_in.data.data_ptr(), out.data_ptr(), F, flags, ncoef, floor, torch.cuda.current_stream().cuda_stream)
    assert raw(8, 0) == INVALID and raw(-1, 0) == INVALID, "a bad flag"
    assert raw(0, 5) == INVALID and raw(4, 0) == INVALID and raw(4, 41) == INVALID, "ncoef and the DCT flag"
    assert raw(2, 0, 0.0) == INVALID and raw(2, 0, -1.0) == INVALID and raw(2, 0, float("nan")) == INVALID, "the floor"
    assert call(ncoef=-3) == INVALID
    # an out that overlaps the frames by one float, from either side
    n, m = x.size, C * F * 40
    buf = torch.full((n + m,), CANARY, dtype=torch.int32, device=DEV).view(torch.float32)
    assert pv.bands_device(buf[:n].view(*x.shape), buf[n - 1:n - 1 + m].view(C, F, 40)) == INVALID
    assert pv.bands_device(buf[m:].view(*x.shape), buf[1:m + 1].view(C, F, 40)) == INVALID
    # refused setups leave the bank as it was
    assert pv.bank_setup([M], [2], [1.0, 1.0]) == INVALID, "a band past M"
    assert pv.bank_setup([0], [2], [1.0, np.inf]) == INVALID and pv.bank_setup([0], [1], [np.nan]) == INVALID
    assert pv.bank_setup([], [], []) == INVALID and pv.bank_setup([0] * 257, [1] * 257, [1.0] * 257) == INVALID
    torch.cuda.synchronize()
    assert g.untouched() and g_in.unchanged() and bool((buf.view(torch.int32) == CANARY).all())
    assert pv.bank_bands() == 40 and pv.bank_state_bytes() == bytes40
    after = run(lambda o: pv.bands_device(g_in.data, o, power=True), (C, F, 40))
    assert np.array_equal(bits(after), bits(before))
    # reset leaves the bank alone
    assert pv.reset() == 0 and pv.bank_bands() == 40
    assert np.array_equal(bits(run(lambda o: pv.bands_device(g_in.data, o, power=True), (C, F, 40))), bits(before))
    # F == 0: success, nothing happens
    e = torch.zeros((C, 0, M + 1, 2), device=DEV)
    assert pv.bands_device(e, torch.zeros((C, 0, 40), device=DEV)) == 0
    assert pv.bands(np.zeros((C, 0, M + 1, 2), f32)).shape == (C, 0, 40)
    # a second setup with another B takes effect
    hand = bm.banks(size)["hand17"]
    assert pv.bank_setup(*hand.args()) == 0 and pv.bank_bands() == 17 and pv.bank_dct().shape == (17, 17)
    assert pv.bank_state_bytes() != bytes40
    assert pv.bands_device(g_in.data, g.data) == INVALID, "the rows hold 17 values now"
    same(run(lambda o: pv.bands_device(g_in.data, o), (C, F, 17)), bm.bands32(x[..., 0], hand), "after the second setup")
    big = bm.banks(size)["random256"]
    assert pv.bank_setup(*big.args()) == 0 and pv.bank_bands() == 256 and pv.bank_state_bytes() > bytes40
    same(run(lambda o: pv.bands_device(g_in.data, o), (C, F, 256)), bm.bands32(x[..., 0], big), "after the third setup")
    # an object without a device
    none = fa.Pvoc(99, size, size // 4, SR, C)
    assert none.get_error() != 0 and none.bands_kernel_name() == ""
    assert none.bank_setup([M], [2], [1.0, 1.0]) == INVALID and none.bank_setup(*mel.args()) == none.get_error()
    assert none.bands_device(g_in.data, g.data, log=True, floor=0.0) == INVALID
    assert none.bands_device(g_in.data, g.data) == INVALID_OPERATION
    torch.cuda.synchronize()
    assert g.untouched()
