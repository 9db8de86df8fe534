"""The drivers of tests/nupconv_cases.py (run, run_aligned, faded), run on CPU tensors: mutation tests of what the device
tests of Nupconv and NupconvMatrix rest on.  A fake object backed by the float64 schedule model, rounded to float32, passes
all three; one float written past a row of out, one element left unwritten, a changed input, a position or a
fade_remaining() that a call did not move, and changed response rows must each fail the assertion that is there for it.
pts0 = 4, pts1 = 8, n1 = 1, two rows."""
import numpy as np
import pytest
import torch

from tests import gpu_guard as gg
from tests import nupconv_cases as nc
from tests.nupconv_model import NupFadeModel, NupTvModel

f32 = np.float32
PTS0, PTS1, N1, ROWS = 4, 8, 1, 2
CVS = nc.cvs(PTS1, N1, 0)
M = PTS1 // PTS0
NBLOCKS = nc.nblocks(M, N1)
rng = np.random.default_rng(1)
HA, HB = (rng.random((ROWS, CVS), dtype=f32) - 0.5 for _ in range(2))
X, W = (rng.random((ROWS, NBLOCKS * PTS0), dtype=f32) - 0.5 for _ in range(2))


def storage(t):
    """the whole buffer behind a view, as int32"""
    return torch.tensor([], dtype=torch.int32).set_(t.untyped_storage())


class Fake:
    """what the drivers use of a Nupconv, on CPU tensors; `fault` names the one thing it does wrong"""
    pts0, pts1, channels = PTS0, PTS1, ROWS

    def __init__(self, fault=None, model=NupFadeModel):
        self.model, self.fault = model(CVS, PTS0, PTS1, ROWS), fault
        self.model.push_ir(HA)
        self.fade = 0

    @property
    def position(self):
        return 0 if self.fault == "position" else self.model.position

    def nparts(self, level):
        return (self.model.n0, self.model.n1)[level]

    def fade_remaining(self):
        r = self.model.fade_remaining()
        return r + 1 if self.fault == "fade_remaining" and r < self.fade else r

    def process_device(self, out, x, w=None):
        y = self.model.process(x.numpy()) if w is None else self.model.process(x.numpy(), w.numpy())
        out.copy_(torch.from_numpy(y.astype(f32)))
        if out.numel() and self.fault == "past":
            storage(out)[out.storage_offset() + out.shape[1]] = 0
        if out.numel() and self.fault == "unwritten":
            storage(out)[out.storage_offset() + out.stride(0) + 1] = gg.CANARY
        if out.numel() and self.fault == "input":
            x[0, 1] += 1.0
        if out.numel() and self.fault == "second input":
            w[1, 0] += 1.0
        return 0

    process_tv_device = process_device

    def _fade(self, rows, fade, device):
        self.model.push_ir_fade(rows.numpy() if device else rows, fade)
        self.fade = fade
        if device and self.fault == "rows":
            rows[1, 2] = 0.0
        return 0

    def push_ir_fade(self, rows, fade):
        return self._fade(rows, fade, False)

    def push_ir_fade_device(self, rows, fade):
        return self._fade(rows, fade, True)


def truth(c=None, fade=None, nblocks=NBLOCKS, w=None, model=NupFadeModel):
    """the model's own output, rounded call by call as the fake rounds it (the rounding is per element: the cuts do not
    matter)"""
    m = model(CVS, PTS0, PTS1, ROWS)
    m.push_ir(HA)
    if c is None:
        return m.process(X, w).astype(f32)
    out = [m.process(X[:, :c * PTS0])]
    m.push_ir_fade(HB, fade)
    out.append(m.process(X[:, c * PTS0:nblocks * PTS0]))
    return np.concatenate(out, axis=1).astype(f32)


CUTS = ([NBLOCKS], [1] * NBLOCKS, [1, M + 2, 2, 0, NBLOCKS - M - 5])


@pytest.mark.parametrize("splits", CUTS)
def test_the_honest_fake_passes_run(splits):
    p = Fake()
    got = nc.run(nc.NUPCONV, p, X, splits, device="cpu")
    assert got.dtype == f32 and np.array_equal(got, truth()) and p.position == NBLOCKS
    assert np.array_equal(nc.run_aligned(nc.NUPCONV, Fake(), X, splits, device="cpu"), truth())


def test_the_honest_fake_passes_run_with_a_second_input():
    splits = [1, M + 2, 2, 0, NBLOCKS - M - 5]
    got = nc.run(nc.NUPCONV, Fake(model=NupTvModel), X, splits, W, device="cpu")
    assert np.array_equal(got, truth(w=W, model=NupTvModel))
    plain = nc.run(nc.NUPCONV, Fake(model=NupTvModel), X, splits, W, plain=range(5), device="cpu")
    assert np.array_equal(plain, truth(model=NupTvModel)) and not np.array_equal(plain, got)


@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("run", [nc.run, nc.run_aligned])
@pytest.mark.parametrize("style", ["one", "singles", "odd"])
def test_the_honest_fake_passes_faded(style, run, host):
    for c in nc.positions(M, N1):
        fade = nc.fades(M)[1]
        nblocks = c + fade + (N1 + 4) * M
        p = Fake()
        got = nc.faded(nc.NUPCONV, p, X, c, HB, fade, style, nblocks, host=host, run=run, device="cpu")
        assert np.array_equal(got, truth(c, fade, nblocks)), c
        assert p.position == nblocks and p.fade_remaining() == 0
        assert not np.array_equal(got[:, (c + fade) * PTS0:], truth()[:, (c + fade) * PTS0:nblocks * PTS0])


@pytest.mark.parametrize("fault,message", [
    ("past", "wrote between the rows"),
    ("unwritten", "an output element was not written"),
    ("input", "the input changed"),
    ("position", "the position after a call"),
])
def test_run_fails_on(fault, message):
    for splits in CUTS[:2]:
        with pytest.raises(AssertionError, match=message):
            nc.run(nc.NUPCONV, Fake(fault), X, splits, device="cpu")


def test_run_fails_on_a_changed_second_input():
    with pytest.raises(AssertionError, match="the second input changed"):
        nc.run(nc.NUPCONV, Fake("second input", NupTvModel), X, [NBLOCKS], W, device="cpu")


@pytest.mark.parametrize("fault,message", [
    ("past", "wrote between the rows"),
    ("unwritten", "an output element was not written"),
    ("input", "the input changed"),
    ("position", "the position after a call"),
    ("fade_remaining", r"fade_remaining\(\) and the position after a call"),
    ("rows", "the response rows changed"),
])
def test_faded_fails_on(fault, message):
    c, fade = 2 * M + 1, M + 1
    for style in ("one", "odd"):
        with pytest.raises(AssertionError, match=message):
            nc.faded(nc.NUPCONV, Fake(fault), X, c, HB, fade, style, c + fade + 4 * M, device="cpu")


def test_a_matrix_form_names_its_own_rows_and_pushes():
    """the drivers read the row counts and the fade pushes through the Form alone"""
    class FakeMatrix(Fake):
        inputs = outputs = ROWS
        channels = None
        fade_ir, fade_ir_device = Fake.push_ir_fade, Fake.push_ir_fade_device
        push_ir_fade = push_ir_fade_device = None   # (not the matrix's names)

    c, fade = M + 1, M + 1
    got = nc.faded(nc.MATRIX, FakeMatrix(), X, c, HB, fade, "odd", c + fade + 4 * M, device="cpu")
    assert np.array_equal(got, truth(c, fade, c + fade + 4 * M))
