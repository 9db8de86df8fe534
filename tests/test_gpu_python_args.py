"""The argument contracts of the Python layer (opencl_fft_amd/conv.py) as a table: each row is a call on the smallest
object that reaches a branch and its outcome — a status code, ValueError with its message, or success with the output
compared (with the oracle, or bit for bit with another call).  The table records what the layer does, so that a change
of its plumbing (shared helpers, base classes) is checked row by row against the behaviour it had.

Objects: Clpconv(0, 128, 32) (4 partitions), Cldconv(0, 48, 16), PconvMatrix(0, 128, 32, 2, 3); signals of 2 blocks.
Cldconv takes any vsize >= 1 (3 included), so its error-callback rows use vsize = 0, the geometry its constructor refuses.
Bounds: Clpconv against the oracle 1e-6 relative L2 (the bound of smoke() for the same route), the matrix 4e-6 (a sum of
two such terms and one float32 rounding, no cancellation in seeded noise), Cldconv the dconv_tol of test_gpu_conv.py."""
import numpy as np
import pytest

import opencl_fft_amd as fa
from oracle import oracle

pytestmark = pytest.mark.gpu

INVALID = -30
CVS, PTS, IRSIZE, VSIZE, NB = 128, 32, 48, 16, 2
MSG = "expected a (%s, L) float32 tensor with stride(1) == 1"
HOST_MSG = "expected a writable C-contiguous numpy array of float32"


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.array(a)).cuda()   # (a copy: the shared cases are read-only)


def _padded(a, extra=5):
    """the rows of `a` as a [:, :L] slice of rows that are `extra` floats wider"""
    wide = _torch().full((a.shape[0], a.shape[1] + extra), 7.0, device="cuda")
    view = wide[:, :a.shape[1]]
    view.copy_(_torch().from_numpy(np.array(a)))
    return view


def _rel(y, ref):
    return float(np.linalg.norm(y.astype(np.float64) - ref) / np.linalg.norm(ref.astype(np.float64)))


# ---- the two block convolutions: one description each, so that every row runs on both ------------------------------
class _Kind:
    def __init__(self, name, cls, orc, size, blk, tol):
        self.name, self.cls, self.orc, self.size, self.blk, self.tol = name, cls, orc, size, blk, tol
        self._data = {}

    def make(self, channels, **kw):
        obj = self.cls(0, self.size, self.blk, channels=channels, **kw)
        assert obj.get_cl_err() == 0
        return obj

    def data(self, channels):
        """seeded responses, a signal of NB blocks and the oracle's output, computed once per channel count"""
        if channels not in self._data:
            rng = np.random.default_rng([self.size, self.blk, channels])
            ir = rng.random((channels, self.size), dtype=np.float32) - 0.5
            x = rng.random((channels, NB * self.blk), dtype=np.float32) - 0.5
            ref = np.zeros_like(x)
            for c in range(channels):
                o = self.orc(self.size, self.blk)
                o.push_ir(ir[c])
                for j in range(NB):
                    ref[c, j * self.blk:(j + 1) * self.blk] = o.convolution(x[c, j * self.blk:(j + 1) * self.blk])
            for a in (ir, x, ref):
                a.setflags(write=False)
            self._data[channels] = (ir, x, ref)
        return self._data[channels]

    def loaded(self, channels):
        obj = self.make(channels)
        ir, x, ref = self.data(channels)
        assert obj.push_ir(ir if channels > 1 else ir[0]) == 0
        return obj, x, ref

    def __repr__(self):
        return self.name


PCONV = _Kind("Clpconv", fa.Clpconv, oracle.Pconv, CVS, PTS, 1e-6)
DCONV = _Kind("Cldconv", fa.Cldconv, oracle.Dconv, IRSIZE, VSIZE, max(1e-6, 2 * float(np.sqrt(IRSIZE)) * 2.0 ** -24))
KINDS = pytest.mark.parametrize("kind", [PCONV, DCONV], ids=repr)


def _run_blocks(kind, channels, wrap_in, wrap_out, **kw):
    """process_blocks_device on a fresh object -> (status, output as numpy)"""
    torch = _torch()
    obj, x, _ = kind.loaded(channels)
    out = wrap_out(np.zeros_like(x))
    e = obj.process_blocks_device(out, wrap_in(x), **kw)
    torch.cuda.synchronize()
    return e, out.cpu().contiguous().numpy()


# ---- process_blocks_device --------------------------------------------------------------------------------------------
@KINDS
def test_blocks_contiguous_padded_and_streams(kind):
    torch = _torch()
    _, _, ref = kind.data(2)
    e, y = _run_blocks(kind, 2, _dev, _dev)
    err = _rel(y, ref)
    print("%s contiguous: relL2 %.3g (bound %.3g)" % (kind, err, kind.tol))
    assert e == 0 and err < kind.tol
    e, yp = _run_blocks(kind, 2, _padded, _padded)
    assert e == 0 and np.array_equal(yp.view(np.uint32), y.view(np.uint32))   # padded-row views: bit-identical
    e, ys = _run_blocks(kind, 2, _dev, _dev, stream=torch.cuda.current_stream().cuda_stream)
    assert e == 0 and np.array_equal(ys.view(np.uint32), y.view(np.uint32))   # stream=None is the current stream


@KINDS
def test_blocks_1d_one_channel(kind):
    _, _, ref = kind.data(1)
    e, y = _run_blocks(kind, 1, lambda a: _dev(a[0]), lambda a: _dev(a[0]))
    assert e == 0 and y.shape == (NB * kind.blk,) and _rel(y, ref[0]) < kind.tol
    e, y2 = _run_blocks(kind, 1, _dev, _dev)
    assert e == 0 and np.array_equal(y2[0].view(np.uint32), y.view(np.uint32))


def _blocks_args(kind, what):
    """(out, in1, in2) for the rows that do not reach the library"""
    torch = _torch()
    L = NB * kind.blk
    z = lambda rows, n, dt=torch.float32: torch.zeros((rows, n), dtype=dt, device="cuda")
    return {
        "1d_two_channels": (z(2, L)[0], z(2, L)[0], None),
        "1d_out_two_channels": (z(2, L)[0], z(2, L), None),
        "float64_in": (z(2, L), z(2, L, torch.float64), None),
        "float64_out": (z(2, L, torch.float64), z(2, L), None),
        "float64_in2": (z(2, L), z(2, L), z(2, L, torch.float64)),
        "strided_samples": (z(2, L), z(2, 2 * L)[:, ::2], None),
        "three_rows": (z(2, L), z(3, L), None),
        "3d": (z(2, L), z(2, L).unsqueeze(0), None),
        "length_not_blocks": (z(2, L + kind.blk // 2), z(2, L + kind.blk // 2), None),
        "out_shorter": (z(2, L - kind.blk), z(2, L), None),
        "in2_shorter": (z(2, L), z(2, L), z(2, L - kind.blk)),
        "in2_other_stride": (z(2, L), z(2, L), z(2, L + 5)[:, :L]),
    }[what]


BLOCKS_ROWS = [("1d_two_channels", ValueError), ("1d_out_two_channels", ValueError), ("float64_in", ValueError),
               ("float64_out", ValueError), ("float64_in2", ValueError), ("strided_samples", ValueError),
               ("three_rows", ValueError), ("3d", ValueError), ("length_not_blocks", INVALID), ("out_shorter", INVALID),
               ("in2_shorter", INVALID), ("in2_other_stride", INVALID)]


@KINDS
@pytest.mark.parametrize("what,outcome", BLOCKS_ROWS, ids=[r[0] for r in BLOCKS_ROWS])
def test_blocks_refusals(kind, what, outcome):
    obj = kind.make(2)
    out, in1, in2 = _blocks_args(kind, what)
    if outcome is ValueError:
        with pytest.raises(ValueError) as ei:
            obj.process_blocks_device(out, in1, in2)
        assert str(ei.value) == MSG % "channels"
    else:
        assert obj.process_blocks_device(out, in1, in2) == outcome


# ---- PconvMatrix.process_device ----------------------------------------------------------------------------------------
MI, MO = 2, 3
_MATRIX = {}


def _matrix_data():
    if not _MATRIX:
        rng = np.random.default_rng([CVS, PTS, MI, MO])
        ir = rng.random((MO, MI, CVS), dtype=np.float32) - 0.5
        x = rng.random((MI, NB * PTS), dtype=np.float32) - 0.5
        ref = np.zeros((MO, NB * PTS), np.float64)
        for o in range(MO):
            for i in range(MI):
                p = oracle.Pconv(CVS, PTS)
                p.push_ir(ir[o, i])
                for j in range(NB):
                    ref[o, j * PTS:(j + 1) * PTS] += p.convolution(x[i, j * PTS:(j + 1) * PTS])
        for a in (ir, x, ref):
            a.setflags(write=False)
        _MATRIX["d"] = (ir, x, ref)
    return _MATRIX["d"]


def _matrix():
    m = fa.PconvMatrix(0, CVS, PTS, MI, MO)
    assert m.get_error() == 0, m.get_log()
    return m


def _run_matrix(wrap, **kw):
    ir, x, _ = _matrix_data()
    m = _matrix()
    assert m.push_ir(ir) == 0
    out = wrap(np.zeros((MO, NB * PTS), np.float32))
    e = m.process_device(out, wrap(x), **kw)
    _torch().cuda.synchronize()
    return e, out.cpu().contiguous().numpy()


def test_matrix_contiguous_padded_and_streams():
    torch = _torch()
    e, y = _run_matrix(_dev)
    err = _rel(y, _matrix_data()[2])
    print("PconvMatrix contiguous: relL2 %.3g (bound 4e-6)" % err)
    assert e == 0 and err < 4e-6
    e, yp = _run_matrix(_padded)
    assert e == 0 and np.array_equal(yp.view(np.uint32), y.view(np.uint32))
    e, ys = _run_matrix(_dev, stream=torch.cuda.current_stream().cuda_stream)
    assert e == 0 and np.array_equal(ys.view(np.uint32), y.view(np.uint32))


def _matrix_args(what):
    torch = _torch()
    L = NB * PTS
    z = lambda rows, n, dt=torch.float32: torch.zeros((rows, n), dtype=dt, device="cuda")
    return {
        "1d_in": (z(MO, L), z(MI, L)[0], MI),
        "1d_out": (z(MO, L)[0], z(MI, L), MO),
        "float64_in": (z(MO, L), z(MI, L, torch.float64), MI),
        "float64_out": (z(MO, L, torch.float64), z(MI, L), MO),
        "strided_samples": (z(MO, L), z(MI, 2 * L)[:, ::2], MI),
        "rows_swapped": (z(MI, L), z(MO, L), MO),
        "length_not_blocks": (z(MO, L + PTS // 2), z(MI, L + PTS // 2), INVALID),
        "out_shorter": (z(MO, L - PTS), z(MI, L), INVALID),
    }[what]


@pytest.mark.parametrize("what", ["1d_in", "1d_out", "float64_in", "float64_out", "strided_samples", "rows_swapped",
                                  "length_not_blocks", "out_shorter"])
def test_matrix_refusals(what):
    out, x, outcome = _matrix_args(what)
    m = _matrix()
    if outcome == INVALID:
        assert m.process_device(out, x) == INVALID
    else:
        with pytest.raises(ValueError) as ei:
            m.process_device(out, x)
        assert str(ei.value) == MSG % outcome   # the row count of the tensor that was refused


# ---- push_ir_device -----------------------------------------------------------------------------------------------------
@KINDS
def test_push_ir_device_1d_row_one_channel(kind):
    torch = _torch()
    ir, x, ref = kind.data(1)
    obj = kind.make(1)
    row = _dev(ir[0])
    assert obj.push_ir_device(row) == 0
    out = _dev(np.zeros_like(x))
    assert obj.process_blocks_device(out, _dev(x)) == 0
    torch.cuda.synchronize()
    assert _rel(out.cpu().numpy(), ref) < kind.tol


@KINDS
def test_push_ir_device_rows(kind):
    torch = _torch()
    ir = kind.data(2)[0]
    obj = kind.make(2)
    good, wide = _dev(ir), _padded(ir)            # (kept until the synchronise below)
    assert obj.push_ir_device(good) == 0
    assert obj.push_ir_device(good, stream=torch.cuda.current_stream().cuda_stream) == 0
    if kind is PCONV:                             # Clpconv wants the whole tensor contiguous, Cldconv takes the row stride
        with pytest.raises(ValueError) as ei:
            obj.push_ir_device(wide)
        assert str(ei.value) == "device tensor must be contiguous"
    else:
        assert obj.push_ir_device(wide) == 0
    assert obj.push_ir_device(_dev(ir[:, :kind.size - 1])) == INVALID                       # short rows
    assert obj.push_ir_device(_dev(ir.astype(np.float64))) == INVALID                       # wrong dtype
    assert obj.push_ir_device(_dev(np.concatenate([ir, ir[:1]]))) == INVALID                # wrong leading shape
    assert obj.push_ir_device(_dev(ir[0])) == INVALID                                       # 1-D row, two channels
    assert obj.push_ir_device(_dev(np.repeat(ir, 2, axis=1))[:, ::2]) == INVALID            # stride(1) != 1
    torch.cuda.synchronize()


def test_push_ir_device_matrix():
    torch = _torch()
    ir = _matrix_data()[0]
    m = _matrix()
    good = _dev(ir)                               # (kept until the synchronise below)
    assert m.push_ir_device(good) == 0
    assert m.push_ir_device(good, stream=torch.cuda.current_stream().cuda_stream) == 0
    assert m.push_ir_device(_dev(ir[:, :, :CVS - 1])) == INVALID                            # short rows
    assert m.push_ir_device(_dev(ir.astype(np.float64))) == INVALID                         # wrong dtype
    assert m.push_ir_device(_dev(ir[:MI])) == INVALID                                       # wrong leading shape
    assert m.push_ir_device(_dev(ir[0])) == INVALID                                         # two axes
    wide = torch.zeros((MO, MI * CVS + 44), device="cuda")
    uneven = torch.as_strided(wide, (MO, MI, CVS), (MI * CVS + 44, CVS, 1))
    assert m.push_ir_device(uneven) == INVALID                                              # stride(0) != inputs * stride(1)
    assert m.push_ir_fade_device(uneven, 2) == INVALID
    torch.cuda.synchronize()


# ---- convolution / convolution_blocks on the host ---------------------------------------------------------------------
@KINDS
@pytest.mark.parametrize("method,n", [("convolution", 1), ("convolution_blocks", NB)])
def test_host_refusals(kind, method, n):
    obj = kind.make(2)
    call = getattr(obj, method)
    L = n * kind.blk
    x = np.zeros((2, L), np.float32)
    out = np.zeros((2, L), np.float32)
    assert call(out, x) == 0
    assert call(out, x, x) == 0
    assert call(out, np.zeros((2, L - 1), np.float32)) == INVALID                           # wrong size
    assert call(np.zeros((2, L + 1), np.float32), x) == INVALID
    assert call(out, x, np.zeros((2, L - 1), np.float32)) == INVALID                        # input2 of a wrong size
    frozen = np.zeros((2, L), np.float32)
    frozen.setflags(write=False)
    for bad in (frozen, np.zeros((2, 2 * L), np.float32)[:, ::2], np.zeros((2, L), np.float64)):
        with pytest.raises(ValueError) as ei:
            call(bad, x)
        assert str(ei.value) == HOST_MSG


# ---- the error callback (cl_conv.h:142-145) ---------------------------------------------------------------------------
BAD = [(fa.Clpconv, (0, CVS, 3)), (fa.Cldconv, (0, IRSIZE, 0))]


@pytest.mark.parametrize("cls,args", BAD, ids=["Clpconv", "Cldconv"])
def test_error_callback(cls, args, capsys):
    calls, ud = [], object()
    obj = cls(*args, errs=lambda msg, data: calls.append((msg, data)), uData=ud)
    assert obj.get_cl_err() == INVALID
    assert calls == [("Invalid value", ud)] and calls[0][1] is ud
    assert obj.cl_error_string(INVALID) == "Invalid value"
    calls.clear()
    cls(*args, errs=lambda msg, data: calls.append((msg, data)))
    assert calls == [("Invalid value", None)]
    assert capsys.readouterr().out == ""
    cls(*args)                                    # neither: printed
    assert capsys.readouterr().out == "Invalid value\n"
    cls(*args, uData=ud)                          # user data only: silent
    assert capsys.readouterr().out == ""
