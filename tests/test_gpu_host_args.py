"""The argument rules of Stft's and the convolutions' entry points at the C ABI, device form and blocking form, one row
per rule: NULL, alignment, stride, counts, direction, overlap (the span rule, and the multi-block device forms' row-precise
one), the matrix pushes during a fade.  Every bad pointer is NULL, misaligned or overlapping; a refused call writes nothing.
Rows that tests/test_gpu_stft.py, test_gpu_python_args.py and the convolutions' own tests assert are not repeated here."""
import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd._lib import lib

pytestmark = pytest.mark.gpu

INVALID, INVALID_OPERATION = -30, -59
SIZE, HOP, CH, SAMPLES, F, STRIDE = 64, 16, 2, 96, 3, 99      # Stft: L = (F - 1) * HOP + SIZE = SAMPLES
NSIG, NSPEC = STRIDE + SAMPLES, 2 * CH * F * (SIZE // 2)      # floats from a signal's first to its last, of the spectra
NB = 3                                                        # blocks of the multi-block calls


def _gpu():
    import torch
    from tests import gpu_guard
    return torch, gpu_guard, torch.cuda.current_stream().cuda_stream


def _host_canary(n):
    from tests.gpu_guard import CANARY
    return np.full(n, CANARY, np.int32)


def _stft(fwd):
    st = fa.Stft(0, SIZE, HOP, fwd=fwd)
    assert st.get_error() == 0, st.get_log()
    return st


# ---- Stft ------------------------------------------------------------------------------------------------------------
def test_stft_device_forms():
    torch, gg, s = _gpu()
    L = lib()
    g = gg.flat((2048,), misalign=0)
    base = g.data.data_ptr()
    sig, spec = base, base + 4 * 256          # apart: [0, 195) and [256, 640) floats
    an, sy = _stft(True), _stft(False)

    def analyze(signal, spectra, stride=STRIDE, samples=SAMPLES, channels=CH, st=an):
        return L.clfa_stft_analyze_dev(st._h, signal, stride, samples, channels, spectra, s)

    def synth(spectra, signal, stride=STRIDE, frames=F, channels=CH, st=sy):
        return L.clfa_stft_synthesize_dev(st._h, spectra, frames, channels, signal, stride, 0, s)

    for call in (analyze, synth):
        a, b = (sig, spec) if call is analyze else (spec, sig)
        flip = (lambda x, y: (x, y)) if call is analyze else (lambda x, y: (y, x))    # (signal, spectra) in the call's order
        assert call(None, b) == INVALID and call(a, None) == INVALID                  # NULL, each array in turn
        for off in (1, 2):                                                            # 4 asked of the signal, 8 of the spectra
            assert call(*flip(sig + off, spec)) == INVALID, off
        for off in (1, 2, 4):
            assert call(*flip(sig, spec + off)) == INVALID, off
        assert call(a, b, stride=SAMPLES - 1) == INVALID                              # one float short
        assert call(a, b, **{"samples" if call is analyze else "frames": -1}) == INVALID
        assert call(a, b, channels=-1) == INVALID
        # counts of 0 succeed before any pointer is looked at
        assert call(None, None, channels=0) == 0
        assert call(None, None, **{"samples" if call is analyze else "frames": 0}) == 0
        # the output overlaps the input by one element at either end, and starts where it starts
        assert call(*flip(base, base + 4 * (NSIG - 1))) == INVALID
        assert call(*flip(base + 4 * (NSPEC - 1), base)) == INVALID
        assert call(*flip(base, base)) == INVALID
    torch.cuda.synchronize()
    assert g.untouched()
    # a signal 4 bytes past an 8-byte boundary is accepted (and runs), so is one channel with a stride of 0
    g.data.zero_()
    assert analyze(sig + 4, spec) == 0 and analyze(sig, spec, stride=0, channels=1) == 0
    assert synth(spec, sig + 4) == 0 and synth(spec, sig, stride=0, channels=1) == 0
    torch.cuda.synchronize()
    assert g.intact()


def test_stft_blocking_forms():
    torch, gg, s = _gpu()
    L = lib()
    x = np.zeros(NSIG, np.float32)
    spec = np.zeros(NSPEC, np.float32)
    out_spec, out_sig = _host_canary(NSPEC), _host_canary(NSIG)
    an, sy = _stft(True), _stft(False)

    def analyze(signal, spectra, stride=STRIDE, samples=SAMPLES, channels=CH, st=an):
        return L.clfa_stft_analyze(st._h, signal, stride, samples, channels, spectra)

    def synth(spectra, signal, stride=STRIDE, frames=F, channels=CH, st=sy):
        return L.clfa_stft_synthesize(st._h, spectra, frames, channels, signal, stride, 0)

    xs, os_, ss, ox = x.ctypes.data, out_spec.ctypes.data, spec.ctypes.data, out_sig.ctypes.data
    assert analyze(None, os_) == INVALID and analyze(xs, None) == INVALID
    assert synth(None, ox) == INVALID and synth(ss, None) == INVALID
    # ... also where there is nothing to do: the blocking forms refuse a NULL before the no-op
    assert analyze(None, os_, channels=0) == INVALID and analyze(xs, None, samples=SIZE - 1) == INVALID
    assert synth(None, ox, frames=0) == INVALID and synth(ss, None, channels=0) == INVALID
    assert analyze(xs, os_, stride=SAMPLES - 1) == INVALID and synth(ss, ox, stride=SAMPLES - 1) == INVALID
    assert analyze(xs, os_, samples=-1) == INVALID and analyze(xs, os_, channels=-1) == INVALID
    assert synth(ss, ox, frames=-1) == INVALID and synth(ss, ox, channels=-1) == INVALID
    assert analyze(xs, os_, st=sy) == INVALID and synth(ss, ox, st=an) == INVALID          # wrong direction
    assert analyze(xs, os_, samples=SIZE - 1) == 0 and analyze(xs, os_, channels=0) == 0   # F = 0, no channels
    assert synth(ss, ox, frames=0) == 0 and synth(ss, ox, channels=0) == 0
    canary = _host_canary(1)[0]
    assert (out_spec == canary).all() and (out_sig == canary).all()
    # host arrays take any address, and one channel any stride
    odd = np.zeros(4 * NSIG + 8, np.uint8)
    assert analyze(odd.ctypes.data + (1 - odd.ctypes.data) % 4, os_) == 0
    assert not (out_spec == canary).any()
    assert synth(ss, ox, stride=0, channels=1) == 0
    assert not (out_sig[:SAMPLES] == canary).any() and (out_sig[SAMPLES:] == canary).all()


def test_stft_blocking_synthesis_writes_padded_rows():
    """signal_stride = L + 3: the rows are the device form's bits, and the three floats behind every row keep their NaN"""
    torch, gg, s = _gpu()
    rng = np.random.default_rng(64)
    spec = (rng.standard_normal((CH, F, SIZE // 2)) + 1j * rng.standard_normal((CH, F, SIZE // 2))).astype(np.complex64)
    w = (rng.random(SIZE, dtype=np.float32) + 0.25).astype(np.float32)
    st = fa.Stft(0, SIZE, HOP, window=w, fwd=False)
    assert st.get_error() == 0, st.get_log()
    for normalize in (0, 1):
        dev_out = gg.rows(CH, SAMPLES, SAMPLES)
        assert st.synthesize_device(gg.dev(spec), dev_out.data, normalize=bool(normalize)) == 0
        torch.cuda.synchronize()
        assert dev_out.intact() and not dev_out.unwritten()
        padded = np.full((CH, STRIDE), np.nan, np.float32)
        assert lib().clfa_stft_synthesize(st._h, spec.ctypes.data, F, CH, padded.ctypes.data, STRIDE, normalize) == 0
        assert np.isnan(padded[:, SAMPLES:]).all()
        assert np.array_equal(gg.bits(padded[:, :SAMPLES]), gg.bits(dev_out.host()))


# ---- the convolutions ------------------------------------------------------------------------------------------------
def _pconv():
    p = fa.Clpconv(0, 64, 32, channels=2)
    assert p.get_cl_err() == 0
    return p, 32, 2, 2, lib().clfa_pconv_process_blocks_dev, lib().clfa_pconv_convolution_blocks


def _dconv():
    d = fa.Cldconv(0, 8, 4, channels=2)
    assert d.get_cl_err() == 0
    return d, 4, 2, 2, lib().clfa_dconv_process_blocks_dev, lib().clfa_dconv_convolution_blocks


def _matrix():
    m = fa.PconvMatrix(0, 64, 32, 2, 2)
    assert m.get_error() == 0, m.get_log()
    dev, host = lib().clfa_pconv_matrix_process_dev, lib().clfa_pconv_matrix_convolution
    return (m, 32, 2, 2, lambda h, o, os_, i1, i2, is_, n, s: dev(h, o, os_, i1, is_, n, s),
            lambda h, o, i1, i2, n: host(h, o, i1, n))


@pytest.mark.parametrize("make", [_pconv, _dconv, _matrix])
def test_multi_block_device_forms(make):
    torch, gg, s = _gpu()
    obj, unit, in_rows, out_rows, dev, _ = make()
    two = make is not _matrix                      # a second input
    n = NB * unit                                  # floats per row
    pitch = 2 * n + 8                              # rows with a gap of n + 8 floats behind each
    g = gg.flat((2 * pitch + 2 * n,), misalign=0)
    base = g.data.data_ptr()
    out = base + 4 * (n + 4)                       # every output row inside a gap between (or behind) the input rows

    def call(o, i1, i2=None, os_=pitch, is_=pitch, k=NB):
        return dev(obj._h, o, os_, i1, i2, is_, k, s)

    # 4 bytes asked of every row pointer, NULL refused (the objects' own tests have out + 2 and a NULL out; the matrix's
    # and Cldconv's a NULL input, the matrix's in + 2)
    assert call(out + 1, base) == INVALID and call(out, base + 1) == INVALID
    if make is _pconv:
        assert call(out, None) == INVALID
    if two:
        assert call(out, base + 2) == INVALID
        for off in (1, 2):
            assert call(out, base, base + off) == INVALID, off
    torch.cuda.synchronize()
    assert g.untouched()
    # the row-precise rule: an output row lying wholly in the gap between two input rows is accepted, and written there
    w = g.words[0]
    rest = torch.ones_like(w, dtype=torch.bool)
    for r in range(2):
        w[r * pitch:r * pitch + n] = 0
        rest[r * pitch:r * pitch + n] = rest[n + 4 + r * pitch:2 * n + 4 + r * pitch] = False
    assert call(out, base, base if two else None) == 0
    torch.cuda.synchronize()
    assert g.intact() and bool((w[rest] == gg.CANARY).all()), "wrote outside the output rows"
    assert not bool((torch.stack([w[n + 4 + r * pitch:2 * n + 4 + r * pitch] for r in range(2)]) == gg.CANARY).any())
    # ... one float further on the first output row still lies in the gap, n + 4 floats further on it meets input row 1
    assert call(out + 4, base) == 0
    assert call(base + 4 * (pitch - n + 1), base) == INVALID


@pytest.mark.parametrize("make", [_pconv, _dconv, _matrix])
def test_multi_block_blocking_forms(make):
    torch, gg, s = _gpu()
    obj, unit, in_rows, out_rows, _, host = make()
    two = make is not _matrix
    n = NB * unit * in_rows                        # floats of a packed input (as many of the output: the shapes are square)
    buf = _host_canary(3 * n)
    base = buf.ctypes.data
    x = np.zeros(n, np.float32).ctypes.data

    def call(o, i1, i2=None, k=NB):
        return host(obj._h, o, i1, i2, k)

    assert call(None, x) == INVALID and call(base, None) == INVALID
    assert call(base, x, k=-1) == INVALID
    assert call(base, x, k=0) == 0
    # the packed spans: out meets in1 by one float at either end, or is in1; the same for in2
    for i1, o in ((base, base + 4 * (n - 1)), (base + 4 * (n - 1), base), (base, base)):
        assert call(o, i1) == INVALID
        if two:
            assert call(o, base + 4 * 2 * n, i1) == INVALID
    assert (buf == _host_canary(1)[0]).all()
    # apart by nothing: accepted; the inputs may be one array
    buf.view(np.float32)[:n] = 0
    assert call(base + 4 * n, base, base if two else None) == 0
    assert not (buf[n:2 * n] == _host_canary(1)[0]).any() and (buf[2 * n:] == _host_canary(1)[0]).all()


def test_pushes():
    torch, gg, s = _gpu()
    L = lib()
    p, d, m = _pconv()[0], _dconv()[0], _matrix()[0]
    g = gg.flat((1024,), misalign=0)
    g.data.zero_()
    base = g.data.data_ptr()
    host = np.zeros(1024, np.float32).ctypes.data
    # NULL, blocking and device form; the strides one float short that no other test asks at this level
    assert L.clfa_pconv_push_ir(p._h, None) == INVALID and L.clfa_pconv_push_ir_dev(p._h, None, 64, s) == INVALID
    assert L.clfa_pconv_push_ir_dev(p._h, base, 63, s) == INVALID
    assert L.clfa_dconv_push_ir(d._h, None) == INVALID
    assert L.clfa_pconv_matrix_push_ir(m._h, None) == INVALID and L.clfa_pconv_matrix_push_ir_dev(m._h, None, 64, s) == INVALID
    assert L.clfa_pconv_matrix_push_ir_fade(m._h, None, 2) == INVALID
    assert L.clfa_pconv_matrix_push_ir_fade_dev(m._h, None, 64, 2, s) == INVALID
    assert L.clfa_pconv_matrix_push_ir_fade_dev(m._h, base, 63, 2, s) == INVALID
    for off in (1, 2):   # device rows on 4 bytes
        assert L.clfa_dconv_push_ir_dev(d._h, base + off, 8, s) == INVALID
        assert L.clfa_pconv_matrix_push_ir_dev(m._h, base + off, 64, s) == INVALID
        assert L.clfa_pconv_matrix_push_ir_fade_dev(m._h, base + off, 64, 2, s) == INVALID
    assert m.fade_remaining() == 0
    # good pushes, blocking and device form, one and several channels
    one = fa.Cldconv(0, 8, 4)
    assert L.clfa_pconv_push_ir(p._h, host) == 0 and L.clfa_pconv_push_ir_dev(p._h, base + 4, 64, s) == 0
    assert L.clfa_dconv_push_ir(d._h, host) == 0 and L.clfa_dconv_push_ir(one._h, host) == 0
    assert L.clfa_dconv_push_ir_dev(d._h, base + 4, 8, s) == 0
    assert L.clfa_pconv_matrix_push_ir(m._h, host) == 0 and L.clfa_pconv_matrix_push_ir_dev(m._h, base + 4, 64, s) == 0
    # during a pending fade both matrix pushes are refused as operations, behind their invalid values
    assert L.clfa_pconv_matrix_push_ir_fade(m._h, host, 2) == 0 and m.fade_remaining() == 2
    assert L.clfa_pconv_matrix_push_ir(m._h, None) == INVALID and L.clfa_pconv_matrix_push_ir(m._h, host) == INVALID_OPERATION
    assert L.clfa_pconv_matrix_push_ir_fade(m._h, host, 0) == INVALID
    assert L.clfa_pconv_matrix_push_ir_fade(m._h, host, 2) == INVALID_OPERATION
    assert L.clfa_pconv_matrix_push_ir_dev(m._h, base + 2, 64, s) == INVALID
    assert L.clfa_pconv_matrix_push_ir_dev(m._h, base, 64, s) == INVALID_OPERATION
    assert L.clfa_pconv_matrix_push_ir_fade_dev(m._h, base, 64, 0, s) == INVALID
    assert L.clfa_pconv_matrix_push_ir_fade_dev(m._h, base, 64, 2, s) == INVALID_OPERATION
    assert m.fade_remaining() == 2
    torch.cuda.synchronize()
    assert g.intact()
