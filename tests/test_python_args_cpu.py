"""The argument contracts of the Python layer of Pvoc and Stft (opencl_fft_amd/pvoc.py, stft.py), and the device
refusals of the convolution classes (conv.py) that need no device, as a table in the style of test_gpu_python_args.py:
each row is one call and its outcome, so that a change of the layer's plumbing is checked row by row against the
behaviour it had.

There is no device here, so every object has failed to set up with -1 (Device not found).  A device call the Python
layer accepts returns the library's answer, which comes before the library touches memory (the
test_argument_errors_come_before_the_device_lookup tests): -1, or -59 for the blur before blur_setup.  A call the layer
refuses returns -30 or raises ValueError; the blocking host forms raise ClError with the code.  The rows take CPU
tensors and stream=0 — never stream=None, which asks torch for a HIP stream.  With a working object the same calls would
hand host addresses to a kernel, so the whole module is skipped where a device is present: there test_gpu_pvoc*.py,
test_gpu_stft*.py and test_gpu_python_args.py make the same checks on device memory.

Objects: Pvoc(0, 64, 16, sr, 2) and one with channels=1 for the rows without the leading axis, Stft(0, 64, 16) forward
and inverse, F = 3; Clpconv(0, 128, 32), Cldconv(0, 48, 16) with two channels, Cldconv(0, 1, 16), PconvMatrix(0, 128,
32, 2, 3).  A failed PconvMatrix has nparts == 0, so its push_ir_device never finds a row too short here; Clpconv(0, 128,
3), refused for its geometry, has none either, which lets a row of one sample reach Clpconv's stride test."""
import numpy as np
import pytest
import torch

import opencl_fft_amd as fa

if fa.device_count() > 0:
    pytest.skip("a HIP device is present: these calls would hand host addresses to a kernel", allow_module_level=True)

INVALID, NO_DEVICE, INVALID_OPERATION = -30, -1, -59
SIZE, HOP, SR, F = 64, 16, 48000.0, 3
M = SIZE // 2
L = F * HOP                       # samples of F frames from adsyn
NS = SIZE + (F - 1) * HOP         # samples that Stft frames into F frames, and that F frames overlap-add to
f32, f64, c64, c128, i32, i64 = (torch.float32, torch.float64, torch.complex64, torch.complex128, torch.int32,
                                 torch.int64)
ROWS_MSG = "%s: expected (channels, n) with contiguous rows"
BLOCK_MSG = "expected a (%s, L) float32 tensor with stride(1) == 1"
CONTIG_MSG = "device tensor must be contiguous"


def _quiet(msg, data):
    pass


PV = fa.Pvoc(0, SIZE, HOP, SR, 2)
PV1 = fa.Pvoc(0, SIZE, HOP, SR, 1)
ST = fa.Stft(0, SIZE, HOP)
STI = fa.Stft(0, SIZE, HOP, fwd=False)
CVS, PTS, IRSIZE, VSIZE, NB, MI, MO = 128, 32, 48, 16, 2, 2, 3
PC = fa.Clpconv(0, CVS, PTS, errs=_quiet, channels=2)
PC1 = fa.Clpconv(0, CVS, PTS, errs=_quiet)
PC0 = fa.Clpconv(0, CVS, 3, errs=_quiet, channels=2)         # no partitions: rows of any length are long enough
DC = fa.Cldconv(0, IRSIZE, VSIZE, errs=_quiet, channels=2)
DC1 = fa.Cldconv(0, 1, VSIZE, errs=_quiet, channels=2)      # responses of one sample
MX = fa.PconvMatrix(0, CVS, PTS, MI, MO)


def test_the_objects_found_no_device():
    assert [o.get_error() for o in (PV, PV1, ST, STI, MX)] == [NO_DEVICE] * 5
    assert [o.get_cl_err() for o in (PC, PC1, DC, DC1)] == [NO_DEVICE] * 4
    assert PC0.get_cl_err() == INVALID and (PC.nparts, PC0.nparts, MX.nparts) == (CVS // PTS, 0, 0)


def fr(c=2, f=F, dt=f32):
    """frames; c=None: without the channel axis"""
    return torch.zeros(((c,) if c else ()) + (f, M + 1, 2), dtype=dt)


def sp(c=2, f=F, dt=c64):
    """spectra; c=None: without the channel axis"""
    return torch.zeros(((c,) if c else ()) + (f, M), dtype=dt)


def per(n=F, dt=f32):
    """a per-frame value"""
    return torch.ones(n, dtype=dt)


def z(*shape, dt=f32):
    return torch.zeros(shape, dtype=dt)


def strided(t):
    """the same shape and values with every stride doubled: not contiguous, stride(-1) == 2"""
    return torch.stack([t, t], dim=-1)[..., 0]


def padded(t, extra=5):
    """the rows of a 2-D tensor as a [:, :n] view of wider rows"""
    return torch.zeros((t.shape[0], t.shape[1] + extra), dtype=t.dtype)[:, :t.shape[1]]


def nfr(c=2, f=F):
    return np.zeros(((c,) if c else ()) + (f, M + 1, 2), np.float32)


def _outcome(call):
    try:
        return call()
    except ValueError as e:
        return ValueError, str(e)
    except fa.ClError as e:
        return fa.ClError, e.code


def _host(code=NO_DEVICE):
    return fa.ClError, code


TABLE = np.ones(M + 1, np.float32)
FRAMES_MSG = ValueError, "frames must be (2, F, %d, 2)" % (M + 1)

ROWS = [
    # ---- Pvoc.analyze_device / synthesize_device: spectra and frames -----------------------------------------------
    ("analyze_device", lambda: PV.analyze_device(sp(), fr(), stream=0), NO_DEVICE),
    ("synthesize_device", lambda: PV.synthesize_device(fr(), sp(), stream=0), NO_DEVICE),
    ("analyze_device one channel, no axis", lambda: PV1.analyze_device(sp(None), fr(None), stream=0), NO_DEVICE),
    ("analyze_device one channel, with axis", lambda: PV1.analyze_device(sp(1), fr(1), stream=0), NO_DEVICE),
    ("analyze_device one channel, mixed", lambda: PV1.analyze_device(sp(None), fr(1), stream=0), NO_DEVICE),
    ("analyze_device complex128", lambda: PV.analyze_device(sp(dt=c128), fr(), stream=0), INVALID),
    ("analyze_device float64 frames", lambda: PV.analyze_device(sp(), fr(dt=f64), stream=0), INVALID),
    ("analyze_device strided spectra", lambda: PV.analyze_device(strided(sp()), fr(), stream=0), INVALID),
    ("analyze_device strided frames", lambda: PV.analyze_device(sp(), strided(fr()), stream=0), INVALID),
    ("analyze_device other F", lambda: PV.analyze_device(sp(f=F + 1), fr(), stream=0), INVALID),
    ("analyze_device three channels", lambda: PV.analyze_device(sp(3), fr(3), stream=0), INVALID),
    ("analyze_device no axis, two channels", lambda: PV.analyze_device(sp(None), fr(None), stream=0), INVALID),
    ("analyze_device one bin more", lambda: PV.analyze_device(z(2, F, M + 1, dt=c64), fr(), stream=0), INVALID),
    ("synthesize_device float64 frames", lambda: PV.synthesize_device(fr(dt=f64), sp(), stream=0), INVALID),
    ("synthesize_device other F", lambda: PV.synthesize_device(fr(), sp(f=F - 1), stream=0), INVALID),
    ("analyze", lambda: PV.analyze(np.zeros((2, F, M), np.complex64)), _host()),
    ("analyze one channel, no axis", lambda: PV1.analyze(np.zeros((F, M), np.complex64)), _host()),
    ("analyze three channels", lambda: PV.analyze(np.zeros((3, F, M), np.complex64)),
     (ValueError, "spectra must be (2, F, %d)" % M)),
    ("synthesize", lambda: PV.synthesize(nfr()), _host()),
    ("synthesize no axis, two channels", lambda: PV.synthesize(nfr(None)), FRAMES_MSG),
    ("synthesize one bin less", lambda: PV.synthesize(np.zeros((2, F, M, 2), np.float32)), FRAMES_MSG),
    # ---- scale, shift, read: one per-frame value -------------------------------------------------------------------------
    ("scale_device number", lambda: PV.scale_device(fr(), fr(), 1.5, stream=0), NO_DEVICE),
    ("scale_device tensor", lambda: PV.scale_device(fr(), fr(), per(), keepform=True, coefs=10, stream=0), NO_DEVICE),
    ("scale_device one channel, no axis", lambda: PV1.scale_device(fr(None), fr(None), 1.5, stream=0), NO_DEVICE),
    ("scale_device float64 in", lambda: PV.scale_device(fr(dt=f64), fr(), 1.5, stream=0), INVALID),
    ("scale_device float64 out", lambda: PV.scale_device(fr(), fr(dt=f64), 1.5, stream=0), INVALID),
    ("scale_device strided in", lambda: PV.scale_device(strided(fr()), fr(), 1.5, stream=0), INVALID),
    ("scale_device strided out", lambda: PV.scale_device(fr(), strided(fr()), 1.5, stream=0), INVALID),
    ("scale_device other F", lambda: PV.scale_device(fr(f=F + 1), fr(), 1.5, stream=0), INVALID),
    ("scale_device three channels", lambda: PV.scale_device(fr(3), fr(3), 1.5, stream=0), INVALID),
    ("scale_device no axis, two channels", lambda: PV.scale_device(fr(None), fr(None), 1.5, stream=0), INVALID),
    ("scale_device per-frame longer", lambda: PV.scale_device(fr(), fr(), per(F + 1), stream=0), INVALID),
    ("scale_device per-frame float64", lambda: PV.scale_device(fr(), fr(), per(dt=f64), stream=0), INVALID),
    ("scale_device per-frame strided", lambda: PV.scale_device(fr(), fr(), strided(per()), stream=0), INVALID),
    ("scale_device per-frame (F, 1)", lambda: PV.scale_device(fr(), fr(), z(F, 1), stream=0), INVALID),
    ("shift_device number", lambda: PV.shift_device(fr(), fr(), 100.0, stream=0), NO_DEVICE),
    ("shift_device tensor", lambda: PV.shift_device(fr(), fr(), per(), lowest_bin=2, stream=0), NO_DEVICE),
    ("shift_device other F", lambda: PV.shift_device(fr(), fr(f=F + 1), 100.0, stream=0), INVALID),
    ("shift_device per-frame shorter", lambda: PV.shift_device(fr(), fr(), per(F - 1), stream=0), INVALID),
    ("read_device", lambda: PV.read_device(fr(), per(5), fr(f=5), stream=0), NO_DEVICE),
    ("read_device number", lambda: PV.read_device(fr(), 1.0, fr(f=5), stream=0), INVALID),
    ("read_device pos of the input's F", lambda: PV.read_device(fr(), per(F), fr(f=5), stream=0), INVALID),
    ("read_device float64 pos", lambda: PV.read_device(fr(), per(5, f64), fr(f=5), stream=0), INVALID),
    ("scale", lambda: PV.scale(nfr(), 1.5), _host()),
    ("scale array", lambda: PV.scale(nfr(), np.full(F, 1.5)), _host()),
    ("scale no axis, two channels", lambda: PV.scale(nfr(None), 1.5), FRAMES_MSG),
    ("shift", lambda: PV.shift(nfr(), 100.0), _host()),
    ("read", lambda: PV.read(nfr(), np.zeros(5)), _host()),
    ("read one channel, no axis", lambda: PV1.read(nfr(None), [0.5, 1.5]), _host()),
    # ---- cross, morph, filter, mix, vocode: two inputs, two per-frame values --------------------------------------------
    ("cross_device numbers", lambda: PV.cross_device(fr(), fr(), fr(), stream=0), NO_DEVICE),
    ("cross_device tensors", lambda: PV.cross_device(fr(), fr(), fr(), per(), per(), stream=0), NO_DEVICE),
    ("cross_device one channel, no axis", lambda: PV1.cross_device(fr(None), fr(None), fr(None), stream=0), NO_DEVICE),
    ("morph_device", lambda: PV.morph_device(fr(), fr(), fr(), 0.25, per(), stream=0), NO_DEVICE),
    ("filter_device", lambda: PV.filter_device(fr(), fr(), fr(), stream=0), NO_DEVICE),
    ("mix_device", lambda: PV.mix_device(fr(), fr(), fr(), stream=0), NO_DEVICE),
    ("vocode_device", lambda: PV.vocode_device(fr(), fr(), fr(), coefs=10, stream=0), NO_DEVICE),
    ("cross_device float64 a", lambda: PV.cross_device(fr(dt=f64), fr(), fr(), stream=0), INVALID),
    ("cross_device float64 b", lambda: PV.cross_device(fr(), fr(dt=f64), fr(), stream=0), INVALID),
    ("cross_device float64 out", lambda: PV.cross_device(fr(), fr(), fr(dt=f64), stream=0), INVALID),
    ("cross_device strided b", lambda: PV.cross_device(fr(), strided(fr()), fr(), stream=0), INVALID),
    ("cross_device other F in a", lambda: PV.cross_device(fr(f=F + 1), fr(), fr(), stream=0), INVALID),
    ("cross_device other F in out", lambda: PV.cross_device(fr(), fr(), fr(f=F + 1), stream=0), INVALID),
    ("cross_device mixed axes", lambda: PV.cross_device(fr(), fr(), fr(None), stream=0), INVALID),
    ("cross_device second value longer", lambda: PV.cross_device(fr(), fr(), fr(), 1.0, per(F + 1), stream=0), INVALID),
    ("morph_device first value float64", lambda: PV.morph_device(fr(), fr(), fr(), per(dt=f64), stream=0), INVALID),
    ("mix_device three channels", lambda: PV.mix_device(fr(3), fr(3), fr(3), stream=0), INVALID),
    ("vocode_device other F in b", lambda: PV.vocode_device(fr(), fr(f=F - 1), fr(), stream=0), INVALID),
    ("cross", lambda: PV.cross(nfr(), nfr()), _host()),
    ("morph", lambda: PV.morph(nfr(), nfr(), np.full(F, 0.5), 0.25), _host()),
    ("filter", lambda: PV.filter(nfr(), nfr()), _host()),
    ("mix", lambda: PV.mix(nfr(), nfr()), _host()),
    ("vocode", lambda: PV.vocode(nfr(), nfr(), coefs=10), _host()),
    ("cross other F in b", lambda: PV.cross(nfr(), nfr(f=F + 1)), (ValueError, "a and b must have the same shape")),
    ("mix no axis, two channels", lambda: PV.mix(nfr(None), nfr(None)), FRAMES_MSG),
    # ---- band, mask, stencil, arp, lock, warp: per-frame rows and a table ---------------------------------------------
    ("band_device numbers", lambda: PV.band_device(fr(), fr(), 100.0, 200.0, 1000.0, 2000.0, stream=0), NO_DEVICE),
    ("band_device tensors", lambda: PV.band_device(fr(), fr(), per(), 200.0, per(), 2000.0, reject=True, stream=0),
     NO_DEVICE),
    ("band_device one channel, no axis", lambda: PV1.band_device(fr(None), fr(None), 1.0, 2.0, 3.0, 4.0, stream=0),
     NO_DEVICE),
    ("mask_device", lambda: PV.mask_device(fr(), fr(), per(M + 1), stream=0), NO_DEVICE),
    ("stencil_device", lambda: PV.stencil_device(fr(), fr(), per(M + 1), 0.5, per(), stream=0), NO_DEVICE),
    ("arp_device", lambda: PV.arp_device(fr(), fr(), 0.5, stream=0), NO_DEVICE),
    ("lock_device", lambda: PV.lock_device(fr(), fr(), stream=0), NO_DEVICE),
    ("warp_device", lambda: PV.warp_device(fr(), fr(), 1.5, coefs=10, stream=0), NO_DEVICE),
    ("band_device float64 in", lambda: PV.band_device(fr(dt=f64), fr(), 1.0, 2.0, 3.0, 4.0, stream=0), INVALID),
    ("band_device other F", lambda: PV.band_device(fr(), fr(f=F + 1), 1.0, 2.0, 3.0, 4.0, stream=0), INVALID),
    ("band_device third value longer", lambda: PV.band_device(fr(), fr(), 1.0, 2.0, per(F + 1), 4.0, stream=0), INVALID),
    ("band_device first value float64", lambda: PV.band_device(fr(), fr(), per(dt=f64), 2.0, 3.0, 4.0, stream=0), INVALID),
    ("mask_device shorter table", lambda: PV.mask_device(fr(), fr(), per(M), stream=0), INVALID),
    ("mask_device float64 table", lambda: PV.mask_device(fr(), fr(), per(M + 1, f64), stream=0), INVALID),
    ("mask_device strided table", lambda: PV.mask_device(fr(), fr(), strided(per(M + 1)), stream=0), INVALID),
    ("mask_device list for a table", lambda: PV.mask_device(fr(), fr(), [1.0] * (M + 1), stream=0), INVALID),
    ("stencil_device longer table", lambda: PV.stencil_device(fr(), fr(), per(M + 2), stream=0), INVALID),
    ("stencil_device strided out", lambda: PV.stencil_device(fr(), strided(fr()), per(M + 1), stream=0), INVALID),
    ("arp_device depth shorter", lambda: PV.arp_device(fr(), fr(), 0.5, per(F - 1), stream=0), INVALID),
    ("lock_device no axis, two channels", lambda: PV.lock_device(fr(None), fr(None), stream=0), INVALID),
    ("warp_device float64 out", lambda: PV.warp_device(fr(), fr(dt=f64), 1.5, stream=0), INVALID),
    ("band", lambda: PV.band(nfr(), 100.0, 200.0, 1000.0, 2000.0), _host()),
    ("mask", lambda: PV.mask(nfr(), TABLE), _host()),
    ("stencil", lambda: PV.stencil(nfr(), TABLE), _host()),
    ("arp", lambda: PV.arp(nfr(), 0.5), _host()),
    ("lock", lambda: PV.lock(nfr(), np.ones(F)), _host()),
    ("warp", lambda: PV.warp(nfr(), 1.5, coefs=10), _host()),
    ("mask shorter table", lambda: PV.mask(nfr(), TABLE[:M]), (ValueError, "table must be (%d,)" % (M + 1))),
    ("stencil longer table", lambda: PV.stencil(nfr(), np.ones(M + 2)), (ValueError, "table must be (%d,)" % (M + 1))),
    ("band three channels", lambda: PV.band(nfr(3), 1.0, 2.0, 3.0, 4.0), FRAMES_MSG),
    # ---- blur, smooth, freeze: along the frames ---------------------------------------------------------------------------
    ("blur_device before blur_setup", lambda: PV.blur_device(fr(), fr(), 2.0, stream=0), INVALID_OPERATION),
    ("blur_device tensor", lambda: PV.blur_device(fr(), fr(), per(), stream=0), INVALID_OPERATION),
    ("smooth_device", lambda: PV.smooth_device(fr(), fr(), stream=0), NO_DEVICE),
    ("freeze_device", lambda: PV.freeze_device(fr(), fr(), per(), per(), stream=0), NO_DEVICE),
    ("smooth_device one channel, no axis", lambda: PV1.smooth_device(fr(None), fr(None), stream=0), NO_DEVICE),
    ("blur_device other F", lambda: PV.blur_device(fr(), fr(f=F + 1), 2.0, stream=0), INVALID),
    ("blur_device length shorter", lambda: PV.blur_device(fr(), fr(), per(F - 1), stream=0), INVALID),
    ("smooth_device float64 in", lambda: PV.smooth_device(fr(dt=f64), fr(), stream=0), INVALID),
    ("smooth_device second value float64", lambda: PV.smooth_device(fr(), fr(), 0.5, per(dt=f64), stream=0), INVALID),
    ("freeze_device strided in", lambda: PV.freeze_device(strided(fr()), fr(), stream=0), INVALID),
    ("blur before blur_setup", lambda: PV.blur(nfr(), 2.0), _host(INVALID_OPERATION)),
    ("smooth", lambda: PV.smooth(nfr()), _host()),
    ("freeze", lambda: PV.freeze(nfr(), np.zeros(F), 1.0), _host()),
    ("freeze no axis, two channels", lambda: PV.freeze(nfr(None)), FRAMES_MSG),
    # ---- describe ----------------------------------------------------------------------------------------------------------
    ("describe_device", lambda: PV.describe_device(fr(), z(2, F, 8), stream=0), NO_DEVICE),
    ("describe_device bins", lambda: PV.describe_device(fr(), z(2, F, 8), 2, 5, rectify=True, stream=0), NO_DEVICE),
    ("describe_device one channel, no axis", lambda: PV1.describe_device(fr(None), z(F, 8), stream=0), NO_DEVICE),
    ("describe_device one channel, out with axis", lambda: PV1.describe_device(fr(None), z(1, F, 8), stream=0), NO_DEVICE),
    ("describe_device seven columns", lambda: PV.describe_device(fr(), z(2, F, 7), stream=0), INVALID),
    ("describe_device float64 out", lambda: PV.describe_device(fr(), z(2, F, 8, dt=f64), stream=0), INVALID),
    ("describe_device strided out", lambda: PV.describe_device(fr(), strided(z(2, F, 8)), stream=0), INVALID),
    ("describe_device out of other F", lambda: PV.describe_device(fr(), z(2, F + 1, 8), stream=0), INVALID),
    ("describe_device out without axis, two channels", lambda: PV.describe_device(fr(), z(F, 8), stream=0), INVALID),
    ("describe_device float64 in", lambda: PV.describe_device(fr(dt=f64), z(2, F, 8), stream=0), INVALID),
    ("describe", lambda: PV.describe(nfr()), _host()),
    ("describe one channel, no axis", lambda: PV1.describe(nfr(None), 2, 5), _host()),
    ("describe three channels", lambda: PV.describe(nfr(3)), FRAMES_MSG),
    # ---- trace -------------------------------------------------------------------------------------------------------------
    ("trace_device number", lambda: PV.trace_device(fr(), fr(), 2, stream=0), NO_DEVICE),
    ("trace_device tensor", lambda: PV.trace_device(fr(), fr(), per(), 2, 5, residual=True, stream=0), NO_DEVICE),
    ("trace_device bins_out", lambda: PV.trace_device(fr(), fr(), 2, bins_out=z(2, F, 4, dt=i32), stream=0), NO_DEVICE),
    ("trace_device one channel, no axis", lambda: PV1.trace_device(fr(None), fr(None), 2, bins_out=z(F, 4, dt=i32),
                                                                   stream=0), NO_DEVICE),
    ("trace_device float64 out", lambda: PV.trace_device(fr(), fr(dt=f64), 2, stream=0), INVALID),
    ("trace_device other F", lambda: PV.trace_device(fr(f=F + 1), fr(), 2, stream=0), INVALID),
    ("trace_device n longer", lambda: PV.trace_device(fr(), fr(), per(F + 1), stream=0), INVALID),
    ("trace_device n float64", lambda: PV.trace_device(fr(), fr(), per(dt=f64), stream=0), INVALID),
    ("trace_device bins_out int64", lambda: PV.trace_device(fr(), fr(), 2, bins_out=z(2, F, 4, dt=i64), stream=0), INVALID),
    ("trace_device bins_out float32", lambda: PV.trace_device(fr(), fr(), 2, bins_out=z(2, F, 4), stream=0), INVALID),
    ("trace_device bins_out one axis", lambda: PV.trace_device(fr(), fr(), 2, bins_out=z(4, dt=i32), stream=0), INVALID),
    ("trace_device bins_out four axes", lambda: PV.trace_device(fr(), fr(), 2, bins_out=z(1, 2, F, 4, dt=i32), stream=0),
     INVALID),
    ("trace_device bins_out without axis, two channels",
     lambda: PV.trace_device(fr(), fr(), 2, bins_out=z(F, 4, dt=i32), stream=0), INVALID),
    ("trace_device bins_out of other F", lambda: PV.trace_device(fr(), fr(), 2, bins_out=z(2, F + 1, 4, dt=i32), stream=0),
     INVALID),
    ("trace_device bins_out of no columns", lambda: PV.trace_device(fr(), fr(), 2, bins_out=z(2, F, 0, dt=i32), stream=0),
     INVALID),
    ("trace_device bins_out strided", lambda: PV.trace_device(fr(), fr(), 2, bins_out=strided(z(2, F, 4, dt=i32)),
                                                                stream=0), INVALID),
    ("trace_device bins_out on another device",
     lambda: PV.trace_device(fr(), fr(), 2, bins_out=torch.zeros((2, F, 4), dtype=i32, device="meta"), stream=0), INVALID),
    ("trace", lambda: PV.trace(nfr(), 2), _host()),
    ("trace with a list", lambda: PV.trace(nfr(), np.full(F, 2.0), residual=True, list_n=4), _host()),
    ("trace no axis, two channels", lambda: PV.trace(nfr(None), 2), FRAMES_MSG),
    # ---- adsyn -------------------------------------------------------------------------------------------------------------
    ("adsyn_device", lambda: PV.adsyn_device(fr(), z(2, L), stream=0), NO_DEVICE),
    ("adsyn_device fmod number", lambda: PV.adsyn_device(fr(), z(2, L), 1.5, 1, 4, 2, 0.5, stream=0), NO_DEVICE),
    ("adsyn_device fmod tensor", lambda: PV.adsyn_device(fr(), z(2, L), per(), stream=0), NO_DEVICE),
    ("adsyn_device longer rows", lambda: PV.adsyn_device(fr(), z(2, L + 7), stream=0), NO_DEVICE),
    ("adsyn_device padded rows", lambda: PV.adsyn_device(fr(), padded(z(2, L)), stream=0), NO_DEVICE),
    ("adsyn_device one channel, one row", lambda: PV1.adsyn_device(fr(None), z(L), stream=0), NO_DEVICE),
    ("adsyn_device one channel, (1, n)", lambda: PV1.adsyn_device(fr(1), z(1, L), stream=0), NO_DEVICE),
    ("adsyn_device one sample short", lambda: PV.adsyn_device(fr(), z(2, L - 1), stream=0), INVALID),
    ("adsyn_device float64 out", lambda: PV.adsyn_device(fr(), z(2, L, dt=f64), stream=0), INVALID),
    ("adsyn_device three rows", lambda: PV.adsyn_device(fr(), z(3, L), stream=0), INVALID),
    ("adsyn_device one row, two channels", lambda: PV.adsyn_device(fr(), z(L), stream=0), INVALID),
    ("adsyn_device float64 frames", lambda: PV.adsyn_device(fr(dt=f64), z(2, L), stream=0), INVALID),
    ("adsyn_device fmod longer", lambda: PV.adsyn_device(fr(), z(2, L), per(F + 1), stream=0), INVALID),
    ("adsyn_device fmod float64", lambda: PV.adsyn_device(fr(), z(2, L), per(dt=f64), stream=0), INVALID),
    ("adsyn_device strided samples", lambda: PV.adsyn_device(fr(), strided(z(2, L)), stream=0),
     (ValueError, ROWS_MSG % "out")),
    ("adsyn_device three axes", lambda: PV.adsyn_device(fr(), z(1, 2, L), stream=0), (ValueError, ROWS_MSG % "out")),
    ("adsyn", lambda: PV.adsyn(nfr()), _host()),
    ("adsyn fmod", lambda: PV1.adsyn(nfr(None), np.ones(F), 1, 4, 2, 0.5), _host()),
    ("adsyn three channels", lambda: PV.adsyn(nfr(3)), FRAMES_MSG),
    # ---- demix, delay, bands, pitch, tanal: one accepted row per form (their refusals: the families' own *_cpu.py files;
    # ---- the delay and the bank are not set up, which the library says before it says that there is no device)
    ("demix_device", lambda: PV.demix_device(fr(), fr(), fr(), (0.0, 3.0), 5, stream=0), NO_DEVICE),
    ("demix", lambda: PV.demix(nfr(), nfr(), 0.0, 3.0, 5), _host()),
    ("delay_device", lambda: PV.delay_device(fr(), fr(), 1, stream=0), INVALID_OPERATION),
    ("delay", lambda: PV.delay(nfr(), 1), _host(INVALID_OPERATION)),
    ("bands_device", lambda: PV.bands_device(fr(), z(2, F, 1), stream=0), INVALID_OPERATION),
    ("bands", lambda: PV.bands(nfr()), _host(INVALID_OPERATION)),
    ("pitch_device", lambda: PV.pitch_device(fr(), z(2, F, 4), 0.1, 50.0, 1000.0, stream=0), NO_DEVICE),
    ("pitch", lambda: PV.pitch(nfr(), 0.1, 50.0, 1000.0), _host()),
    ("tanal_device", lambda: PV.tanal_device(z(2, 100), z(SIZE), z(F, dt=i32), fr(), stream=0), NO_DEVICE),
    ("tanal", lambda: PV.tanal(np.zeros((2, 100), np.float32), np.ones(SIZE, np.float32), np.zeros(F, np.int32)), _host()),
    # ---- Stft --------------------------------------------------------------------------------------------------------------
    ("Stft.analyze_device", lambda: ST.analyze_device(z(2, NS), sp(), stream=0), NO_DEVICE),
    ("Stft.analyze_device one row", lambda: ST.analyze_device(z(NS), sp(1), stream=0), NO_DEVICE),
    ("Stft.analyze_device padded rows", lambda: ST.analyze_device(padded(z(2, NS)), sp(), stream=0), NO_DEVICE),
    ("Stft.analyze_device float64 (not looked at)", lambda: ST.analyze_device(z(2, NS, dt=f64), sp(), stream=0), NO_DEVICE),
    ("Stft.analyze_device three axes", lambda: ST.analyze_device(z(1, 2, NS), sp(), stream=0),
     (ValueError, ROWS_MSG % "signal")),
    ("Stft.analyze_device strided samples", lambda: ST.analyze_device(strided(z(2, NS)), sp(), stream=0),
     (ValueError, ROWS_MSG % "signal")),
    ("Stft.analyze_device strided spectra", lambda: ST.analyze_device(z(2, NS), strided(sp()), stream=0),
     (ValueError, "spectra tensor must be contiguous")),
    ("Stft.synthesize_device", lambda: STI.synthesize_device(sp(), z(2, NS), normalize=True, stream=0), NO_DEVICE),
    ("Stft.synthesize_device one channel", lambda: STI.synthesize_device(sp(None), z(NS), stream=0), NO_DEVICE),
    ("Stft.synthesize_device padded rows", lambda: STI.synthesize_device(sp(), padded(z(2, NS)), stream=0), NO_DEVICE),
    ("Stft.synthesize_device three rows", lambda: STI.synthesize_device(sp(), z(3, NS), stream=0),
     (ValueError, "out has 3 rows for 2 channels")),
    ("Stft.synthesize_device one row, two channels", lambda: STI.synthesize_device(sp(), z(NS), stream=0),
     (ValueError, "out has 1 rows for 2 channels")),
    ("Stft.synthesize_device strided spectra", lambda: STI.synthesize_device(strided(sp()), z(2, NS), stream=0),
     (ValueError, "spectra tensor must be contiguous")),
    ("Stft.synthesize_device strided samples", lambda: STI.synthesize_device(sp(), strided(z(2, NS)), stream=0),
     (ValueError, ROWS_MSG % "signal")),
    ("Stft.analyze", lambda: ST.analyze(np.zeros((2, NS), np.float32)), _host()),
    ("Stft.analyze one row", lambda: ST.analyze(np.zeros(NS)), _host()),
    ("Stft.synthesize", lambda: STI.synthesize(np.zeros((2, F, M), np.complex64), normalize=True), _host()),
    ("Stft.synthesize one channel", lambda: STI.synthesize(np.zeros((F, M), np.complex64)), _host()),
    ("Stft.synthesize one bin more", lambda: STI.synthesize(np.zeros((2, F, M + 1), np.complex64)),
     (ValueError, "spectra must be (channels, F, %d)" % M)),
    ("Stft.synthesize one axis", lambda: STI.synthesize(np.zeros(M, np.complex64)),
     (ValueError, "spectra must be (channels, F, %d)" % M)),
    ("Stft window", lambda: fa.Stft(0, SIZE, HOP, window=np.ones(SIZE)).get_error(), NO_DEVICE),
    ("Stft window as a tensor", lambda: fa.Stft(0, SIZE, HOP, window=torch.ones(SIZE, dtype=f64)).get_error(), NO_DEVICE),
    ("Stft window one short", lambda: fa.Stft(0, SIZE, HOP, window=np.ones(SIZE - 1)),
     (ValueError, "window must hold size = %d floats" % SIZE)),
    ("Stft window one long", lambda: fa.Stft(0, SIZE, HOP, window=torch.ones(SIZE + 1), fwd=False),
     (ValueError, "window must hold size = %d floats" % SIZE)),
]

# ---- process_blocks_device: the rows of test_gpu_python_args.py, on both block convolutions ---------------------------
for _name, _obj, _blk in (("Clpconv", PC, PTS), ("Cldconv", DC, VSIZE)):
    _n = NB * _blk
    _bad = ValueError, BLOCK_MSG % "channels"
    ROWS += [(_name + ".process_blocks_device " + what, call, outcome) for what, call, outcome in [
        ("good", lambda o=_obj, n=_n: o.process_blocks_device(z(2, n), z(2, n), stream=0), NO_DEVICE),
        ("two inputs, padded", lambda o=_obj, n=_n: o.process_blocks_device(padded(z(2, n)), padded(z(2, n)),
                                                                          padded(z(2, n)), stream=0), NO_DEVICE),
        ("1d_two_channels", lambda o=_obj, n=_n: o.process_blocks_device(z(n), z(n), stream=0), _bad),
        ("1d_out_two_channels", lambda o=_obj, n=_n: o.process_blocks_device(z(n), z(2, n), stream=0), _bad),
        ("float64_in", lambda o=_obj, n=_n: o.process_blocks_device(z(2, n), z(2, n, dt=f64), stream=0), _bad),
        ("float64_out", lambda o=_obj, n=_n: o.process_blocks_device(z(2, n, dt=f64), z(2, n), stream=0), _bad),
        ("float64_in2", lambda o=_obj, n=_n: o.process_blocks_device(z(2, n), z(2, n), z(2, n, dt=f64), stream=0), _bad),
        ("strided_samples", lambda o=_obj, n=_n: o.process_blocks_device(z(2, n), strided(z(2, n)), stream=0), _bad),
        ("three_rows", lambda o=_obj, n=_n: o.process_blocks_device(z(2, n), z(3, n), stream=0), _bad),
        ("3d", lambda o=_obj, n=_n: o.process_blocks_device(z(2, n), z(1, 2, n), stream=0), _bad),
        ("length_not_blocks", lambda o=_obj, n=_n + _blk // 2: o.process_blocks_device(z(2, n), z(2, n), stream=0), INVALID),
        ("out_shorter", lambda o=_obj, n=_n, b=_blk: o.process_blocks_device(z(2, n - b), z(2, n), stream=0), INVALID),
        ("in2_shorter", lambda o=_obj, n=_n, b=_blk: o.process_blocks_device(z(2, n), z(2, n), z(2, n - b), stream=0),
         INVALID),
        ("in2_other_stride", lambda o=_obj, n=_n: o.process_blocks_device(z(2, n), z(2, n), padded(z(2, n)), stream=0),
         INVALID),
    ]]

ROWS += [
    # ---- push_ir_device: what the two checks share, then where they differ ---------------------------------------------
    ("Clpconv.push_ir_device", lambda: PC.push_ir_device(z(2, CVS), stream=0), NO_DEVICE),
    ("Cldconv.push_ir_device", lambda: DC.push_ir_device(z(2, IRSIZE), stream=0), NO_DEVICE),
    ("Clpconv.push_ir_device one row", lambda: PC1.push_ir_device(z(CVS), stream=0), NO_DEVICE),
    ("Clpconv.push_ir_device float64", lambda: PC.push_ir_device(z(2, CVS, dt=f64), stream=0), INVALID),
    ("Cldconv.push_ir_device float64", lambda: DC.push_ir_device(z(2, IRSIZE, dt=f64), stream=0), INVALID),
    ("Clpconv.push_ir_device three rows", lambda: PC.push_ir_device(z(3, CVS), stream=0), INVALID),
    ("Cldconv.push_ir_device three rows", lambda: DC.push_ir_device(z(3, IRSIZE), stream=0), INVALID),
    ("Clpconv.push_ir_device one row, two channels", lambda: PC.push_ir_device(z(CVS), stream=0), INVALID),
    ("Cldconv.push_ir_device one row, two channels", lambda: DC.push_ir_device(z(IRSIZE), stream=0), INVALID),
    ("Clpconv.push_ir_device three axes", lambda: PC.push_ir_device(z(1, 2, CVS), stream=0), INVALID),
    ("Cldconv.push_ir_device three axes", lambda: DC.push_ir_device(z(1, 2, IRSIZE), stream=0), INVALID),
    ("Clpconv.push_ir_device strided samples", lambda: PC.push_ir_device(strided(z(2, CVS)), stream=0), INVALID),
    ("Cldconv.push_ir_device strided samples", lambda: DC.push_ir_device(strided(z(2, IRSIZE)), stream=0), INVALID),
    ("Clpconv.push_ir_device short rows", lambda: PC.push_ir_device(z(2, CVS - 1), stream=0), INVALID),
    ("Cldconv.push_ir_device short rows", lambda: DC.push_ir_device(z(2, IRSIZE - 1), stream=0), INVALID),
    ("Clpconv.push_ir_device overlapping rows", lambda: PC.push_ir_device(
        torch.as_strided(z(2 * CVS), (2, CVS), (CVS - 1, 1)), stream=0), INVALID),
    ("Cldconv.push_ir_device overlapping rows", lambda: DC.push_ir_device(
        torch.as_strided(z(2 * IRSIZE), (2, IRSIZE), (IRSIZE - 1, 1)), stream=0), INVALID),
    # Clpconv wants the whole tensor contiguous (after its own checks), Cldconv takes the row stride
    ("Clpconv.push_ir_device padded rows", lambda: PC.push_ir_device(padded(z(2, CVS)), stream=0),
     (ValueError, CONTIG_MSG)),
    ("Cldconv.push_ir_device padded rows", lambda: DC.push_ir_device(padded(z(2, IRSIZE)), stream=0), NO_DEVICE),
    ("Clpconv.push_ir_device padded float64 rows", lambda: PC.push_ir_device(padded(z(2, CVS, dt=f64)), stream=0), INVALID),
    # rows of one sample: Clpconv looks at their stride(1) (and so never at the tensor's contiguity), Cldconv does not
    ("Clpconv.push_ir_device one-sample rows, stride(1) == 2", lambda: PC0.push_ir_device(z(2, 2)[:, ::2], stream=0),
     INVALID),
    ("Clpconv.push_ir_device padded rows, no partitions", lambda: PC0.push_ir_device(padded(z(2, 2)), stream=0),
     (ValueError, CONTIG_MSG)),
    ("Cldconv.push_ir_device one-sample rows, stride(1) == 2", lambda: DC1.push_ir_device(z(2, 2)[:, ::2], stream=0),
     NO_DEVICE),
    ("Cldconv.push_ir_device two-sample rows, stride(1) == 2", lambda: DC1.push_ir_device(z(2, 4)[:, ::2], stream=0),
     INVALID),
    # ---- the single-block device calls --------------------------------------------------------------------------------------
    ("Clpconv.process_device", lambda: PC.process_device(z(2, PTS), z(2, PTS), z(2, PTS), stream=0), NO_DEVICE),
    ("Clpconv.process_device strided", lambda: PC.process_device(z(2, PTS), strided(z(2, PTS)), stream=0),
     (ValueError, CONTIG_MSG)),
    ("Cldconv.process_device", lambda: DC.process_device(z(2, VSIZE), z(2, VSIZE), z(2, VSIZE), stream=0), NO_DEVICE),
    ("Cldconv.process_device float64", lambda: DC.process_device(z(2, VSIZE), z(2, VSIZE, dt=f64), stream=0), INVALID),
    ("Cldconv.process_device float64 in2", lambda: DC.process_device(z(2, VSIZE), z(2, VSIZE), z(2, VSIZE, dt=f64),
                                                                     stream=0), INVALID),
    ("Cldconv.process_device one sample more", lambda: DC.process_device(z(2, VSIZE + 1), z(2, VSIZE), stream=0), INVALID),
    ("Cldconv.process_device strided", lambda: DC.process_device(strided(z(2, VSIZE)), z(2, VSIZE), stream=0), INVALID),
    # ---- PconvMatrix ----------------------------------------------------------------------------------------------------------
    ("PconvMatrix.process_device", lambda: MX.process_device(z(MO, NB * PTS), z(MI, NB * PTS), stream=0), NO_DEVICE),
    ("PconvMatrix.process_device 1d_in", lambda: MX.process_device(z(MO, NB * PTS), z(NB * PTS), stream=0),
     (ValueError, BLOCK_MSG % MI)),
    ("PconvMatrix.process_device 1d_out", lambda: MX.process_device(z(NB * PTS), z(MI, NB * PTS), stream=0),
     (ValueError, BLOCK_MSG % MO)),
    ("PconvMatrix.process_device float64_in", lambda: MX.process_device(z(MO, NB * PTS), z(MI, NB * PTS, dt=f64), stream=0),
     (ValueError, BLOCK_MSG % MI)),
    ("PconvMatrix.process_device float64_out", lambda: MX.process_device(z(MO, NB * PTS, dt=f64), z(MI, NB * PTS), stream=0),
     (ValueError, BLOCK_MSG % MO)),
    ("PconvMatrix.process_device strided_samples", lambda: MX.process_device(z(MO, NB * PTS), strided(z(MI, NB * PTS)),
                                                                             stream=0), (ValueError, BLOCK_MSG % MI)),
    ("PconvMatrix.process_device rows_swapped", lambda: MX.process_device(z(MI, NB * PTS), z(MO, NB * PTS), stream=0),
     (ValueError, BLOCK_MSG % MO)),
    ("PconvMatrix.process_device length_not_blocks", lambda: MX.process_device(z(MO, NB * PTS + 5), z(MI, NB * PTS + 5),
                                                                               stream=0), INVALID),
    ("PconvMatrix.process_device out_shorter", lambda: MX.process_device(z(MO, PTS), z(MI, NB * PTS), stream=0), INVALID),
    ("PconvMatrix.push_ir_device", lambda: MX.push_ir_device(z(MO, MI, CVS), stream=0), NO_DEVICE),
    ("PconvMatrix.push_ir_device float64", lambda: MX.push_ir_device(z(MO, MI, CVS, dt=f64), stream=0), INVALID),
    ("PconvMatrix.push_ir_device two axes", lambda: MX.push_ir_device(z(MI, CVS), stream=0), INVALID),
    ("PconvMatrix.push_ir_device rows swapped", lambda: MX.push_ir_device(z(MI, MO, CVS), stream=0), INVALID),
    ("PconvMatrix.push_ir_device uneven rows", lambda: MX.push_ir_device(
        torch.as_strided(z(MO * (MI * CVS + 44)), (MO, MI, CVS), (MI * CVS + 44, CVS, 1)), stream=0), INVALID),
    ("PconvMatrix.push_ir_fade_device uneven rows", lambda: MX.push_ir_fade_device(
        torch.as_strided(z(MO * (MI * CVS + 44)), (MO, MI, CVS), (MI * CVS + 44, CVS, 1)), 2, stream=0), INVALID),
]


def test_row_names_are_unique():
    names = [r[0] for r in ROWS]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("what,call,outcome", ROWS, ids=[r[0] for r in ROWS])
def test_row(what, call, outcome):
    assert _outcome(call) == outcome


def test_every_device_method_and_twin_has_an_accepted_row():
    """every public *_device method of Pvoc and Stft, and the blocking form of the same name, in a row that reaches
    the library"""
    reached = {r[0].split()[0] for r in ROWS if r[2] in (NO_DEVICE, INVALID_OPERATION, _host(), _host(INVALID_OPERATION))}
    for cls, prefix in ((fa.Pvoc, ""), (fa.Stft, "Stft.")):
        dev = [n for n in dir(cls) if n.endswith("_device") and not n.startswith("_")]   # Pvoc's come from its bases
        assert len(dev) == (27 if cls is fa.Pvoc else 2)
        for n in dev:
            assert prefix + n in reached and prefix + n[:-len("_device")] in reached, n
