"""The cepstral envelope of clfa_pvoc on the device (pvoc_env.hpp), bin by bin, in both kernels that hold it
(k_pvoc_formant of pvoc_ops.hip, k_pvoc_vocode of pvoc_pair.hip) at all nine sizes 64 .. 16384: eighteen kernels, each
with its own LdsGeom (lanes per transform, frames per workgroup, pass chain, tables in LDS or from cache).

The inputs are the probe frames of tests/pvoc_env_probe.py: impulse frames (ones and one bin of 256, 1 / 256 or 0, at
the ends, around the lane count of the pair loop, around M / 2 and below M) between constant frames of 2^40 and 2^-40,
in enough frames for three full groups of a workgroup and a ragged one, the groups straddling the channel boundary.
coefs runs through coefs_for(size): 1, 2, around the lane count, around M / 2 (where the partner j = M / 2 of the
special pair switches between kept and zeroed) and M - 2, M - 1.  tests/test_pvoc_ops_cpu.py shows that an impulse moved
by one bin changes log E by more than 1 once coefs >= M / 2 - 1; the low coefs pin the smooth part only.

What is compared is |log(out amp) - log(truth amp)| in float64 at EVERY bin of every frame, the truth being the float64
model with env64_fft.  Bins the definition makes exactly 0, copies, empty bins and every freq are held to bits instead.
Every launch goes into a guarded output, and runs twice: on a free object and on one created with at most 2 workgroups
per launch, bit-identical.

The bound of a case (one size, one coefs, one call) is MARGIN_BIN x max(E32, ulp32(Lmax)): E32 the float32 model's worst
per-bin log error against the same truth (env32 / op32 / pair32: the reference's error, never the device's), ulp32(Lmax)
one float32 ulp at the largest |log amp| of the case's inputs (3.8e-6 at the floor 1e-20): the rounding of logf's result
alone, which keeps the bound from collapsing where the model's error is exactly 0.

MARGIN_BIN.  The rule: the smallest of 2, 4, 8 that clears the largest ratio measured over every case of this file by a
factor 1.5.  Every case prints its ratio (`PVOCENV ...` lines, pytest -s); profiles/pvoc_env.txt holds a device run's.
MEASURED over every case of this file on an MI355X (440 cases: nine sizes, every coefs_for value, five calls): the
ratios lie between 0.03 and 1.61.  The largest, 1.61, is size 256, coefs 127 (M - 1), formant scale: 9.13e-6 at channel
0, frame 22, bin 64 (the impulse frame with the floor at bin M / 2) against a model error of 5.65e-6; by call the
largest are envelope A 1.36, envelope B 1.44, both 1.33, formant shift 1.27, formant scale 1.61.  Where no frame's
error reaches an ulp of 46 (the low coefs) the bound is that ulp and the ratios are 0.03 .. 0.2.  1.61 x 1.5 = 2.4 rules
out 2, so MARGIN_BIN is 4.  No case came near 8 / 1.5: nothing about the kernels to explain.

A whole size (all its coefs, both objects) takes well under a second on the device, so size 16384 runs every coefs
value in every call like the other sizes.
"""
import numpy as np
import pytest

from tests import pvoc_env_probe as ep
from tests import pvoc_ops_model as om
from tests import pvoc_pair_model as pp
from tests.gpu_guard import bits, dev, run
from tests.pvoc_inputs import SR, make_pvoc

pytestmark = pytest.mark.gpu
MARGIN_BIN = 4.0        # see the docstring: the largest ratio measured is 1.61
GAIN = 0.7
f32 = np.float32
RATIO = {"max": 0.0, "case": ""}


def make(size, channels, grid_max=None, monkeypatch=None):
    return make_pvoc(size, size // 4, channels, env={"CLFA_PVOC_OPS_GRID_MAX": grid_max}, monkeypatch=monkeypatch)


def both(size, monkeypatch):
    """(the probe, a free object, one whose launches have at most 2 workgroups)"""
    fr = ep.probe_for(size)
    return fr, make(size, fr.shape[0]), make(size, fr.shape[0], grid_max=2, monkeypatch=monkeypatch)


def run_both(pvs, call, shape, what):
    """the call on the free and on the capped object: one result, bit-identical"""
    free, capped = (run(lambda o: call(pv, o), shape) for pv in pvs)
    assert np.array_equal(bits(free), bits(capped)), what + ": the grid cap changed the result"
    return free


def alternately(F, even, odd):
    return np.where(np.arange(F) % 2 == 0, f32(even), f32(odd)).astype(f32)


def ones_like(fr):
    """all-ones amps with the freqs of `fr` reversed (arbitrary, and not the probe's own in any slot)"""
    o = np.array(fr[::-1, ::-1])
    o[..., 0] = 1
    return o


def reversed_frames(fr):
    """the frames of `fr` in reversed order of the flat index"""
    C, F = fr.shape[:2]
    return np.ascontiguousarray(fr.reshape((C * F,) + fr.shape[2:])[::-1]).reshape(fr.shape)


def worst(amp, truth, where):
    """(the largest |log amp - log truth| over the bins `where`, its index): float64; a NaN, a zero or a negative amp
    gives a NaN or an Inf, which no bound admits"""
    with np.errstate(all="ignore"):
        e = np.abs(np.log(np.asarray(amp, np.float64)) - np.log(truth))
    e = np.where(where, e, 0.0)
    e = np.where(np.isnan(e), np.inf, e)
    at = tuple(int(i) for i in np.unravel_index(int(np.argmax(e)), e.shape))
    return float(e[at]), at


def ulp32_of_log(*amps):
    """one float32 ulp at the largest |log amp| of the inputs, the floor applied as the definition applies it"""
    lmax = max(float(np.abs(np.log(np.fmax(a, om.FLOOR).astype(np.float64))).max()) for a in amps)
    return float(np.spacing(f32(lmax)))


def judge(what, got, m32, truth, where, ulp):
    """got and m32 against truth at the bins `where`; where the truth is exactly 0 the device's amp is exactly 0"""
    zero = where & (truth == 0)
    assert (got[zero] == 0).all(), what + ": a bin the definition makes 0"
    where = where & ~zero
    assert np.isfinite(truth[where]).all() and (truth[where] > 0).all(), what + ": the inputs overflow the model"
    (e_dev, at), (e_f32, _) = worst(got, truth, where), worst(m32, truth, where)
    bound = max(e_f32, ulp)
    ratio = e_dev / bound
    if ratio > RATIO["max"]:
        RATIO["max"], RATIO["case"] = ratio, what
    print("PVOCENV %s: worst |dlog| %.3g at %s (float32 model %.3g, ulp %.3g, ratio %.2f; largest so far %.2f, %s)"
          % (what, e_dev, at, e_f32, ulp, ratio, RATIO["max"], RATIO["case"]))
    assert e_dev <= MARGIN_BIN * bound, "%s: %.3g at %s against %.3g" % (what, e_dev, at, bound)


_ENV64 = {}


def env64_of(size, coefs):
    """env64_fft of the probe's amps (read-only, shared by the cases of a size)"""
    if (size, coefs) not in _ENV64:
        e = om.env64_fft(ep.probe_for(size)[..., 0], coefs)
        e.setflags(write=False)
        _ENV64[(size, coefs)] = e
    return _ENV64[(size, coefs)]


def vocode64(a, b, ea, eb, depth, gain):
    """pvoc_pair_model.vocode64_amps with the envelopes given (env64_fft in place of env64)"""
    F = a.shape[1]
    d = pp.clamp(np.broadcast_to(np.asarray(depth, f32), (F,)).reshape(1, F, 1)).astype(np.float64)
    with np.errstate(all="ignore"):
        return float(f32(gain)) * (b[..., 0].astype(np.float64) * ((1.0 - d) + d * (ea / eb)))


def check_vocode(pvs, a, b, ea, eb, depth, gain, coefs, what):
    size = pvs[0].size
    da, db = dev(a), dev(b)
    dd = dev(depth) if isinstance(depth, np.ndarray) else depth
    got = run_both(pvs, lambda pv, o: pv.vocode_device(da, db, o, dd, gain, coefs=coefs), a.shape, what)
    assert np.array_equal(bits(got[..., 1]), bits(b[..., 1])), what + ": freq"
    m32 = pp.pair32(pp.VOCODE, a, b, depth, gain, size, SR, coefs)
    truth = vocode64(a, b, ea, eb, depth, gain)
    judge(what, got[..., 0], m32[..., 0], truth, np.ones(truth.shape, bool), ulp32_of_log(a[..., 0], b[..., 0]))
    return got


@pytest.mark.parametrize("size", ep.SIZES)
def test_kernel_names(size):
    pv = make(size, 2)
    assert pv.ops_kernel_name("shift", True) == "k_pvoc_formant" and pv.ops_kernel_name("scale", True) == "k_pvoc_formant"
    assert pv.pair_kernel_name("vocode") == "k_pvoc_vocode"


@pytest.mark.parametrize("size", ep.SIZES)
def test_envelope_a_alone(size, monkeypatch):
    """b's amps are 1, so envB is exactly 1 and the output amp is envA[k] itself"""
    fr, *pvs = both(size, monkeypatch)
    ones = ones_like(fr)
    for coefs in ep.coefs_for(size):
        e = env64_of(size, coefs)
        check_vocode(pvs, fr, ones, e, np.ones_like(e), 1.0, 1.0, coefs, "size %d coefs %d envelope A" % (size, coefs))


@pytest.mark.parametrize("size", ep.SIZES)
def test_envelope_b_alone(size, monkeypatch):
    """the second pvoc_envelope call of k_pvoc_vocode, in the exchange buffer the a-frames have just left: b / envB
    (exactly 0 where b's amp is 0)"""
    fr, *pvs = both(size, monkeypatch)
    ones = ones_like(fr)
    for coefs in ep.coefs_for(size):
        e = env64_of(size, coefs)
        check_vocode(pvs, ones, fr, np.ones_like(e), e, 1.0, 1.0, coefs, "size %d coefs %d envelope B" % (size, coefs))


@pytest.mark.parametrize("size", ep.SIZES)
def test_both_envelopes(size, monkeypatch):
    """a = the probe's frames in reversed order, b = the probe: other contents in every slot (but the middle one of an
    odd count); depth 0.5 and 1 alternately"""
    fr, *pvs = both(size, monkeypatch)
    a = reversed_frames(fr)
    depth = alternately(fr.shape[1], 0.5, 1.0)
    for coefs in ep.coefs_for(size):
        e = env64_of(size, coefs)
        check_vocode(pvs, a, fr, reversed_frames(e), e, depth, GAIN, coefs, "size %d coefs %d both envelopes" % (size, coefs))


def formant_calls(size, F):
    """(name, op, the per-frame values, the model's keywords, the device call).  A scale of 1 would map every bin to
    itself and cancel the envelope"""
    hz, s = alternately(F, 3 * SR / size, -2 * SR / size), alternately(F, 2.0, 0.5)
    return [("shift", hz, lambda pv, d, o, coefs: pv.shift_device(d, o, dev(hz), lowest_bin=1, keepform=True, gain=1.0, coefs=coefs)),
            ("scale", s, lambda pv, d, o, coefs: pv.scale_device(d, o, dev(s), keepform=True, gain=1.0, coefs=coefs))]


@pytest.mark.parametrize("size", ep.SIZES)
def test_formant(size, monkeypatch):
    """bins with a source: amp / env[source] * env[bin] in log against the float64 model; copied and empty bins and every
    freq: the float32 model's bits"""
    fr, *pvs = both(size, monkeypatch)
    C, F, B, _ = fr.shape
    M = size // 2
    d = dev(fr)
    ulp = ulp32_of_log(fr[..., 0])
    for op, par, call in formant_calls(size, F):
        srcs = om.maps(op, M, par, 1, om.bpf_of(size, SR))
        moved = np.broadcast_to(np.stack(srcs) >= 0, (C, F, B))
        assert moved.sum() > C * F * M // 4
        for coefs in ep.coefs_for(size):
            what = "size %d coefs %d formant %s" % (size, coefs, op)
            got = run_both(pvs, lambda pv, o: call(pv, d, o, coefs), fr.shape, what)
            m32 = om.op32(op, fr, par, size, SR, lowest=1, keepform=True, gain=1.0, coefs=coefs)
            assert np.array_equal(bits(got[..., 1]), bits(m32[..., 1])), what + ": freq"
            assert np.array_equal(bits(got[..., 0])[~moved], bits(m32[..., 0])[~moved]), what + ": copied and empty bins"
            truth = om._apply(fr, srcs, par, op, 1.0, om.cf_of(size, SR), env64_of(size, coefs), np.float64)[0]
            judge(what, got[..., 0], m32[..., 0], truth, moved, ulp)


@pytest.mark.parametrize("size", ep.SIZES)
def test_exact_after_a_loud_launch(size, monkeypatch):
    """all-ones amps: log 1 = 0, the transforms of zeros are zeros, exp 0 = 1, so the vocoder gives the float32 model's
    bits and a keepform move gives 1.0 at every moved bin — on objects that have just run the probe, whose 2^40 and
    1e-20 would show if a slot kept anything"""
    fr, *pvs = both(size, monkeypatch)
    C, F, B, _ = fr.shape
    M = size // 2
    x, y = ones_like(fr), ones_like(reversed_frames(fr))
    dfr, dx, dy = dev(fr), dev(x), dev(y)
    depth = alternately(F, 0.5, 1.0)
    ddepth = dev(depth)
    for coefs in ep.coefs_for(size):
        what = "size %d coefs %d exact" % (size, coefs)
        run_both(pvs, lambda pv, o: pv.vocode_device(dfr, dfr, o, 1.0, 1.0, coefs=coefs), fr.shape, what + ": loud")
        got = run_both(pvs, lambda pv, o: pv.vocode_device(dx, dy, o, ddepth, GAIN, coefs=coefs), fr.shape, what)
        assert np.array_equal(bits(got), bits(pp.pair32(pp.VOCODE, x, y, depth, GAIN, size, SR, coefs))), what + ": vocode"
        for op, par, call in formant_calls(size, F):
            moved = np.broadcast_to(np.stack(om.maps(op, M, par, 1, om.bpf_of(size, SR))) >= 0, (C, F, B))
            run_both(pvs, lambda pv, o: call(pv, dfr, o, coefs), fr.shape, what + ": loud " + op)
            got = run_both(pvs, lambda pv, o: call(pv, dx, o, coefs), fr.shape, what + " " + op)
            assert (bits(got[..., 0])[moved] == bits(f32(1))).all(), "%s %s: a moved bin is not 1.0" % (what, op)
            assert np.array_equal(bits(got), bits(om.op32(op, x, par, size, SR, lowest=1, keepform=True, coefs=coefs))), what + " " + op
