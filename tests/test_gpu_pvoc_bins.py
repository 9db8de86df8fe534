"""The core conversion of clfa_pvoc on the device (pvoc_kernels.hip: k_pvoc_analyze, k_pvoc_sums, k_pvoc_scan,
k_pvoc_walk), bin by bin, at all nine sizes 64 .. 16384 and four hops each: size / 4, size (e[k] = 1), 3 (does not divide
the size) and size / 4 + 1 (odd: k hop mod size takes every residue, so every entry of the e[k] table is a different one).

tests/test_gpu_pvoc.py holds the same kernels to a relative L2 over the whole call, which a loud bin dominates: one bin
wrong by a hundred of its own roundings passes there (tests/test_pvoc_probe_cpu.py, mutant (a)).  Here the inputs are the
ranged probe of tests/pvoc_probe.py — every bin at a level of its own over 80 octaves, a zero frame, a doubled and a
negated one, 69 = scan_chunk() + 5 frames (across the synthesis' chunk, neither a multiple of the analysis' run of 4 nor
one short of one), 2 channels — and EVERY bin of every frame is held to its own scale (pvoc_probe's docstring):
  amp    |amp - |z|| <= bound x 2^-24 |z|;
  dev    the distance on the circle of turns <= bound x s_k, s_k = 2^-24 (1.5 + k hop / size);
  synth  |z - z_truth| <= bound x 2^-24 amp, against float64 on the exact integer phases of the device's own frames;
bound = MARGIN_BIN x max(U32, 1), U32 the float32 model's worst bin on the same inputs against the same truth (the
reference's error, never the device's; capped by tests/test_pvoc_probe_cpu.py).  Besides: every launch goes into a guarded
output with every element written; the analysis whole and cut at frame 5 (run 1 of the first call has one frame; the
second call starts from the carried state) gives the same bits and the same state, which is z of the last frame; the zero
frame and its successor report the bin centres to the bit; the synthesis on a free object and in sub-batches of one chunk
gives the same bits, and its phase state is the model's integer sum.

Two exact probes per size give values, not tolerances: phases that are whole quarter turns (the spectrum is
amp x {1, i, -1, -i} at every element, `==`, over two calls of 2 chunks + 3 frames in all) and a stationary spectrum of
Gaussian integers at hop = size (dev = 0: freq is (float)k (float)(sr / size) and amp the integer modulus, to the bit,
from frame 1 of the first call and from frame 0 of the second).

MARGIN_BIN (tests/pvoc_probe.py).  The rule: the smallest of 2, 4, 8 that clears, by a factor 1.5, the largest ratio
worst / max(U32, 1) over every case of this file on the device.  Every case prints its ratios (`PVOCBIN ...` lines,
pytest -s); profiles/pvoc_bins.txt holds a device run's.
MEASURED over every case of this file on an MI355X (36 cases: nine sizes, four hops), in units of the scales above:
  amp    the ratio is 1.00 in every case: the device's worst bin is the model's worst bin, 1.54 .. 1.94; the largest,
         1.94, is size 16384, hop 16384, channel 0, frame 16, bin 3504;
  dev    0.77 .. 1.00: the device's worst bin 0.90 .. 1.71 against the model's 1.08 .. 1.71.  At the hops size / 4, size
         and size / 4 + 1 the ratio is 1.00 and the worst bin is the model's in every case but one (size 64, hop 17:
         0.98); the largest, 1.71, is size 8192, hop 8192, channel 0, frame 64, bin 2803.  At hop 3 it is 0.77 .. 0.97;
  synth  0.33 .. 0.56: the device's worst bin 1.43 .. 2.91 against the model's 4.03 .. 6.16 (sincospif takes half turns;
         numpy rounds the product with pi first).  The largest ratio, 0.56, is size 8192, hop 2048: 2.68 at channel 0,
         frame 9, bin 2 against 4.80; the largest value, 2.91, is size 16384, hop 3, channel 1, frame 24, bin 4031.
The largest ratio of all is 1.00, and 1.00 x 1.5 = 1.5 stays under 2, so MARGIN_BIN is 2.  No case came near 8 / 1.5:
nothing about the kernels to explain.  Both exact probes hold at every size.

A case (three objects, five guarded launches, the float64 and float32 models of 2 x 69 x (M + 1) bins) takes 0.2 s at
size 16384.
"""
import numpy as np
import pytest
import torch

from tests import pvoc_model as pm
from tests import pvoc_probe as pp
from tests.gpu_guard import bits, dev, flat
from tests.pvoc_inputs import make_pvoc

pytestmark = pytest.mark.gpu
SR = pp.SR
MARGIN_BIN = pp.MARGIN_BIN
C = 2
RATIO = {"max": 0.0, "case": ""}


def make(size, hop, sr=SR, chunks_max=None, monkeypatch=None):
    pv = make_pvoc(size, hop, C, sr, env={"CLFA_PVOC_CHUNKS_MAX": chunks_max}, monkeypatch=monkeypatch)
    assert pv.kernel_name() == "k_pvoc_analyze" and pv.kernel_name(True) == "k_pvoc_walk"
    return pv


def finish(g, what):
    """after the launches into g: the guard bands intact, every element written"""
    torch.cuda.synchronize()
    assert g.intact(), what + ": wrote outside the output"
    assert not g.unwritten(), what + ": an output element was not written"
    return g.data


def analyze(pv, spec, cuts, what):
    """the analysis of spec (C, F, M) on the device in calls cut at `cuts`, each into a guarded output of its own: the
    frames (C, F, M + 1, 2) as a device tensor"""
    F, M = spec.shape[1:]
    parts = []
    for a, b in zip([0] + cuts, cuts + [F]):
        g = flat((C, b - a, M + 1, 2))
        assert pv.analyze_device(spec[:, a:b].contiguous(), g.data) == 0
        parts.append(finish(g, what))
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)


def synthesize(pv, fr, cuts, what):
    """the synthesis of the frames fr (device tensor) in calls cut at `cuts`, guarded: the spectra (C, F, M) complex64, numpy"""
    F, B = fr.shape[1:3]
    parts = []
    for a, b in zip([0] + cuts, cuts + [F]):
        g = flat((C, b - a, B - 1, 2))
        assert pv.synthesize_device(fr[:, a:b].contiguous(), torch.view_as_complex(g.data)) == 0
        parts.append(finish(g, what).cpu().numpy().view(np.complex64)[..., 0])
    return np.concatenate(parts, axis=1)


def note(ratio, what):
    if ratio > RATIO["max"]:
        RATIO["max"], RATIO["case"] = ratio, what


@pytest.mark.parametrize("hopk", ["quarter", "size", "3", "quarter+1"])
@pytest.mark.parametrize("size", pp.SIZES)
def test_every_bin_of_the_ranged_probe(size, hopk, monkeypatch):
    hop = dict(zip(["quarter", "size", "3", "quarter+1"], pp.hops(size)))[hopk]
    what = "size %d hop %d" % (size, hop)
    M = size // 2
    pv, cut = make(size, hop), make(size, hop)
    F = pv.scan_chunk() + 5
    assert F == 69
    P = pp.probe_spectra(size, hop, C, F)
    spec = dev(P)
    prev0 = pm.initial_prev(C, size)

    # analysis: whole, and cut at frame 5 on a second object
    fr_t = analyze(pv, spec, [], what + " analysis")
    fr = fr_t.cpu().numpy()
    fr_cut = analyze(cut, spec, [pp.CUT], what + " analysis cut").cpu().numpy()
    assert np.array_equal(bits(fr), bits(fr_cut)), what + ": the cut at frame %d changed the frames" % pp.CUT
    prev = pv.read_prev()
    assert np.array_equal(bits(prev), bits(cut.read_prev())), what + ": the cut changed prev"
    assert np.array_equal(bits(prev), bits(pm.bins(P[:, -1]))), what + ": prev is not z of the last frame"

    amp64, dev64, _, _ = pm.analyze64(P, prev0, size, hop, SR)
    e_dev = pp.analysis_errors(fr, amp64, dev64, size, hop, SR)
    e_f32 = pp.analysis_errors(pm.analyze32(P, prev0, size, hop, SR), amp64, dev64, size, hop, SR)

    # synthesis of the device's frames: the free object, and one that takes one chunk per sub-batch
    small = make(size, hop, chunks_max=1, monkeypatch=monkeypatch)
    sp = synthesize(pv, fr_t, [], what + " synthesis")
    sp_small = synthesize(small, fr_t, [], what + " synthesis by chunks")
    assert np.array_equal(bits(sp), bits(sp_small)), what + ": sub-batches of one chunk changed the spectra"
    th, new_theta = pm.phases(fr[..., 1], pm.initial_phase(C, size), hop, SR)
    assert np.array_equal(pv.read_phase(), new_theta) and np.array_equal(small.read_phase(), new_theta), what + ": phase state"
    e_dev["synth"] = pp.synth_worst(sp, fr, th)
    e_f32["synth"] = pp.synth_worst(pm.synth32(fr, th), fr, th)

    ratios = {}
    line = "PVOCBIN %s:" % what
    for q in ("amp", "dev", "synth"):
        ratios[q] = e_dev[q][0] / max(e_f32[q][0], 1.0)
        note(ratios[q], "%s %s" % (what, q))
        line += "  %s %.2f at %s (float32 model %.2f, ratio %.2f)" % (q, e_dev[q][0], e_dev[q][1], e_f32[q][0], ratios[q])
    print(line + "  [largest ratio so far %.2f, %s]" % (RATIO["max"], RATIO["case"]))

    for q in ("amp", "dev", "synth"):
        assert e_f32[q][0] <= pp.CAPS[q], "%s: the model's own %s error %.2f widens the bound" % (what, q, e_f32[q][0])
        assert e_dev[q][0] <= pp.bound(MARGIN_BIN, e_f32[q][0]), \
            "%s: %s %.2f at %s against %.2f of the float32 model" % (what, q, e_dev[q][0], e_dev[q][1], e_f32[q][0])
    # the zero frame and its successor: d = (0, 0), the bin centre to the bit; the zero frame is silent
    centre = np.arange(M + 1, dtype=np.float32) * np.float32(SR / size)
    for f in (pp.ZERO_F, pp.ZERO_F + 1):
        assert np.array_equal(bits(fr[:, f, :, 1]), bits(np.broadcast_to(centre, (C, M + 1)))), what + ": frame %d's freq" % f
    assert not bits(fr[:, pp.ZERO_F, :, 0]).any(), what + ": the zero frame's amp"
    assert not sp[:, pp.ZERO_F].any(), what + ": the zero frame's spectrum"


@pytest.mark.parametrize("size", pp.SIZES)
def test_exact_quarter_turns(size, monkeypatch):
    """every phase a multiple of a quarter turn: amp x {1, i, -1, -i} at every element, in two calls (the second starts
    from a non-zero state), on the free object and in sub-batches of one chunk"""
    free = make(size, size // 4, sr=pp.SR_EXACT)
    ch = free.scan_chunk()
    frames, want, state, hop = pp.exact_synth(size, C, 2 * ch + 3)
    assert hop == free.hop
    fr_t = dev(frames)
    for name, pv in (("free", free), ("by chunks", make(size, hop, sr=pp.SR_EXACT, chunks_max=1, monkeypatch=monkeypatch))):
        what = "size %d exact synthesis, %s" % (size, name)
        sp = synthesize(pv, fr_t, [ch + 1], what)
        wrong = np.argwhere(sp != want)           # (-0 equals 0)
        assert wrong.size == 0, "%s: %d elements differ, the first at %s: %s against %s" \
            % (what, len(wrong), tuple(wrong[0]), sp[tuple(wrong[0])], want[tuple(wrong[0])])
        assert np.array_equal(pv.read_phase(), state), what + ": phase state"


@pytest.mark.parametrize("size", pp.SIZES)
def test_exact_stationary_analysis(size):
    """hop = size, Gaussian integers, each frame a small integer times the one before: amp the integer modulus and freq the
    bin centre to the bit, from frame 1 of the first call and from frame 0 of the second (the carried prev, bin by bin)"""
    M, first = size // 2, 6
    P, want_amp, want_freq = pp.exact_analysis(size, C, 13)
    pv = make(size, size)
    spec = dev(P)
    what = "size %d exact analysis" % size
    a = analyze(pv, spec[:, :first].contiguous(), [], what).cpu().numpy()
    assert np.array_equal(bits(pv.read_prev()), bits(pm.bins(P[:, first - 1])))
    b = analyze(pv, spec[:, first:].contiguous(), [], what + ", second call").cpu().numpy()
    fr = np.concatenate([a, b], axis=1)
    wrong = np.argwhere(bits(fr[..., 0]) != bits(want_amp))
    assert wrong.size == 0, "%s: %d amps differ, the first at %s: %r against %r" \
        % (what, len(wrong), tuple(wrong[0]), fr[..., 0][tuple(wrong[0])], want_amp[tuple(wrong[0])])
    wrong = np.argwhere(bits(fr[:, 1:, :, 1]) != bits(np.broadcast_to(want_freq, (C, 12, M + 1))))
    assert wrong.size == 0, "%s: %d freqs differ, the first at (frame - 1) %s" % (what, len(wrong), tuple(wrong[0]))
    assert np.array_equal(bits(pv.read_prev()), bits(pm.bins(P[:, -1])))
