"""tests/pvoc_probe.py without a GPU: the probes are what they claim, the float32 model alone stays under the caps on
every probe the GPU test uses (so the device's bound, MARGIN_BIN x max(U32, 1), is never inflated by the probe), and the
per-bin yardstick bites: mutants of the float32 model's output, fed to the functions tests/test_gpu_pvoc_bins.py feeds
the device's output to, each miss the bound with MARGIN_BIN = 8, the rule's largest value.  Mutant (a) also passes the
aggregate rule of tests/test_gpu_pvoc.py on that file's kind of input: the gap the per-bin tests close."""
import numpy as np
import pytest

from tests import pvoc_model as pm
from tests import pvoc_probe as pp
from tests.pvoc_inputs import two_tones

f32 = np.float32
SR = pp.SR
LARGEST_MARGIN = 8.0


def model_case(size, hop, F=69):
    """the float32 model on the ranged probe, as the GPU test runs the device: everything the yardstick needs"""
    P = pp.probe_spectra(size, hop, 2, F)
    C = P.shape[0]
    prev = pm.initial_prev(C, size)
    amp, dev, _, _ = pm.analyze64(P, prev, size, hop, SR)
    fr = pm.analyze32(P, prev, size, hop, SR)
    th, _ = pm.phases(fr[..., 1], pm.initial_phase(C, size), hop, SR)
    return dict(size=size, hop=hop, P=P, prev=prev, amp=amp, dev=dev, fr=fr, th=th, sp=pm.synth32(fr, th))


@pytest.mark.parametrize("size", pp.SIZES)
def test_ranged_probe_is_what_it_claims(size):
    M = size // 2
    for hop in pp.hops(size):
        P = pp.probe_spectra(size, hop)
        assert P.shape == (2, 69, M) and P.dtype == np.complex64 and not P.flags.writeable
        assert np.isfinite(P.view(f32)).all()
        again = pp._PROBES.pop((size, hop, 2, 69))
        assert np.array_equal(pp.probe_spectra(size, hop).view(np.uint32), again.view(np.uint32)), "not deterministic"
        z = pm.bins(P)
        a = np.abs(z.astype(np.complex128))
        live = np.arange(69) != pp.ZERO_F
        assert not a[:, pp.ZERO_F].any()
        assert a[:, live].min() >= 2.0 ** -44.01 and a[:, live].max() <= 2.0 ** 44.01
        # every bin has a level of its own: the bins' medians over the frames span more than 70 octaves
        med = np.log2(np.median(a[:, live], axis=1))
        assert med.max() - med.min() > 70
        assert np.array_equal(z[:, pp.DOUBLE_F], z[:, pp.DOUBLE_F - 1] * f32(2))
        assert np.array_equal(z[:, pp.NEG_F], -z[:, pp.NEG_F - 1])
        assert pp.ZERO_F % pp.RUN == pp.RUN - 1 and pp.NEG_F % pp.RUN == 0 and 69 % pp.RUN not in (0, pp.RUN - 1)
        # |z| |z_prev| is a normal float32 wherever it is not 0
        prod = a[:, 1:] * a[:, :-1]
        assert prod[prod > 0].min() >= 2.0 ** -88.1 and prod.max() <= 2.0 ** 88.1
        # the cut: d of NEG_F is on the negative real axis before the rotation, exactly
        amp, dev, _, _ = pm.analyze64(P, pm.initial_prev(2, size), size, hop, SR)
        if hop == size:
            assert np.all(np.abs(dev[:, pp.NEG_F]) == 0.5)
            assert not dev[:, pp.DOUBLE_F].any()
        assert not dev[:, pp.ZERO_F].any() and not dev[:, pp.ZERO_F + 1].any() and not amp[:, pp.ZERO_F].any()


@pytest.mark.parametrize("size", pp.SIZES)
def test_exact_synthesis_probe_follows_from_the_model(size):
    frames, want, state, hop = pp.exact_synth(size, 2, 2 * 64 + 3)
    assert hop == size // 4 and np.float32(hop / pp.SR_EXACT) == hop / pp.SR_EXACT
    q = frames[..., 1].astype(np.float64) * size / pp.SR_EXACT
    assert np.array_equal(q, np.rint(q)) and np.abs(q).max() < 2 ** 20
    qi = q.astype(np.int64)
    for r in range(4):
        assert ((qi % 4) == r).any(axis=1).all(), "residue %d is missing in a bin" % r
    inc = pm.increments(frames[..., 1], hop, pp.SR_EXACT)
    assert np.array_equal(inc.astype(np.int64), (qi % 4) << 30), "the increments are not exact multiples of 2^30"
    th, new = pm.phases(frames[..., 1], pm.initial_phase(2, size), hop, pp.SR_EXACT)
    assert np.array_equal(new, state) and not (th & (2 ** 30 - 1)).any()
    amps = frames[..., 0]
    assert np.array_equal(amps, np.rint(amps)) and amps.min() == -3 and amps.max() == 3 and (amps == 0).any()
    assert np.abs(pm.synth64(frames, th) - want).max() < 1e-14
    assert np.abs(pm.bins(want)).max() == 3


@pytest.mark.parametrize("size", pp.SIZES)
def test_exact_analysis_probe_follows_from_the_model(size):
    P, want_amp, want_freq = pp.exact_analysis(size, 2, 13)
    M = size // 2
    e = pm.etab(size, size)
    assert np.all(e.real == 1) and not e.imag.any()      # (1, +-0): dy = tx (+-0) + (+0) = +0 either way
    amp, dev, freq, _ = pm.analyze64(P, pm.initial_prev(2, size), size, size, SR)
    assert np.all(np.abs(amp - want_amp) <= 2.0 ** -51 * want_amp)       # (numpy's hypot is not exact; the integers are)
    assert not dev[:, 1:].any() and np.array_equal(freq[:, 1:].astype(f32), np.broadcast_to(want_freq, freq[:, 1:].shape))
    assert (want_amp[..., [0, M]] > 0).all() and (want_amp[..., 1:M] >= 5).all()
    # the float32 evaluation reaches those bits, whole and cut into two calls
    whole = pm.analyze32(P, pm.initial_prev(2, size), size, size, SR)
    second = pm.analyze32(P[:, 6:], pm.bins(P[:, 5]), size, size, SR)
    assert np.array_equal(whole[:, 6:].view(np.uint32), second.view(np.uint32))
    assert np.array_equal(whole[..., 0].view(np.uint32), want_amp.view(np.uint32))
    assert np.array_equal(whole[:, 1:, :, 1].view(np.uint32), np.broadcast_to(want_freq, (2, 12, M + 1)).view(np.uint32))


@pytest.mark.parametrize("size", pp.SIZES)
def test_float32_model_stays_under_the_caps(size):
    """the conditions of the yardstick: on every probe of the GPU test the model's own worst bin is at most CAPS; a probe
    that pushed it further would widen the device's bound and has to be changed instead"""
    for hop in pp.hops(size):
        m = model_case(size, hop)
        e = pp.analysis_errors(m["fr"], m["amp"], m["dev"], size, hop, SR)
        e["synth"] = pp.synth_worst(m["sp"], m["fr"], m["th"])
        print("PVOCBIN model size %d hop %d: amp %.2f at %s  dev %.2f at %s  synth %.2f at %s"
              % (size, hop, e["amp"][0], e["amp"][1], e["dev"][0], e["dev"][1], e["synth"][0], e["synth"][1]))
        for what, cap in pp.CAPS.items():
            assert e[what][0] <= cap, "size %d hop %d: the model's %s error %.2f at %s" % ((size, hop, what) + e[what])


# ---- the mutants: size 1024, hop 256 ----

@pytest.fixture(scope="module")
def case():
    m = model_case(1024, 256)
    m["u_dev"] = pp.dev_worst(m["fr"], m["dev"], 1024, 256, SR)[0]
    m["u_amp"] = pp.amp_worst(m["fr"], m["amp"])[0]
    m["u_syn"] = pp.synth_worst(m["sp"], m["fr"], m["th"])[0]
    for v in m.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return m


def plant_dev(fr, c, f, k, turns, size, hop):
    """frames with `turns` added to dev of one bin of one frame: freq moves by turns (size / hop) (sr / size), rounded to
    float32 as the model rounds it"""
    out = np.array(fr)
    out[c, f, k, 1] = f32(float(out[c, f, k, 1]) + turns * (size / hop) * (SR / size))
    return out


def stft_style_spectra(size, hop, F, seed):
    """the input of tests/test_gpu_pvoc.py's stft_spectra, in numpy: Hann-windowed frames of noise plus two sinusoids"""
    x = two_tones(size, hop, 1, F, seed)[0]
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(size) / size)
    X = np.fft.rfft(np.stack([x[f * hop:f * hop + size] * w for f in range(F)]), axis=-1)
    return pm.unbins(X).astype(np.complex64)[None]


def test_mutant_a_one_bin_of_one_frame_off_by_1e_4_turns(case):
    """1e-4 turns on dev of bin M in one frame.  At bin M of size 1024, hop 256 that is 1e-4 / s_M = 12.95 units, and the
    bound at margin 8 is 8 x U32 = 13.1 on this probe: the plant alone sits AT the bound, and what decides is the
    element's own error and the rounding of freq to its float32 grid (one step at 24000 Hz is 2^-9 Hz = 1.35 units; the
    plant is 0.01875 Hz = 9.6 steps, so it lands as 9 or 10).  So the plant goes where both are known: the zero frame,
    whose freq is the bin centre exactly (own error 0), and there 9.6 steps round to 10 = 13.5 units.  At the margin in
    use (pvoc_probe.MARGIN_BIN) the same plant misses the bound in every frame."""
    size, hop, M = 1024, 256, 512
    bad = plant_dev(case["fr"], 1, pp.ZERO_F, M, 1e-4, size, hop)
    e, at = pp.dev_worst(bad, case["dev"], size, hop, SR)
    assert at == (1, pp.ZERO_F, M) and e > pp.bound(LARGEST_MARGIN, case["u_dev"]), (e, at, case["u_dev"])
    assert pp.amp_worst(bad, case["amp"])[0] == case["u_amp"]
    for f in range(69):
        e, at = pp.dev_worst(plant_dev(case["fr"], 0, f, M, 1e-4, size, hop), case["dev"], size, hop, SR)
        assert at == (0, f, M) and e > pp.bound(pp.MARGIN_BIN, case["u_dev"]), (f, e)
    # the aggregate rule of tests/test_gpu_pvoc.py does not see it: relative L2 of the phasors over the whole call
    F = 65
    P = stft_style_spectra(size, hop, F, 7)
    prev = pm.initial_prev(1, size)
    amp, dev, _, _ = pm.analyze64(P, prev, size, hop, SR)
    truth = amp * np.exp(2j * np.pi * dev)
    fr = pm.analyze32(P, prev, size, hop, SR)
    e_f32 = pm.rel_l2(pm.phasors(fr, size, hop, SR), truth)
    for f in (1, F // 2, F - 1):
        ratio = pm.rel_l2(pm.phasors(plant_dev(fr, 0, f, M, 1e-4, size, hop), size, hop, SR), truth) / e_f32
        assert ratio < 2.0, ratio          # (it moves by less than 1 %)
    # in EVERY frame (the stronger plant, 16 %): still far inside the aggregate margin
    every = np.array(fr)
    every[0, :, M, 1] += f32(1e-4 * (size / hop) * (SR / size))
    assert pm.rel_l2(pm.phasors(every, size, hop, SR), truth) / e_f32 < 2.0


def test_mutant_b_bin_half_m_not_conjugated(case):
    size, hop, M = 1024, 256, 512
    P = np.array(case["P"])
    P[..., M // 2] = np.conj(P[..., M // 2])
    bad = pm.analyze32(P, case["prev"], size, hop, SR)
    keep = np.arange(M + 1) != M // 2
    assert np.array_equal(bad[:, :, keep].view(np.uint32), case["fr"][:, :, keep].view(np.uint32))
    e, at = pp.dev_worst(bad, case["dev"], size, hop, SR)
    assert at[2] == M // 2 and e > pp.bound(LARGEST_MARGIN, case["u_dev"])
    assert pp.amp_worst(bad, case["amp"])[0] <= case["u_amp"], "the amp does not see a conjugation"


def test_mutant_c_a_run_starts_from_the_wrong_frame(case):
    """bin 170 of frame 4 (the first of run 1) takes frame 2 as its predecessor"""
    size, hop, k = 1024, 256, 170
    P = np.array(case["P"])
    P[0, 3, k] = P[0, 2, k]
    bad = np.array(case["fr"])
    bad[0, 4, k] = pm.analyze32(P, case["prev"], size, hop, SR)[0, 4, k]
    e, at = pp.dev_worst(bad, case["dev"], size, hop, SR)
    assert at == (0, 4, k) and e > pp.bound(LARGEST_MARGIN, case["u_dev"])


def test_mutant_d_one_phase_off_by_2_to_minus_16_turn(case):
    k = 170
    th = np.array(case["th"])
    th[1, 40, k] += np.uint32(1 << 16)
    bad = pm.synth32(case["fr"], th)
    e, at = pp.synth_worst(bad, case["fr"], case["th"])
    assert at == (1, 40, k) and e > pp.bound(LARGEST_MARGIN, case["u_syn"])


def test_mutant_e_bins_0_and_m_swapped_in_the_packing(case):
    bad = np.array(case["sp"])
    bad[..., 0] = bad[..., 0].imag + 1j * bad[..., 0].real
    e, at = pp.synth_worst(bad, case["fr"], case["th"])
    assert at[2] in (0, 512) and e > pp.bound(LARGEST_MARGIN, case["u_syn"])


def test_the_unmutated_model_passes(case):
    size, hop = 1024, 256
    assert pp.dev_worst(case["fr"], case["dev"], size, hop, SR)[0] <= pp.bound(2.0, case["u_dev"])
    assert pp.amp_worst(case["fr"], case["amp"])[0] <= pp.bound(2.0, case["u_amp"])
    assert pp.synth_worst(case["sp"], case["fr"], case["th"])[0] <= pp.bound(2.0, case["u_syn"])
    # and the yardstick has no opinion on the sign of the cut: dev off by one whole turn is the same answer
    turn = np.array(case["fr"], np.float64)
    turn[0, pp.NEG_F, :, 1] += (size / hop) * (SR / size)
    assert pp.dev_worst(turn, case["dev"], size, hop, SR)[0] <= case["u_dev"] + 1e-6
    # a NaN, and a non-zero amp where the truth is 0, are infinite errors
    nan = np.array(case["fr"])
    nan[0, 3, 9, 1] = np.nan
    assert pp.dev_worst(nan, case["dev"], size, hop, SR) == (np.inf, (0, 3, 9))
    loud = np.array(case["fr"])
    loud[1, pp.ZERO_F, 9, 0] = 1e-30
    assert pp.amp_worst(loud, case["amp"]) == (np.inf, (1, pp.ZERO_F, 9))
