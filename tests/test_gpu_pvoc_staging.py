"""The blocking forms of Pvoc stage their arrays in slots shared by role (pvoc_host.hpp): the output rows of desc, bands and
pitch are one slot, the lists of trace, demix and pitch another, the second per-frame rows, the float table and the int
table each serve two families.  On one object (size 64, hop 16, 2 channels) the families that share a slot run interleaved,
at 3 frames, at 70 and at 3 again (a slot that holds a longer call's leftovers), and every result must equal, bit for bit,
the same call on an object that has only ever made that family's calls: the same state history, no other family in its
slots.  The host outputs sit in guard bands (tests/gpu_guard.py): a copy-out may write its array and nothing else."""
import numpy as np
import pytest
import torch

import opencl_fft_amd as fa
from tests import gpu_guard as G
from tests import pvoc_inputs

pytestmark = pytest.mark.gpu

SIZE, HOP, CH, M, SR = 64, 16, 2, 32, pvoc_inputs.SR
ROUNDS = (3, 70, 3)
f32 = np.float32


def frames(F, seed):
    return np.array(pvoc_inputs.raw(SIZE, CH, F, seed, tilt=True))


def call(pv, name, shapes, args):
    """one blocking call with its outputs (shape, torch dtype) in host guard bands: args(pointers) are the arguments
    after the object.  The outputs' words, and the guard bands checked"""
    outs = [G.flat(shape, dtype=torch.float32, device="cpu") for shape in shapes]
    assert pv._get(name, *args(*[g.data.data_ptr() for g in outs])) == 0, name
    for g in outs:
        g.check_sides(name + "'s output")
    return [g.words.numpy().copy() for g in outs]


def desc(pv, F, seed):
    x = frames(F, seed)
    return call(pv, "desc", [(CH, F, 8)], lambda o: (x.ctypes.data, o, F, 0, M + 1, 1))


def bands(pv, F, seed):
    x = frames(F, seed)
    return call(pv, "bands", [(CH, F, 5)], lambda o: (x.ctypes.data, o, F, 7, 5, 1e-6))


def pitch(pv, F, seed):
    x = frames(F, seed)
    return call(pv, "pitch", [(CH, F, 4), (CH, F, 8, 2)],
                lambda rows, peaks: (x.ctypes.data, rows, peaks, F, 1, M - 1, 8, 0.0, 50.0, SR / 4, 0.03, 0.84))


def trace(pv, F, seed):
    x, n = frames(F, seed), np.random.default_rng(seed).uniform(0, 12, F).astype(f32)
    return call(pv, "trace", [(CH, F, M + 1, 2), (CH, F, 6)],     # the bin list is int32: compared as words like the rest
                lambda out, bins: (x.ctypes.data, out, n.ctypes.data, bins, 6, F, 0, M + 1, 0))


def demix(pv, F, seed):
    rng = np.random.default_rng(seed)
    l, r = frames(F, seed), frames(F, seed + 1000)
    par = np.stack([rng.uniform(-1, 1, F), rng.uniform(1, 11, F)], axis=1).astype(f32)
    return call(pv, "demix", [(CH, F, M + 1, 2), (CH, F, 11)],
                lambda out, az: (l.ctypes.data, r.ctypes.data, out, par.ctypes.data, az, F, 5, 0, M + 1))


def smooth(pv, F, seed):
    rng = np.random.default_rng(seed)
    x, p, q = frames(F, seed), rng.random(F).astype(f32), rng.random(F).astype(f32)
    return call(pv, "time", [(CH, F, M + 1, 2)], lambda o: (1, x.ctypes.data, o, F, p.ctypes.data, q.ctypes.data))


def tanal(pv, F, seed):
    signal = np.ascontiguousarray(pvoc_inputs.two_tones(SIZE, HOP, CH, 8, seed), dtype=f32)
    window, n = pvoc_inputs.hann(SIZE), signal.shape[1]
    starts = np.random.default_rng(seed).integers(-SIZE, n, F).astype(np.int32)
    return call(pv, "tanal", [(CH, F, M + 1, 2)],
                lambda o: (signal.ctypes.data, n, n, window.ctypes.data, starts.ctypes.data, o, F))


def delay(pv, F, seed):
    rng = np.random.default_rng(seed)
    x, d, g = frames(F, seed), rng.integers(0, 4, M + 1).astype(np.int32), rng.uniform(-0.8, 0.8, M + 1).astype(f32)
    return call(pv, "delay", [(CH, F, M + 1, 2)], lambda o: (x.ctypes.data, o, F, d.ctypes.data, g.ctypes.data))


# neighbours in this order share slots: the output rows (desc, bands, pitch), the output list (pitch, trace, demix), the
# float and the int table (tanal's window and starts, delay's feedback and delays); all but tanal share the frames in, and
# trace, demix, smooth, tanal and delay the frames out
FAMILIES = [desc, bands, pitch, trace, demix, smooth, tanal, delay]


def make():
    pv = fa.Pvoc(0, SIZE, HOP, SR, CH)
    assert pv.get_error() == 0, pv.get_log()
    assert pv.delay_setup(3) == 0
    assert pv.bank_setup(*fa.Pvoc.mel_bank(SIZE, SR, 8)) == 0
    return pv


@pytest.fixture(scope="module")
def interleaved():
    pv = make()
    return {(fam.__name__, r): fam(pv, F, 100 * r + i) for r, F in enumerate(ROUNDS) for i, fam in enumerate(FAMILIES)}


@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f.__name__)
def test_shared_slots_leave_every_family_its_bits(interleaved, fam):
    pv, i = make(), FAMILIES.index(fam)
    for r, F in enumerate(ROUNDS):
        alone = fam(pv, F, 100 * r + i)
        for k, (got, want) in enumerate(zip(interleaved[(fam.__name__, r)], alone)):
            assert np.array_equal(got, want), "%s, round %d (F = %d), output %d" % (fam.__name__, r, F, k)
