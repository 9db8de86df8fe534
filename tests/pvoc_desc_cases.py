"""The inputs of the descriptor tests that need no device: tests/test_gpu_pvoc_desc.py runs them on the GPU against the
model, tests/test_pvoc_desc_cpu.py runs the model's mutants on the same ones (a case that no mutant changes proves nothing).
A case is (name, frames (C, F, M + 1, 2) float32, first_bin, nbins, rectify); nbins None = up to M."""
import numpy as np

from tests import pvoc_inputs
from tests.pvoc_desc_model import lanes
from tests.pvoc_inputs import SR

f32 = np.float32
SIZES = (64, 128, 256, 512, 1024, 16384)      # W below a wave, one wave, two waves, 256 with one row, two rows, 32 rows
MORE_SIZES = (2048, 4096, 8192)
FRAME_COUNTS = (1, 5, 37, 200)


def plain(size, C, F, seed):
    """amps |N(0, 1)| + 0.01 (sums whose bits depend on the order of the additions), freqs near the bin centres"""
    rng = np.random.default_rng(1000 + seed)
    B = size // 2 + 1
    amp = np.abs(rng.standard_normal((C, F, B))).astype(f32) + f32(0.01)
    freq = (np.arange(B) * (SR / size) + rng.standard_normal((C, F, B)) * SR / size / 4).astype(f32)
    return np.stack([amp, freq], axis=-1)


def raw(size, C, F, seed):
    """tests/pvoc_inputs.py's raw(): amps log-uniform over 1e-30 .. 1e30 with a few zeros, any freq; pow and flux
    overflow to inf on purpose"""
    return pvoc_inputs.raw(size, C, F, seed)


def ranges(M):
    """(name, first_bin, nbins): everything, 1..M-1, the Nyquist bin alone, bin 0 alone, two bins crossing into the
    Nyquist term and, where a lane has a second row, two bins straddling two rows"""
    W = lanes(M)
    out = [("all", 0, None), ("inner", 1, M - 1), ("nyquist", M, 1), ("dc", 0, 1), ("into nyquist", M - 1, 2)]
    if M > W:
        out.append(("two rows", W - 1, 2))
    return out


def planted(size, C, seed=7):
    """plain frames with values planted; the name says what"""
    M = size // 2
    W = lanes(M)
    F = 6
    c = C - 1
    out = []

    def case(name, first_bin=0, nbins=None, rectify=False):
        x = plain(size, C, F, seed + len(out))
        out.append((name, x, first_bin, nbins, rectify))
        return x

    for rectify in (False, True):
        x = case("one NaN amp" + (", rectified" if rectify else ""), rectify=rectify)
        x[c, 2, M // 3, 0] = np.nan
        x = case("one NaN amp outside the range" + (", rectified" if rectify else ""), M // 2, M // 4, rectify)
        x[c, 2, M // 3, 0] = np.nan
    x = case("an all-NaN range", 3, 4)
    x[c, 1, 3:7, 0] = np.nan
    x = case("a NaN Nyquist amp, alone in the range", M, 1)
    x[c, 4, M, 0] = np.nan
    x = case("equal maxima at M - 1 and M")
    x[c, 3, M - 1:, 0] = 50.0
    x = case("the maximum at M alone")
    x[c, 3, M, 0] = 50.0
    x = case("equal maxima in one lane's neighbours", 1, M - 1)
    x[:, 2, [5, 6], 0] = 50.0
    if M > W:
        x = case("equal maxima at k and k + W")
        x[c, 3, [9, 9 + W], 0] = 50.0
        x = case("equal maxima at k + W and a higher lane's k")
        x[c, 3, [9 + W, 11], 0] = 50.0
    x = case("a frame of zeros")
    x[:, 2, :, 0] = 0.0
    x = case("a frame of -0")
    x[:, 2, :, 0] = -0.0
    x = case("-0 below +0", 4, 8)
    x[:, 1, 4:12, 0] = 0.0
    x[:, 1, 4, 0] = -0.0
    x = case("+0 below -0", 4, 8)
    x[:, 1, 4:12, 0] = -0.0
    x[:, 1, 4, 0] = 0.0
    x = case("negative amps, the largest a -0")
    x[..., 0] = -x[..., 0]
    x[c, 2, M // 2, 0] = -0.0
    return out


def streams(size, C, counts=FRAME_COUNTS, kinds=("plain", "raw")):
    """the random cases of one size: every frame count and kind over everything, alternately rectified, and every range
    at 37 frames (or the most there is)"""
    M = size // 2
    out = []
    n = 0
    for F in counts:
        for kind in kinds:
            x = plain(size, C, F, F) if kind == "plain" else raw(size, C, F, F + 1)
            out.append(("%s F %d" % (kind, F), x, 0, None, bool(n & 1)))
            n += 1
    F = 37 if 37 in counts else max(counts)
    for kind in kinds:
        x = plain(size, C, F, F) if kind == "plain" else raw(size, C, F, F + 1)
        for name, first, nb in ranges(M)[1:]:
            out.append(("%s F %d range %s" % (kind, F, name), x, first, nb, bool(n & 1)))
            n += 1
    return out
