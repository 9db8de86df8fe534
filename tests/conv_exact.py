"""Exact test families for the convolution objects: block impulses against single-tap responses (partitioned convolution,
the convolution matrix) and unit taps against noise (direct convolution).  No GPU and no torch here; the tests that use this
are tests/test_conv_exact_cpu.py (the oracle and the float64 models) and tests/test_gpu_conv_impulses.py (the HIP routes).

Partitioned convolution.  Input: one non-zero sample, sample s of block b0.  Response: one non-zero tap, tap k of partition
p.  By the reference's formula (tests/util.py pconv_f64) output blocks b0 + p and b0 + p + 1 are the two halves of ONE
2 pts-point inverse transform of X H, and every other block is exactly zero.  The float64 rfft of those two blocks
(readback) is X H bin by bin: every bin has magnitude 1, bins 0 and pts 1/2 (the packed-bin gain, SURVEY.md section 8a,
fact 3) — so max|dY| / max|Y| (worst_bin) is the worst SINGLE bin of one partition, where a norm over a channel of noise
divides one bad table entry by sqrt(bins x partitions).  A comb response (unit taps in the even, or the odd, partitions)
keeps partitions p - 1 and p + 1 empty: the pair (b0 + p, b0 + p + 1) then holds partition p alone, and two channels cover
every partition of a route in one run.

The truth is always one of the existing float64 models (util.pconv_f64, util.pconv_tv_f64, pconv_matrix_model.MatrixModel,
dconv_blocks_model.DconvBlocksModel).  pair_truth() is pconv_f64 at its smallest geometry (one partition, two blocks); that
every pair of a comb run equals it exactly, for any b0 and p, static and time-varying, is what test_conv_exact_cpu.py
checks on the full models.

Direct convolution.  A response with one unit tap at k makes every output a sum with ONE non-zero term: the input delayed
by k + 1 samples, value for value whatever the order, chunking or segmenting of the sum — those tests use ==."""
import functools

import numpy as np

from tests import util
from tests.dconv_blocks_model import DconvBlocksModel

DCONV_TAPS = (0, 1, 7, 8, 255, 256, 4095, 4096)   # ... and irsize - 1: the chunk (256) and segment (4096) boundaries


# ---- positions ------------------------------------------------------------------------------------------------------------------

def tap_positions(pts):
    """k over {0, 1, pts / 2, pts - 1}"""
    return sorted({k for k in (0, 1, pts // 2, pts - 1) if 0 <= k < pts})


def sample_positions(pts):
    """s over {0, 1, pts / 2 + 1, pts - 1}"""
    return sorted({s for s in (0, 1, pts // 2 + 1, pts - 1) if 0 <= s < pts})


def ks_pairs(pts, full):
    """the (k, s) pairs of a geometry: all of tap_positions x sample_positions (full: objects with channels to spare), or
    every k and every s once (k_i with s_(i+1): one run per pair where a route has one or two channels)"""
    ks, ss = tap_positions(pts), sample_positions(pts)
    if full:
        return [(k, s) for k in ks for s in ss]
    return [(ks[i % len(ks)], ss[(i + 1) % len(ss)]) for i in range(max(len(ks), len(ss)))]


def comb(nparts, parity):
    """the partitions of a comb: parity 0 the even ones, 1 the odd ones"""
    return np.arange(parity, nparts, 2)


def slots(pts, channels):
    """the (parity, k, s) cases of a geometry, even and odd comb of every pair"""
    return [(parity, k, s) for k, s in ks_pairs(pts, channels >= 32) for parity in (0, 1)]


# The routes of Clpconv's single-block call and the geometries that select them (tests/test_gpu_conv.py): name, kernel_name(),
# pts, nparts, channels, b0 (nparts + 1: the ring has wrapped when the impulse comes).
PCONV_ROUTES = [
    ("cooperative", "k_pconv_coop", 32, 5, 1, 1),
    ("cooperative", "k_pconv_coop", 512, 5, 1, 6),
    ("cooperative", "k_pconv_coop", 1024, 94, 2, 1),
    ("cooperative, partition segments", "k_pconv_coop", 512, 600, 1, 601),
    ("cooperative, partition segments", "k_pconv_coop", 512, 2048, 1, 1),
    ("cooperative, many channels", "k_pconv_coop", 512, 6, 100, 7),
    ("fused", "k_pconv_fused", 512, 5, 162, 6),
    ("fused, partitions requested ahead", "k_pconv_fused", 1024, 40, 160, 41),
    ("launch chain", "chain", 2, 1, 3, 2),
    ("launch chain", "chain", 8, 4, 1, 5),
    ("launch chain", "chain", 8192, 2, 1, 1),
    ("launch chain", "chain", 16384, 2, 2, 3),
    ("launch chain, four-step", "chain", 32768, 3, 1, 1),
]
# the multi-block call (process_blocks_device): blocks_kernel_name(), pts, nparts, channels, b0
# k_pconvb_mac at every transform size of the route, 32 .. 4096 (one instantiation of the forward and inverse kernels each)
PCONV_BLOCK_ROUTES = [("loop", 8, 3, 3, 1), ("k_pconvb_mac", 64, 3, 3, 4), ("k_pconvb_mac", 1024, 94, 3, 1),
                      ("k_pconvb_mac", 32, 5, 3, 6), ("k_pconvb_mac", 128, 3, 3, 4), ("k_pconvb_mac", 256, 5, 1, 1),
                      ("k_pconvb_mac", 512, 3, 3, 2), ("k_pconvb_mac", 2048, 5, 3, 6), ("k_pconvb_mac", 4096, 3, 3, 1)]
# the convolution matrix: inputs, outputs, pts, nparts
MATRIX_GEOMS = [(3, 5, 256, 12), (4, 4, 64, 3), (2, 3, 128, 5), (3, 2, 2048, 3)]


def nblocks_for(nparts, b0):
    """the last pair ends with block b0 + nparts; one more block that must be zero"""
    return b0 + nparts + 2


# ---- builders -------------------------------------------------------------------------------------------------------------------

def single_tap_response(pts, nparts, p, k):
    ir = np.zeros(nparts * pts, np.float32)
    ir[p * pts + k] = 1.0
    return ir


def comb_response(pts, nparts, parity, k):
    """unit tap k in every partition of the comb"""
    ir = np.zeros(nparts * pts, np.float32)
    ir[comb(nparts, parity) * pts + k] = 1.0
    return ir


def block_impulse(pts, nblocks, b0, s):
    x = np.zeros(nblocks * pts, np.float32)
    x[b0 * pts + s] = 1.0
    return x


def tv_comb_input(pts, nparts, nblocks, parity, k):
    """the comb as a second input: block t overwrites partition t mod nparts (util.pconv_tv_f64), so every block whose
    partition belongs to the comb carries the tap — through the whole signal, the ring keeps being rewritten"""
    x = np.zeros((nblocks, pts), np.float32)
    t = np.arange(nblocks)
    x[(t % nparts) % 2 == parity, k] = 1.0
    return x.reshape(-1)


def matrix_entry(inputs, outputs, pts, nparts, i, o, parts, k):
    """responses (outputs, inputs, nparts * pts) with the entries (i, o, p, k), p in parts, set to one"""
    ir = np.zeros((outputs, inputs, nparts * pts), np.float32)
    ir[o, i, np.asarray(parts, dtype=np.int64) * pts + k] = 1.0
    return ir


def nonzero_noise(seed, shape):
    """uniform [-0.5, 0.5) float32 without a zero in it"""
    x = np.random.default_rng(seed).random(shape, dtype=np.float32) - np.float32(0.5)
    x[x == 0] = np.float32(0.25)
    return x


# ---- truth: the float64 models --------------------------------------------------------------------------------------------------

def pconv_truth(ir, x, pts):
    """util.pconv_f64 of a signal of any number of blocks (the model wants at least nparts: zero blocks appended)"""
    nparts = ir.size // pts
    blocks = x.size // pts
    xp = np.zeros(max(blocks, nparts) * pts)
    xp[:x.size] = x
    return util.pconv_f64(np.asarray(ir, np.float64), xp, pts)[:x.size]


def pconv_tv_truth(x1, x2, pts, nparts):
    return util.pconv_tv_f64(np.asarray(x1, np.float64), np.asarray(x2, np.float64), pts, nparts)


@functools.lru_cache(maxsize=None)
def pair_truth(pts, k, s):
    """float64[2 pts]: the block pair of tap k against sample s — pconv_f64 of one partition and two blocks"""
    y = pconv_truth(single_tap_response(pts, 1, 0, k), block_impulse(pts, 2, 0, s), pts)
    y.setflags(write=False)
    return y


def readback(out, pts, block):
    """float64 rfft of output blocks `block` and `block + 1` (last axis: samples): X H, 2 pts / 2 + 1 = pts + 1 bins"""
    out = np.asarray(out)
    return np.fft.rfft(out[..., block * pts:(block + 2) * pts].astype(np.float64), axis=-1)


def worst_bin(got, truth):
    """max |dY| / max |Y|"""
    return float(np.max(np.abs(np.asarray(got) - truth)) / np.max(np.abs(truth)))


def worst_sample(got, truth):
    """max |dy| / max |y| in the time domain"""
    return float(np.max(np.abs(np.asarray(got, np.float64) - truth)) / np.max(np.abs(truth)))


def outside_pairs(nblocks, b0, parts):
    """bool[nblocks]: the blocks that belong to no pair (b0 + p, b0 + p + 1)"""
    m = np.ones(nblocks, bool)
    parts = np.asarray(parts, dtype=np.int64)
    m[b0 + parts] = False
    m[b0 + parts + 1] = False
    return m


def check_channel(out, pts, b0, parts, k, s):
    """One channel's output (nblocks * pts samples) against the family's expectation.  Returns (worst bin, worst sample,
    number of non-zero samples outside the pairs, (partition, bin) of the worst bin)."""
    out = np.asarray(out).reshape(-1, pts)
    parts = np.asarray(parts, dtype=np.int64)
    stray = int(np.count_nonzero(out[outside_pairs(out.shape[0], b0, parts)]))
    if parts.size == 0:
        return 0.0, 0.0, stray, (-1, -1)
    truth = pair_truth(pts, k, s)
    pairs = np.concatenate([out[b0 + parts], out[b0 + parts + 1]], axis=1).astype(np.float64)
    Y = np.fft.rfft(truth)
    d = np.abs(np.fft.rfft(pairs, axis=1) - Y)
    at = np.unravel_index(int(np.argmax(d)), d.shape)
    return (float(d[at] / np.max(np.abs(Y))), float(np.max(np.abs(pairs - truth)) / np.max(np.abs(truth))), stray,
            (int(parts[at[0]]), int(at[1])))


# ---- direct convolution ---------------------------------------------------------------------------------------------------------

def dconv_taps(irsize):
    return sorted({k for k in DCONV_TAPS + (irsize - 1,) if k < irsize})


def unit_tap(irsize, k):
    ir = np.zeros(irsize, np.float32)
    ir[k] = 1.0
    return ir


def dconv_delayed(x, k):
    """static form on a fresh object: out[t] = x[t - 1 - k] (the one-sample delay is the reference's, cl_dconv.cpp:40-41),
    zero before the signal; last axis: samples"""
    x = np.asarray(x, np.float32)
    out = np.zeros_like(x)
    if k + 1 < x.shape[-1]:
        out[..., k + 1:] = x[..., :x.shape[-1] - k - 1]
    return out


def dconv_blocks_needed(irsize, vsize, wraps=2):
    """blocks that take the delay ring (irsize + vsize samples) round `wraps` times, and one more"""
    return (wraps * (irsize + vsize) + vsize - 1) // vsize + 1


def dconv_tv_impulses(irsize, vsize, nblocks):
    """a second input with unit samples irsize + vsize + 3 apart: the coefficient ring never holds two of them, and they
    land on different ring positions"""
    x2 = np.zeros(nblocks * vsize, np.float32)
    x2[vsize + 1::irsize + vsize + 3] = 1.0
    return x2


def dconv_tv_expected(irsize, vsize, x1, x2):
    """time-varying form on a fresh object by the contract of include/clfft_amd.h as dconv_blocks_model restates it; with
    dconv_tv_impulses every sum has at most one non-zero term, a float32 value times one: float64 holds it exactly"""
    x1, x2 = np.atleast_2d(x1), np.atleast_2d(x2)
    m = DconvBlocksModel(irsize, vsize, channels=x1.shape[0])
    return m.blocks(x1, x2).astype(np.float32)
