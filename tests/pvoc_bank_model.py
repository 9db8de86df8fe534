"""The filter bank on (amp, freq) frames of clfa_pvoc (include/clfft_amd.h: TERM, BAND, LOG, DCT) restated in numpy,
operation by operation in float32, with a float64 version of every stage, the named mutants the tests must notice, and
the banks and inputs the CPU and the device tests share.

Every float32 step is one numpy operation on float32 arrays, so it is rounded on its own.  The DCT table is an argument:
the bits are defined given the table the device uses (Pvoc.bank_dct()); dct_table() is the header's formula in float64.

Mutants (the `mutant` argument): "serial" (a band's terms added one after the other), "halving" (the tree pairs s[i] with
s[i + n/2], not with its neighbour), "w32" (32 lanes), "fma" (the term's product not rounded on its own), "dct_descending"
(the DCT's sum from the last band down), "nan_no_floor" (a NaN energy passes the floor)."""
import numpy as np

f32 = np.float32
SR = 48000.0
LANES = 16
MUTANTS = ("serial", "halving", "w32", "fma", "dct_descending", "nan_no_floor")
U = 2.0 ** -24


class Bank:
    """first, count: int (B,); weights: float32 (sum(count),); w(b): the weights of band b"""

    def __init__(self, first, count, weights):
        self.first = np.asarray(first, np.int64)
        self.count = np.asarray(count, np.int64)
        self.weights = np.ascontiguousarray(weights, dtype=f32)
        self.off = np.concatenate([[0], np.cumsum(self.count)])
        self.B = len(self.first)
        assert self.weights.size == self.off[-1]

    def w(self, b):
        return self.weights[self.off[b]:self.off[b + 1]]

    def args(self):
        return self.first.astype(np.int32), self.count.astype(np.int32), self.weights


def valid(M, first, count, weights):
    """the setup's own validation (bank_plan.hpp's bank_ok)"""
    first, count, weights = np.asarray(first), np.asarray(count), np.asarray(weights)
    if not (1 <= first.size <= 256 and first.size == count.size):
        return False
    if (count < 1).any() or (first < 0).any() or (first.astype(np.int64) + count > M + 1).any():
        return False
    return weights.size == int(count.sum()) and bool(np.isfinite(weights).all())


def x_of(amps, power):
    """TERM's x: the amps, or their float32 squares"""
    amps = np.asarray(amps, f32)
    with np.errstate(all="ignore"):
        return amps * amps if power else amps


def s16(x, w, mutant=None):
    """S16 of the terms fl(x[..., i] w[i]): x float32 (..., count), w float32 (count,) -> float32 (...,)"""
    width = 32 if mutant == "w32" else LANES
    n = x.shape[-1]
    with np.errstate(all="ignore"):
        t = x * w
        if mutant == "serial":
            s = t[..., 0]
            for i in range(1, n):
                s = s + t[..., i]
            return s
        p = np.zeros(x.shape[:-1] + (width,), f32)
        p[..., :min(n, width)] = t[..., :width]
        for i in range(width, n, width):
            m = min(width, n - i)
            if mutant == "fma":   # the product exact (48 bits in a double), one rounding for the multiply-add
                p[..., :m] = (p[..., :m].astype(np.float64) + x[..., i:i + m].astype(np.float64) * w[i:i + m].astype(np.float64)).astype(f32)
            else:
                p[..., :m] = p[..., :m] + t[..., i:i + m]
        while p.shape[-1] > 1:
            h = p.shape[-1] // 2
            p = p[..., :h] + p[..., h:] if mutant == "halving" else p[..., 0::2] + p[..., 1::2]
        return p[..., 0]


def bands32(amps, bank, power=False, mutant=None):
    """E: amps float32 (..., M + 1) -> float32 (..., B)"""
    x = x_of(amps, power)
    E = np.zeros(x.shape[:-1] + (bank.B,), f32)
    for b in range(bank.B):
        E[..., b] = s16(x[..., bank.first[b]:bank.first[b] + bank.count[b]], bank.w(b), mutant)
    return E


def log32(E, floor, mutant=None):
    with np.errstate(all="ignore"):
        m = np.maximum(E, f32(floor)) if mutant == "nan_no_floor" else np.fmax(E, f32(floor))
        return np.log(m.astype(f32))


def dct32(v, D, ncoef, mutant=None):
    """C_q, q < ncoef: the float32 sum of fl(D[q][b] v_b) from +0, ascending b"""
    v = np.asarray(v, f32)
    B = v.shape[-1]
    D = np.asarray(D, f32)
    acc = np.zeros(v.shape[:-1] + (ncoef,), f32)
    order = range(B - 1, -1, -1) if mutant == "dct_descending" else range(B)
    with np.errstate(all="ignore"):
        for b in order:
            acc = acc + D[:ncoef, b] * v[..., b:b + 1]
    return acc


def run32(amps, bank, D, power=False, log=False, ncoef=0, floor=1e-10, mutant=None):
    v = bands32(amps, bank, power, mutant)
    if log:
        v = log32(v, floor, mutant)
    return dct32(v, D, ncoef, mutant) if ncoef else v


# ---- float64 ----

def dct_table(B):
    """the header's D[q][b] in float64"""
    q, b = np.arange(B)[:, None], np.arange(B)[None, :]
    s = np.where(q == 0, np.sqrt(1.0 / B), np.sqrt(2.0 / B))
    return s * np.cos(np.pi * q * (2 * b + 1) / (2.0 * B))


def bands64(amps, bank, power=False):
    """(E, sum |t|) in float64 from the float32 amps and weights: the products exact, the squares not rounded"""
    a = np.asarray(amps, np.float64)
    x = a * a if power else a
    E = np.zeros(x.shape[:-1] + (bank.B,))
    A = np.zeros(E.shape)
    with np.errstate(all="ignore"):
        for b in range(bank.B):
            t = x[..., bank.first[b]:bank.first[b] + bank.count[b]] * bank.w(b).astype(np.float64)
            E[..., b], A[..., b] = t.sum(axis=-1), np.abs(t).sum(axis=-1)
    return E, A


def log64(E, floor):
    with np.errstate(all="ignore"):
        return np.log(np.fmax(np.asarray(E, np.float64), float(f32(floor))))


def dct64(v, D, ncoef):
    """(C, sum |D v|) in float64"""
    t = np.asarray(D, np.float64)[:ncoef] * np.asarray(v, np.float64)[..., None, :]
    return t.sum(axis=-1), np.abs(t).sum(axis=-1)


def gamma(n):
    return n * U / (1 - n * U)


# ---- the banks and inputs of the tests ----

def mel(size, nbands=40):
    import opencl_fft_amd as fa
    return Bank(*fa.Pvoc.mel_bank(size, SR, nbands))


def banks(size):
    """{name: Bank}: the 40-band mel bank; 256 random overlapping bands; one band; seventeen hand-made ones (not a multiple
    of the kernel's sixteen rows): counts 1, 15, 16, 17, 33 and M + 1, bin M alone, two identical bands, negative weights"""
    M = size // 2
    rng = np.random.default_rng(size + 7)
    out = {"mel": mel(size)}
    first = rng.integers(0, M + 1, 256)
    first[0] = 0   # one band over the low bins, where frames() puts a NaN
    count = np.minimum(rng.integers(1, 101, 256), M + 1 - first)
    count[0] = 33
    out["random256"] = Bank(first, count, rng.standard_normal(int(count.sum())).astype(f32))
    out["one"] = Bank([3], [M - 5], rng.uniform(0, 1, M - 5).astype(f32))
    hf = [5, 1, 7, 2, 0, 0, M, 2, 2]
    hc = [1, 15, 16, 17, 33, M + 1, 1, 20, 20]
    while len(hf) < 17:
        c = int(rng.integers(1, 30))
        hf.append(int(rng.integers(0, M + 2 - c)))
        hc.append(c)
    w = [rng.standard_normal(c).astype(f32) for c in hc]
    w[8] = w[7]
    w[3] = -np.abs(w[3])
    out["hand17"] = Bank(hf, hc, np.concatenate(w))
    for b in out.values():
        assert valid(M, *b.args())
    return out


def frames(size, seed=11):
    """(plain, odd): tests/pvoc_inputs.py's raw(size, 2, 9, seed, tilt, 3 decades), and a copy with a few NaN, inf, -0
    and negative amps"""
    from tests import pvoc_inputs
    plain = pvoc_inputs.raw(size, 2, 9, seed, tilt=True, decades=3)
    odd = np.array(plain)
    M = size // 2
    odd[0, 1, 4, 0] = np.nan
    odd[1, 2, M, 0] = np.nan
    odd[0, 3, 9, 0] = np.inf
    odd[1, 4, M - 1, 0] = -0.0
    odd[0, 5, 0, 0] = -0.0
    odd[1, 6, 2:20:3, 0] *= -1
    odd[0, 8, M // 2, 0] = -np.inf
    odd.setflags(write=False)
    return plain, odd
