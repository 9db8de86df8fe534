"""What the non-uniformly partitioned convolutions must meet, in float64 and without a line of their schedule
(tests/nupconv_model.py): Nupconv from tests/util.pconv_f64, NupconvMatrix from two MatrixModel objects, the timed
crossfade as a mix of two such results, the time-varying second input as a composition of pushes and as a closed-form
impulse readout."""
import numpy as np

from tests import util
from tests.pconv_matrix_model import MatrixModel


def delayed_tail(yt, pts1, length):
    """yt[n - 2*pts1] for n < length, zero before"""
    out = np.zeros(length)
    n = max(0, min(length - 2 * pts1, yt.size))
    out[2 * pts1:2 * pts1 + n] = yt[:n]
    return out


def definition(h, x, cvs, pts0, pts1):
    """one channel in float64: pconv_f64(h[:2*pts1], x, pts0) + pconv_f64(h[2*pts1:cvs], x, pts1) delayed by 2*pts1 (x is
    padded with zeros to whole tail blocks for the second term: the convolution is causal)"""
    h, x = np.asarray(h, np.float64), np.asarray(x, np.float64)
    yh = util.pconv_f64(h[:2 * pts1], x, pts0)
    xp = np.zeros(-(-x.size // pts1) * pts1)
    xp[:x.size] = x
    yt = util.pconv_f64(h[2 * pts1:cvs], xp, pts1)
    return yh + delayed_tail(yt, pts1, x.size)


def delayed_tails(yt, pts1, length):
    """yt[:, n - 2*pts1] for n < length, zero before"""
    out = np.zeros((yt.shape[0], length))
    n = max(0, min(length - 2 * pts1, yt.shape[1]))
    out[:, 2 * pts1:2 * pts1 + n] = yt[:, :n]
    return out


def matrix_definition(h, x, cvs, pts0, pts1, segs=(1, 1), push=None):
    """(outputs, L) in float64 from two MatrixModel objects: the head on h[:, :, :2*pts1] in partitions of pts0, the tail on
    h[:, :, 2*pts1:cvs] in partitions of pts1 (x padded with zeros to whole tail blocks: the convolution is causal), the
    tail's output delayed by 2*pts1.  push = (h2, head blocks before it, tail blocks before it)."""
    h, x = np.asarray(h, np.float64), np.asarray(x, np.float64)
    O, I = h.shape[:2]
    n1 = (cvs - 2 * pts1) // pts1
    xp = np.zeros((I, -(-x.shape[1] // pts1) * pts1))
    xp[:, :x.shape[1]] = x
    head = MatrixModel(2 * pts1 // pts0, pts0, I, O, cap=5, segs=segs[0])
    tail = MatrixModel(n1, pts1, I, O, cap=3, segs=segs[1])
    head.push_ir(h[:, :, :2 * pts1])
    tail.push_ir(h[:, :, 2 * pts1:cvs])
    if push is None:
        yh, yt = head.process(x), tail.process(xp)
    else:
        h2, cb, tb = push
        h2 = np.asarray(h2, np.float64)
        ya, ta = head.process(x[:, :cb * pts0]), tail.process(xp[:, :tb * pts1])
        head.push_ir(h2[:, :, :2 * pts1])
        tail.push_ir(h2[:, :, 2 * pts1:cvs])
        yh = np.concatenate([ya, head.process(x[:, cb * pts0:])], axis=1)
        yt = np.concatenate([ta, tail.process(xp[:, tb * pts1:])], axis=1)
    return yh + delayed_tails(yt, pts1, x.shape[1])


def mixed(ya, yb, c, fade_blocks, pts0):
    """the fade: ya before sample c * pts0, ya + g * (yb - ya) over the next N = fade_blocks * pts0, yb after them"""
    n0, N = c * pts0, fade_blocks * pts0
    out = np.array(ya)
    out[:, n0:n0 + N] = ya[:, n0:n0 + N] + (np.arange(N) / N) * (yb[:, n0:n0 + N] - ya[:, n0:n0 + N])
    out[:, n0 + N:] = yb[:, n0 + N:]
    return out


class Composition:
    """the time-varying second input: a plain object beside a response array hc; before each head block hc is rewritten
    by steps 1 and 2 and, whenever it changed, pushed; then the block is processed as a plain one.  `plain` is the plain
    object (push_ir(rows) and process(x) -> samples); the bookkeeping of steps 1 .. 3 is this class's own"""

    def __init__(self, plain, pts0, pts1, n1, channels, ir=None):
        self.p, self.pts0, self.pts1, self.m, self.n1, self.ch = plain, pts0, pts1, pts1 // pts0, n1, channels
        self.R1, self.R0, self.L = n1 + 2, (n1 + 2) * (pts1 // pts0), (n1 + 2) * pts1
        self.hc = np.zeros((channels, self.L), np.float32) if ir is None else np.array(ir, np.float32).reshape(channels, -1)[:, :self.L]
        self.stage2 = np.zeros((channels, pts1), np.float32)
        self.tv_count = self.c = 0

    def block(self, x, w=None):
        c, m, pts0, pts1 = self.c, self.m, self.pts0, self.pts1
        changed = False
        if c % m == 0:
            if c >= m:
                r = (c // m - 1) % self.R1
                if r >= 2 and self.tv_count == m:
                    self.hc[:, r * pts1:(r + 1) * pts1] = self.stage2
                    changed = True
            self.tv_count = 0
        if w is not None:
            a = c % self.R0
            if a < 2 * m:
                self.hc[:, a * pts0:(a + 1) * pts0] = w
                changed = True
            self.stage2[:, (c % m) * pts0:(c % m + 1) * pts0] = w
            self.tv_count += 1
        if changed:
            self.p.push_ir(self.hc)
        self.c += 1
        return self.p.process(x)

    def run(self, x, w, plain=()):
        """the whole stream, block by block; the head blocks listed in `plain` go without their second input"""
        n = self.pts0
        return np.concatenate([self.block(x[:, j * n:(j + 1) * n], None if j in plain else w[:, j * n:(j + 1) * n])
                               for j in range(x.shape[1] // n)], axis=1)


def readout_stream(L, nsamples):
    """w[j] = (1 + j div 4) * (1, 1, -1, -1)[j mod 4] for j < L, repeated with period L: no block of it has DC or Nyquist
    content at either level, so the half gain of the packed bins stays out"""
    j = np.arange(L)
    return np.resize((1 + j // 4) * np.array([1.0, 1.0, -1.0, -1.0])[j % 4], nsamples)


def readout(w, b, s, pts0, pts1, n1):
    """x = one unit sample at block b, sample s: y[b * pts0 + s + k] = v(k), 0 <= k < L, read from the stream w"""
    m, R1 = pts1 // pts0, n1 + 2
    R0, L = R1 * m, R1 * pts1
    v = np.zeros(L)
    for k in range(L):
        if k < 2 * pts1:
            a = k // pts0
            c = b + a
            u = c - ((c - a) % R0)
            v[k] = w[u * pts0 + k % pts0] if u >= 0 else 0.0
        else:
            q = k // pts1 - 2
            T = b // m + q
            U = T - ((T - q - 2) % R1)
            v[k] = w[U * pts1 + k % pts1] if U >= 0 else 0.0
    return v
