"""float64 model of the non-uniformly partitioned convolution matrix (clfa_nupconv_matrix, include/clfft_amd.h) that follows
the schedule of nupconv_host.cpp / pconv_nupm.hip literally, head block by head block, segments included; and the definition
it must meet: two MatrixModel objects, the tail's output delayed by 2 * pts1."""
import numpy as np

from tests.nupconv_model import olap, spectra
from tests.pconv_matrix_model import MatrixModel, seg_bounds


class NupMatrixModel:
    """Head block c has phase s = c mod m in period P = c div m.  At phase 0 the stage rows (tail block P - 1 of every
    input) are transformed into ring frame w; every phase files its samples in the stage rows, computes slice s of tail
    block P - 1's bins for every output, runs the head and adds the pending rows at the stream's position; after phase
    m - 1 the accumulators are inverse-transformed into the pending rows and w advances.  Every bin of a level sums the
    sequence r = i * nparts + p segment by segment, then the segments in order."""

    def __init__(self, cvs, pts0, pts1, inputs, outputs, segs=(1, 1)):
        assert pts1 % pts0 == 0 and pts1 > pts0 and cvs >= 3 * pts1
        self.pts0, self.pts1, self.m, self.I, self.O = pts0, pts1, pts1 // pts0, inputs, outputs
        self.n0, self.n1 = 2 * self.m, (cvs - 2 * pts1) // pts1
        self.segs = tuple(segs)
        self.H0 = np.zeros((outputs, inputs, self.n0, pts0 + 1), np.complex128)
        self.H1 = np.zeros((outputs, inputs, self.n1, pts1 + 1), np.complex128)
        self.reset()

    def reset(self):
        self.A0 = np.zeros((self.I, self.n0, self.pts0 + 1), np.complex128)
        self.A1 = np.zeros((self.I, self.n1, self.pts1 + 1), np.complex128)
        self.w0 = self.w1 = 0
        self.tail0, self.tail1 = np.zeros((self.O, self.pts0)), np.zeros((self.O, self.pts1))
        self.stage, self.pend = np.zeros((self.I, self.pts1)), np.zeros((self.O, self.pts1))
        self.Y1 = np.zeros((self.O, self.pts1 + 1), np.complex128)
        self.position = 0

    def need(self):
        return 2 * self.pts1 + self.n1 * self.pts1

    def push_ir(self, ir):
        ir = np.asarray(ir, np.float64)
        assert ir.shape[:2] == (self.O, self.I)
        self.H0 = spectra(ir[:, :, :2 * self.pts1], self.pts0)
        self.H1 = spectra(ir[:, :, 2 * self.pts1:self.need()], self.pts1)

    def slice_bins(self, s):
        """the bins of slice s: items [s * pts0/2, (s+1) * pts0/2) of two bins; item 0 packs DC with Nyquist"""
        bins = list(range(s * self.pts0, (s + 1) * self.pts0))
        return bins + [self.pts1] if s == 0 else bins

    def _mac(self, A, H, w, bins, segs):
        """outputs x len(bins): frame (w - (P - 1) + p) mod P of input i meets partition P - 1 - p of (o, i)"""
        P = A.shape[1]
        Y = np.zeros((self.O, len(bins)), np.complex128)
        for r0, r1 in seg_bounds(self.I * P, segs):
            part = np.zeros_like(Y)
            for r in range(r0, r1):
                i, p = divmod(r, P)
                part += A[i, (w - (P - 1) + p) % P][bins] * H[:, i, P - 1 - p][:, bins]
            Y += part
        return Y

    def _block(self, x):
        pts0, m = self.pts0, self.m
        P, s = divmod(self.position, m)
        if P >= 1 and s == 0:
            self.A1[:, self.w1] = spectra(self.stage, self.pts1)[:, 0]
        self.stage[:, s * pts0:(s + 1) * pts0] = x
        if P >= 1:
            b = self.slice_bins(s)
            self.Y1[:, b] = self._mac(self.A1, self.H1, self.w1, b, self.segs[1])
        self.A0[:, self.w0] = spectra(x, pts0)[:, 0]
        Y = self._mac(self.A0, self.H0, self.w0, list(range(pts0 + 1)), self.segs[0])
        self.w0 = (self.w0 + 1) % self.n0
        head, self.tail0 = olap(Y, self.tail0, pts0)
        out = head + self.pend[:, s * pts0:(s + 1) * pts0]
        if P >= 1 and s == m - 1:
            self.pend, self.tail1 = olap(self.Y1, self.tail1, self.pts1)
            self.w1 = (self.w1 + 1) % self.n1
        self.position += 1
        return out

    def process(self, x):
        """a call of K blocks is K blocks: (inputs, K * pts0) -> (outputs, K * pts0)"""
        x = np.asarray(x, np.float64).reshape(self.I, -1)
        K = x.shape[1] // self.pts0
        if not K:
            return np.zeros((self.O, 0))
        return np.concatenate([self._block(x[:, j * self.pts0:(j + 1) * self.pts0]) for j in range(K)], axis=1)


def delayed_tails(yt, pts1, length):
    """yt[:, n - 2*pts1] for n < length, zero before"""
    out = np.zeros((yt.shape[0], length))
    n = max(0, min(length - 2 * pts1, yt.shape[1]))
    out[:, 2 * pts1:2 * pts1 + n] = yt[:, :n]
    return out


def definition(h, x, cvs, pts0, pts1, segs=(1, 1), push=None):
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
