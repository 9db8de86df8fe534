"""float64 model of the non-uniformly partitioned convolution (clfa_nupconv, include/clfft_amd.h) that follows the schedule
of nupconv_host.cpp / pconv_nup.hip literally, head block by head block, for the tests; and the definition it must meet."""
import numpy as np

from tests import util


def spectra(x, pts):
    """rfft of every pts-sample block of the last axis, zero-padded to 2 pts"""
    x = np.asarray(x, np.float64)
    z = np.zeros(x.shape[:-1] + (x.shape[-1] // pts, 2 * pts))
    z[..., :pts] = x.reshape(x.shape[:-1] + (-1, pts))
    return np.fft.rfft(z, axis=-1)


def olap(Y, tail, pts):
    """one block: the packed DC / Nyquist products' gain (tests/util.py, _olap64), inverse transform, overlap-add;
    returns (samples, new tail)"""
    Y = Y.copy()
    Y[..., 0] *= 0.5
    Y[..., pts] *= 0.5
    y = np.fft.irfft(Y, n=2 * pts, axis=-1)
    return y[..., :pts] + tail, y[..., pts:]


class NupModel:
    """Head block c has phase s = c mod m in period P = c div m.  At phase 0 the stage row (tail block P - 1) is
    transformed into ring frame w; every phase files its samples in the stage row, computes slice s of tail block
    P - 1's bins over all n1 partitions, runs the head and adds the pending row at the stream's position; after phase
    m - 1 the accumulators are inverse-transformed into the pending row and w advances."""

    def __init__(self, cvs, pts0, pts1, channels=1):
        assert pts1 % pts0 == 0 and pts1 > pts0 and cvs >= 3 * pts1
        self.pts0, self.pts1, self.m, self.ch = pts0, pts1, pts1 // pts0, channels
        self.n0, self.n1 = 2 * self.m, (cvs - 2 * pts1) // pts1
        self.H0 = np.zeros((channels, self.n0, pts0 + 1), np.complex128)
        self.H1 = np.zeros((channels, self.n1, pts1 + 1), np.complex128)
        self.reset()

    def reset(self):
        ch, pts0, pts1 = self.ch, self.pts0, self.pts1
        self.A0 = np.zeros((ch, self.n0, pts0 + 1), np.complex128)
        self.A1 = np.zeros((ch, self.n1, pts1 + 1), np.complex128)
        self.w0 = self.w1 = 0
        self.tail0, self.tail1 = np.zeros((ch, pts0)), np.zeros((ch, pts1))
        self.stage, self.pend = np.zeros((ch, pts1)), np.zeros((ch, pts1))
        self.Y1 = np.zeros((ch, pts1 + 1), np.complex128)
        self.position = 0

    def need(self):
        return 2 * self.pts1 + self.n1 * self.pts1

    def push_ir(self, ir):
        ir = np.asarray(ir, np.float64).reshape(self.ch, -1)
        self.H0 = spectra(ir[:, :2 * self.pts1], self.pts0)
        self.H1 = spectra(ir[:, 2 * self.pts1:self.need()], self.pts1)

    def slice_bins(self, s):
        """the bins of slice s: items [s * pts0/2, (s+1) * pts0/2) of two bins; item 0 packs DC with Nyquist"""
        bins = list(range(s * self.pts0, (s + 1) * self.pts0))
        return bins + [self.pts1] if s == 0 else bins

    def _block(self, x):
        pts0, m, n0, n1 = self.pts0, self.m, self.n0, self.n1
        P, s = divmod(self.position, m)
        if P >= 1 and s == 0:
            self.A1[:, self.w1] = spectra(self.stage, self.pts1)[:, 0]
        self.stage[:, s * pts0:(s + 1) * pts0] = x
        if P >= 1:
            b = self.slice_bins(s)
            acc = np.zeros((self.ch, len(b)), np.complex128)
            for p in range(n1):   # the oldest input block first: it meets the last partition
                acc += self.A1[:, (self.w1 - (n1 - 1) + p) % n1][:, b] * self.H1[:, n1 - 1 - p][:, b]
            self.Y1[:, b] = acc
        # the head: a uniformly partitioned block
        self.A0[:, self.w0] = spectra(x, pts0)[:, 0]
        Y = np.zeros((self.ch, pts0 + 1), np.complex128)
        for p in range(n0):
            Y += self.A0[:, (self.w0 - (n0 - 1) + p) % n0] * self.H0[:, n0 - 1 - p]
        self.w0 = (self.w0 + 1) % n0
        head, self.tail0 = olap(Y, self.tail0, pts0)
        out = head + self.pend[:, s * pts0:(s + 1) * pts0]
        if P >= 1 and s == m - 1:
            self.pend, self.tail1 = olap(self.Y1, self.tail1, self.pts1)
            self.w1 = (self.w1 + 1) % n1
        self.position += 1
        return out

    def process(self, x):
        """a call of K blocks is K blocks: (channels, K * pts0) -> (channels, K * pts0)"""
        x = np.asarray(x, np.float64).reshape(self.ch, -1)
        K = x.shape[1] // self.pts0
        if not K:
            return np.zeros((self.ch, 0))
        return np.concatenate([self._block(x[:, j * self.pts0:(j + 1) * self.pts0]) for j in range(K)], axis=1)


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
