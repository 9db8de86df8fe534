"""float64 model of Nupconv with the timed crossfade of response changes (clfa_nupconv_push_ir_fade, include/clfft_amd.h),
following the schedule of nupconv_host.cpp literally: one pair of input-spectra rings shared by both paths, the tail's of
n1 + 2 frames; a second set of everything that depends on the responses, primed at the push from the rings alone; the two
sets exchanged when the fade's last block has run.  And the definition the fade must meet: two objects fed alike, mixed."""
import numpy as np

from tests.nupconv_model import NupModel, olap, spectra


class _Set:
    """what depends on the responses: their spectra, both levels' tails, the pending row, the tail block's accumulators"""

    def __init__(self, ch, n0, n1, pts0, pts1):
        self.H0 = np.zeros((ch, n0, pts0 + 1), np.complex128)
        self.H1 = np.zeros((ch, n1, pts1 + 1), np.complex128)
        self.clear(ch, pts0, pts1)
        self.Y1 = np.zeros((ch, pts1 + 1), np.complex128)

    def clear(self, ch, pts0, pts1):
        self.tail0, self.tail1, self.pend = np.zeros((ch, pts0)), np.zeros((ch, pts1)), np.zeros((ch, pts1))


class NupFadeModel:
    """NupModel's schedule (tests/nupconv_model.py) with a tail ring of n1 + `extra` frames, of which the sums walk the
    newest n1, and push_ir_fade.  extra = 2 is the object's; extra = 1 is there to show why."""

    def __init__(self, cvs, pts0, pts1, channels=1, extra=2):
        assert pts1 % pts0 == 0 and pts1 > pts0 and cvs >= 3 * pts1
        self.pts0, self.pts1, self.m, self.ch = pts0, pts1, pts1 // pts0, channels
        self.n0, self.n1 = 2 * self.m, (cvs - 2 * pts1) // pts1
        self.R = self.n1 + extra
        self.a = _Set(channels, self.n0, self.n1, pts0, pts1)
        self.b = _Set(channels, self.n0, self.n1, pts0, pts1)
        self.A0 = np.zeros((channels, self.n0, pts0 + 1), np.complex128)
        self.A1 = np.zeros((channels, self.R, pts1 + 1), np.complex128)
        self.w0 = self.w1 = 0
        self.stage = np.zeros((channels, pts1))
        self.position = 0
        self.fade_len = self.fade_done = 0

    def need(self):
        return 2 * self.pts1 + self.n1 * self.pts1

    def fade_remaining(self):
        return self.fade_len - self.fade_done

    def _spectra(self, S, ir):
        ir = np.asarray(ir, np.float64).reshape(self.ch, -1)
        S.H0 = spectra(ir[:, :2 * self.pts1], self.pts0)
        S.H1 = spectra(ir[:, 2 * self.pts1:self.need()], self.pts1)

    def push_ir(self, ir):
        assert not self.fade_len, "CLFA_INVALID_OPERATION"
        self._spectra(self.a, ir)

    def slice_bins(self, s0, s1):
        """the bins of slices [s0, s1): items [s0 * pts0/2, s1 * pts0/2) of two bins; item 0 packs DC with Nyquist"""
        bins = list(range(s0 * self.pts0, s1 * self.pts0))
        return bins + [self.pts1] if s0 == 0 and s1 > 0 else bins

    @staticmethod
    def _mac(A, w, H, bins):
        """the block in frame w of ring A: the sum over H's partitions, the oldest input block first"""
        ring, n = A.shape[1], H.shape[1]
        acc = np.zeros((A.shape[0], len(bins)), np.complex128)
        for p in range(n):
            acc += A[:, (w - (n - 1) + p) % ring][:, bins] * H[:, n - 1 - p][:, bins]
        return acc

    def push_ir_fade(self, ir, fade_blocks):
        """the second set: the responses' spectra, then its history from the rings alone.  With P = c div m, s = c mod m:
        the head's tail from head block c - 1 (frame w0 - 1); the tail level's tail from tail block P - 3 (frame w1 - 2);
        the pending row and the tail again from tail block P - 2 (frame w1 - 1); slices [0, s) of tail block P - 1
        (frame w1).  A block of negative index is not computed."""
        assert fade_blocks >= 1, "CLFA_INVALID_VALUE"
        assert not self.fade_len, "CLFA_INVALID_OPERATION"
        pts0, pts1, b = self.pts0, self.pts1, self.b
        P, s = divmod(self.position, self.m)
        self._spectra(b, ir)
        b.clear(self.ch, pts0, pts1)
        b.Y1[:] = np.nan          # nothing of the accumulators' past is used: every bin is written before its inverse
        all0, all1 = list(range(pts0 + 1)), list(range(pts1 + 1))
        if self.position >= 1:
            _, b.tail0 = olap(self._mac(self.A0, self.w0 - 1, b.H0, all0), b.tail0, pts0)
        if P >= 3:
            _, b.tail1 = olap(self._mac(self.A1, self.w1 - 2, b.H1, all1), b.tail1, pts1)
        if P >= 2:
            b.pend, b.tail1 = olap(self._mac(self.A1, self.w1 - 1, b.H1, all1), b.tail1, pts1)
        if P >= 1 and s > 0:
            bins = self.slice_bins(0, s)
            b.Y1[:, bins] = self._mac(self.A1, self.w1, b.H1, bins)
        self.fade_len, self.fade_done = int(fade_blocks), 0

    def _block(self, x):
        pts0, pts1, m = self.pts0, self.pts1, self.m
        P, s = divmod(self.position, m)
        fading = self.fade_len > 0
        sets = [self.a, self.b] if fading else [self.a]
        # the shared part: the input spectra, written once
        if P >= 1 and s == 0:
            self.A1[:, self.w1] = spectra(self.stage, pts1)[:, 0]
        self.stage[:, s * pts0:(s + 1) * pts0] = x
        self.A0[:, self.w0] = spectra(x, pts0)[:, 0]
        outs = []
        for S in sets:
            if P >= 1:
                bins = self.slice_bins(s, s + 1)
                S.Y1[:, bins] = self._mac(self.A1, self.w1, S.H1, bins)
            head, S.tail0 = olap(self._mac(self.A0, self.w0, S.H0, list(range(pts0 + 1))), S.tail0, pts0)
            outs.append(head + S.pend[:, s * pts0:(s + 1) * pts0])
        self.w0 = (self.w0 + 1) % self.n0
        out = outs[0]
        if fading:
            g = (self.fade_done * pts0 + np.arange(pts0)) / (self.fade_len * pts0)
            out = outs[0] + g * (outs[1] - outs[0])
        if P >= 1 and s == m - 1:
            for S in sets:
                S.pend, S.tail1 = olap(S.Y1, S.tail1, pts1)
            self.w1 = (self.w1 + 1) % self.R
        self.position += 1
        if fading:
            self.fade_done += 1
            if self.fade_done == self.fade_len:      # the exchange: the second set is the first from here on
                self.a, self.b = self.b, self.a
                self.fade_len = self.fade_done = 0
        return out

    def process(self, x):
        x = np.asarray(x, np.float64).reshape(self.ch, -1)
        K = x.shape[1] // self.pts0
        if not K:
            return np.zeros((self.ch, 0))
        return np.concatenate([self._block(x[:, j * self.pts0:(j + 1) * self.pts0]) for j in range(K)], axis=1)


def plain(h, x, cvs, pts0, pts1):
    """what an object that held h since its creation returns for x"""
    model = NupModel(cvs, pts0, pts1, x.shape[0])
    model.push_ir(h)
    return model.process(x)


def mixed(ya, yb, c, fade_blocks, pts0):
    """the definition: ya before sample c * pts0, ya + g * (yb - ya) over the next N = fade_blocks * pts0, yb after them"""
    n0, N = c * pts0, fade_blocks * pts0
    out = np.array(ya)
    out[:, n0:n0 + N] = ya[:, n0:n0 + N] + (np.arange(N) / N) * (yb[:, n0:n0 + N] - ya[:, n0:n0 + N])
    out[:, n0 + N:] = yb[:, n0 + N:]
    return out
