"""float64 model of NupconvMatrix with the timed crossfade of response changes (clfa_nupconv_matrix_push_ir_fade,
include/clfft_amd.h), following the schedule of nupconv_host.cpp literally, segments included: one pair of inputs' spectra
rings shared by both paths, the tail's of n1 + 2 frames per input; a second set of everything that depends on the
responses, primed at the push from the rings alone; the two sets exchanged when the fade's last block has run.  The
definition the fade must meet is `mixed` of two tests.nupconv_matrix_model.definition results."""
import numpy as np

from tests.nupconv_fade_model import mixed  # noqa: F401  (the definition's mix, shared with Nupconv's fade)
from tests.nupconv_model import olap, spectra
from tests.pconv_matrix_model import seg_bounds


class _Set:
    """what depends on the responses: their spectra, both levels' tails, the pending rows, the tail block's accumulators"""

    def __init__(self, O, I, n0, n1, pts0, pts1):
        self.H0 = np.zeros((O, I, n0, pts0 + 1), np.complex128)
        self.H1 = np.zeros((O, I, n1, pts1 + 1), np.complex128)
        self.clear(O, pts0, pts1)
        self.Y1 = np.zeros((O, pts1 + 1), np.complex128)

    def clear(self, O, pts0, pts1):
        self.tail0, self.tail1, self.pend = np.zeros((O, pts0)), np.zeros((O, pts1)), np.zeros((O, pts1))


class NupMatrixFadeModel:
    """NupMatrixModel's schedule (tests/nupconv_matrix_model.py) with a tail ring of n1 + `extra` frames per input, of
    which the sums walk the newest n1, and push_ir_fade.  extra = 2 is the object's; extra = 1 is there to show why."""

    def __init__(self, cvs, pts0, pts1, inputs, outputs, segs=(1, 1), extra=2):
        assert pts1 % pts0 == 0 and pts1 > pts0 and cvs >= 3 * pts1
        self.pts0, self.pts1, self.m, self.I, self.O = pts0, pts1, pts1 // pts0, inputs, outputs
        self.n0, self.n1 = 2 * self.m, (cvs - 2 * pts1) // pts1
        self.segs = tuple(segs)
        self.R = self.n1 + extra
        self.a = _Set(outputs, inputs, self.n0, self.n1, pts0, pts1)
        self.b = _Set(outputs, inputs, self.n0, self.n1, pts0, pts1)
        self.A0 = np.zeros((inputs, self.n0, pts0 + 1), np.complex128)
        self.A1 = np.zeros((inputs, self.R, pts1 + 1), np.complex128)
        self.w0 = self.w1 = 0
        self.stage = np.zeros((inputs, pts1))
        self.position = 0
        self.fade_len = self.fade_done = 0

    def need(self):
        return 2 * self.pts1 + self.n1 * self.pts1

    def fade_remaining(self):
        return self.fade_len - self.fade_done

    def _spectra(self, S, ir):
        ir = np.asarray(ir, np.float64)
        assert ir.shape[:2] == (self.O, self.I)
        S.H0 = spectra(ir[:, :, :2 * self.pts1], self.pts0)
        S.H1 = spectra(ir[:, :, 2 * self.pts1:self.need()], self.pts1)

    def push_ir(self, ir):
        assert not self.fade_len, "CLFA_INVALID_OPERATION"
        self._spectra(self.a, ir)

    def slice_bins(self, s0, s1):
        """the bins of slices [s0, s1): items [s0 * pts0/2, s1 * pts0/2) of two bins; item 0 packs DC with Nyquist"""
        bins = list(range(s0 * self.pts0, s1 * self.pts0))
        return bins + [self.pts1] if s0 == 0 and s1 > 0 else bins

    def _mac(self, A, H, w, bins, segs):
        """outputs x len(bins) of the block in frame w of ring A: frame (w - (n - 1) + p) mod ring of input i meets
        partition n - 1 - p of (o, i); the sequence r = i * n + p segment by segment, then the segments in order"""
        ring, n = A.shape[1], H.shape[2]
        Y = np.zeros((self.O, len(bins)), np.complex128)
        for r0, r1 in seg_bounds(self.I * n, segs):
            part = np.zeros_like(Y)
            for r in range(r0, r1):
                i, p = divmod(r, n)
                part += A[i, (w - (n - 1) + p) % ring][bins] * H[:, i, n - 1 - p][:, bins]
            Y += part
        return Y

    def push_ir_fade(self, ir, fade_blocks):
        """the second set: the responses' spectra, then its history from the rings alone.  With P = c div m, s = c mod m:
        the head's tail from head block c - 1 (frame w0 - 1); the tail level's tail from tail block P - 3 (frame w1 - 2);
        the pending rows and the tail again from tail block P - 2 (frame w1 - 1); slices [0, s) of tail block P - 1
        (frame w1).  A block of negative index is not computed."""
        assert fade_blocks >= 1, "CLFA_INVALID_VALUE"
        assert not self.fade_len, "CLFA_INVALID_OPERATION"
        pts0, pts1, b = self.pts0, self.pts1, self.b
        P, s = divmod(self.position, self.m)
        self._spectra(b, ir)
        b.clear(self.O, pts0, pts1)
        b.Y1[:] = np.nan          # nothing of the accumulators' past is used: every bin is written before its inverse
        all0, all1 = list(range(pts0 + 1)), list(range(pts1 + 1))
        if self.position >= 1:
            _, b.tail0 = olap(self._mac(self.A0, b.H0, self.w0 - 1, all0, self.segs[0]), b.tail0, pts0)
        if P >= 3:
            _, b.tail1 = olap(self._mac(self.A1, b.H1, self.w1 - 2, all1, self.segs[1]), b.tail1, pts1)
        if P >= 2:
            b.pend, b.tail1 = olap(self._mac(self.A1, b.H1, self.w1 - 1, all1, self.segs[1]), b.tail1, pts1)
        if P >= 1 and s > 0:
            bins = self.slice_bins(0, s)
            b.Y1[:, bins] = self._mac(self.A1, b.H1, self.w1, bins, self.segs[1])
        self.fade_len, self.fade_done = int(fade_blocks), 0

    def _block(self, x):
        pts0, pts1, m = self.pts0, self.pts1, self.m
        P, s = divmod(self.position, m)
        fading = self.fade_len > 0
        sets = [self.a, self.b] if fading else [self.a]
        # the shared part: the inputs' spectra, written once
        if P >= 1 and s == 0:
            self.A1[:, self.w1] = spectra(self.stage, pts1)[:, 0]
        self.stage[:, s * pts0:(s + 1) * pts0] = x
        self.A0[:, self.w0] = spectra(x, pts0)[:, 0]
        outs = []
        for S in sets:
            if P >= 1:
                bins = self.slice_bins(s, s + 1)
                S.Y1[:, bins] = self._mac(self.A1, S.H1, self.w1, bins, self.segs[1])
            head, S.tail0 = olap(self._mac(self.A0, S.H0, self.w0, list(range(pts0 + 1)), self.segs[0]), S.tail0, pts0)
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
        """a call of K blocks is K blocks: (inputs, K * pts0) -> (outputs, K * pts0)"""
        x = np.asarray(x, np.float64).reshape(self.I, -1)
        K = x.shape[1] // self.pts0
        if not K:
            return np.zeros((self.O, 0))
        return np.concatenate([self._block(x[:, j * self.pts0:(j + 1) * self.pts0]) for j in range(K)], axis=1)
