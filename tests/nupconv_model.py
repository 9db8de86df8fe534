"""float64 model of the non-uniformly partitioned convolutions (clfa_nupconv, clfa_nupconv_matrix, include/clfft_amd.h)
that follows the schedule of nupconv_host.cpp literally, head block by head block, for the tests: one schedule (plain
blocks, the timed crossfade, its priming from the rings alone) for both objects, which differ in their row counts, the
shape of their responses and their multiply-accumulate; and the time-varying second input on top of it.  What the
schedule must meet is in tests/nupconv_definitions.py, which uses nothing of this file."""
import numpy as np

from tests.pconv_matrix_model import seg_bounds


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


def channel_mac(A, w, H, bins, level):
    """channels x len(bins) of the block in frame w of ring A (channels, ring, bins) under H (channels, n, bins): the sum
    over H's partitions, the oldest input block first (it meets the last partition)"""
    ring, n = A.shape[1], H.shape[1]
    acc = np.zeros((A.shape[0], len(bins)), np.complex128)
    for p in range(n):
        acc += A[:, (w - (n - 1) + p) % ring][:, bins] * H[:, n - 1 - p][:, bins]
    return acc


def matrix_mac(segs):
    """outputs x len(bins) of the block in frame w of ring A (inputs, ring, bins) under H (outputs, inputs, n, bins):
    frame (w - (n - 1) + p) mod ring of input i meets partition n - 1 - p of (o, i); the sequence r = i * n + p segment by
    segment (segs[level] of them), then the segments in order"""
    def mac(A, w, H, bins, level):
        ring, n = A.shape[1], H.shape[2]
        Y = np.zeros((H.shape[0], len(bins)), np.complex128)
        for r0, r1 in seg_bounds(A.shape[0] * n, segs[level]):
            part = np.zeros_like(Y)
            for r in range(r0, r1):
                i, p = divmod(r, n)
                part += A[i, (w - (n - 1) + p) % ring][bins] * H[:, i, n - 1 - p][:, bins]
            Y += part
        return Y
    return mac


class _Set:
    """what depends on the responses: their spectra, both levels' tails, the pending rows, the tail block's accumulators"""

    def __init__(self, lead, rows_out, n0, n1, pts0, pts1):
        self.H0 = np.zeros(lead + (n0, pts0 + 1), np.complex128)
        self.H1 = np.zeros(lead + (n1, pts1 + 1), np.complex128)
        self.clear(rows_out, pts0, pts1)
        self.Y1 = np.zeros((rows_out, pts1 + 1), np.complex128)

    def clear(self, rows_out, pts0, pts1):
        self.tail0, self.tail1, self.pend = np.zeros((rows_out, pts0)), np.zeros((rows_out, pts1)), np.zeros((rows_out, pts1))


class NupSchedule:
    """Head block c has phase s = c mod m in period P = c div m.  At phase 0 the stage rows (tail block P - 1 of every
    input row) are transformed into ring frame w1; every phase files its samples in the stage rows, computes slice s of
    tail block P - 1's bins, runs the head and adds the pending rows at the stream's position; after phase m - 1 the
    accumulators are inverse-transformed into the pending rows and w1 advances.

    One pair of input-spectra rings serves every response set; the tail's has n1 + `extra` frames, of which the sums walk
    the newest n1.  extra = 0 is enough for plain blocks; the objects have 2, which push_ir_fade needs to prime the second
    set from the rings alone; extra = 1 is there to show why.  During a fade both sets run and are mixed, and the two
    are exchanged when the fade's last block has run.

    `lead` is the shape of the response array in front of its samples and `mac(A, w, H, bins, level)` the
    multiply-accumulate: (channels,) with channel_mac, (outputs, inputs) with matrix_mac(segs)."""

    def __init__(self, cvs, pts0, pts1, rows_in, rows_out, lead, mac, extra=0):
        assert pts1 % pts0 == 0 and pts1 > pts0 and cvs >= 3 * pts1
        self.pts0, self.pts1, self.m, self.rows_in, self.rows_out = pts0, pts1, pts1 // pts0, rows_in, rows_out
        self.n0, self.n1 = 2 * self.m, (cvs - 2 * pts1) // pts1
        self.lead, self.mac, self.R = tuple(lead), mac, self.n1 + extra
        self.a = _Set(self.lead, rows_out, self.n0, self.n1, pts0, pts1)
        self.b = _Set(self.lead, rows_out, self.n0, self.n1, pts0, pts1)
        self.reset()

    H0 = property(lambda self: self.a.H0)   # the responses in use
    H1 = property(lambda self: self.a.H1)

    def reset(self):
        """the stream starts again; the responses stay"""
        self.A0 = np.zeros((self.rows_in, self.n0, self.pts0 + 1), np.complex128)
        self.A1 = np.zeros((self.rows_in, self.R, self.pts1 + 1), np.complex128)
        self.w0 = self.w1 = 0
        self.stage = np.zeros((self.rows_in, self.pts1))
        self.a.clear(self.rows_out, self.pts0, self.pts1)
        self.a.Y1[:] = 0
        self.position = 0
        self.fade_len = self.fade_done = 0

    def need(self):
        return 2 * self.pts1 + self.n1 * self.pts1

    def fade_remaining(self):
        return self.fade_len - self.fade_done

    def _spectra(self, S, ir):
        ir = np.asarray(ir, np.float64)
        if len(self.lead) == 1:
            ir = ir.reshape(self.lead + (-1,))
        assert ir.shape[:-1] == self.lead
        S.H0 = spectra(ir[..., :2 * self.pts1], self.pts0)
        S.H1 = spectra(ir[..., 2 * self.pts1:self.need()], self.pts1)

    def push_ir(self, ir):
        assert not self.fade_len, "CLFA_INVALID_OPERATION"
        self._spectra(self.a, ir)

    def slice_bins(self, s0, s1):
        """the bins of slices [s0, s1): items [s0 * pts0/2, s1 * pts0/2) of two bins; item 0 packs DC with Nyquist"""
        bins = list(range(s0 * self.pts0, s1 * self.pts0))
        return bins + [self.pts1] if s0 == 0 and s1 > 0 else bins

    def push_ir_fade(self, ir, fade_blocks):
        """the second set: the responses' spectra, then its history from the rings alone.  With P = c div m, s = c mod m:
        the head's tail from head block c - 1 (frame w0 - 1); the tail level's tail from tail block P - 3 (frame w1 - 2);
        the pending rows and the tail again from tail block P - 2 (frame w1 - 1); slices [0, s) of tail block P - 1
        (frame w1).  A block of negative index is not computed."""
        assert fade_blocks >= 1, "CLFA_INVALID_VALUE"
        assert not self.fade_len, "CLFA_INVALID_OPERATION"
        pts0, pts1, b, mac = self.pts0, self.pts1, self.b, self.mac
        P, s = divmod(self.position, self.m)
        self._spectra(b, ir)
        b.clear(self.rows_out, pts0, pts1)
        b.Y1[:] = np.nan          # nothing of the accumulators' past is used: every bin is written before its inverse
        all0, all1 = list(range(pts0 + 1)), list(range(pts1 + 1))
        if self.position >= 1:
            _, b.tail0 = olap(mac(self.A0, self.w0 - 1, b.H0, all0, 0), b.tail0, pts0)
        if P >= 3:
            _, b.tail1 = olap(mac(self.A1, self.w1 - 2, b.H1, all1, 1), b.tail1, pts1)
        if P >= 2:
            b.pend, b.tail1 = olap(mac(self.A1, self.w1 - 1, b.H1, all1, 1), b.tail1, pts1)
        if P >= 1 and s > 0:
            bins = self.slice_bins(0, s)
            b.Y1[:, bins] = mac(self.A1, self.w1, b.H1, bins, 1)
        self.fade_len, self.fade_done = int(fade_blocks), 0

    def _second_input(self, w):
        """what a block does with a time-varying second input before anything else: nothing here (NupTvModel)"""
        assert w is None

    def _block(self, x, w=None):
        pts0, pts1, m = self.pts0, self.pts1, self.m
        self._second_input(w)
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
                S.Y1[:, bins] = self.mac(self.A1, self.w1, S.H1, bins, 1)
            # the head: a uniformly partitioned block
            head, S.tail0 = olap(self.mac(self.A0, self.w0, S.H0, list(range(pts0 + 1)), 0), S.tail0, pts0)
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

    def process(self, x, w=None):
        """a call of K blocks is K blocks: (rows in, K * pts0) -> (rows out, K * pts0); w, of x's shape, is the
        time-varying second input of NupTvModel"""
        x = np.asarray(x, np.float64).reshape(self.rows_in, -1)
        K, n = x.shape[1] // self.pts0, self.pts0
        if not K:
            return np.zeros((self.rows_out, 0))
        if w is None:
            return np.concatenate([self._block(x[:, j * n:(j + 1) * n]) for j in range(K)], axis=1)
        w = np.asarray(w, np.float64).reshape(self.rows_in, -1)
        assert w.shape == x.shape
        return np.concatenate([self._block(x[:, j * n:(j + 1) * n], w[:, j * n:(j + 1) * n]) for j in range(K)], axis=1)


def NupModel(cvs, pts0, pts1, channels=1, extra=0):
    """Nupconv: a response and a chain of sums per channel"""
    return NupSchedule(cvs, pts0, pts1, channels, channels, (channels,), channel_mac, extra)


def NupFadeModel(cvs, pts0, pts1, channels=1, extra=2):
    """Nupconv with the object's tail ring of n1 + 2 frames (clfa_nupconv_push_ir_fade)"""
    return NupModel(cvs, pts0, pts1, channels, extra)


def NupMatrixModel(cvs, pts0, pts1, inputs, outputs, segs=(1, 1), extra=0):
    """NupconvMatrix: a response per (output, input), every bin of a level summed in segs[level] segments"""
    return NupSchedule(cvs, pts0, pts1, inputs, outputs, (outputs, inputs), matrix_mac(tuple(segs)), extra)


def NupMatrixFadeModel(cvs, pts0, pts1, inputs, outputs, segs=(1, 1), extra=2):
    """NupconvMatrix with the object's tail rings of n1 + 2 frames (clfa_nupconv_matrix_push_ir_fade)"""
    return NupMatrixModel(cvs, pts0, pts1, inputs, outputs, segs, extra)


class NupTvModel(NupSchedule):
    """Nupconv's time-varying second input (clfa_nupconv_process_tv_dev).  R1 = n1 + 2 tail blocks and R0 = R1 * m head
    blocks make one response period of L = R1 * pts1 samples.  A block with a second input w does steps 1 .. 4; a plain
    one (w None) steps 1 and 4, and spoils the tail block it falls into.  Step 4 is the schedule's block."""

    def __init__(self, cvs, pts0, pts1, channels=1):
        super().__init__(cvs, pts0, pts1, channels, channels, (channels,), channel_mac)
        self.R1 = self.n1 + 2
        self.R0 = self.R1 * self.m
        self.L = self.R1 * pts1

    def reset(self):
        super().reset()
        self.stage2 = np.zeros((self.rows_in, self.pts1))
        self.tv_count = 0

    def due(self):
        """step 1 at the position the next block has: the tail partition to rewrite, or None"""
        c, m = self.position, self.m
        if c % m or c < m:
            return None
        r = (c // m - 1) % self.R1
        return r - 2 if r >= 2 and self.tv_count == m else None

    def _second_input(self, w):
        c, m, pts0 = self.position, self.m, self.pts0
        q = self.due()
        if q is not None:
            self.H1[:, q] = spectra(self.stage2, self.pts1)[:, 0]
        if c % m == 0:
            self.tv_count = 0
        if w is not None:
            a = c % self.R0
            if a < self.n0:
                self.H0[:, a] = spectra(w, pts0)[:, 0]
            self.stage2[:, (c % m) * pts0:(c % m + 1) * pts0] = w
            self.tv_count += 1


def plain(h, x, cvs, pts0, pts1):
    """what a Nupconv that held h since its creation returns for x"""
    model = NupModel(cvs, pts0, pts1, x.shape[0])
    model.push_ir(h)
    return model.process(x)
