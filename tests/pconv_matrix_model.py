"""float64 model of the convolution matrix (clfa_pconv_matrix, include/clfft_amd.h) with the sub-batch algebra of
pconv_matrix.hip, for the tests."""
import numpy as np

from tests import util


def seg_bounds(total, segs):
    """the reduction's segments: [floor(s * total / segs), floor((s + 1) * total / segs))"""
    return [(total * s // segs, total * (s + 1) // segs) for s in range(segs)]


class MatrixModel:
    """One object under process calls, sub-batch by sub-batch of at most `cap` blocks.  Input of partition p for output j
    is m = j - (nparts - 1) + p: the sub-batch's X_i[m] for m >= 0, ring A_i frame (w + m) mod nparts before it; it meets
    response partition nparts - 1 - p.  Each output bin sums r = i * nparts + p over the segments, each segment on its own,
    then the segments in order.  The rings and tails change only after the whole sub-batch."""

    def __init__(self, nparts, pts, inputs, outputs, cap, segs=1):
        self.nparts, self.pts, self.inputs, self.outputs, self.cap, self.segs = nparts, pts, inputs, outputs, cap, segs
        self.A = np.zeros((inputs, nparts, pts + 1), np.complex128)
        self.H = np.zeros((outputs, inputs, nparts, pts + 1), np.complex128)
        self.tail = np.zeros((outputs, pts))
        self.wp = 0

    def spectra(self, x):
        x = np.asarray(x, np.float64)
        z = np.zeros(x.shape[:-1] + (x.shape[-1] // self.pts, 2 * self.pts))
        z[..., :self.pts] = x.reshape(x.shape[:-1] + (-1, self.pts))
        return np.fft.rfft(z, axis=-1)

    def push_ir(self, ir):
        self.H = self.spectra(np.asarray(ir)[:, :, :self.nparts * self.pts])

    def process(self, x):
        x = np.asarray(x, np.float64)
        n, pts, P = x.shape[1] // self.pts, self.pts, self.nparts
        out = np.zeros((self.outputs, n * pts))
        for j0 in range(0, n, self.cap):
            K = min(self.cap, n - j0)
            X = self.spectra(x[:, j0 * pts:(j0 + K) * pts])   # inputs x K x bins
            w = self.wp
            for j in range(K):
                for o in range(self.outputs):
                    Y = np.zeros(pts + 1, np.complex128)
                    for r0, r1 in seg_bounds(self.inputs * P, self.segs):
                        part = np.zeros(pts + 1, np.complex128)
                        for r in range(r0, r1):
                            i, p = divmod(r, P)
                            m = j - (P - 1) + p
                            F = X[i, m] if m >= 0 else self.A[i, (w + m) % P]
                            part += F * self.H[o, i, P - 1 - p]
                        Y += part
                    Y[0] *= 0.5   # the packed DC / Nyquist products' gain (tests/util.py, _olap64)
                    Y[pts] *= 0.5
                    y = np.fft.irfft(Y, n=2 * pts)
                    out[o, (j0 + j) * pts:(j0 + j + 1) * pts] = y[:pts] + self.tail[o]
                    self.tail[o] = y[pts:]
            for m in range(max(0, K - P), K):
                self.A[:, (w + m) % P] = X[:, m]
            self.wp = (w + K) % P
        return out


def truth_with_push(h1, h2, t_push, x, pts):
    """the definition with a push before block t_push: block t sums X_i[t - q] H_{o,i}[q] with h1's partitions for
    t < t_push and h2's after, and every block's second half carries into the next one (the tails are kept)"""
    X = util._block_spectra64(x.reshape(-1), pts).reshape(x.shape[0], -1, pts + 1)   # inputs x blocks x bins
    H1 = util._block_spectra64(h1.reshape(-1), pts).reshape(h1.shape[0], h1.shape[1], -1, pts + 1)
    H2 = util._block_spectra64(h2.reshape(-1), pts).reshape(h2.shape[0], h2.shape[1], -1, pts + 1)
    n, P = X.shape[1], H1.shape[2]
    out = []
    for o in range(h1.shape[0]):
        Y = np.zeros((n, pts + 1), np.complex128)
        for t in range(n):
            H = H1 if t < t_push else H2
            for q in range(min(P, t + 1)):
                Y[t] += np.sum(X[:, t - q] * H[o, :, q], axis=0)
        out.append(util._olap64(Y, pts))
    return np.stack(out)
