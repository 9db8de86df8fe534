"""float64 model of the convolution matrix's timed crossfade (clfa_pconv_matrix_push_ir_fade, include/clfft_amd.h) with
the algebra of pconv_matrix.hip, on top of MatrixModel: one shared ring, a second response set whose tails are primed from
the ring at the push, sub-batches cut at the fade's end, the second set copied over the first after the last fade block."""
import numpy as np

from tests.pconv_matrix_model import MatrixModel, seg_bounds


def ramp(n0, count, N):
    """g(n) = n / N for the samples n0 .. n0 + count - 1 of a fade of N samples"""
    return (n0 + np.arange(count)) / float(N)


class FadeModel(MatrixModel):
    def __init__(self, nparts, pts, inputs, outputs, cap, segs=1):
        MatrixModel.__init__(self, nparts, pts, inputs, outputs, cap, segs)
        self.H2, self.tail2 = None, np.zeros((outputs, pts))
        self.fade_len = self.fade_done = 0

    def fade_remaining(self):
        return self.fade_len - self.fade_done

    def _block(self, H, X, w, j, o):
        """both halves of block j of output o under H: input frames from X (m >= 0) and the ring before the sub-batch"""
        P, pts = self.nparts, self.pts
        Y = np.zeros(pts + 1, np.complex128)
        for r0, r1 in seg_bounds(self.inputs * P, self.segs):
            part = np.zeros(pts + 1, np.complex128)
            for r in range(r0, r1):
                i, p = divmod(r, P)
                m = j - (P - 1) + p
                F = X[i, m] if m >= 0 else self.A[i, (w + m) % P]
                part += F * H[o, i, P - 1 - p]
            Y += part
        Y[0] *= 0.5
        Y[pts] *= 0.5
        y = np.fft.irfft(Y, n=2 * pts)
        return y[:pts], y[pts:]

    def push_ir(self, ir):
        if self.fade_remaining():
            raise RuntimeError("a fade is pending")
        MatrixModel.push_ir(self, ir)

    def push_ir_fade(self, ir, fade_blocks):
        if fade_blocks < 1:
            raise ValueError("fade_blocks")
        if self.fade_remaining():
            raise RuntimeError("a fade is pending")
        self.H2 = self.spectra(np.asarray(ir)[:, :, :self.nparts * self.pts])
        # the second path's tail: block -1 under the new responses, from the nparts frames the ring holds
        for o in range(self.outputs):
            self.tail2[o] = self._block(self.H2, None, self.wp, -1, o)[1]
        self.fade_len, self.fade_done = int(fade_blocks), 0

    def process(self, x):
        x = np.asarray(x, np.float64)
        n, pts, P = x.shape[1] // self.pts, self.pts, self.nparts
        out = np.zeros((self.outputs, n * pts))
        j0 = 0
        while j0 < n:
            fade = self.fade_remaining()
            K = min(self.cap, n - j0)
            if fade:
                K = min(K, fade)   # a sub-batch lies wholly inside or wholly outside a fade
            X = self.spectra(x[:, j0 * pts:(j0 + K) * pts])
            w = self.wp
            for j in range(K):
                sl = slice((j0 + j) * pts, (j0 + j + 1) * pts)
                for o in range(self.outputs):
                    a, self_tail = self._block(self.H, X, w, j, o)
                    a = a + self.tail[o]
                    self.tail[o] = self_tail
                    if fade:
                        b, t2 = self._block(self.H2, X, w, j, o)
                        b = b + self.tail2[o]
                        self.tail2[o] = t2
                        g = ramp((self.fade_done + j) * pts, pts, self.fade_len * pts)
                        a = a + g * (b - a)
                    out[o, sl] = a
            for m in range(max(0, K - P), K):
                self.A[:, (w + m) % P] = X[:, m]
            self.wp = (w + K) % P
            if fade:
                self.fade_done += K
                if self.fade_done == self.fade_len:
                    self.H, self.tail = self.H2.copy(), self.tail2.copy()
                    self.fade_len = self.fade_done = 0
            j0 += K
        return out


def definition(ir_a, ir_b, x, t_push, fade_blocks, pts, nparts, model=None):
    """the definition itself: two objects fed alike from the first block, one holding A and one B, mixed by g from block
    t_push on and B alone after the fade.  model(ir) -> the (outputs, L) output of an object holding ir for x."""
    if model is None:
        def model(ir):
            m = MatrixModel(nparts, pts, ir.shape[1], ir.shape[0], cap=x.shape[1] // pts)
            m.push_ir(ir)
            return m.process(x)
    ya, yb = np.asarray(model(ir_a), np.float64), np.asarray(model(ir_b), np.float64)
    out = ya.copy()
    n0, N = t_push * pts, fade_blocks * pts
    cnt = min(N, x.shape[1] - n0)
    g = ramp(0, cnt, N)
    out[:, n0:n0 + cnt] = ya[:, n0:n0 + cnt] + g * (yb[:, n0:n0 + cnt] - ya[:, n0:n0 + cnt])
    out[:, n0 + cnt:] = yb[:, n0 + cnt:]
    return out
