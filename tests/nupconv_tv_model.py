"""float64 model of Nupconv's time-varying second input (clfa_nupconv_process_tv_dev, include/clfft_amd.h): NupModel with
the four steps of a time-varying block, the push composition that defines its bits, and the closed-form impulse readout."""
import numpy as np

from tests.nupconv_model import NupModel, spectra


class NupTvModel(NupModel):
    """R1 = n1 + 2 tail blocks and R0 = R1 * m head blocks make one response period of L = R1 * pts1 samples.  A block
    with a second input w does steps 1 .. 4; a plain one (w None) steps 1 and 4, and spoils the tail block it falls into."""

    def __init__(self, cvs, pts0, pts1, channels=1):
        super().__init__(cvs, pts0, pts1, channels)
        self.R1 = self.n1 + 2
        self.R0 = self.R1 * self.m
        self.L = self.R1 * pts1

    def reset(self):
        super().reset()
        self.stage2 = np.zeros((self.ch, self.pts1))
        self.tv_count = 0

    def due(self):
        """step 1 at the position the next block has: the tail partition to rewrite, or None"""
        c, m = self.position, self.m
        if c % m or c < m:
            return None
        r = (c // m - 1) % self.R1
        return r - 2 if r >= 2 and self.tv_count == m else None

    def _block(self, x, w=None):
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
        return super()._block(x)

    def process(self, x, w=None):
        """a call of K blocks is K blocks: (channels, K * pts0) each -> (channels, K * pts0)"""
        x = np.asarray(x, np.float64).reshape(self.ch, -1)
        K, n = x.shape[1] // self.pts0, self.pts0
        if not K:
            return np.zeros((self.ch, 0))
        if w is None:
            return np.concatenate([self._block(x[:, j * n:(j + 1) * n]) for j in range(K)], axis=1)
        w = np.asarray(w, np.float64).reshape(self.ch, -1)
        assert w.shape == x.shape
        return np.concatenate([self._block(x[:, j * n:(j + 1) * n], w[:, j * n:(j + 1) * n]) for j in range(K)], axis=1)


class Composition:
    """the definition: a plain object beside a response array hc; before each head block hc is rewritten by steps 1 and
    2 and, whenever it changed, pushed; then the block is processed as a plain one.  `make` builds the plain object
    (push_ir(rows) and process(x) -> samples, position); the bookkeeping of steps 1 .. 3 is this class's own"""

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
