"""numpy model of the multi-block direct convolution's contract (clfa_dconv_process_blocks_dev, include/clfft_amd.h):
the static form, the time-varying form and the state a call leaves, for any write point wp0.  Plain restatements of
the three definitions in float64 — nothing of the kernels' tiling.  tests/test_dconv_blocks_cpu.py checks it against
oracle.Dconv driven block by block; tests/test_gpu_dconv_blocks.py takes the expected write point from it."""
import numpy as np


class DconvBlocksModel:
    def __init__(self, irsize, vsize, channels=1):
        self.irsize, self.vsize, self.channels = irsize, vsize, channels
        self.end = irsize + vsize
        self.delay = np.zeros((channels, self.end))
        self.coefs = np.zeros((channels, self.end))
        self.wp = 0

    def push_ir(self, ir):
        self.coefs[:, :self.irsize] = np.asarray(ir, np.float64).reshape(self.channels, -1)[:, :self.irsize]

    def _x(self, c, in1, tau):
        """x_c[tau], -irsize <= tau: the call's input, or the delay ring at (wp0 + tau) mod end"""
        return in1[c, tau] if tau >= 0 else self.delay[c, (self.wp + tau) % self.end]

    def _coef(self, c, in2, j, k):
        """coef_c^(j)[k] of the time-varying form"""
        last = (j + 1) * self.vsize - 1
        tp = last - ((last - (k - self.wp)) % self.end)
        return in2[c, tp] if tp >= 0 else self.coefs[c, k]

    def blocks(self, in1, in2=None):
        in1 = np.asarray(in1, np.float64).reshape(self.channels, -1)
        if in2 is not None:
            in2 = np.asarray(in2, np.float64).reshape(self.channels, -1)
        L = in1.shape[1]
        assert L % self.vsize == 0
        out = np.zeros((self.channels, L))
        for c in range(self.channels):
            for t in range(L):
                acc = 0.0
                for k in range(self.irsize):
                    h = self.coefs[c, k] if in2 is None else self._coef(c, in2, t // self.vsize, k)
                    acc += h * self._x(c, in1, t - 1 - k)
                out[c, t] = acc
        # state: the last `end` samples at (wp0 + tau) mod end; earlier content stays where fewer came
        for tau in range(max(0, L - self.end), L):
            self.delay[:, (self.wp + tau) % self.end] = in1[:, tau]
            if in2 is not None:
                self.coefs[:, (self.wp + tau) % self.end] = in2[:, tau]
        self.wp = (self.wp + L) % self.end
        return out
