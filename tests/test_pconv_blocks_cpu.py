"""Multi-block partitioned convolution without a GPU: the new ABI symbols, the Python surface's answers without a device,
and a float64 model of the frame / version algebra of pconv_blocks.hip checked against the oracle driven block by
block."""
import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd._lib import lib
from oracle import oracle

CL_DEVICE_NOT_FOUND = -1
NAMES = ["clfa_pconv_process_blocks_dev", "clfa_pconv_convolution_blocks", "clfa_pconv_blocks_workspace_bytes",
         "clfa_pconv_blocks_kernel_name"]


@pytest.mark.parametrize("name", NAMES)
def test_symbol_exported(name):
    assert hasattr(lib(), name)


def test_methods_without_a_device():
    if fa.device_count() > 0:
        pytest.skip("a device is present (tests/test_gpu_pconv_blocks.py)")
    p = fa.Clpconv(0, 4 * 64, 64, channels=2)
    assert p.get_cl_err() == CL_DEVICE_NOT_FOUND
    x = np.zeros((2, 3 * 64), np.float32)
    assert p.convolution_blocks(np.zeros_like(x), x) == CL_DEVICE_NOT_FOUND
    assert p.convolution_blocks(np.zeros_like(x), x, x.copy()) == CL_DEVICE_NOT_FOUND
    assert p.blocks_kernel_name() == ""
    assert p.blocks_workspace_bytes() == 0
    import torch
    t = torch.zeros((2, 3 * 64))
    assert p.process_blocks_device(torch.zeros_like(t), t, stream=0) == CL_DEVICE_NOT_FOUND


class BlocksModel:
    """float64 restatement of one object under multi-block calls, sub-batch by sub-batch, with the index algebra of
    pconv_blocks.hip: input of partition p for output j is m = j - (nparts - 1) + p (this sub-batch's X[m] for m >= 0,
    ring A frame (w + m) mod nparts before it); the time-varying response of partition p is the sub-batch's XB[k_p],
    k_p = (w2 - p) mod nparts, once k_p <= j, else ring B frame p.  The rings change only after the whole sub-batch."""

    def __init__(self, nparts, pts, cap):
        self.nparts, self.pts, self.cap = nparts, pts, cap
        self.A = np.zeros((nparts, pts + 1), np.complex128)
        self.B = np.zeros((nparts, pts + 1), np.complex128)
        self.tail = np.zeros(pts)
        self.wp, self.wp2 = 0, nparts - 1

    def spectra(self, x):
        z = np.zeros((x.size // self.pts, 2 * self.pts))
        z[:, :self.pts] = x.reshape(-1, self.pts)
        return np.fft.rfft(z, axis=1)

    def push_ir(self, ir):
        H = self.spectra(np.asarray(ir[:self.nparts * self.pts], np.float64))
        for i in range(self.nparts):
            self.B[self.wp2] = H[i]
            self.wp2 = self.wp2 - 1 if self.wp2 else self.nparts - 1

    def blocks(self, x1, x2=None):
        n, pts, P = x1.size // self.pts, self.pts, self.nparts
        kmax = min(self.cap, P) if x2 is not None else self.cap
        out = []
        for j0 in range(0, n, kmax):
            K = min(kmax, n - j0)
            X = self.spectra(np.asarray(x1[j0 * pts:(j0 + K) * pts], np.float64))
            XB = self.spectra(np.asarray(x2[j0 * pts:(j0 + K) * pts], np.float64)) if x2 is not None else None
            w, w2 = self.wp, self.wp2
            for j in range(K):
                Y = np.zeros(pts + 1, np.complex128)
                for p in range(P):
                    m = j - (P - 1) + p
                    F = X[m] if m >= 0 else self.A[(w + m) % P]
                    k = (w2 - p) % P
                    H = XB[k] if (XB is not None and k < K and k <= j) else self.B[p]
                    Y += F * H
                Y[0] *= 0.5   # the packed DC / Nyquist products' gain (tests/util.py, _olap64)
                Y[pts] *= 0.5
                y = np.fft.irfft(Y, n=2 * pts)
                out.append(y[:pts] + self.tail)
                self.tail = y[pts:].copy()
            for m in range(max(0, K - P), K):
                self.A[(w + m) % P] = X[m]
            if XB is not None:
                for k in range(K):
                    self.B[(w2 - k) % P] = XB[k]
                self.wp2 = (w2 - K) % P
            self.wp = (w + K) % P
        return np.concatenate(out) if out else np.zeros(0)


@pytest.mark.parametrize("tv", [False, True], ids=["static", "tv"])
@pytest.mark.parametrize("nparts,cap", [(1, 1), (3, 1), (3, 2), (4, 5), (5, 3), (7, 100)])
def test_index_algebra_matches_the_oracle_loop(nparts, cap, tv):
    pts = 16
    rng = np.random.default_rng(nparts * 10 + cap + tv)
    m, o = BlocksModel(nparts, pts, cap), oracle.Pconv(nparts * pts, pts)
    for call, nb in enumerate([1, nparts + 2, 2 * nparts + 3, nparts, 4]):
        if call == 2:   # push_ir between multi-block calls
            ir = rng.random(nparts * pts, dtype=np.float32) - 0.5
            m.push_ir(ir)
            o.push_ir(ir)
        elif call == 0:
            ir = rng.random(nparts * pts, dtype=np.float32) - 0.5
            m.push_ir(ir)
            o.push_ir(ir)
        x1 = rng.random(nb * pts, dtype=np.float32) - 0.5
        x2 = rng.random(nb * pts, dtype=np.float32) - 0.5 if tv else None
        got = m.blocks(x1, x2)
        want = np.concatenate([o.convolution(x1[j * pts:(j + 1) * pts], None if x2 is None else x2[j * pts:(j + 1) * pts])
                               for j in range(nb)])
        err = np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-30)
        assert err < 1e-5, (call, nb, err)
        assert (m.wp, m.wp2) == (o.wp, o.wp2)
