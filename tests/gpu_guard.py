"""Guard bands for the device tests: an output (or an input) sits inside an int32 buffer of CANARY, so a store outside it
and an element that no store reached both show.  One class, two constructors: flat() puts one contiguous view of any
shape in the middle, rows() puts rows a stride apart, whose gaps are guard too.  tests/test_gpu_guard_cpu.py runs all of
it on CPU tensors: a stray word anywhere, and an unwritten one, must fail the checks."""
import numpy as np
import torch

DEV = "cuda:0"
CANARY = 0x7FC0BEEF     # a quiet NaN whose payload no kernel produces: as a float it is never a result, as bits it is exact


class Guarded:
    """buf: the whole int32 buffer; data: the float32 (or complex64) view a call may write, `misalign` floats past a
    16-byte boundary; the words before, after and (rows) between the rows are the guard"""

    def __init__(self, buf, lo, nrows, rowlen, stride, misalign):
        self.buf, self.lo, self.hi = buf, lo, lo + nrows * stride
        self.body = buf[lo:self.hi].view(nrows, stride)
        self.words = self.body[:, :rowlen]
        self.data = self.words.view(torch.float32)
        assert self.data.data_ptr() % 16 == 4 * misalign

    @property
    def mask(self):
        """the words of buf a call may write"""
        m = torch.zeros(self.buf.shape, dtype=torch.bool, device=self.buf.device)
        m[self.lo:self.hi].view(self.body.shape)[:, :self.words.shape[1]] = True
        return m

    def sides(self):
        """(nothing written before, nothing after, nothing between the rows)"""
        return tuple(bool((part == CANARY).all()) for part in
                     (self.buf[:self.lo], self.buf[self.hi:], self.body[:, self.words.shape[1]:]))

    def intact(self):
        return all(self.sides())

    def check_sides(self, what):
        before, after, between = self.sides()
        assert before, "wrote before " + what
        assert after, "wrote after " + what
        assert between, "wrote between the rows"

    def unwritten(self):
        """how many words a call may write still hold the canary"""
        return int((self.words == CANARY).sum())

    def untouched(self):
        """nothing written at all: what a refused call leaves"""
        return bool((self.buf == CANARY).all())

    def fill(self, host):
        """an input: the values go in, and unchanged() holds until something writes anywhere in the buffer"""
        self.data.copy_(torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)).to(self.buf.device).view(self.data.shape))
        self.kept = self.buf.clone()
        return self

    def unchanged(self):
        return bool(torch.equal(self.buf, self.kept))

    def host(self):
        return self.data.contiguous().cpu().numpy()


def flat(shape, dtype=torch.float32, misalign=2, before=1024, after=1024 + 4, device=DEV):
    """a view of `shape` and dtype (float32 or complex64) behind `before` + misalign canaries and before `after` more;
    `before` is a multiple of 4, so the view starts misalign floats (of 4 bytes) past a 16-byte boundary"""
    n = int(np.prod(shape)) * (2 if dtype == torch.complex64 else 1)
    lo = before + misalign
    g = Guarded(torch.full((lo + n + after,), CANARY, dtype=torch.int32, device=device), lo, 1, n, n, misalign)
    g.data = g.data[0].view(dtype).view(*shape)
    return g


def rows(nrows, rowlen, stride, misalign=0, before=1024, after=1024, device=DEV):
    """nrows rows of rowlen floats, `stride` floats apart: data is the (nrows, rowlen) view; the stride - rowlen words
    behind every row, the last one included, are guard"""
    assert stride >= rowlen
    lo = before + misalign
    return Guarded(torch.full((lo + nrows * stride + after,), CANARY, dtype=torch.int32, device=device), lo, nrows, rowlen,
                   stride, misalign)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(a, device=DEV):
    return torch.from_numpy(np.array(a, order="C")).to(device)      # a copy: the cached inputs are read-only


def same(got, want, what):
    """bit-equal where the model is a number, a NaN where it is a NaN"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what + ": where the NaNs are"
    assert np.array_equal(bits(got)[~nan], bits(want)[~nan]), what


def run(call, shape, device=DEV):
    """one device call into a guarded output: the result as numpy, the guard bands checked, every element written"""
    g = flat(shape, device=device)
    assert call(g.data) == 0
    if g.buf.is_cuda:
        torch.cuda.synchronize()
    assert g.intact(), "wrote outside the output"
    assert not g.unwritten(), "an output element was not written"
    return g.data.cpu().numpy()
