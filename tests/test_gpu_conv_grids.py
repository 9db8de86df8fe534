"""The capped grid-stride launches of the convolution family, each taken round its loop a second time where a real shape
that does so is cheap.  grid_clamp(groups, cap) (pconv_device.hpp) sizes 16 launches; every call site has a row here (and
in DESIGN.md, "The capped launches of the convolution family"), derived from the launcher's own arithmetic: what one
workgroup covers, the cap, the smallest object and call that exceed it, the largest single device buffer that takes, and
the test that wraps it or the size that puts it out of reach.  "Cheap" is at most 64 MiB in any one buffer.  The
sub-batch workspaces of Clpconv, PconvMatrix and Cldconv are sized by the object's sub-batch cap whatever the call, about
128 MiB each at these channel counts, so the tests lower the cap with the objects' own switches (CLFA_PCONV_BLOCKS_MAX,
CLFA_PCONV_MATRIX_BLOCKS_MAX), which changes no bit (tests/test_gpu_pconv_blocks.py test_sub_batches_bit_exact).

 # launch (file)                      one workgroup      cap   wraps when                      smallest object and call                                largest buffer  covered by
 1 k_pconvb_fwd (pconv_blocks)        256 lanes x 16     8192  channels * K * pts > 2^25       the sub-batch cap (3 workspaces in 384 MiB) keeps       256 MiB (X)     out of reach: 8192 groups
                                      points of spectra                                        channels * K * pts <= 2^24 for Clpconv and the                          are 256 MiB of spectra
                                                                                               Nupconv head; PconvMatrix: inputs * K * pts > 2^25                       whatever the size
 2 k_pconvb_inv (pconv_blocks)        the same, per run  8192  channels * runs * pts > 2^25    as row 1 (a run is one block or more)                  256 MiB (Y)     out of reach, as row 1
 3 k_pconvb_commit (pconv_blocks)     256 floats (y=1:   4096  channels * pts > 2^20           Clpconv(pts 4096, 1 partition, 257 channels), a call   16.1 MiB (X, Y) test_pconvb_commit_tail
                                      commit_tail), 256                                        of 2 blocks at CLFA_PCONV_BLOCKS_MAX=2; y=0/2
                                      items (y=0, 2:                                           (commit_spectra) loops whenever more than two spectra
                                      commit_spectra)                                          are committed, which the existing tests do
 4 k_pconvm_reduce (pconv_matrix)     256 items of 2     8192  outputs * K * pts / 2 > 2^21,   PconvMatrix(2 -> 16, pts 4096, 94 partitions), 97      88.5 MiB (Y)    test_gpu_pconv_matrix.py
                                      bins                     segments > 1                    blocks: 4 segments from 65 CUs on, cap 177, n = 3.2e6                  test_equals_the_composition
                                                                                                                                                                      [2-16-4096-94], second call
 5 k_pconvm_commit (pconv_matrix)     as row 3           4096  max(inputs, outputs) * pts      PconvMatrix(1 -> 257, pts 4096, 1 partition), 2 blocks 16.2 MiB (Y)    test_pconvm_commit_tails
                                                               > 2^20 (y=1: outputs * pts)     at CLFA_PCONV_MATRIX_BLOCKS_MAX=2                                      [plain]
 6 k_pconvm_mix (pconv_matrix)        256 samples        8192  outputs * K * pts > 2^21        PconvMatrix(1 -> 4, pts 4096), a fade call of 129      16.1 MiB (Y)    test_pconvm_mix
                                                                                               blocks at CLFA_PCONV_MATRIX_BLOCKS_MAX=129
 7 k_pconvm_commit_tail (pconv_matrix) 256 floats        4096  outputs * pts > 2^20            as row 5, 2 blocks of a fade                           16.2 MiB (Y)    test_pconvm_commit_tails
                                                                                                                                                                      [fade]
 8 k_nupc_stage (pconv_nup)           256 units of V     4096  channels * n / V > 2^20,        Nupconv(2048, 4096), 257 channels, a two-block call    48.3 MiB at     test_nupc_stage_and_mix
                                      floats                   n <= pts1 the call's samples    that starts on a tail period, rows 4 bytes off a       515 channels    [plain]; single blocks:
                                                               inside one tail period; V = 1   16-byte boundary (V = 4: four times the channels)      (tail ring)     test_nupc_fade_mix
                                                               for misaligned rows, else 4
 9 k_nupc_stage2 (pconv_nup)          as row 8, y = 0, 1 4096  as row 8                        as row 8, process_tv_device                            as row 8        test_nupc_stage_and_mix[tv]
10 k_nupc_fwd (pconv_nup)             FPW = 4096 / pts   8192  channels > 8192 * FPW           Nupconv(pts0, 4096) tail level: 8193 channels          768 MiB         out of reach (tail ring
                                      rows                                                                                                            (tail ring)     of 3 frames x 8193 x 32 KiB)
11 k_nupc_mix (pconv_nup)             as row 8           4096  as row 8 (V by the output rows) as row 8                                               as row 8        test_nupc_stage_and_mix
12 k_nupc_fade_mix (pconv_nup)        as row 8           4096  channels * pts0 / V > 2^20      Nupconv(2048, 4096), 513 channels, one block of a fade 48.3 MiB at     test_nupc_fade_mix
                                                               (a fade runs block by block)                                                           515 channels
13 k_pconv_fwd (pconv_chain)          FPW = min(256,     4096  channels > 4096 * FPW           in bytes the smallest is the chain at pts 2 (FPW 256): 32 MiB (a ring  test_pconv_chain_forward_
                                      max(1, 4096 / pts))                                      Clpconv(pts 2, 2 partitions, 2^20 + 1 channels), a     of 2 frames)    and_inverse; at pts 8192
                                      rows                                                     push and single-block calls; at the chain's large                      (FPW 1) 4097 channels are a
                                                                                               sizes, pts 8192: 4097 channels                                         ring of 256 MiB a partition
14 k_pconv_inv (pconv_chain)          as row 13          4096  as row 13                       as row 13                                              as row 13       as row 13
15 k_dconvb_reduce (dconv_blocks)     256 samples of one 4096  L > 2^20 samples in a sub-batch Cldconv(irsize 4097, vsize 2048), 513 blocks           8.0 MiB a       test_dconvb_reduce
                                      channel (y)              and irsize > 4096 (2 segments)                                                         channel         (3 channels)
                                                                                                                                                      (partials)
16 k_dconvb_commit (dconv_blocks)     256 samples of one 4096  min(L, irsize + vsize) > 2^20   irsize > 2^20 - vsize: 64 segments whose partials of   256 MiB         out of reach
                                      channel (y)                                              a sub-batch with L > 2^20 are 64 * L floats            (partials)
(Row 3's launch is one call site for its three jobs, blockIdx.y = 0, 1, 2.  The chain's k_pconv_mac, k_pconv_reduce, k_pconv_pad
and k_pconv_olap cap their grids in words of their own, not through grid_clamp: they are not rows of this table.)

Every test here: guarded rows (tests/gpu_guard.py: bands intact, every output element written, inputs unchanged);
channels (the matrix's outputs) picked from the first pass of the loop, from the second — by row arithmetic it starts at
element cap * 256 of the launch — and the very last one; for each picked channel parity with the float64 definition at
util.TOL, bit equality with a small object fed the picked rows (it does not wrap), and one more block after the call that
must again be the small object's, bit for bit: a commit that missed its second pass shows only there."""
import numpy as np
import pytest
import torch

import opencl_fft_amd as fa
from tests import conv_exact as cx
from tests import gpu_guard as gg
from tests import util
from tests.nupconv_definitions import definition, mixed
from tests.nupconv_model import NupFadeModel, NupTvModel

pytestmark = pytest.mark.gpu

WG = 256   # units per workgroup of every launch tested here


def _noise(seed, *shape):
    return np.random.default_rng(seed).random(shape, dtype=np.float32) - np.float32(0.5)


def _picks(n, per_row, cap):
    """rows 0 and the last of the first pass, the first of every later pass, the very last: row r of a launch over n rows of
    per_row units starts at unit r * per_row, and pass q starts at unit q * cap * 256"""
    total, step = n * per_row, cap * WG
    assert total > step, "the launch does not wrap: %d units, %d per pass" % (total, step)
    firsts = [-(-q * step // per_row) for q in range(1, -(-total // step))]   # the first row that lies wholly in pass q
    picks = sorted({0, firsts[0] - 1, n - 1} | {r for r in firsts if r < n})
    assert picks[0] == 0 and picks[-1] == n - 1 and picks[-1] * per_row >= step
    return picks


def _stream(call, pts, steps, inputs, nrows_out):
    """`steps`: block counts, each one call over the next blocks of the guarded rows, and callables run between calls (a
    push).  Every row set at its own stride and 4, 8 bytes past a 16-byte boundary; out 4 bytes past one.  Returns the output
    after the checks of the bands, of every output element and of the inputs."""
    L = inputs[0].shape[1]
    ins = [gg.rows(a.shape[0], L, L + 5 + 2 * i, misalign=1 + i).fill(np.array(a)) for i, a in enumerate(inputs)]
    out = gg.rows(nrows_out, L, L + 9, misalign=1)
    j = 0
    for n in steps:
        if callable(n):
            torch.cuda.synchronize()
            assert n() == 0
            continue
        a, b = j * pts, (j + n) * pts
        assert call(out.data[:, a:b], *[g.data[:, a:b] for g in ins]) == 0
        j += n
    torch.cuda.synchronize()
    assert j * pts == L
    out.check_sides("the output rows")
    assert not out.unwritten(), "an output element was not written"
    assert all(g.unchanged() for g in ins), "an input changed"
    return out.host()


def _same_and_parity(got, small, want, picks, last, what):
    """got: the large object's output; small, want: the small object's and the float64 definition's for the picked rows;
    `last`: samples of the one block after the call"""
    for k, c in enumerate(picks):
        l2, mx = util.rel_err(got[c], want[k])
        print("%s, row %d: relL2 %.3g max/max %.3g" % (what, c, l2, mx))
        util.assert_parity(got[c], want[k], what="%s, row %d" % (what, c))
        gg.same(got[c, :-last], small[k, :-last], "%s, row %d: the call" % (what, c))
        gg.same(got[c, -last:], small[k, -last:], "%s, row %d: the block after the call" % (what, c))


# ---- row 3: k_pconvb_commit, the tails ----------------------------------------------------------------------------------------------

def test_pconvb_commit_tail(monkeypatch):
    pts, channels, cap = 4096, 259, 4096
    picks = _picks(channels, pts, cap)
    assert picks == [0, 255, 256, 258]
    monkeypatch.setenv("CLFA_PCONV_BLOCKS_MAX", "2")   # workspaces of 2 blocks, not 15
    h, x = _noise(31, channels, pts), _noise(32, channels, 3 * pts)
    outs = []
    for rows in (slice(None), picks):
        p = fa.Clpconv(0, pts, pts, channels=len(h[rows]))
        assert p.get_cl_err() == 0 and p.nparts == 1 and p.blocks_kernel_name() == "k_pconvb_mac"
        assert p.push_ir(h[rows]) == 0
        outs.append(_stream(p.process_blocks_device, pts, [2, 1], [x[rows]], p.channels))
        assert p.wp == 0
    want = [util.pconv_f64(h[c].astype(np.float64), x[c].astype(np.float64), pts) for c in picks]
    _same_and_parity(outs[0], outs[1], want, picks, pts, "Clpconv 4096 x 1 x 259")


# ---- rows 13 and 14: k_pconv_fwd and k_pconv_inv, the launch chain of the single-block call ----------------------------------------

def test_pconv_chain_forward_and_inverse():
    """partitions of 2 samples: one lane per transform, 256 transforms per workgroup, so 4096 workgroups take 2^20 channels
    and channels 2^20 .. 2^20 + 2 are the second pass of the forward launch (the push's too) and of the inverse launch.
    Two partitions: a block's output needs the ring frame the block before it filed, and the tail it left"""
    pts, nparts, cap, fpw, nblocks = 2, 2, 4096, 256, 4
    channels = cap * fpw + 3
    picks = _picks(channels, 1, cap)
    assert picks == [0, cap * fpw - 1, cap * fpw, channels - 1]
    h, x = _noise(131, channels, nparts * pts), _noise(132, channels, nblocks * pts)
    outs = []
    for rows in (slice(None), picks):
        p = fa.Clpconv(0, nparts * pts, pts, channels=len(h[rows]))
        assert p.get_cl_err() == 0 and p.nparts == nparts and p.kernel_name() == "chain"
        assert p.push_ir(h[rows]) == 0
        blocks = []
        for j in range(nblocks):
            xin = gg.flat((p.channels, pts)).fill(x[rows][:, j * pts:(j + 1) * pts])
            blocks.append(gg.run(lambda o: p.process_device(o, xin.data), (p.channels, pts)))
            assert xin.unchanged(), "the input changed"
        outs.append(np.concatenate(blocks, axis=1))
        assert p.wp == nblocks % nparts
    want = [util.pconv_f64(h[c].astype(np.float64), x[c].astype(np.float64), pts) for c in picks]
    _same_and_parity(outs[0], outs[1], want, picks, pts, "Clpconv 2 x 2 x (2^20 + 3), the launch chain")


# ---- rows 5 and 7: k_pconvm_commit and k_pconvm_commit_tail -------------------------------------------------------------------------

def _matrix(pts, inputs, h):
    m = fa.PconvMatrix(0, pts, pts, inputs, h.shape[0])
    assert m.get_error() == 0, m.get_log()
    assert m.nparts == 1 and m.kernel_name() == "k_pconvm_mac"
    assert m.push_ir(h) == 0
    return m


def _matrix_f64(hA, hB, x, pts, c, fade):
    """one input: every output's pconv_f64 under hA, and where there is a fade mixed with that under hB"""
    x64 = x[0].astype(np.float64)
    ya = np.stack([util.pconv_f64(h[0].astype(np.float64), x64, pts) for h in hA])
    if not fade:
        return ya
    yb = np.stack([util.pconv_f64(h[0].astype(np.float64), x64, pts) for h in hB])
    return mixed(ya, yb, c, fade, pts)


@pytest.mark.parametrize("fade", [0, 2], ids=["plain", "fade"])
def test_pconvm_commit_tails(monkeypatch, fade):
    """plain: the call of 2 blocks commits 259 tails (k_pconvm_commit, y = 1).  fade: 2 blocks, then a fade of 2 blocks in one
    call, which commits the second path's 259 tails as well (k_pconvm_commit_tail): they are the tails after the fade"""
    pts, outputs, cap = 4096, 259, 4096
    picks = _picks(outputs, pts, cap)
    monkeypatch.setenv("CLFA_PCONV_MATRIX_BLOCKS_MAX", "2")
    hA, hB = _noise(51, outputs, 1, pts), _noise(52, outputs, 1, pts)
    nblocks = 3 + fade
    x = _noise(53, 1, nblocks * pts)
    outs = []
    for rows in (slice(None), picks):
        m = _matrix(pts, 1, hA[rows])
        steps = [2, 1] if not fade else [2, lambda: m.push_ir_fade(hB[rows], fade), fade, 1]
        outs.append(_stream(m.process_device, pts, steps, [x], m.outputs))
        assert m.fade_remaining() == 0
    want = _matrix_f64(hA[picks], hB[picks], x, pts, 2, fade)
    _same_and_parity(outs[0], outs[1], want, picks, pts, "PconvMatrix 1 -> 259 at 4096, %s" % ("fade" if fade else "plain"))


# ---- row 6: k_pconvm_mix ------------------------------------------------------------------------------------------------------------

def test_pconvm_mix(monkeypatch):
    """a fade of 129 blocks in one call and one sub-batch: 4 x 129 x 4096 samples are mixed, 16384 more than 8192 workgroups
    cover, so the second pass is the end of output 3.  The small object runs the same fade in sub-batches of 16 blocks"""
    pts, outputs, fade, cap = 4096, 4, 129, 8192
    assert outputs * fade * pts > cap * WG and (outputs - 1) * fade * pts < cap * WG
    picks = [0, 3]
    hA, hB = _noise(61, outputs, 1, pts), _noise(62, outputs, 1, pts)
    x = _noise(63, 1, (2 + fade + 1) * pts)
    outs = []
    for rows, blocks_max in ((slice(None), fade), (picks, 16)):
        monkeypatch.setenv("CLFA_PCONV_MATRIX_BLOCKS_MAX", str(blocks_max))
        m = _matrix(pts, 1, hA[rows])
        outs.append(_stream(m.process_device, pts, [2, lambda: m.push_ir_fade(hB[rows], fade), fade, 1], [x], m.outputs))
        assert m.fade_remaining() == 0
    want = _matrix_f64(hA[picks], hB[picks], x, pts, 2, fade)
    _same_and_parity(outs[0], outs[1], want, picks, pts, "PconvMatrix 1 -> 4 at 4096, a fade of 129 blocks")


# ---- rows 8, 9, 11, 12: the stage and mix kernels of Nupconv ----------------------------------------------------------------------------

PTS0, PTS1, N1, NUP_CHANNELS = 2048, 4096, 1, 515
NUP_CVS = 2 * PTS1 + N1 * PTS1 + 5


def _nupconv(h):
    p = fa.Nupconv(0, NUP_CVS, PTS0, PTS1, channels=h.shape[0])
    assert p.get_error() == 0, p.get_log()
    assert p.nparts(0) == 4 and p.nparts(1) == N1 and p.kernel_name() == "k_nupc_mac"
    assert p.push_ir(h) == 0
    return p


@pytest.mark.parametrize("tv", [False, True], ids=["plain", "tv"])
def test_nupc_stage_and_mix(tv):
    """calls of two blocks, each a whole tail period: the stage launch (k_nupc_stage; tv: k_nupc_stage2, both inputs) and
    k_nupc_mix move 515 x 4096 floats one by one (rows 4 and 8 bytes off a 16-byte boundary), two passes and a bit.  Five
    periods and one block: what the second pass staged in periods 0 .. 2 is heard in periods 2 .. 4 (tv: the second input
    staged in period 2 is the tail's response from period 3 on, heard in period 4)"""
    picks = _picks(NUP_CHANNELS, PTS1, 4096)
    assert picks == [0, 255, 256, 512, 514]
    steps = [2] * 5 + [1]
    L = sum(steps) * PTS0
    h, x = _noise(81, NUP_CHANNELS, NUP_CVS), _noise(82, NUP_CHANNELS, L)
    inputs = [x, _noise(83, NUP_CHANNELS, L)] if tv else [x]
    outs = []
    for rows in (slice(None), picks):
        p = _nupconv(h[rows])
        outs.append(_stream(p.process_tv_device if tv else p.process_device, PTS0, steps, [a[rows] for a in inputs], p.channels))
        assert p.position == sum(steps)
    if tv:
        model = NupTvModel(NUP_CVS, PTS0, PTS1, len(picks))
        model.push_ir(h[picks])
        want = model.process(x[picks], inputs[1][picks])
    else:
        want = [definition(h[c], x[c], NUP_CVS, PTS0, PTS1) for c in picks]
    _same_and_parity(outs[0], outs[1], want, picks, PTS0, "Nupconv(2048, 4096) x 515, %s" % ("tv" if tv else "plain"))


def test_nupc_fade_mix():
    """a fade runs block by block: k_nupc_fade_mix (and the single-block stage launch) over 515 x 2048 floats, 6144 more than
    4096 workgroups cover.  The push comes in period 2, when both paths' pending rows are heard"""
    picks = _picks(NUP_CHANNELS, PTS0, 4096)
    assert picks == [0, 511, 512, 514]
    c, fade = 5, 3
    hA, hB = _noise(121, NUP_CHANNELS, NUP_CVS), _noise(122, NUP_CHANNELS, NUP_CVS)
    x = _noise(123, NUP_CHANNELS, (c + fade + 2 + 1) * PTS0)
    outs = []
    for rows in (slice(None), picks):
        p = _nupconv(hA[rows])
        steps = [c, lambda: p.push_ir_fade(hB[rows], fade)] + [1] * fade + [2, 1]
        outs.append(_stream(p.process_device, PTS0, steps, [x[rows]], p.channels))
        assert p.fade_remaining() == 0
    model = NupFadeModel(NUP_CVS, PTS0, PTS1, len(picks))
    model.push_ir(hA[picks])
    want = [model.process(x[picks, :c * PTS0])]
    model.push_ir_fade(hB[picks], fade)
    want.append(model.process(x[picks, c * PTS0:]))
    _same_and_parity(outs[0], outs[1], np.concatenate(want, axis=1), picks, PTS0, "Nupconv(2048, 4096) x 515, a fade of 3 blocks")


# ---- row 15: k_dconvb_reduce --------------------------------------------------------------------------------------------------------

def test_dconvb_reduce():
    """513 blocks of 2048 samples in one sub-batch, two tap segments: the reduce walks 2^20 + 2048 samples per channel, the
    last block in its second pass.  Unit taps at 0, 4095 (the first segment's last) and 4096 (the second's first) make the
    float64 definition an exact delay (tests/conv_exact.py): parity is equality.  The small object: calls of 128 blocks"""
    irsize, vsize, nblocks, taps = 4097, 2048, 513, (0, 4095, 4096)
    L = nblocks * vsize
    assert L > 4096 * WG and L - vsize <= 4096 * WG
    ir = np.stack([cx.unit_tap(irsize, k) for k in taps])
    x = cx.nonzero_noise(151, (len(taps), L + vsize))
    outs = []
    for steps in ([nblocks, 1], [128] * 4 + [1, 1]):
        d = fa.Cldconv(0, irsize, vsize, channels=len(taps))
        assert d.get_cl_err() == 0 and d.push_ir(ir) == 0
        outs.append(_stream(lambda o, a: d.process_blocks_device(o, a, None), vsize, steps, [x], len(taps)))
        assert d.wp == (L + vsize) % (irsize + vsize)
    want = np.stack([cx.dconv_delayed(x[c], k) for c, k in enumerate(taps)])
    for c, k in enumerate(taps):
        assert np.array_equal(outs[0][c], want[c]), "tap %d: not the input delayed by %d samples" % (k, k + 1)
    _same_and_parity(outs[0], outs[1], want.astype(np.float64), range(len(taps)), vsize, "Cldconv 4097 x 2048, 513 blocks")
