"""CPU tests of tests/conv_exact.py: the oracle (the reference's arithmetic in float32) stays within the per-bin bar on
every family tests/test_gpu_conv_impulses.py uses — which is what entitles that file to hold the HIP routes to TOL per bin —
is exactly zero outside the block pairs, and delays by exactly k + 1; the comb isolates partitions in the float64 models,
where every pair equals conv_exact.pair_truth.  Each oracle case prints `CONV-IMPULSE oracle ...`; the lines are the oracle
half of profiles/conv_impulses.txt."""
import numpy as np
import pytest

from oracle import oracle
from tests import conv_exact as cx
from tests.pconv_matrix_model import MatrixModel
from tests.util import TOL

# The oracle's arithmetic for one partition's pair does not depend on how many empty partitions there are beside it (they
# add exact zeros), so the long filters of the GPU table run here with at most 94 partitions (config 4's count, in full).
ORACLE_MAX_PARTS = 94
ORACLE_GEOMS = sorted({(pts, min(nparts, ORACLE_MAX_PARTS), min(ch, 32), min(b0, min(nparts, ORACLE_MAX_PARTS) + 1))
                       for _, _, pts, nparts, ch, b0 in cx.PCONV_ROUTES}
                      | {(pts, nparts, ch, b0) for _, pts, nparts, ch, b0 in cx.PCONV_BLOCK_ROUTES}
                      | {(pts, nparts, 1, 1) for _, _, pts, nparts in cx.MATRIX_GEOMS})


def _oracle_run(pts, nparts, ir, x1, x2=None):
    o = oracle.Pconv(pts * nparts, pts)
    if ir is not None:
        o.push_ir(ir)
    return np.concatenate([o.convolution(x1[j * pts:(j + 1) * pts], None if x2 is None else x2[j * pts:(j + 1) * pts])
                           for j in range(x1.size // pts)])


@pytest.mark.parametrize("tv", [False, True], ids=["static", "tv"])
@pytest.mark.parametrize("pts,nparts,channels,b0", ORACLE_GEOMS)
def test_oracle_within_the_bar_and_exactly_zero_elsewhere(pts, nparts, channels, b0, tv):
    nblocks = cx.nblocks_for(nparts, b0)
    wb = ws = 0.0
    for parity, k, s in cx.slots(pts, channels):
        x1 = cx.block_impulse(pts, nblocks, b0, s)
        if tv:
            out = _oracle_run(pts, nparts, None, x1, cx.tv_comb_input(pts, nparts, nblocks, parity, k))
        else:
            out = _oracle_run(pts, nparts, cx.comb_response(pts, nparts, parity, k), x1)
        b, t, stray, at = cx.check_channel(out, pts, b0, cx.comb(nparts, parity), k, s)
        assert stray == 0, "oracle: %d non-zero samples outside the pairs (parity %d k %d s %d)" % (stray, parity, k, s)
        assert b <= TOL and t <= TOL, "oracle: worst bin %.3g (partition, bin) %s, worst sample %.3g (k %d s %d)" % (b, at, t, k, s)
        wb, ws = max(wb, b), max(ws, t)
    print("CONV-IMPULSE oracle %dx%d %s b0=%d worst-bin %.3g worst-sample %.3g" % (pts, nparts, "tv" if tv else "static", b0, wb, ws))


def test_the_multi_block_table_holds_every_transform_size_of_the_route():
    """k_pconvb_mac's forward and inverse kernels are one instantiation per size, 32 .. 4096: each has a row, the new ones
    with 3 or 5 partitions, and the impulse does not always come in block 1"""
    rows = [r for r in cx.PCONV_BLOCK_ROUTES if r[0] == "k_pconvb_mac"]
    assert sorted(r[1] for r in rows) == [32, 64, 128, 256, 512, 1024, 2048, 4096]
    assert ("k_pconvb_mac", 64, 3, 3, 4) in rows and ("k_pconvb_mac", 1024, 94, 3, 1) in rows
    new = [r for r in rows if r[1] not in (64, 1024)]
    assert all(r[2] in (3, 5) and r[3] in (1, 3) for r in new) and sum(r[3] == 1 for r in new) == 1
    assert sum(r[4] != 1 for r in new) >= 2
    assert {g[2] for g in cx.MATRIX_GEOMS} >= {128, 2048}
    # every row is one of the oracle's cases below, as it stands
    assert {r[1:] for r in cx.PCONV_BLOCK_ROUTES} <= set(ORACLE_GEOMS)


BLOCK_ROUTE_COMBS = sorted({(pts, nparts, b0) for _, pts, nparts, _, b0 in cx.PCONV_BLOCK_ROUTES if nparts <= 5})


@pytest.mark.parametrize("pts,nparts,b0", [(8, 4, 1), (8, 4, 5), (64, 3, 4), (2, 1, 2), (256, 5, 2), (32, 5, 6)]
                         + [g for g in BLOCK_ROUTE_COMBS if g not in ((64, 3, 4), (32, 5, 6))])
def test_comb_isolates_partitions_in_the_models(pts, nparts, b0):
    """float64 models, static and time-varying: the pair of partition p in a comb run is the pair of a run with partition p
    alone and is pair_truth (any b0, any p), and everything outside the pairs is exactly zero"""
    nblocks = cx.nblocks_for(nparts, b0)
    for parity, k, s in cx.slots(pts, 1):
        x1 = cx.block_impulse(pts, nblocks, b0, s)
        parts = cx.comb(nparts, parity)
        y = cx.pconv_truth(cx.comb_response(pts, nparts, parity, k), x1, pts)
        ytv = cx.pconv_tv_truth(x1, cx.tv_comb_input(pts, nparts, nblocks, parity, k), pts, nparts)
        for name, got in (("static", y), ("tv", ytv)):
            assert not got.reshape(-1, pts)[cx.outside_pairs(nblocks, b0, parts)].any(), name
        for p in parts:
            alone = cx.pconv_truth(cx.single_tap_response(pts, nparts, p, k), x1, pts)
            assert np.array_equal(cx.readback(y, pts, b0 + p), cx.readback(alone, pts, b0 + p))
            assert not alone.reshape(-1, pts)[cx.outside_pairs(nblocks, b0, [p])].any()
            for got in (y, ytv):
                assert np.array_equal(got[(b0 + p) * pts:(b0 + p + 2) * pts], cx.pair_truth(pts, k, s)), (p, k, s)


def test_time_varying_impulses_land_where_the_formula_says():
    """256 x 5: an impulse in block 2 of the first input and in block 3 of the second: blocks 5 and 6 only, model and oracle"""
    pts, nparts, nblocks = 256, 5, 9
    x1, x2 = cx.block_impulse(pts, nblocks, 2, 7), cx.block_impulse(pts, nblocks, 3, 100)
    y = cx.pconv_tv_truth(x1, x2, pts, nparts).reshape(nblocks, pts)
    o = _oracle_run(pts, nparts, None, x1, x2).reshape(nblocks, pts)
    for got in (y, o):
        assert [j for j in range(nblocks) if got[j].any()] == [5, 6]
    assert np.array_equal(y[5:7].reshape(-1), cx.pair_truth(pts, 100, 7))
    assert cx.worst_bin(cx.readback(o.reshape(-1), pts, 5), np.fft.rfft(cx.pair_truth(pts, 100, 7))) <= TOL


def test_pair_truth_bins_have_unit_magnitude():
    for pts, k, s in ((8, 1, 5), (512, 256, 511), (1024, 1023, 0)):
        mag = np.abs(np.fft.rfft(cx.pair_truth(pts, k, s)))
        assert np.allclose(mag[1:pts], 1.0, rtol=0, atol=1e-12) and np.allclose(mag[[0, pts]], 0.5, rtol=0, atol=1e-12)


@pytest.mark.parametrize("inputs,outputs,pts,nparts", cx.MATRIX_GEOMS)
def test_matrix_entry_in_the_model(inputs, outputs, pts, nparts):
    """one (input, output) pair with a comb response: output o holds pair_truth at every pair, every other output and a
    run with the impulse on another input are exactly zero (tests/pconv_matrix_model.py)"""
    i0, o0, b0 = 1, outputs - 2, nparts + 1
    nblocks = cx.nblocks_for(nparts, b0)
    for parity, k, s in cx.slots(pts, 1)[:4]:
        parts = cx.comb(nparts, parity)
        m = MatrixModel(nparts, pts, inputs, outputs, cap=nblocks)
        m.push_ir(cx.matrix_entry(inputs, outputs, pts, nparts, i0, o0, parts, k))
        x = np.zeros((inputs, nblocks * pts))
        x[i0] = cx.block_impulse(pts, nblocks, b0, s)
        y = m.process(x)
        assert not np.delete(y, o0, axis=0).any()
        b, t, stray, _ = cx.check_channel(y[o0], pts, b0, parts, k, s)
        assert stray == 0 and b <= 1e-12 and t <= 1e-12, (b, t, stray)
        m2 = MatrixModel(nparts, pts, inputs, outputs, cap=nblocks)
        m2.push_ir(cx.matrix_entry(inputs, outputs, pts, nparts, i0, o0, parts, k))
        assert not m2.process(np.roll(x, 1, axis=0)).any()


# ---- direct convolution -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("irsize,vsize,taps,nblocks", [(16, 8, None, None), (65, 7, None, None), (1000, 64, None, None),
                                                      (4097, 32, None, None), (96000, 64, (0, 4096), 80)])
def test_oracle_unit_tap_is_an_exact_delay(irsize, vsize, taps, nblocks):
    """(96000 taps: two taps over 80 blocks, the oracle's serial sum is slow)"""
    nblocks = nblocks or cx.dconv_blocks_needed(irsize, vsize)
    x = cx.nonzero_noise([irsize, vsize], nblocks * vsize)
    for k in taps or cx.dconv_taps(irsize):
        o = oracle.Dconv(irsize, vsize)
        o.push_ir(cx.unit_tap(irsize, k))
        got = np.concatenate([o.convolution(x[j * vsize:(j + 1) * vsize]) for j in range(nblocks)])
        assert np.array_equal(got, cx.dconv_delayed(x, k)), "tap %d" % k


@pytest.mark.parametrize("irsize,vsize", [(16, 8), (65, 7)])
def test_oracle_time_varying_unit_samples_equal_the_contract(irsize, vsize):
    nblocks = cx.dconv_blocks_needed(irsize, vsize, wraps=3)
    x1 = cx.nonzero_noise([irsize, vsize, 1], nblocks * vsize)
    x2 = cx.dconv_tv_impulses(irsize, vsize, nblocks)
    assert np.count_nonzero(x2) >= 3
    o = oracle.Dconv(irsize, vsize)
    got = np.concatenate([o.convolution(x1[j * vsize:(j + 1) * vsize], x2[j * vsize:(j + 1) * vsize]) for j in range(nblocks)])
    want = cx.dconv_tv_expected(irsize, vsize, x1, x2)[0]
    assert np.count_nonzero(want) > irsize
    assert np.array_equal(got, want)
