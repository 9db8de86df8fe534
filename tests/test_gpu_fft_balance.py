"""The resident n = 65536 kernel's transform assignment (opencl_fft_amd/csrc/fft_resident.hip): the static one and the
shared one (positions drawn from per-XCD counters, the tail taken over by the XCDs that finish early), at the batches
where an assignment can go wrong on 256 CUs — below, at and just above one transform per workgroup, ragged tails, several
windows.  Every transform has to run exactly once, whoever runs it; nothing may be written outside the batch or, in the
plan's workspace, outside the first word of each counter line (a guard line lies on either side of the counters); and the
counters have to be zero again when a launch has ended, ready for the next.

Which workgroup takes which transform depends on timing, so no test asserts that a steal happened: only sums."""
import numpy as np
import pytest

import opencl_fft_amd as fa
from tests.gpu_guard import flat
from tests.util import TOL, lcg_complex, rel_err

pytestmark = pytest.mark.gpu

N = 65536
BATCHES = [255, 256, 257, 300, 511, 513, 777, 1029]
ROWS = 64          # rows per chunk of float64 reference on the device (64 MiB)


@pytest.fixture(scope="module")
def plans():
    out = {}
    for fwd in (True, False):
        p = fa.Clcfft(0, N, fwd)
        assert p.get_error() == 0, p.get_log()
        assert p.kernel_name() == "k_fft_res16"
        out[fwd] = p
    return out


GUARD_WORD = 0xA5A5A5A5
INVALID_OPERATION = -59    # CLFA_INVALID_OPERATION (include/clfft_amd.h)


def _counters_clean(plan):
    """after a launch: the guard lines in front of and behind the counters hold their pattern, and every word of the nine
    counter lines is zero again"""
    before, lines, after = plan.balance_counters()
    assert (before == GUARD_WORD).all(), "the guard line in front of the counters was written: %s" % before
    assert (after == GUARD_WORD).all(), "the guard line behind the counters was written: %s" % after
    assert not lines.any(), "the counters are not zero after the launch: %s" % lines[:, 0]


def _run(plan, src, batch, oop):
    """one launch on the guarded input; returns the guarded buffer that holds the result"""
    import torch
    if not oop:
        assert plan.exec_device(src.data, batch) == 0
        dst = src
    else:
        dst = flat((batch, N), torch.complex64, misalign=2)
        src.kept = src.buf.clone()
        assert plan.exec_device_oop(src.data, dst.data, batch) == 0
    torch.cuda.synchronize()
    _counters_clean(plan)
    assert dst.intact(), "wrote outside the batch"
    assert not dst.unwritten(), "an output element was not written"
    if oop:
        assert src.unchanged(), "the source of an out-of-place call was written"
    return dst


def _impulses(batch):
    """row r: amplitude r + 1 at position 7 r mod N"""
    import torch
    g = flat((batch, N), torch.complex64, misalign=2)
    g.data.zero_()
    r = torch.arange(batch, device=g.data.device)
    g.data[r, (7 * r) % N] = (r + 1).to(torch.complex64)
    return g


def _worst_impulse_error(y, batch, fwd):
    """(worst relL2, worst max / max) over the rows, each against its closed form in float64:
    X[k] = (r + 1) exp(-+ 2 pi i (7 r mod N) k / N), forward divided by N (the criterion of util.assert_parity, per row)"""
    import torch
    k = torch.arange(N, device=y.device, dtype=torch.int64)
    l2w = mxw = 0.0
    for lo in range(0, batch, ROWS):
        hi = min(batch, lo + ROWS)
        r = torch.arange(lo, hi, device=y.device, dtype=torch.int64)
        turn = (((7 * r) % N)[:, None] * k[None, :]) % N
        ang = turn.to(torch.float64) * (2.0 * np.pi / N) * (-1.0 if fwd else 1.0)
        amp = (r + 1).to(torch.float64)[:, None] * (1.0 / N if fwd else 1.0)
        want = torch.complex(amp * torch.cos(ang), amp * torch.sin(ang))
        d = (y[lo:hi].to(torch.complex128) - want).abs()
        l2 = torch.linalg.norm(d, dim=1) / torch.linalg.norm(want.abs(), dim=1)
        mx = d.max(dim=1).values / want.abs().max(dim=1).values
        l2w, mxw = max(l2w, float(l2.max())), max(mxw, float(mx.max()))
    return l2w, mxw


@pytest.mark.parametrize("oop", [False, True], ids=["inplace", "oop"])
@pytest.mark.parametrize("fwd", [True, False], ids=["fwd", "inv"])
@pytest.mark.parametrize("batch", BATCHES)
def test_every_transform_exactly_once(plans, batch, fwd, oop):
    """a skipped row stays an impulse, a row done twice is wrong by a factor: every row against float64"""
    y = _run(plans[fwd], _impulses(batch), batch, oop)
    l2, mx = _worst_impulse_error(y.data, batch, fwd)
    print("BALANCE impulses batch=%d %s %s worst relL2 %.3g max/max %.3g" % (batch, "fwd" if fwd else "inv", "oop" if oop else "in place", l2, mx))
    assert l2 <= TOL and mx <= TOL, "batch=%d fwd=%s oop=%s: relL2=%.3g max/max=%.3g (tol %.1g)" % (batch, fwd, oop, l2, mx, TOL)


@pytest.fixture(scope="module")
def one_transform():
    x = lcg_complex(4711, N)
    x.setflags(write=False)
    return x, {fwd: (np.fft.fft(x.astype(np.complex128)) / N if fwd else np.fft.ifft(x.astype(np.complex128)) * N)
               for fwd in (True, False)}


@pytest.mark.parametrize("oop", [False, True], ids=["inplace", "oop"])
@pytest.mark.parametrize("fwd", [True, False], ids=["fwd", "inv"])
@pytest.mark.parametrize("batch", BATCHES)
def test_result_does_not_depend_on_the_worker(plans, one_transform, batch, fwd, oop):
    """every row holds the same random transform: all output rows are bit-identical to row 0, and row 0 is right"""
    import torch
    x, want = one_transform
    g = flat((batch, N), torch.complex64, misalign=2)
    g.data[:] = torch.from_numpy(x.copy()).to(g.data.device)[None, :]      # a copy: the shared input is read-only
    y = _run(plans[fwd], g, batch, oop).data
    bits = torch.view_as_real(y).view(torch.int32)
    assert bool((bits == bits[0:1]).all()), "rows of one batch differ"
    l2, mx = rel_err(y[0].cpu().numpy(), want[fwd])
    assert l2 <= TOL and mx <= TOL, "row 0: relL2=%.3g max/max=%.3g (tol %.1g)" % (l2, mx, TOL)


@pytest.mark.parametrize("fwd", [True, False], ids=["fwd", "inv"])
@pytest.mark.parametrize("batch", BATCHES)
def test_workgroup_records_add_up(batch, fwd):
    """the per-workgroup record: the counts sum to the batch, and nobody goes without work when there is enough of it;
    twice on one plan (the second launch finds the counters as the first left them: zero)"""
    import torch
    plan = fa.Clcfft(0, N, fwd)
    assert plan.get_error() == 0, plan.get_log()
    assert plan.balance_read() is None
    assert plan.balance_record(True) == 0
    _counters_clean(plan)          # as the plan's creation leaves them
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    g = flat((batch, N), torch.complex64, misalign=2)
    g.data.zero_()
    for launch in range(2):
        assert plan.exec_device(g.data, batch) == 0
        rec = plan.balance_read()
        assert rec is not None and len(rec) == min(batch, cus)
        counts = rec["count"].astype(np.int64)
        assert counts.sum() == batch, (launch, counts)
        if batch >= cus:
            assert counts.min() >= 1, (launch, counts)
        assert np.array_equal(rec["xcd"], np.arange(len(rec)) % 8)
        assert rec["stamp"].min() > 0
        _counters_clean(plan)
    assert g.intact()
    assert plan.balance_record(False) == 0
    assert plan.balance_read() is None


@pytest.mark.parametrize("fwd", [True, False], ids=["fwd", "inv"])
def test_packed_real_plans_have_no_counters(fwd):
    """the packed real size-131072 transforms run on the same kernel with the static assignment: no counters, no record"""
    plan = fa.Clrfft(0, 2 * N, fwd)
    assert plan.get_error() == 0, plan.get_log()
    assert plan.kernel_name() == "k_fft_res16"
    assert plan.balance_record(True) == INVALID_OPERATION
    assert plan.balance_read() is None and plan.balance_counters() is None
    small = fa.Clcfft(0, 4096, fwd)
    assert small.balance_record(True) == INVALID_OPERATION and small.balance_counters() is None
