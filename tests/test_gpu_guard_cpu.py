"""tests/gpu_guard.py, run on CPU tensors: mutation tests of the checker the device tests rest on.  A clean write passes; one
word written anywhere in a guard, and one element left unwritten, must each fail the check that is there for it.  The
guard widths are the call sites' (1024 words before, 1024 + 4 after), the views a few dozen elements."""
import numpy as np
import pytest
import torch

from tests import gpu_guard as gg

f32 = np.float32
FORMS = {
    "flat": lambda misalign=2: gg.flat((2, 3, 5), misalign=misalign, device="cpu"),
    "flat complex": lambda misalign=0: gg.flat((3, 4), torch.complex64, misalign=misalign, before=2048, after=2048, device="cpu"),
    "rows": lambda misalign=1: gg.rows(3, 7, 12, misalign=misalign, device="cpu"),
}
forms = pytest.mark.parametrize("form", list(FORMS))


def written(form, **kw):
    g = FORMS[form](**kw)
    g.data.fill_(1.5)
    return g


def strays(g):
    """(where, index into buf, the message of check_sides) of one word in every part of the guard: next to the view and
    at the far end of each band, and for rows the first and last word of a gap and the gap behind the last row"""
    n = g.buf.numel()
    out = [("just before", g.lo - 1, "wrote before it"), ("the first word", 0, "wrote before it"),
           ("just after", g.hi, "wrote after it"), ("the last word", n - 1, "wrote after it")]
    nrows, stride = g.body.shape
    rowlen = g.words.shape[1]
    if stride > rowlen:
        out += [("behind row 0", g.lo + rowlen, "wrote between the rows"),
                ("before row 1", g.lo + stride - 1, "wrote between the rows"),
                ("behind the last row", g.lo + (nrows - 1) * stride + rowlen, "wrote between the rows")]
    return out


@forms
def test_a_clean_write_passes(form):
    g = written(form)
    assert g.intact() and g.sides() == (True, True, True) and g.unwritten() == 0 and not g.untouched()
    g.check_sides("it")
    assert g.data.numel() * (2 if g.data.is_complex() else 1) == g.words.numel() == int(g.mask.sum())
    assert bool((g.buf[g.mask] != gg.CANARY).all()) and bool((g.buf[~g.mask] == gg.CANARY).all())


@forms
def test_one_stray_word_anywhere_fails(form):
    seen = set()
    for where, i, message in strays(written(form)):
        g = written(form)
        assert not g.mask[i], where
        g.buf[i] = 0
        assert not g.intact(), where
        assert g.unwritten() == 0, where
        with pytest.raises(AssertionError, match=message):
            g.check_sides("it")
        seen.add(message)
    assert len(seen) == (3 if form == "rows" else 2)


@forms
def test_one_unwritten_element_fails(form):
    g = written(form)
    nrows, rowlen = g.words.shape
    for r, c in ((0, 0), (nrows - 1, rowlen - 1), (nrows // 2, rowlen // 2)):
        g = written(form)
        g.words[r, c] = gg.CANARY
        assert g.unwritten() == 1 and g.intact()
    g.words[0, 0] = gg.CANARY
    assert g.unwritten() == 2


@forms
def test_untouched_until_the_first_write(form):
    g = FORMS[form]()
    assert g.untouched() and g.intact() and g.unwritten() == g.words.numel()
    g.words[0, 3] = 0
    assert not g.untouched()
    g = FORMS[form]()
    g.buf[-1] = 0           # a write into the guard alone
    assert not g.untouched()


@forms
@pytest.mark.parametrize("misalign", [0, 2])
def test_alignment(form, misalign):
    g = FORMS[form](misalign=misalign)
    assert g.data.data_ptr() % 16 == 4 * misalign and g.buf.data_ptr() % 16 == 0
    assert g.lo >= 1024 and g.buf.numel() - g.hi >= 1024


def test_the_alignment_assertion_can_fail():
    with pytest.raises(AssertionError):
        gg.flat((4,), misalign=2, before=1023, device="cpu")
    with pytest.raises(AssertionError):
        gg.rows(2, 4, 6, misalign=0, before=1022, device="cpu")


def test_shapes_and_dtypes():
    g = FORMS["flat"]()
    assert g.data.shape == (2, 3, 5) and g.data.dtype == torch.float32 and g.data.is_contiguous()
    g = FORMS["flat complex"]()
    assert g.data.shape == (3, 4) and g.data.dtype == torch.complex64 and g.words.numel() == 24
    g = FORMS["rows"]()
    assert g.data.shape == (3, 7) and g.data.stride() == (12, 1)
    assert [r.data_ptr() - g.data.data_ptr() for r in g.data] == [0, 48, 96]


def test_fill_unchanged_and_host():
    x = np.arange(21, dtype=f32).reshape(3, 7)
    g = FORMS["rows"]().fill(x)
    assert g.unchanged() and g.intact() and g.unwritten() == 0
    assert np.array_equal(g.host(), x)
    g.data[1, 2] = -1.0
    assert not g.unchanged()
    g = FORMS["rows"]().fill(x)
    g.buf[g.lo + 8] = 0     # a gap word
    assert not g.unchanged() and not g.intact()


def test_same():
    want = np.array([1.0, np.nan, -0.0, 3.5], f32)
    got = want.copy()
    gg.bits(got)[1] = 0x7FC00001        # another NaN payload, and the canary's own
    gg.same(got, want, "payloads")
    gg.bits(got)[1] = gg.CANARY
    gg.same(got, want, "the canary is a NaN")
    assert np.isnan(got[1])
    one_ulp = want.copy()
    gg.bits(one_ulp)[3] += 1
    with pytest.raises(AssertionError, match="one ulp"):
        gg.same(one_ulp, want, "one ulp")
    zero = want.copy()
    zero[2] = 0.0
    with pytest.raises(AssertionError, match="the sign of zero"):
        gg.same(zero, want, "the sign of zero")
    number = want.copy()
    number[1] = 2.0
    with pytest.raises(AssertionError, match="where the NaNs are"):
        gg.same(number, want, "a number for a NaN")
    with pytest.raises(AssertionError, match="where the NaNs are"):
        gg.same(want, number, "a NaN for a number")


def test_bits_and_dev():
    a = np.arange(12, dtype=f32).reshape(3, 4)
    assert gg.bits(f32(1.0)) == 0x3F800000 and gg.bits(a[:, ::2]).shape == (3, 2)
    a.setflags(write=False)
    t = gg.dev(a, device="cpu")
    t[0, 0] = 7.0           # a copy: the read-only source keeps its value
    assert a[0, 0] == 0.0 and t.dtype == torch.float32 and t.shape == (3, 4)
    assert gg.dev(a.T, device="cpu").is_contiguous()
    assert gg.dev(np.ones(3, np.complex64), device="cpu").dtype == torch.complex64


def test_run():
    def clean(o):
        o.copy_(torch.arange(6.0).view(2, 3))
        return 0

    out = gg.run(clean, (2, 3), device="cpu")
    assert isinstance(out, np.ndarray) and np.array_equal(out, np.arange(6, dtype=f32).reshape(2, 3))

    def base(o):            # the whole buffer behind the view, as int32
        return torch.tensor([], dtype=torch.int32).set_(o.untyped_storage())

    def before(o):
        clean(o)
        base(o)[1024 + 2 - 1] = 0
        return 0

    def after(o):
        clean(o)
        base(o)[1024 + 2 + 6] = 0
        return 0

    def short(o):
        o.view(-1)[:5] = 0.0
        return 0

    for call in (before, after):
        with pytest.raises(AssertionError, match="wrote outside the output"):
            gg.run(call, (2, 3), device="cpu")
    with pytest.raises(AssertionError, match="an output element was not written"):
        gg.run(short, (2, 3), device="cpu")
    with pytest.raises(AssertionError):
        gg.run(lambda o: clean(o) - 30, (2, 3), device="cpu")
