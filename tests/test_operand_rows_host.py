"""autograd._rows, the one helper that turns a cotangent or a row input into what the C entries take (unit column stride, a row pitch of
at least the width), on every layout of tests/operand_layouts.py: equal values, a legal pitch, no copy of a tensor that already
qualifies -- and, over autograd.py's text, no site left that tests the column stride alone.  No GPU."""
import os
import re

import pytest
import torch

import operand_layouts as OL
from pna_amd import autograd as AG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 1), (5, 4), (17, 75), (45, 3)]


def _bases(rows, width, dtype=torch.float32):
    """A random tensor, one of equal rows and one of equal elements: together they admit every layout."""
    gen = torch.Generator().manual_seed(rows * 131 + width)
    rnd = torch.randn(rows, width, generator=gen)
    if dtype is torch.int64:
        rnd = (rnd * 10).to(torch.int64)
    rnd = rnd.to(dtype)
    return [rnd, rnd[:1].repeat(rows, 1), rnd[:1, :1].repeat(rows, width)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.int64])
@pytest.mark.parametrize("rows,width", SHAPES)
def test_rows_returns_equal_values_at_a_legal_pitch_and_copies_only_what_does_not_qualify(rows, width, dtype):
    seen = set()
    for base in _bases(rows, width, dtype):
        for name, v in OL.layouts(base):
            seen.add(name)
            assert torch.equal(v, base), name                                        # (the helper module itself: same values)
            r = AG._rows(v)
            assert r.shape == v.shape and r.dtype == v.dtype and torch.equal(r, base), name
            assert r.stride(1) == 1 and r.stride(0) >= width, (name, r.stride())
            if name in OL.NO_COPY:
                assert r.data_ptr() == v.data_ptr() and r.stride() == v.stride() and r is v, name
            elif width > 1:
                assert r.data_ptr() != v.data_ptr(), name                            # (width 1: a transposed column is a contiguous one)
    assert seen == set(OL.NAMES)


def test_the_layouts_have_the_strides_their_names_say():
    base = _bases(6, 4)
    got = {name: v.stride() for b in base for name, v in OL.layouts(b)}
    assert got == {"contiguous": (4, 1), "pitched": (7, 1), "sliced_rows": (8, 1), "transposed": (1, 6), "expanded_rows": (0, 1), "expanded_all": (0, 0)}
    assert [n for n, _ in OL.layouts(base[0])] == ["contiguous", "pitched", "sliced_rows", "transposed"]      # random rows: nothing to expand
    wide = OL.layout(base[0], "pitched")
    assert bool(torch.isnan(wide._base).sum() == 6 * 3)                              # NaN wherever the view does not look


def test_rows_leaves_at_most_one_row_alone_and_still_fixes_its_column_stride():
    one = torch.randn(1, 8)
    assert AG._rows(one) is one and AG._rows(one.expand(1, 8)).data_ptr() == one.data_ptr()
    none = torch.randn(0, 8)
    assert AG._rows(none) is none
    col = torch.randn(8, 3)[:, :1].t()                                               # (1, 8) with column stride 3
    assert col.stride(1) == 3 and AG._rows(col).stride(1) == 1 and torch.equal(AG._rows(col), col)


def test_no_backward_or_forward_of_autograd_tests_the_column_stride_alone():
    """Every cotangent and row input goes through _rows: the one-sided `t if t.stride(1) == 1 else t.contiguous()` lets an expanded
    tensor (pitch 0) through to a C entry that refuses it."""
    src = open(os.path.join(ROOT, "pna_amd", "autograd.py")).read()
    assert not re.findall(r"stride\(1\) == 1 else", src)
    assert "_gru_rows" not in src and src.count("def _rows(") == 1
    # every backward that hands a cotangent's pitch to a C entry normalises the cotangent with the helper first
    for m in re.finditer(r"def (backward\(ctx, (\w+)\)|_tower_train_backward\(ctx, (\w+), lead\)):", src):
        name = m.group(2) or m.group(3)
        end = src.find("\n    @staticmethod", m.end())
        nxt = src.find("\ndef ", m.end())
        cls = src.find("\nclass ", m.end())
        body = src[m.end():min(x for x in (end, nxt, cls, len(src)) if x > 0)]
        if f"{name}.stride(0)" in body:
            assert f"{name} = _rows({name})" in body, m.group(0)
            assert body.index(f"{name} = _rows({name})") < body.index(f"{name}.stride(0)"), m.group(0)
