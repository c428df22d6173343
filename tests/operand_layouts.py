"""The storage layouts an operand of the one-call routes can arrive in: `layouts(t)` yields (name, variant) pairs of a 2-D tensor, every
variant holding t's values in another arrangement of memory.  A helper module like tower_train_cases, imported by the tests
(test_operand_rows_host.py, test_gpu_train_operand_layouts.py); it collects nothing itself.

    contiguous      row-major, pitch = width
    pitched         a column slice of a wider tensor: unit column stride, pitch = width + 3 (what autograd hands a layer whose output is
                    one block of a torch.cat)
    sliced_rows     every second row of a tensor of twice the rows: pitch = 2 width
    transposed      t.t().contiguous().t(): column stride != 1 (a weight re-stored by a conversion script)
    expanded_rows   one row expanded, strides (0, 1) -- only where all rows of t are equal (the cotangent of (out.sum(0) * c).sum())
    expanded_all    one element expanded, strides (0, 0) -- only where all elements of t are equal (the cotangent of out.sum())

What a view does not cover is poisoned: NaN in a floating-point tensor, -1 in an integer one, so a read past the width shows."""
import torch

NO_COPY = ("contiguous", "pitched", "sliced_rows")          # unit column stride and pitch >= width: the routes take them as they are
COPIED = ("transposed", "expanded_rows", "expanded_all")
NAMES = NO_COPY + COPIED


def _poison(shape, like):
    return torch.full(shape, float("nan") if like.is_floating_point() else -1, dtype=like.dtype, device=like.device)


def layouts(t):
    """(name, variant) for every layout t's values admit; each variant equals t elementwise and shares no memory with it."""
    assert t.dim() == 2
    rows, width = t.shape
    t = t.detach()
    yield "contiguous", t.contiguous().clone()
    wide = _poison((rows, width + 3), t)
    wide[:, 1:1 + width] = t
    yield "pitched", wide[:, 1:1 + width]
    tall = _poison((2 * rows, width), t)
    tall[::2] = t
    yield "sliced_rows", tall[::2]
    yield "transposed", t.t().contiguous().t()
    if rows and bool((t == t[:1]).all()):
        yield "expanded_rows", t[:1].contiguous().clone().expand(rows, width)
        if width and bool((t == t[:1, :1]).all()):
            yield "expanded_all", t[:1, :1].contiguous().clone().expand(rows, width)


def layout(t, name):
    """The one variant `name` of t."""
    for n, v in layouts(t):
        if n == name:
            return v
    raise KeyError(f"{name}: not a layout of this tensor (an expanded layout needs equal rows)")
