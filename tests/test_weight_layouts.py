"""Host test of the weight-layout table (nnr_amd.ops.LAYOUTS): every kind's extents / strides / offset applied to a CPU array with
numpy's as_strided equal the torch.permute / flip statement of the layout (tests/layout_ref.py).  No device, no library call."""
import numpy as np
import pytest
import torch
from numpy.lib.stride_tricks import as_strided

import layout_ref


@pytest.mark.parametrize('kind,dims', layout_ref.CASES, ids=lambda v: v if isinstance(v, str) else 'x'.join(map(str, v)))
def test_layout_table_matches_the_permute_expression(kind, dims):
    from nnr_amd import ops
    n, si, so, off, shape = ops.LAYOUTS[kind](*dims)
    src = layout_ref.source(kind, dims)
    s = src.numpy().ravel()
    # every address the table names lies inside the source / the destination
    for strides, base, size in ((si, off, s.size), (so, 0, int(np.prod(shape)))):
        lo = base + sum((m - 1) * st for m, st in zip(n, strides) if st < 0)
        hi = base + sum((m - 1) * st for m, st in zip(n, strides) if st > 0)
        assert 0 <= lo and hi < size, (kind, dims)
    assert so[3] == 1                                  # the destination's unit-stride axis is the fastest index
    dst = np.full(int(np.prod(shape)), np.nan, dtype=np.float32)
    as_strided(dst, n, [4 * v for v in so])[...] = as_strided(s[off:], n, [4 * v for v in si])
    exp = layout_ref.expected(kind, src, dims, torch.full(shape, float('nan')))
    assert np.array_equal(dst.reshape(shape), exp.numpy(), equal_nan=True)
    # a destination element is written at most once, and the pad elements are exactly the ones no index reaches
    hits = np.zeros(dst.size, dtype=np.int32)
    np.add.at(hits, as_strided(np.arange(dst.size), n, [8 * v for v in so]).ravel(), 1)
    assert hits.max() == 1 and np.array_equal(hits == 0, np.isnan(dst))
