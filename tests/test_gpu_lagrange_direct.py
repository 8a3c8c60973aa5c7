"""k_lagrange (csrc/aggregate.hip) called directly: cck_lagrange(n, len, t, d_ids, d_l, NULL) through
ctypes on torch device buffers with the null stream, the way tests/test_gpu_miller_wide_direct.py calls
its kernels.  The output is filled with 0xC3 beforehand and followed by sentinel words; the return code,
every output row and the sentinels are asserted.

Small shapes are compared row by row with the oracle's oc_lagrange; the launches either side of the
switch from ids staged in LDS to ids read from global memory (field_edges.largest_lds_t(), from the
launcher's own expression) are compared with Python integers on sampled entries and through the power
sums of the Lagrange basis on all of them.  Ids, shapes and samples come from tests/field_edges.py
(tests/test_field_edges_model.py asserts what they cover).
"""
import ctypes

import numpy as np
import pytest

import field_edges as F

pytestmark = pytest.mark.gpu

R = F.R
SENT = 64       # sentinel words after the output
FILL = 0xC3


@pytest.fixture(scope="module")
def K():
    from coconut._lib import lib
    sz, p = ctypes.c_size_t, ctypes.c_void_p
    lib.cck_lagrange.argtypes, lib.cck_lagrange.restype = [sz, sz, sz, p, p, p], ctypes.c_int
    return lib


def lagrange(K, n, ln, t, rows):
    """One launch over rows (n lists of ln ids); returns the n t coefficients as integers."""
    import torch
    dev = torch.device("cuda", 0)
    ids = np.array(rows, dtype=np.uint64).reshape(-1)
    assert ids.size == n * ln
    d_ids = torch.from_numpy(ids.view(np.int64).copy()).to(dev)
    d_l = torch.full(((n * t * 8 + SENT) * 4,), FILL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rc = K.cck_lagrange(n, ln, t, ctypes.c_void_p(d_ids.data_ptr()), ctypes.c_void_p(d_l.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == 0
    out = d_l.cpu().numpy()
    assert bytes(out[n * t * 32:]) == bytes([FILL]) * (4 * SENT), "written past n t 8 words"
    assert np.array_equal(d_ids.cpu().numpy().view(np.uint64), ids)
    return [int.from_bytes(bytes(out[32 * k:32 * (k + 1)]), "little") for k in range(n * t)]


@pytest.mark.parametrize("t,n,ln", F.small_cases())
def test_small_shapes_against_the_oracle(K, oc, t, n, ln):
    kinds, rows = F.small_ids(t, n, ln)
    got = lagrange(K, n, ln, t, rows)
    for c, row in enumerate(rows):
        buf = ctypes.create_string_buffer(48 * t)
        oc.oc_lagrange(ctypes.c_size_t(t), (ctypes.c_uint64 * t)(*row[:t]), buf)
        want = [int.from_bytes(buf.raw[48 * k:48 * (k + 1)], "big") for k in range(t)]
        assert got[c * t:(c + 1) * t] == want, (t, n, ln, c, kinds[c])


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("side", ["lds", "global"])
def test_either_side_of_the_lds_switch(K, side, n):
    """t = the largest value whose ids are staged in LDS (a dynamic request of exactly 64 KiB) and t + 1,
    ids read from global memory; len = t + 1."""
    t = F.largest_lds_t() + (side == "global")
    assert (F.lds_bytes(t) <= 64 * 1024) == (side == "lds")
    rows = F.switch_ids(t, n)
    got = lagrange(K, n, t + 1, t, rows)
    for task in F.switch_samples(t, n, rows):
        c, i = divmod(task, t)
        assert got[task] == F.lagrange_at(rows[c][:t], i), (side, n, c, i)
    for c, row in enumerate(rows):
        ids, l = row[:t], got[c * t:(c + 1) * t]
        where = {}
        for i, x in enumerate(ids):
            assert l[i] < R
            assert l[where.setdefault(x, i)] == l[i], (side, n, c, i)      # equal ids, equal coefficients
        assert len(where) == t - (c == 0)
        sums = [0, 0, 0, 0]
        for x, i in where.items():                                         # first occurrences
            xk = 1
            for k in range(4):
                sums[k] = (sums[k] + l[i] * xk) % R
                xk = xk * x % R
        assert sums == [1, 0, 0, 0], (side, n, c)
        if 0 in ids:
            assert [l[i] for i in range(t) if ids[i] == 0] == [1] and sum(l) == 1


def test_empty_calls_write_nothing(K):
    import torch
    dev = torch.device("cuda", 0)
    d_ids = torch.ones((8,), dtype=torch.int64, device=dev)
    d_l = torch.full((256,), FILL, dtype=torch.uint8, device=dev)
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    for n, ln, t in ((0, 4, 4), (2, 4, 0), (0, 0, 0)):
        assert K.cck_lagrange(n, ln, t, p(d_ids), p(d_l), None) == 0
    torch.cuda.synchronize()
    assert bytes(d_l.cpu().numpy()) == bytes([FILL]) * 256
