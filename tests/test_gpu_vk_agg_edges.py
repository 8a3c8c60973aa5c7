"""GPU tests of Verkey::aggregate from the resident issuer table (k_vk_agg_fixed<Fp, 8>, k_vk_agg_fixed_g2pl<8>,
cc_set_issuers) on the rows of tests/vk_agg_edges.py, whose branch coverage tests/test_vk_agg_edges_model.py
asserts on the CPU.  Every comparison is byte equality with the C oracle's oc_verkey_aggregate on the row's own
keys.

* per (mode, width): every build of V.builds() is handed to cc_set_issuers in a shuffled order, then every
  row, with len = t and with two trailing ids no table holds, goes through cc_verkey_aggregate_ids,
  cc_verkey_aggregate_ids_device (the context's stream and a caller's; a sentinel behind outX and outY
  survives) and cc_aggregate_credential_batch_device (both streams; its sigma outputs equal
  cc_signature_aggregate_batch_device's): the same bytes from all of them.  q = 0 passes no Y and a NULL
  outY; rows tiled to 1, 31, 32, 33 and 65 tasks (q = 0), 32 and 34 (q = 1), 36 and 66 (q = 5: a credential's
  six tasks straddle a block of 32);
* the same table sorted, reversed and shuffled gives the same bytes;
* a duplicated issuer id is CC_ERR_DECODE and leaves CC_ERR_STATE behind;
* an unknown id at positions 0 .. 7, 8 and t - 1 of a t = 17 row among neighbours in its block: the device
  forms write the identity for that row alone and raise the error word once, the host form returns
  CC_ERR_DECODE, and the next call is right.

What the file notices, measured on an MI355X with one change at a time, each run once and never committed:
ft_digit without its `k[i + 1] << (32 - sh)` term fails test_rows_through_three_entries at widths 10, 12 and 13
in both modes and passes at 8 and 16 (the golden issuer-table tests at those three widths fail with it too:
their random coefficients fill every window); cc_set_issuers copying the keys in the caller's order instead of
through its sort permutation fails all 16 tests here (every build is handed over unsorted; in
test_issuer_order_does_not_matter the sorted table passes and the reversed one fails), while the 37 other
issuer-table tests of the suite, whose callers all pass sorted ids, pass.
"""
import ctypes
import random
import sys

import numpy as np
import pytest

import vk_agg_edges as V
from conftest import ROOT
from fixed_edges import G1_IDENTITY, G2_IDENTITY, R, gen_mul

sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

MODES = {"G2": 0, "G1": 1}
CC_ERR_DECODE, CC_ERR_STATE = -4, -7
PAD, SENT = 64, 0xA5


@pytest.fixture(scope="module")
def ctxs():
    import coconut
    c = {m: coconut.Context(0, coconut.GroupMode(m)) for m in MODES.values()}
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(scope="module")
def side_stream():
    import torch
    return torch.cuda.Stream(device=0)


@pytest.fixture(scope="module")
def sig_pool(oc):
    """35 valid signature-group points a mode (any valid sigma serves: the fused entry's sigma half is compared
    with cc_signature_aggregate_batch_device on the same rows)."""
    rng = random.Random(4)
    return {m: gen_mul(oc, 2 if m == 0 else 1, [rng.randrange(1, R) for _ in range(35)]) for m in MODES.values()}


def _vp(a):
    """The pointer of a numpy array, a torch tensor or None"""
    if a is None:
        return None
    return ctypes.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())


def _set_issuers(ctx, oc, b, order=None):
    from coconut._lib import lib
    ids, X, Y = V.issuer_arrays(oc, b, order)
    ctx.set_table_bits(0, b["wbits"])
    st = lib.cc_set_issuers(ctx.h, len(ids), b["q"], (ctypes.c_uint64 * len(ids))(*ids), X, Y if b["q"] else None)
    assert st == 0, (b["wbits"], b["q"], len(ids), st)
    assert ctx.table_bits()[1] == b["wbits"]


def _host(ctx, q, t, L, idrows, status=0):
    """cc_verkey_aggregate_ids with a sentinel behind both outputs: (X, Y) bytes."""
    from coconut._lib import lib
    n, ob = len(idrows), ctx.mode.other_bytes
    ids = np.ascontiguousarray(np.array(idrows, dtype=np.uint64).reshape(n, L))
    oX = np.full(n * ob + PAD, SENT, dtype=np.uint8)
    oY = np.full(n * q * ob + PAD, SENT, dtype=np.uint8) if q else None
    st = lib.cc_verkey_aggregate_ids(ctx.h, n, L, t, _vp(ids), _vp(oX), _vp(oY))
    assert st == status, (st, status)
    if status:
        return None
    assert bytes(oX[n * ob:]) == bytes([SENT]) * PAD and (oY is None or bytes(oY[n * q * ob:]) == bytes([SENT]) * PAD)
    return bytes(oX[:n * ob]), bytes(oY[:n * q * ob]) if q else b""


def _device(ctx, q, t, L, idrows, stream, sigs=None, errword=0):
    """cc_verkey_aggregate_ids_device, or with sigs = (s1, s2 device tensors) the fused entry, on `stream` (None:
    the context's) with a sentinel behind outX and outY: (X, Y[, sigma_1, sigma_2]) bytes."""
    import torch
    from coconut._lib import lib
    n, ob, sb = len(idrows), ctx.mode.other_bytes, ctx.mode.sig_bytes
    dev = torch.device("cuda", 0)
    d_ids = torch.from_numpy(np.array(idrows, dtype=np.uint64).reshape(-1).view(np.int64).copy()).to(dev)
    oX = torch.full((n * ob + PAD,), SENT, dtype=torch.uint8, device=dev)
    oY = torch.full((n * q * ob + PAD,), SENT, dtype=torch.uint8, device=dev) if q else None
    sp = ctypes.c_void_p(stream.cuda_stream) if stream is not None else None
    torch.cuda.synchronize()
    if sigs is None:
        st = lib.cc_verkey_aggregate_ids_device(ctx.h, n, L, t, _vp(d_ids), _vp(oX), _vp(oY), sp)
        extra = ()
    else:
        o1, o2 = (torch.zeros(n * sb, dtype=torch.uint8, device=dev) for _ in range(2))
        st = lib.cc_aggregate_credential_batch_device(ctx.h, n, L, t, _vp(d_ids), _vp(sigs[0]), _vp(sigs[1]), _vp(o1),
                                                      _vp(o2), _vp(oX), _vp(oY), sp)
        extra = (o1, o2)
    assert st == 0, st
    assert ctx.device_error(sp) == errword  # synchronises the stream
    assert ctx.device_error(sp) == 0  # read once, then clear
    X, Y = bytes(oX.cpu().numpy()), bytes(oY.cpu().numpy()) if q else bytes([SENT]) * PAD
    assert X[n * ob:] == bytes([SENT]) * PAD and Y[n * q * ob:] == bytes([SENT]) * PAD
    return (X[:n * ob], Y[:n * q * ob]) + tuple(bytes(o.cpu().numpy()) for o in extra)


def _sig_reference(ctx, t, L, idrows, sigs):
    import torch
    from coconut._lib import lib
    n, sb = len(idrows), ctx.mode.sig_bytes
    dev = torch.device("cuda", 0)
    d_ids = torch.from_numpy(np.array(idrows, dtype=np.uint64).reshape(-1).view(np.int64).copy()).to(dev)
    o1, o2 = (torch.zeros(n * sb, dtype=torch.uint8, device=dev) for _ in range(2))
    torch.cuda.synchronize()
    assert lib.cc_signature_aggregate_batch_device(ctx.h, n, L, t, _vp(d_ids), _vp(sigs[0]), _vp(sigs[1]), _vp(o1), _vp(o2),
                                                   None) == 0
    torch.cuda.synchronize()
    return bytes(o1.cpu().numpy()), bytes(o2.cpu().numpy())


def _sigs(ctx, pool, n, L):
    import torch
    sb = ctx.mode.sig_bytes
    s = torch.frombuffer(bytearray(pool[:L * sb] * n), dtype=torch.uint8).to(torch.device("cuda", 0))
    return s, s


def _three_entries(ctx, q, t, L, idrows, side, pool, what):
    """The rows through the host form, the device form and the fused entry, the latter two on both streams:
    one (X, Y), the same from all."""
    want = _host(ctx, q, t, L, idrows)
    sigs = _sigs(ctx, pool, len(idrows), L)
    sref = _sig_reference(ctx, t, L, idrows, sigs)
    for stream in (None, side):
        assert _device(ctx, q, t, L, idrows, stream) == want, (what, "device form", stream is not None)
        got = _device(ctx, q, t, L, idrows, stream, sigs)
        assert got[:2] == want, (what, "fused entry", stream is not None)
        assert got[2:] == sref, (what, "fused entry's sigma", stream is not None)
    return want


def _check_rows(oc, b, rows, got, what, n=None):
    """Row i of the n results is rows[i mod len(rows)]'s oracle aggregate."""
    ob, q = (97 if b["mode"] == 0 else 192), b["q"]
    n = len(rows) if n is None else n
    assert len(got[0]) == n * ob and len(got[1]) == n * q * ob
    for i in range(n):
        r = rows[i % len(rows)]
        wX, wY = V.oracle_row(oc, b, r)
        assert got[0][i * ob:(i + 1) * ob] == wX, (what, r["name"], i, "X")
        assert got[1][i * q * ob:(i + 1) * q * ob] == wY, (what, r["name"], i, "Y")


def _groups(b):
    out = {}
    for r in b["rows"]:
        out.setdefault(r["t"], []).append(r)
    return out


@pytest.mark.parametrize("wbits", V.WIDTHS)
@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_rows_through_three_entries(ctxs, oc, side_stream, sig_pool, mode, wbits):
    m = MODES[mode]
    ctx, pool = ctxs[m], sig_pool[m]
    tiled = set()
    for bi, b in enumerate(V.builds(m, wbits)):
        assert b["bytes"] <= V.LIMIT
        _set_issuers(ctx, oc, b)
        q = b["q"]
        groups = _groups(b)
        for t, rows in groups.items():
            for extra in (0, 2):  # two trailing ids no table holds: not among the first t, ignored
                idrows = [r["ids"] + list(V.UNKNOWN[:extra]) for r in rows]
                what = (mode, wbits, bi, t, extra)
                _check_rows(oc, b, rows, _three_entries(ctx, q, t, t + extra, idrows, side_stream, pool, what), what)
        if q in tiled:
            continue
        tiled.add(q)  # task counts around one block and above two, on the q's first build
        t, rows = max(groups.items(), key=lambda g: len(g[1]))
        for n in V.TASK_ROWS[q]:
            idrows = [rows[i % len(rows)]["ids"] for i in range(n)]
            what = (mode, wbits, bi, t, "tiled", n)
            _check_rows(oc, b, rows, _three_entries(ctx, q, t, t, idrows, side_stream, pool, what), what, n)


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_issuer_order_does_not_matter(ctxs, oc, mode):
    """cc_set_issuers sorts the ids and carries every key along: sorted, reversed and shuffled tables agree."""
    m = MODES[mode]
    ctx = ctxs[m]
    b = next(b for b in V.builds(m, 8) if b["q"] == 1)
    orders = {"sorted": sorted(b["ids"]), "reversed": sorted(b["ids"], reverse=True), "shuffled": list(b["ids"])}
    random.Random(99).shuffle(orders["shuffled"])
    assert len({tuple(o) for o in orders.values()}) == 3
    got = {}
    for name, order in orders.items():
        _set_issuers(ctx, oc, b, order)
        got[name] = []
        for t, rows in _groups(b).items():
            res = _host(ctx, b["q"], t, t, [r["ids"] for r in rows])
            _check_rows(oc, b, rows, res, (mode, name, t))
            got[name].append(res)
    assert got["sorted"] == got["reversed"] == got["shuffled"]


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_duplicate_issuer_id_leaves_no_table(ctxs, oc, mode):
    from coconut._lib import lib
    m = MODES[mode]
    ctx = ctxs[m]
    b = next(b for b in V.builds(m, 8) if b["q"] == 5)
    _set_issuers(ctx, oc, b)
    rows = _groups(b)[3]
    good = _host(ctx, 5, 3, 3, [r["ids"] for r in rows])
    ids, X, Y = V.issuer_arrays(oc, b)
    dup = list(ids)
    dup[-1] = dup[1]  # not neighbours before the sort
    assert lib.cc_set_issuers(ctx.h, len(dup), 5, (ctypes.c_uint64 * len(dup))(*dup), X, Y) == CC_ERR_DECODE
    _host(ctx, 5, 3, 3, [r["ids"] for r in rows], status=CC_ERR_STATE)
    one = np.zeros(8, dtype=np.uint64)
    assert lib.cc_verkey_aggregate_ids_device(ctx.h, 1, 1, 1, _vp(one), _vp(one), _vp(one), None) == CC_ERR_STATE
    _set_issuers(ctx, oc, b)
    assert _host(ctx, 5, 3, 3, [r["ids"] for r in rows]) == good
    _check_rows(oc, b, rows, good, (mode, "after a failed cc_set_issuers"))


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_unknown_id_at_every_lane_and_round(ctxs, oc, side_stream, sig_pool, mode):
    m = MODES[mode]
    ctx, pool = ctxs[m], sig_pool[m]
    ob = ctx.mode.other_bytes
    ident = G1_IDENTITY if m == 0 else G2_IDENTITY
    b, row = next((b, r) for b in V.builds(m, 8) for r in b["rows"] if r["t"] == 17)
    _set_issuers(ctx, oc, b)
    t, q, n, victim = 17, b["q"], 5, 2  # at most 10 tasks: one block
    base = [row["ids"][i:] + row["ids"][:i] for i in range(n)]  # the same id set: the same aggregate from every row
    good = _host(ctx, q, t, t, base)
    wX, wY = V.oracle_row(oc, b, row)
    assert good == (wX * n, wY * n)
    sigs = _sigs(ctx, pool, n, t)
    for pos in list(range(8)) + [8, t - 1]:
        idrows = [list(r) for r in base]
        idrows[victim][pos] = V.UNKNOWN[pos % 2]
        want = (b"".join(ident if i == victim else wX for i in range(n)),
                b"".join(ident * q if i == victim else wY for i in range(n)))
        stream = side_stream if pos % 2 else None
        assert _device(ctx, q, t, t, idrows, stream, errword=1) == want, (mode, pos, "device form")
        assert _device(ctx, q, t, t, idrows, stream, sigs, errword=1)[:2] == want, (mode, pos, "fused entry")
        assert _device(ctx, q, t, t, base, stream) == good, (mode, pos, "the next call")
        _host(ctx, q, t, t, idrows, status=CC_ERR_DECODE)
        assert _host(ctx, q, t, t, base) == good, (mode, pos, "the host form after its error")
    assert ob * n == len(good[0])
