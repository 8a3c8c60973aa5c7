"""GPU tests of verify_share over commitment sets (csrc/vss.hip, capi_vss.cpp): cc_vss_verify_sets,
cc_vss_verify_sets_device and cc_keygen_verify_shares_batch_device, with rlc = 0 and rlc = 1, against the
cases' intents, the C oracle and cc_vss_verify_batch on the same rows.  The cases are those of
tests/vss_sets_cases.py (modelled on the CPU by tests/test_vss_sets_model.py) and the CSR form of
tests/issuer_edges.py's share lists:
* every (t, h) of issuer_edges' VSS_CALLS under a SigG2 and a SigG1 context: t = 1 .. 33, ids 0 .. 2^64 - 1, shares
  0, r - 1, >= r, identity / off-curve / equal / opposite commitments, h the identity, off the curve and +-g;
* the torsion sets: verdicts equal the oracle's and the host form's, and exactly those sets are irregular;
* the cancelling pairs: rlc = 1 rejects the set and finds both rows;
* the size list 0, 1, 2, 63, 64, 65, 130, 257 with a bad share at set edges and at a block boundary;
* the keygen-shaped call on the device deal's and the device combine's outputs;
* the argument checks, n = 0, a caller stream, sentinels beyond n."""
import ctypes

import numpy as np
import pytest

import issuer_edges as E
import keygen_deal_cases as KC
import vss_sets_cases as V
from fixed_edges import R, be48

pytestmark = pytest.mark.gpu

MODES = {"G2": 0, "G1": 1}
OK, ERR_THRESHOLD, ERR_DECODE, ERR_STATE = 0, -3, -4, -7
VSS_CALLS = [(t, "rand") for t in E.VSS_T] + [(3, h) for h in E.VSS_H[1:]]
SEED_A, SEED_B = bytes(range(32)), bytes(range(100, 132))


@pytest.fixture(scope="module")
def ctxs():
    import coconut
    c = {m: coconut.Context(0, coconut.GroupMode(v)) for m, v in MODES.items()}
    yield c
    for x in c.values():
        x.close()


def _bind(ctx, mode, call):
    ctx.set_keygen_params(KC.base_bytes(mode)[0], call["g"], call["h"], table_bits=8)


def _dev(call, rows, begin):
    """The device form's tensors: (n, t, n_sets, set_begin, commitments, ids, shares)."""
    import torch
    t, sets, begin, ids, shares = V.sets_args(call, rows, begin)
    d = torch.device("cuda", 0)
    up = lambda b: torch.frombuffer(bytearray(b or b"\0"), dtype=torch.uint8).to(d)  # noqa: E731
    idt = torch.from_numpy(np.asarray(ids or [0], dtype=np.uint64).view(np.int64)).to(d)
    out = (len(rows), t, len(sets), begin, up(b"".join(c for s in sets for c in s)), idt,
           up(b"".join(a + b for a, b in shares)))
    torch.cuda.synchronize()  # the uploads run on torch's stream, the calls on the context's
    return out


def _list(v):
    """A verdict tensor on the host, once the context's stream has written it."""
    import torch
    torch.cuda.synchronize()
    return v.cpu().tolist()


def _both(ctx, call, rows, begin, seed=SEED_A):
    """[(name, verdicts, stats)] of the host and the device form with rlc = 0 and rlc = 1."""
    from coconut import vss_verify_sets, vss_verify_sets_device
    out = []
    args = V.sets_args(call, rows, begin)
    dev = _dev(call, rows, begin)
    for rlc in (False, True):
        v, st = vss_verify_sets(ctx, *args, rlc=rlc, want_stats=True)
        out.append((f"host rlc={int(rlc)}", list(map(int, v)), st))
        v, st = vss_verify_sets_device(ctx, *dev, rlc=rlc, seed=seed if rlc else None)
        out.append((f"device rlc={int(rlc)}", _list(v), st))
    return out


def _old(ctx, call, rows):
    from coconut import vss_verify_batch
    return list(map(int, vss_verify_batch(ctx, *V.batch_args(call, rows))))


# ---------------------------------------------------------------- issuer_edges' share lists in the CSR form
@pytest.mark.parametrize("t,hkind", VSS_CALLS)
@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_share_edges_as_sets(oc, ctxs, mode, t, hkind):
    call = E.vss_call(oc, t, hkind)
    _bind(ctxs[mode], mode, call)
    for n, order in ((len(call["cases"]), 0), (130, 1), (1, 0)):
        batch = call["cases"] if n == len(call["cases"]) else E.vss_batch(call, n, order)
        rows, begin = V.csr(call, batch)
        want = [c["intent"] for c in rows]
        assert _old(ctxs[mode], call, rows) == want
        for name, got, st in _both(ctxs[mode], call, rows, begin):
            bad = [(i, c["name"], g) for i, (c, g, w) in enumerate(zip(rows, got, want)) if g != w]
            assert not bad, (name, n, bad)
            assert st[0] == len(call["sets"]) and st[2] == 0, (name, st)  # every point of these calls lies in G1
            if "rlc=0" in name:
                assert st[1] == 0 and st[3] == len(rows), (name, st)


# ---------------------------------------------------------------- torsion: the subgroup gate
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_torsion_sets_take_the_exact_route(oc, ctxs, mode, which):
    """Verdicts equal the C oracle's in the host and the device form, and exactly the sets holding a point outside
    G1 are irregular.  Call 0 (g, h in G1) also equals cc_vss_verify_batch on the same rows.  Call 1 (g = k G + T3)
    is not compared with it: k_vss_verify adds (r - s) g, which for a g of order 3 r is -(s g) + T3, so
    cc_vss_verify_batch differs from the oracle there ([1, 0, 0, 0, 0, 0, 0, 0] against
    [0, 0, 0, 0, 1, 0, 0, 0] on the call's rows); the irregular route hands that kernel -g, -h and r - s, r - s',
    which is the reference's sum whatever the order of g and h."""
    tc = V.torsion_calls(oc)[which]
    call = tc["call"]
    env = E.Env(oc, 1)
    _bind(ctxs[mode], mode, call)
    rows, begin = V.csr(call, call["cases"])
    want = [E.expect_share(env, call, c) for c in rows]
    if which == 0:
        assert _old(ctxs[mode], call, rows) == want
    sizes = [begin[j + 1] - begin[j] for j in range(len(call["sets"]))]
    per_share = [j for j in range(len(sizes)) if j in tc["irregular"] or not all(want[begin[j]:begin[j + 1]])]
    for name, got, st in _both(ctxs[mode], call, rows, begin):
        bad = [(c["name"], g, w) for c, g, w in zip(rows, got, want) if g != w]
        assert not bad, (name, bad)
        assert st[0] == len(call["sets"]) and st[2] == len(tc["irregular"]), (name, st)
        if "rlc=1" in name:  # per share: the irregular sets and the regular sets holding a bad share
            assert st[1] == len([j for j in per_share if j not in tc["irregular"]]), (name, st)
            assert st[3] == sum(sizes[j] for j in per_share), (name, st)
        else:
            assert st[1] == 0 and st[3] == len(rows), (name, st)


# ---------------------------------------------------------------- cancelling errors: independent deltas
@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_cancelling_pairs_are_rejected_and_located(oc, ctxs, mode):
    call = V.cancel_call(oc)
    _bind(ctxs[mode], mode, call)
    rows, begin = V.csr(call, call["cases"])
    want = [c["intent"] for c in rows]
    assert want.count(0) == 4 and _old(ctxs[mode], call, rows) == want
    for name, got, st in _both(ctxs[mode], call, rows, begin):
        assert got == want, (name, got)
        if "rlc=1" in name:  # the two sets holding a pair are rejected, the clean one is accepted
            assert st == (3, 2, 0, begin[2]), (name, st)
    # one set alone: the pair gives 0, 0, the set's other shares 1, one rejected set
    from coconut import vss_verify_sets
    one = [c for c in rows if c["set"] == 0]
    v, st = vss_verify_sets(ctxs[mode], call["t"], call["sets"][:1], [0, len(one)], [c["id"] for c in one],
                            [(be48(c["s"]), be48(c["st"])) for c in one], rlc=True, want_stats=True)
    assert list(map(int, v)) == [1, 0, 1, 1, 0, 1, 1] and st == (1, 1, 0, 7)


# ---------------------------------------------------------------- set sizes, bad shares at set edges
@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_set_sizes_and_bad_shares_at_edges(oc, ctxs, mode):
    from coconut import vss_verify_sets_device
    call = V.sizes_call(oc)
    _bind(ctxs[mode], mode, call)
    rows, begin = V.csr(call, call["cases"])
    want = [c["intent"] for c in rows]
    assert _old(ctxs[mode], call, rows) == want
    rechecked = sum(size for size in V.SIZES if size in V.SIZES_BAD)
    for name, got, st in _both(ctxs[mode], call, rows, begin):
        assert got == want, (name, [i for i, (g, w) in enumerate(zip(got, want)) if g != w])
        if "rlc=1" in name:  # only the sets holding a bad share are rejected and rechecked
            assert st == (len(V.SIZES), len(V.SIZES_BAD), 0, rechecked), (name, st)
        else:
            assert st == (len(V.SIZES), 0, 0, len(rows)), (name, st)
    v, st = vss_verify_sets_device(ctxs[mode], *_dev(call, rows, begin), rlc=True, seed=SEED_B)  # another seed
    assert _list(v) == want and st == (len(V.SIZES), len(V.SIZES_BAD), 0, rechecked)


# ---------------------------------------------------------------- the keygen outputs in place
def _rand_coeffs(seed, count):
    import random
    rng = random.Random(seed)
    return b"".join(be48(rng.randrange(R)) for _ in range(count))


def _repack(m, q, t, total, x, y, xt, yt, comm):
    """The keygen outputs as cc_vss_verify_batch's rows, in the verdict order (keygen, polynomial, signer)."""
    sets = [[comm[(j * t + k) * 97:(j * t + k + 1) * 97] for k in range(t)] for j in range(m * (q + 1))]
    set_of, ids, shares = [], [], []
    for kg in range(m):
        for p in range(q + 1):
            for s in range(total):
                sr = kg * total + s
                o = sr if p == 0 else sr * q + p - 1
                a, b = (x, xt) if p == 0 else (y, yt)
                set_of.append(kg * (q + 1) + p)
                ids.append(s + 1)
                shares.append((a[o * 48:(o + 1) * 48], b[o * 48:(o + 1) * 48]))
    return sets, set_of, ids, shares


@pytest.mark.parametrize("shape", [(3, 3, 5, 2), (1, 33, 40, 1)], ids=str)
@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_keygen_outputs_verify_in_place(ctxs, mode, shape):
    import torch
    from coconut import (keygen_combine_batch_device, keygen_deal_batch_device, keygen_verify_shares_device,
                         vss_verify_batch)
    ctx = ctxs[mode]
    gt, g, h = KC.base_bytes(mode)
    ctx.set_keygen_params(gt, g, h, table_bits=8)
    m, t, total, q = shape
    d = torch.device("cuda", 0)
    nc = 2 * m * (q + 1) * t  # two dealers a keygen for the combine
    cf = torch.frombuffer(bytearray(_rand_coeffs(1, nc)), dtype=torch.uint8).to(d)
    ct = torch.frombuffer(bytearray(_rand_coeffs(2, nc)), dtype=torch.uint8).to(d)
    torch.cuda.synchronize()
    x, y, xt, yt, comm, _, _ = keygen_deal_batch_device(ctx, 2 * m, q, t, total, cf, ct)
    n = m * (q + 1) * total
    for rlc in (False, True):
        v, st = keygen_verify_shares_device(ctx, m, q, t, total, x, y, xt, yt, comm, rlc=rlc, seed=SEED_A)
        assert _list(v) == [1] * n and st == (m * (q + 1), 0, 0, 0 if rlc else n)
    # the combined shares of d = 2 dealers verify against the combined commitments
    cx, cy, cxt, cyt, ccomm, _, _ = keygen_combine_batch_device(ctx, m, 2, q, t, total, x, y, xt, yt, comm)
    for rlc in (False, True):
        v, st = keygen_verify_shares_device(ctx, m, q, t, total, cx, cy, cxt, cyt, ccomm, rlc=rlc, seed=SEED_B)
        assert _list(v) == [1] * n, (rlc, st)
    # one byte of one x share and of one y_j share flipped in HBM: exactly those two verdicts are 0
    kg, sx, sy, j = m - 1, 1, total - 1, q - 1
    x2, y2 = x.clone(), y.clone()
    ix, iy = (kg * total + sx) * 48 + 47, ((kg * total + sy) * q + j) * 48 + 40
    x2[ix] = x2[ix] ^ 1
    y2[iy] = y2[iy] ^ 0x80
    torch.cuda.synchronize()
    bad = {(kg * (q + 1)) * total + sx, (kg * (q + 1) + 1 + j) * total + sy}
    want = [0 if i in bad else 1 for i in range(n)]
    for rlc in (False, True):
        v, st = keygen_verify_shares_device(ctx, m, q, t, total, x2, y2, xt, yt, comm, rlc=rlc, seed=SEED_A)
        assert _list(v) == want, rlc
        assert st == (m * (q + 1), 2 if rlc else 0, 0, 2 * total if rlc else n)
    host = [bytes(a.cpu().numpy().tobytes()) for a in (x2, y2, xt, yt, comm)]
    sets, set_of, ids, shares = _repack(m, q, t, total, *host)
    assert list(map(int, vss_verify_batch(ctx, t, g, h, sets, set_of, ids, shares))) == want


# ---------------------------------------------------------------- arguments, n = 0, streams, sentinels
def test_argument_checks(oc, ctxs):
    import coconut
    import torch
    from coconut._lib import lib
    call = V.cancel_call(oc)
    ctx = ctxs["G2"]
    _bind(ctx, "G2", call)
    rows, begin = V.csr(call, call["cases"])
    n, t, ns, _, cm, ids, sh = _dev(call, rows, begin)
    v = torch.zeros(n, dtype=torch.uint8, device=cm.device)
    sb = np.asarray(begin, dtype=np.uint64)
    p = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    sbp, seed = ctypes.c_void_p(sb.ctypes.data), ctypes.c_char_p(SEED_A)
    dev = lambda *a: lib.cc_vss_verify_sets_device(*a)  # noqa: E731
    good = [ctx.h, n, t, ns, sbp, p(cm), p(ids), p(sh), 1, seed, p(v), None, None]
    assert dev(*good) == OK

    def with_(**kw):
        a = list(good)
        for k, val in kw.items():
            a[int(k[1:])] = val
        return a
    # NULLs first: the context, a buffer the call reads or writes, set_begin, the seed with rlc
    for k in (0, 4, 5, 6, 7, 9, 10):
        assert dev(*with_(**{f"a{k}": None})) == ERR_DECODE, k
    assert dev(*with_(a8=0, a9=None)) == OK  # no seed is read without rlc
    for bad_t in (0, 4097):
        assert dev(*with_(a2=bad_t)) == ERR_DECODE
    big = (1 << 26) + 1
    assert dev(*with_(a1=big)) == ERR_DECODE and dev(*with_(a3=big)) == ERR_DECODE
    for mut in ((0, 1), (ns, n - 1), (1, n + 1)):  # set_begin[0] != 0, set_begin[n_sets] != n, decreasing
        b2 = sb.copy()
        b2[mut[0]] = mut[1]
        assert dev(*with_(a4=ctypes.c_void_p(b2.ctypes.data))) == ERR_DECODE, mut
    # n_sets t above CC_MAX_BATCH with n_sets and t themselves inside their bounds
    many = np.zeros((1 << 15) + 1, dtype=np.uint64)
    assert dev(*with_(a1=0, a2=4096, a3=1 << 15, a4=ctypes.c_void_p(many.ctypes.data))) == ERR_DECODE
    # the host form: the same checks, no seed
    hv = np.zeros(n, dtype=np.uint8)
    host = [ctx.h, n, t, ns, sbp, p(cm), p(ids), p(sh), 1, ctypes.c_void_p(hv.ctypes.data), None]
    for k in (0, 4, 5, 6, 7, 9):
        a = list(host)
        a[k] = None
        assert lib.cc_vss_verify_sets(*a) == ERR_DECODE, k
    # n = 0: CC_OK with nothing read (NULL buffers), empty sets allowed; state and argument errors come first
    zero = np.zeros(4, dtype=np.uint64)
    zp = ctypes.c_void_p(zero.ctypes.data)
    assert dev(ctx.h, 0, t, 3, zp, None, None, None, 1, seed, None, None, None) == OK
    assert dev(ctx.h, 0, t, 0, zp, None, None, None, 0, None, None, None, None) == OK
    assert lib.cc_vss_verify_sets(ctx.h, 0, t, 3, zp, None, None, None, 1, None, None) == OK
    assert dev(ctx.h, 0, 0, 3, zp, None, None, None, 0, None, None, None, None) == ERR_DECODE
    # the keygen-shaped call
    kg = lambda *a: lib.cc_keygen_verify_shares_batch_device(*a)  # noqa: E731
    b = p(cm)  # any device pointer: the checks come before any read
    assert kg(ctx.h, 0, 2, 3, 5, None, None, None, None, None, 0, None, None, None, None) == OK
    assert kg(ctx.h, 1, 2, 3, 5, None, b, b, b, b, 0, None, b, None, None) == ERR_DECODE
    assert kg(ctx.h, 1, 2, 3, 5, b, b, b, b, b, 1, None, b, None, None) == ERR_DECODE
    assert kg(ctx.h, 1, 2, 0, 5, b, b, b, b, b, 0, None, b, None, None) == ERR_DECODE
    assert kg(ctx.h, 1, 2, 6, 5, b, b, b, b, b, 0, None, b, None, None) == ERR_THRESHOLD
    assert kg(ctx.h, 1, 2, 3, (1 << 16) + 1, b, b, b, b, b, 0, None, b, None, None) == ERR_DECODE
    assert kg(ctx.h, 1, 4097, 3, 5, b, b, b, b, b, 0, None, b, None, None) == ERR_DECODE
    assert kg(ctx.h, 1 << 20, 63, 3, 5, b, b, b, b, b, 0, None, b, None, None) == ERR_DECODE  # m (q + 1) total
    # no keygen params / no g, h bound: CC_ERR_STATE, after the NULL checks
    fresh = coconut.Context(0, coconut.GroupMode(0))
    try:
        assert dev(*with_(a0=fresh.h)) == ERR_STATE
        assert dev(*with_(a0=fresh.h, a4=None)) == ERR_DECODE
        fresh.set_keygen_params(KC.base_bytes("G2")[0], table_bits=8)  # Shamir only: no g, h
        assert dev(*with_(a0=fresh.h)) == ERR_STATE
        assert kg(fresh.h, 1, 2, 3, 5, b, b, b, b, b, 0, None, b, None, None) == ERR_STATE
        assert lib.cc_vss_verify_sets(*([fresh.h] + host[1:])) == ERR_STATE
    finally:
        fresh.close()


@pytest.mark.parametrize("rlc", [False, True])
def test_caller_stream_and_sentinels(oc, ctxs, rlc):
    import torch
    from coconut import vss_verify_sets_device
    from coconut._lib import lib
    call = V.sizes_call(oc)
    ctx = ctxs["G1"]
    _bind(ctx, "G1", call)
    rows, begin = V.csr(call, call["cases"])
    want = [c["intent"] for c in rows]
    args = _dev(call, rows, begin)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    stream.wait_stream(torch.cuda.current_stream())  # the uploads
    v, st = vss_verify_sets_device(ctx, *args, rlc=rlc, seed=SEED_A, stream=stream)
    stream.synchronize()
    assert v.cpu().tolist() == want
    assert st[0] == len(V.SIZES)
    # verdicts into a longer buffer: the bytes beyond n stay as they were
    n, t, ns, _, cm, ids, sh = args
    out = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=cm.device)
    torch.cuda.synchronize()
    sb = np.asarray(begin, dtype=np.uint64)
    p = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    assert lib.cc_vss_verify_sets_device(ctx.h, n, t, ns, ctypes.c_void_p(sb.ctypes.data), p(cm), p(ids), p(sh),
                                         int(rlc), ctypes.c_char_p(SEED_B), p(out), None, None) == OK
    torch.cuda.synchronize()
    got = out.cpu().tolist()
    assert got[:n] == want and got[n:] == [0xA5] * 64
