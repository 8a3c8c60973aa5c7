"""PoKOfSignatureProof::verify with one verkey per proof (cc_pok_verify_batch_pervk_device, pok_pervk.hip)
on the device, both group modes: verdicts and 576-byte GT values against the C oracle's oc_pok_verify called
per proof with that proof's own verkey, against the committed fixtures and the shared-verkey entry point,
and against verdicts known by construction (tests/pok_pervk_cases.py; tests/test_pok_pervk_model.py
checks those lists on the CPU)."""
import ctypes

import numpy as np
import pytest

import pok_pervk_cases as C
from conftest import golden, host_threads

pytestmark = pytest.mark.gpu

MODES = {"G2": 0, "G1": 1}
WIDE_MAX, FEXP_WIDE_MAX = 4096, 2048  # slots.h kWideMax, kFexpWideMax
OK, ERR_LEN, ERR_BASES, DECODE, STATE = 0, -1, -2, -4, -7
ARGS = ("s1", "s2", "J", "T", "resp", "chal")


@pytest.fixture(scope="module")
def ctxs():
    import coconut
    c = {m: coconut.Context(0, coconut.GroupMode(v)) for m, v in MODES.items()}
    yield c
    for x in c.values():
        x.close()


def _cat(hexes):
    return b"".join(bytes.fromhex(h) for h in hexes)


def _to(x):
    import torch
    return torch.frombuffer(bytearray(x) if len(x) else bytearray(1), dtype=torch.uint8).to(torch.device("cuda", 0))


def _P(x):
    return ctypes.c_void_p(x.data_ptr())


def _upload(b):
    return {k: _to(b[k]) for k in ARGS + ("rev", "X", "Y")}


def _ridx(b):
    return (ctypes.c_uint64 * max(len(b["revealed"]), 1))(*b["revealed"])


def _call(ctx, b, D, v, gt, stream=None, n=None, vk=None):
    from coconut import _lib
    X, Y = vk or (D["X"], D["Y"])
    return _lib.lib.cc_pok_verify_batch_pervk_device(
        ctx.h, b["n"] if n is None else n, b["q"], len(b["revealed"]), b["nresp"], *[_P(D[k]) for k in ARGS], _ridx(b),
        _P(D["rev"]), _P(X), _P(Y), _P(v), _P(gt) if gt is not None else None,
        ctypes.c_void_p(stream.cuda_stream) if stream is not None else None)


def _run(ctx, b, n=None, D=None, vk=None):
    """(verdicts, GT bytes) of the first n proofs of b through the device entry point."""
    import torch
    n = b["n"] if n is None else n
    D = D or _upload(b)
    dev = torch.device("cuda", 0)
    v = torch.zeros(n, dtype=torch.uint8, device=dev)
    gt = torch.zeros(n * 576, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    assert _call(ctx, b, D, v, gt, n=n, vk=vk) == OK
    torch.cuda.synchronize()
    return [int(x) for x in v.cpu().numpy()], bytes(gt.cpu().numpy())


def _same(b, v, gt, want, idx=None, tag=""):
    """verdicts and GT of proofs idx (default: all, in order) equal the oracle's [(verdict, GT or None)]"""
    idx = range(len(want)) if idx is None else idx
    for k, i in enumerate(idx):
        assert v[k] == want[k][0], (tag, i, b["names"][i])
        if want[k][1] is not None:
            assert gt[576 * k:576 * (k + 1)] == want[k][1], (tag, i, b["names"][i])


_DISTINCT = {}


def _distinct(ctx, oc, mode, shape, n=C.SIZES[-1]):
    """One list of n proofs under distinct verkeys per (mode, shape), with the oracle's results; shared."""
    key = (mode, shape, n)
    if key not in _DISTINCT:
        q, rev = shape
        b = C.distinct_batch(C.gpu_mul(ctx), MODES[mode], n, q, rev, seed=7000 + 100 * q + 10 * len(rev) + MODES[mode],
                             gk=C.shared_gk(MODES[mode]))
        _DISTINCT[key] = (b, C.oracle_pok(oc, b, threads=host_threads()))
    return _DISTINCT[key]


@pytest.mark.parametrize("name", ["pok_g2_q6.json", "pok_g1_q6.json", "pok_g2_q32.json", "pok_g1_q32.json"])
def test_golden_fixture_with_its_verkey_repeated(ctxs, name):
    """The shared-verkey fixtures with the verkey repeated per proof: verdicts and GT equal the fixture's
    and, byte for byte, cc_pok_verify_batch_device's on the same proofs; every corruption kind."""
    import torch
    from coconut import _lib
    d = golden(name)
    ctx = ctxs[d["mode"]]
    ctx.set_params(bytes.fromhex(d["g_tilde"]))
    pr = d["proofs"]
    n, q = len(pr), d["q"]
    assert len({p["kind"] for p in pr}) > 2 and {p["verdict"] for p in pr} == {0, 1}
    X, Y = bytes.fromhex(d["vk"]["X"]), _cat(d["vk"]["Y"])
    b = dict(mode=MODES[d["mode"]], n=n, q=q, revealed=d["revealed"], nresp=len(pr[0]["responses"]),
             s1=_cat(p["sigma1"] for p in pr), s2=_cat(p["sigma2"] for p in pr), J=_cat(p["J"] for p in pr),
             T=_cat(p["T"] for p in pr), resp=_cat(x for p in pr for x in p["responses"]),
             chal=_cat(p["chal"] for p in pr), rev=_cat(m for p in pr for m in p["revealed_msgs"]), X=X * n, Y=Y * n,
             names=[p["kind"] for p in pr])
    D = _upload(b)
    v, gt = _run(ctx, b, D=D)
    for i, p in enumerate(pr):
        assert v[i] == p["verdict"], (i, p["kind"])
        if p["gt"] is not None:
            assert gt[576 * i:576 * (i + 1)].hex() == p["gt"], (i, p["kind"])
    ctx.set_verkey(X, [bytes.fromhex(y) for y in d["vk"]["Y"]])
    dev = torch.device("cuda", 0)
    v2 = torch.zeros(n, dtype=torch.uint8, device=dev)
    g2 = torch.zeros(n * 576, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    assert _lib.lib.cc_pok_verify_batch_device(ctx.h, n, q, len(d["revealed"]), b["nresp"], *[_P(D[k]) for k in ARGS],
                                               _ridx(b), _P(D["rev"]), _P(v2), _P(g2), None) == OK
    torch.cuda.synchronize()
    assert v == [int(x) for x in v2.cpu().numpy()]
    assert gt == bytes(g2.cpu().numpy())


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_distinct_verkeys(ctxs, oc, mode, shape):
    """Each proof valid under its own key, every fourth corrupted (a response, a revealed message, made
    under the next proof's key), at 257, 65 and single proofs: a partial wave, a wave boundary and a block
    boundary of the lane and the lane-pair kernels."""
    ctx = ctxs[mode]
    b, want = _distinct(ctx, oc, mode, shape)
    assert [w[0] for w in want] == b["expect"] and set(b["expect"]) == {0, 1}
    ctx.set_params(b["g"])
    D = _upload(b)
    for n in sorted(C.SIZES, reverse=True)[:-1]:
        v, gt = _run(ctx, b, n=n, D=D)
        _same(b, v, gt, want[:n], tag=(mode, shape, n))
    for i in (0, 3):  # a valid proof and a corrupted one, alone
        one = C.take(b, [i])
        v, gt = _run(ctx, one)
        _same(b, v, gt, [want[i]], idx=[i], tag=(mode, shape, "single"))


@pytest.mark.parametrize("shape", [C.SHAPES[3], C.SHAPES[0]], ids=["q6r2", "q1r0"])
@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_rotated_keys_are_rejected(ctxs, oc, mode, shape):
    """The valid proofs with the verkey rows rotated by one: every proof rejected, so the kernel reads
    proof i's key; the whole list rotated accepts exactly the proofs made under the next proof's key."""
    ctx = ctxs[mode]
    b, _ = _distinct(ctx, oc, mode, shape)
    ctx.set_params(b["g"])
    valid = C.take(b, [i for i, e in enumerate(b["expect"]) if e])
    v, _ = _run(ctx, C.rotate_keys(valid))
    assert v == [0] * valid["n"] and valid["n"] > 100
    v, _ = _run(ctx, C.rotate_keys(b))
    assert v == [int(nm == "next_key") for nm in b["names"]]


@pytest.mark.parametrize("name", sorted(C.EDGE_LISTS))
@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_edge_scalars_and_bases(ctxs, oc, mode, name):
    """Edge scalars (0, 1, r - 1, r, r + 1, 2^384 - 1, the recoding edges) as responses, challenge and
    revealed messages; identity, off-curve and >= p encodings; equal, opposite and steered bases; J and T
    degenerate; X~ = -J; small-order points as X~, Y~_j and J: verdicts and GT equal the oracle's."""
    ctx = ctxs[mode]
    b = C.edge_batch(oc, C.EDGE_LISTS[name](MODES[mode]))
    want = C.oracle_pok(oc, b, threads=host_threads())
    assert [w[0] for w in want] == b["expect"] and set(b["expect"]) == {0, 1}
    ctx.set_params(b["g"])
    v, gt = _run(ctx, b)
    _same(b, v, gt, want, tag=(mode, name))


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_miller_and_fexp_regimes_agree(ctxs, oc, mode):
    """WIDE_MAX + 6 proofs (the batch Miller loop and final exponentiation) by construction and, the first
    7, against the oracle; sub-batches in the one-wave regimes (7, FEXP_WIDE_MAX, FEXP_WIDE_MAX + 1 proofs)
    give the same bytes."""
    ctx = ctxs[mode]
    N = WIDE_MAX + 6
    b = C.distinct_batch(C.gpu_mul(ctx), MODES[mode], N, 6, (1, 4), seed=4242 + MODES[mode])
    ctx.set_params(b["g"])
    D = _upload(b)
    v, gt = _run(ctx, b, D=D)
    assert v == b["expect"]
    _same(b, v, gt, C.oracle_pok(oc, b, idx=range(7), threads=host_threads()), idx=range(7), tag=mode)
    for n in (7, FEXP_WIDE_MAX, FEXP_WIDE_MAX + 1):
        vn, gn = _run(ctx, b, n=n, D=D)
        assert vn == v[:n], (mode, n)
        assert gn == gt[:576 * n], (mode, n)


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_concurrent_slots(ctxs, oc, mode):
    """cc_set_concurrency(2): four calls on two streams, each with its own verkey buffer and revealed set
    (one with a larger r), no synchronisation in between; results equal the one-slot runs'."""
    import torch
    ctx = ctxs[mode]
    shapes = [C.SHAPES[2], C.SHAPES[3], C.SHAPES[6], C.SHAPES[4]]  # r = 0, 2, 2 (unsorted), 6
    bs = [_distinct(ctx, oc, mode, s)[0] for s in shapes]
    assert len({b["g"] for b in bs}) == 1  # a context holds one g~
    ctx.set_params(bs[0]["g"])
    Ds = [_upload(b) for b in bs]
    ref = [_run(ctx, b, D=D) for b, D in zip(bs, Ds)]
    assert [r[0] for r in ref] == [b["expect"] for b in bs]
    dev = torch.device("cuda", 0)
    ctx.set_concurrency(2)
    try:
        streams = [torch.cuda.Stream(dev) for _ in range(2)]
        outs = [(torch.zeros(b["n"], dtype=torch.uint8, device=dev),
                 torch.zeros(b["n"] * 576, dtype=torch.uint8, device=dev)) for b in bs]
        torch.cuda.synchronize()
        for k, (b, D) in enumerate(zip(bs, Ds)):
            assert _call(ctx, b, D, outs[k][0], outs[k][1], stream=streams[k % 2]) == OK
        torch.cuda.synchronize()
        for k, (v, gt) in enumerate(outs):
            assert [int(x) for x in v.cpu().numpy()] == ref[k][0], (mode, k)
            assert bytes(gt.cpu().numpy()) == ref[k][1], (mode, k)
    finally:
        ctx.set_concurrency(1)


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_aggregated_verkeys_stay_in_device_memory(ctxs, oc, mode):
    """set_issuers -> cc_verkey_aggregate_ids_device -> cc_pok_verify_batch_pervk_device, t = 3 of 5
    issuers, q = 6: every credential's verkey is aggregated from its own subset into HBM and the showings
    (made under the master key, every fourth corrupted) are checked against those buffers."""
    import torch
    from coconut import _lib
    m = MODES[mode]
    ctx = ctxs[mode]
    og, _ = C.groups(m)
    ob = 97 if og == 1 else 192
    n, t, q, n_iss = 33, 3, 6, 5
    sk = C.shamir_keys(m, n_iss, t, q, seed=606 + m)
    mul = C.gpu_mul(ctx)
    iss = mul(og, [sk["gk"] * v for row in sk["shares"] for v in row])
    iX = b"".join(iss[(k * (q + 1)) * ob:(k * (q + 1) + 1) * ob] for k in range(n_iss))
    iY = b"".join(iss[(k * (q + 1) + 1) * ob:(k + 1) * (q + 1) * ob] for k in range(n_iss))
    b = C.distinct_batch(mul, m, n, q, (1, 4), seed=707 + m, keys=[sk["master"]] * n, gk=sk["gk"])
    assert set(b["expect"]) == {0, 1}
    ctx.set_params(b["g"])
    ctx.set_issuers(sk["ids"], iX, iY, q)
    rng = np.random.default_rng(5 + m)
    ids = np.stack([rng.choice(np.asarray(sk["ids"], dtype=np.uint64), size=t, replace=False) for _ in range(n)])
    assert len({tuple(sorted(r)) for r in ids.tolist()}) > 3
    dev = torch.device("cuda", 0)
    d_ids = torch.from_numpy(ids.astype(np.int64)).to(dev)
    d_X = torch.zeros(n * ob, dtype=torch.uint8, device=dev)
    d_Y = torch.zeros(n * q * ob, dtype=torch.uint8, device=dev)
    D = _upload(b)
    v = torch.zeros(n, dtype=torch.uint8, device=dev)
    gt = torch.zeros(n * 576, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    assert _lib.lib.cc_verkey_aggregate_ids_device(ctx.h, n, t, t, _P(d_ids), _P(d_X), _P(d_Y), None) == OK
    assert _call(ctx, b, D, v, gt, vk=(d_X, d_Y)) == OK
    torch.cuda.synchronize()
    assert bytes(d_X.cpu().numpy()) == b["X"] and bytes(d_Y.cpu().numpy()) == b["Y"]  # the master key, n times
    v, gt = [int(x) for x in v.cpu().numpy()], bytes(gt.cpu().numpy())
    assert v == b["expect"]
    _same(b, v, gt, C.oracle_pok(oc, b, threads=host_threads()), tag=mode)


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_abi_errors_in_order_and_host_form(oc, mode):
    """Every argument error in the header's order on a context that has params and NO verkey; n = 0 with
    NULL buffers; n > CC_MAX_BATCH; the host form and the Python vk= path against the device form."""
    import coconut
    import torch
    from coconut import _lib, pok_verify_batch
    lib = _lib.lib
    m = MODES[mode]
    ctx = coconut.Context(0, coconut.GroupMode(m))
    try:
        b = C.distinct_batch(C.oracle_mul(oc, host_threads()), m, 9, 6, (5, 2), seed=31 + m)
        D = _upload(b)
        dev = torch.device("cuda", 0)
        v = torch.zeros(b["n"], dtype=torch.uint8, device=dev)
        N = None
        good = [_P(D[k]) for k in ARGS] + [_ridx(b), _P(D["rev"]), _P(D["X"]), _P(D["Y"]), _P(v), N, N]

        def dev_call(n=9, q=6, r=2, nresp=5, h=ctx.h, **nulls):
            a = list(good)
            for k in nulls:
                a[{"s1": 0, "T": 3, "resp": 4, "idx": 6, "rev": 7, "X": 8, "Y": 9, "v": 10}[k]] = N
            return lib.cc_pok_verify_batch_pervk_device(h, n, q, r, nresp, *a)

        idx = lambda *xs: (ctypes.c_uint64 * len(xs))(*xs)  # noqa: E731
        assert dev_call(h=N) == DECODE
        for k in ("s1", "T", "resp", "idx", "rev", "X", "Y", "v"):
            assert dev_call(**{k: True}) == DECODE, k
        assert dev_call() == STATE  # no params yet
        assert dev_call(q=5000) == STATE  # the state comes before the ceiling
        ctx.set_params(b["g"])
        assert dev_call(q=4097, nresp=4096) == DECODE
        good[6] = idx(6, 2)
        assert dev_call(q=4097) == DECODE  # the ceiling before the index rules
        assert dev_call(nresp=9) == ERR_LEN  # an index >= q before the response count
        good[6] = idx(2, 2)
        assert dev_call(nresp=9) == DECODE  # a repeated index
        good[6] = _ridx(b)
        assert dev_call(nresp=6, n=(1 << 26) + 1) == ERR_BASES  # the response count before CC_MAX_BATCH
        assert dev_call(n=(1 << 26) + 1) == DECODE
        # n = 0: checked, then a no-op with NULL buffers
        assert lib.cc_pok_verify_batch_pervk_device(ctx.h, 0, 6, 0, 7, N, N, N, N, N, N, N, N, N, N, N, N, N) == OK
        assert lib.cc_pok_verify_batch_pervk(ctx.h, 0, 6, 0, 7, N, N, N, N, N, N, N, N, N, N, N, N) == OK
        assert lib.cc_pok_verify_batch_pervk_device(ctx.h, 0, 6, 0, 6, N, N, N, N, N, N, N, N, N, N, N, N, N) == ERR_BASES
        assert lib.cc_pok_verify_batch_pervk(ctx.h, 0, 6, 0, 6, N, N, N, N, N, N, N, N, N, N, N, N) == ERR_BASES
        # the call itself, without any cc_set_verkey: the device form, the host form through Python
        want = C.oracle_pok(oc, b, threads=host_threads())
        vd, gd = _run(ctx, b, D=D)
        _same(b, vd, gd, want, tag=mode)
        assert vd == b["expect"]
        vh, gh = pok_verify_batch(ctx, b["n"], b["q"], b["revealed"], b["nresp"], b["s1"], b["s2"], b["J"], b["T"],
                                  b["resp"], b["chal"], b["rev"], want_gt=True, vk=(b["X"], b["Y"]))
        assert [int(x) for x in vh] == vd and gh == gd
        vh = pok_verify_batch(ctx, b["n"], b["q"], b["revealed"], b["nresp"], b["s1"], b["s2"], b["J"], b["T"],
                              b["resp"], b["chal"], b["rev"], vk=(b["X"], b["Y"]))
        assert [int(x) for x in vh] == vd
        with pytest.raises(coconut.CoconutError):  # the shared-verkey form still needs its verkey
            pok_verify_batch(ctx, b["n"], b["q"], b["revealed"], b["nresp"], b["s1"], b["s2"], b["J"], b["T"],
                             b["resp"], b["chal"], b["rev"])
    finally:
        ctx.close()
