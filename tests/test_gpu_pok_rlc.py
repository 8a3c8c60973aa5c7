"""GPU tests of the RLC batch mode for PoKOfSignatureProof::verify (csrc/pok_rlc.hip,
cc_pok_rlc_partial_device + cc_rlc_finish_device, cc_pok_verify_batch_rlc).  Reference semantics are per
proof (ps_sig PoKOfSignatureProof::verify): the batch check may only accept a batch whose every proof
verifies, and on reject the fall-back verdicts must equal the per-proof path's."""
import ctypes

import numpy as np
import pytest

from conftest import golden
from test_gpu_parity import MODES, _cat
from test_pok_rlc_model import BASE_INDEX, SEED, expected_gt, sub_batch

pytestmark = pytest.mark.gpu

FIXTURES = ["pok_g2_q6.json", "pok_g1_q6.json", "pok_g2_q32.json", "pok_g1_q32.json"]
PARTIAL_FLAG = 144
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


@pytest.fixture(scope="module")
def ctxs():
    import coconut
    c = {m: coconut.Context(0, coconut.GroupMode(v)) for m, v in MODES.items()}
    yield c
    for x in c.values():
        x.close()


def _load(ctx, d):
    ctx.set_params(bytes.fromhex(d["g_tilde"]))
    ctx.set_verkey(bytes.fromhex(d["vk"]["X"]), [bytes.fromhex(y) for y in d["vk"]["Y"]])


def _fix_batch(d, pr):
    """Fixture proofs as one batch dict in make_pok_batch's layout."""
    return dict(mode=MODES[d["mode"]], n=len(pr), q=d["q"], revealed=list(d["revealed"]),
                nresp=len(pr[0]["responses"]), s1=_cat(p["sigma1"] for p in pr), s2=_cat(p["sigma2"] for p in pr),
                J=_cat(p["J"] for p in pr), T=_cat(p["T"] for p in pr),
                resp=_cat(x for p in pr for x in p["responses"]), chal=_cat(p["chal"] for p in pr),
                rev=_cat(m for p in pr for m in p["revealed_msgs"]))


KEYS = ("s1", "s2", "J", "T", "resp", "chal", "rev")


def _host(ctx, b, rlc, **over):
    from coconut import pok_verify_batch
    a = {k: over.get(k, b[k]) for k in KEYS}
    return pok_verify_batch(ctx, b["n"], b["q"], b["revealed"], b["nresp"], a["s1"], a["s2"], a["J"], a["T"], a["resp"],
                            a["chal"], a["rev"], rlc=rlc)


def _to_dev(b, **over):
    import torch
    dev = torch.device("cuda", 0)
    # one spare byte so an empty array (r = 0) still has a device pointer
    return {k: torch.frombuffer(bytearray(over.get(k, b[k]) + b"\0"), dtype=torch.uint8).to(dev) for k in KEYS}


def _engine(ctx, b, D, lo=0, hi=None, base_index=None, seed=None):
    """A PokDeviceEngine over proofs [lo, hi) of the device batch D."""
    from coconut.dist import PokDeviceEngine
    hi = b["n"] if hi is None else hi
    sb, ob = (192, 97) if b["mode"] == 0 else (97, 192)
    r, nresp = len(b["revealed"]), b["nresp"]
    w = dict(s1=sb, s2=sb, J=ob, T=ob, resp=nresp * 48, chal=48, rev=r * 48)
    s = {k: D[k][lo * w[k]:] for k in KEYS}
    return PokDeviceEngine(ctx, hi - lo, b["q"], b["revealed"], s["s1"], s["s2"], s["J"], s["T"], s["resp"], s["chal"],
                           s["rev"], base_index=lo if base_index is None else base_index, seed=seed)


def _decide(ctx, b, D=None, shards=None, seed=None, base_index=None, want_gt=False):
    """partial(s) + one finish -> (accept, OR of the partials' fall-back words, GT bytes or None)."""
    import torch
    from coconut._lib import lib
    D = D or _to_dev(b)
    shards = shards or [(0, b["n"])]
    parts = []
    for lo, hi in shards:
        e = _engine(ctx, b, D, lo, hi, base_index=base_index, seed=seed)
        parts.append(e.partial().clone())
    torch.cuda.synchronize()
    allp = torch.stack(parts).contiguous()
    flag = int(allp[:, PARTIAL_FLAG].cpu().numpy().any())
    acc = torch.zeros(1, dtype=torch.uint8, device=allp.device)
    gt = torch.zeros(576, dtype=torch.uint8, device=allp.device)
    st = lib.cc_rlc_finish_device(ctx.h, len(parts), ctypes.c_void_p(allp.data_ptr()), ctypes.c_void_p(acc.data_ptr()),
                                  ctypes.c_void_p(gt.data_ptr()) if want_gt else None, None)
    assert st == 0
    torch.cuda.synchronize()
    return bool(acc.item()), flag, (gt.cpu().numpy().tobytes() if want_gt else None)


# ---------------------------------------------------------------- golden fixtures
@pytest.mark.parametrize("name", FIXTURES)
def test_golden_parity(ctxs, name):
    """All 8 fixture proofs (valid + every corruption kind) through rlc=True equal the fixture verdicts;
    the 3 valid proofs alone are accepted by partial + finish."""
    d = golden(name)
    ctx = ctxs[d["mode"]]
    _load(ctx, d)
    pr = d["proofs"]
    assert list(_host(ctx, _fix_batch(d, pr), True)) == [p["verdict"] for p in pr]
    good = _fix_batch(d, [p for p in pr if p["kind"] == "valid"])
    assert good["n"] == 3
    accept, flag, _ = _decide(ctx, good)
    assert accept and flag == 0
    assert _host(ctx, good, True).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_delta_weighting_byte_exact(ctxs, name):
    """[valid, valid, bad_revealed, valid] under a fixed seed at base_index 5: every Schnorr relation
    holds, so the fall-back word stays clear and the finish's GT is the bad proof's fixture GT raised to
    its delta (global index 7, from the CPU key stream): pins the key-stream index, the delta J'
    scaling and the fold against the CPU (tests/test_pok_rlc_model.py evaluates the same product)."""
    d = golden(name)
    ctx = ctxs[d["mode"]]
    _load(ctx, d)
    b = _fix_batch(d, sub_batch(d))
    accept, flag, gt = _decide(ctx, b, seed=SEED, base_index=BASE_INDEX, want_gt=True)
    assert flag == 0
    assert not accept
    assert gt == expected_gt(d)


@pytest.mark.parametrize("kind", ["bad_chal", "bad_response", "bad_J", "sigma1_inf", "bad_revealed"])
@pytest.mark.parametrize("name", ["pok_g2_q6.json", "pok_g1_q6.json"])
def test_each_failure_kind_alone_is_rejected(ctxs, name, kind):
    d = golden(name)
    ctx = ctxs[d["mode"]]
    _load(ctx, d)
    valid = [p for p in d["proofs"] if p["kind"] == "valid"]
    bad = next(p for p in d["proofs"] if p["kind"] == kind)
    b = _fix_batch(d, [valid[0], valid[1], bad, valid[2]])
    accept, flag, _ = _decide(ctx, b)
    assert not accept
    assert flag == (0 if kind == "bad_revealed" else 1)  # only the pairing equation fails without a flag
    assert list(_host(ctx, b, True)) == [1, 1, 0, 1]


# ---------------------------------------------------------------- synthetic batches
def _synthetic(ctx, mode, n, q=6, revealed=(1, 4), seed=5):
    import bench_modes
    b = bench_modes.make_pok_batch(ctx, MODES[mode], n, q=q, revealed=list(revealed), seed=seed, bad_every=0)
    ctx.set_params(b["g_tilde"])
    ctx.set_verkey(b["X"], b["Y"])
    return b


def _swap_in(b, key, dst, src):
    w = len(b[key]) // b["n"]
    x = bytearray(b[key])
    x[dst * w:(dst + 1) * w] = b[key][src * w:(src + 1) * w]
    return bytes(x)


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_ragged_shards_and_quad_positions(ctxs, mode):
    """Shards of 1, 2, 3, 5, 6 and 7 proofs plus an empty one into one finish (partial last quads of the
    four-proof Miller loop): all valid is accepted; another Schnorr-valid proof's sigma'_2 at quad
    positions 0, 1, 2 and 3 of a partial last quad is rejected, and the host form falls back exactly."""
    sizes = (1, 2, 3, 5, 6, 7)
    n = sum(sizes)
    offs = np.cumsum((0,) + sizes)
    ctx = ctxs[mode]
    b = _synthetic(ctx, mode, n, seed=31)
    shards = [(int(offs[k]), int(offs[k + 1])) for k in range(len(sizes))] + [(n, n)]
    accept, flag, _ = _decide(ctx, b, shards=shards)
    assert accept and flag == 0
    for shard, local in ((3, 4), (2, 1), (4, 2), (4, 3), (5, 6)):  # (index into sizes, shard-local index)
        bad = int(offs[shard]) + local
        s2 = _swap_in(b, "s2", bad, (bad + 1) % n)
        accept, flag, _ = _decide(ctx, b, D=_to_dev(b, s2=s2), shards=shards)
        assert not accept and flag == 0, (shard, local)
        expect = np.ones(n, np.uint8)
        expect[bad] = 0
        assert np.array_equal(_host(ctx, b, True, s2=s2), expect), bad


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_block_edge_of_the_prep(ctxs, mode):
    """n = 127, 128, 129: the 128-proofs-a-block edge of the SigG2 PoK prep (and the 128 lane pairs a
    block of the SigG1 one).  All valid is accepted; the last proof with another's sigma'_2, or with
    another's challenge (its Schnorr relation then fails), is rejected with exact fall-back verdicts."""
    ctx = ctxs[mode]
    b = _synthetic(ctx, mode, 129, seed=37)
    sb, ob = (192, 97) if MODES[mode] == 0 else (97, 192)
    w = dict(s1=sb, s2=sb, J=ob, T=ob, resp=b["nresp"] * 48, chal=48, rev=len(b["revealed"]) * 48)
    for n in (127, 128, 129):
        c = dict(b, n=n, **{k: b[k][:n * w[k]] for k in KEYS})
        accept, flag, _ = _decide(ctx, c)
        assert accept and flag == 0, n
        expect = np.ones(n, np.uint8)
        expect[n - 1] = 0
        s2 = _swap_in(c, "s2", n - 1, 0)
        accept, flag, _ = _decide(ctx, c, D=_to_dev(c, s2=s2))
        assert not accept and flag == 0, n
        assert np.array_equal(_host(ctx, c, True, s2=s2), expect), n
        chal = _swap_in(c, "chal", n - 1, 0)
        accept, flag, _ = _decide(ctx, c, D=_to_dev(c, chal=chal))
        assert not accept and flag == 1, n
        assert np.array_equal(_host(ctx, c, True, chal=chal), expect), n


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_batch_past_the_two_proof_loop(ctxs, mode):
    """The partial runs two proofs per Miller loop while those waves fit one a SIMD (65,536 proofs on
    an MI355X) and four per loop beyond: 65,667 proofs (a partial last quad)
    take the four-proof loop over the PoK prep's twin layout.  All valid is accepted, one proof with
    its neighbour's sigma'_2 rejected."""
    n = 65664 + 3
    ctx = ctxs[mode]
    b = _synthetic(ctx, mode, n, seed=61)
    accept, flag, _ = _decide(ctx, b)
    assert accept and flag == 0
    accept, flag, _ = _decide(ctx, b, D=_to_dev(b, s2=_swap_in(b, "s2", n - 2, n - 1)))
    assert not accept and flag == 0


def _own_batch(ctx, mode, n, q, revealed, seed, chal_of=None, r2_of=None):
    """make_pok_batch's construction with the challenge and r2 under the test's control."""
    import bench_modes
    import coconut
    from bench_modes import _be, _fr
    rng = np.random.default_rng(seed)
    m_ = MODES[mode]
    og, sg = (1, 2) if m_ == 0 else (2, 1)
    gen = {1: coconut.G1_GENERATOR, 2: coconut.G2_GENERATOR}
    x, y, gk = _fr(rng), [_fr(rng) for _ in range(q)], _fr(rng) or 1
    ob = 97 if og == 1 else 192
    vk = coconut.fixed_base_mul(ctx, og, gen[og], b"".join(_be(v * gk) for v in [x] + y + [1]))
    X, Y, g_tilde = vk[:ob], vk[ob:ob * (q + 1)], vk[ob * (q + 1):]
    hidden = [i for i in range(q) if i not in revealed]
    s1s, s2s, js, ts, resp, chal, rev = [], [], [], [], [], [], []
    for p in range(n):
        m = [_fr(rng) for _ in range(q)]
        k, r1, r2, c = _fr(rng) or 1, _fr(rng) or 1, _fr(rng), _fr(rng)
        if chal_of:
            c = chal_of(c)
        if r2_of:
            r2 = r2_of(p, r2)
        s = (x + sum(y[i] * m[i] for i in range(q))) % R
        s1s.append(_be(k * r1))
        s2s.append(_be(r1 * k * (s + r2)))
        secrets = [r2] + [m[i] for i in hidden]
        ylog = [1] + [y[i] for i in hidden]
        bl = [_fr(rng) for _ in secrets]
        js.append(_be(gk * sum(a * b for a, b in zip(ylog, secrets))))
        ts.append(_be(gk * sum(a * b for a, b in zip(ylog, bl))))
        resp.append(b"".join(_be((b - c * sc) % R) for b, sc in zip(bl, secrets)))
        chal.append(_be(c))
        rev.append(b"".join(_be(m[i]) for i in revealed))
    mul = lambda g, ks: coconut.fixed_base_mul(ctx, g, gen[g], b"".join(ks))  # noqa: E731
    assert bench_modes.R == R
    b = dict(mode=m_, n=n, q=q, revealed=list(revealed), nresp=len(hidden) + 1, s1=mul(sg, s1s), s2=mul(sg, s2s),
             J=mul(og, js), T=mul(og, ts), resp=b"".join(resp), chal=b"".join(chal), rev=b"".join(rev))
    ctx.set_params(g_tilde)
    ctx.set_verkey(X, Y)
    return b


@pytest.mark.parametrize("mode", ["G2", "G1"])
@pytest.mark.parametrize("case", ["r0", "rq", "rq_J_identity"])
def test_revealed_set_edges(ctxs, mode, case):
    """q = 6 with nothing revealed, everything revealed (one response), and everything revealed with
    r2 = 0 in proof 1, whose J is then the identity encoding: a valid proof, accepted.  One proof with
    another's sigma'_2 is rejected and the verdicts equal the per-proof path's."""
    from oracle import bls12_381 as B
    ctx = ctxs[mode]
    q, n = 6, 5
    revealed = () if case == "r0" else tuple(range(q))
    b = _own_batch(ctx, mode, n, q, revealed, seed=41,
                   r2_of=(lambda p, r2: 0 if p == 1 else r2) if case == "rq_J_identity" else None)
    assert b["nresp"] == q - len(revealed) + 1
    if case == "rq_J_identity":
        ident = B.g1_to_bytes(None) if MODES[mode] == 0 else B.g2_to_bytes(None)
        ob = len(ident)
        assert b["J"][ob:2 * ob] == ident
    assert _host(ctx, b, False).all()
    accept, flag, _ = _decide(ctx, b)
    assert accept and flag == 0
    assert _host(ctx, b, True).all()
    s2 = _swap_in(b, "s2", 1, 3)
    per_proof = _host(ctx, b, False, s2=s2)
    assert list(per_proof) == [1, 0, 1, 1, 1]
    accept, _, _ = _decide(ctx, b, D=_to_dev(b, s2=s2))
    assert not accept
    assert np.array_equal(_host(ctx, b, True, s2=s2), per_proof)


def test_J_outside_the_subgroup_sigg2(ctxs):
    """SigG2: J + (0, 2), the point of order 3, under a challenge that is a multiple of 3: the Schnorr
    relation still holds (chal (0, 2) = O) and the pairing is cofactor-blind on its G1 side, so the
    per-proof verdict stays 1, but the linear-combination argument does not cover such a J: the partial
    raises the fall-back word, the finish rejects and the host form returns the per-proof verdicts."""
    from oracle import bls12_381 as B
    ctx = ctxs["G2"]
    b = _own_batch(ctx, "G2", 4, 6, (1, 4), seed=43, chal_of=lambda c: c - c % 3)
    accept, flag, _ = _decide(ctx, b)
    assert accept and flag == 0
    t3 = (0, 2)
    assert B.G1.on_curve(t3) and B.G1.mul_any(t3, 3) is None
    J2 = B.g1_to_bytes(B.G1.add(B.g1_from_bytes(b["J"][2 * 97:3 * 97]), t3))
    J = b["J"][:2 * 97] + J2 + b["J"][3 * 97:]
    per_proof = _host(ctx, b, False, J=J)
    assert per_proof.all()
    accept, flag, _ = _decide(ctx, b, D=_to_dev(b, J=J))
    assert flag == 1 and not accept
    assert np.array_equal(_host(ctx, b, True, J=J), per_proof)


def test_J_outside_the_subgroup_sigg1(ctxs):
    """SigG1: a G2 point on the curve but outside the subgroup (status 1 of the subgroup fixture) as J:
    the fall-back word is raised and the verdicts equal the per-proof path's."""
    ctx = ctxs["G1"]
    b = _own_batch(ctx, "G1", 4, 6, (1, 4), seed=47)
    pt = next(bytes.fromhex(e["point"]) for e in golden("subgroup.json")["G2"] if int(e["status"]) == 1)
    J = b["J"][:192] + pt + b["J"][2 * 192:]
    per_proof = _host(ctx, b, False, J=J)
    accept, flag, _ = _decide(ctx, b, D=_to_dev(b, J=J))
    assert flag == 1 and not accept
    assert np.array_equal(_host(ctx, b, True, J=J), per_proof)


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_partials_on_concurrency_slots(ctxs, mode):
    """cc_set_concurrency(2): successive PoK partials take alternating slots (each its own prep, flags,
    tables of d J and revealed indices) with the finishes pipelined behind them, as
    test_gpu_rlc.test_partials_on_concurrency_slots does for signatures.  Good and bad engines with
    differing revealed sets, a larger one partway through, keep their own decisions, and the context
    returns to one slot afterwards."""
    from coconut.dist import gather_partials
    n, q = 2048, 6
    ctx = ctxs[mode]
    small = _synthetic(ctx, mode, n, q=q, revealed=(1, 4), seed=53)
    large = _synthetic(ctx, mode, n, q=q, revealed=(0, 2, 3, 5), seed=53)  # same seed: the same verkey
    assert small["X"] == large["X"] and small["Y"] == large["Y"] and small["g_tilde"] == large["g_tilde"]
    engs = {}
    for name, b in (("small", small), ("large", large)):
        engs[(name, True)] = _engine(ctx, b, _to_dev(b))
        engs[(name, False)] = _engine(ctx, b, _to_dev(b, s2=_swap_in(b, "s2", 9, 10)))
    plan = [("small", True), ("small", False), ("small", True), ("large", True), ("large", False), ("small", False),
            ("large", True), ("small", True)]
    order = [engs[k] for k in plan]
    ctx.set_concurrency(2)
    try:
        assert ctx.concurrency() == 2
        decisions = []
        part = order[0].partial()
        for s, eng in enumerate(order):
            allp, k = gather_partials(part)
            d = eng.finish_async(allp, k)
            if s + 1 < len(order):
                part = order[s + 1].partial()
            decisions.append(d())
        assert decisions == [g for _, g in plan]
    finally:
        ctx.set_concurrency(1)
    assert ctx.concurrency() == 1
    one = engs[("large", False)]
    allp, k = gather_partials(one.partial())
    assert one.finish_async(allp, k)() is False
    assert np.array_equal(one.per_credential(), np.array([i != 9 for i in range(n)], np.uint8))


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_empty_batch(ctxs, mode):
    """n = 0 writes the neutral partial (the one cc_rlc_partial_device writes), which a finish accepts;
    the host form returns CC_OK with NULL buffers."""
    import torch
    from coconut._lib import lib
    ctx = ctxs[mode]
    _synthetic(ctx, mode, 1, seed=59)
    dev = torch.device("cuda", 0)
    pp = torch.full((929,), -1, dtype=torch.int32, device=dev)
    ps = torch.full((929,), -1, dtype=torch.int32, device=dev)
    N = None
    seed = bytes(32)
    assert lib.cc_pok_rlc_partial_device(ctx.h, 0, 6, 2, 5, 0, seed, N, N, N, N, N, N,
                                         (ctypes.c_uint64 * 2)(1, 4), N, ctypes.c_void_p(pp.data_ptr()), N) == 0
    assert lib.cc_rlc_partial_device(ctx.h, 0, 6, 0, seed, N, N, N, ctypes.c_void_p(ps.data_ptr()), N) == 0
    assert lib.cc_pok_rlc_partial_device(ctx.h, 0, 6, 2, 4, 0, seed, N, N, N, N, N, N,
                                         (ctypes.c_uint64 * 2)(1, 4), N, ctypes.c_void_p(pp.data_ptr()), N) == -2
    torch.cuda.synchronize()
    assert torch.equal(pp, ps)
    assert int(pp[PARTIAL_FLAG]) == 0
    acc = torch.zeros(1, dtype=torch.uint8, device=dev)
    assert lib.cc_rlc_finish_device(ctx.h, 1, ctypes.c_void_p(pp.data_ptr()), ctypes.c_void_p(acc.data_ptr()), N, N) == 0
    torch.cuda.synchronize()
    assert int(acc.item()) == 1
    assert lib.cc_pok_verify_batch_rlc(ctx.h, 0, 6, 0, 7, N, N, N, N, N, N, N, N, N) == 0
    assert lib.cc_pok_verify_batch_rlc(ctx.h, 0, 6, 0, 6, N, N, N, N, N, N, N, N, N) == -2
