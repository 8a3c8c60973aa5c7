"""GPU tests of the keygen entry points (csrc/keygen.hip, capi_keygen.cpp): cc_set_keygen_params,
cc_keygen_deal_batch(_device) and cc_keygen_combine_batch(_device), byte for byte against the oracle's
pedersen_deal / get_shared_secret and the restatement in tests/keygen_deal_cases.py (whose cases
tests/test_keygen_deal_model.py checks on the CPU), in both group modes, with forced 8-bit tables unless a test
says otherwise; then the chains the layouts promise and the reference's own keygen tests (keygen.rs:216-369,
signature.rs:668-708) with every key from the device."""
import ctypes

import numpy as np
import pytest

import keygen_deal_cases as KC

pytestmark = pytest.mark.gpu

MODES = KC.MODES
R = KC.R
OK, ERR_THRESHOLD, ERR_DECODE, ERR_STATE = 0, -3, -4, -7
KEYS = ("x", "y", "xt", "yt", "comm", "X", "Y")


@pytest.fixture(scope="module")
def ctxs():
    import coconut
    c = {m: coconut.Context(0, coconut.GroupMode(v)) for m, v in MODES.items()}
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(scope="module")
def stream():
    import torch
    return torch.cuda.Stream(torch.device("cuda", 0))


def _bind(ctx, mode, bits=8, gt=None, g=None, h=None):
    gtb, gb, hb = KC.base_bytes(mode)
    ctx.set_keygen_params(gt or gtb, g or gb, h or hb, table_bits=bits)


def _deal(ctx, case, pedersen=True):
    from coconut import keygen_deal_batch
    t, total, q = case["shape"]
    out = keygen_deal_batch(ctx, case["m"], q, t, total, KC.coeff_bytes(case["cf"]),
                            KC.coeff_bytes(case["ct"]) if pedersen else None)
    return dict(zip(KEYS, out))


def _same(got, want, what=""):
    for k in KEYS:
        if k in want:
            assert got[k] == want[k], (what, k, _first_diff(got[k], want[k], k))
        else:
            assert got[k] is None, (what, k)


def _first_diff(a, b, k):
    w = {"comm": 97}.get(k, 48)
    return next((i // w for i in range(0, min(len(a), len(b)), w) if a[i:i + w] != b[i:i + w]), "length")


def _want(mode, case, gt="default"):
    gtp = KC.bases()[2][mode] if gt == "default" else gt
    return KC.pack(case["vals"], mode, gtp)


# ---------------------------------------------------------------- byte for byte against the oracle
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("kind", ["pedersen", "shamir"])
@pytest.mark.parametrize("shape", KC.SHAPES, ids=str)
def test_one_keygen_matches_the_oracle(ctxs, mode, kind, shape):
    _bind(ctxs[mode], mode)
    if kind == "pedersen":
        case = KC.first_keygen(KC.pedersen_case(shape, 3 if shape in KC.M3_SHAPES else 1))
    else:
        case = KC.shamir_case(shape)
    _same(_deal(ctxs[mode], case, kind == "pedersen"), _want(mode, case), (shape, kind))


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("shape", KC.M3_SHAPES, ids=str)
def test_three_keygens_over_distinct_coefficients(ctxs, mode, shape):
    _bind(ctxs[mode], mode)
    case = KC.pedersen_case(shape, 3)
    assert len(set(case["cf"])) == len(case["cf"])
    _same(_deal(ctxs[mode], case), _want(mode, case), shape)
    shamir = dict(case, ct=None, vals=dict(case["vals"], xt=[], yt=[], comm=[]))
    _same(_deal(ctxs[mode], shamir, False), _want(mode, shamir), shape)


def test_shamir_only_params_need_no_generators(ctxs):
    ctx, case = ctxs["G2"], KC.shamir_case((1, 3, 1))
    ctx.set_keygen_params(KC.base_bytes("G2")[0], table_bits=8)
    _same(_deal(ctx, case, False), _want("G2", case))


# ---------------------------------------------------------------- edge scalars, table widths
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("bits", [8, 13, 16])
def test_edge_scalars_and_table_widths(ctxs, mode, bits):
    """Coefficients 0, 1, r - 1, r, r + 1, 2^384 - 1 and the bits beside every window boundary of the 8- and
    13-bit tables, as f_0 (so as share and verkey scalar too) and as coefficients of every degree; the zero
    polynomial; f_i = 0 beside f'_i != 0 and the reverse; and the reference's shape, at three table widths."""
    _bind(ctxs[mode], mode, bits)
    for case in (KC.edge_unit_case(), KC.edge_poly_case(), KC.first_keygen(KC.pedersen_case((3, 5, 7), 1))):
        _same(_deal(ctxs[mode], case), _want(mode, case), (bits, case["shape"]))


@pytest.mark.parametrize("mode", sorted(MODES))
def test_related_generators_double_cancel_and_restart(ctxs, mode):
    """h = g with f_i = f'_i in one window: the second entry equals the running sum; h = -g: it cancels it;
    with a further window the sum restarts from the identity (test_keygen_deal_model.py traces the walk)."""
    from oracle import bls12_381 as B
    for name, h, case, _ in KC.related_cases():
        _bind(ctxs[mode], mode, h=B.g1_to_bytes(h))
        _same(_deal(ctxs[mode], case), _want(mode, case), name)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_bases_that_decode_to_the_identity_are_skipped(ctxs, mode):
    """g, h and g~ in turn as the identity, with a bad prefix (G1), off the curve, and with coordinates >= p
    (which decode mod p to the point itself)."""
    cf, ct = KC.bad_base_inputs()
    case = {"shape": (2, 2, 1), "m": 1, "cf": cf, "ct": ct}
    for name, gt, g, h, want in KC.bad_base_cases(mode):
        _bind(ctxs[mode], mode, gt=gt, g=g, h=h)
        _same(_deal(ctxs[mode], case), want, name)


# ---------------------------------------------------------------- block boundaries
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("count", [63, 64, 65, 255, 256, 257])
def test_task_counts_around_the_block_sizes(ctxs, mode, count):
    """Keygens of shape (1, 1, 0) are one task each in the evaluation, commitment and derivation spaces, so m is
    the task count of all three: below, at and above the 64-lane wave, the 128-pair and the 256-lane block;
    the odd counts leave a lane pair's block half empty."""
    _bind(ctxs[mode], mode)
    case = KC.cycled(KC.unit_pool(), count)
    _same(_deal(ctxs[mode], case), _want(mode, case), count)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_several_blocks_of_a_shape_with_every_axis(ctxs, mode):
    """43 keygens of (2, 2, 2): 258 evaluation, commitment and derivation tasks, indices with all of keygen,
    polynomial, signer and coefficient in them, across a block boundary."""
    _bind(ctxs[mode], mode)
    case = KC.cycled(KC.pedersen_case((2, 2, 2), 3), 43)
    _same(_deal(ctxs[mode], case), _want(mode, case))


# ---------------------------------------------------------------- device forms
def _to(b):
    import torch
    return torch.frombuffer(bytearray(b) or bytearray(1), dtype=torch.uint8)[:len(b)].to(torch.device("cuda", 0))


def _host(t):
    return None if t is None else bytes(t.cpu().numpy())


@pytest.mark.parametrize("mode", sorted(MODES))
def test_device_forms_give_the_host_forms_bytes(ctxs, stream, mode):
    import torch
    from coconut import keygen_combine_batch, keygen_combine_batch_device, keygen_deal_batch_device
    ctx = ctxs[mode]
    _bind(ctx, mode)
    case = KC.pedersen_case((2, 2, 1), 4)
    t, total, q = case["shape"]
    host = _deal(ctx, case)
    _same(host, _want(mode, case))
    cf, ct = _to(KC.coeff_bytes(case["cf"])), _to(KC.coeff_bytes(case["ct"]))
    stream.wait_stream(torch.cuda.current_stream())  # the uploads
    dev = keygen_deal_batch_device(ctx, 4, q, t, total, cf, ct, stream=stream)
    sss = keygen_deal_batch_device(ctx, 4, q, t, total, cf, None, stream=stream)
    comb = keygen_combine_batch_device(ctx, 2, 2, q, t, total, *dev[:5], stream=stream)
    comb_sss = keygen_combine_batch_device(ctx, 2, 2, q, t, total, *sss[:2], stream=stream)
    stream.synchronize()
    assert [_host(o) for o in dev] == [host[k] for k in KEYS]
    assert [_host(o) for o in sss] == [host["x"], host["y"], None, None, None, host["X"], host["Y"]]
    want = keygen_combine_batch(ctx, 2, 2, q, t, total, *[host[k] for k in KEYS[:5]])
    assert [_host(o) for o in comb] == list(want)
    assert [_host(o) for o in comb_sss] == [want[0], want[1], None, None, None, want[5], want[6]]


# ---------------------------------------------------------------- the chains the layouts promise
@pytest.mark.parametrize("mode", sorted(MODES))
def test_outputs_chain_into_share_verification_and_verkey_aggregation(ctxs, mode):
    from coconut import fixed_base_mul, verkey_aggregate_ids, vss_verify_batch
    ctx = ctxs[mode]
    _bind(ctx, mode)
    case = KC.pedersen_case((2, 2, 2), 3)
    t, total, q = case["shape"]
    m = case["m"]
    got = _deal(ctx, case)
    gtb, gb, hb = KC.base_bytes(mode)
    ctx.set_params(gtb)
    # 1. out_comm is cc_vss_verify_batch's commitments with n_sets = m (q + 1); the shares as (s, s') pairs
    sets = [[got["comm"][(s * t + i) * 97:(s * t + i + 1) * 97] for i in range(t)] for s in range(m * (q + 1))]
    set_of, ids, shares = [], [], []
    for k in range(m):
        for p in range(q + 1):
            for i in range(total):
                o = (k * total + i) if p == 0 else ((k * total + i) * q + p - 1)
                a, b = (got["x"], got["xt"]) if p == 0 else (got["y"], got["yt"])
                set_of.append(k * (q + 1) + p)
                ids.append(i + 1)
                shares.append((a[o * 48:(o + 1) * 48], b[o * 48:(o + 1) * 48]))
    assert vss_verify_batch(ctx, t, gb, hb, sets, set_of, ids, shares).all()
    bad = list(shares)
    bad[7] = (KC.be48((int.from_bytes(bad[7][0], "big") + 1) % R), bad[7][1])
    v = vss_verify_batch(ctx, t, gb, hb, sets, set_of, ids, bad)
    assert v[7] == 0 and v.sum() == len(ids) - 1
    # 2. a keygen's out_X / out_Y slice is cc_set_issuers' X / Y; the first t verkeys aggregate to g~ * secret
    ob = KC.oth(mode)[3]
    for k in range(m):
        ctx.set_issuers(list(range(1, total + 1)), got["X"][k * total * ob:(k + 1) * total * ob],
                        got["Y"][k * total * q * ob:(k + 1) * total * q * ob], q)
        oX, oY = verkey_aggregate_ids(ctx, 1, t, t, np.array([list(range(1, t + 1))], np.uint64))
        secrets = b"".join(KC.be48(case["secrets"][k][p][0]) for p in range(q + 1))
        assert oX + oY == fixed_base_mul(ctx, 1 if mode == "G2" else 2, gtb, secrets), k


# ---------------------------------------------------------------- combine
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", ["d1_identity_map", "d5_dealers", "two_equal_dealers", "two_opposite_dealers",
                                  "three_dealers_two_opposite", "identity_and_undecodable_commitments", "shares_ge_r",
                                  "two_groups"])
def test_combine_matches_the_sums(ctxs, mode, name):
    from coconut import keygen_combine_batch
    cases = {c[0]: c for c in KC.combine_cases()}
    assert name in cases and len(cases) == 8
    _, m, d, (t, total, q), ins, exp = cases[name]
    ctx = ctxs[mode]
    _bind(ctx, mode)
    got = dict(zip(KEYS, keygen_combine_batch(ctx, m, d, q, t, total, *[ins[k] for k in KEYS[:5]])))
    want = {k: exp[k] for k in KEYS[:5]}
    want["X"], want["Y"] = KC.combine_verkeys(mode, exp, total, q)
    _same(got, want, name)
    # without the Pedersen buffers: the same shares and verkeys
    got = dict(zip(KEYS, keygen_combine_batch(ctx, m, d, q, t, total, ins["x"], ins["y"])))
    _same(got, {k: want[k] for k in ("x", "y", "X", "Y")}, name)


# ---------------------------------------------------------------- the reference's own flows
def _lagrange0(ids, i):
    num = den = 1
    for x in ids:
        if x != i:
            num, den = num * x % R, den * (x - i) % R
    return num * pow(den, -1, R) % R


def _as_flow_signers(signers):
    return [{"id": s.id, "x": int.from_bytes(s.sigkey.x, "big"), "y": [int.from_bytes(v, "big") for v in s.sigkey.y],
             "vk": s.verkey} for s in signers]


def _check_reconstructed_keys(f, t, secret_x, secret_y, signers):
    """keygen.rs:231-297: the first t shares reconstruct every secret, and Verkey::aggregate of the first t
    verkeys is g~ * secret (check_key_aggregation compares it with cc_fixed_base_mul, twice)."""
    from test_gpu_reference_flows import check_key_aggregation
    ids = [s["id"] for s in signers[:t]]
    sx = int.from_bytes(secret_x, "big")
    sy = [int.from_bytes(v, "big") for v in secret_y]
    assert sum(_lagrange0(ids, s["id"]) * s["x"] for s in signers[:t]) % R == sx
    for j in range(f.q):
        assert sum(_lagrange0(ids, s["id"]) * s["y"][j] for s in signers[:t]) % R == sy[j]
    check_key_aggregation(f, t, sx, sy, [(s["id"], s["vk"]) for s in signers[:t]])


def _draw(f, count):
    return b"".join(KC.be48(f.rng.fr()) for _ in range(count))


def _sss(f, t, total):
    import coconut
    sx, sy, signers = coconut.trusted_party_SSS_keygen(t, total, f.params, ctx=f.ctx, coeffs=_draw(f, (f.q + 1) * t))
    return sx, sy, _as_flow_signers(signers), signers


def _pvss_gens(f):
    return f.co.hash_to_curve(f.ctx, 1, [b"testPVSS : g", b"testPVSS : h"])  # PedersenVSS::gens("testPVSS")


def _pvss(f, t, total):
    """trusted_party_PVSS_keygen with every dealt share checked by verify_share on the GPU (keygen.rs:333-352)."""
    import coconut
    g, h = _pvss_gens(f)
    n = (f.q + 1) * t
    out = coconut.trusted_party_PVSS_keygen(t, total, f.params, g, h, ctx=f.ctx, coeffs=_draw(f, n), coeffs_t=_draw(f, n))
    sx, sy, signers, _sxt, cx, xs, xts, _syt, cy, ys, yts = out
    sets = [[cx[i] for i in range(t)]] + [[c[i] for i in range(t)] for c in cy]
    set_of = [p for p in range(f.q + 1) for _ in range(total)]
    ids = [i for _ in range(f.q + 1) for i in range(1, total + 1)]
    shares = [(xs[i], xts[i]) for i in range(1, total + 1)]
    shares += [(ys[j][i], yts[j][i]) for j in range(f.q) for i in range(1, total + 1)]
    assert f.co.vss_verify_batch(f.ctx, t, g, h, sets, set_of, ids, shares).all()
    return sx, sy, _as_flow_signers(signers)


def _dvss(f, t, total):
    """setup_signers_for_test (keygen.rs:169-205): every participant deals a (t, total) sharing of its own secret
    for x and for every y, every share is verified against its dealer's commitments, and the final shares,
    commitments and verkeys are the sums over the dealers; the distributed secret is the sum of theirs."""
    from coconut import keygen_combine_batch, keygen_deal_batch
    g, h = _pvss_gens(f)
    q, n = f.q, total * (f.q + 1) * t
    f.ctx.set_keygen_params(f.params.g_tilde, g, h)
    cf, ct = _draw(f, n), _draw(f, n)
    x, y, xt, yt, comm, _, _ = keygen_deal_batch(f.ctx, total, q, t, total, cf, ct)
    sets = [[comm[(s * t + i) * 97:(s * t + i + 1) * 97] for i in range(t)] for s in range(total * (q + 1))]
    set_of, ids, shares = [], [], []
    for k in range(total):
        for p in range(q + 1):
            for i in range(total):
                o = (k * total + i) if p == 0 else ((k * total + i) * q + p - 1)
                a, b = (x, xt) if p == 0 else (y, yt)
                set_of.append(k * (q + 1) + p)
                ids.append(i + 1)
                shares.append((a[o * 48:(o + 1) * 48], b[o * 48:(o + 1) * 48]))
    assert f.co.vss_verify_batch(f.ctx, t, g, h, sets, set_of, ids, shares).all()
    cx, cy, cxt, cyt, ccomm, X, Y = keygen_combine_batch(f.ctx, 1, total, q, t, total, x, y, xt, yt, comm)
    # the combined shares verify against the combined commitments
    sets = [[ccomm[(p * t + i) * 97:(p * t + i + 1) * 97] for i in range(t)] for p in range(q + 1)]
    fin = [(cx[i * 48:(i + 1) * 48], cxt[i * 48:(i + 1) * 48]) for i in range(total)]
    fin += [(cy[(i * q + j) * 48:(i * q + j + 1) * 48], cyt[(i * q + j) * 48:(i * q + j + 1) * 48])
            for j in range(q) for i in range(total)]
    assert f.co.vss_verify_batch(f.ctx, t, g, h, sets, [p for p in range(q + 1) for _ in range(total)],
                                 [i + 1 for _ in range(q + 1) for i in range(total)], fin).all()
    sec = [sum(int.from_bytes(cf[((k * (q + 1) + p) * t) * 48:((k * (q + 1) + p) * t + 1) * 48], "big")
               for k in range(total)) % R for p in range(q + 1)]
    ob = f.ob
    signers = [{"id": i + 1, "x": int.from_bytes(cx[i * 48:(i + 1) * 48], "big"),
                "y": [int.from_bytes(cy[(i * q + j) * 48:(i * q + j + 1) * 48], "big") for j in range(q)],
                "vk": f.co.Verkey(X[i * ob:(i + 1) * ob], [Y[(i * q + j) * ob:(i * q + j + 1) * ob] for j in range(q)])}
               for i in range(total)]
    return KC.be48(sec[0]), [KC.be48(v) for v in sec[1:]], signers


def _flow(ctxs, mode, seed, q):
    from test_gpu_reference_flows import Flow
    return Flow(ctxs[mode], mode, seed=seed, q=q)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_keygen(ctxs, mode):
    """keygen.rs:216-229."""
    f = _flow(ctxs, mode, 901, 7)
    _, _, _, signers = _sss(f, 3, 5)
    assert len(signers) == 5
    for i, s in enumerate(signers):
        assert s.id == i + 1 and len(s.sigkey.y) == 7 and len(s.verkey.Y_tilde) == 7


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("keygen", ["shamir", "verifiable", "decentralized_verifiable"])
def test_keygen_reconstruction_secret_sharing(ctxs, mode, keygen):
    """test_keygen_reconstruction_{shamir, verifiable, decentralized_verifiable}_secret_sharing
    (keygen.rs:299-369): t = 3 of 5, msg_count = 7."""
    f = _flow(ctxs, mode, 911 + len(keygen), 7)
    sx, sy, signers = {"shamir": lambda: _sss(f, 3, 5)[:3], "verifiable": lambda: _pvss(f, 3, 5),
                       "decentralized_verifiable": lambda: _dvss(f, 3, 5)}[keygen]()
    _check_reconstructed_keys(f, 3, sx, sy, signers)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("keygen", ["shamir", "verifiable", "decentralized_verifiable"])
def test_sign_verify_secret_sharing_keygen(ctxs, mode, keygen):
    """test_sign_verify_{shamir, verifiable, decentralized_verifiable}_secret_sharing_keygen
    (signature.rs:668-708 and the decentralized one beside them): t = 3 of 5, msg_count = 6, 2 hidden."""
    from test_gpu_reference_flows import check_signing_on_random_msgs
    f = _flow(ctxs, mode, 931 + len(keygen), 6)
    _, _, signers = {"shamir": lambda: _sss(f, 3, 5)[:3], "verifiable": lambda: _pvss(f, 3, 5),
                     "decentralized_verifiable": lambda: _dvss(f, 3, 5)}[keygen]()
    check_signing_on_random_msgs(f, 3, 6, 2, signers)


# ---------------------------------------------------------------- errors and empties
def _raw_deal(ctx, m, q, t, total, null=(), pedersen=True):
    """cc_keygen_deal_batch on one-byte dummies (every case here is refused before anything is read)."""
    from coconut._lib import lib
    keep = [ctypes.create_string_buffer(8) for _ in range(9)]
    names = ("coeffs", "coeffs_t", "x", "y", "xt", "yt", "comm", "X", "Y")
    ptr = [None if n in null or (not pedersen and n in ("coeffs_t", "xt", "yt", "comm")) else ctypes.cast(b, ctypes.c_void_p)
           for n, b in zip(names, keep)]
    return lib.cc_keygen_deal_batch(ctx.h, m, q, t, total, *ptr)


def _raw_combine(ctx, m, d, q, t, total, null=(), pedersen=True):
    from coconut._lib import lib
    keep = [ctypes.create_string_buffer(8) for _ in range(12)]
    names = ("x", "y", "xt", "yt", "comm", "ox", "oy", "oxt", "oyt", "ocomm", "oX", "oY")
    ped = ("xt", "yt", "comm", "oxt", "oyt", "ocomm")
    ptr = [None if n in null or (not pedersen and n in ped) else ctypes.cast(b, ctypes.c_void_p)
           for n, b in zip(names, keep)]
    return lib.cc_keygen_combine_batch(ctx.h, m, d, q, t, total, *ptr)


def test_errors_in_the_headers_order_and_empty_batches():
    import coconut
    from coconut._lib import lib
    BIG = 1 << 26
    ctx = coconut.Context(0, coconut.GroupMode.SIG_G2)
    try:
        gtb, gb, hb = KC.base_bytes("G2")
        p = lambda b: ctypes.cast(ctypes.create_string_buffer(bytes(b)), ctypes.c_void_p)  # noqa: E731
        # cc_set_keygen_params: exactly one generator, a width outside {0, 8..16}, no g~
        for args in ((p(gtb), p(gb), None, 8), (p(gtb), None, p(hb), 8), (p(gtb), p(gb), p(hb), 7),
                     (p(gtb), p(gb), p(hb), 17), (None, p(gb), p(hb), 8)):
            assert lib.cc_set_keygen_params(ctx.h, *args) == ERR_DECODE
        # 2 before 3: a NULL buffer is refused before the missing params are noticed; q = 0 needs no y buffers
        for n in ("coeffs", "x", "X", "y", "Y", "xt", "yt", "comm"):
            assert _raw_deal(ctx, 1, 1, 1, 1, null=(n,)) == ERR_DECODE, n
        for n in ("x", "ox", "oX", "y", "oy", "oY", "xt", "comm", "oxt", "ocomm", "yt", "oyt"):
            assert _raw_combine(ctx, 1, 1, 1, 1, 1, null=(n,)) == ERR_DECODE, n
        # 3: no keygen params (before the threshold and the ceilings), also for m = 0
        for m in (1, 0):
            assert _raw_deal(ctx, m, 1, 0, 1) == ERR_STATE
            assert _raw_deal(ctx, m, 0, 1, 1, null=("y", "Y", "yt")) == ERR_STATE
            assert _raw_combine(ctx, m, 0, 1, 1, 1) == ERR_STATE
        # a failed cc_set_keygen_params leaves the context without params
        ctx.set_keygen_params(gtb, gb, hb, table_bits=8)
        assert _raw_deal(ctx, 0, 1, 1, 1) == OK
        assert lib.cc_set_keygen_params(ctx.h, p(gtb), p(gb), None, 8) == ERR_DECODE
        ctx._kg = None
        assert _raw_deal(ctx, 0, 1, 1, 1) == ERR_STATE
        # 3: Shamir-only params refuse coeffs_t / comm
        ctx.set_keygen_params(gtb, table_bits=8)
        assert _raw_deal(ctx, 1, 1, 1, 1) == ERR_STATE and _raw_deal(ctx, 0, 1, 1, 1) == ERR_STATE
        assert _raw_combine(ctx, 1, 1, 1, 1, 1) == ERR_STATE
        assert _raw_deal(ctx, 0, 1, 1, 1, pedersen=False) == OK
        assert _raw_combine(ctx, 0, 1, 1, 1, 1, pedersen=False) == OK
        ctx.set_keygen_params(gtb, gb, hb, table_bits=8)
        # 4: the threshold, before the ceilings and for m = 0
        for m in (1, 0):
            assert _raw_deal(ctx, m, 1, 0, 1) == ERR_THRESHOLD
            assert _raw_deal(ctx, m, 1, 3, 2) == ERR_THRESHOLD
            assert _raw_deal(ctx, m, 5000, 0, 1 << 17) == ERR_THRESHOLD
            assert _raw_combine(ctx, m, 0, 1, 2, 1) == ERR_THRESHOLD
        # 5: the ceilings, for m = 0 too where they do not depend on m
        for m in (1, 0):
            assert _raw_deal(ctx, m, 1, 1, (1 << 16) + 1) == ERR_DECODE
            assert _raw_deal(ctx, m, 4097, 1, 1) == ERR_DECODE
            assert _raw_combine(ctx, m, 0, 1, 1, 1) == ERR_DECODE  # d = 0
        assert _raw_deal(ctx, BIG, 1, 1, 1) == ERR_DECODE          # m total (q + 1) = 2^27
        assert _raw_deal(ctx, BIG + 1, 0, 1, 1) == ERR_DECODE      # m alone
        assert _raw_deal(ctx, 1 << 11, 0, 1 << 16, 1 << 16) == ERR_DECODE  # m total (q + 1) = m (q + 1) t = 2^27
        assert _raw_deal(ctx, 1 << 15, 4095, 1, 1) == ERR_DECODE   # 2^27 again, through q
        assert _raw_combine(ctx, 1 << 13, 1 << 14, 0, 1, 1) == ERR_DECODE  # m d = 2^27
        # 6: m = 0 is a no-op with NULL buffers
        N = None
        assert lib.cc_keygen_deal_batch(ctx.h, 0, 3, 2, 4, N, N, N, N, N, N, N, N, N) == OK
        assert lib.cc_keygen_deal_batch_device(ctx.h, 0, 3, 2, 4, N, N, N, N, N, N, N, N, N, N) == OK
        assert lib.cc_keygen_combine_batch(ctx.h, 0, 2, 3, 2, 4, N, N, N, N, N, N, N, N, N, N, N, N) == OK
        assert lib.cc_keygen_combine_batch_device(ctx.h, 0, 2, 3, 2, 4, N, N, N, N, N, N, N, N, N, N, N, N, N) == OK
        # the context still deals after all of the above
        case = KC.first_keygen(KC.pedersen_case((1, 3, 1), 3))
        _same(_deal(ctx, case), _want("G2", case))
    finally:
        ctx.close()
