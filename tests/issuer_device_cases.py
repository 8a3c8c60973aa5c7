"""Inputs for the exceptional steps of the device form of the request-proof verifier
(cc_sigreq_verify_batch_device, csrc/issue_dev.hip), with a model of its window schedule.

Plain Python, the C oracle and the Python oracle's curve arithmetic through tests/issuer_edges.py (Env,
_finish, expect_request); no product code and no context.  The related-base cases of issuer_edges.py were
steered at the bit ladder of k_sigreq_checks (two scalars that share their top BIT); the ones here are
steered at signed 4-bit windows and at the fixed-base tables' 8-bit windows.

THE SCHEDULE.  Per request one table holds the multiples 1..8 of pk, h, the commitment and every c1_i, c2_i
(prove_common.h sp_fill_*: P, 2P by a doubling, then one mixed addition each; an identity multiple is
flagged and skipped).  Every scalar is reduced mod r and recoded into 65 signed digits (straus.h recode_w4:
v = nibble + carry, carry = v > 8, digit = v - 16 carry).  A check walks the windows 64 .. 0 with four
doublings between two windows unless the accumulator is the identity, and adds per window, in this order,
the digit multiples of
    sk, comm, ct1 : the challenge over pk / the commitment / c1_i
    ct2           : r_2a over pk, r_2b over h, the challenge over c2_i
then the fixed-base terms from the request params' tables (comm: h_0 .. h_(k-1) by r_comm[i], then g by
r_comm[k]; sk, ct1: g by r_sk / r_1; per base the windows 0 .. 31 of 8 bits, entry d 2^(8 w) B), then -T
where T decodes to a finite point, and accepts when the sum is the identity.  model() restates that on affine
points and names the branch of every addition (the CHAIN names of tests/fixed_edges.py) behind the stream it
belongs to:

    pk: h: c:     the variable-base streams        fixed:   a fixed-base table entry
    table:        an addition while the multiples 1..8 are built
    final:        the addition of -T ('final:skipped': T decoded to the identity)
    <stream>:skipped-multiple   a digit whose multiple of a small-order base is the identity

UNREACHABLE BY CONSTRUCTION.  A carry out of the top window (digit 64 != 0) and a digit -8: a reduced
scalar is below r < 0x74 2^248, so nibble 63 is at most 7 and nibble 62 at most 3 when it is, and v = 8
recodes to +8 with no carry (the digits are in [-7, 8]).  test_issuer_device_model.py asserts both over every
scalar used here.  A doubling that lands on the identity needs a point of order 2, which neither curve has.
"""
import functools
import random

import issuer_edges as E
from fixed_edges import R
from torsion_edges import fixture as torsion_fixture

Q, K = 3, 1
WBITS = 8  # the table width the GPU test binds for these cases
ALL8 = int("8" * 63, 16)
ALL9 = int("9" * 63, 16)
ZERO_MIDDLE = (5 << 248) + 3
W50 = 1 << 200  # window 50 of the 4-bit recoding, window 25 of the 8-bit tables
EDGE_SCALARS = (("zero", 0), ("one", 1), ("eight", 8), ("nine", 9), ("r_minus_1", R - 1), ("r", R), ("r_plus_1", R + 1),
                ("max", (1 << 384) - 1), ("all8", ALL8), ("all9", ALL9), ("zero_middle", ZERO_MIDDLE))


def recode(v):
    """straus.h recode_w4 of v mod r: 65 signed digits, least significant first."""
    v %= R
    d, carry = [], 0
    for w in range(64):
        x = ((v >> (4 * w)) & 15) + carry
        carry = int(x > 8)
        d.append(x - 16 * carry)
    return d + [carry]


class _Acc:
    def __init__(self, curve):
        self.curve, self.pt, self.seen, self.log = curve, None, False, []

    def add(self, pt, tag):
        c = self.curve
        if self.pt is None:
            b = "from-identity" if self.seen else "fresh"
        elif self.pt == pt:
            b = "doubling"
        elif self.pt == c.neg(pt):
            b = "to-identity"
        else:
            b = "general"
        self.seen = True
        self.pt = c.add(self.pt, pt)
        self.log.append(f"{tag}:{b}")
        return b


def multiples(curve, P, log):
    """sp_fill_*: [P, 2P, .., 8P] (None: the identity), the branches of its additions into log."""
    if P is None:
        return [None] * 8
    out, J = [], P
    for d in range(8):
        if d == 1:
            J = curve.add(J, J)
        elif d > 1:
            b = ("from-identity" if J is None else "doubling" if J == P else
                 "to-identity" if J == curve.neg(P) else "general")
            log.append(f"table:{b}")
            J = curve.add(J, P)
        out.append(J)
    return out


def model(env, call, req, key):
    """The walk of one check (key = (kind, i)): dict(log: ['stream:branch'], ok: the kernel's verdict)."""
    curve, k = env.curve, call["k"]
    kind, i = key
    d = env.dec
    acc = _Acc(curve)
    chal = recode(req["chal"])
    if kind == "ct2":
        streams = [("pk", d(req["pk"]), recode(req["r2a"][i])), ("h", d(req["h"]), recode(req["r2b"][i])),
                   ("c", d(req["cts"][i][1]), chal)]
        fixed = []
    else:
        C = {"sk": req["pk"], "comm": req["commitment"], "ct1": req["cts"][i][0] if k else None}[kind]
        streams = [("c", d(C), chal)]
        g = d(call["g"])
        fixed = {"sk": [(g, req["r_sk"])], "ct1": [(g, req["r1"][i] if k else 0)],
                 "comm": [(d(call["hvec"][j]), req["r_comm"][j]) for j in range(k)] + [(g, req["r_comm"][k])]}[kind]
    tabs = []
    for tag, P, dig in streams:
        if P is None:
            acc.log.append(f"{tag}:skipped")
        tabs.append((tag, multiples(curve, P, acc.log), dig, P is None))
    for win in range(64, -1, -1):
        if win != 64 and acc.pt is not None:
            for _ in range(4):
                acc.pt = curve.add(acc.pt, acc.pt)
        for tag, mult, dig, ident in tabs:
            dv = dig[win]
            if not dv or ident:
                continue
            e = mult[abs(dv) - 1]
            if e is None:
                acc.log.append(f"{tag}:skipped-multiple")
                continue
            acc.add(curve.neg(e) if dv < 0 else e, tag)
    for B, s in fixed:
        if B is None:
            acc.log.append("fixed:skipped")
            continue
        s %= R
        for w in range((256 + WBITS - 1) // WBITS):
            dv = (s >> (WBITS * w)) & ((1 << WBITS) - 1)
            if not dv:
                continue
            e = curve.mul_any(B, dv << (WBITS * w))
            if e is None:
                acc.log.append("fixed:skipped-multiple")
                continue
            acc.add(e, "fixed")
    T = d(req["T"][key])
    if T is None:
        acc.log.append("final:skipped")
    else:
        acc.add(curve.neg(T), "final")
    return dict(log=acc.log, ok=acc.pt is None)


def keys(call):
    return [("sk", 0), ("comm", 0)] + [(kd, i) for i in range(call["k"]) for kd in ("ct1", "ct2")]


def model_request(env, call, req):
    """The device verdict the model predicts, and the union of its checks' logs per kind."""
    logs = {key: model(env, call, req, key) for key in keys(call)}
    ok = all(v["ok"] for v in logs.values()) and all(a % R == b % R for a, b in zip(req["r2b"], req["r_comm"]))
    return int(ok), {key: v["log"] for key, v in logs.items()}


def scalars_of(req):
    return [req["r_sk"], req["chal"]] + req["r_comm"] + req["r1"] + req["r2a"] + req["r2b"]


@functools.lru_cache(maxsize=None)
def _call(oc_key, mode):
    env = E.Env(E._OC[oc_key], 2 if mode == "G2" else 1)
    seed = 7000 + E.MODES[mode]
    g, hvec = E._params(env, Q, seed)
    call = dict(name="device_cases", q=Q, k=K, g=g, hvec=hvec, slices=())
    rng = random.Random(seed + 1)
    fr = lambda: rng.randrange(1 << 250, R)  # noqa: E731
    small = lambda: rng.randrange(1 << 60, 1 << 100)  # noqa: E731  (every digit below window 25)
    out = []

    def new(name, intent, *reach):
        rc = [fr() for _ in range(K + 1)]
        req = dict(name=name, intent=intent, reach=list(reach), pk=env.rand_pt(rng), commitment=env.rand_pt(rng),
                   known=[fr() for _ in range(Q - K)], cts=[[env.rand_pt(rng), env.rand_pt(rng)] for _ in range(K)],
                   r_sk=fr(), r_comm=rc, r1=[fr() for _ in range(K)], r2a=[fr() for _ in range(K)], r2b=list(rc[:K]),
                   chal=fr(), T_mod={}, T_chal={}, post=[])
        out.append(req)
        return req

    def set_all(req, vals):
        it = iter(vals * (3 * K + 3))
        req["r_sk"], req["chal"] = next(it), next(it)
        req["r_comm"] = [next(it) for _ in range(K + 1)]
        req["r1"], req["r2a"] = [next(it) for _ in range(K)], [next(it) for _ in range(K)]
        req["r2b"] = list(req["r_comm"][:K])

    # ---- challenge and responses on the edges of the signed-digit recoding
    for nm, v in EDGE_SCALARS:
        set_all(new(f"scalars_all_{nm}", 1), [v])
    set_all(new("scalars_mixed", 1), [v for _, v in EDGE_SCALARS])
    set_all(new("scalars_mixed_rotated", 1), [v for _, v in EDGE_SCALARS[5:] + EDGE_SCALARS[:5]])
    # ---- related variable bases: the streams of ct2 double, cancel and restart from the identity
    v = 3 * W50 + 5  # digit 3 in window 50, 5 in window 0
    r0 = new("pk_eq_h", 1, ("ct2", "h:doubling"))
    r0.update(pk=(lambda h: h), chal=small())
    r0["r2a"][0] = r0["r2b"][0] = r0["r_comm"][0] = v
    r0 = new("pk_eq_neg_h", 1, ("ct2", "h:to-identity"), ("ct2", "c:from-identity"))
    r0.update(pk=env.neg, chal=small())
    r0["r2a"][0] = r0["r2b"][0] = r0["r_comm"][0] = v
    r0 = new("c2_eq_pk", 1, ("ct2", "c:doubling"))
    r0["cts"][0][1], r0["chal"] = r0["pk"], v
    r0["r2a"][0], r0["r2b"][0], r0["r_comm"][0] = v, 0, 0
    r0 = new("c2_eq_neg_pk", 1, ("ct2", "c:to-identity"), ("ct2", "pk:from-identity"))
    r0["cts"][0][1], r0["chal"] = env.neg(r0["pk"]), v
    r0["r2a"][0], r0["r2b"][0], r0["r_comm"][0] = v, 0, 0
    # ---- the fixed-base part against the challenge multiple: F = S1, F = -S1 (T the identity against an
    # identity sum), in the checks of kind 0 (sk, ct1) and in comm
    w = 7 << 16  # one 8-bit window of the tables, digits 7 in the 4-bit window 4
    ng = env.neg(g)
    r0 = new("c1_eq_g_F_eq_S1", 1, ("ct1", "fixed:doubling"))
    r0["cts"][0][0], r0["r1"][0], r0["chal"] = g, w, w
    r0 = new("c1_eq_neg_g_F_eq_neg_S1", 1, ("ct1", "fixed:to-identity"), ("ct1", "final:skipped"))
    r0["cts"][0][0], r0["r1"][0], r0["chal"] = ng, w, w
    r0 = new("pk_eq_g_F_eq_S1", 1, ("sk", "fixed:doubling"))
    r0.update(pk=g, r_sk=w, chal=w)
    r0 = new("pk_eq_neg_g_F_eq_neg_S1", 1, ("sk", "fixed:to-identity"), ("sk", "final:skipped"))
    r0.update(pk=ng, r_sk=w, chal=w)
    r0 = new("commitment_eq_h0_F_eq_S1", 1, ("comm", "fixed:doubling"))
    r0.update(commitment=hvec[0], chal=w)
    r0["r_comm"][0] = r0["r2b"][0] = w
    r0 = new("commitment_eq_neg_g", 1, ("comm", "fixed:to-identity"), ("comm", "final:skipped"))
    r0.update(commitment=ng, chal=w)
    r0["r_comm"] = [0, w]
    r0["r2b"][0] = 0
    # F + S1 = T with T finite is every accepted request above ('final:to-identity'); a finite T against an
    # identity sum, and the identity T against a finite sum, are refused
    for key in (("sk", 0), ("ct2", 0)):
        r0 = new(f"zero_sum_finite_T_{key[0]}", 0, (key[0], "final:fresh"))
        set_all(r0, [0, R])
        r0["T_mod"][key] = lambda t, pt=env.rand_pt(rng): pt
        r0 = new(f"finite_sum_identity_T_{key[0]}", 0, (key[0], "final:skipped"))
        r0["T_mod"][key] = lambda t: env.identity
    # ---- small-order elgamal_pk and ciphertext halves: multiples that are the identity, sums that pass
    # through it (the decoders test the curve equation alone)
    tor = torsion_fixture()["G1" if env.group == 1 else "G2"]
    for nm in sorted(tor):  # every point of the fixture, as the key and as both halves of the ciphertext
        new(f"pk_{nm}", 1)["pk"] = tor[nm]["point"]
        new(f"c1_c2_{nm}", 1)["cts"][0] = [tor[nm]["point"], tor[nm]["point"]]
    m = 3 if env.group == 1 else 13
    t0 = tor["T3" if env.group == 1 else "T13"]["point"]
    # the challenge m on a base of order m: 3 is one digit whose multiple is the identity; 13 recodes to
    # (-3, 1), and 16 P - 3 P is the identity
    r0 = new(f"pk_order_{m}_chal_{m}", 1, ("sk", "c:skipped-multiple" if m == 3 else "c:to-identity"))
    r0.update(pk=t0, chal=m)
    r0 = new(f"c2_order_{m}_chal_{m}", 1, ("ct2", "c:skipped-multiple" if m == 3 else "c:to-identity"))
    r0["cts"][0][1], r0["chal"] = t0, m
    r0["r2a"][0] = r0["r2b"][0] = r0["r_comm"][0] = 0  # the challenge's stream alone
    if m == 3:  # the table of an order-3 base: 2P = -P, 3P = O, 4P = P again, 5P by the doubling branch
        r0 = new("pk_order_3_chal_0x363", 1, ("sk", "table:to-identity"), ("sk", "table:from-identity"),
                 ("sk", "table:doubling"), ("sk", "c:skipped-multiple"))
        r0.update(pk=t0, chal=0x363)
    call["reqs"] = [E._finish(env, call, r) for r in out]
    return call


def device_call(oc, mode):
    """The one call (q = 3, k = 1) of a group mode: dict(name, q, k, g, hvec, reqs), shared, not to be modified."""
    E._OC[id(oc)] = oc
    return _call(id(oc), mode)
