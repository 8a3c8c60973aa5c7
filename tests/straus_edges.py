"""Edge-case inputs for the variable-base windowed Straus MSMs (csrc/straus.h, aggregate.hip k_msm_straus
and k_msm_straus_g2lz_g, pervk.hip k_prep_sig*_var and their one-wave forms), with every discrete
logarithm known, and a model of the order in which each kernel adds its table entries.

Plain Python over integers plus the C oracle's oc_gen_mul / oc_msm (points from scalars); no product code
and no context.  Chain, join and the constants come from tests/fixed_edges.py.

POINTS.  Every base is a known multiple of the generator, or of the group's small-order base T of order
ORDER[group]: in G1 the order-3 point (0, 2) of y^2 = x^3 + 4 (2 T = -T = (0, -2)), in G2 the order-13 point
T13 of tests/golden/torsion.json (the twist's cofactor is divisible by 13^2); the decoders accept both: they
check the curve equation, not the subgroup.  A point a G + b T is the integer v mod M = 39 r with v = a mod r
and v = b mod the order of T (the Chinese remainder theorem: Z_39r = Z_r x Z_3 x Z_13; a G1 point has no
part mod 13 and a G2 point none mod 3), so equality, negation and the identity are what they are in the
group, and a scalar acts by integer multiplication.  For the order-3 base the multiples 3 T and 6 T are the
identity (flagged in the table and skipped in the walk) and the table build's 5 T = 4 T + T = T + T comes
from the doubling branch of the mixed addition.  The order-13 base's table 1 T .. 8 T meets neither (no
multiple below 13 is the identity, and k T = +-T needs k = 12 or 14), so in G2 the build stays on the general
branch; what the order-13 rows add is a small-order base in every G2 walk and join, whose sums (and, in
SigG1 verify, the Miller loop over a pr of order 13 r) the oracle pins.

DIGITS.  recode_w4 restates straus.h: 64 nibbles with a carry, digit v - 16 if v > 8, and a 65th digit
that is the last carry.  Two facts follow from the code, and tests/test_straus_edges_model.py asserts them:
  * the digits lie in [-7, 8]: -8 never occurs (v - 16 = -8 needs v = 8, which is kept as +8);
  * for a canonical scalar d[64] = 0 and d[63] <= 7.  The top nibble of r = 0x73ED... is 7 and the nibble
    below is 3, so a top nibble of 7 with an incoming carry (d[63] = 8) needs a value >= 0x78 16^62 > r.
    Such values are kept apart, for the restatement alone (RAW_ONLY); the device reduces every scalar
    before it takes digits (k_scalars_w8, k_lagrange, k_blind_assemble), so it sees k mod r.

LAYOUTS (trace()).  Per base the table build is P, dbl, +P ... 8P (table_build()).  The walk of a lane,
pair or group over its bases in index order, win = 64 .. 0: four doublings, skipped while the accumulator
is the identity, then one addition of digit x base per base; zero digits and identity multiples skipped.
    lane     k_prep_sigg2_var (straus_g1lz_lane, NG = 1): one chain, then + X~
    pair     k_prep_sigg1_var (straus_g2lz_pair, NG = 1): the same in G2
    wide16   k_prep_sigg2_var_wide: base k to group k mod 16, full additions of Jacobian entries, the
             jg_group_sum butterfly (group distance 1, 2, 4, 8, lower group first), then + X~
    wide8    k_prep_sigg1_var_wide: 8 groups of pairs, jl_group_sum
    lanes16  k_msm_straus<Fp, 16>: base k to lane k mod 16, lane_group_sum (distance 8, 4, 2, 1)
    pairsG   k_msm_straus_g2lz_g: base k to pair k mod G, G = straus_pairs(t); pair 0 adds the others'
             sums serially, acc + o_1 + ... + o_{G-1}; a pair with no base contributes the identity
A chain addition takes one of CHAIN (fresh, general, doubling, to-identity, from-identity), a join one of
JOIN (left-identity, right-identity, general, doubling, to-identity), as in fixed_edges.

CASES.  Related bases are made from the scalars' digits: steer() walks a lane up to the first addition
of base j and sets P_j = +-acc / d, so that addition is a doubling, or goes to the identity and the next
one starts from it (and the following window's doublings are skipped).  steer_sum() makes one lane's sum
equal or opposite to another's, so their join is a doubling or the identity.  This works for any scalars,
Lagrange coefficients included.
"""
import ctypes
import functools
import json
import math
import os
import random
import re

import fixed_edges as F
from fixed_edges import (CHAIN, G1_GENERATOR, G1_IDENTITY, G2_GENERATOR, G2_IDENTITY, JOIN, R, Chain, be48,  # noqa: F401
                         join)

ORDER = {1: 3, 2: 13}  # the order of each group's small-order base
M = 3 * 13 * R


def _crt_unit(m):
    """1 mod m, 0 mod M / m"""
    return (M // m) * pow(M // m, -1, m) % M


GEN = _crt_unit(R)  # the generator: 1 mod r, 0 mod 39
TORSION = {ell: _crt_unit(ell) for ell in ORDER.values()}  # the base of order ell: 1 mod ell, 0 mod M / ell
T3, T13 = TORSION[3], TORSION[13]  # (0, 2) in G1; T13 of tests/golden/torsion.json in G2
G1_ORDER3 = b"\x04" + bytes(48) + (2).to_bytes(48, "big")
G1_ORDER3_NEG = b"\x04" + bytes(48) + (F.P - 2).to_bytes(48, "big")


@functools.lru_cache(maxsize=None)
def g2_order13():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "torsion.json")) as f:
        return next(bytes.fromhex(r["point"]) for r in json.load(f)["G2"] if r["name"] == "T13")
HLOG = random.Random(0xC0C0).randrange(1 << 250, R)  # stands in for the unknown logarithm of a hashed point
WALK = "skipped-doublings"


def sub(a):
    """a G as a point"""
    return a % R * GEN % M


def _wide_ng():
    """Lane groups of the one-wave kernels from curve_wide_lz.h wide::G: 64 / G in G1, 32 / G pairs in G2."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "coconut-rust_amd", "csrc",
                       "curve_wide_lz.h")
    with open(src) as f:
        g = int(re.search(r"constexpr int G = (\d+);", f.read()).group(1))
    return {0: 64 // g, 1: 32 // g}


WIDE_NG = _wide_ng()
assert WIDE_NG == F.NGROUPS, (WIDE_NG, F.NGROUPS)
NPARTS = {"lane": 1, "pair": 1, "wide16": WIDE_NG[0], "wide8": WIDE_NG[1], "lanes16": 16}
G1_LAYOUTS = ("lane", "wide16", "lanes16")
LAYOUTS = ("lane", "pair", "wide16", "wide8", "lanes16", "pairsG")
HAS_JOIN = ("wide16", "wide8", "lanes16", "pairsG")


# ---------------------------------------------------------------- digits
def recode_w4(k):
    """straus.h recode_w4 on a raw 256-bit value: 65 signed digits, least significant first."""
    assert 0 <= k < 1 << 256
    d, carry = [], 0
    for w in range(64):
        v = ((k >> (4 * w)) & 0xF) + carry
        carry = int(v > 8)
        d.append(v - 16 * carry)
    d.append(carry)
    return d


def digits(m):
    """The digits the device takes of an encoded scalar: reduced mod r first."""
    return recode_w4(m % R)


RAW_ONLY = (0x79 << 248, (0x78 << 248) | (9 << 244), int("7" + "9" * 63, 16))  # d[63] = 8: all >= r


def edge_scalars():
    """Encoded scalars (some non-canonical) on the edges of recode_w4."""
    out = [0, 1, 7, 8, 9, 15, 16, int("8" * 64, 16), int("8" * 63, 16), int("F" * 63, 16), R - 1, R - 2, (R - 1) // 2,
           int("6" + "F" * 63, 16), int("7" + "0" * 62 + "9", 16), int("9" * 63, 16), int("7" * 63, 16) + 1,
           0x73 << 248, (0x73 << 248) | int("8" * 60, 16)]
    out += [d << (4 * w) for w in (0, 31, 63) for d in (8, 9)]  # (window 63: >= r, taken mod r)
    out += [3, 5, 6, R - 3]  # on an order-3 base: identity multiples and the doubling-branch entry
    out += [R, R + 5, (1 << 256) - 1, (1 << 384) - 1]
    return out


def lagrange(ids):
    """Lagrange basis at 0 over distinct ids (aggregate.hip k_lagrange, oracle oc_lagrange)."""
    assert len(set(ids)) == len(ids)
    out = []
    for a in ids:
        num = den = 1
        for b in ids:
            if b != a:
                num, den = num * b % R, den * (b - a) % R
        out.append(num * pow(den, -1, R) % R)
    return out


def straus_pairs_launch(t, ntask, cus=256):
    """aggregate.hip cck_msm_straus restated: lane pairs per task for a launch."""
    slots = cus * 4 * 2
    G, best = 0, 0.0
    for c in range(4, 17):
        per = ((t + c - 1) // c) * 73.0 + 143.0
        tb = 256 // (2 * c)
        waves = ((ntask + tb - 1) // tb) * ((2 * c * tb + 63) // 64)
        est = per * math.ceil(waves / slots)
        if not G or est < best:
            G, best = c, est
    return G


def straus_pairs(t):
    """G for launches of <= 64 tasks (one round of wave slots on any device of >= 32 CUs): the first c in
    4 .. 16 that minimises ceil(t / c)."""
    return min(range(4, 17), key=lambda c: ((t + c - 1) // c, c))


# ---------------------------------------------------------------- the model
def partition(layout, t):
    n = straus_pairs(t) if layout == "pairsG" else NPARTS[layout]
    return [list(range(p, t, n)) for p in range(n)]


def table_build(log):
    """Branches of the mixed additions 2P + P ... 7P + P (after P and dbl); none for an identity base."""
    if log % M == 0:
        return []
    c = Chain(2 * log, M)
    for _ in range(3, 9):
        c.add(log)
    return c.log


def walk(terms, stop_at=None):
    """One lane's 65 windows over terms [(log, digits)].  Returns (Chain, skipped doubling rounds in
    mid-walk); with stop_at = j: (accumulator, digit) at the first addition of term j, or None."""
    c, skipped = Chain(0, M), 0
    for win in range(64, -1, -1):
        if win != 64:
            if c.acc:
                c.acc = c.acc * 16 % M
            elif c.seen:
                skipped += 1
        for j, (log, dg) in enumerate(terms):
            d = dg[win]
            if not d:
                continue
            if j == stop_at:
                return c.acc, d
            if d * log % M:
                c.add(d * log)
    return None if stop_at is not None else (c, skipped)


def butterfly_stage(vals, m, log):
    """One butterfly stage at distance m: both partners get lower + upper (the lower one is the left operand)."""
    new = list(vals)
    for g in range(len(vals)):
        if not g & m:
            new[g] = new[g | m] = join(vals[g], vals[g | m], log, M)
    return new


def _butterfly(vals, dists, log):
    for m in dists:
        vals = butterfly_stage(vals, m, log)
    return vals[0]


def trace(layout, logs, scalars, xlog=None):
    """dict(build, chain, join, walk, final) for sum scalars_k P_k (+ X~ where xlog is given)."""
    t = len(logs)
    dg = [digits(s) for s in scalars]
    build = [b for k in range(t) for b in table_build(logs[k])]
    chain, jn, sums, skipped = [], [], [], 0
    last = None
    for part in partition(layout, t):
        last, sk = walk([(logs[k], dg[k]) for k in part])
        chain += last.log
        sums.append(last.acc)
        skipped += sk
    if layout in ("lane", "pair"):
        total = sums[0]
    elif layout in ("wide16", "wide8"):
        total = _butterfly(sums, [1 << i for i in range(len(sums).bit_length() - 1)], jn)
    elif layout == "lanes16":
        total = _butterfly(sums, [8, 4, 2, 1], jn)
    else:
        total = sums[0]
        for o in sums[1:]:
            total = join(total, o, jn, M)
    if xlog is not None and xlog % M:
        cx = Chain(total, M)
        cx.seen = bool(chain)
        cx.add(xlog)
        chain += cx.log
        total = cx.acc
    return dict(build=build, chain=chain, join=jn, walk=[WALK] * skipped, final=total)


def expected(logs, scalars, xlog=None):
    return (sum((s % R) * p for s, p in zip(scalars, logs)) + (xlog or 0)) % M


def steer(layout, logs, scalars, j, sign):
    """A log for base j whose first addition meets sign x the accumulator (None if that is empty)."""
    part = next(p for p in partition(layout, len(logs)) if j in p)
    hit = walk([(logs[k], digits(scalars[k])) for k in part], stop_at=part.index(j))
    if not hit or not hit[0] or hit[0] % (M // R):
        return None
    return sub(sign * hit[0] * pow(hit[1], -1, R))


def steer_sum(logs, scalars, part, j, target):
    """A log for base j of `part` so that the part's sum is `target` (a subgroup point)."""
    rest = sum((scalars[k] % R) * logs[k] for k in part if k != j) % M
    if rest % (M // R) or target % (M // R) or not scalars[j] % R:
        return None
    return sub((target - rest) * pow(scalars[j] % R, -1, R))


# ---------------------------------------------------------------- cases of one MSM
def msm_cases(layout, scalars, seed, opaque=None, with_x=False):
    """[dict(name, logs, xlog, off (indices encoded off-curve), reach [(where, branch)])] for fixed scalars.
    opaque: {index: stand-in log} of bases the caller cannot choose (a hashed point); their lanes take no
    part in any steering."""
    t, g1 = len(scalars), layout in G1_LAYOUTS
    ell = ORDER[1 if g1 else 2]
    tors = TORSION[ell]
    opaque = opaque or {}
    rng = random.Random(seed)
    rnd = lambda: sub(rng.randrange(1 << 200, R))  # noqa: E731
    base = [opaque.get(k) or rnd() for k in range(t)]
    x0 = rnd() if with_x else None
    parts = [p for p in partition(layout, t) if p]
    usable = [p for p in parts if not set(p) & set(opaque) and all(scalars[k] % R for k in p)]
    cases = []

    def case(name, logs, reach, xlog=x0, off=()):
        cases.append(dict(name=name, logs=list(logs), xlog=xlog, off=tuple(off), reach=list(reach)))

    def with_(k, v, src=None):
        out = list(src or base)
        out[k] = v
        return out

    case("random", base, [("chain", "fresh")])
    two = next((p for p in usable if len(p) >= 2), None)
    if two:
        for name, sign, br in (("chain_doubling", 1, "doubling"), ("chain_cancel", -1, "to-identity")):
            # the base to relate: one whose first addition finds the accumulator occupied; for the cancellation
            # preferably above window 0, so that a round of doublings meets the identity in mid-walk
            cand = [with_(j, v) for j in reversed(two) for v in [steer(layout, base, scalars, j, sign)] if v is not None]
            logs = next((c for c in cand if sign < 0 and trace(layout, c, scalars, x0)["walk"]), cand[0])
            tr = trace(layout, logs, scalars, x0)
            case(name, logs, [("chain", br)] + [(w, b) for w, b in (("chain", "from-identity"), ("walk", WALK))
                                                if sign < 0 and b in tr[w]])
    if layout in HAS_JOIN:
        for name, sign, br in (("join_equal", 1, "doubling"), ("join_opposite", -1, "to-identity")):
            done = False
            for A in usable:
                for B in usable:
                    if A is B or done or A[0] > B[0]:
                        continue
                    tgt = sign * sum((scalars[k] % R) * base[k] for k in A) % M
                    v = steer_sum(base, scalars, B, B[-1], tgt)
                    if v is not None and br in trace(layout, with_(B[-1], v), scalars, x0)["join"]:
                        case(name, with_(B[-1], v), [("join", br)])
                        done = True
        free = [p for p in parts if not set(p) & set(opaque)]
        if free and len(parts) > 1:
            logs = list(base)
            for k in free[0]:
                logs[k] = 0
            if "left-identity" in trace(layout, logs, scalars, x0)["join"] and any(logs):
                case("first_lane_absent", logs, [("join", "left-identity")])
            logs = list(base)
            for k in free[-1]:
                logs[k] = 0
            case("last_lane_absent", logs, [("join", "right-identity")])
    longest = max((p for p in parts if not set(p) & set(opaque)), key=len, default=None)
    if longest:
        where = sorted({0, len(longest) // 2, len(longest) - 1})
        for n, i in enumerate(where):
            k = longest[i]
            case(f"identity_base_{('first', 'middle', 'last')[n] if len(where) == 3 else i}", with_(k, 0), [],
                 off=[k] if n % 2 else [])
        # the group's small-order base (order 3 in G1, 13 in G2): in G1 its table build 2 T .. 8 T meets the
        # identity twice and the doubling branch; an order-13 base's meets nothing (8 < 12)
        case(f"order{ell}_first", with_(longest[0], tors), [("build", "to-identity"), ("build", "from-identity"),
                                                            ("build", "doubling")] if g1 else [])
        case(f"order{ell}_neg_last", with_(longest[-1], (ell - 1) * tors), [("build", "doubling")] if g1 else [])
    allz = [0 if k not in opaque else base[k] for k in range(t)]
    case("all_identity", allz, [], off=[k for k in range(1, t, 2) if k not in opaque])
    case(f"all_order{ell}", [tors if k not in opaque else base[k] for k in range(t)],
         [("build", "to-identity")] if g1 else [])
    if with_x:
        s = expected(base, scalars)
        case("x_identity", base, [], xlog=0)
        if s:
            case("x_cancels", base, [("chain", "to-identity")], xlog=M - s)
            case("x_equal", base, [("chain", "doubling")], xlog=s)
        case("x_only", allz, [("chain", "fresh")])
        case(f"x_order{ell}", base, [("chain", "general")], xlog=tors)
    return cases


# ---------------------------------------------------------------- Signature::verify, a verkey per credential
VERIFY_LAYOUTS = {0: ("lane", "wide16"), 1: ("pair", "wide8")}
VERIFY_Q = (3, 18)


@functools.lru_cache(maxsize=None)
def verify_cases(mode, q):
    """[dict(name, msgs, logs (Y~_j), xlog, off, reach [(layout, where, branch)])]; shared, not to be
    modified.  Every edge scalar on an otherwise random credential, then msm_cases() steered for each of the
    mode's two layouts (a steering is specific to the layout whose accumulator it reads)."""
    rng = random.Random(9100 + 10 * q + mode)
    fr = lambda: rng.randrange(1 << 250, R)  # noqa: E731
    out = []
    for i, e in enumerate(edge_scalars()):
        msgs = [fr() for _ in range(q)]
        msgs[i % q] = e
        out.append(dict(name=f"edge_{i}_{e % R:x}"[:40], msgs=msgs, logs=[sub(fr()) for _ in range(q)], xlog=sub(fr()),
                        off=(), reach=[]))
    for lay in VERIFY_LAYOUTS[mode]:
        msgs = [fr() for _ in range(q)]
        msgs[0], msgs[q - 1] = 5, 6  # on an order-3 base: 5 T from the doubling branch, 6 T the identity
        for c in msm_cases(lay, msgs, 77 + q + mode, with_x=True):
            out.append(dict(name=f"{lay}/{c['name']}", msgs=msgs, logs=c["logs"], xlog=c["xlog"], off=c["off"],
                            reach=[(lay, w, b) for w, b in c["reach"]]))
    return out


def verify_gk(mode, q):
    return random.Random(4400 + 10 * q + mode).randrange(1 << 200, R)


# ---------------------------------------------------------------- aggregation (Lagrange scalars)
AGG_T = (1, 2, 3, 5, 17, 33)
SIG_LAYOUT = {0: "pairsG", 1: "lanes16"}  # the signature group's MSM: Signature::aggregate, blind signing
VK_LAYOUT = {0: "lanes16", 1: "pairsG"}  # the other group's: Verkey::aggregate


def id_sets(t):
    """Two id rows of t + 1 entries: 1 .. t + 1 (t = 2: Lagrange scalars 2 and r - 1), and, of 24 random
    candidates, the one whose Lagrange scalars have the most digits 8."""
    rng = random.Random(500 + t)
    cands = [rng.sample(range(1, 1 << 20), t + 1) for _ in range(24)]
    best = max(cands, key=lambda ids: sum(d == 8 for s in lagrange(ids[:t]) for d in digits(s)))
    return [list(range(1, t + 2)), best]


@functools.lru_cache(maxsize=None)
def agg_rows(layout, t):
    """[dict(name, ids (t + 1), scalars (t), logs (t + 1: the last entry is not used), off, reach)]"""
    rows = []
    for v, ids in enumerate(id_sets(t)):
        sc = lagrange(ids[:t])
        rng = random.Random(31 * t + v)
        for c in msm_cases(layout, sc, 1000 * t + v):
            rows.append(dict(name=f"ids{v}/{c['name']}", ids=ids, scalars=sc, off=c["off"], reach=c["reach"],
                             logs=c["logs"] + [sub(rng.randrange(1 << 200, R))]))
    assert len(rows) <= 64  # one round of wave slots: G depends on t alone
    return rows


@functools.lru_cache(maxsize=None)
def vkagg_rows(mode, t):
    """Verkey::aggregate with q = 2: X~ takes row i's bases, Y~_1 row i + 1's (same ids, so the same
    scalars), Y~_0 random ones: the three MSMs of a row differ per column.  3 n <= 64 tasks."""
    rows = [r for r in agg_rows(VK_LAYOUT[mode], t) if r["name"].startswith("ids1/")][:21]
    rng = random.Random(77 * t + mode)
    out = []
    for i, r in enumerate(rows):
        y1 = rows[(i + 1) % len(rows)]
        out.append(dict(name=r["name"], ids=r["ids"], scalars=r["scalars"], X=r, Y1=y1,
                        Y0=[sub(rng.randrange(1 << 200, R)) for _ in range(t + 1)]))
    return out


# ---------------------------------------------------------------- blind signing
BLIND_K = (2, 17)


@functools.lru_cache(maxsize=None)
def blind_sets(mode, k):
    """[dict(y (k + 1 encoded), x, requests [dict(name, a, b (cases of msm_cases), known, e)])]: one call a
    y vector.  q = k + 1: one known message m, e = x + y_k m; the last request has e = 0.  c~1 = sum y_i a_i
    + 0 h, c~2 = sum y_i b_i + e h; h is a hashed point, HLOG in the model."""
    lay = SIG_LAYOUT[mode]
    es = [e for e in edge_scalars() if e % R]  # (a zero y_i is in the list as R)
    es = es + [0] + es
    rng = random.Random(60 + k + mode)
    calls = []
    for c in range(2 if k > 2 else 3):
        y = [es[(c * (k if k > 2 else 7) + i) % len(es)] for i in range(k)] + [rng.randrange(1 << 250, R)]
        x = rng.randrange(1 << 250, R)
        m = rng.randrange(1 << 250, R)
        m0 = (R - x) * pow(y[k], -1, R) % R
        e = (x + y[k] * m) % R
        A = msm_cases(lay, y[:k] + [0], 300 + c, opaque={k: sub(HLOG)})
        B = msm_cases(lay, y[:k] + [e], 400 + c, opaque={k: sub(HLOG)})
        B0 = msm_cases(lay, y[:k] + [0], 500 + c, opaque={k: sub(HLOG)})
        n = min(max(len(A), len(B)), 30)
        reqs = [dict(name=f"{A[i % len(A)]['name']}+{B[(i + 3) % len(B)]['name']}", a=A[i % len(A)],
                     b=B[(i + 3) % len(B)], known=m, e=e) for i in range(n)]
        reqs.append(dict(name="e_zero", a=A[0], b=B0[1 % len(B0)], known=m0, e=0))
        assert 2 * len(reqs) <= 64
        calls.append(dict(y=y, x=x, requests=reqs))
    return calls


# ---------------------------------------------------------------- points and expectations from the oracle
def _sz(n):
    return ctypes.c_size_t(n)


def msm(oc, group, pts, scalars):
    """oc_msm over encoded points and encoded (possibly non-canonical) scalars."""
    eb = 97 if group == 1 else 192
    out = ctypes.create_string_buffer(eb)
    oc.oc_msm(group, _sz(len(scalars)), pts, b"".join(be48(s) for s in scalars), out)
    return out.raw


def point_bytes(oc, group, vals, off=()):
    """Encodings of points given as integers mod M = 39 r (of `group`: no part of the other group's small
    order); index in `off`: an off-curve encoding (it decodes to
    the identity) where the point is the identity."""
    eb = 97 if group == 1 else 192
    ident = G1_IDENTITY if group == 1 else G2_IDENTITY
    raw = F.gen_mul(oc, group, [v % R for v in vals])
    out = []
    for i, v in enumerate(vals):
        p, b = raw[eb * i:eb * (i + 1)], v % ORDER[group]
        assert v % (M // R) == _crt_unit(ORDER[group]) * b % (M // R), "the other group's small-order part"
        if b:
            t = g2_order13() if group == 2 else G1_ORDER3
            p = msm(oc, group, t, [b]) if v % R == 0 else msm(oc, group, p + t, [1, b])
        elif v % R == 0:
            p = ident
            if i in off:
                g = bytearray(G1_GENERATOR if group == 1 else G2_GENERATOR)
                g[-1] ^= 1
                p = bytes(g)
        out.append(p)
    return b"".join(out)


def verify_batch_inputs(oc, mode, q):
    """Every case of verify_cases() as a credential and its twin with sigma_2 off by G.  pr = X~ + sum m_j
    Y~_j = s g~; sigma = (k G, k s G).  Valid iff s != 0: an order-3 part b T of pr pairs to
    one (e(P, T) has order dividing both 3 and r), so it changes neither verdict nor GT.  In SigG1 pr is the
    Miller loop's Q side: with an order-13 part it is a point of order 13 r (or 13), on which the loop's value is
    no pairing; the oracle rejects every such credential (expect 0; the GT bytes still pin the MSM's point,
    its order-13 part included).
    Returns dict(names, n, s1, s2, msgs, X, Y, g, expect)."""
    og, sg = (1, 2) if mode == 0 else (2, 1)
    gk = verify_gk(mode, q)
    rng = random.Random(17 + mode + q)
    e1, e2, names, expect, mb, xs, ys, offs = [], [], [], [], [], [], [], []
    for c in verify_cases(mode, q):
        pr = expected(c["logs"], c["msgs"], c["xlog"])
        s = pr % R * pow(gk, -1, R) % R
        k = rng.randrange(1 << 250, R)
        for bad in (0, 1):
            e1.append(k)
            e2.append(k * s + bad)
            names.append(c["name"] + ("/off_by_g" if bad else "/valid"))
            expect.append(int(not bad and s != 0 and pr % 13 == 0))
            mb.append(b"".join(be48(m) for m in c["msgs"]))
            base = len(ys)
            offs += [base + j for j in c["off"]]
            ys += c["logs"]
            xs.append(c["xlog"])
    return dict(names=names, n=len(names), s1=F.gen_mul(oc, sg, e1), s2=F.gen_mul(oc, sg, e2), msgs=b"".join(mb),
                X=point_bytes(oc, og, xs), Y=point_bytes(oc, og, ys, offs), g=F.gen_mul(oc, og, [gk]), expect=expect)


def oracle_verify(oc, mode, q, b, nthreads=8):
    """(verdicts, GT bytes) of oc_verify_batch with a verkey per credential."""
    n = b["n"]
    ver = ctypes.create_string_buffer(n)
    gts = ctypes.create_string_buffer(576 * n)
    oc.oc_verify_batch(mode, _sz(n), _sz(q), b["s1"], b["s2"], b["msgs"], b["X"], b["Y"], 1, b["g"], ver, gts, nthreads)
    return list(ver.raw), gts.raw


def agg_inputs(oc, group, rows):
    """(ids flat, points n x (t + 1) encoded) of agg_rows()."""
    ids = [i for r in rows for i in r["ids"]]
    vals, offs = [], []
    for r in rows:
        offs += [len(vals) + j for j in r["off"]]
        vals += r["logs"]
    return ids, point_bytes(oc, group, vals, offs)


def oracle_sig_aggregate(oc, mode, t, ids, s1, s2):
    """oc_signature_aggregate for one row of t + 1 entries: (sigma_1, sigma_2) out."""
    sb = 192 if mode == 0 else 97
    o1, o2 = ctypes.create_string_buffer(sb), ctypes.create_string_buffer(sb)
    assert oc.oc_signature_aggregate(mode, _sz(t + 1), _sz(t), (ctypes.c_uint64 * (t + 1))(*ids), s1, s2, o1, o2) == 0
    return o1.raw, o2.raw


def oracle_vk_aggregate(oc, mode, t, q, ids, X, Y):
    ob = 97 if mode == 0 else 192
    oX, oY = ctypes.create_string_buffer(ob), ctypes.create_string_buffer(ob * q)
    assert oc.oc_verkey_aggregate(mode, _sz(t + 1), _sz(t), _sz(q), (ctypes.c_uint64 * (t + 1))(*ids), X, Y, oX, oY) == 0
    return oX.raw, oY.raw


def vkagg_inputs(oc, mode, rows):
    """(ids flat, X n x (t + 1), Y n x (t + 1) x 2) of vkagg_rows(): Y is [row][signer][column]."""
    og = 1 if mode == 0 else 2
    ids = [i for r in rows for i in r["ids"]]
    xv, xo, yv, yo = [], [], [], []
    for r in rows:
        xo += [len(xv) + j for j in r["X"]["off"]]
        xv += r["X"]["logs"]
        for s in range(len(r["Y0"])):
            if s in r["Y1"]["off"]:
                yo.append(len(yv) + 1)
            yv += [r["Y0"][s], r["Y1"]["logs"][s]]
    return ids, point_bytes(oc, og, xv, xo), point_bytes(oc, og, yv, yo)
