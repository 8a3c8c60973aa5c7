"""Inputs and the oracle's expected bytes for the keygen entry points (cc_keygen_deal_batch,
cc_keygen_combine_batch), built at test time and cached per process.  TEST INFRASTRUCTURE ONLY.

The main shapes come from the oracle itself: oracle.keygen.pedersen_deal (t coefficients of f, then t of f',
per polynomial) and oracle.coconut_ref.get_shared_secret, each fed a Drbg; the device inputs are rebuilt
from a second Drbg with the same seed, so the bytes can be compared.  The edge cases (scalars >= r, related
and undecodable bases, the combine) have no oracle generator; restate_deal / restate_combine restate them
over the oracle's curve classes, and tests/test_keygen_deal_model.py ties the restatement to pedersen_deal
on the main shapes.

The commitments, the shares and the Pedersen generators g, h are in G1 in both group modes; only g~ and the
verkeys depend on the mode.  Everything mode-independent is computed once.
"""
import functools

from oracle import bls12_381 as B
from oracle import coconut_ref as C
from oracle import keygen as K

R, P = B.R, B.P
MODES = {"G2": 0, "G1": 1}
SHAPES = ((1, 1, 0), (1, 3, 1), (2, 2, 2), (3, 5, 7), (33, 40, 1))  # (t, total, q); (3, 5, 7): the reference's
M3_SHAPES = SHAPES[:3]  # also dealt three at a time, over distinct coefficients
EDGE_SCALARS = (0, 1, R - 1, R, R + 1, (1 << 384) - 1)
# single bits on both sides of every window boundary of the 8-bit and 13-bit tables, and the top bit below r
EDGE_BITS = tuple(sorted({b for k in range(1, 32) for b in (8 * k - 1, 8 * k)} |
                         {b for k in range(1, 20) for b in (13 * k - 1, 13 * k)} | {254}))
G1_ID = B.g1_to_bytes(None)


def be48(v):
    return int(v).to_bytes(48, "big")


def oth(mode):
    """OtherGroup of a mode: (curve, to_bytes, from_bytes, encoding bytes)."""
    return (B.G1, B.g1_to_bytes, B.g1_from_bytes, 97) if mode == "G2" else (B.G2, B.g2_to_bytes, B.g2_from_bytes, 192)


@functools.lru_cache(None)
def bases():
    """(g, h, {mode: g~}) as points: known multiples of the generators."""
    rng = C.Drbg("keygen-deal-bases")
    g, h = B.G1.mul(B.G1.gen, rng.fr()), B.G1.mul(B.G1.gen, rng.fr())
    return g, h, {"G2": B.G1.mul(B.G1.gen, rng.fr()), "G1": B.G2.mul(B.G2.gen, rng.fr())}


def base_bytes(mode):
    g, h, gt = bases()
    return oth(mode)[1](gt[mode]), B.g1_to_bytes(g), B.g1_to_bytes(h)


@functools.lru_cache(None)
def _g1_mul(pt, k):
    return B.G1.mul(pt, k)


@functools.lru_cache(None)
def _gt_mul(mode, gt, k):
    return oth(mode)[0].mul(gt, k)


def poly(c, x):
    acc = 0
    for a in reversed(c):
        acc = (acc * x + a) % R
    return acc


# ---------------------------------------------------------------- the restatement
def restate_deal(t, total, q, m, cf, ct, g, h):
    """cf, ct: m (q + 1) t integers (any size below 2^384; ct None for Shamir), g, h points or None.
    Returns the mode-independent outputs as integers / points: x[m][total], y[m][total][q], xt, yt, comm."""
    out = {"x": [], "y": [], "xt": [], "yt": [], "comm": []}
    for k in range(m):
        c = [[v % R for v in cf[(k * (q + 1) + p) * t:(k * (q + 1) + p + 1) * t]] for p in range(q + 1)]
        out["x"].append([poly(c[0], i) for i in range(1, total + 1)])
        out["y"].append([[poly(c[1 + j], i) for j in range(q)] for i in range(1, total + 1)])
        if ct is not None:
            b = [[v % R for v in ct[(k * (q + 1) + p) * t:(k * (q + 1) + p + 1) * t]] for p in range(q + 1)]
            out["xt"].append([poly(b[0], i) for i in range(1, total + 1)])
            out["yt"].append([[poly(b[1 + j], i) for j in range(q)] for i in range(1, total + 1)])
            out["comm"] += [B.G1.add(_g1_mul(g, a), _g1_mul(h, bb)) for p in range(q + 1) for a, bb in zip(c[p], b[p])]
    return out


def pack(vals, mode=None, gt=None):
    """The byte layouts of the header from restate_deal's integers / points; with a mode, X and Y too."""
    flat = lambda rows: b"".join(be48(v) for row in rows for v in row)  # noqa: E731
    o = {"x": flat(vals["x"]), "y": b"".join(be48(v) for kg in vals["y"] for row in kg for v in row)}
    if vals["xt"]:
        o["xt"] = flat(vals["xt"])
        o["yt"] = b"".join(be48(v) for kg in vals["yt"] for row in kg for v in row)
        o["comm"] = b"".join(B.g1_to_bytes(c) for c in vals["comm"])
    if mode is not None:
        enc = oth(mode)[1]
        o["X"] = b"".join(enc(_gt_mul(mode, gt, v)) for row in vals["x"] for v in row)
        o["Y"] = b"".join(enc(_gt_mul(mode, gt, v)) for kg in vals["y"] for row in kg for v in row)
    return o


def verkeys(mode, vals, gt="default"):
    """X, Y bytes of a case under the mode's g~ (or the point given; None: the identity)."""
    gt = bases()[2][mode] if gt == "default" else gt
    o = pack(vals, mode, gt)
    return o["X"], o["Y"]


def coeff_bytes(ints):
    return b"".join(be48(v) for v in ints)


# ---------------------------------------------------------------- main shapes, from the oracle's generators
@functools.lru_cache(None)
def pedersen_case(shape, m):
    """m keygens dealt by oracle.keygen.pedersen_deal, polynomial after polynomial, from one Drbg; the
    coefficients rebuilt from a second Drbg with the same seed."""
    t, total, q = shape
    g, h, _ = bases()
    seed = "keygen-deal-pedersen-%d-%d-%d" % shape
    rng, twin = C.Drbg(seed), C.Drbg(seed)
    cf, ct = [], []
    vals = {"x": [], "y": [], "xt": [], "yt": [], "comm": []}
    secrets = []
    for _ in range(m):
        deals = [K.pedersen_deal(t, total, g, h, rng) for _ in range(q + 1)]
        for _ in range(q + 1):
            cf += [twin.fr() for _ in range(t)]
            ct += [twin.fr() for _ in range(t)]
        secrets.append([(d[0], d[1]) for d in deals])
        sh = [d[3] for d in deals]
        vals["x"].append([sh[0][i][0] for i in range(1, total + 1)])
        vals["xt"].append([sh[0][i][1] for i in range(1, total + 1)])
        vals["y"].append([[sh[1 + j][i][0] for j in range(q)] for i in range(1, total + 1)])
        vals["yt"].append([[sh[1 + j][i][1] for j in range(q)] for i in range(1, total + 1)])
        vals["comm"] += [c for d in deals for c in d[2]]
    return {"shape": shape, "m": m, "cf": cf, "ct": ct, "vals": vals, "secrets": secrets}


@functools.lru_cache(None)
def shamir_case(shape):
    """One keygen by oracle.coconut_ref.get_shared_secret per polynomial (trusted_party_sss_keygen's order)."""
    t, total, q = shape
    seed = "keygen-deal-shamir-%d-%d-%d" % shape
    rng, twin = C.Drbg(seed), C.Drbg(seed)
    got = [C.get_shared_secret(t, total, rng) for _ in range(q + 1)]
    cf = [twin.fr() for _ in range((q + 1) * t)]
    vals = {"x": [[got[0][1][i] for i in range(1, total + 1)]],
            "y": [[[got[1 + j][1][i] for j in range(q)] for i in range(1, total + 1)]], "xt": [], "yt": [], "comm": []}
    return {"shape": shape, "m": 1, "cf": cf, "ct": None, "vals": vals, "secrets": [[(s, None) for s, _ in got]]}


def first_keygen(case):
    """The m = 1 case made of a case's first keygen."""
    t, total, q = case["shape"]
    n = (q + 1) * t
    v = case["vals"]
    vals = {k: v[k][:1] for k in ("x", "y", "xt", "yt")}
    vals["comm"] = v["comm"][:n]
    return {"shape": case["shape"], "m": 1, "cf": case["cf"][:n], "ct": None if case["ct"] is None else case["ct"][:n],
            "vals": vals, "secrets": case["secrets"][:1]}


def cycled(case, m):
    """m keygens that repeat a case's keygens in turn (period = the case's m): the oracle's bytes at every
    position of a batch that spans several blocks, at the oracle cost of the pool."""
    t, total, q = case["shape"]
    n, pm, v = (q + 1) * t, case["m"], case["vals"]
    idx = [k % pm for k in range(m)]
    vals = {key: [v[key][i] for i in idx] for key in ("x", "y", "xt", "yt")}
    vals["comm"] = [c for i in idx for c in v["comm"][i * n:(i + 1) * n]]
    return {"shape": case["shape"], "m": m, "cf": [c for i in idx for c in case["cf"][i * n:(i + 1) * n]],
            "ct": [c for i in idx for c in case["ct"][i * n:(i + 1) * n]], "vals": vals,
            "secrets": [case["secrets"][i] for i in idx]}


@functools.lru_cache(None)
def unit_pool():
    """Seven keygens of shape (1, 1, 0): one task each in all three task spaces.  7 is coprime to the block
    sizes, so a task that lands in another keygen's slot shows."""
    return pedersen_case((1, 1, 0), 7)


# ---------------------------------------------------------------- edge scalars
@functools.lru_cache(None)
def edge_unit_case():
    """Shape (1, 1, 0): every edge scalar and boundary bit as f_0 (so also as the share and the verkey's
    scalar) beside a small f'_0, the edge scalars as f'_0 beside a small f_0, and the zero patterns."""
    pairs = [(v, 1 + i % 5) for i, v in enumerate(EDGE_SCALARS + tuple(1 << b for b in EDGE_BITS))]
    pairs += [(2 + i, v) for i, v in enumerate(EDGE_SCALARS)]
    names = ["f=%#x" % a for a, _ in pairs[:len(EDGE_SCALARS) + len(EDGE_BITS)]] + ["f'=%#x" % b for _, b in pairs[-6:]]
    pairs += [(0, 0), (0, 5), (7, 0)]
    names += ["all_zero", "f_zero", "ft_zero"]
    g, h, _ = bases()
    cf, ct = [a for a, _ in pairs], [b for _, b in pairs]
    return {"shape": (1, 1, 0), "m": len(pairs), "cf": cf, "ct": ct, "names": names,
            "vals": restate_deal(1, 1, 0, len(pairs), cf, ct, g, h)}


@functools.lru_cache(None)
def edge_poly_case():
    """Shape (3, 3, 1), m = 3: the edge scalars as coefficients of every degree (Horner over values >= r),
    and a keygen whose polynomial 0 is all zero in f and f' and whose polynomial 1 has f = 0, f' != 0."""
    e = EDGE_SCALARS
    cf = [e[(i + 0) % 6] for i in range(6)] + [e[(i + 2) % 6] for i in range(6)] + [0] * 6
    ct = [e[(i + 3) % 6] for i in range(6)] + [e[(i + 5) % 6] for i in range(6)] + [0, 0, 0, 3, R - 2, 1 << 200]
    g, h, _ = bases()
    return {"shape": (3, 3, 1), "m": 3, "cf": cf, "ct": ct, "vals": restate_deal(3, 3, 1, 3, cf, ct, g, h)}


# ---------------------------------------------------------------- related bases: the exceptional additions
def window_trace(terms, wbits=8):
    """The walk of the commitment kernel over the window tables: terms [(base point, scalar)] in order, per
    base the windows from the lowest.  Returns (events, sum); an event is 'load' (the accumulator was the
    identity), 'add', 'double' (the entry equals the accumulator) or 'cancel' (it is its negative)."""
    acc, ev = None, []
    for pt, k in terms:
        k %= R
        if pt is None:
            continue
        for w in range((256 + wbits - 1) // wbits):
            d = (k >> (w * wbits)) & ((1 << wbits) - 1)
            if not d:
                continue
            e = _g1_mul(pt, d << (w * wbits))
            if e is None:
                continue
            ev.append("load" if acc is None else "double" if acc == e else "cancel" if acc == B.G1.neg(e) else "add")
            acc = B.G1.add(acc, e)
    return ev, acc


RELATED_V = 0xA5 << 16  # one nonzero 8-bit window
RELATED_U = 0x3C << 40  # a further one


@functools.lru_cache(None)
def related_cases():
    """[(name, h point, case, the events of each commitment at 8 bits)], shape (1, 1, 0)."""
    g = bases()[0]
    ng = B.G1.neg(g)
    out = []
    for name, h, pairs, want in (
            ("h_eq_g_doubles", g, [(RELATED_V, RELATED_V)], [["load", "double"]]),
            ("h_neg_g_cancels_and_restarts", ng, [(RELATED_V, RELATED_V), (RELATED_V, RELATED_V + RELATED_U)],
             [["load", "cancel"], ["load", "cancel", "load"]])):
        cf, ct = [a for a, _ in pairs], [b for _, b in pairs]
        case = {"shape": (1, 1, 0), "m": len(pairs), "cf": cf, "ct": ct,
                "vals": restate_deal(1, 1, 0, len(pairs), cf, ct, g, h)}
        out.append((name, h, case, want))
    return out


# ---------------------------------------------------------------- bases that do not decode
def g1_forms(pt):
    """[(name, encoding, what it decodes to)] for a G1 point."""
    enc = B.g1_to_bytes(pt)
    shifted = b"\x04" + be48(pt[0] + P) + be48(pt[1] + P)
    return [("identity", G1_ID, None), ("bad_prefix", b"\x03" + enc[1:], None),
            ("off_curve", enc[:-1] + bytes([enc[-1] ^ 1]), None), ("coord_ge_p", shifted, pt)]


def g2_forms(pt):
    enc = B.g2_to_bytes(pt)
    (xa, xb), (ya, yb) = pt
    shifted = be48(xa + P) + be48(xb + P) + be48(ya + P) + be48(yb + P)
    return [("identity", B.g2_to_bytes(None), None), ("off_curve", enc[:-1] + bytes([enc[-1] ^ 1]), None),
            ("coord_ge_p", shifted, pt)]


@functools.lru_cache(None)
def bad_base_inputs():
    rng = C.Drbg("keygen-deal-bad-bases")
    n = 2 * 2  # shape (2, 2, 1): (q + 1) t coefficients
    return [rng.fr() for _ in range(n)], [rng.fr() for _ in range(n)]


def bad_base_cases(mode):
    """[(name, g~ bytes, g bytes, h bytes, expected outputs)] at shape (2, 2, 1): each base in turn sent in
    every form; the other two stay valid.  The expectation decodes the encodings as the oracle does."""
    g, h, gts = bases()
    gt = gts[mode]
    gtb, gb, hb = base_bytes(mode)
    cf, ct = bad_base_inputs()
    out = []
    for which, forms in (("g", g1_forms(g)), ("h", g1_forms(h)), ("g_tilde", (g1_forms if mode == "G2" else g2_forms)(gt))):
        for name, enc, dec in forms:
            assert (B.g1_from_bytes if which != "g_tilde" else oth(mode)[2])(enc) == dec, (which, name)
            use = {"g": g, "h": h, "g_tilde": gt, which: dec}
            vals = restate_deal(2, 2, 1, 1, cf, ct, use["g"], use["h"])
            exp = pack(vals, mode, use["g_tilde"])
            sent = {"g": gb, "h": hb, "g_tilde": gtb, which: enc}
            out.append(("%s_%s" % (which, name), sent["g_tilde"], sent["g"], sent["h"], exp))
    return out


# ---------------------------------------------------------------- the combine
def restate_combine(m, d, q, t, total, ins):
    """ins: the byte buffers x, y, xt, yt, comm of m d keygens (xt, yt, comm may be absent).  The sums over
    the dealer axis as bytes, the combined shares as integers in 'xi' / 'yi' for the verkeys."""
    def fr_sum(buf, inner):
        v = [B.fr_from_bytes(buf[i * 48:(i + 1) * 48]) for i in range(m * d * inner)]
        return [sum(v[(g * d + dd) * inner + e] for dd in range(d)) % R for g in range(m) for e in range(inner)]
    out = {"xi": fr_sum(ins["x"], total), "yi": fr_sum(ins["y"], total * q)}
    out["x"], out["y"] = coeff_bytes(out["xi"]), coeff_bytes(out["yi"])
    if "comm" in ins:
        out["xt"], out["yt"] = coeff_bytes(fr_sum(ins["xt"], total)), coeff_bytes(fr_sum(ins["yt"], total * q))
        inner = (q + 1) * t
        pts = [B.g1_from_bytes(ins["comm"][i * 97:(i + 1) * 97]) for i in range(m * d * inner)]
        sums = []
        for g in range(m):
            for e in range(inner):
                acc = None
                for dd in range(d):
                    acc = B.G1.add(acc, pts[(g * d + dd) * inner + e])
                sums.append(acc)
        out["comm"] = b"".join(B.g1_to_bytes(s) for s in sums)
    return out


def combine_verkeys(mode, exp, total, q):
    gt, enc = bases()[2][mode], oth(mode)[1]
    return (b"".join(enc(_gt_mul(mode, gt, v)) for v in exp["xi"]), b"".join(enc(_gt_mul(mode, gt, v)) for v in exp["yi"]))


def _dealer_bytes(case, k):
    """Keygen k of a Pedersen case as the five input buffers of a combine."""
    t, total, q = case["shape"]
    v = case["vals"]
    one = {key: v[key][k:k + 1] for key in ("x", "y", "xt", "yt")}
    one["comm"] = v["comm"][k * (q + 1) * t:(k + 1) * (q + 1) * t]
    return pack(one)


def _negated(b):
    """A dealer with every coefficient negated: shares mod r and commitments."""
    neg_fr = lambda buf: b"".join(be48(-int.from_bytes(buf[i:i + 48], "big") % R) for i in range(0, len(buf), 48))  # noqa: E731
    out = {k: neg_fr(b[k]) for k in ("x", "y", "xt", "yt")}
    out["comm"] = b"".join(B.g1_to_bytes(B.G1.neg(B.g1_from_bytes(b["comm"][i:i + 97]))) for i in range(0, len(b["comm"]), 97))
    return out


def _join(dealers):
    return {k: b"".join(dl[k] for dl in dealers) for k in ("x", "y", "xt", "yt", "comm")}


@functools.lru_cache(None)
def combine_cases():
    """[(name, m, d, shape, inputs, expected, notes)]: the mode-independent part of every combine case."""
    big, small = pedersen_case((3, 5, 1), 5), pedersen_case((2, 2, 1), 4)
    D = [_dealer_bytes(small, k) for k in range(4)]
    N0 = _negated(D[0])
    bad = dict(D[1])
    c = bytearray(bad["comm"])
    c[0:97] = G1_ID                      # an identity commitment
    c[97 + 96] ^= 1                      # an off-curve one
    c[2 * 97] = 3                        # a bad prefix
    bad["comm"] = bytes(c)
    over = dict(D[0])
    over["x"] = b"".join(be48(int.from_bytes(D[0]["x"][i:i + 48], "big") + R) for i in range(0, len(D[0]["x"]), 48))
    over["yt"] = b"".join(be48(int.from_bytes(D[0]["yt"][i:i + 48], "big") + 3 * R)
                          for i in range(0, len(D[0]["yt"]), 48))
    cases = [("d1_identity_map", 1, 1, (2, 2, 1), [D[0]]),
             ("d5_dealers", 1, 5, (3, 5, 1), [_dealer_bytes(big, k) for k in range(5)]),
             ("two_equal_dealers", 1, 2, (2, 2, 1), [D[0], D[0]]),
             ("two_opposite_dealers", 1, 2, (2, 2, 1), [D[0], N0]),
             ("three_dealers_two_opposite", 1, 3, (2, 2, 1), [D[0], N0, D[1]]),
             ("identity_and_undecodable_commitments", 1, 2, (2, 2, 1), [D[0], bad]),
             ("shares_ge_r", 1, 2, (2, 2, 1), [over, D[1]]),
             ("two_groups", 2, 2, (2, 2, 1), [D[0], D[1], D[2], D[3]])]
    out = []
    for name, m, d, (t, total, q), dealers in cases:
        ins = _join(dealers)
        out.append((name, m, d, (t, total, q), ins, restate_combine(m, d, q, t, total, ins)))
    return out
