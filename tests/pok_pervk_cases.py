"""Proofs for PoKOfSignatureProof::verify with one verkey per proof (csrc/pok_pervk.hip,
cc_pok_verify_batch_pervk_device), every discrete logarithm known, each with its intended verdict, and a
model of the additions the prep's two chains make.

Plain Python over integers; points come from scalars through a `mul` function: the C oracle's
oc_gen_mul_mt (oracle_mul) or the product's fixed-base multiplication (gpu_mul, as
bench_modes.make_pok_batch builds its batches).  No expectation is taken from the code under test.

TWO KINDS OF LISTS.
  distinct_batch()  n proofs, proof i valid under ITS OWN verkey (x_i, y_i,j uniform), as ps_sig makes them
                    (sigma' = (r1 k G, r1 k (s + r2) G), J = (r2 + sum_hidden y_j m_j) g~, T = (b_0 +
                    sum_hidden y_j b_j) g~, responses b - chal * secret); every bad_every-th corrupted,
                    cycling KINDS: a response off by 5, a revealed message off by 1 (with nothing revealed:
                    sigma'_2 off by G), the proof made under the NEXT proof's key.
  edge lists        scalar_list / base_list / unrevealed_list: one steered or degenerate proof a case, three
                    ways (valid as built, g~'s response off by one, sigma'_2 off by G: its GT pins J').

POINTS of the edge lists are integers mod M = 39 r as in tests/straus_edges.py (a G + b T, T the group's
small-order base of order 3 in G1, 13 in G2), so equality, negation and the identity are the group's and a
scalar acts by integer multiplication mod r.  Any responses, challenge and revealed messages give a valid
proof once T = sum rho_k B_k + chal J and sigma'_2 = (log J' / log g~) sigma'_1.  One slot of a case may
instead hold an OPAQUE point: a small-order point of tests/golden/torsion.json (pure, of known order),
which the model carries as a multiple mod its order.

INTENDED VERDICT (intended()).  Schnorr: the sum is the identity, mod M and in the opaque point.  Pairing:
sigma' is not the identity and log sigma'_1 * log J' = log sigma'_2 * log g~ mod r, where only J''s part in
the order-r subgroup counts in SigG2 (a G1 point of order 3 or 11 pairs to one); in SigG1 a J' with a
small-order part is the Miller loop's Q outside G2, which the reference's check rejects.

THE MODEL (trace()).  pok_pervk.hip keeps one table [g~, Y~_0..q-1, J] and walks it twice: chain A over g~,
the hidden Y~_j and J (responses, chal), then + (-T); chain B over the revealed Y~_j in INDEX order (their
messages), then + X~, then + J.  Each walk is straus_edges.walk (65 signed windows, doublings skipped on
the identity, zero digits and identity multiples skipped); every addition takes one of fixed_edges.CHAIN.
steer() relates a base to the accumulator it meets first, so that addition doubles or cancels.
"""
import ctypes
import functools
import random
from concurrent.futures import ThreadPoolExecutor

import fixed_edges as F
import straus_edges as SE
import torsion_edges as TE
from fixed_edges import G1_GENERATOR, G2_GENERATOR, P, R, be48
from straus_edges import M, ORDER, TORSION, digits, sub

SHAPES = ((1, ()), (1, (0,)), (6, ()), (6, (1, 4)), (6, (0, 1, 2, 3, 4, 5)), (32, (3, 5, 7, 11, 13, 17, 19, 23)),
          (6, (5, 2)))  # (q, revealed); the last one unsorted
SIZES = (1, 65, 257)  # a partial wave, a wave boundary, a block boundary (lanes and lane pairs)
KINDS = ("bad_response", "bad_revealed", "next_key")
VARIANTS = ("valid", "resp0_off_by_1", "sigma2_off_by_g")
EDGE_SCALARS = (0, 1, R - 1, R, R + 1, (1 << 384) - 1, int("8" * 64, 16), int("7" * 64, 16), (1 << 254) | (0xF << 248))


def shape_id(s):
    """q6r2, and q6r2u for an unsorted index list"""
    return f"q{s[0]}r{len(s[1])}" + ("u" if list(s[1]) != sorted(s[1]) else "")


def groups(mode):
    """(other group, signature group) of a mode"""
    return (1, 2) if mode == 0 else (2, 1)


def _sz(n):
    return ctypes.c_size_t(n)


# ---------------------------------------------------------------- points from scalars
def oracle_mul(oc, threads=8):
    def mul(group, scalars):
        eb, n = (97 if group == 1 else 192), len(scalars)
        out = ctypes.create_string_buffer(eb * max(n, 1))
        oc.oc_gen_mul_mt(group, _sz(n), b"".join(be48(s % R) for s in scalars), out, threads)
        return out.raw[:eb * n]
    return mul


def gpu_mul(ctx):
    import coconut
    gen = {1: coconut.G1_GENERATOR, 2: coconut.G2_GENERATOR}
    return lambda group, scalars: bytes(coconut.fixed_base_mul(ctx, group, gen[group],
                                                               b"".join(be48(s % R) for s in scalars)))


# ---------------------------------------------------------------- distinct verkeys
def shared_gk(mode):
    """log of the g~ every list of a mode is built on (a context holds one g~)"""
    return random.Random(0x9E + mode).randrange(1 << 250, R)


def distinct_batch(mul, mode, n, q, revealed, seed, bad_every=4, keys=None, gk=None):
    """dict(mode, n, q, revealed, nresp, s1, s2, J, T, resp, chal, rev, X, Y, g, expect, names, keys, gk).
    keys: the n verkeys' logarithms [x, y_0 ..] relative to g~ (default: uniform, all different; with keys
    given, "the next proof's key" is a fresh random one); gk: log g~ (default: from the seed)."""
    og, sg = groups(mode)
    ob = 97 if og == 1 else 192
    revealed = list(revealed)
    rng = random.Random(seed)
    fr = lambda: rng.randrange(1, R)  # noqa: E731
    gk = gk or fr()
    hidden = [i for i in range(q) if i not in revealed]
    own = keys is None
    keys = keys or [[fr() for _ in range(q + 1)] for _ in range(n)]
    e1, e2, ej, et, resp, chal, rev, expect, names = [], [], [], [], [], [], [], [], []
    for p in range(n):
        kind = KINDS[(p // bad_every) % 3] if bad_every and p % bad_every == bad_every - 1 else "valid"
        if kind == "bad_revealed" and not revealed:
            kind = "sigma2_off_by_g"
        key = keys[p]  # the key the holder proved under
        if kind == "next_key":
            key = keys[(p + 1) % n] if own else [fr() for _ in range(q + 1)]
        x, y = key[0], key[1:]
        m = [fr() for _ in range(q)]
        k, r1, r2, c = fr(), fr(), fr(), fr()
        s = (x + sum(a * b for a, b in zip(y, m))) % R
        e1.append(k * r1)
        e2.append(r1 * k * (s + r2) + (kind == "sigma2_off_by_g"))
        secrets = [r2] + [m[i] for i in hidden]
        ylog = [1] + [y[i] for i in hidden]
        bl = [fr() for _ in secrets]
        ej.append(gk * sum(a * b for a, b in zip(ylog, secrets)))
        et.append(gk * sum(a * b for a, b in zip(ylog, bl)))
        rs = [(b - c * sc) % R for b, sc in zip(bl, secrets)]
        if kind == "bad_response":
            rs[-1] = (rs[-1] + 5) % R
        rm = [m[i] for i in revealed]
        if kind == "bad_revealed":
            rm[0] = (rm[0] + 1) % R
        resp.append(b"".join(be48(v) for v in rs))
        chal.append(be48(c))
        rev.append(b"".join(be48(v) for v in rm))
        expect.append(int(kind == "valid"))
        names.append(kind)
    vk = mul(og, [gk * v for row in keys for v in row])
    X = b"".join(vk[(i * (q + 1)) * ob:(i * (q + 1) + 1) * ob] for i in range(n))
    Y = b"".join(vk[(i * (q + 1) + 1) * ob:(i + 1) * (q + 1) * ob] for i in range(n))
    return dict(mode=mode, n=n, q=q, revealed=revealed, nresp=len(hidden) + 1, s1=mul(sg, e1), s2=mul(sg, e2),
                J=mul(og, ej), T=mul(og, et), resp=b"".join(resp), chal=b"".join(chal), rev=b"".join(rev), X=X, Y=Y,
                g=mul(og, [gk]), expect=expect, names=names, keys=keys, gk=gk)


def _items(b):
    sb, ob = (192, 97) if b["mode"] == 0 else (97, 192)
    return dict(s1=sb, s2=sb, J=ob, T=ob, resp=b["nresp"] * 48, chal=48, rev=len(b["revealed"]) * 48, X=ob,
                Y=b["q"] * ob)


def take(b, idx):
    """The batch of proofs idx (a list of indices) of b."""
    out = dict(b, n=len(idx), expect=[b["expect"][i] for i in idx], names=[b["names"][i] for i in idx])
    for k, w in _items(b).items():
        out[k] = b"".join(b[k][i * w:(i + 1) * w] for i in idx)
    return out


def rotate_keys(b):
    """b with proof i checked against proof i + 1's verkey."""
    it = _items(b)
    return dict(b, X=b["X"][it["X"]:] + b["X"][:it["X"]], Y=b["Y"][it["Y"]:] + b["Y"][:it["Y"]])


def oracle_pok(oc, b, idx=None, threads=8):
    """[(verdict, GT bytes or None)] of oc_pok_verify per proof, each with ITS OWN verkey (no GT where the
    oracle rejects before the pairing: an identity sigma' or a failed Schnorr check)."""
    it = _items(b)
    r, nr, q = len(b["revealed"]), b["nresp"], b["q"]
    ridx = (ctypes.c_uint64 * max(r, 1))(*b["revealed"])
    cut = lambda k, i: b[k][i * it[k]:(i + 1) * it[k]]  # noqa: E731

    def one(i):
        gt = ctypes.create_string_buffer(576)
        v = oc.oc_pok_verify(b["mode"], _sz(q), _sz(r), cut("s1", i), cut("s2", i), cut("J", i), cut("T", i),
                             cut("resp", i), _sz(nr), cut("chal", i), ridx, cut("rev", i), cut("X", i), cut("Y", i),
                             b["g"], gt)
        return v, (gt.raw if any(gt.raw) else None)

    idx = list(range(b["n"])) if idx is None else list(idx)
    if not idx:
        return []
    first = one(idx[0])  # the oracle's one-time initialisation, alone
    with ThreadPoolExecutor(max(1, threads)) as ex:
        return [first] + list(ex.map(one, idx[1:]))


# ---------------------------------------------------------------- edge lists: the integer model
def hidden_of(L):
    return [i for i in range(L["q"]) if i not in L["rev"]]


def terms_a(L, c):
    """chain A's (log, encoded scalar) in table order: g~, the hidden Y~_j, J"""
    return ([(sub(L["gk"]), c["resp"][0])] + [(c["y"][j], c["resp"][1 + s]) for s, j in enumerate(hidden_of(L))] +
            [(c["j"], c["chal"])])


def terms_b(L, c):
    """chain B's: the revealed Y~_j in index order, each with its message"""
    return [(c["y"][j], c["revm"][L["rev"].index(j)]) for j in sorted(L["rev"])]


def sum_a(L, c):
    return sum((s % R) * lg for lg, s in terms_a(L, c)) % M


def jprime(L, c):
    return (c["x"] + c["j"] + sum((s % R) * lg for lg, s in terms_b(L, c))) % M


def _opaque_multiples(L, c):
    """(multiple in the Schnorr sum, multiple in J') of the case's opaque point, mod its order"""
    o = c["opq"]
    if not o:
        return 0, 0
    slot, m = o["slot"], o["order"]
    if slot == "X":
        return 0, 1 % m
    if slot == "J":
        return c["chal"] % R % m, 1 % m
    j = slot[1]
    if j in L["rev"]:
        return 0, c["revm"][L["rev"].index(j)] % R % m
    return c["resp"][1 + hidden_of(L).index(j)] % R % m, 0


def intended(L, c):
    oa, ob_ = _opaque_multiples(L, c)
    schnorr = (sum_a(L, c) - c["t"]) % M == 0 and oa == 0
    jp = jprime(L, c)
    in_g2 = jp % (M // R) == 0 and ob_ == 0
    pair = (c["e1"] % R != 0 and c["e2"] % R != 0 and (c["e1"] * (jp % R) - c["e2"] * L["gk"]) % R == 0 and
            (L["mode"] == 0 or in_g2))
    return int(schnorr and pair)


def trace(L, c):
    """dict(A, B: the branches of each chain's additions, the closing ones included; skipA, skipB: rounds of
    doublings skipped on a mid-walk identity; finalA, finalB: what each chain ends on)"""
    ca, ska = SE.walk([(lg, digits(s)) for lg, s in terms_a(L, c)])
    if c["t"] % M:
        ca.add(-c["t"])
    cb, skb = SE.walk([(lg, digits(s)) for lg, s in terms_b(L, c)])
    for v in (c["x"], c["j"]):
        if v % M:
            cb.add(v)
    return dict(A=ca.log, B=cb.log, skipA=ska, skipB=skb, finalA=ca.acc, finalB=cb.acc)


def steer(terms, k, sign):
    """A log for term k whose first addition meets sign x the accumulator (None if that is empty)."""
    hit = SE.walk([(lg, digits(s)) for lg, s in terms], stop_at=k)
    if not hit or not hit[0] or hit[0] % (M // R):
        return None
    return sub(sign * hit[0] * pow(hit[1], -1, R))


def _finish(L, c):
    if c["t"] is None:
        c["t"] = sum_a(L, c)
    if c["e2"] is None:
        c["e2"] = c["e1"] * (jprime(L, c) % R) * pow(L["gk"], -1, R) % R
    return c


def _new_list(mode, q, rev, seed):
    rng = random.Random(seed)
    L = dict(mode=mode, q=q, rev=list(rev), gk=rng.randrange(1 << 200, R), cases=[], rng=rng)
    return L


def _case(L, name, reach=(), **kw):
    """A random valid proof with the given fields replaced.  t / e2 left None are derived (valid)."""
    fr = lambda: L["rng"].randrange(1 << 250, R)  # noqa: E731
    q, r = L["q"], len(L["rev"])
    c = dict(name=name, x=sub(fr()), y=[sub(fr()) for _ in range(q)], j=sub(fr()), resp=[fr() for _ in range(q - r + 1)],
             chal=fr(), revm=[fr() for _ in range(r)], e1=fr(), t=None, e2=None, forms={}, off=(), opq=None,
             reach=list(reach))
    c.update(kw)
    L["cases"].append(c)
    return c


def _seal(L):
    for c in L["cases"]:
        _finish(L, c)
    L.pop("rng")
    return L


def _zero_sum_resp0(L, c):
    """g~'s response that makes the Schnorr sum the identity (every point in the subgroup)"""
    rest = sum((s % R) * lg for lg, s in terms_a(L, c)[1:]) % M
    assert rest % (M // R) == 0
    return (R - rest % R) * pow(L["gk"], -1, R) % R


@functools.lru_cache(maxsize=None)
def scalar_list(mode):
    """q = 6, revealed [1, 4]: every edge value as all responses, as the challenge, as all revealed messages."""
    L = _new_list(mode, 6, (1, 4), 8100 + mode)
    for i, e in enumerate(EDGE_SCALARS):
        _case(L, f"resp_{i}", resp=[e] * 5)
        _case(L, f"chal_{i}", chal=e)
        _case(L, f"rev_{i}", revm=[e, e])
    return _seal(L)


def _flip(pt):
    return pt[:-1] + bytes([pt[-1] ^ 1])


def _shift(group, j):
    def f(pt):
        head, body = (pt[:1], pt[1:]) if group == 1 else (b"", pt)
        out = []
        for o in range(0, len(body), 48):
            v = int.from_bytes(body[o:o + 48], "big")
            jj = ((1 << 384) - 1 - v) // P if j == "max" else j
            assert jj >= 1 and v + jj * P < 1 << 384
            out.append(be48(v + jj * P))
        return head + b"".join(out)
    return f


def identity_forms(group):
    """[(name, bytes -> an encoding that decodes to the identity)]"""
    gen = G1_GENERATOR if group == 1 else G2_GENERATOR
    forms = [("identity", lambda pt: pt), ("all_zero", lambda pt: bytes(len(pt))), ("off_curve", lambda pt: _flip(gen))]
    if group == 1:
        forms.append(("bad_prefix", lambda pt: b"\x03" + gen[1:]))
    return forms


@functools.lru_cache(maxsize=None)
def base_list(mode):
    """q = 6, revealed [1, 4] (hidden 0, 2, 3, 5; chain A: g~ Y0 Y2 Y3 Y5 J; chain B: Y1 Y4)."""
    og, _ = groups(mode)
    tors = TORSION[ORDER[og]]
    L = _new_list(mode, 6, (1, 4), 8200 + mode)
    fr = lambda: L["rng"].randrange(1 << 250, R)  # noqa: E731
    _case(L, "random", reach=[("A", "fresh"), ("A", "general"), ("A", "to-identity"), ("B", "fresh")])
    # ---- encodings of the identity, and coordinates >= p
    for nm, form in identity_forms(og):
        c = _case(L, f"y_hidden_{nm}", forms={("Y", 2): form})
        c["y"][2] = 0
        c = _case(L, f"y_revealed_{nm}", forms={("Y", 4): form})
        c["y"][4] = 0
    _case(L, "y_coords_plus_p", forms={("Y", 0): _shift(og, 1), ("Y", 1): _shift(og, "max")})
    # ---- related bases, literally
    c = _case(L, "hidden_equal_equal_scalars", reach=[("A", "fresh"), ("A", "doubling")])
    c["y"][2], c["resp"][0], c["resp"][2] = c["y"][0], 0, c["resp"][1]
    c = _case(L, "hidden_equal_opposite_scalars")
    c["y"][2], c["resp"][2] = c["y"][0], R - c["resp"][1]
    c = _case(L, "revealed_equal_equal_scalars", reach=[("B", "fresh"), ("B", "doubling")])
    c["y"][4], c["revm"][1] = c["y"][1], c["revm"][0]
    c = _case(L, "revealed_equal_opposite_scalars")
    c["y"][4], c["revm"][1] = c["y"][1], R - c["revm"][0]
    # ---- steered: the addition of Y3 (chain A) / Y4 (chain B) meets +-the accumulator
    for nm, sign, br in (("doubling", 1, ["doubling"]), ("cancel", -1, ["to-identity", "from-identity"])):
        c = _case(L, f"chainA_{nm}", reach=[("A", b) for b in br])
        c["y"][3] = steer(terms_a(L, c), 3, sign)
        c = _case(L, f"chainB_{nm}", reach=[("B", b) for b in br])
        c["y"][4] = steer(terms_b(L, c), 1, sign)
    c = _case(L, "x_equals_chainB", reach=[("B", "doubling")])
    c["x"] = sum((s % R) * lg for lg, s in terms_b(L, c)) % M
    c = _case(L, "j_equals_chainB_plus_x", reach=[("B", "doubling")])
    c["j"] = (c["x"] + sum((s % R) * lg for lg, s in terms_b(L, c))) % M
    c = _case(L, "jprime_identity", reach=[("B", "to-identity")])
    c["x"] = (M - c["j"] - sum((s % R) * lg for lg, s in terms_b(L, c))) % M
    # ---- J and T
    c = _case(L, "j_equals_y_hidden")
    c["j"] = c["y"][0]
    c = _case(L, "j_equals_neg_y_hidden")
    c["j"] = M - c["y"][3]
    _case(L, "j_equals_g_tilde", j=sub(L["gk"]))
    _case(L, "j_identity", j=0)
    _case(L, "j_off_curve", j=0, forms={"J": identity_forms(og)[2][1]})
    c = _case(L, "t_identity", t=0, reach=[("A", "to-identity")])
    c["resp"][0] = _zero_sum_resp0(L, c)
    c = _case(L, "t_off_curve_sum_zero", t=0, forms={"T": identity_forms(og)[2][1]}, reach=[("A", "to-identity")])
    c["resp"][0] = _zero_sum_resp0(L, c)
    _case(L, "t_off_curve_sum_nonzero", t=0, forms={"T": identity_forms(og)[2][1]})
    _case(L, "x_identity", x=0)
    _case(L, "x_all_zero", x=0, forms={"X": identity_forms(og)[1][1]})
    # ---- the group's small-order base (order 3 in G1, 13 in G2), alone and added to subgroup points
    ell = ORDER[og]
    _case(L, "x_small_order", x=tors)
    _case(L, "x_mixed", x=(sub(fr()) + tors) % M)
    c = _case(L, "y_hidden_small_order")
    c["y"][0] = tors
    c = _case(L, "y_hidden_mixed")
    c["y"][5] = (sub(fr()) + (ell - 1) * tors) % M
    c = _case(L, "y_revealed_small_order_message_multiple")
    c["y"][1], c["revm"][0] = tors, ell * 1990
    c = _case(L, "y_revealed_small_order")
    c["y"][1] = tors
    c = _case(L, "y_revealed_mixed")
    c["y"][4] = (sub(fr()) + tors) % M
    _case(L, "j_small_order", j=tors)
    _case(L, "j_mixed", j=(sub(fr()) + tors) % M)
    # ---- the other small-order points of tests/golden/torsion.json, opaque
    for nm, row in sorted(TE.fixture()["G1" if og == 1 else "G2"].items()):
        m = row["order"]
        if m > 1000:
            continue  # the mixed rows: covered above with known logarithms
        o = lambda slot: dict(slot=slot, order=m, point=row["point"])  # noqa: E731
        _case(L, f"x_{nm}", x=0, opq=o("X"))
        _case(L, f"j_{nm}_chal_multiple", j=0, chal=m * (fr() // m), opq=o("J"))
        _case(L, f"j_{nm}", j=0, opq=o("J"))
        c = _case(L, f"y_hidden_{nm}_resp_multiple", opq=o(("Y", 2)))
        c["y"][2], c["resp"][2] = 0, m
        c = _case(L, f"y_hidden_{nm}", opq=o(("Y", 2)))
        c["y"][2], c["resp"][2] = 0, m + 1
        c = _case(L, f"y_revealed_{nm}_message_multiple", opq=o(("Y", 4)))
        c["y"][4], c["revm"][1] = 0, 7 * m
        c = _case(L, f"y_revealed_{nm}", opq=o(("Y", 4)))
        c["y"][4], c["revm"][1] = 0, 1
    return _seal(L)


@functools.lru_cache(maxsize=None)
def unrevealed_list(mode):
    """q = 6, nothing revealed: chain B is empty, J' = X~ + J."""
    L = _new_list(mode, 6, (), 8300 + mode)
    _case(L, "random", reach=[("B", "fresh"), ("B", "general")])
    c = _case(L, "x_equals_neg_j", reach=[("B", "fresh"), ("B", "to-identity")])
    c["x"] = M - c["j"]
    c = _case(L, "x_equals_j", reach=[("B", "fresh"), ("B", "doubling")])
    c["x"] = c["j"]
    _case(L, "x_identity", x=0, reach=[("B", "fresh")])
    _case(L, "x_and_j_identity", x=0, j=0)
    return _seal(L)


EDGE_LISTS = {"scalars": scalar_list, "bases": base_list, "unrevealed": unrevealed_list}


# ---------------------------------------------------------------- edge lists as batches
def edge_batch(oc, L):
    """Every case of L three ways (VARIANTS) as a batch in distinct_batch()'s layout; expect = intended()."""
    mode, q, rev = L["mode"], L["q"], L["rev"]
    og, sg = groups(mode)
    ob = 97 if og == 1 else 192
    cs = L["cases"]
    n = len(cs)
    pts = [c["x"] for c in cs] + [c["j"] for c in cs] + [c["t"] for c in cs] + [v for c in cs for v in c["y"]]
    enc = SE.point_bytes(oc, og, pts)
    cut = lambda i: enc[i * ob:(i + 1) * ob]  # noqa: E731
    g = F.gen_mul(oc, og, [L["gk"]])
    out = dict(mode=mode, q=q, revealed=list(rev), nresp=q - len(rev) + 1, g=g, expect=[], names=[])
    col = {k: [] for k in ("s1", "s2", "J", "T", "resp", "chal", "rev", "X", "Y")}
    e1, e2 = [], []
    for i, c in enumerate(cs):
        pt = {"X": cut(i), "J": cut(n + i), "T": cut(2 * n + i)}
        for j in range(q):
            pt[("Y", j)] = cut(3 * n + i * q + j)
        if c["opq"]:
            pt[c["opq"]["slot"]] = c["opq"]["point"]
        for slot, form in c["forms"].items():
            pt[slot] = form(pt[slot])
        for v in VARIANTS:
            d = dict(c, resp=list(c["resp"]))
            if v == "resp0_off_by_1":
                d["resp"][0] = (d["resp"][0] % R + 1) % R
            if v == "sigma2_off_by_g":
                d["e2"] = c["e2"] + 1
            e1.append(d["e1"])
            e2.append(d["e2"])
            col["J"].append(pt["J"])
            col["T"].append(pt["T"])
            col["X"].append(pt["X"])
            col["Y"].append(b"".join(pt[("Y", j)] for j in range(q)))
            col["resp"].append(b"".join(be48(s) for s in d["resp"]))
            col["chal"].append(be48(d["chal"]))
            col["rev"].append(b"".join(be48(s) for s in d["revm"]))
            out["expect"].append(intended(L, d))
            out["names"].append(f"{c['name']}/{v}")
    col["s1"], col["s2"] = [F.gen_mul(oc, sg, e1)], [F.gen_mul(oc, sg, e2)]
    out.update({k: b"".join(v) for k, v in col.items()})
    out["n"] = len(out["names"])
    return out


# ---------------------------------------------------------------- threshold keys for the flow test
def shamir_keys(mode, n_iss, t, q, seed):
    """dict(gk, master [x, y_0..] (the polynomials' constant terms), ids 1..n_iss, shares [[x_k, y_k,j]])"""
    rng = random.Random(seed)
    fr = lambda: rng.randrange(1, R)  # noqa: E731
    polys = [[fr() for _ in range(t)] for _ in range(q + 1)]
    ev = lambda c, x: sum(a * pow(x, e, R) for e, a in enumerate(c)) % R  # noqa: E731
    ids = list(range(1, n_iss + 1))
    return dict(gk=fr(), master=[c[0] for c in polys], ids=ids, shares=[[ev(c, i) for c in polys] for i in ids])
