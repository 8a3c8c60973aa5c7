"""Edge-case rows for Verkey::aggregate from the resident issuer table (aggregate.hip k_vk_agg_fixed<Fp, 8>
and k_vk_agg_fixed_g2pl<8>, their chains fixed.h ft_add_lz and curve_pl.h pl::ft_add_g2_lz, the butterflies
curve.h lane_group_sum and curve_pl.h pl::pair_group_sum, capi_aggregate.cpp cc_set_issuers), with every
discrete logarithm known, and a model of the order in which a task adds its table entries.

Plain Python over integers plus the C oracle (oc_gen_mul, oc_msm through straus_edges.point_bytes, and
oc_verkey_aggregate for the expectations); no product code and no context.  Chain, the branch names and
ft_digit come from tests/fixed_edges.py; lagrange, the butterfly stage, steer_sum and the points mod
M = 39 r (a G + b T, T the group's small-order base) from tests/straus_edges.py.  straus_edges.steer reads a
Straus walk's accumulator; a table chain has no doublings, so steer_chain() below solves its own relation.

THE TASK (restated from the kernels).  One task is (credential, column j): j = 0 is X~, j = 1 .. q is
Y~_{j-1}.  The t terms l_k K_k (l_k the Lagrange coefficient of the row's k-th id over the de-duplicated first
t ids, K_k that issuer's key of column j) are shared out over NPART parts:

    mode 0 (SigG2, G1 keys)   8 lanes a task, term k to lane k mod 8
    mode 1 (SigG1, G2 keys)   4 lane pairs a task, term k to pair k mod 4

A part takes its issuers in rising k; an issuer whose key decoded to the identity (binf) is skipped; for
every other it takes the windows w = 0 .. nwin - 1, skipping zero digits and empty entries (the identity
multiples of a small-order key), and adds entry d 2^(wbits w) K_k with a mixed addition.  Then the butterfly
at lane distances 4, 2, 1 (mode 1: 4, 2, which are pair distances 2, 1), the lower part as the left operand.
A chain addition takes one of CHAIN, a join one of JOIN (tests/fixed_edges.py).

ROWS.  Every key is a known multiple of the generator (or of the small-order base).  A row either OWNS its
issuers (ids no other row uses; its key logarithms are chosen per row, so they can be solved from the row's
own coefficients) or draws from the POOL (the key of (id, column) is a fixed function of both, so rows that
share an id agree on its key): the coefficient edges, which are steered through the ids alone.  rows() lists
them, builds() packs them into cc_set_issuers calls whose tables stay at or below LIMIT bytes.

Widths FULL run the whole list; widths REDUCED the coefficient edges of the width, steered chain rows for
doubling and to-identity / from-identity, and one steered join row per butterfly distance, all with q = 0
and the smallest t (at 16 bits a build holds 10 G1 or 5 G2 bases).
"""
import ctypes
import functools
import random

import straus_edges as S
from fixed_edges import CHAIN, JOIN, P, R, Chain, be48, ft_digit, limbs, nwin  # noqa: F401
from straus_edges import M, lagrange, steer_sum, sub

NPART = {0: 8, 1: 4}  # parts a task: lanes (G1 keys), lane pairs (G2 keys)
DISTS = {0: (4, 2, 1), 1: (2, 1)}  # butterfly distances, in parts
FULL = (8, 10, 13)
REDUCED = (12, 16)
WIDTHS = FULL + REDUCED
LIMIT = 1 << 30  # bytes of one build's tables
UNKNOWN = (0xFFFFFFFF00000005, 0xFFFFFFFF00000007)  # ids no build holds
TASK_ROWS = {0: (1, 31, 32, 33, 65), 1: (16, 17), 5: (6, 11)}  # rows a call, per q: n (q + 1) tasks, 32 a block


def table_bytes(mode, wbits, nbases):
    return nbases * nwin(wbits) * ((1 << wbits) - 1) * (96 if mode == 0 else 192)


def coefficients(ids):
    """The Lagrange coefficients of the first t ids as Verkey::aggregate takes them: over the de-duplicated
    set, a repeated id with the same coefficient at each of its positions (oracle oc_lagrange)."""
    seen = list(dict.fromkeys(ids))
    l = dict(zip(seen, lagrange(seen)))
    return [l[i] for i in ids]


def digit_plain(v, w, wbits):
    """Window w of v from the integer itself (ft_digit works on 32-bit limbs)."""
    return (v >> (wbits * w)) & ((1 << wbits) - 1)


# ---------------------------------------------------------------- the model
def trace(mode, wbits, coef, logs):
    """The additions of one task: dict(chain=[branches of part p], join={distance: [branches]}, sums=[part
    sums], final).  coef: t canonical scalars; logs: the t keys of the task's column as points mod M."""
    npart, n = NPART[mode], nwin(wbits)
    chain, sums = [], []
    for p in range(npart):
        c = Chain(0, M)
        for k in range(p, len(coef), npart):
            if logs[k] % M == 0:  # binf
                continue
            kl = limbs(coef[k])
            for w in range(n):
                d = ft_digit(kl, w, wbits)
                e = d * pow(2, wbits * w, M) * logs[k] % M
                if d and e:  # a zero digit; an empty entry
                    c.add(e)
        chain.append(c.log)
        sums.append(c.acc)
    jn, vals = {}, sums
    for m in DISTS[mode]:
        jn[m] = []
        vals = S.butterfly_stage(vals, m, jn[m])
    return dict(chain=chain, join=jn, sums=sums, final=vals[0])


def expected(coef, logs):
    return sum(c * x for c, x in zip(coef, logs)) % M


def steer_chain(mode, wbits, coef, logs, k2, where, sign):
    """A log for issuer k2 (not the first of its part) so that its addition at its first / middle / last
    non-zero window meets sign x the accumulator: with A the sum of the part's earlier issuers and
    lo = l mod 2^(wbits w), A + lo x = sign d_w 2^(wbits w) x."""
    npart = NPART[mode]
    A = sum(coef[k] * logs[k] for k in range(k2 % npart, k2, npart)) % M
    assert A % (M // R) == 0 and A
    nz = [w for w in range(nwin(wbits)) if digit_plain(coef[k2], w, wbits)]
    w = {"first": nz[0], "middle": nz[len(nz) // 2], "last": nz[-1]}[where]
    lo = coef[k2] % (1 << (wbits * w))
    den = (sign * digit_plain(coef[k2], w, wbits) * (1 << (wbits * w)) - lo) % R
    return sub(A % R * pow(den, -1, R))


def join_sides(mode, stage, t):
    """(left, right): the term indices whose sum is the left / right operand at part 0 of butterfly stage
    `stage` (the parts joined before it differ in the earlier distances' bits only)."""
    d = DISTS[mode]
    earlier = sum(d[:stage])
    left = [p for p in range(NPART[mode]) if p & ~earlier == 0]
    right = [p | d[stage] for p in left]
    pick = lambda parts: [k for k in range(t) if k % NPART[mode] in parts]  # noqa: E731
    return pick(left), pick(right)


def steer_join(mode, coef, logs, stage, sign):
    """(j, log): the right side's last key so that the two operands of stage `stage` are equal or opposite."""
    left, right = join_sides(mode, stage, len(coef))
    target = sign * expected([coef[k] for k in left], [logs[k] for k in left]) % M
    v = steer_sum(logs, coef, right, right[-1], target)
    assert v is not None
    return right[-1], v


# ---------------------------------------------------------------- rows
def pool_log(i, j):
    """The key of pool issuer i, column j"""
    return sub(random.Random(f"pool/{i}/{j}").randrange(1 << 200, R))


def boundary_bits(wbits):
    """s <= 63 on or beside a window boundary"""
    return [s for w in range(1, 64 // wbits + 1) for s in (wbits * w - 1, wbits * w, wbits * w + 1) if s <= 63]


class _Rows:
    def __init__(self, mode, wbits):
        self.mode, self.wbits, self.rows = mode, wbits, []
        self.rng = random.Random(100 * wbits + mode)

    def fresh_ids(self, t):
        r = len(self.rows) + 1
        return [(r << 32) | x for x in self.rng.sample(range(16, 1 << 20), t)]

    def rnd(self):
        return sub(self.rng.randrange(1 << 200, R))

    def add(self, name, q, ids, logs=None, forms=None, reach=(), claim=(), solo=False):
        t = len(ids)
        pool = logs is None
        if pool:
            logs = [[pool_log(i, j) for j in range(q + 1)] for i in ids]
        self.rows.append(dict(name=name, q=q, t=t, ids=list(ids), coef=coefficients(ids), logs=logs, forms=forms or {},
                              reach=list(reach), claim=list(claim), pool=pool, solo=solo))

    def own(self, t, q):
        ids = self.fresh_ids(t)
        return ids, coefficients(ids), [[self.rnd() for _ in range(q + 1)] for _ in range(t)]

    def chain_row(self, where, t, signs):
        q, k2 = len(signs) - 1, NPART[self.mode]
        ids, coef, logs = self.own(t, q)
        reach = []
        for j, sign in enumerate(signs):
            col = [l[j] for l in logs]
            logs[k2][j] = steer_chain(self.mode, self.wbits, coef, col, k2, where, sign)
            reach += [(j, "chain", 0, b) for b in (("doubling",) if sign > 0 else ("to-identity", "from-identity"))]
        self.add(f"chain/{where}/t{t}/" + "".join("+" if s > 0 else "-" for s in signs), q, ids, logs, reach=reach)

    def join_row(self, stage, t, signs):
        q = len(signs) - 1
        ids, coef, logs = self.own(t, q)
        reach = []
        for j, sign in enumerate(signs):
            k, v = steer_join(self.mode, coef, [l[j] for l in logs], stage, sign)
            logs[k][j] = v
            reach.append((j, "join", DISTS[self.mode][stage], "doubling" if sign > 0 else "to-identity"))
        self.add(f"join/d{DISTS[self.mode][stage]}/t{t}/" + "".join("+" if s > 0 else "-" for s in signs), q, ids, logs,
                 reach=reach)


@functools.lru_cache(maxsize=None)
def rows(mode, wbits):
    """The rows of one (mode, width): [dict(name, q, t, ids (t), coef (t), logs (t x (q + 1), points mod M),
    forms {(k, j): encoding form}, reach [(column, 'chain' / 'join', part or distance, branch)], claim [(k,
    coefficient)], pool, solo)]; shared between tests, not to be modified."""
    B = _Rows(mode, wbits)
    npart, full = NPART[mode], wbits in FULL
    # ---- steered chains (part 0: issuers 0, npart, 2 npart, ...)
    if full:
        B.chain_row("first", npart + 1, (1, -1))
        B.chain_row("middle", 2 * npart, (-1, 1))
        B.chain_row("last", 2 * npart + 1, (1, -1))  # the third issuer restarts from the identity
        B.chain_row("middle", 33, (-1,))
    else:
        B.chain_row("middle", npart + 1, (1,))
        B.chain_row("first", npart + 1, (-1,))
    # ---- steered joins, every distance
    for stage in range(len(DISTS[mode])):
        if full:
            B.join_row(stage, ((8, 7, 9), (4, 7))[mode][stage], (1, -1))
            B.join_row(stage, npart, (-1, 1))
        else:
            B.join_row(stage, npart, (1 if stage % 2 == 0 else -1,))
    # ---- coefficient edges through the ids alone (pool keys), q = 0
    for p in range(npart + 1):  # id 0 at position p: coefficient 1 there, 0 elsewhere
        ids = list(range(1, npart + 1))
        ids.insert(p, 0)
        B.add(f"coef/id0_at_{p}", 0, ids, claim=[(k, int(k == p)) for k in range(npart + 1)])
    B.add("coef/r_minus_1", 0, [2, 1], claim=[(0, R - 1), (1, 2)])
    for s in boundary_bits(wbits):
        B.add(f"coef/pow2_{s}", 0, [(1 << s) - 1, 1 << s], claim=[(0, 1 << s), (1, R - ((1 << s) - 1))])
        B.add(f"coef/ones_{s}", 0, [(1 << s) - 2, (1 << s) - 1], claim=[(0, (1 << s) - 1), (1, R - ((1 << s) - 2))])
        if s >= 2:  # (a, a + 1, a + 2), a + 1 = 2^s: bits above 64
            B.add(f"coef/three_{s}", 0, [(1 << s) - 1, 1 << s, (1 << s) + 1],
                  claim=[(0, (1 << (s - 1)) * ((1 << s) + 1)), (1, R - ((1 << (2 * s)) - 1)),
                         (2, ((1 << s) - 1) * (1 << (s - 1)))])
    B.add("coef/high_words", 0, [1 << 63, (1 << 64) - 2, (1 << 64) - 1])
    B.add("coef/repeated_id", 0, [5, 7, 5, 6] if full else [5, 7, 5])
    B.add("n_iss_1", 0, [1 << 63], claim=[(0, 1)], solo=True)
    if not full:
        return B.rows
    # ---- shapes: t = 16, 17 with q = 0 (own keys); t = 1 .. 5 with q = 5 (pool keys: 6 tasks a credential)
    for t in (16, 17):
        ids, _, logs = B.own(t, 0)
        B.add(f"shape/t{t}", 0, ids, logs)
    for t in (1, 2, 3, 4, 5):
        ids = list(range(1, 6))
        B.rng.shuffle(ids)
        B.add(f"shape/q5/t{t}", 5, ids[:t])
    # ---- key encodings (q = 1)
    t = npart  # X~: even issuers undecodable, odd ones fine (one with coordinates >= p); Y~_0 the other way round
    ids, _, logs = B.own(t, 1)
    bad = ("identity", "off", "prefix" if mode == 0 else "zero")
    forms = {}
    for k in range(t):
        j = k % 2  # the column whose key is undecodable
        logs[k][j] = 0
        forms[(k, j)] = bad[(k // 2) % 3]
    forms[(1, 0)] = forms[(2, 1)] = "gep"
    B.add("enc/undecodable", 1, ids, logs, forms,
          reach=[(0, "join", 1, "left-identity"), (1, "join", 1, "right-identity")])
    ids, _, logs = B.own(3, 1)
    logs[0][1] = logs[0][0]  # X~ = Y~_0
    logs[1][1] = M - logs[1][0]  # X~ = -Y~_0
    logs[2] = [logs[0][0], M - logs[0][0]]  # another issuer's key, and its negative
    B.add("enc/related_keys", 1, ids, logs)
    ids, _, logs = B.own(3, 1)  # one key of small order: empty table entries
    tors = S.TORSION[S.ORDER[1 if mode == 0 else 2]]
    logs[1] = [tors, (logs[1][1] + 2 * tors) % M]
    B.add("enc/small_order", 1, ids, logs)
    return B.rows


# ---------------------------------------------------------------- builds
@functools.lru_cache(maxsize=None)
def builds(mode, wbits):
    """[dict(mode, wbits, q, ids (in the shuffled order cc_set_issuers is given them), keys {id: (logs, forms)},
    rows)]: the rows of rows() packed greedily, in order, per q, into tables of at most LIMIT bytes."""
    cap = max(n for n in range(1, 1 << 12) if table_bytes(mode, wbits, n) <= LIMIT)
    out = []

    def keys_of(r):
        return {i: (r["logs"][k], [r["forms"].get((k, j)) for j in range(r["q"] + 1)]) for k, i in enumerate(r["ids"])}

    for q in sorted({r["q"] for r in rows(mode, wbits)}):
        cur = None
        for r in (r for r in rows(mode, wbits) if r["q"] == q):
            ks = keys_of(r)
            assert len(ks) * (q + 1) <= cap, (r["name"], "does not fit a table")
            if cur is None or r["solo"] or cur["solo"] or len({**cur["keys"], **ks}) * (q + 1) > cap:
                cur = dict(mode=mode, wbits=wbits, q=q, keys={}, rows=[], solo=r["solo"])
                out.append(cur)
            for i, v in ks.items():
                assert cur["keys"].setdefault(i, v) == v, (r["name"], i)
            cur["rows"].append(r)
    for n, b in enumerate(out):
        b["ids"] = sorted(b["keys"])
        random.Random(1000 * wbits + 10 * n + mode).shuffle(b["ids"])
        if b["ids"] == sorted(b["ids"]):  # never the order cc_set_issuers sorts them into
            b["ids"].reverse()
        b["bytes"] = table_bytes(mode, wbits, len(b["ids"]) * (b["q"] + 1))
    return out


# ---------------------------------------------------------------- points and expectations from the oracle
def _sz(n):
    return ctypes.c_size_t(n)


def key_bytes(oc, mode, log, form=None):
    """The encoding of one key: the point's own, or one of the forms identity (log 0), off (an off-curve
    encoding), prefix (G1: a prefix byte other than 4), zero (all bytes zero), which all decode to the identity,
    and gep (every coordinate + p: it decodes to the point)."""
    og = 1 if mode == 0 else 2
    if form in ("off", "prefix", "zero", "identity"):
        assert log % M == 0
        g = bytearray(S.G1_GENERATOR if og == 1 else S.G2_GENERATOR)
        if form == "off":
            g[-1] ^= 1
        elif form == "prefix":
            g[0] = 3
        elif form == "zero":
            g = bytearray(len(g))
        else:
            g = bytearray(S.G1_IDENTITY if og == 1 else S.G2_IDENTITY)
        return bytes(g)
    b = S.point_bytes(oc, og, [log])
    if form == "gep":
        assert log % M
        head, body = (b[:1], b[1:]) if og == 1 else (b"", b)
        b = head + b"".join(be48(int.from_bytes(body[o:o + 48], "big") + P) for o in range(0, len(body), 48))
    else:
        assert form is None
    return b


_ENC = {}


def build_bytes(oc, b):
    """{id: [encoded key of column j]} of a build (cached by the build's place in builds())."""
    key = (b["mode"], b["wbits"], id(b))
    if key not in _ENC:
        _ENC[key] = {i: [key_bytes(oc, b["mode"], x, f) for x, f in zip(*b["keys"][i])] for i in b["ids"]}
    return _ENC[key]


def issuer_arrays(oc, b, order=None):
    """(ids, X, Y) as cc_set_issuers takes them, in `order` (default: the build's shuffled order)."""
    enc = build_bytes(oc, b)
    ids = list(order if order is not None else b["ids"])
    return ids, b"".join(enc[i][0] for i in ids), b"".join(e for i in ids for e in enc[i][1:])


_WANT = {}


def oracle_row(oc, b, r):
    """(X, Y) of oc_verkey_aggregate on the row's own keys (first t ids alone), cached."""
    key = (b["mode"], b["wbits"], r["name"])
    if key not in _WANT:
        enc, q, t = build_bytes(oc, b), b["q"], r["t"]
        ob = 97 if b["mode"] == 0 else 192
        X = b"".join(enc[i][0] for i in r["ids"])
        Y = b"".join(e for i in r["ids"] for e in enc[i][1:])
        oX, oY = ctypes.create_string_buffer(ob), ctypes.create_string_buffer(ob * max(q, 1))
        assert oc.oc_verkey_aggregate(b["mode"], _sz(t), _sz(t), _sz(q), (ctypes.c_uint64 * t)(*r["ids"]), X, Y, oX, oY) == 0
        _WANT[key] = (oX.raw, oY.raw[:ob * q])
    return _WANT[key]
