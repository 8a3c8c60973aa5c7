"""Inputs and expectations for the direct test of the pair-lane Miller loops (csrc/miller_lz.hip:
k_miller<SIG, false> two pairs a credential, k_miller<SIG, true> twin, k_miller4<SIG> quad), read by
tests/test_miller_lz_model.py on the CPU, tests/test_gpu_miller_lz_direct.py on the device and the
millerlz recipe of tests/golden/make_golden.py.

Encoding (csrc/soa.h, the header of miller_lz.hip).  Word w of Fp slot s of element i of the prep structure
of arrays is at (s * 12 + w) * pstride + i.  A twist point Q is affine in S_Q1 = 0..3 (pair 0) or
S_Q2 = 4..7 (pair 1): x real, x imaginary, y real, y imaginary, each value v stored as v 2^406 mod p
(fexp_direct_cases.R_STORE).  A G1 point P is affine in S_P1 = 8, 9 (pair 0) or S_P2 = 11, 12 (pair 1) in
the lazy field's R' form, v 2^392 mod p, canonical.  The launchers hard-wire pform = kAffRp, so the third
P slot (10, 13) is never read and the kJac and kAffR branches of eval_mul cannot be reached from any
launcher: there is nothing to test there, and the builder leaves those slots at the buffer's fill.  One
flag word per credential.

Constant operand.  SigG2: g~ in G1, 24 words in R' form (what cck_lazy_form(2, ...) makes of the 24
storage-form words x, y).  SigG1: the 68 x 72 line words cck_gtilde_lines makes of g~ in G2 (48
storage-form words xa, xb, ya, yb).  GTILDE1 / GTILDE2 are fixed seeded points, not the generators.

Launches.  A credential is (slot, ..., flag word); a Slot is what the prep holds for one pair: a real
(P, Q) or one of three kinds of garbage (zeros, an off-curve canonical point, all-0xFFFFFFFF words).
  two-pair  credential i = element i: (slot 0, slot 1, flags).  Pair 0 = (P1, Q1) is skipped on flags & 5.
            Pair 1 is skipped on flags & 18; SigG2 reads its Q2 (P is g~), SigG1 its P2 (Q is g~'s lines).
  twin      credential c = (slot, flags) sits at element c / 2 in the pair slots c & 1, skipped on flags & 5.
            TAIL: with n odd the pair-1 slots of the last element (n - 1) / 2 belong to no credential.
  quad      the twin layout; element j of the output is the product over credentials 4 j .. 4 j + 3.
            TAIL: the credentials n .. 4 ceil(n / 4) - 1 are absent; of their twin positions only the
            pair-1 slots of twin element (n - 1) / 2 for odd n lie inside the prep (stride ceil(n / 2)).
absent(kind, n) lists those positions.  The expectation of an element is the product of e(P, Q) over its
pairs that are present and not skipped (a skipped or absent pair counts as 1), as GT bytes from the C
oracle's oc_pairing (cached per distinct pair) and oracle/bls12_381.py f12_mul.

Tiled layouts (layout2, layout1).  Credential c takes P of pair c mod 16 of miller_wide_cases.pairs() and Q of
pair (c + (c / 16) mod 4) mod 16.  The plain block (PLAIN credentials: 16, quad 32) has no flags and
starts with the 16 pairs themselves, the bilinearity pair among them: it fills the 8 elements whose words
are recorded.  After it the credentials walk a list of combinations (flag word, what the skipped slots
hold): every skipping flag word once over real points and once over garbage, every other word over real
points.  The lists have odd lengths (25 and 13), so over 2 (4) rounds every combination meets every pair
position of the twin (quad) layout, and skipped and computed pairs sit side by side in every wave.
"""
import functools
import random
from collections import namedtuple

import numpy as np

import fexp_direct_cases as C
import miller_wide_cases as W
from oracle import bls12_381 as B
from oracle import subgroup as S

P = B.P
NW = C.NW
R_LAZY = pow(2, 392, P)  # csrc/lazy.h: the lazy field's R'
S_Q = (0, 4)             # csrc/soa.h S_Q1, S_Q2
S_P = (8, 11)            # S_P1, S_P2
PREP_SLOTS = 14
NLINES, LINE_WORDS = 68, 72
ONE_WORDS = W.ONE_WORDS
ONE_GT = C.ONE_GT
NPAIR = W.NPAIR

REAL, ZEROS, OFFCURVE, ONES = "real", "zeros", "off-curve", "ones"
GARBAGE = (ZEROS, OFFCURVE, ONES)
Slot = namedtuple("Slot", "kind p q")  # p / q: None where the slot's side is not a real point
EMPTY = Slot(ZEROS, None, None)

KINDS = ("g2", "g1", "twin", "quad")   # the launches: two-pair SigG2, two-pair SigG1, twin, quad
NP = {"g2": 1, "g1": 1, "twin": 2, "quad": 4}      # credentials per output element
PLAIN = {"g2": 16, "g1": 16, "twin": 16, "quad": 32}
SIZES = {"g2": (1, 2, 127, 128, 129), "g1": (1, 2, 127, 128, 129), "twin": (1, 2, 3, 255, 256, 257),
         "quad": (1, 2, 3, 4, 5, 511, 512, 513)}
BLOCK_PAIRS = 128  # 256 lanes a block, one output element per lane pair

FLAGS2 = (0, 1, 4, 5, 2, 16, 18, 3, 20, 23, 8, 32, 0x28, 0xFFFFFFE8, 0x80000001)
FLAGS1 = (0, 1, 4, 5, 2, 8, 16, 32, 0x3A, 0xFFFFFFFA)


def skips2(fl):
    """(pair 0 skipped, pair 1 skipped) of the two-pair loop."""
    return bool(fl & 5), bool(fl & 18)


def skips1(fl):
    return bool(fl & 5)


def _combos(flags, skipping):
    out = []
    for fl in flags:
        out.append((fl, False))
        if skipping(fl):
            out.append((fl, True))  # the skipped slots hold garbage
    return tuple(out)


COMBOS2 = _combos(FLAGS2, lambda fl: any(skips2(fl)))
COMBOS1 = _combos(FLAGS1, skips1)
assert len(COMBOS2) == 25 and len(COMBOS1) == 13  # odd: coprime to the 2 and 4 pair positions


# ---------------------------------------------------------------- points
@functools.lru_cache(maxsize=None)
def gtilde1():
    return B.G1.mul(B.G1.gen, random.Random(0x61D1).randrange(2, B.R))


@functools.lru_cache(maxsize=None)
def gtilde2(k=0):
    """The SigG1 constant; k = 1: a second one for the test of the line words."""
    return B.G2.mul(B.G2.gen, random.Random(0x61D2 + k).randrange(2, B.R))


def tiled_pair(c):
    b, t = divmod(c, NPAIR)
    pr = W.pairs()
    return pr[t][0], pr[(t + b % 4) % NPAIR][1]


def second(c):
    """Pair 1 of two-pair credential c: (P2 for SigG1, Q2 for SigG2)."""
    pr = W.pairs()
    return pr[(c + 7) % NPAIR][0], pr[(c + 3 + c // NPAIR) % NPAIR][1]


@functools.lru_cache(maxsize=None)
def twist_points():
    """{name: (Q, order or None)}: the twist points outside G2 of the qcheck tests.  The first three are
    tests/golden/torsion.json's (tests/torsion_edges.py models them); 'random' is a curve point without
    cofactor clearing, whose order divides h2 r and not r."""
    import torsion_edges as T
    fx = T.fixture()["G2"]
    out = {name: (B.g2_from_bytes(fx[name]["point"]), fx[name]["order"]) for name in ("T13", "T23", "kG+T13")}
    out["random"] = (S.random_curve_point(B.G2, 0x7E57C0DE), None)
    return out


# ---------------------------------------------------------------- words
def _words(v, r):
    v = v * r % P
    return [(v >> (32 * w)) & 0xFFFFFFFF for w in range(NW)]


def q_words(q):
    """48 words of an affine twist point, storage form."""
    (xa, xb), (ya, yb) = q
    return np.array(sum((_words(v, C.R_STORE) for v in (xa, xb, ya, yb)), []), dtype=np.uint32)


def p_words(p):
    """24 words of an affine G1 point, R' form."""
    return np.array(_words(p[0], R_LAZY) + _words(p[1], R_LAZY), dtype=np.uint32)


def p_store_words(p):
    """24 words of an affine G1 point, storage form (the input of cck_lazy_form)."""
    return np.array(_words(p[0], C.R_STORE) + _words(p[1], C.R_STORE), dtype=np.uint32)


def lazy_value(words):
    """The value of 12 R'-form words (the inverse of the encoding; asserts canonical)."""
    v = sum(int(x) << (32 * k) for k, x in enumerate(words))
    assert v < P
    return v * pow(R_LAZY, -1, P) % P


OFFCURVE_Q = ((1, 0), (1, 0))  # 1 != 1 + 4 (1 + i)
OFFCURVE_P = (1, 1)            # 1 != 1 + 4


def slot_words(slot):
    """(48 Q words, 24 P words) of a slot."""
    if slot.kind == ZEROS:
        return np.zeros(48, np.uint32), np.zeros(24, np.uint32)
    if slot.kind == ONES:
        return np.full(48, 0xFFFFFFFF, np.uint32), np.full(24, 0xFFFFFFFF, np.uint32)
    if slot.kind == OFFCURVE:
        return q_words(OFFCURVE_Q), p_words(OFFCURVE_P)
    return (q_words(slot.q) if slot.q is not None else None), (p_words(slot.p) if slot.p is not None else None)


def cells(kind, creds):
    """[(element, pair position, slot, sides)] of a launch: where each slot goes; sides: 'pq', 'q' or 'p'."""
    out = []
    for c, cr in enumerate(creds):
        if NP[kind] == 1:
            out.append((c, 0, cr[0], "pq"))
            out.append((c, 1, cr[1], "q" if kind == "g2" else "p"))
        else:
            out.append((c // 2, c & 1, cr[0], "pq"))
    return out


def elements_in(kind, n):
    """Prep elements of a launch of n credentials (the least pstride)."""
    return n if NP[kind] == 1 else (n + 1) // 2


def outputs(kind, n):
    return (n + NP[kind] - 1) // NP[kind]


def encode_prep(kind, creds, pstride=None, fill=0):
    """The prep structure of arrays of a launch; every word no slot owns holds `fill`."""
    m = elements_in(kind, len(creds))
    pstride = m if pstride is None else pstride
    a = np.full((PREP_SLOTS * NW, pstride), fill, dtype=np.uint32)
    for e, pos, slot, sides in cells(kind, creds):
        qw, pw = slot_words(slot)
        if "q" in sides and qw is not None:
            a[S_Q[pos] * NW:S_Q[pos] * NW + 48, e] = qw
        if "p" in sides and pw is not None:
            a[S_P[pos] * NW:S_P[pos] * NW + 24, e] = pw
    return np.ascontiguousarray(a.reshape(-1))


def flags_of(creds):
    return np.array([cr[-1] for cr in creds], dtype=np.uint32)


def absent(kind, n):
    """[(twin element, pair position)] inside the prep that belong to no credential (module docstring)."""
    if NP[kind] == 1 or n % 2 == 0:
        return []
    return [((n - 1) // 2, 1)]


# ---------------------------------------------------------------- tiled layouts
def _garbage(j):
    return GARBAGE[(j + j // 13) % 3]


def layout2(sig, n):
    """Two-pair launch of n: [(slot 0, slot 1, flag word)]."""
    out = []
    for c in range(n):
        p1, q1 = tiled_pair(c)
        p2, q2 = second(c)
        s0, s1 = Slot(REAL, p1, q1), (Slot(REAL, None, q2) if sig == "g2" else Slot(REAL, p2, None))
        fl = 0
        if c >= PLAIN[sig]:
            j = c - PLAIN[sig]
            fl, junk = COMBOS2[j % len(COMBOS2)]
            if junk:
                k0, k1 = skips2(fl)
                g = Slot(_garbage(j), None, None)
                s0, s1 = (g if k0 else s0), (g if k1 else s1)
        out.append((s0, s1, fl))
    return out


def layout1(kind, n):
    """Twin / quad launch of n credentials: [(slot, flag word)]."""
    out = []
    for c in range(n):
        p, q = tiled_pair(c)
        s, fl = Slot(REAL, p, q), 0
        if c >= PLAIN[kind]:
            j = c - PLAIN[kind]
            fl, junk = COMBOS1[j % len(COMBOS1)]
            if junk:
                s = Slot(_garbage(j), None, None)
        out.append((s, fl))
    return out


def layout(kind, n):
    return layout2(kind, n) if NP[kind] == 1 else layout1(kind, n)


def coverage(kind, creds, lo, hi):
    """{(flag word, pair position, slot kind is REAL)} over the credentials whose output element lies in
    [lo, hi); for the two-pair loop the position is the pair (0 / 1) and only skipped pairs of a
    skipping word, or any pair of a word that skips nothing, are counted."""
    seen = set()
    for c, cr in enumerate(creds):
        if not lo <= c // NP[kind] < hi:
            continue
        fl = cr[-1]
        if NP[kind] == 1:
            sk = skips2(fl)
            for pos in (0, 1):
                if sk[pos] or not any(sk):
                    seen.add((fl, pos, cr[pos].kind == REAL))
        else:
            seen.add((fl, c % NP[kind], cr[0].kind == REAL))
    return seen


def full_coverage(kind):
    """What coverage() must reach in each half of a block."""
    want = set()
    if NP[kind] == 1:
        for fl in FLAGS2:
            sk = skips2(fl)
            for pos in (0, 1):
                if sk[pos]:
                    want |= {(fl, pos, True), (fl, pos, False)}
                elif not any(sk):
                    want.add((fl, pos, True))
    else:
        for fl in FLAGS1:
            for pos in range(NP[kind]):
                want.add((fl, pos, True))
                if skips1(fl):
                    want.add((fl, pos, False))
    return want


# ---------------------------------------------------------------- launches built for one property
def _skipped(c):
    """A skipped twin / quad credential: a real point under flag 1 or 4, or garbage under 5."""
    p, q = tiled_pair(c + 1)
    return ((Slot(REAL, p, q), 1), (Slot(REAL, p, q), 4), (Slot(GARBAGE[c % 3], None, None), 5))[c % 3]


def bilinear_launch(kind):
    """(credentials, [(a, b or None, base)]): element a holds e(A P0, Q0), element b e(P0, A Q0), element
    base e(P0, Q0), every other pair of those elements skipped; the two-pair launch also runs the
    constant's pair alone (SigG2: e(g~, A Q0) against e(g~, Q0); SigG1: e(A P0, g~) against e(P0, g~))."""
    pr = W.pairs()
    trio = [pr[NPAIR - 2], pr[NPAIR - 1], pr[0]]
    assert trio[0][1] == trio[2][1] and trio[1][0] == trio[2][0]
    if NP[kind] == 1:
        p2, q2 = second(1)
        s1 = Slot(REAL, None, q2) if kind == "g2" else Slot(REAL, p2, None)
        creds = [(Slot(REAL, p, q), s1, fl) for (p, q), fl in zip(trio, (18, 2, 16))]
        s0 = Slot(REAL, *pr[3])
        ap0, aq0 = trio[0][0], trio[1][1]
        p0, q0 = trio[2]
        if kind == "g2":
            creds += [(s0, Slot(REAL, None, aq0), 1), (s0, Slot(REAL, None, q0), 4)]
        else:
            creds += [(s0, Slot(REAL, ap0, None), 5), (s0, Slot(REAL, p0, None), 0x80000001)]
        return creds, [(0, 1, 2), (3, None, 4)]
    npos = NP[kind]
    creds = []
    for e, (p, q) in enumerate(trio):
        for pos in range(npos):
            creds.append((Slot(REAL, p, q), 0) if pos == (e + 1) % npos else _skipped(len(creds)))
    return creds, [(0, 1, 2)]


def inverse_launch(kind, n, single=False):
    """Twin / quad credentials (P, Q), (-P, Q), ...: every element's product is one.  single: the second
    of each couple skipped (under flag 4, the point left in place), so that each element shows the
    Miller values that are left."""
    assert n % NP[kind] == 0
    out = []
    for c in range(n):
        p, q = tiled_pair(c // 2)
        out.append((Slot(REAL, B.G1.neg(p) if c & 1 else p, q), 4 if single and c & 1 else 0))
    return out


def exchange(kind, creds):
    """creds with two computed credentials of different elements exchanged, one on each side of the
    block edge where the launch crosses it: (new credentials, (element a, element b))."""
    npos, edge = NP[kind], BLOCK_PAIRS * NP[kind]
    live = [c for c, cr in enumerate(creds) if not skips1(cr[-1])]
    if len(creds) > edge:
        a, b = max(c for c in live if c < edge), min(c for c in live if c >= edge)
    else:
        a = live[1]
        b = next(c for c in live if c // npos > a // npos)
    assert a // npos != b // npos and creds[a][0] != creds[b][0]
    out = list(creds)
    out[a], out[b] = creds[b], creds[a]
    return out, (a // npos, b // npos)


def twist_launch(kind, where, q, fl=0):
    """The small twin (5 credentials) or quad (7) launch of the qcheck tests with the twist point q in
    credential `where`.  TWIST_WHERE lists the credentials that take it: every pair position, and the last
    credential of the odd launch."""
    n = {"twin": 5, "quad": 7}[kind]
    out = []
    for c in range(n):
        p, qq = tiled_pair(c + 2)
        out.append((Slot(REAL, p, q if c == where else qq), fl if c == where else 0))
    return out


TWIST_WHERE = {"twin": (2, 3, 4), "quad": (0, 1, 2, 3, 6)}


# ---------------------------------------------------------------- expectations
_GT = {}


def pairing_gt(oc, p, q):
    """GT bytes of e(p, q) from the C oracle, once per distinct pair (q may lie outside G2)."""
    key = (p, q)
    if key not in _GT:
        import torsion_edges as T
        _GT[key] = T.oc_pairing(oc, B.g1_to_bytes(p), B.g2_to_bytes(q))
    return _GT[key]


def gt_product(gts):
    if not gts:
        return ONE_GT
    f = list(B.gt_from_bytes(gts[0]))
    for g in gts[1:]:
        f = B.f12_mul(f, list(B.gt_from_bytes(g)))
    return B.gt_to_bytes(f)


def computed_pairs(kind, creds, g=None):
    """Per output element, the (P, Q) of the pairs the loop must compute.  g: the constant's point."""
    out = [[] for _ in range(outputs(kind, len(creds)))]
    for c, cr in enumerate(creds):
        fl = cr[-1]
        if NP[kind] == 1:
            k0, k1 = skips2(fl)
            if not k0:
                out[c].append((cr[0].p, cr[0].q))
            if not k1:
                out[c].append((g, cr[1].q) if kind == "g2" else (cr[1].p, g))
        elif not skips1(fl):
            out[c // NP[kind]].append((cr[0].p, cr[0].q))
    for el in out:
        assert all(p is not None and q is not None for p, q in el), "a computed pair over garbage"
    return out


def expected(oc, kind, creds, g=None):
    """GT bytes per output element."""
    if NP[kind] == 1 and g is None:
        g = gtilde1() if kind == "g2" else gtilde2()
    return [gt_product([pairing_gt(oc, p, q) for p, q in el]) for el in computed_pairs(kind, creds, g)]
