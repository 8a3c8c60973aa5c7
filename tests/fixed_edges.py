"""Edge-case inputs for the fixed-base window-table paths, with every discrete logarithm known, and a
model in discrete-log space of the order in which each kernel adds its table entries.

Plain Python over integers mod r plus the C oracle's oc_gen_mul (points from scalars); no product code
and no context.  Everything is a known multiple of the generator, as tests/test_gpu_parity.py _gen_batch
builds its batches: g~ = gk G, X~ = x g~, Y~_j = y_j g~.

The verkeys are built PER TABLE WIDTH wbits (nwin = ceil(256 / wbits) windows) with related bases, so
that two different table entries are the same point or opposite points and the exceptional branches of
the table additions are reached on purpose:

    y_1 = sign 2^(wbits a) y_0     entry (base 1, window w, digit d) = sign entry (base 0, window w + a, d)
    y_2 = -y_0                     entry (base 2, window w, digit d) = -entry (base 0, window w, d)

and X~ random, X~ = Y~_0 or X~ = identity.  `a` (it may be zero or negative: 2^(wbits a) mod r) is chosen
per kernel layout: nwin / 2 puts the two related entries on the two lanes of k_prep_sigg2_pair; for the
one-wave kernels (term t = j nwin + w to lane group t mod NG) one `a` puts them in different groups, so
they meet in the butterfly, and one in the same group, so they meet in a group's chain.

The model (trace_verify, trace_pok) restates, from kernels.hip / aggregate.hip / fixed.h /
curve_wide_lz.h, which additions a kernel performs in which order, and classifies every one by the
branch of the group law it takes.  A chain addition (accumulator + affine table entry: lz::jg_add_aff,
jl_add_aff_c, their spread forms) takes one of

    fresh          the accumulator is the identity because nothing was added yet
    general
    doubling       the accumulator equals the entry (h == 0, r == 0)
    to-identity    the accumulator is the entry's negative (h == 0, r != 0)
    from-identity  the accumulator is the identity again after a to-identity, mid-chain

and a join (full addition of two partial sums: jac_add, lz::wide::jg_add / jl_add) one of

    left-identity, right-identity, general, doubling, to-identity.

tests/test_fixed_edges_model.py asserts that the cases below reach the branches they are named for and
that per width and layout all five of each kind are reached; tests/test_gpu_fixed_edges.py runs them on
the device against the oracle.
"""
import ctypes
import functools
import random

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB

WIDTHS = (8, 9, 10, 14, 16, 21)  # the widths the device test runs
POK_WIDTHS = (8, 14)
NGROUPS = {0: 16, 1: 8}  # lane groups of k_prep_sigg2_wide / k_prep_sigg1_wide
CHAIN = ("fresh", "general", "doubling", "to-identity", "from-identity")
JOIN = ("left-identity", "right-identity", "general", "doubling", "to-identity")
Q = 3

G1_IDENTITY = b"\x04" + bytes(95) + b"\x01"
G2_IDENTITY = bytes(143) + b"\x01" + bytes(48)
G1_GENERATOR = bytes.fromhex(
    "04"
    "17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb"
    "08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1")
G2_GENERATOR = bytes.fromhex(
    "024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8"
    "13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e"
    "0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801"
    "0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be")


def nwin(wbits):
    return (256 + wbits - 1) // wbits


def be48(v):
    """The 48-byte big-endian encoding of v < 2^384, NOT reduced (non-canonical values stay so)."""
    return int(v).to_bytes(48, "big")


def limbs(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def ft_digit(k, w, wbits):
    """fixed.h ft_digit restated: window w of a canonical scalar given as 8 little-endian 32-bit limbs."""
    if wbits == 16:
        return (k[w >> 1] >> (16 * (w & 1))) & 0xFFFF
    if wbits == 8:
        return (k[w >> 2] >> (8 * (w & 3))) & 0xFF
    o = w * wbits
    i, sh = o >> 5, o & 31
    v = k[i] >> sh
    if sh and i + 1 < 8:
        v |= (k[i + 1] << (32 - sh)) & 0xFFFFFFFF
    return v & ((1 << wbits) - 1)


def digits(m, wbits):
    """The table digits of an encoded scalar: reduced mod r first (codec.h fr_from_be48)."""
    k = limbs(m % R)
    return [ft_digit(k, w, wbits) for w in range(nwin(wbits))]


def edge_scalars(wbits):
    """Scalars (as encoded, possibly non-canonical) whose digits sit at the edges of ft_digit."""
    n, ones = nwin(wbits), (1 << wbits) - 1
    top = (R - 1) >> (wbits * (n - 1))
    out = [0, 1, 2, R - 1, R - 2, 18, 1990, 7, R - (1 << 200), R - (1 << 200) - 1, R + 5, R, 2 * R + 7, (1 << 256) - 1,
           (1 << 384) - 1, (1 << 255), int("01" * 32, 16), ones, top << (wbits * (n - 1)), ones << (wbits * (n // 2))]
    out += [1 << (wbits * w) for w in range(n) if (1 << (wbits * w)) < R]
    out += [(1 << (wbits * w)) - 1 for w in range(1, n)] + [(1 << (wbits * w)) + 1 for w in range(1, n - 1)]
    out += [0xFF << (8 * k) for k in (0, 15, 31)]
    return out


# ---------------------------------------------------------------- the model: branches of the additions
class Chain:
    """An accumulator and the branch each mixed addition into it takes (points as multiples mod r; `mod`:
    the order of another cyclic group the points are counted in, tests/straus_edges.py)."""

    def __init__(self, start=0, mod=R):
        self.mod, self.acc, self.seen, self.log = mod, start % mod, start % mod != 0, []

    def add(self, e):
        e %= self.mod
        assert e, "a table entry is never the identity"
        if self.acc == 0:
            b = "from-identity" if self.seen else "fresh"
        elif self.acc == e:
            b = "doubling"
        elif (self.acc + e) % self.mod == 0:
            b = "to-identity"
        else:
            b = "general"
        self.seen = True
        self.log.append(b)
        self.acc = (self.acc + e) % self.mod
        return b


def join(p, q, log, mod=R):
    """A full addition p + q (the exceptional cases in the order jg_add / jac_add test them)."""
    if p == 0:
        b = "left-identity"
    elif q == 0:
        b = "right-identity"
    elif p == q:
        b = "doubling"
    elif (p + q) % mod == 0:
        b = "to-identity"
    else:
        b = "general"
    log.append(b)
    return (p + q) % mod


def butterfly_low_first(vals, log):
    """curve_wide_lz.h jg_group_sum / jl_group_sum: group distance 1, 2, 4, ...; the lower group's point
    is the first operand on both partners."""
    n = len(vals)
    m = 1
    while m < n:
        new = list(vals)
        for g in range(n):
            if g & m:
                continue
            s = join(vals[g], vals[g | m], log)
            new[g] = new[g | m] = s
        vals, m = new, m << 1
    return vals[0]


def butterfly_high_first(vals, log):
    """curve.h lane_group_sum / curve_pl.h pair_group_sum: distance L/2, L/4, ..., 1; lower lane first."""
    n = len(vals)
    m = n >> 1
    while m:
        new = list(vals)
        for g in range(n):
            if g & m:
                continue
            s = join(vals[g], vals[g | m], log)
            new[g] = new[g | m] = s
        vals, m = new, m >> 1
    return vals[0]


def entry(ylog, w, d, wbits):
    """The table entry d 2^(wbits w) B as a multiple of the generator."""
    return d * pow(2, wbits * w, R) * ylog % R


def trace_verify(vk, msgs, layout):
    """The additions of X~ + sum m_j Y~_j for one credential in one layout.  Returns
    dict(chain=[branches], join=[branches], final=multiple of the generator)."""
    wbits, mode = vk["wbits"], vk["mode"]
    n = nwin(wbits)
    dg = [digits(m, wbits) for m in msgs]
    ylog = [vk["gk"] * y % R for y in vk["y"]]
    xlog = vk["gk"] * vk["x"] % R  # 0: X~ is the identity (Xinf)
    chain, jn = [], []

    def run(c, terms):
        for j, w in terms:
            if dg[j][w]:
                c.add(entry(ylog[j], w, dg[j][w], wbits))
        chain.extend(c.log)
        return c.acc

    if layout == "pair" and mode == 0:  # k_prep_sigg2_pair: two half-chains and jac_add
        h = n // 2
        even = run(Chain(xlog), [(j, w) for j in range(Q) for w in range(0, h)])
        odd = run(Chain(0), [(j, w) for j in range(Q) for w in range(h, n)])
        final = join(even, odd, jn)
    elif layout == "pair":  # k_prep_sigg1_pair: one chain on the lane pair, no join
        final = run(Chain(xlog), [(j, w) for j in range(Q) for w in range(n)])
    else:  # k_prep_sigg{2,1}_wide: term t to group t mod NG, X~ in group 0, butterfly
        ng = NGROUPS[mode]
        vals = []
        for g in range(ng):
            ts = range(g, Q * n, ng)
            vals.append(run(Chain(xlog if g == 0 else 0), [(t // n, t % n) for t in ts]))
        final = butterfly_low_first(vals, jn)
    return dict(chain=chain, join=jn, final=final)


def scalar_of(vk, msgs):
    """x + sum m_j y_j mod r: the credential's MSM as a multiple of g~."""
    return (vk["x"] + sum((m % R) * y for m, y in zip(msgs, vk["y"]))) % R


# ---------------------------------------------------------------- verkeys and message cases
def _choose_a(wbits, mode):
    """a_pair = nwin / 2; a_same: entries (0, w + a) and (1, w) in the SAME one-wave group (a = nwin mod
    NG, the representative of least magnitude: 0 means plainly duplicated bases, which is the same group
    only where nwin mod NG == 0); a_diff candidates: in different groups for both relations (base 1 /
    base 0 and base 2 / base 1), neighbouring groups first (they meet in the butterfly's first stage, away
    from X~'s group 0)."""
    n, ng = nwin(wbits), NGROUPS[mode]
    same = [a for a in range(-(n - 1), n) if (n - a) % ng == 0]
    a_same = min(same, key=lambda a: (abs(a), a < 0))
    diff = sorted((a for a in range(-(n - 1), n) if (n - a) % ng and (n + a) % ng),
                  key=lambda a: ((n - a) % ng not in (1, ng - 1), abs(a), a < 0))
    return n // 2, a_same, diff


def make_verkeys(wbits, mode):
    """The four verkeys of a (width, mode): dict(name, a, sign of y_1, X~ kind, x, y, gk)."""
    a_pair, a_same, a_diff = _choose_a(wbits, mode)
    rng = random.Random(1000 * wbits + mode)
    out = []
    for name, cand, sign, xkind in (("K0", a_diff, 1, "rand"), ("K1", [a_pair], 1, "inf"), ("K2", [a_same], 1, "y0"),
                                    ("K3", [a_same], -1, "rand")):
        y0, xr, gk = rng.randrange(1 << 253, R), rng.randrange(1 << 253, R), rng.randrange(1 << 200, R)
        x = {"rand": xr, "inf": 0, "y0": y0}[xkind]
        for k, a in enumerate(cand):  # K0: the first `a` with which both butterfly cases can be built
            vk = dict(name=name, wbits=wbits, mode=mode, a=a, sign=sign, xkind=xkind, x=x, gk=gk,
                      y=[y0, sign * pow(2, wbits * a, R) * y0 % R, R - y0])
            try:
                make_cases(vk)
                break
            except Unreachable:  # only this: any other failure of the construction shows as it is
                if k == len(cand) - 1:
                    raise
        out.append(vk)
    return out


class Unreachable(LookupError):
    """No candidate of a case family reaches the branch asked for (with this verkey)."""


def _find(vk, layout, where, branch, candidates, nonzero=True, after=None):
    """The first candidate message vector whose trace in `layout` takes `branch` at `where` ('chain' /
    'join'); nonzero: the whole sum is not the identity; after: a branch that must also occur (so that a
    chain or butterfly demonstrably goes on after the exceptional step)."""
    for msgs in candidates:
        t = trace_verify(vk, msgs, layout)
        if branch in t[where] and (not nonzero or t["final"]) and (after is None or after in t[where]):
            return msgs
    raise Unreachable(f"no candidate reaches {layout}/{where}/{branch} for {vk['name']} at {vk['wbits']} bits, "
                         f"mode {vk['mode']}")


def make_cases(vk):
    """The message cases of one verkey: [dict(name, msgs (encoded ints), reach [(layout, where, branch)])]."""
    wbits, mode, a = vk["wbits"], vk["mode"], vk["a"]
    n, h, ones = nwin(wbits), nwin(wbits) // 2, (1 << wbits) - 1
    top = (R - 1) >> (wbits * (n - 1))

    def D(w, d=1):
        return d << (wbits * w)

    ws = range(n)
    cases = []

    def case(name, msgs, *reach):
        cases.append(dict(name=name, msgs=[int(m) for m in msgs], reach=list(reach)))

    pj = [("pair", "join")] if mode == 0 else []  # only k_prep_sigg2_pair joins two halves
    if vk["name"] == "K0":  # generic edges, the butterfly's doubling and cancellation, the identity sum
        case("zero", [0, 0, 0], *[(l, w, "right-identity") for l, w in pj])
        case("one", [1, 0, 0], *[(l, w, "right-identity") for l, w in pj])
        case("r_minus_1", [R - 1] * 3, ("wide", "chain", "general"), ("wide", "join", "general"))
        case("small", [18, 1990, 7], *[(l, w, "right-identity") for l, w in pj], ("wide", "join", "left-identity"),
             ("wide", "join", "right-identity"))
        for w in (0, h - 1, h, n - 1):
            case(f"bit_w{w}", [D(w), 0, 0])
        case("bits_three", [D(h - 1), D(h, 2), D(n - 1)], *[(l, w, "general") for l, w in pj])
        case("ones_low", [D(0, ones), 0, 0])
        case("ones_mid", [0, D(h, ones), 0])
        case("ones_top", [0, 0, D(n - 1, top)])
        case("ones_all", [D(0, ones), D(h, ones) | D(1, ones), D(n - 1, top) | D(n - 2, ones)])
        case("near_r", [R - (1 << 200) - j for j in range(3)])
        case("noncanon_a", [R + 5, R, (1 << 256) - 1])
        case("noncanon_b", [(1 << 384) - 1, 2 * R + 7, R - 1])
        # equal / opposite entries in DIFFERENT one-wave groups: they meet in the butterfly, which goes on
        fill = [0] + [D(w, 5) for w in ws if D(w, 5) < R]
        eq = [[D(w + a, 3) + f, D(w, 3), 0] for w in ws if 0 <= w + a < n and D(w + a, 3) < R
              for f in fill if not (f and D(w + a, 3) & f)]
        case("equal_groups", _find(vk, "wide", "join", "doubling", eq, after="general"), ("wide", "join", "doubling"))
        op = [[f, D(w, 3), D(w + a, 3)] for w in ws if 0 <= w + a < n - 1 for f in fill[1:]]
        op += [[D(w, 3), f, D(w, 3)] for w in ws[:-1] for f in fill[1:]]
        case("opposite_groups", _find(vk, "wide", "join", "to-identity", op, after="general"),
             ("wide", "join", "to-identity"))
        # the whole sum is the identity: m_0 = -x / y_0 (flag 4; sigma_2 is then the identity too)
        case("identity_sum", [(R - vk["x"]) * pow(vk["y"][0], -1, R) % R, 0, 0],
             *[(l, w, "to-identity") for l, w in pj])
    elif vk["name"] == "K1":  # X~ = identity, a = nwin / 2: the lane pair's join
        case("zero_xinf", [0, 0, 0], ("wide", "join", "left-identity"), *[(l, w, "left-identity") for l, w in pj])
        case("small_xinf", [18, 1990, 7], ("pair", "chain", "fresh"), *[(l, w, "right-identity") for l, w in pj])
        case("odd_half_only", [D(h, 3), D(n - 2) | D(h + 1, ones), D(n - 1)], *[(l, w, "left-identity") for l, w in pj])
        case("equal_halves", [D(a, 7), D(0, 7), 0], *[(l, w, "doubling") for l, w in pj])
        case("equal_halves_more", [D(a, 7) | D(a + 1, 2), D(0, 7) | D(1, 2), 0], *[(l, w, "doubling") for l, w in pj])
        case("opposite_halves", [0, D(0, 7), D(a, 7)], *[(l, w, "to-identity") for l, w in pj])
        case("cancel_then_more_xinf", [D(1, 9), 0, D(1, 9) | D(2, 5)], ("pair", "chain", "to-identity"),
             ("pair", "chain", "from-identity"))
        case("r_minus_1_xinf", [R - 1] * 3)
    elif vk["name"] == "K2":  # X~ = Y~_0 and equal entries in the SAME group: doubling inside a chain
        more = D(1, 2) | D(h, 3) | D(n - 2, 1)
        allw = sum(D(w) for w in range(n - 1))
        case("chain_doubling_x", [1 | more, allw, 0], ("pair", "chain", "doubling"), ("wide", "chain", "doubling"))
        case("chain_doubling_x_only", [1, 0, 0], ("pair", "chain", "doubling"), ("wide", "chain", "doubling"))
        fill = [0] + [D(w, 5) for w in ws[:-1]]
        eq = [[D(w + a, 3), D(w, 3), f] for w in ws if 0 <= w + a < n - 1 for f in fill]
        # (a chain that starts from X~ never EQUALS a later entry, so in the pair layouts the doubling is X~'s)
        case("chain_doubling_rel", _find(vk, "wide", "chain", "doubling", [m for m in eq if m[2]] + eq),
             ("wide", "chain", "doubling"))
        case("cancel_x", [0, 0, 1 | D(1, 2) | D(h, 3)], ("pair", "chain", "to-identity"), ("pair", "chain", "from-identity"))
    else:  # K3: y_1 = -2^(wbits a) y_0 in the same group: a chain reaches the identity and goes on from it
        fill = [D(w, 5) for w in ws[:-1]]
        op = [[D(w + a, 3), D(w, 3), f] for w in ws if 0 <= w + a < n - 1 for f in fill]
        op += [[D(w + a, 3), D(w, 3) | f, 0] for w in ws if 0 <= w + a < n - 1 for f in fill if not D(w, 3) & f]
        # (a chain that starts from a random X~ never returns to the identity: in the pair layouts only
        # SigG2's odd lane, which starts empty, can; SigG1's single chain does with X~ = Y~_0 or X~ = identity)
        for lay in ("wide", "pair") if mode == 0 else ("wide",):
            case(f"chain_cancel_rel_{lay}", _find(vk, lay, "chain", "from-identity", op),
                 (lay, "chain", "to-identity"), (lay, "chain", "from-identity"))
        if mode == 0:  # m_0 = d and m_2 = d in one window (y_2 = -y_0), then further digits of m_2
            same = [[D(w, 9), 0, D(w, 9) | f] for w in ws[:-1] for f in fill if not D(w, 9) & f]
            case("chain_cancel_y2", _find(vk, "pair", "chain", "from-identity", same), ("pair", "chain", "to-identity"),
                 ("pair", "chain", "from-identity"))
        case("small_k3", [7, 18, 1990])
    for c in cases:
        assert all(0 <= m < (1 << 384) for m in c["msgs"])
    return cases


@functools.lru_cache(maxsize=None)
def verify_sets(wbits, mode):
    """[(verkey, cases)] for one (width, mode); shared between tests, not to be modified."""
    return [(vk, make_cases(vk)) for vk in make_verkeys(wbits, mode)]


# ---------------------------------------------------------------- points and expectations from the oracle
def _sz(n):
    return ctypes.c_size_t(n)


def gen_mul(oc, group, scalars):
    """k G for each k (mod r) by the C oracle; 0 gives the identity encoding."""
    eb = 97 if group == 1 else 192
    out = ctypes.create_string_buffer(eb * max(len(scalars), 1))
    oc.oc_gen_mul(group, _sz(len(scalars)), b"".join(be48(s % R) for s in scalars), out)
    return out.raw[:eb * len(scalars)]


def verkey_bytes(oc, vk):
    """(X~, Y~ concatenated, g~) encodings of a verkey dict; X~ = identity where x == 0."""
    og = 1 if vk["mode"] == 0 else 2
    ob = 97 if og == 1 else 192
    pts = gen_mul(oc, og, [vk["gk"] * vk["x"]] + [vk["gk"] * y for y in vk["y"]] + [vk["gk"]])
    nq = len(vk["y"])
    return pts[:ob], pts[ob:ob * (nq + 1)], pts[ob * (nq + 1):]


def verify_batch_inputs(oc, vk, cases, seed=1):
    """Every case as a valid credential (sigma_1 = k G, sigma_2 = k s G, s = x + sum m_j y_j) followed
    by its twin with sigma_2 off by the generator.  Returns dict(names, s1, s2, msgs, expect) where
    expect is the verdict known by construction: valid and s != 0."""
    sg = 2 if vk["mode"] == 0 else 1
    rng = random.Random(seed)
    e1, e2, names, expect, mb = [], [], [], [], []
    for c in cases:
        s = scalar_of(vk, c["msgs"])
        k = rng.randrange(1 << 250, R)
        for bad in (0, 1):
            e1.append(k)
            e2.append(k * s + bad)
            names.append(c["name"] + ("/off_by_g" if bad else "/valid"))
            expect.append(int(not bad and s != 0))
            mb.append(b"".join(be48(m) for m in c["msgs"]))
    return dict(names=names, s1=gen_mul(oc, sg, e1), s2=gen_mul(oc, sg, e2), msgs=b"".join(mb), expect=expect,
                n=len(names))


def oracle_verify(oc, vk, vkb, b, nthreads=8):
    """(verdicts list, GT bytes) of the batch from oc_verify_batch with the shared verkey."""
    n = b["n"]
    ver = ctypes.create_string_buffer(n)
    gts = ctypes.create_string_buffer(576 * n)
    oc.oc_verify_batch(vk["mode"], _sz(n), _sz(len(vk["y"])), b["s1"], b["s2"], b["msgs"], vkb[0], vkb[1], 0, vkb[2],
                       ver, gts, nthreads)
    return list(ver.raw), gts.raw


# ---------------------------------------------------------------- PoK of a signature
POK_Q = 6


def make_pok_verkey(wbits, mode, q=POK_Q):
    """q >= 6 bases with related ones among the hidden bases of the revealed set {1, 4}: y_2 = -y_0,
    y_3 = 2^(2 wbits) y_0 (entry (3, w, d) = entry (0, w + 2, d); two windows apart, so that in the one-block
    prep the two equal terms can sit on lanes of the same parity, away from the lane that adds -T)."""
    rng = random.Random(7000 + 10 * wbits + mode + 100 * q)
    y = [rng.randrange(1 << 253, R) for _ in range(q)]
    y[2] = R - y[0]
    y[3] = pow(2, 2 * wbits, R) * y[0] % R
    return dict(name="P", wbits=wbits, mode=mode, x=rng.randrange(1 << 253, R), y=y, gk=rng.randrange(1 << 200, R))


def pok_split(q, r, wbits):
    """aggregate.hip cck_prep_pok: the hidden responses role A takes in k_prep_pok_split."""
    hidden, n = q - r, nwin(wbits)
    s = int((n * (hidden + r - 1) - 223) / (2 * n))  # C division truncates toward zero
    return max(0, min(hidden, s))


def make_pok_cases(vk, revealed):
    """Proof cases for one revealed-index set: [dict(name, resp (encoded), chal, rev (encoded), msgs (all q,
    canonical), r2)].  A proof is valid whatever responses and challenge are chosen, once
    T = sum rho_k B_k + c J; hidden responses are listed in ascending base order after g~'s.
    With q = 6, pok_split() is 0 at every width (role A of k_prep_pok_split takes g~'s term alone), so
    "roleA_zero" means rho_0 = 0 and no case here puts the A / B boundary inside the hidden responses."""
    wbits, y, q = vk["wbits"], vk["y"], len(vk["y"])
    n, ones = nwin(wbits), (1 << wbits) - 1
    hid = [i for i in range(q) if i not in revealed]
    nh, nr = len(hid), len(revealed)
    rng = random.Random(31 * wbits + 7 * nr + vk["mode"] + 1000 * sum(revealed))
    fr = lambda: rng.randrange(1 << 250, R)  # noqa: E731
    take = lambda lst, k: [lst[i % len(lst)] for i in range(k)]  # noqa: E731
    cases = []

    def case(name, resp, rev=None, chal=None, r2=None, msgs=None):
        msgs = list(msgs) if msgs else [fr() for _ in range(q)]
        rev = list(rev) if rev is not None else [msgs[i] for i in revealed]
        for z, i in enumerate(revealed):
            msgs[i] = rev[z] % R
        cases.append(dict(name=name, resp=[int(v) for v in resp], chal=fr() if chal is None else chal, rev=rev,
                          msgs=msgs, r2=fr() if r2 is None else r2))

    hsum = lambda rs: sum(a * y[i] for a, i in zip(rs, hid)) % R  # noqa: E731
    rnd = [fr() for _ in range(nh)]
    case("random", [fr()] + rnd)
    case("resp_zero", [0] * (nh + 1))
    case("resp_r_minus_1", [R - 1] * (nh + 1))
    case("resp_small", take([18, 1990, 7, 1, 2, 3, 4], nh + 1))
    case("resp_noncanon", take([R + 5, R, (1 << 256) - 1, (1 << 384) - 1, 2 * R + 7, R - 1, R + 1], nh + 1))
    case("chal_zero", [fr()] + rnd, chal=0)
    if nh:
        case("roleA_zero", [0] + rnd)  # g~'s response 0: role A's table sum is empty
        case("roleB_zero", [fr()] + [0] * nh)  # every hidden response 0
        case("roles_opposite", [(R - hsum(rnd)) % R] + rnd)  # rho_0 g~ = -sum rho_k Y~_k
        case("roles_equal", [hsum(rnd)] + rnd)
    if 0 in hid and 2 in hid and 3 in hid:
        i0, i2, i3 = hid.index(0) + 1, hid.index(2) + 1, hid.index(3) + 1
        v = [0] * (nh + 1)
        v[i0], v[i2], v[nh] = 9 << wbits, (9 << wbits) | (5 << (wbits * (n // 2))), 77
        case("chain_cancel", v)  # Y~_2 = -Y~_0: to the identity, and on from it
        v = [0] * (nh + 1)
        v[i0], v[i3], v[nh] = 6 << (3 * wbits), (6 << wbits) | (ones << (4 * wbits)), 5
        case("chain_doubling", v)  # entry (3, 1, 6) = entry (0, 3, 6)
        # the same two equal terms alone, in windows that put them on two lanes (pairs) of the one-block
        # prep whose partial sums meet in the butterfly before -T's lane joins them: a doubling there
        for w in range(n - 3):
            v = [0] * (nh + 1)
            v[i0], v[i3] = 6 << ((w + 2) * wbits), 6 << (w * wbits)
            case("lanes_equal", v)
            if "doubling" in trace_pok(vk, cases[-1], revealed, "wide")["join"]:
                break
            cases.pop()
    if nr:
        case("rev_zero", [fr()] + rnd, rev=[0] * nr)
        case("rev_small", [fr()] + rnd, rev=take([18, 1990, 7, 1, 2, 3], nr))
        case("rev_r_minus_1", [fr()] + rnd, rev=[R - 1] * nr)
        case("rev_noncanon", [fr()] + rnd, rev=take([R + 5, (1 << 384) - 1, R, (1 << 256) - 1, 2 * R + 7, R + 1], nr))
    # J' = X~ + J + sum revealed = identity: r2 = -(x + sum_all y_i m_i); sigma'_2 is then the identity
    msgs = [fr() for _ in range(q)]
    case("jprime_identity", [fr()] + rnd, msgs=msgs, r2=(R - (vk["x"] + sum(a * b for a, b in zip(y, msgs))) % R) % R)
    return cases


def pok_batch_inputs(oc, vk, cases, revealed, seed=3):
    """Each case three ways: valid, one response off by one, sigma'_2 off by the generator (its GT pins
    J').  sigma' = (r1 k G, r1 k (s + r2) G), J = (r2 + sum_hidden y_i m_i) g~, T = sum rho_k B_k + c J."""
    mode = vk["mode"]
    og, sg = (1, 2) if mode == 0 else (2, 1)
    hid = [i for i in range(len(vk["y"])) if i not in revealed]
    rng = random.Random(seed)
    y, gk = vk["y"], vk["gk"]
    e1, e2, ej, et, resp, chal, rev, names = [], [], [], [], [], [], [], []
    for c in cases:
        k, r1 = rng.randrange(1 << 250, R), rng.randrange(1 << 250, R)
        s = (vk["x"] + sum(a * b for a, b in zip(y, c["msgs"]))) % R
        jlog = (c["r2"] + sum(y[i] * c["msgs"][i] for i in hid)) % R
        ylog = [1] + [y[i] for i in hid]
        tlog = (sum(a * (b % R) for a, b in zip(ylog, c["resp"])) + (c["chal"] % R) * jlog) % R
        for kind in ("valid", "resp_off_by_1", "sigma2_off_by_g"):
            rs = list(c["resp"])
            if kind == "resp_off_by_1":
                rs[-1] = (rs[-1] % R + 1) % R
            e1.append(k * r1)
            e2.append(k * r1 * (s + c["r2"]) + (kind == "sigma2_off_by_g"))
            ej.append(gk * jlog)
            et.append(gk * tlog)
            resp.append(b"".join(be48(v) for v in rs))
            chal.append(be48(c["chal"]))
            rev.append(b"".join(be48(v) for v in c["rev"]))
            names.append(f"{c['name']}/{kind}")
    return dict(names=names, n=len(names), nresp=len(hid) + 1, revealed=list(revealed), s1=gen_mul(oc, sg, e1),
                s2=gen_mul(oc, sg, e2), J=gen_mul(oc, og, ej), T=gen_mul(oc, og, et), resp=b"".join(resp),
                chal=b"".join(chal), rev=b"".join(rev))


def oracle_pok(oc, vk, vkb, b):
    """[(verdict, GT bytes or None)] from oc_pok_verify (it leaves no GT where it rejects before the
    pairing: an identity sigma' or a failed Schnorr check)."""
    mode = vk["mode"]
    sb, ob = (192, 97) if mode == 0 else (97, 192)
    r, nr = len(b["revealed"]), b["nresp"]
    idx = (ctypes.c_uint64 * max(r, 1))(*b["revealed"])
    out = []
    for i in range(b["n"]):
        gt = ctypes.create_string_buffer(576)
        v = oc.oc_pok_verify(mode, _sz(len(vk["y"])), _sz(r), b["s1"][i * sb:(i + 1) * sb], b["s2"][i * sb:(i + 1) * sb],
                             b["J"][i * ob:(i + 1) * ob], b["T"][i * ob:(i + 1) * ob],
                             b["resp"][i * nr * 48:(i + 1) * nr * 48], _sz(nr), b["chal"][48 * i:48 * (i + 1)], idx,
                             b["rev"][i * r * 48:(i + 1) * r * 48], vkb[0], vkb[1], vkb[2], gt)
        out.append((v, gt.raw if any(gt.raw) else None))
    return out


def trace_pok(vk, c, revealed, layout):
    """The table additions of one proof's Schnorr sum and of J' in a PoK prep layout:
    'split' k_prep_pok_split (SigG2: role A takes g~ and the first `split` hidden responses, role B the
            rest; each role one chain), 'pair' k_prep_pok_g1pl (SigG1: one chain),
    'wide'  k_prep_pok_wide_*: term (response s, window w) on lane (pair) (s nwin + w) mod L, the J' terms
            continue the rotation; lane_group_sum / pair_group_sum butterflies (-T and X~ + J, which are
            not table terms: -T is added on the last lane (pair) before the Schnorr butterfly and is part of
            that lane's operand here; X~ + J belongs to the J' butterfly, which is not modelled).
    Returns dict(chain, join, jchain, roles=(A, B) table sums as multiples of the generator)."""
    wbits, mode, y, gk = vk["wbits"], vk["mode"], vk["y"], vk["gk"]
    n, q = nwin(wbits), len(y)
    hid = [i for i in range(q) if i not in revealed]
    bases = [gk] + [gk * y[i] % R for i in hid]
    dg = [digits(v, wbits) for v in c["resp"]]
    rdg = [digits(v, wbits) for v in c["rev"]]
    rbase = [gk * y[i] % R for i in revealed]
    chain, jn, jchain = [], [], []

    def run(cn, terms, d, b, log):
        for s, w in terms:
            if d[s][w]:
                cn.add(entry(b[s], w, d[s][w], wbits))
        log.extend(cn.log)
        return cn.acc

    jlog = (c["r2"] + sum(y[i] * c["msgs"][i] for i in hid)) % R
    jstart = (gk * vk["x"] + gk * jlog) % R  # X~ + J before the revealed terms
    if layout == "wide":
        L = 64 if mode == 0 else 32
        lanes = []
        for l in range(L):
            ts = [(s, w) for s in range(len(bases)) for w in range(n) if (s * n + w) % L == l]
            lanes.append(run(Chain(0), ts, dg, bases, chain))
        ylog = [1] + [y[i] for i in hid]
        tlog = gk * (sum(a * (b % R) for a, b in zip(ylog, c["resp"])) + (c["chal"] % R) * jlog) % R
        lanes[L - 1] = (lanes[L - 1] - tlog) % R  # jac_add_aff(acc, -T) on lane 63 / pair 31
        butterfly_high_first(lanes, jn)
        for l in range(L):
            ts = [(z, w) for z in range(len(rbase)) for w in range(n) if ((len(bases) + z) * n + w) % L == l]
            run(Chain(0), ts, rdg, rbase, jchain)
        A = bases[0] * c["resp"][0] % R
        B = sum(bases[s] * c["resp"][s] for s in range(1, len(bases))) % R
        return dict(chain=chain, join=jn, jchain=jchain, roles=(A, B))
    split = pok_split(q, len(revealed), wbits) if layout == "split" else len(hid)
    allw = lambda ss: [(s, w) for s in ss for w in range(n)]  # noqa: E731
    A = run(Chain(0), allw(range(0, 1 + split)), dg, bases, chain)
    B = run(Chain(0), allw(range(1 + split, len(bases))), dg, bases, chain) if layout == "split" else 0
    if layout == "split":
        join(A, B, jn)  # (the device joins A + chal J with B - T; the table sums meet there)
    run(Chain(jstart), allw(range(len(rbase))), rdg, rbase, jchain)
    return dict(chain=chain, join=jn, jchain=jchain, roles=(A, B))


# ---------------------------------------------------------------- cc_fixed_base_mul
def fbm_scalars():
    """Encoded scalars for cc_fixed_base_mul's 8-bit tables (32 windows of one byte)."""
    return [0, 1, 2, R - 1, R, R + 1, 1 << 255, (1 << 384) - 1, int("01" * 32, 16), ((1 << 256) - 1) % R] + \
        [0xFF << (8 * k) for k in (0, 15, 31)]


def fbm_bases(oc, group):
    """[(name, encoding)]: the generator, a random point, the identity encoding, an off-curve encoding
    (which decodes to the identity)."""
    gen, ident = (G1_GENERATOR, G1_IDENTITY) if group == 1 else (G2_GENERATOR, G2_IDENTITY)
    rnd = gen_mul(oc, group, [random.Random(55 + group).randrange(1 << 250, R)])
    off = bytearray(gen)
    off[-1] ^= 1
    return [("generator", gen), ("random", rnd), ("identity", ident), ("off_curve", bytes(off))]


def oracle_mul(oc, group, base, scalars):
    """oc_msm(group, 1, base, k) for every encoded scalar k, concatenated."""
    eb = 97 if group == 1 else 192
    out = b""
    for k in scalars:
        o = ctypes.create_string_buffer(eb)
        oc.oc_msm(group, _sz(1), base, be48(k), o)
        out += o.raw
    return out
