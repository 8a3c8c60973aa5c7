"""Inputs and the exact model of the RLC batch mode's g~-side fold (csrc/fold.hip) and finish (rlc.hip
k_rlc_gather, fold.hip k_fold_fixed, miller_wide.hip), shared by tests/test_rlc_fold_model.py (CPU) and
tests/test_gpu_rlc_fold_direct.py (device).  Plain Python: the delta key stream of
test_pok_rlc_model.rlc_delta_signed and the curve and pairing of oracle/bls12_381.py.

THE MODEL.  Credential i of a launch with (seed, base_index) gets the 16 signed digits d_w,i of the key
stream's block base_index + i; its fold point is X_i = -sigma_2,i; window w of the partial holds
S_w = sum_i d_w,i X_i, affine, in the storage form x 2^406 mod p (tests/fexp_direct_cases.py), twelve
little-endian 32-bit words a coordinate (SigG1: x, y, 24 zero words; SigG2: x.a, x.b, y.a, y.b), then the
identity flag; the identity is 48 zero words and flag 1 (rlc_part.h).

THE CASES.  A valid credential (sigma_1, sigma_2) stays valid as (k sigma_1, k sigma_2) for k != 0 mod r,
so every valid case is a list of multipliers k_i over ONE fixture credential: X_i = k_i X with
X = -sigma_2, every bucket, lane and window sum is a known multiple of X, and a case places equal, opposite
and proportional points wherever the fold is to meet them while the batch stays valid.  S_w is then one
scalar multiplication, (sum_i d_w,i k_i mod r) X.

THE MIRROR.  `mirror` walks the fold's structure on those multiples (integers mod r): bucket lists in
chunks of FS = 16, the chunk and bucket additions, the window kernels' running sums over the CK digits of a
lane (SigG1, CK = 2) or lane pair (SigG2, CK = 4) -- a "unit" below -- the final u + v, and the butterfly
whose partner at step m is unit t ^ m.  It records what kind every addition is (a doubling, a sum to the
identity, an identity operand, generic), so the CPU test can show that a case reaches the branch it names.
It proves nothing about the device; the device is compared with the window sums only.

The base indices below were found once by a search over the key stream for the digit patterns the cases
need (each has probability >= 1/256 a candidate); tests/test_rlc_fold_model.py asserts every pattern."""
import functools
import random

import numpy as np

from conftest import golden
from oracle import bls12_381 as B
from test_pok_rlc_model import rlc_delta_signed

P, R = B.P, B.R
Q = 6
MODES = ("G2", "G1")
SEED = bytes((29 * k + 7) & 0xFF for k in range(32))
FW, FD, FS = 16, 128, 16          # fold.hip: windows, |digit| values a window, list entries a chunk
CK = {"G2": 4, "G1": 2}           # digits a unit: a lane pair of k_fold_window_g2pl, a lane of k_fold_window
UNITS = {"G2": 32, "G1": 64}      # units a window wave
UNIT_LANES = {"G2": 2, "G1": 1}   # butterfly step m of the kernels, in lanes, is UNIT_LANES x the unit step
R_STORE = pow(2, 406, P)
R_STORE_INV = pow(R_STORE, -1, P)
NW = 12
WIN_OFF, WIN_WORDS, PART_WORDS, FLAG = 145, 49, 929, 144
# 2^406 mod p as the kernels store it (tests/test_gpu_rlc.py test_empty_shard_partial_is_neutral)
ONE_WORDS = (0x03a9fb84, 0xc57400d2, 0x629c4a23, 0x6147acde, 0x7e6d26cb, 0x6b0f4b0b, 0xc2b7d6e1, 0x91ecbde7,
             0x4fdd80b8, 0xd56a23c3, 0xf3a0d636, 0x13317c30)
HIGH = 1 << 40

# ---------------------------------------------------------------- committed search results
# n = 1 launches whose digits together hold 0, -128, 127, +1, -1, +-4 and +-8
SINGLE_BASES = (303, 1406)
# first index of each two-credential pattern, by mode (the patterns: the predicates below)
BASES = {
    "G2": {"same_bucket": 12, "same_lane": 4, "partner_hi": 6, "partner_lo": 4, "high_index": HIGH + 8},
    "G1": {"same_bucket": 12, "same_lane": 12, "partner_hi": 6, "partner_lo": 4, "high_index": HIGH + 12},
}
COPIES_BASE = 1000
CHUNKS_N, CHUNKS_BASE = 2163, 5000
CHUNK_COUNTS = (15, 16, 17, 32, 33)
FILL = (2, 3, 5, 7)   # multipliers of the four credentials put in front of a two-credential case to split it


# ---------------------------------------------------------------- the key stream
def digits(seed, base_index, n):
    """n x 16 signed digits: row i is credential i's d_0 .. d_15."""
    return [rlc_delta_signed(seed, base_index + i)[1] for i in range(n)]


def deltas(seed, base_index, n):
    return [rlc_delta_signed(seed, base_index + i)[0] for i in range(n)]


def unit_of(mode, d):
    """The lane (SigG1) or lane pair (SigG2) of the window kernels that holds digit d != 0."""
    return (abs(d) - 1) // CK[mode]


def sgn(d):
    return -1 if d < 0 else 1


# the digit patterns of two consecutive credentials (rows a, b): the first window that has the pattern
def find_same_bucket(mode, a, b):
    return next((w for w in range(FW) if a[w] == b[w] != 0), None)


def find_same_lane(mode, a, b):
    return next((w for w in range(FW) if a[w] and b[w] and abs(a[w]) != abs(b[w])
                 and unit_of(mode, a[w]) == unit_of(mode, b[w])), None)


def find_partner(mode, a, b, hi):
    """The two digits sit in units whose butterfly paths first meet at the first step (unit distance
    UNITS / 2: lane step m = 32) when hi, at the last (lane step m = 1 in SigG1, 2 in SigG2) otherwise."""
    for w in range(FW):
        if a[w] and b[w]:
            x = unit_of(mode, a[w]) ^ unit_of(mode, b[w])
            if (x == UNITS[mode] // 2) if hi else (x & 1):
                return w
    return None


def meeting_step(ta, tb):
    """Unit step at which the butterfly first adds the sums of units ta != tb: the lowest set bit of ta ^ tb
    (after the steps above it every unit holds the sum of the units equal to it in the lower bits)."""
    x = ta ^ tb
    return x & -x


# ---------------------------------------------------------------- curve helpers
def curve(mode):
    return B.G2 if mode == "G2" else B.G1


def smul(cv, pt, k):
    """k pt with k mod r, through the shorter of k and r - k."""
    k %= R
    return cv.neg(cv.mul(pt, R - k)) if k > R // 2 else cv.mul(pt, k)


def _codec(mode):
    return (B.g2_from_bytes, B.g2_to_bytes) if mode == "G2" else (B.g1_from_bytes, B.g1_to_bytes)


@functools.lru_cache(maxsize=None)
def fixture(mode):
    return golden(f"verify_{mode.lower()}_q6.json")


def valid_creds(mode):
    return [c for c in fixture(mode)["creds"] if c["kind"] == "valid"]


@functools.lru_cache(maxsize=None)
def base_points(mode):
    """(sigma_1, sigma_2) of the fixture's first valid credential, decoded."""
    c = valid_creds(mode)[0]
    dec = _codec(mode)[0]
    return dec(bytes.fromhex(c["sigma1"])), dec(bytes.fromhex(c["sigma2"]))


def base_msgs(mode):
    return b"".join(bytes.fromhex(m) for m in valid_creds(mode)[0]["msgs"])


@functools.lru_cache(maxsize=None)
def X(mode):
    """The fold point of the base credential, -sigma_2."""
    return curve(mode).neg(base_points(mode)[1])


@functools.lru_cache(maxsize=None)
def cred_bytes(mode, k):
    """(k sigma_1, k sigma_2) of the base credential, encoded (the Python oracle's multiplication)."""
    s1, s2 = base_points(mode)
    cv, enc = curve(mode), _codec(mode)[1]
    return enc(smul(cv, s1, k)), enc(smul(cv, s2, k))


def inputs(mode, ks):
    """(sigma_1, sigma_2, msgs) bytes of the credentials k_i x base credential."""
    cb = [cred_bytes(mode, k % R) for k in ks]
    return b"".join(c[0] for c in cb), b"".join(c[1] for c in cb), base_msgs(mode) * len(ks)


# ---------------------------------------------------------------- window sums
def window_sums(mode, points, dig):
    """S_w = sum_i d_w,i points[i] (points: the fold points -sigma_2,i), None for the identity."""
    cv = curve(mode)
    out = []
    for w in range(FW):
        acc = None
        for pt, d in zip(points, dig):
            if d[w]:
                acc = cv.add(acc, smul(cv, pt, d[w]))
        out.append(acc)
    return out


def window_scalars(ks, dig):
    """s_w = sum_i d_w,i k_i mod r: S_w = s_w X where every fold point is k_i X."""
    return [sum(d[w] * k for d, k in zip(dig, ks)) % R for w in range(FW)]


@functools.lru_cache(maxsize=None)
def multiple_of_X(mode, s):
    return smul(curve(mode), X(mode), s) if s % R else None


def window_sums_of_multiples(mode, ks, dig):
    return [multiple_of_X(mode, s) for s in window_scalars(ks, dig)]


# ---------------------------------------------------------------- the partial's words
def _fp_words(x):
    v = x * R_STORE % P
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(NW)]


def _fp_from_words(ws):
    v = sum(int(x) << (32 * k) for k, x in enumerate(ws))
    assert v < P, "non-canonical stored coordinate"
    return v * R_STORE_INV % P


def partial_words(mode, S):
    """The 49 words of one window as the kernels write them."""
    if S is None:
        return [0] * 48 + [1]
    x, y = S
    if mode == "G2":
        return _fp_words(x[0]) + _fp_words(x[1]) + _fp_words(y[0]) + _fp_words(y[1]) + [0]
    return _fp_words(x) + _fp_words(y) + [0] * 24 + [0]


def window_point(mode, ws):
    """Inverse of partial_words: the point, or None; every stored coordinate must be < p."""
    ws = [int(x) for x in ws]
    assert len(ws) == WIN_WORDS and ws[48] in (0, 1)
    c = [_fp_from_words(ws[NW * j:NW * (j + 1)]) for j in range(4)]
    if ws[48]:
        assert not any(ws[:48])
        return None
    if mode == "G2":
        return ((c[0], c[1]), (c[2], c[3]))
    assert c[2] == c[3] == 0
    return (c[0], c[1])


def windows_words(mode, sums):
    """Words [145, 929) of a partial: the 16 windows."""
    return np.array([x for S in sums for x in partial_words(mode, S)], dtype=np.uint32)


def hand_partial(mode, sums):
    """A whole partial with the Miller product one, a clear flag and the given window sums."""
    p = np.zeros(PART_WORDS, dtype=np.uint32)
    p[:NW] = ONE_WORDS
    p[WIN_OFF:] = windows_words(mode, sums)
    return p


# ---------------------------------------------------------------- the mirror of the fold's structure
def _kind(a, b):
    if a == 0 or b == 0:
        return "id"
    if a == b:
        return "dbl"
    return "inf" if (a + b) % R == 0 else "add"


def _butterfly(vals, ev, stage, mode):
    """lane_group_sum / pair_group_sum over len(vals) units; the value every unit ends with."""
    vals = list(vals)
    m = len(vals) // 2
    while m:
        nxt = list(vals)
        for t in range(len(vals)):
            lo, hi = min(t, t ^ m), max(t, t ^ m)
            if t == lo:
                ev.append((stage, (m * UNIT_LANES[mode], t), _kind(vals[lo], vals[hi])))
            nxt[t] = (vals[lo] + vals[hi]) % R
        vals = nxt
        m //= 2
    assert len(set(vals)) == 1
    return vals[0]


def mirror(mode, ks, dig):
    """One dict a window: counts[b] entries of bucket b (|digit| b + 1), buckets[b] the bucket's multiple
    of X, shares[t] unit t's share, S the window's multiple, events [(stage, where, kind)] with stage in
    sum (a chunk's mixed additions, in list order = credential order here; the device's order inside a
    bucket is the scatter's), reduce (a bucket's chunk partials), run / u / uv (the window kernels'
    recurrences and final addition of a unit), bfly (the window's butterfly; where = (lane step m, unit))."""
    ck, nu = CK[mode], UNITS[mode]
    out = []
    for w in range(FW):
        ev = []
        lists = [[] for _ in range(FD)]
        for d, k in zip(dig, ks):
            if d[w]:
                lists[abs(d[w]) - 1].append(sgn(d[w]) * k % R)
        buckets = []
        for b, lst in enumerate(lists):
            chunks = []
            for c in range(0, len(lst), FS):
                acc = 0
                for e, v in enumerate(lst[c:c + FS]):
                    ev.append(("sum", (b, c // FS, e), _kind(acc, v)))
                    acc = (acc + v) % R
                chunks.append(acc)
            if not chunks:
                buckets.append(0)
                continue
            lanes = [0] * nu
            for c, v in enumerate(chunks):      # lane-strided, then the butterfly
                ev.append(("reduce", (b, c), _kind(lanes[c % nu], v)))
                lanes[c % nu] = (lanes[c % nu] + v) % R
            sub = []
            tot = _butterfly(lanes, sub, "reduce", mode)
            ev += [(s, (b,) + wh, kd) for s, wh, kd in sub if kd != "id"]
            buckets.append(tot)
        shares = []
        for t in range(nu):
            run = u = 0
            for k in range(ck - 1, -1, -1):
                bk = buckets[ck * t + k]
                ev.append(("run", (t, k), _kind(run, bk)))
                run = (run + bk) % R
                ev.append(("u", (t, k), _kind(u, run)))
                u = (u + run) % R
            v = ck * t * run % R
            ev.append(("uv", t, _kind(u, v)))
            shares.append((u + v) % R)
        S = _butterfly(shares, ev, "bfly", mode)
        assert S == window_scalars(ks, dig)[w]
        out.append({"counts": [len(x) for x in lists], "buckets": buckets, "shares": shares, "S": S,
                    "events": [e for e in ev if e[2] != "id"]})
    return out


# ---------------------------------------------------------------- the valid cases
class Case:
    """n credentials k_i x base credential, launched at base_index; wstar: the window the case is about."""

    def __init__(self, name, base_index, ks, wstar=None):
        self.name, self.base_index, self.ks, self.wstar = name, base_index, tuple(k % R for k in ks), wstar
        self.n = len(ks)

    def __repr__(self):
        return f"Case({self.name})"

    def dig(self, lo=0, hi=None):
        return _digits_cached(self.base_index + lo, (self.n if hi is None else hi) - lo)

    def expected(self, mode, lo=0, hi=None):
        """Words [145, 929) of the partial of credentials [lo, hi) launched at base_index + lo."""
        hi = self.n if hi is None else hi
        return windows_words(mode, window_sums_of_multiples(mode, self.ks[lo:hi], self.dig(lo, hi)))

    def split(self):
        """(case, seg) whose partial_seg(seg) has at least two segments: a two-credential case gets four
        credentials (FILL x base credential) in front and starts four indices earlier, so that segment 1 at
        seg = 4 is the case itself; longer cases are cut where they lie.  None for n = 1."""
        if self.n == 1:
            return None
        if self.n == 2:
            return Case(self.name + "+fill", self.base_index - 4, FILL + self.ks, self.wstar), 4
        return self, 16 if self.n <= 64 else 2048


@functools.lru_cache(maxsize=None)
def _digits_cached(base_index, n):
    return digits(SEED, base_index, n)


def chunk_ks(n):
    """n distinct multipliers (k_i = A (i + 1) mod r, A a fixed 250-bit constant)."""
    a = random.Random(0xF01D).getrandbits(250) | 1
    return [a * (i + 1) % R for i in range(n)]


def _ratio(da, db):
    """k with db k X = da X: the second credential's multiplier that makes its digit's share equal the first's."""
    return da * pow(db, -1, R) % R


@functools.lru_cache(maxsize=None)
def cases(mode):
    """name -> Case.  single_<base>: n = 1 launches.  The two-credential cases take their window from the
    committed base index's digits (the model test asserts the pattern is there)."""
    out = [Case(f"single_{b}", b, (1,)) for b in SINGLE_BASES]
    bs = BASES[mode]

    def two(name, key, find, mult):
        base = bs[key]
        a, b = _digits_cached(base, 2)
        w = find(mode, a, b)
        assert w is not None, (mode, name, base)
        for tag, s in (("eq", 1), ("op", -1)):
            out.append(Case(f"{name}_{tag}", base, (1, s * mult(a[w], b[w])), w))

    two("same_bucket", "same_bucket", find_same_bucket, lambda da, db: 1)
    two("same_lane", "same_lane", find_same_lane, _ratio)
    # the same digits with B_hi = +-B_lo: the running sum itself meets equal and opposite operands
    two("same_lane_run", "same_lane", find_same_lane, lambda da, db: sgn(da) * sgn(db))
    two("partner_hi", "partner_hi", lambda m, a, b: find_partner(m, a, b, True), _ratio)
    two("partner_lo", "partner_lo", lambda m, a, b: find_partner(m, a, b, False), _ratio)
    two("high_index", "high_index", lambda m, a, b: find_partner(m, a, b, True), _ratio)
    out.append(Case("copies", COPIES_BASE, (1, -1) * 32))
    out.append(Case("chunks", CHUNKS_BASE, chunk_ks(CHUNKS_N)))
    assert len({c.name for c in out}) == len(out)
    return {c.name: c for c in out}


def small_cases(mode):
    """Every case the Python oracle can build credentials for (n <= 64)."""
    return [c for c in cases(mode).values() if c.n <= 64]


# ---------------------------------------------------------------- the rejecting batches
REJECT_BASE = 77
REJECTS = {
    # name: (bad fixture kinds by position, total n): the first six valid credentials with the bad ones put in
    "reject_one": {3: "msg_plus_1"},
    "reject_two": {0: "msg_plus_1", 5: "sigma2_plus_g"},
}


@functools.lru_cache(maxsize=None)
def reject_creds(mode, name):
    """The fixture credentials of a rejecting batch, in order, and the bad positions."""
    bad = REJECTS[name]
    creds = list(valid_creds(mode)[:6])
    for pos in sorted(bad):
        creds.insert(pos, next(c for c in fixture(mode)["creds"] if c["kind"] == bad[pos]))
    assert [i for i, c in enumerate(creds) if c["verdict"] == 0] == sorted(bad)
    return tuple(creds), tuple(sorted(bad))


def reject_inputs(mode, name):
    cr, _ = reject_creds(mode, name)
    cat = lambda hs: b"".join(bytes.fromhex(h) for h in hs)  # noqa: E731
    return cat(c["sigma1"] for c in cr), cat(c["sigma2"] for c in cr), cat(m for c in cr for m in c["msgs"])


@functools.lru_cache(maxsize=None)
def reject_windows(mode, name):
    cr, _ = reject_creds(mode, name)
    dec, cv = _codec(mode)[0], curve(mode)
    pts = [cv.neg(dec(bytes.fromhex(c["sigma2"]))) for c in cr]
    return windows_words(mode, window_sums(mode, pts, digits(SEED, REJECT_BASE, len(cr))))


@functools.lru_cache(maxsize=None)
def reject_gt(mode, name):
    """GT bytes the finish must give: prod over the bad credentials of gt_i^(delta_i mod r), gt_i the
    fixture's own per-credential GT (a valid credential's factor is one)."""
    cr, bad = reject_creds(mode, name)
    dl = deltas(SEED, REJECT_BASE, len(cr))
    f = B.f12_one()
    for i in bad:
        f = B.f12_mul(f, B.f12_pow(B.gt_from_bytes(bytes.fromhex(cr[i]["gt"])), dl[i] % R))
    return B.gt_to_bytes(f)


# ---------------------------------------------------------------- hand-built partials for the finish
def _hand_scalars():
    rnd = random.Random(0xF1A15)
    full = [rnd.randrange(1, R) for _ in range(FW)]
    s1 = rnd.randrange(1, R)
    return {
        "all_finite": full,
        "interleaved": [full[w] if w % 2 == 0 else 0 for w in range(FW)],
        "interleaved_odd": [0 if w % 2 == 0 else full[FW - 1 - w] for w in range(FW)],
        "same_point": [full[3]] * FW,
        "only_15": [0] * 15 + [full[7]],
        "cancels": [-256 * s1 % R, s1] + [0] * 14,    # S_0 = -256 S_1: the weighted sum is the identity
        "neutral": [0] * FW,
    }


HAND = _hand_scalars()
# the gathered sets (k = 2) of the finish test
HAND_PAIRS = (("all_finite", "interleaved"), ("same_point", "only_15"), ("interleaved_odd", "all_finite"),
              ("cancels", "neutral"), ("only_15", "neutral"))


def hand_total(names):
    """sum over the partials of sum_w 256^w s_w mod r: the finish pairs (that multiple of X) with g~."""
    return sum(s << (8 * w) for nm in names for w, s in enumerate(HAND[nm])) % R


def hand_partials(mode, names):
    return np.stack([hand_partial(mode, [multiple_of_X(mode, s) for s in HAND[nm]]) for nm in names])


@functools.lru_cache(maxsize=None)
def hand_gt(mode, names):
    """(GT bytes, accept) of the finish over the named hand-built partials: e(sum_w 256^w S_w, g~) with S in
    G2 and g~ in G1 (SigG2), the arguments swapped in SigG1."""
    S = multiple_of_X(mode, hand_total(names))
    g = bytes.fromhex(fixture(mode)["g_tilde"])
    gt = B.pairing(B.g1_from_bytes(g), S) if mode == "G2" else B.pairing(S, B.g2_from_bytes(g))
    return B.gt_to_bytes(gt), int(S is None)
