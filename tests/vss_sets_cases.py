"""Cases of verify_share over commitment SETS (cc_vss_verify_sets(_device), cc_keygen_verify_shares_batch_device;
csrc/vss.hip): the CSR form of tests/issuer_edges.py's vss_call lists, and three lists of their own.

A call is issuer_edges' dict(t, g, h, sets: [[C_k encodings]], cases: [dict(name, set, id, s, st, intent)]);
csr() sorts a batch's rows by set and returns the offsets.

TORSION SETS (torsion_calls).  The fast path replaces sum_k (id^k mod r) C_k by Horner with id as a plain
integer, which is the same element only for points of order r.  For a commitment honest + T with T of order 3
or 11 the two differ by ((id^k mod r) - id^k) T, and for id = 2^64 - 1

    id^4 mod r = 1 (mod 3)   while id^4 = 0 (mod 3)
    id^4 mod r = 1 (mod 11)  while id^4 = 3 (mod 11),   id^5 mod r = 0 (mod 11) while id^5 = 1 (mod 11)

so with C_4 = honest + T3 an honest share is INVALID by the reference and valid by integer Horner, and with
C_0 = honest + T3, C_4 = honest - T3 it is valid by the reference and invalid by integer Horner.  A kernel
without the subgroup gate fails one of them whichever way it errs.  Expected verdicts: the C oracle's MSM
with the scalars pow(id, k, R) (issuer_edges.expect_share); horner_verdict() is the other opinion.

CANCELLING ERRORS (cancel_call).  Two shares of one set with s + 1 and s - 1 (and two with s' + 1 and s' - 1):
their defects s g + s' h - sum id^k C_k are +g and -g, so an UNWEIGHTED sum over the set would accept; the
RLC's independent deltas do not.

SET SIZES (sizes_call).  Sets of 0, 1, 2, 63, 64, 65, 130 and 257 shares in one call, one bad share at the
first row, the last row and at row 256 of the call (a block boundary of the per-share kernel) of chosen sets.
"""
import functools
import random

import issuer_edges as E
from fixed_edges import R, be48
from torsion_edges import fixture as torsion_fixture

TORSION_IDS = ((1 << 64) - 1, 2)
SIZES = (0, 1, 2, 63, 64, 65, 130, 257)
# set size -> rows of the set holding a bad share (row 61 of the 130-set is row 256 of the call)
SIZES_BAD = {2: (0,), 63: (62,), 130: (61,), 257: (0, 256)}
_OC = {}


def csr(call, batch):
    """(rows of the batch sorted by set, set_begin over every set of the call)."""
    rows = sorted(batch, key=lambda c: c["set"])  # stable: a set's rows keep their order
    begin = [0] * (len(call["sets"]) + 1)
    for c in rows:
        begin[c["set"] + 1] += 1
    for j in range(len(call["sets"])):
        begin[j + 1] += begin[j]
    return rows, begin


def sets_args(call, rows, begin):
    """The arguments of coconut.vss_verify_sets after ctx (rlc excepted)."""
    return (call["t"], call["sets"], begin, [c["id"] for c in rows], [(be48(c["s"]), be48(c["st"])) for c in rows])


def batch_args(call, rows):
    """The same rows for coconut.vss_verify_batch (after ctx)."""
    return (call["t"], call["g"], call["h"], call["sets"], [c["set"] for c in rows], [c["id"] for c in rows],
            [(be48(c["s"]), be48(c["st"])) for c in rows])


def _coef(rng, t):
    return [(rng.randrange(1 << 250, R), rng.randrange(1 << 250, R)) for _ in range(t)]


def _share(coef, i):
    return E._poly([a for a, _ in coef], i), E._poly([b for _, b in coef], i)


def _commit(env, g, h, coef):
    return [env.msm([g, h], [a, b]) for a, b in coef]


def _plus(env, a, b):
    return env.msm([a, b], [1, 1])


def _call(t, g, h, sets, cases):
    return dict(t=t, hkind="rand", g=g, h=h, sets=sets, cases=cases)


def torsion_calls(oc):
    """[dict(name, call, irregular: the sets the device must report irregular)]: a call under g, h in G1 with
    one regular set and the torsion sets, and a call whose g is kG + T3 (every set irregular)."""
    _OC[id(oc)] = oc
    return _torsion_calls(id(oc))


@functools.lru_cache(maxsize=None)
def _torsion_calls(oc_key):
    env = E.Env(_OC[oc_key], 1)
    tor = torsion_fixture()["G1"]
    T3, nT3, T11 = tor["T3"]["point"], tor["-T3"]["point"], tor["T11"]["point"]
    rng = random.Random(9100)
    t = 5
    g, h = env.muls([rng.randrange(1 << 250, R), rng.randrange(1 << 250, R)])
    out = []

    def build(name, g, h, shapes):
        sets, cases = [], []
        for sname, tweak in shapes:
            coef = _coef(rng, t)
            enc = _commit(env, g, h, coef)
            for k, T in tweak:
                enc[k] = _plus(env, enc[k], T)
            sets.append(enc)
            for i in TORSION_IDS:
                s, st = _share(coef, i)
                cases.append(dict(name=f"{sname}/honest_id_{i:x}", set=len(sets) - 1, id=i, s=s, st=st, intent=None))
                cases.append(dict(name=f"{sname}/s_plus_1_id_{i:x}", set=len(sets) - 1, id=i, s=(s + 1) % R, st=st,
                                  intent=None))
        return dict(name=name, call=_call(t, g, h, sets, cases))

    c = build("commitments", g, h, (("regular", ()), ("c4_plus_T3", ((4, T3),)),
                                    ("c0_plus_c4_minus_T3", ((0, T3), (4, nT3))), ("c4_plus_T11", ((4, T11),)),
                                    ("c1_is_mixed", ())))
    # one commitment replaced by the fixture's k G + T11 itself (an honest share no longer fits it: both invalid)
    c["call"]["sets"][4][1] = tor["kG+T11"]["point"]
    c["irregular"] = [1, 2, 3, 4]
    out.append(c)
    c = build("g_is_kG_plus_T3", tor["kG+T3"]["point"], h, (("a", ()), ("b", ())))
    c["irregular"] = [0, 1]
    out.append(c)
    return out


def horner_verdict(env, call, c):
    """The share equation with Horner over the INTEGER id (no reduction of id^k mod r), on the Python curve."""
    cv = env.curve
    acc = None
    for enc in reversed(call["sets"][c["set"]]):
        acc = cv.add(cv.mul_any(acc, c["id"]), env.dec(enc))
    return int(acc == env.dec(env.msm([call["g"], call["h"]], [c["s"], c["st"]])))


def defect(env, call, c):
    """s g + s' h - sum (id^k mod r) C_k of one share, encoded."""
    C = call["sets"][c["set"]]
    return env.msm([call["g"], call["h"]] + C,
                   [c["s"], c["st"]] + [(R - pow(c["id"], k, R)) % R for k in range(call["t"])])


def cancel_call(oc):
    """One call of t = 3: set 0 holds seven shares, rows 1 and 4 with s + 1 and s - 1; set 1 five, rows 0 and 4
    with s' + 1 and s' - 1; set 2 is clean.  cases[i]['pair'] names the pair a bad row belongs to."""
    _OC[id(oc)] = oc
    return _cancel_call(id(oc))


@functools.lru_cache(maxsize=None)
def _cancel_call(oc_key):
    env = E.Env(_OC[oc_key], 1)
    rng = random.Random(9200)
    t = 3
    g, h = env.muls([rng.randrange(1 << 250, R), rng.randrange(1 << 250, R)])
    sets, cases = [], []
    for si, (size, bad) in enumerate(((7, {1: (1, 0), 4: (R - 1, 0)}), (5, {0: (0, 1), 4: (0, R - 1)}), (4, {}))):
        coef = _coef(rng, t)
        sets.append(_commit(env, g, h, coef))
        for row in range(size):
            i = row + 1
            s, st = _share(coef, i)
            ds, dst = bad.get(row, (0, 0))
            cases.append(dict(name=f"set{si}/row{row}", set=si, id=i, s=(s + ds) % R, st=(st + dst) % R,
                              intent=int(row not in bad), pair=si if row in bad else None))
    return _call(t, g, h, sets, cases)


def sizes_call(oc):
    """One call of t = 3 with a set per entry of SIZES, ids 1 .. size, the rows of SIZES_BAD with s + 1."""
    _OC[id(oc)] = oc
    return _sizes_call(id(oc))


@functools.lru_cache(maxsize=None)
def _sizes_call(oc_key):
    env = E.Env(_OC[oc_key], 1)
    rng = random.Random(9300)
    t = 3
    g, h = env.muls([rng.randrange(1 << 250, R), rng.randrange(1 << 250, R)])
    sets, cases = [], []
    for si, size in enumerate(SIZES):
        coef = _coef(rng, t)
        sets.append(_commit(env, g, h, coef))
        for row in range(size):
            s, st = _share(coef, row + 1)
            bad = row in SIZES_BAD.get(size, ())
            cases.append(dict(name=f"size{size}/row{row}", set=si, id=row + 1, s=(s + 1) % R if bad else s, st=st,
                              intent=int(not bad)))
    return _call(t, g, h, sets, cases)
