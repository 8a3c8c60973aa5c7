"""The pair-lane Miller loops driven directly (csrc/miller_lz.hip: k_miller<SIG, false>, two pairs a
credential; k_miller<SIG, true>, twin; k_miller4<SIG>, quad), byte for byte against the C oracle's
pairing and against Miller words recorded from the kernels themselves.

cck_miller_lz_g2 / _g1 (twin = 0 and 1) and cck_miller4_lz_g2 / _g1 are called through ctypes on torch
device buffers with the null stream, with the constant operands cck_lazy_form and cck_gtilde_lines make;
the Miller words then go through cck_fexp_q (one element: cck_fexp with wide_max = 1), which
tests/test_gpu_fexp_direct.py tests on their own.  Inputs and expectations come from
tests/miller_lz_cases.py (asserted on the CPU by tests/test_miller_lz_model.py): flag words the project's
preps never write, set over real points and over garbage beside computed neighbours; odd tails over
buffers filled with zeros and with 0xFF; strides wider than the launch; twist points outside G2 for the
qcheck word.  Every output is filled with 0xC3 beforehand and followed by 64 sentinel elements, every
input is compared with its upload after the call, and each tiled launch runs once and is shared by the
tests that read it.  Every comparison is byte equality.

tests/golden/miller_lz_words.json holds the 144 raw output words of the first 8 elements of the plain
block per launcher (recipe: tests/golden/make_golden.py millerlz): a change of the loops that alters the
representation of any value shows up there word for word.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import fexp_direct_cases as C
import miller_lz_cases as M
import miller_wide_cases as W
import torsion_edges as T
from oracle import bls12_381 as B
from test_gpu_miller_wide_direct import FILL, SENT, _dev, _ptr, _upload, run_fexp

pytestmark = pytest.mark.gpu

LAUNCHERS = ("lz_g2", "lz_g1", "twin_g2", "twin_g1", "quad_g2", "quad_g1")
KIND = {"lz_g2": "g2", "lz_g1": "g1", "twin_g2": "twin", "twin_g1": "twin", "quad_g2": "quad", "quad_g1": "quad"}
FILL_WORD = int.from_bytes(bytes([FILL]) * 4, "little")
QC = 0xA0        # the qcheck word before a launch that must leave it alone
PREP_PAD = 256   # words behind the prep, part of the upload
FLAG_PAD = 8
SMALL_BIG = {"g2": (2, 129), "g1": (2, 129), "twin": (3, 257), "quad": (5, 513)}
RECORDED = 8     # elements per launcher in the fixture


@pytest.fixture(scope="module")
def K():
    return launchers()


def launchers():
    """The launchers (csrc/launch.h) with their prototypes."""
    from coconut._lib import lib
    sz, p, i = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int
    for f in (lib.cck_miller_lz_g2, lib.cck_miller_lz_g1):
        f.argtypes, f.restype = [i, sz, sz, p, p, p, p, sz, sz, p, p], i
    for f in (lib.cck_miller4_lz_g2, lib.cck_miller4_lz_g1):
        f.argtypes, f.restype = [sz, sz, p, p, p, sz, sz, p, p], i
    lib.cck_gtilde_lines.argtypes, lib.cck_gtilde_lines.restype = [p, p, p], i
    lib.cck_lazy_form.argtypes, lib.cck_lazy_form.restype = [sz, p, p, p], i
    lib.cck_fexp_q.argtypes, lib.cck_fexp_q.restype = [sz, p, p, p, p, p], i
    lib.cck_fexp.argtypes, lib.cck_fexp.restype = [sz, p, p, p, p, p, sz, p], i
    return lib


def _filled(nwords):
    import torch
    return torch.full((4 * nwords,), FILL, dtype=torch.uint8, device=_dev())


def _words_of(t):
    return t.cpu().numpy().view(np.uint32)


def lazy_form(K, words):
    """cck_lazy_form on 12-word storage-form values; returns the output words (sentinels checked)."""
    import torch
    n = len(words) // 12
    d_in, d_out = _upload(words), _filled(12 * n + SENT)
    torch.cuda.synchronize()
    assert K.cck_lazy_form(n, _ptr(d_in), _ptr(d_out), None) == 0
    torch.cuda.synchronize()
    out = _words_of(d_out)
    assert (out[12 * n:] == FILL_WORD).all(), "sentinels"
    assert np.array_equal(_words_of(d_in), words)
    return out[:12 * n].copy()


def gtilde_lines(K, q):
    """cck_gtilde_lines of an affine twist point: the 68 x 72 words (sentinels checked)."""
    import torch
    nw = M.NLINES * M.LINE_WORDS
    d_in, d_out = _upload(M.q_words(q)), _filled(nw + SENT)
    torch.cuda.synchronize()
    assert K.cck_gtilde_lines(_ptr(d_in), _ptr(d_out), None) == 0
    torch.cuda.synchronize()
    out = _words_of(d_out)
    assert (out[nw:] == FILL_WORD).all(), "sentinels"
    return out[:nw].copy()


@functools.lru_cache(maxsize=None)
def const_operand(K, sig, k=0):
    """The device buffer of the two-pair loops' constant: g~ in G1 in R' form, or g~'s lines."""
    if sig == "g2":
        return _upload(lazy_form(K, M.p_store_words(M.gtilde1())))
    return _upload(gtilde_lines(K, M.gtilde2(k)))


def run(K, lid, creds, pstride=None, fstride=None, foff=0, fill=0, qc=QC, const=None, pstride_arg=None):
    """One launch of launcher lid over the credentials; returns (rc, output words, qcheck word after).
    The output is the (144, fstride) array of the whole buffer (flat when fstride < foff + m).  Checks the
    sentinels behind the output and the qcheck word and that the inputs are untouched."""
    import torch
    kind, n = KIND[lid], len(creds)
    m_in, m_out = M.elements_in(kind, n), M.outputs(kind, n)
    pstride = m_in if pstride is None else pstride
    fstride = m_out if fstride is None else fstride
    prep = np.concatenate([M.encode_prep(kind, creds, pstride, fill), np.full(PREP_PAD, fill, np.uint32)])
    fl = np.concatenate([M.flags_of(creds), np.full(FLAG_PAD, fill, np.uint32)])
    d_prep, d_fl = _upload(prep), _upload(fl)
    nout = C.F12_WORDS * max(fstride, foff + m_out)
    d_f = _filled(nout + SENT * C.F12_WORDS)
    qc0 = np.array([0 if qc is None else qc] + [FILL_WORD] * SENT, dtype=np.uint32)
    d_qc = _upload(qc0)
    p_qc = _ptr(d_qc) if qc is not None else None
    ps = pstride if pstride_arg is None else pstride_arg
    torch.cuda.synchronize()
    if kind == "quad":
        f = K.cck_miller4_lz_g2 if lid == "quad_g2" else K.cck_miller4_lz_g1
        rc = f(n, ps, _ptr(d_prep), _ptr(d_fl), _ptr(d_f), fstride, foff, p_qc, None)
    else:
        f = K.cck_miller_lz_g2 if lid.endswith("g2") else K.cck_miller_lz_g1
        if kind == "twin":
            p_c = None  # unused by the twin loop
        else:
            p_c = _ptr(const if const is not None else const_operand(K, kind))
        rc = f(int(kind == "twin"), n, ps, _ptr(d_prep), _ptr(d_fl), p_c, _ptr(d_f), fstride, foff, p_qc, None)
    torch.cuda.synchronize()
    out = _words_of(d_f)
    assert (out[nout:] == FILL_WORD).all(), "sentinels"
    assert np.array_equal(_words_of(d_prep), prep) and np.array_equal(_words_of(d_fl), fl)
    qc1 = _words_of(d_qc)
    assert np.array_equal(qc1[1:], qc0[1:]), "qcheck sentinels"
    out = out[:nout].copy()
    return rc, (out.reshape(C.F12_WORDS, fstride) if fstride >= foff + m_out else out), int(qc1[0])


def run_fexp_q(K, words):
    """cck_fexp_q on a (144, n) word array of Miller values; returns the GT bytes per element."""
    import torch
    n = words.shape[1]
    flat = np.ascontiguousarray(words).reshape(-1)
    d_f = _upload(flat)
    d_v = torch.full((n + SENT,), FILL, dtype=torch.uint8, device=_dev())
    d_gt = torch.full(((n + SENT) * C.GT_BYTES,), FILL, dtype=torch.uint8, device=_dev())
    torch.cuda.synchronize()
    assert K.cck_fexp_q(n, _ptr(d_f), None, _ptr(d_v), _ptr(d_gt), None) == 0
    torch.cuda.synchronize()
    v, g = d_v.cpu().numpy(), d_gt.cpu().numpy()
    assert bytes(v[n:]) == bytes([FILL]) * SENT, "verdict sentinels"
    assert bytes(g[n * C.GT_BYTES:]) == bytes([FILL]) * (SENT * C.GT_BYTES), "GT sentinels"
    assert np.array_equal(_words_of(d_f), flat)
    gts = [bytes(g[C.GT_BYTES * i:C.GT_BYTES * (i + 1)]) for i in range(n)]
    assert [int(x) for x in v[:n]] == [int(gt == C.ONE_GT) for gt in gts]
    return gts


def fexp(K, words):
    """GT bytes per element: the quad-lane kernel from two elements on, the one-wave kernel for one."""
    return run_fexp_q(K, words) if words.shape[1] >= 2 else run_fexp(K, np.ascontiguousarray(words))


@functools.lru_cache(maxsize=None)
def _tiled(K, lid, n):
    """The tiled launch of n (miller_lz_cases.layout), once: (credentials, Miller words, GT bytes, qcheck)."""
    creds = M.layout(KIND[lid], n)
    rc, words, qc = run(K, lid, creds)
    assert rc == 0
    words.setflags(write=False)
    return creds, words, fexp(K, words), qc


def check_against_oracle(K, oc, lid, n):
    """Test 1 on the tiled launch of n; returns its Miller words."""
    kind = KIND[lid]
    creds, words, gts, qc = _tiled(K, lid, n)
    want, pairs = M.expected(oc, kind, creds), M.computed_pairs(kind, creds, "g")
    assert len(gts) == len(want) == M.outputs(kind, n)
    for e in range(len(want)):
        assert gts[e] == want[e], (lid, n, e)
        assert np.array_equal(words[:, e], M.ONE_WORDS) == (not pairs[e]), (lid, n, e)
    C.decode(words.reshape(-1), len(want))  # every stored value canonical
    assert qc == QC  # every computed Q lies in G2, garbage only under skip flags: the word is left alone
    return words


@pytest.mark.parametrize("lid,n", [(lid, n) for lid in LAUNCHERS for n in M.SIZES[KIND[lid]]])
def test_gt_against_the_oracle(K, oc, lid, n):
    """Every element's GT is the oracle's product over its computed pairs; an element whose pairs are all
    skipped holds exactly the stored form of 1 (and no other does)."""
    kind = KIND[lid]
    check_against_oracle(K, oc, lid, n)
    if n == M.SIZES[kind][-1]:  # the launch held every flag word at every pair position over a real point
        creds = _tiled(K, lid, n)[0]
        real = {(fl, pos) for fl, pos, is_real in M.coverage(kind, creds, 0, n) if is_real}
        assert real == {(fl, pos) for fl, pos, _ in M.full_coverage(kind)}
        junk = {(fl, pos) for fl, pos, is_real in M.coverage(kind, creds, 0, n) if not is_real}
        assert junk == {(fl, pos) for fl, pos, is_real in M.full_coverage(kind) if not is_real}
        assert any(not p for p in M.computed_pairs(kind, creds, "g"))  # an element with every pair skipped


@pytest.mark.parametrize("lid,n", [(lid, n) for lid in LAUNCHERS[2:] for n in M.SIZES[KIND[lid]]
                                   if n % M.NP[KIND[lid]]])
def test_tail_reads_nothing_it_uses(K, oc, lid, n):
    """Twin with odd n, quad with n mod 4 != 0: whatever lies behind the last credential (the prep's
    absent pair slots and unused words, the flags past n), zeros or 0xFF, the output words are the same
    and the oracle's."""
    kind = KIND[lid]
    creds, words, gts, _ = _tiled(K, lid, n)  # fill = 0
    rc, ff, qc = run(K, lid, creds, fill=0xFFFFFFFF)
    assert rc == 0 and qc == QC
    assert np.array_equal(ff, words), (lid, n)
    assert gts == M.expected(oc, kind, creds)
    if n % 2:
        assert M.absent(kind, n) == [((n - 1) // 2, 1)]


@pytest.mark.parametrize("lid", LAUNCHERS)
def test_placement(K, lid):
    """pstride = m + 5, fstride = m + 7, foff = 3: the words are the dense launch's, at elements
    foff .. foff + m, and nothing else is written."""
    kind = KIND[lid]
    for n in SMALL_BIG[kind]:
        creds, words, _, _ = _tiled(K, lid, n)
        m_in, m = M.elements_in(kind, n), M.outputs(kind, n)
        fstride, foff = m + 7, 3
        rc, out, qc = run(K, lid, creds, pstride=m_in + 5, fstride=fstride, foff=foff, fill=0xFFFFFFFF)
        assert rc == 0 and qc == QC
        assert np.array_equal(out[:, foff:foff + m], words), (lid, n)
        rest = np.delete(out, np.s_[foff:foff + m], axis=1)
        assert (rest == FILL_WORD).all(), (lid, n)


@pytest.mark.parametrize("lid", LAUNCHERS)
def test_rejected_and_empty_launches(K, lid):
    """fstride < foff + m and pstride < m (twin and quad: m of the twin layout, ceil(n / 2)) return -1 and
    write nothing; n = 0 returns 0 and writes nothing."""
    import torch
    kind, n = KIND[lid], 5
    creds = M.layout(kind, n)
    m_in, m = M.elements_in(kind, n), M.outputs(kind, n)
    assert m_in == (n if M.NP[kind] == 1 else 3)
    for kw in (dict(fstride=m - 1), dict(fstride=m + 2, foff=3), dict(pstride_arg=m_in - 1), dict(pstride_arg=0)):
        rc, out, qc = run(K, lid, creds, **kw)
        assert rc == -1 and qc == QC, kw
        assert (out == FILL_WORD).all(), kw
    rc0, dense, _ = run(K, lid, creds)
    rc, out, _ = run(K, lid, creds, fstride=m + 3, foff=3)  # the least stride that holds the launch
    assert rc0 == 0 and rc == 0 and np.array_equal(out[:, 3:], dense) and (out[:, :3] == FILL_WORD).all()
    d = _filled(C.F12_WORDS)
    if kind == "quad":
        f = K.cck_miller4_lz_g2 if lid == "quad_g2" else K.cck_miller4_lz_g1
        rc = f(0, 0, _ptr(d), _ptr(d), _ptr(d), 0, 0, _ptr(d), None)
    else:
        f = K.cck_miller_lz_g2 if lid.endswith("g2") else K.cck_miller_lz_g1
        rc = f(int(kind == "twin"), 0, 0, _ptr(d), _ptr(d), _ptr(d), _ptr(d), 0, 0, _ptr(d), None)
    torch.cuda.synchronize()
    assert rc == 0 and (_words_of(d) == FILL_WORD).all()


@pytest.mark.parametrize("lid", LAUNCHERS[2:])
def test_exchanged_credentials_change_their_elements_only(K, oc, lid):
    """Two computed credentials of different elements exchanged (at the block-crossing size one on each
    side of the block edge): exactly those two elements' GT change, to the oracle's."""
    kind = KIND[lid]
    npos = M.NP[kind]
    for n in (3 * npos, M.BLOCK_PAIRS * npos + 4):
        creds = M.layout(kind, n)
        swapped, (ea, eb) = M.exchange(kind, creds)
        rc0, w0, _ = run(K, lid, creds)
        rc1, w1, _ = run(K, lid, swapped)
        assert rc0 == 0 and rc1 == 0
        g0, g1 = fexp(K, w0), fexp(K, w1)
        assert g0 == M.expected(oc, kind, creds) and g1 == M.expected(oc, kind, swapped)
        assert [e for e in range(len(g0)) if g0[e] != g1[e]] == [ea, eb], (lid, n)


@pytest.mark.parametrize("lid", LAUNCHERS[2:])
def test_inverse_couples_multiply_to_one(K, oc, lid):
    """(P, Q), (-P, Q) in one element (quad: two couples) give exactly one, while the Miller values left
    when the second of each couple is skipped do not."""
    kind = KIND[lid]
    npos = M.NP[kind]
    for n in (3 * npos, (M.BLOCK_PAIRS + 1) * npos):
        rc, words, _ = run(K, lid, M.inverse_launch(kind, n))
        assert rc == 0
        for e in (0, n // npos - 1):
            assert not np.array_equal(words[:, e], M.ONE_WORDS)
        assert fexp(K, words) == [C.ONE_GT] * (n // npos)
    single = M.inverse_launch(kind, 3 * npos, single=True)
    rc, words, _ = run(K, lid, single)
    got = fexp(K, words)
    assert rc == 0 and got == M.expected(oc, kind, single) and C.ONE_GT not in got


@pytest.mark.parametrize("lid", LAUNCHERS)
def test_bilinearity(K, oc, lid):
    """e(a P, Q) = e(P, a Q) = e(P, Q)^a through each launcher, every other pair of the element skipped."""
    kind = KIND[lid]
    creds, rel = M.bilinear_launch(kind)
    rc, words, _ = run(K, lid, creds)
    gts = fexp(K, words)
    assert rc == 0 and gts == M.expected(oc, kind, creds)
    for a, b, base in rel:
        assert gts[a] != gts[base]
        assert b is None or gts[a] == gts[b]
        assert B.gt_to_bytes(B.f12_pow(list(B.gt_from_bytes(gts[base])), W.A)) == gts[a]


# ---------------------------------------------------------------- qcheck
MODELLED = ("T13", "T23", "kG+T13")  # the twist points tests/torsion_edges.py models


@pytest.mark.parametrize("kind", ["twin", "quad"])
def test_qcheck_is_set_by_a_computed_q_outside_g2(K, oc, kind):
    """One Q outside G2 at every pair position in turn (the last credential of the odd launch included)
    sets bit 0 of the word, pre-set to 0 and to 0xA0 in turn, and leaves the other bits; the GT is the
    oracle's, and for the modelled points the projective Python model's."""
    lid, k = kind + "_g2", 0
    seen = set()
    for t, (name, (q, _)) in enumerate(M.twist_points().items()):
        for w, where in enumerate(M.TWIST_WHERE[kind]):
            preset = (0, QC)[k % 2]
            k += 1
            creds = M.twist_launch(kind, where, q)
            rc, words, qc = run(K, lid, creds, qc=preset)
            assert rc == 0 and qc == preset | 1, (name, where, preset)
            gts = fexp(K, words)
            assert gts == M.expected(oc, kind, creds), (name, where)
            e = where // M.NP[kind]
            if name == "T13":  # T ends as (0, 0, 0): a zero Miller value
                assert gts[e] == C.ZERO_GT and not words[:, e].any()
            if name in MODELLED and w == t:
                assert gts[e] == T.gt_bytes(M.computed_pairs(kind, creds)[e]), (name, where)
            seen.add((where, preset))
    assert seen == {(w, p) for w in M.TWIST_WHERE[kind] for p in (0, QC)}


@pytest.mark.parametrize("kind", ["twin", "quad"])
def test_qcheck_is_left_alone_otherwise(K, oc, kind):
    """All Q in G2; the same points outside G2 under a skip flag; a null d_qcheck; the SigG1 builds and the
    two-pair loop, which do not test: the word is unchanged and the GT the oracle's."""
    tw = [q for q, _ in M.twist_points().values()]
    honest = M.twist_launch(kind, -1, None)
    skipped = list(honest)
    for k, where in enumerate(M.TWIST_WHERE[kind]):
        skipped[where] = (M.Slot(M.REAL, honest[where][0].p, tw[k % len(tw)]), (1, 4, 5)[k % 3])
    for preset in (0, QC):
        for creds in (honest, skipped):
            rc, words, qc = run(K, kind + "_g2", creds, qc=preset)
            assert rc == 0 and qc == preset
            assert fexp(K, words) == M.expected(oc, kind, creds)
    bad = M.twist_launch(kind, M.TWIST_WHERE[kind][-1], tw[1])
    rc, words, _ = run(K, kind + "_g2", bad, qc=None)
    assert rc == 0 and fexp(K, words) == M.expected(oc, kind, bad)
    rc, words, qc = run(K, kind + "_g1", bad, qc=QC)
    assert rc == 0 and qc == QC and fexp(K, words) == M.expected(oc, kind, bad)
    if kind == "twin":  # the two-pair SigG2 loop with sigma_1 outside G2
        two = M.layout("g2", 3)
        two[1] = (M.Slot(M.REAL, two[1][0].p, tw[1]),) + two[1][1:]
        rc, words, qc = run(K, "lz_g2", two, qc=QC)
        assert rc == 0 and qc == QC and fexp(K, words) == M.expected(oc, "g2", two)


# ---------------------------------------------------------------- the constant operands
def test_lazy_form(K):
    """cck_lazy_form: v 2^406 -> v 2^392 mod p, canonical, for the P coordinates used here and 0, 1, p - 1."""
    vals = [v for p, _ in W.pairs() for v in p] + list(M.gtilde1()) + [0, 1, B.P - 1]
    words = np.array(sum((M._words(v, C.R_STORE) for v in vals), []), dtype=np.uint32)
    want = np.array(sum((M._words(v, M.R_LAZY) for v in vals), []), dtype=np.uint32)
    assert np.array_equal(lazy_form(K, words), want)
    assert np.array_equal(_words_of(const_operand(K, "g2")), M.p_words(M.gtilde1()))


def test_gtilde_lines(K, oc):
    """cck_gtilde_lines writes 68 x 72 words (every one of the 68 x 6 Fp values canonical: the 0xC3 fill is
    not) and nothing past them; two different g~ through the SigG1 two-pair loop give the two oracle values."""
    lines = [gtilde_lines(K, M.gtilde2(k)) for k in (0, 1)]
    for ln in lines:
        for v in ln.reshape(-1, 12):
            assert sum(int(x) << (32 * j) for j, x in enumerate(v)) < B.P
    assert not np.array_equal(lines[0], lines[1])
    creds = M.layout("g1", 3)
    gts = []
    for k in (0, 1):
        rc, words, _ = run(K, "lz_g1", creds, const=const_operand(K, "g1", k))
        assert rc == 0
        gts.append(fexp(K, words))
        assert gts[k] == M.expected(oc, "g1", creds, M.gtilde2(k))
    assert all(a != b for a, b in zip(*gts))


# ---------------------------------------------------------------- recorded words
@functools.lru_cache(maxsize=None)
def golden():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "miller_lz_words.json")
    with open(path) as f:
        d = json.load(f)
    assert sorted(d["words"]) == ["lz_g1", "lz_g2", "quad", "twin"]
    assert all(len(v) == RECORDED for v in d["words"].values())
    return {k: [np.frombuffer(bytes.fromhex(h), dtype="<u4") for h in v] for k, v in d["words"].items()}


def recorded_key(lid):
    return lid if lid.startswith("lz") else lid[:4]


@pytest.mark.parametrize("lid", LAUNCHERS)
def test_recorded_words(K, lid):
    """The complete elements among the first 8 (the plain block) reproduce the recorded words exactly, at
    the small and at the block-crossing size; the SigG2 and SigG1 builds of twin and quad share one record."""
    kind = KIND[lid]
    want = golden()[recorded_key(lid)]
    for n in SMALL_BIG[kind]:
        creds, words, _, _ = _tiled(K, lid, n)
        full = min(RECORDED, n // M.NP[kind])
        assert full >= 1 and all(cr[-1] == 0 for cr in creds[:full * M.NP[kind]])
        for e in range(full):
            assert np.array_equal(words[:, e], want[e]), (lid, n, e)
