"""The final-exponentiation kernels and the wide Fp12 product tree driven directly, byte for byte
against the oracle (tests/fexp_direct_cases.py; the regime of every input is asserted on the CPU by
tests/test_fexp_direct_model.py).

cck_fexp_q (csrc/fexp_q.hip k_fexp_q: one element per lane quad), cck_fexp with wide_max = n
(csrc/fexp_pl.hip k_fexp1: one element per wave) and cck_f12_reduce_wide (k_f12_reduce_wide) are
called through ctypes on torch device buffers with the null stream.  Elsewhere these kernels only see
Miller-loop outputs: dense values, the value 1 of an identity sum and the all-zero value of the order-13
twist point.  Here they get sparse values (zero Fp2 coefficients through the inversion, the Frobenius
maps, the products and the storage/lazy conversions), values other than 1 that the easy part sends to
exactly 1 (the Granger-Scott fallback of every pow-by-x, beside quads of the same wave that take the
normal path), r-th powers (a GT of exactly one through the normal path), and each flag bit of the
verdict rule.

The fallback ladder itself only ever sees the base 0 or 1: a non-zero input whose three snapshot
denominators all vanish has an easy part of exactly 1 (the model test asserts it for every case), so a
ladder that drops a multiplication by its base cannot be told from a right one through these entry
points; one that multiplies by a wrong operand is caught here and by the identity-sum cases of the
verify suites.
"""
import ctypes
import random

import numpy as np
import pytest

import fexp_direct_cases as C
from oracle import bls12_381 as B

pytestmark = pytest.mark.gpu

SENT = 64       # sentinel elements after every output buffer
FILL = 0xC3     # their contents (and the outputs' before the call)
FLAG_WORDS = (0, 1, 2, 4, 8, 16, 32, 11)


@pytest.fixture(scope="module")
def K():
    """The three launchers (csrc/launch.h) with their prototypes."""
    from coconut._lib import lib
    sz, p, i = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int
    lib.cck_fexp_q.argtypes, lib.cck_fexp_q.restype = [sz, p, p, p, p, p], i
    lib.cck_fexp.argtypes, lib.cck_fexp.restype = [sz, p, p, p, p, p, sz, p], i
    lib.cck_f12_reduce_wide.argtypes, lib.cck_f12_reduce_wide.restype = [sz, p, p, p], i
    return lib


def _dev():
    import torch
    return torch.device("cuda", 0)


def _upload(arr, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(dtype).copy()).to(_dev())


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def run_fexp(K, form, fs, flags=None, want_gt=True, scratch_fill=0x00):
    """One call of form 'quad' (cck_fexp_q) or 'wave' (cck_fexp, wide_max = n) on a fresh upload of fs;
    returns (verdicts, GT bytes or None) after checking the sentinels behind both outputs."""
    import torch
    n = len(fs)
    words = C.encode(fs)
    d_f = _upload(words, np.int32)
    d_fl = _upload(np.array(flags, dtype=np.uint32), np.int32) if flags is not None else None
    d_v = torch.full((n + SENT,), FILL, dtype=torch.uint8, device=_dev())
    d_gt = torch.full(((n + SENT) * C.GT_BYTES,), FILL, dtype=torch.uint8, device=_dev()) if want_gt else None
    torch.cuda.synchronize()
    if form == "quad":
        rc = K.cck_fexp_q(n, _ptr(d_f), _ptr(d_fl), _ptr(d_v), _ptr(d_gt), None)
    else:
        d_s = torch.full((72 * 12 * n * 4,), scratch_fill, dtype=torch.uint8, device=_dev())  # slots.h: 72 x 12 x n words
        rc = K.cck_fexp(n, _ptr(d_f), _ptr(d_s), _ptr(d_fl), _ptr(d_v), _ptr(d_gt), n, None)
    torch.cuda.synchronize()
    assert rc == 0
    v = d_v.cpu().numpy()
    assert bytes(v[n:]) == bytes([FILL]) * SENT, "verdict sentinels"
    gt = None
    if want_gt:
        g = d_gt.cpu().numpy()
        assert bytes(g[n * C.GT_BYTES:]) == bytes([FILL]) * (SENT * C.GT_BYTES), "GT sentinels"
        gt = bytes(g[:n * C.GT_BYTES])
    if form == "quad":  # its input is const
        assert np.array_equal(d_f.cpu().numpy().view(np.uint32), words)
    return [int(x) for x in v[:n]], gt


def want(fs, flags=None):
    exp = [C.expected(C.f12(f)) for f in fs]
    fl = flags if flags is not None else [0] * len(fs)
    return [int(one and (w & 11) == 0) for (_, one), w in zip(exp, fl)], b"".join(gt for gt, _ in exp)


def check(K, form, fs, names, flags=None, **kw):
    v, gt = run_fexp(K, form, fs, flags, **kw)
    wv, wgt = want(fs, flags)
    for i in range(len(fs)):
        assert gt[576 * i:576 * (i + 1)] == wgt[576 * i:576 * (i + 1)], (form, len(fs), i, names[i])
        assert v[i] == wv[i], (form, len(fs), i, names[i])
    return v, gt


def pools():
    """Values of each kind for the placement tests: the fallback pool is sparse, non-trivial values (and
    one itself), the generic pool sparse and dense ones."""
    pick = lambda names: [C.by_name(x) for x in names]  # noqa: E731
    p = {
        C.FALLBACK: pick(["sup024", "sup14", "sup3", "sub_fp4", "sub_fp6", "unit-W5i", "one", "sup135_pm1", "sub_fp",
                          "unit+W2", "sup25_ones"]),
        C.ZERO_KIND: pick(["zero"]),
        C.RTH: pick(["rth0", "rth1"]),
        C.GENERIC: pick(["generic0", "sup01", "sup012345_pm1", "sup0123", "generic1", "sup34", "scale_pm1",
                         "sup01_ones", "sup12345"]),
    }
    for kind, cs in p.items():
        assert all(c.kind == kind for c in cs)
    return p


def interleaved(n, rot):
    """Element i is of kind KINDS[(i + rot) % 4]: the four kinds alternate quad by quad (and wave by wave in
    the one-wave form); over rot = 0..3 every position takes every kind."""
    p = pools()
    cs = []
    for i in range(n):
        pool = p[C.KINDS[(i + rot) % 4]]
        cs.append(pool[(i // 4 + rot) % len(pool)])
    return [c.f for c in cs], [c.name for c in cs]


def test_every_case_in_both_forms(K):
    cs = C.cases()
    fs, names = [c.f for c in cs], [c.name for c in cs]
    vq, gq = check(K, "quad", fs, names)
    vw, gw = check(K, "wave", fs, names)
    assert (vq, gq) == (vw, gw)
    by = dict(zip(names, range(len(cs))))
    for c in cs:  # what the model test derives, restated on the device's own outputs
        i = by[c.name]
        g = gq[576 * i:576 * (i + 1)]
        assert (g == C.ONE_GT, vq[i]) == ((True, 1) if c.kind in (C.FALLBACK, C.RTH) else (False, 0)), c.name
        if c.same_as:
            j = by[c.same_as]
            assert g == gq[576 * j:576 * (j + 1)], c.name
    assert gq[576 * by["zero"]:576 * (by["zero"] + 1)] == C.ZERO_GT


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 130])
def test_quad_kernel_placement(K, n):
    """One quad per element, 16 quads a wave, 64 a block: every kind at quads 0, 1, 15, 16, 63, 64 and
    n - 1, the kinds alternating quad by quad, last waves and blocks partly empty."""
    seen = {}
    for rot in range(4):
        fs, names = interleaved(n, rot)
        check(K, "quad", fs, names)
        for i in (0, 1, 15, 16, 63, 64, n - 1):
            if i < n:
                seen.setdefault(i, set()).add(C.KINDS[(i + rot) % 4])
    assert all(s == set(C.KINDS) for s in seen.values())


def test_quad_kernel_uniform_batches(K):
    fb = pools()[C.FALLBACK]
    for n in (65, 130):
        cs = [fb[i % len(fb)] for i in range(n)]
        v, gt = check(K, "quad", [c.f for c in cs], [c.name for c in cs])
        assert v == [1] * n and gt == C.ONE_GT * n
        v, gt = check(K, "quad", [C.ZERO] * n, ["zero"] * n)
        assert v == [0] * n and gt == C.ZERO_GT * n


@pytest.mark.parametrize("n", [1, 2, 65])
def test_wave_kernel_placement(K, n):
    for rot in range(4):
        fs, names = interleaved(n, rot)
        check(K, "wave", fs, names)


def _flag_batch():
    fs, names, flags = [], [], []
    for name in ("sup024", "one", "rth0", "rth1", "generic0", "sup01", "zero"):
        for w in FLAG_WORDS + (0xFFFFFFF4,):
            fs.append(C.by_name(name).f)
            names.append(f"{name}/flags={w:#x}")
            flags.append(w)
    return fs, names, flags


@pytest.mark.parametrize("form", ["quad", "wave"])
def test_verdict_rule_per_flag_bit(K, form):
    """verdict = (GT == 1) and (flags & 11) == 0: bits 0, 1 and 3 reject, bits 2, 4, 5 and the rest do not;
    the GT bytes do not depend on the flags; a GT other than one is rejected whatever the flags."""
    fs, names, flags = _flag_batch()
    v, gt = check(K, form, fs, names, flags)
    v0, gt0 = check(K, form, fs, names, [0] * len(fs))
    assert gt == gt0
    m = len(FLAG_WORDS) + 1
    for b, name in enumerate(("sup024", "one", "rth0", "rth1")):
        assert C.by_name(name).kind in (C.FALLBACK, C.RTH)
        assert v[b * m:(b + 1) * m] == [1, 0, 0, 1, 0, 1, 1, 0, 1], name
        assert v0[b * m:(b + 1) * m] == [1] * m
    assert v[4 * m:] == [0] * (3 * m) and v0[4 * m:] == [0] * (3 * m)


@pytest.mark.parametrize("form", ["quad", "wave"])
def test_null_flags_and_null_gt(K, form):
    """A null flags pointer is zero flags (both kernels test the pointer: fexp_q.hip qexp_out, fexp_pl.hip
    fexp_out); without a GT buffer the verdicts are the same."""
    fs, names = interleaved(37, 1)
    v, gt = check(K, form, fs, names, flags=None)
    assert check(K, form, fs, names, flags=[0] * len(fs)) == (v, gt)
    v2, none = run_fexp(K, form, fs, flags=None, want_gt=False)
    assert none is None and v2 == v
    fs, names, flags = _flag_batch()
    v3, _ = run_fexp(K, form, fs, flags, want_gt=False)
    assert v3 == want(fs, flags)[0]


def test_scratch_contents_do_not_matter(K):
    fs, names = interleaved(21, 2)
    a = check(K, "wave", fs, names, scratch_fill=0x00)
    b = check(K, "wave", fs, names, scratch_fill=0xA5)
    assert a == b


# ---------------------------------------------------------------- the wide product tree
def _tree_pool():
    minus_one = ((C.P - 1, 0),) + (C.F2Z,) * 5
    names = ["sup024", "sup14", "sup3", "sup01", "sup0123", "sup25", "sup12345", "sup012345_pm1", "sup135_pm1",
             "sup01_ones", "unit-W5i", "unit+W3", "generic0", "generic1", "generic2", "rth0"]
    return [("zero", C.ZERO), ("one", C.ONE), ("-1", minus_one)] + [(x, C.by_name(x).f) for x in names]


def run_tree(K, fs):
    import torch
    n, n_out = len(fs), (len(fs) + 1) // 2
    words = C.encode(fs)
    d_in = _upload(words, np.int32)
    d_out = torch.full(((n_out * C.F12_WORDS + SENT) * 4,), FILL, dtype=torch.uint8, device=_dev())
    torch.cuda.synchronize()
    rc = K.cck_f12_reduce_wide(n, _ptr(d_in), _ptr(d_out), None)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint32)
    assert np.array_equal(d_in.cpu().numpy().view(np.uint32), words)
    assert bytes(out[n_out * C.F12_WORDS:].view(np.uint8)) == bytes([FILL]) * (4 * SENT), "output sentinels"
    return rc, out[:n_out * C.F12_WORDS], words


@pytest.mark.parametrize("n", [2, 3, 4, 5, 9])
def test_product_tree_level(K, n):
    """out[t] = in[2t] in[2t+1] in the storage form (input stride n, output stride (n + 1) / 2), the odd
    tail copied word for word.  a R times b R must come back as a b R: this is what fixes the encoder's
    storage constant R = 2^406, which the final exponentiation (invariant under Fp scaling) cannot."""
    pool = _tree_pool()
    rnd = random.Random(100 + n)
    batches = [[pool[(3 * k + n) % len(pool)] for k in range(n)]]                   # 0, 1, -1 and sparse operands in turn
    batches += [[pool[k % 3] if k % 2 == 0 else rnd.choice(pool[3:]) for k in range(n)]]  # 0 | 1 | -1 times a value
    batches += [[rnd.choice(pool) for _ in range(n)] for _ in range(4)]
    for batch in batches:
        fs = [f for _, f in batch]
        rc, out, words = run_tree(K, fs)
        assert rc == 0
        n_out = (n + 1) // 2
        got = C.decode(out, n_out)  # asserts canonical words
        for t in range(n // 2):
            assert got[t] == C.f12(B.f12_mul(list(fs[2 * t]), list(fs[2 * t + 1]))), (n, t, batch[2 * t][0], batch[2 * t + 1][0])
        if n % 2:
            assert np.array_equal(out.reshape(C.F12_WORDS, n_out)[:, n_out - 1],
                                  words.reshape(C.F12_WORDS, n)[:, n - 1]), (n, batch[-1][0])


def test_product_tree_rejects_one_input(K):
    rc, out, _ = run_tree(K, [C.by_name("generic0").f])
    assert rc == -1
    assert bytes(out.view(np.uint8)) == bytes([FILL]) * (4 * C.F12_WORDS)  # nothing written
