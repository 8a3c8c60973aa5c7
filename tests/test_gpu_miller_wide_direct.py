"""The wide Miller loop driven directly (csrc/miller_wide.hip: k_miller_wide2, two waves a pair, for
launches of up to kWide2Max = 256 pairs; k_miller_wide, one wave a pair, above), against the oracle's
pairing and against Miller words recorded from the kernels themselves.

cck_miller_wide is called through ctypes on torch device buffers with the null stream, then cck_fexp
with wide_max = n (k_fexp1) and, where a product is needed, cck_f12_reduce_wide.  Inputs come from
tests/miller_wide_cases.py: 16 seeded pairs tiled to the launch size, P scaled by 1 or by a random k in
Fp*, skipped and computed pairs interleaved.  Every output is filled with 0xC3 beforehand and followed
by 64 sentinel elements.  Each launch size is run once and shared by the tests that read it.

tests/golden/miller_wide_words.json holds the 144 raw output words of each of the 16 pairs as the
kernels wrote them (recipe: tests/golden/make_golden.py millerwide): the two kernels run the same field
operations on every value, so one set serves both, and a change of either loop that alters any
intermediate value's representation shows up here word for word.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import fexp_direct_cases as C
import miller_wide_cases as M
from oracle import bls12_381 as B

pytestmark = pytest.mark.gpu

SENT = 64       # sentinel elements after every output buffer
FILL = 0xC3     # their contents (and the outputs' before the call)
SIZES = (1, 2, 16, 255, 256, 257)  # <= 256: k_miller_wide2; 257: k_miller_wide


@pytest.fixture(scope="module")
def K():
    return launchers()


def launchers():
    """The three launchers (csrc/launch.h) with their prototypes."""
    from coconut._lib import lib
    sz, p, i = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int
    lib.cck_miller_wide.argtypes, lib.cck_miller_wide.restype = [sz, p, p, p, sz, sz, p], i
    lib.cck_fexp.argtypes, lib.cck_fexp.restype = [sz, p, p, p, p, p, sz, p], i
    lib.cck_f12_reduce_wide.argtypes, lib.cck_f12_reduce_wide.restype = [sz, p, p, p], i
    return lib


def _dev():
    import torch
    return torch.device("cuda", 0)


def _upload(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32).copy()).to(_dev())


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def run_miller(K, items, flags, fstride=None, foff=0):
    """One cck_miller_wide launch of items [(P, Q, k)]; returns (rc, the whole output buffer as a
    (144, fstride) word array) after checking the sentinels and that the inputs are untouched."""
    import torch
    n = len(items)
    fstride = n if fstride is None else fstride
    prep, fl = M.encode_prep(items), np.array(flags, dtype=np.uint32)
    d_prep, d_fl = _upload(prep), _upload(fl)
    d_f = torch.full(((C.F12_WORDS * fstride + SENT * C.F12_WORDS) * 4,), FILL, dtype=torch.uint8, device=_dev())
    torch.cuda.synchronize()
    rc = K.cck_miller_wide(n, _ptr(d_prep), _ptr(d_fl), _ptr(d_f), fstride, foff, None)
    torch.cuda.synchronize()
    out = d_f.cpu().numpy().view(np.uint32)
    assert bytes(out[C.F12_WORDS * fstride:].view(np.uint8)) == bytes([FILL]) * (4 * SENT * C.F12_WORDS), "sentinels"
    assert np.array_equal(d_prep.cpu().numpy().view(np.uint32), prep)
    assert np.array_equal(d_fl.cpu().numpy().view(np.uint32), fl)
    return rc, out[:C.F12_WORDS * fstride].reshape(C.F12_WORDS, fstride).copy()


def run_fexp(K, words):
    """cck_fexp (k_fexp1) on a (144, n) word array of Miller values; returns the GT bytes per element."""
    import torch
    n = words.shape[1]
    d_f = _upload(words.reshape(-1))
    d_s = torch.zeros((72 * 12 * n,), dtype=torch.int32, device=_dev())  # slots.h: 72 x 12 x n words
    d_v = torch.full((n + SENT,), FILL, dtype=torch.uint8, device=_dev())
    d_gt = torch.full(((n + SENT) * C.GT_BYTES,), FILL, dtype=torch.uint8, device=_dev())
    torch.cuda.synchronize()
    rc = K.cck_fexp(n, _ptr(d_f), _ptr(d_s), None, _ptr(d_v), _ptr(d_gt), n, None)
    torch.cuda.synchronize()
    assert rc == 0
    v, g = d_v.cpu().numpy(), d_gt.cpu().numpy()
    assert bytes(v[n:]) == bytes([FILL]) * SENT, "verdict sentinels"
    assert bytes(g[n * C.GT_BYTES:]) == bytes([FILL]) * (SENT * C.GT_BYTES), "GT sentinels"
    gts = [bytes(g[C.GT_BYTES * i:C.GT_BYTES * (i + 1)]) for i in range(n)]
    assert [int(x) for x in v[:n]] == [int(gt == C.ONE_GT) for gt in gts]
    return gts


def run_reduce(K, words):
    """One level of the wide product tree on a (144, n) word array: (144, (n + 1) / 2)."""
    import torch
    n, n_out = words.shape[1], (words.shape[1] + 1) // 2
    d_in = _upload(words.reshape(-1))
    d_out = torch.full(((n_out * C.F12_WORDS + SENT) * 4,), FILL, dtype=torch.uint8, device=_dev())
    torch.cuda.synchronize()
    rc = K.cck_f12_reduce_wide(n, _ptr(d_in), _ptr(d_out), None)
    torch.cuda.synchronize()
    assert rc == 0
    out = d_out.cpu().numpy().view(np.uint32)
    assert bytes(out[n_out * C.F12_WORDS:].view(np.uint8)) == bytes([FILL]) * (4 * SENT), "output sentinels"
    return out[:n_out * C.F12_WORDS].reshape(C.F12_WORDS, n_out).copy()


@functools.lru_cache(maxsize=None)
def _tiled(K, n):
    """The tiled launch of n (miller_wide_cases.layout), once: (layout, Miller words, GT bytes)."""
    lay = M.layout(n)
    rc, words = run_miller(K, [M.pairs()[t] + (k,) for t, k, _ in lay], [fl for _, _, fl in lay])
    assert rc == 0
    words.setflags(write=False)
    return lay, words, run_fexp(K, words)


@functools.lru_cache(maxsize=None)
def golden():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "miller_wide_words.json")
    with open(path) as f:
        d = json.load(f)
    assert len(d["words"]) == M.NPAIR
    return [np.frombuffer(bytes.fromhex(h), dtype="<u4") for h in d["words"]]


@pytest.mark.parametrize("n", SIZES)
def test_gt_against_the_oracle(K, n):
    """GT bytes after cck_fexp equal the oracle's pairing for every computed pair, with P scaled by 1 and
    by a random k; a skipped pair (flag bit 0 or 2) writes exactly the stored form of 1; flag bits 1, 3,
    4, 5 and the high bits do not skip."""
    lay, words, gts = _tiled(K, n)
    seen = set()
    for i, (t, k, fl) in enumerate(lay):
        if fl & M.SKIP_MASK:
            assert np.array_equal(words[:, i], M.ONE_WORDS), (n, i, hex(fl))
            assert gts[i] == C.ONE_GT
        else:
            assert gts[i] == M.gt_of_pair(t), (n, i, t, k != 1, hex(fl))
        seen.add((k != 1, fl))
    C.decode(words.reshape(-1), n)  # every stored value canonical
    if n >= 255:  # both scalings under every flag word
        assert seen == {(s, fl) for s in (False, True) for fl in M.FLAG_WORDS}
        assert {fl for fl in M.FLAG_WORDS if not fl & M.SKIP_MASK} >= {2, 8, 16, 32, 0x3A}


@pytest.mark.parametrize("n", [16, 257])
def test_recorded_words(K, n):
    """The first 16 elements (the 16 pairs, k = 1, no flags) reproduce the recorded words exactly."""
    lay, words, _ = _tiled(K, n)
    assert [(t, k, fl) for t, k, fl in lay[:M.NPAIR]] == [(t, 1, 0) for t in range(M.NPAIR)]
    for t, want in enumerate(golden()):
        assert np.array_equal(words[:, t], want), (n, t)


@pytest.mark.parametrize("n", [16, 257])
def test_bilinearity(K, n):
    """e(a P, Q) = e(P, a Q) = e(P, Q)^a, byte for byte."""
    _, _, gts = _tiled(K, n)
    assert gts[M.NPAIR - 2] == gts[M.NPAIR - 1] != gts[0]
    e = B.gt_from_bytes(gts[0])
    assert B.gt_to_bytes(B.f12_pow(list(e), M.A)) == gts[M.NPAIR - 1]


@pytest.mark.parametrize("n", [4, 258])
def test_inverse_pairs_multiply_to_one(K, n):
    """e(P, Q) e(-P, Q) through cck_f12_reduce_wide and cck_fexp is exactly one (and neither factor is)."""
    items = []
    for t in range(n // 2):
        p, q = M.pairs()[t % M.NPAIR]
        k = M.scales()[t % M.NPAIR] if t % 2 else 1
        items += [(p, q, 1), (B.G1.neg(p), q, k)]
    rc, words = run_miller(K, items, [0] * n)
    assert rc == 0
    for i in (0, 1, n - 1):
        assert not np.array_equal(words[:, i], M.ONE_WORDS)
    assert run_fexp(K, run_reduce(K, words)) == [C.ONE_GT] * (n // 2)


@pytest.mark.parametrize("n", [5, 257])
def test_output_placement(K, n):
    """Element i goes to foff + i of stride fstride and nothing else is written; the words do not depend
    on the placement."""
    lay, words, _ = _tiled(K, 16 if n < 16 else n)
    lay = lay[:n]
    fstride, foff = n + 7, 3
    rc, out = run_miller(K, [M.pairs()[t] + (k,) for t, k, _ in lay], [fl for _, _, fl in lay], fstride, foff)
    assert rc == 0
    assert np.array_equal(out[:, foff:foff + n], words[:, :n])
    rest = np.delete(out, np.s_[foff:foff + n], axis=1)
    assert bytes(rest.view(np.uint8).reshape(-1)) == bytes([FILL]) * (4 * C.F12_WORDS * (fstride - n))


def test_rejected_and_empty_launches(K):
    """fstride < foff + n returns -1 and writes nothing; n = 0 returns 0 and writes nothing."""
    items = [M.pairs()[t] + (1,) for t in range(3)]
    for fstride, foff in ((2, 0), (3, 1), (5, 3)):
        rc, out = run_miller(K, items, [0] * 3, fstride, foff)
        assert rc == -1
        assert bytes(out.view(np.uint8).reshape(-1)) == bytes([FILL]) * (4 * C.F12_WORDS * fstride)
    import torch
    d = torch.full((4 * C.F12_WORDS,), FILL, dtype=torch.uint8, device=_dev())
    assert K.cck_miller_wide(0, _ptr(d), _ptr(d), _ptr(d), 0, 0, None) == 0
    torch.cuda.synchronize()
    assert bytes(d.cpu().numpy()) == bytes([FILL]) * (4 * C.F12_WORDS)
