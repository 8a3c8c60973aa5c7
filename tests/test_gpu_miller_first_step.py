"""The two-pair Miller loops' first step (csrc/miller_lz.hip k_miller<SIG, false>): at the top bit f = 1,
so g starts from pair 0's line (or from the unit when pair 0 is skipped) and pair 1's line is multiplied
in; nothing is multiplied into the unit f.  Every combination of the two pairs' skip bits must still give
the oracle's pairing product over the pairs that are left, and exactly one when both are skipped.

cck_miller_lz_g2 and cck_miller_lz_g1 (twin = 0) are called as in tests/test_gpu_miller_lz_direct.py, on
credentials of tests/miller_lz_cases.py's tiled points; each Miller value goes through the quad final
exponentiation (cck_fexp with wide_max = 0) and is compared byte for byte with the C oracle's product.
The flag words 0, 1, 2, 4, 16 and 5 | 16 rotate credential by credential (neighbouring lane pairs of a
wave hold different combinations), at n = 2 (one partial wave; six launches, one per rotation) and at
n = 129 (crosses a 256-lane block; two rotations, so the credential past the block edge sees two
combinations).  The expectations are asserted on the CPU first (test_expectations).
"""
import numpy as np
import pytest

import fexp_direct_cases as C
import miller_lz_cases as M
from oracle import bls12_381 as B

FLAGS = (0, 1, 2, 4, 16, 5 | 16)
SKIPS = {0: (False, False), 1: (True, False), 2: (False, True), 4: (True, False), 16: (False, True),
         5 | 16: (True, True)}
SIZES = ((2, range(6)), (129, (0, 3)))
KINDS = ("g2", "g1")


def credentials(kind, n, rot):
    """Two-pair credentials over real points; credential c carries FLAGS[(c + c // 6 + rot) % 6]."""
    out = []
    for c in range(n):
        p1, q1 = M.tiled_pair(c)
        p2, q2 = M.second(c)
        s1 = M.Slot(M.REAL, None, q2) if kind == "g2" else M.Slot(M.REAL, p2, None)
        out.append((M.Slot(M.REAL, p1, q1), s1, FLAGS[(c + c // 6 + rot) % 6]))
    return out


def with_flags(creds, fl):
    return [(s0, s1, fl) for s0, s1, _ in creds]


def test_expectations(oc):
    """The skip rule of the six words; every combination reached at every size; an element's expectation
    is the product of its two pairs' own values, either one's alone, or exactly one."""
    assert {fl: M.skips2(fl) for fl in FLAGS} == SKIPS
    for kind in KINDS:
        for n, rots in SIZES:
            seen = set()
            for rot in rots:
                creds = credentials(kind, n, rot)
                fl = [cr[-1] for cr in creds]
                assert all(a != b for a, b in zip(fl, fl[1:]))  # neighbours differ
                seen |= set(fl)
                want = M.expected(oc, kind, creds)
                both = M.expected(oc, kind, with_flags(creds, 0))
                only0 = M.expected(oc, kind, with_flags(creds, 16))
                only1 = M.expected(oc, kind, with_flags(creds, 4))
                for c in range(n):
                    k0, k1 = SKIPS[fl[c]]
                    assert want[c] == (C.ONE_GT if k0 and k1 else only1[c] if k0 else only0[c] if k1 else both[c])
                    prod = B.f12_mul(list(B.gt_from_bytes(only0[c])), list(B.gt_from_bytes(only1[c])))
                    assert B.gt_to_bytes(prod) == both[c]
                    assert len({C.ONE_GT, both[c], only0[c], only1[c]}) == 4
            assert seen == set(FLAGS), (kind, n)
        fl129 = [[cr[-1] for cr in credentials(kind, 129, rot)] for rot in (0, 3)]
        assert fl129[0][128] != fl129[1][128] and fl129[0][127] != fl129[1][127]


def fexp_quad(K, words):
    """cck_fexp with wide_max = 0 (the quad kernel at every n) on a (144, n) word array: GT bytes per element."""
    import torch
    import test_gpu_miller_lz_direct as D
    n = words.shape[1]
    flat = np.ascontiguousarray(words).reshape(-1)
    d_f = D._upload(flat)
    d_v = torch.full((n + D.SENT,), D.FILL, dtype=torch.uint8, device=D._dev())
    d_gt = torch.full(((n + D.SENT) * C.GT_BYTES,), D.FILL, dtype=torch.uint8, device=D._dev())
    torch.cuda.synchronize()
    assert K.cck_fexp(n, D._ptr(d_f), None, None, D._ptr(d_v), D._ptr(d_gt), 0, None) == 0
    torch.cuda.synchronize()
    v, g = d_v.cpu().numpy(), d_gt.cpu().numpy()
    assert bytes(v[n:]) == bytes([D.FILL]) * D.SENT, "verdict sentinels"
    assert bytes(g[n * C.GT_BYTES:]) == bytes([D.FILL]) * (D.SENT * C.GT_BYTES), "GT sentinels"
    gts = [bytes(g[C.GT_BYTES * i:C.GT_BYTES * (i + 1)]) for i in range(n)]
    assert [int(x) for x in v[:n]] == [int(gt == C.ONE_GT) for gt in gts]
    return gts


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,rots", SIZES)
def test_every_skip_combination(oc, kind, n, rots):
    import test_gpu_miller_lz_direct as D
    K = D.launchers()
    for rot in rots:
        creds = credentials(kind, n, rot)
        rc, words, qc = D.run(K, "lz_" + kind, creds)
        assert rc == 0 and qc == D.QC
        want = M.expected(oc, kind, creds)
        got = fexp_quad(K, words)
        for c in range(n):
            assert got[c] == want[c], (kind, n, rot, c, creds[c][-1])
            # both pairs skipped: the stored form of 1 itself, and only then
            assert np.array_equal(words[:, c], M.ONE_WORDS) == (SKIPS[creds[c][-1]] == (True, True)), (kind, n, rot, c)
        C.decode(words.reshape(-1), n)  # every stored value canonical
