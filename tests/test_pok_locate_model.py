"""CPU side of the PoK RLC locate mode (cc_pok_verify_batch_locate*): the inputs of tests/test_gpu_pok_locate.py
(tests/pok_locate_cases.py) checked against the fixtures' recorded verdicts, and the product tree's alignment
that the segmented partial relies on when two proofs share a Miller value, so a GPU failure there is the
library's and not the test's."""
import numpy as np
import pytest

import pok_locate_cases as P
import rlc_locate_cases as L


@pytest.mark.parametrize("mode", [0, 1])
def test_placed_proofs_carry_the_fixture_verdicts(mode):
    """Every fixture proof's recorded verdict is 1 for the three valid ones and 0 for each corruption kind; a
    built batch holds exactly the placed proofs, and its expected verdicts are the recorded ones."""
    d = P.fixture(mode)
    rec = {p["kind"]: p["verdict"] for p in d["proofs"]}
    assert rec == dict(valid=1, **{k: 0 for k in P.KINDS})
    assert sum(p["kind"] == "valid" for p in d["proofs"]) == 3
    assert P.batch(mode, P.N)["expect"].all()
    w = None
    for kind in P.KINDS:
        b = P.batch(mode, P.N, ((P.KIND_AT, kind),))
        w = w or P.widths(mode, b["nresp"], len(b["revealed"]))
        assert b["nresp"] == P.Q - len(b["revealed"]) + 1
        assert list(np.flatnonzero(b["expect"] == 0)) == [P.KIND_AT]
        bad = next(p for p in d["proofs"] if p["kind"] == kind)
        one = P.slice_of(b, P.KIND_AT, P.KIND_AT + 1)
        assert one["s1"] == bytes.fromhex(bad["sigma1"]) and one["chal"] == bytes.fromhex(bad["chal"])
        assert one["J"] == bytes.fromhex(bad["J"]) and one["T"] == bytes.fromhex(bad["T"])
        for k in P.KEYS:
            assert len(b[k]) == P.N * w[k], k
    # the tiling: proof i is valid proof i % 3
    b = P.batch(mode, 7)
    assert P.slice_of(b, 3, 4)["s2"] == P.slice_of(b, 0, 1)["s2"] != P.slice_of(b, 1, 2)["s2"]


def test_flagged_kinds_are_those_the_unsegmented_partial_flags():
    """tests/test_gpu_pok_rlc.py test_each_failure_kind_alone_is_rejected asserts the batch-wide word is 0 for
    bad_revealed alone (only the pairing equation fails) and 1 for the other four kinds; the per-segment words
    must follow the same split."""
    assert set(P.FLAGGED) | set(P.UNFLAGGED) == set(P.KINDS) and not set(P.FLAGGED) & set(P.UNFLAGGED)
    assert P.UNFLAGGED == ("bad_revealed",)
    assert set(P.FLAGGED) == {"bad_chal", "bad_response", "bad_J", "sigma1_inf"}


@pytest.mark.parametrize("n,seg", P.SHAPES + ((149, 16), (300, 4), (65536, 1024), (65535, 16384)))
def test_twin_product_tree_keeps_segments_aligned(n, seg):
    """k_miller<SIG, true> puts proofs 2 j and 2 j + 1 into Miller value j: N = ceil(n / 2) values.  The tree is
    pairwise with the tail kept alone; after log2(seg / 2) levels (fewer when the tree is already down to one
    value) the level must have S = ceil(n / seg) elements, element s holding exactly the Miller values of the
    proofs [s seg, (s + 1) seg), and the loop's flag word index j >> (log2 seg - 1) must be j's segment."""
    k = (seg // 2).bit_length() - 1
    assert 2 << k == seg
    nv, S = (n + 1) // 2, -(-n // seg)
    size, steps = nv, 0
    while size > S:
        size, steps = (size + 1) // 2, steps + 1
    assert size == S and steps <= k and (steps == k or S == 1)
    if nv > 4096:  # the big shapes: the index arithmetic alone
        return
    level = L.tree_level(nv, steps)
    values = P.twin_values(n)
    assert len(level) == S
    for s, idx in enumerate(level):
        proofs = [c for j in idx for c in values[j]]
        assert proofs == list(range(s * seg, min(n, (s + 1) * seg)))
        assert all(j >> k == s for j in idx)


def test_bad_indices_fall_in_the_expected_segments():
    for n, seg, i, s, length in P.LOCATE_ONE:
        assert i // seg == s and min(n, (s + 1) * seg) - s * seg == length, i
    one = {(n, seg): [] for n, seg, *_ in P.LOCATE_ONE}
    for n, seg, i, *_ in P.LOCATE_ONE:
        one[(n, seg)].append(i)
    assert one[(150, 16)][0] % 16 == 0 and one[(150, 16)][1] % 16 == 15
    assert [i % 2 for i in one[(150, 16)][2:]] == [0, 1] and one[(150, 16)][2] // 2 == one[(150, 16)][3] // 2
    assert one[(149, 16)] == [148] and 149 % 2 == 1       # the last loop's second pair is skipped
    assert one[(129, 64)] == [127, 128]                   # either side of the 128-proof block edge of the prep
    for bad, segs, rechecked in P.LOCATE_TWO:
        assert tuple(i // P.SEG for i in bad) == segs
        assert rechecked == sum(min(P.N, (s + 1) * P.SEG) - s * P.SEG for s in segs)
    assert sorted(i // P.EVERY_SEG for i in P.EVERY_BAD) == list(range(-(-P.EVERY_N // P.EVERY_SEG)))
    assert P.KIND_AT // P.SEG == 4 and -(-P.N // P.SEG) == 10
