"""CPU model of the cases in tests/vss_sets_cases.py (run on the device by tests/test_gpu_vss_sets.py): the CSR
form is a permutation of issuer_edges' batches, the torsion sets separate the reference's sum from Horner over
the integer id in both directions, the cancelling pairs cancel, and the size list is what its name says."""
import pytest

import issuer_edges as E
import vss_sets_cases as V
from fixed_edges import G1_IDENTITY, R


@pytest.fixture(scope="module")
def env(oc):
    return E.Env(oc, 1)


def test_the_arithmetic_behind_the_torsion_sets():
    i = (1 << 64) - 1
    assert pow(i, 4, R) % 3 == 1 and i ** 4 % 3 == 0
    assert pow(i, 4, R) % 11 == 1 and i ** 4 % 11 == 3
    assert pow(i, 5, R) % 11 == 0 and i ** 5 % 11 == 1


def test_csr_is_a_stable_sort_by_set(oc):
    call = E.vss_call(oc, 3, "rand")
    empty = 0
    for n in E.VSS_SIZES:
        batch = E.vss_batch(call, n, 1 if n > 1 else 0)
        rows, begin = V.csr(call, batch)
        assert len(begin) == len(call["sets"]) + 1 and begin[0] == 0 and begin[-1] == n
        assert sorted(map(id, rows)) == sorted(map(id, batch))
        for j in range(len(call["sets"])):
            assert all(c["set"] == j for c in rows[begin[j]:begin[j + 1]])
            assert [id(c) for c in rows[begin[j]:begin[j + 1]]] == [id(c) for c in batch if c["set"] == j]
        empty += sum(begin[j] == begin[j + 1] for j in range(len(call["sets"])))
    assert empty  # batches with empty sets among them


def test_torsion_sets_separate_the_reference_from_integer_horner(oc, env):
    calls = V.torsion_calls(oc)
    ref_only, horner_only = [], []
    for tc in calls:
        call = tc["call"]
        for j, C in enumerate(call["sets"]):  # irregular: exactly the sets with a point outside G1 (or such a g)
            outside = any(env.curve.mul_any(env.dec(p), R) is not None for p in C + [call["g"], call["h"]])
            assert outside == (j in tc["irregular"]), (tc["name"], j)
        for c in call["cases"]:
            ref, hor = E.expect_share(env, call, c), V.horner_verdict(env, call, c)
            assert ref == E.python_share(env, call, c), c["name"]
            if c["set"] not in tc["irregular"]:
                assert ref == hor == int("honest" in c["name"]), c["name"]
            elif ref and not hor:
                ref_only.append(c["name"])
            elif hor and not ref:
                horner_only.append(c["name"])
    assert f"c4_plus_T3/honest_id_{(1 << 64) - 1:x}" in horner_only  # valid by integer Horner, invalid by the reference
    assert f"c0_plus_c4_minus_T3/honest_id_{(1 << 64) - 1:x}" in ref_only  # the other way round
    want = [E.expect_share(env, calls[0]["call"], c) for c in calls[0]["call"]["cases"]]
    assert 0 < sum(want) < len(want)


def test_cancelling_pairs_cancel_unweighted(oc, env):
    call = V.cancel_call(oc)
    assert [E.expect_share(env, call, c) for c in call["cases"]] == [c["intent"] for c in call["cases"]]
    for pair in (0, 1):
        a, b = [c for c in call["cases"] if c["pair"] == pair]
        da, db = V.defect(env, call, a), V.defect(env, call, b)
        assert da != G1_IDENTITY and db != G1_IDENTITY
        assert env.msm([da, db], [1, 1]) == G1_IDENTITY
    assert all(V.defect(env, call, c) == G1_IDENTITY for c in call["cases"] if c["intent"])


def test_size_list(oc, env):
    call = V.sizes_call(oc)
    rows, begin = V.csr(call, call["cases"])
    assert rows == call["cases"]
    assert tuple(begin[j + 1] - begin[j] for j in range(len(V.SIZES))) == V.SIZES
    bad = [i for i, c in enumerate(rows) if not c["intent"]]
    assert 256 in bad and begin[V.SIZES.index(257)] in bad and begin[V.SIZES.index(63) + 1] - 1 in bad
    assert len(bad) == sum(len(v) for v in V.SIZES_BAD.values())
    probe = bad + [0, 1, 64, 65, 200, 581]  # every bad row and a few good ones through the oracle
    assert [E.expect_share(env, call, rows[i]) for i in probe] == [rows[i]["intent"] for i in probe]
