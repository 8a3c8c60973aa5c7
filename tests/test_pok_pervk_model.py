"""CPU checks of tests/pok_pervk_cases.py, the inputs of tests/test_gpu_pok_pervk.py:

* every list's intended verdicts equal oc_pok_verify called per proof with that proof's own verkey, and
  every list holds both verdicts;
* each steered case reaches the branch it is named for in the model of pok_pervk.hip's two chains (the
  sum doubles, cancels, or restarts from the identity), and each chain of the model ends on the sum the
  integers give;
* the table order and the roles k_pok_var_scalars derives from an unsorted index list."""
import pytest

import pok_pervk_cases as C
from conftest import host_threads
from fixed_edges import CHAIN, R
from straus_edges import M

MODES = (0, 1)


def _check(oc, b):
    want = C.oracle_pok(oc, b, threads=host_threads())
    bad = [(nm, e, w[0]) for nm, e, w in zip(b["names"], b["expect"], want) if e != w[0]]
    assert not bad, bad[:8]
    assert set(b["expect"]) == {0, 1}
    return want


@pytest.mark.parametrize("name", sorted(C.EDGE_LISTS))
@pytest.mark.parametrize("mode", MODES)
def test_edge_lists_intended_verdicts_equal_the_oracle(oc, mode, name):
    b = C.edge_batch(oc, C.EDGE_LISTS[name](mode))
    want = _check(oc, b)
    # a proof rejected before the pairing leaves no GT; an accepted one pairs to one
    one = bytes(47) + b"\x01" + bytes(528)
    assert all(gt == one for (v, gt) in want if v == 1)


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
@pytest.mark.parametrize("mode", MODES)
def test_distinct_verkey_lists_intended_verdicts_equal_the_oracle(oc, mode, shape):
    q, rev = shape
    b = C.distinct_batch(C.oracle_mul(oc, host_threads()), mode, 13, q, rev, seed=900 + 10 * q + mode)
    _check(oc, b)
    assert set(b["names"]) >= {"valid", "bad_response", "next_key"}
    # the valid proofs under one another's keys: every one rejected; the proof made under the next proof's
    # key is accepted under it
    rot = C.rotate_keys(C.take(b, [i for i, e in enumerate(b["expect"]) if e]))
    assert [v for v, _ in C.oracle_pok(oc, rot, threads=host_threads())] == [0] * rot["n"]
    got = [v for v, _ in C.oracle_pok(oc, C.rotate_keys(b), threads=host_threads())]
    assert got == [int(nm == "next_key") for nm in b["names"]]


@pytest.mark.parametrize("name", sorted(C.EDGE_LISTS))
@pytest.mark.parametrize("mode", MODES)
def test_steered_cases_reach_their_branches(mode, name):
    L = C.EDGE_LISTS[name](mode)
    seen = set()
    for c in L["cases"]:
        tr = C.trace(L, c)
        assert set(tr["A"]) | set(tr["B"]) <= set(CHAIN)
        assert tr["finalA"] == (C.sum_a(L, c) - c["t"]) % M, c["name"]
        assert tr["finalB"] == C.jprime(L, c), c["name"]
        for chain, br in c["reach"]:
            assert br in tr[chain], (c["name"], chain, br, tr[chain])
            seen.add((chain, br))
    if name == "bases":
        assert seen >= {(ch, br) for ch in "AB" for br in ("fresh", "doubling", "to-identity", "from-identity")}
        cancel = next(c for c in L["cases"] if c["name"] == "chainB_cancel")
        assert C.trace(L, cancel)["skipB"] >= 1  # the identity met a round of doublings in mid-walk
    if name == "unrevealed":
        assert seen >= {("B", "fresh"), ("B", "doubling"), ("B", "to-identity")}


def test_table_order_and_roles_of_an_unsorted_index_list():
    """The scalars kernel's mapping restated: base 1 + j takes revealed message z where idx[z] = j, else
    response 1 + (j - #revealed indices below j).  terms_a / terms_b must pick the same scalars."""
    rev, q = [5, 2], 6
    L = dict(mode=0, q=q, rev=rev, gk=7)
    c = dict(resp=[100, 101, 102, 103, 104], chal=9, revm=[55, 22], y=[10 ** (j + 1) for j in range(q)], j=3, x=1)
    role, scal = [], []
    for j in range(q):
        below = sum(x < j for x in rev)
        if j in rev:
            role.append(1)
            scal.append(c["revm"][rev.index(j)])
        else:
            role.append(0)
            scal.append(c["resp"][1 + j - below])
    assert role == [0, 0, 1, 0, 0, 1]
    assert scal == [101, 102, 22, 103, 104, 55]
    assert [s for _, s in C.terms_a(L, c)] == [100, 101, 102, 103, 104, 9]
    assert C.terms_b(L, c) == [(10 ** 3, 22), (10 ** 6, 55)]


def test_edge_scalars_cover_the_recoding_edges():
    from straus_edges import digits
    assert {0, 1, R - 1, R, R + 1, (1 << 384) - 1} <= set(C.EDGE_SCALARS)
    d8, d7 = digits(int("8" * 64, 16)), digits(int("7" * 64, 16))
    assert len(d8) == 65 and len(d7) == 65
    top = digits((1 << 254) | (0xF << 248))
    assert top[62] == -1 and top[63] == 5 and top[64] == 0  # the carry out of nibble 62 into the top nibble
