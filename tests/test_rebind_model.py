"""CPU checks of tests/rebind_cases.py: conditions on the inputs under which tests/test_gpu_rebind.py cannot
pass on stale context state.

* Discrimination: at every step of the rebind sequence, and for every consumer the GPU test observes there,
  what the oracle expects differs from what it expected before the step, so a buffer the step forgot to
  rewrite shows.  (Step 5 binds the same key at another table width: there nothing may change, and the GPU
  test reads the width back instead.)
* Under a world's own (g~, verkey) exactly its 6 valid rows verify, in all four forms; under each mismatched
  state none does and every GT differs from the matched states' GT.
* Every g~ encoding that decodes to the identity gives one and the same expectation, the encoding with
  coordinates >= p the honest one, and the small-order point is on the curve outside the subgroup.
* Under an identity g~ the pr = O row has oracle verdict 1 in all four forms: verdicts are at stake there,
  not only GT bytes.
"""
import pytest

import keygen_deal_cases as KD
import rebind_cases as RC

MODES = sorted(RC.MODES)
FORMS = ("verify", "verify_pervk", "pok", "pok_pervk")
WANT = [1] * RC.VALID + [0] * (RC.ROWS - RC.VALID)


def _gt_rows(gt):
    return [gt[576 * i:576 * (i + 1)] for i in range(RC.ROWS)] if isinstance(gt, bytes) else list(gt)


@pytest.mark.parametrize("mode", MODES)
def test_every_step_changes_what_every_consumer_is_expected_to_return(mode):
    before = None
    for label, (gw, vw) in RC.SEQUENCE:
        now = RC.observed(mode, RC.state(mode, gw, vw))
        if before is not None:
            for c in RC.CONSUMERS:
                if label in RC.SAME_STATE_STEPS:
                    assert now[c] == before[c], (label, c)
                else:
                    assert now[c] != before[c], (label, c)
        before = now


@pytest.mark.parametrize("mode", MODES)
def test_lone_g_tilde_rebind_changes_every_gt(mode):
    """Steps 1 and 4 change g~ alone: every row's GT moves in both plain forms, so no row can pass on a stale
    g~ constant whichever kernel reads it."""
    a = RC.observed(mode, RC.state(mode, "A", "A"))
    b = RC.observed(mode, RC.state(mode, "B", "A"))
    for f in ("verify", "verify_pervk"):
        for i, (x, y) in enumerate(zip(_gt_rows(a[f][1]), _gt_rows(b[f][1]))):
            assert x != y, (f, i)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(RC.WORLDS))
def test_matched_state_accepts_exactly_the_valid_rows(mode, name):
    e = RC.observed(mode, RC.state(mode, name, name))
    assert RC.world_of(mode, RC.state(mode, name, name)) == name
    for f in FORMS:
        assert list(e[f][0]) == WANT, f
        assert all(g is not None and any(g) for g in _gt_rows(e[f][1])), f
    assert e["engine"] is True


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gw,vw", [("B", "A"), ("A", "B")])
def test_mismatched_state_accepts_nothing_and_moves_every_gt(mode, gw, vw):
    e = RC.observed(mode, RC.state(mode, gw, vw))
    matched = [RC.observed(mode, RC.state(mode, n, n)) for n in sorted(RC.WORLDS)]
    for f in FORMS:
        assert not any(e[f][0]), f
    assert e["engine"] is False
    for f in ("verify", "verify_pervk"):
        for i, g in enumerate(_gt_rows(e[f][1])):
            assert any(g)
            for m in matched:
                assert g not in _gt_rows(m[f][1]), (f, i)
    # the proofs were made for another g~: the Schnorr check fails before any pairing
    for f in ("pok", "pok_pervk"):
        assert all(g is None for g in e[f][1]), f


@pytest.mark.parametrize("mode", MODES)
def test_degenerate_forms_decode_as_their_kind_says(mode):
    curve, _, dec, nbytes = KD.oth(mode)
    w = RC.world(mode, "A")
    kinds = {}
    for name, enc, kind in RC.degenerate_forms(mode):
        assert len(enc) == nbytes, name
        pt = dec(enc)
        kinds.setdefault(kind, []).append(name)
        if kind == "identity":
            assert pt is None, name
        elif kind == "alias":
            assert pt == w.g_tilde and enc != w.vk_bytes()[0], name
        else:
            assert pt is not None and curve.mul_any(pt, RC.R) is not None, name
        assert RC.in_subgroup(mode, enc) is (kind == "alias"), name
    assert len(kinds["identity"]) == (3 if mode == "G2" else 2)  # SigG2's g~ is in G1: a bad prefix too
    assert len(kinds["alias"]) == 1 and len(kinds["torsion"]) == 1


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("proofs", ["pok", "pok_id"])
def test_identity_forms_share_one_expectation_and_the_alias_is_honest(mode, proofs):
    honest = RC.state(mode, "A", "A")
    seen = []
    for name, enc, kind in RC.degenerate_forms(mode):
        e = RC.observed(mode, (enc,) + honest[1:], proofs)
        if kind == "identity":
            seen.append(e)
            assert e["engine"] is False, name
        elif kind == "alias":
            assert e == RC.observed(mode, honest, proofs), name
        else:
            assert e["engine"] is False, name
    assert all(e == seen[0] for e in seen[1:])
    assert seen[0] != RC.observed(mode, honest, proofs)


@pytest.mark.parametrize("mode", MODES)
def test_identity_g_tilde_accepts_the_pr_identity_row(mode):
    """e(sigma_1, O) e(-sigma_2, O) = 1: the oracle accepts row 7, and only row 7, under an identity g~.  The
    PoK forms reach the pairing with the proofs made under g~ = O (every row has a GT there); the proofs made
    under the honest g~ fail the Schnorr check."""
    honest = RC.state(mode, "A", "A")
    only = [int(i == RC.PR_O_ROW) for i in range(RC.ROWS)]
    one = None
    for name, enc, kind in RC.degenerate_forms(mode):
        if kind != "identity":
            continue
        e = RC.observed(mode, (enc,) + honest[1:], "pok_id")
        for f in FORMS:
            assert list(e[f][0]) == only, (name, f)
            gts = _gt_rows(e[f][1])
            assert all(g is not None for g in gts), (name, f)
            one = one or gts[RC.PR_O_ROW]
            assert gts[RC.PR_O_ROW] == one  # GT's identity
        e = RC.observed(mode, (enc,) + honest[1:], "pok")
        assert not any(e["pok"][0]) and all(g is None for g in e["pok"][1]), name
    # under the honest g~ the same row is one more bad credential
    assert RC.observed(mode, honest)["verify"][0][RC.PR_O_ROW] == 0


def test_tiling_repeats_rows_and_expectations_alike():
    b = RC.batch("G2", "B")
    t = RC.tile_batch(b, 24)
    assert t["n"] == 24 and t["s1"] == b["s1"] * 3 and t["vkY"] == b["vkY"] * 3
    e = RC.observed("G2", RC.state("G2", "B", "B"))
    v, gt = RC.tile_expect(e["verify"], 24)
    assert v == e["verify"][0] * 3 and gt[576 * 8:576 * 16] == e["verify"][1]
    v, gt = RC.tile_expect(e["pok"], 16)
    assert len(gt) == 16 and gt[8:] == e["pok"][1]
