"""CPU test of the cases of tests/issuer_device_cases.py themselves: conditions on the INPUTS that
tests/test_gpu_issuer_device.py feeds cc_sigreq_verify_batch_device, not on the device.

* the model of the device form's window schedule (issuer_device_cases.model: signed 4-bit digits over a
  per-request table of multiples, the fixed-base tables' 8-bit windows, then -T) gives, for every request, the
  verdict of the C oracle's sums (issuer_edges.expect_request) and the verdict the construction intends;
* every named case reaches, in that model, the branch it is named for, in the check kind it names;
* the union of the cases reaches every branch of an addition in the variable-base streams, in the fixed-base
  part and at -T, and (SigG1, the order-3 points) in the construction of the table;
* the recoding: every scalar used recodes to 65 digits in [-7, 8] that sum back to the scalar mod r with
  digit 64 zero (no carry leaves the top window of a reduced scalar, no digit is -8), the all-8 and all-9
  scalars give the digits 8 and -7 / -6, and the zero-middle scalar has 61 zero digits in a row.
"""
import collections

import pytest

import issuer_device_cases as D
import issuer_edges as E
from fixed_edges import R

MODES = ("G2", "G1")


def _env(oc, mode):
    return E.Env(oc, 2 if mode == "G2" else 1)


@pytest.mark.parametrize("mode", MODES)
def test_model_verdicts_and_branches(oc, mode):
    env = _env(oc, mode)
    call = D.device_call(oc, mode)
    assert (call["q"], call["k"]) == (D.Q, D.K)
    union = collections.defaultdict(set)
    named = 0
    for req in call["reqs"]:
        want = E.expect_request(env, call, req)
        assert want == req["intent"], req["name"]
        got, logs = D.model_request(env, call, req)
        assert got == want, (req["name"], got, want)
        for key, log in logs.items():
            union[key[0]] |= set(log)
        for kind, branch in req["reach"]:
            seen = set().union(*(set(log) for key, log in logs.items() if key[0] == kind))
            assert branch in seen, (req["name"], kind, branch, sorted(seen))
            named += 1
    assert named >= 20
    exp = [r["intent"] for r in call["reqs"]]
    assert 0 < sum(exp) < len(exp)
    assert len({r["name"] for r in call["reqs"]}) == len(call["reqs"])
    every = set().union(*union.values())
    for stream in ("c", "fixed", "final"):
        for b in ("fresh", "doubling", "to-identity", "general") + (("from-identity",) if stream == "c" else ()):
            if (stream, b) in (("fixed", "fresh"), ("final", "doubling"), ("final", "general")):
                continue  # a zero challenge multiple / a negated T / a wrong T: issuer_edges.py's cases
            assert f"{stream}:{b}" in every, (stream, b)
    assert {"h:doubling", "h:to-identity", "pk:from-identity", "final:skipped", "c:skipped-multiple" if mode == "G1"
            else "c:to-identity"} <= every
    if mode == "G1":
        assert {"table:to-identity", "table:from-identity", "table:doubling", "table:general"} <= every
    # in ct2 all three streams add in one window; in every kind the fixed part follows the chain
    assert {"pk:fresh", "h:general", "c:general"} <= union["ct2"]
    assert not any(b.startswith("fixed:") for b in union["ct2"])
    for kind in ("sk", "comm", "ct1"):
        assert any(b.startswith("fixed:") for b in union[kind]), kind


@pytest.mark.parametrize("mode", MODES)
def test_recoding_of_every_scalar_used(oc, mode):
    call = D.device_call(oc, mode)
    vals = {v for r in call["reqs"] for v in D.scalars_of(r)} | {v for _, v in D.EDGE_SCALARS}
    assert {0, 1, R - 1, R, R + 1, (1 << 384) - 1} <= vals
    lo, hi = 0, 0
    for v in vals:
        d = D.recode(v)
        assert len(d) == 65 and d[64] == 0, hex(v)
        assert sum(x << (4 * w) for w, x in enumerate(d)) == v % R, hex(v)
        lo, hi = min(lo, *d), max(hi, *d)
    assert (lo, hi) == (-7, 8)
    assert D.recode(D.ALL8)[:63] == [8] * 63
    assert D.recode(D.ALL9)[:63] == [-7] + [-6] * 62 and D.recode(D.ALL9)[63] == 1
    z = D.recode(D.ZERO_MIDDLE)
    assert z[0] == 3 and z[62] == 5 and not any(z[1:62])
    assert D.recode(8) == [8] + [0] * 64 and D.recode(9)[:2] == [-7, 1]
    top = D.recode(R - 1)
    assert top[63] == 7 and top[64] == 0  # the top window of the largest reduced scalar
