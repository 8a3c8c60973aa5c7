"""GPU tests of the fixed-base window-table paths at edge scalars and exceptional sums (the cases of
tests/fixed_edges.py, whose branch coverage tests/test_fixed_edges_model.py asserts on the CPU):

* shared-verkey verify at table widths 8, 9, 10, 14, 16, 21 in both group modes: every case as a valid
  credential and as its twin with sigma_2 off by G (whose GT bytes pin the MSM's point), run as a small
  batch (one-wave prep), as single credentials, and tiled by repetition past kFexpWideMax (lane-pair prep)
  and past kWideMax (batch Miller loop): verdicts and GT bytes byte-exact against oc_verify_batch and the
  same every way; the RLC form's verdicts (rlc.hip reads the same tables);
* PoK verify at widths 8 and 14 with chosen responses (0, r - 1, small, non-canonical, empty / equal /
  opposite role shares, a chain through the identity), revealed messages 0 / small / r - 1 /
  non-canonical, J' = identity, for revealed sets {1, 4}, {} and all: against oc_pok_verify, through the
  one-block prep and, tiled past kPrepWideMax, the lane-pair prep (with q = 6 k_prep_pok_split's role A
  takes g~'s term alone: the boundary between the roles never falls inside the hidden responses here);
* cc_fixed_base_mul (8-bit storage-form tables) for edge scalars over the generator, a random point, the
  identity and an off-curve encoding, both groups, against oc_msm;
* the pinned staging ring of a concurrency slot (slots.h Staging): more cc_pok_verify_batch_device calls
  per slot than the ring has entries, each with its own revealed-index set, one of them large enough to
  regrow the ring.
"""
import ctypes
import sys

import numpy as np
import pytest

import fixed_edges as F
from conftest import ROOT, host_threads

sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

MODES = {"G2": 0, "G1": 1}
WIDE_MAX, FEXP_WIDE_MAX, PREP_WIDE_MAX = 4096, 2048, 1024  # slots.h kWideMax, kFexpWideMax, kPrepWideMax


def _ctx(mode):
    import coconut
    return coconut.Context(0, coconut.GroupMode(MODES[mode]))


def _tile(data, item, n):
    """The first n items of `data` (items of `item` bytes) repeated."""
    if not item:
        return b""  # nothing per item (no revealed message)
    k = len(data) // item
    return (data * ((n + k - 1) // k))[:n * item]


def _same_as_tiled(got, want, item, n):
    """got (n items) equals want (k items) repeated; returns the first differing index or -1."""
    k = len(want) // item
    g = np.frombuffer(got, np.uint8).reshape(n, item)
    w = np.frombuffer(want, np.uint8).reshape(k, item)
    bad = np.nonzero((g != w[np.arange(n) % k]).any(axis=1))[0]
    return int(bad[0]) if len(bad) else -1


@pytest.mark.parametrize("key", ["K0", "K1", "K2", "K3"])  # one table build a test (21 bits: seconds each)
@pytest.mark.parametrize("bits", F.WIDTHS)
@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_verify_edge_cases_every_table_width(oc, mode, bits, key):
    from coconut import verify_batch
    m = MODES[mode]
    sb = 192 if m == 0 else 97
    ctx = _ctx(mode)
    try:
        ctx.set_table_bits(bits, 0)
        vk, cases = next(s for s in F.verify_sets(bits, m) if s[0]["name"] == key)
        X, Y, g = F.verkey_bytes(oc, vk)
        b = F.verify_batch_inputs(oc, vk, cases)
        want_v, want_gt = F.oracle_verify(oc, vk, (X, Y, g), b, host_threads())
        assert want_v == b["expect"]  # the oracle agrees with the construction
        n, q, tag = b["n"], F.Q, (mode, bits, vk["name"])
        ctx.set_params(g)
        ctx.set_verkey(X, Y)
        assert ctx.table_bits()[0] == bits
        # a small batch: the one-wave prep
        v, gt = verify_batch(ctx, n, q, b["s1"], b["s2"], b["msgs"], want_gt=True)
        for i, name in enumerate(b["names"]):
            assert v[i] == want_v[i], (tag, name)
            assert gt[576 * i:576 * (i + 1)] == want_gt[576 * i:576 * (i + 1)], (tag, name)
        # single credentials
        for i in sorted(set(range(0, n, 7)) | {n - 2, n - 1}):
            v1, g1 = verify_batch(ctx, 1, q, b["s1"][i * sb:(i + 1) * sb], b["s2"][i * sb:(i + 1) * sb],
                                  b["msgs"][i * q * 48:(i + 1) * q * 48], want_gt=True)
            assert v1[0] == want_v[i] and g1 == want_gt[576 * i:576 * (i + 1)], (tag, b["names"][i])
        # tiled: the lane-pair prep (n > kFexpWideMax), then also the batch Miller loop (n > kWideMax)
        for N in (FEXP_WIDE_MAX + 1, WIDE_MAX + 8):
            vN, gN = verify_batch(ctx, N, q, _tile(b["s1"], sb, N), _tile(b["s2"], sb, N),
                                  _tile(b["msgs"], q * 48, N), want_gt=True)
            i = _same_as_tiled(vN.tobytes(), bytes(want_v), 1, N)
            assert i < 0, (tag, N, i, b["names"][i % n])
            i = _same_as_tiled(gN, want_gt, 576, N)
            assert i < 0, (tag, N, i, b["names"][i % n])
        # the RLC form reads the same tables (delta-MSM and fold points)
        vr = verify_batch(ctx, n, q, b["s1"], b["s2"], b["msgs"], rlc=True)
        assert [int(x) for x in vr] == want_v, (tag, [nm for nm, a, e in zip(b["names"], vr, want_v) if a != e])
        # ... and accepts the valid ones on its own (fixed seed): above, a rejected batch falls back to the
        # per-credential path, which gives these verdicts whatever the RLC check computed.  K1's X~ is the
        # identity, which the RLC mode does not count as a subgroup point (capi_ctx.cpp refresh_vk_subgroup):
        # under that verkey it never accepts
        from test_gpu_rlc_fold_direct import rlc_engine_accepts
        ok = [i for i in range(n) if want_v[i]]
        pick = lambda x, item: b"".join(x[i * item:(i + 1) * item] for i in ok)  # noqa: E731
        assert ok and rlc_engine_accepts(ctx, len(ok), q, pick(b["s1"], sb), pick(b["s2"], sb),
                                         pick(b["msgs"], q * 48)) is (vk["x"] != 0), tag
    finally:
        ctx.close()


POK_SETS = ([1, 4], [], list(range(F.POK_Q)))


def _run_pok(ctx, b, q, lo=0, hi=None, tile=None):
    from coconut import pok_verify_batch
    m = int(ctx.mode)
    sb, ob = (192, 97) if m == 0 else (97, 192)
    nr, r = b["nresp"], len(b["revealed"])
    if tile:
        f = lambda k, item: _tile(b[k], item, tile)  # noqa: E731
        n = tile
    else:
        hi = b["n"] if hi is None else hi
        f = lambda k, item: b[k][lo * item:hi * item]  # noqa: E731
        n = hi - lo
    return pok_verify_batch(ctx, n, q, b["revealed"], nr, f("s1", sb), f("s2", sb), f("J", ob), f("T", ob),
                            f("resp", nr * 48), f("chal", 48), f("rev", r * 48), want_gt=True)


@pytest.mark.parametrize("bits", F.POK_WIDTHS)
@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_pok_edge_cases(oc, mode, bits):
    m = MODES[mode]
    ctx = _ctx(mode)
    try:
        ctx.set_table_bits(bits, 0)
        vk = F.make_pok_verkey(bits, m)
        vkb = F.verkey_bytes(oc, vk)
        ctx.set_params(vkb[2])
        ctx.set_verkey(vkb[0], vkb[1])
        assert ctx.table_bits()[0] == bits
        for rev in POK_SETS:
            b = F.pok_batch_inputs(oc, vk, F.make_pok_cases(vk, rev), rev)
            want = F.oracle_pok(oc, vk, vkb, b)
            n = b["n"]
            assert n <= PREP_WIDE_MAX
            v, gt = _run_pok(ctx, b, F.POK_Q)  # the one-block-per-proof prep
            for i, name in enumerate(b["names"]):
                assert v[i] == want[i][0], (mode, bits, rev, name)
                if want[i][1] is not None:
                    assert gt[576 * i:576 * (i + 1)] == want[i][1], (mode, bits, rev, name)
            N = PREP_WIDE_MAX + 1  # the lane-pair prep
            vN, gN = _run_pok(ctx, b, F.POK_Q, tile=N)
            i = _same_as_tiled(vN.tobytes(), v.tobytes(), 1, N)
            assert i < 0, (mode, bits, rev, i, b["names"][i % n])
            i = _same_as_tiled(gN, gt, 576, N)
            assert i < 0, (mode, bits, rev, i, b["names"][i % n])
            for i in (0, 1, n - 1):  # and one at a time
                v1, g1 = _run_pok(ctx, b, F.POK_Q, i, i + 1)
                assert v1[0] == v[i] and g1 == gt[576 * i:576 * (i + 1)], (mode, bits, rev, b["names"][i])
    finally:
        ctx.close()


@pytest.mark.parametrize("group", [1, 2])
def test_fixed_base_mul_edge_scalars(oc, group):
    import coconut
    eb = 97 if group == 1 else 192
    ks = F.fbm_scalars()
    kb = b"".join(F.be48(k) for k in ks)
    ctx = _ctx("G2")
    try:
        for name, base in F.fbm_bases(oc, group):
            got = coconut.fixed_base_mul(ctx, group, base, kb)
            want = F.oracle_mul(oc, group, base, ks)
            for i, k in enumerate(ks):
                assert got[eb * i:eb * (i + 1)] == want[eb * i:eb * (i + 1)], (group, name, hex(k))
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_concurrent_pok_slots_many_uploads(oc, mode):
    """cc_set_concurrency(2), fourteen cc_pok_verify_batch_device calls on two streams with no host
    synchronisation in between: seven per slot, more than the four entries of a slot's pinned staging ring,
    so entries are reused.  Every call has its own revealed-index set; the seventh and eighth have r = 17
    (68 bytes, past the ring's first 64-byte entries: the grow path, once per slot), later calls return to
    small sets.  A proof checked against another call's indices fails its Schnorr check, so an entry
    overwritten before its copy ran shows as a wrong verdict."""
    import torch
    from coconut import _lib
    m = MODES[mode]
    q, bits = 20, 8
    big = list(range(1, 18))
    sets = [[1, 4], [0], [2, 3], [5], [6, 7], [3, 9], big, big[1:] + [19], [1], [4, 1], [10, 11, 12], [19], [0, 2],
            [8]]
    assert len(sets) >= 2 * 6 and len({tuple(s) for s in sets}) == len(sets)
    assert all(4 * len(s) <= 64 for s in sets[:6]) and 4 * len(big) > 64
    ctx = _ctx(mode)
    try:
        ctx.set_table_bits(bits, 0)
        vk = F.make_pok_verkey(bits, m, q=q)
        vkb = F.verkey_bytes(oc, vk)
        ctx.set_params(vkb[2])
        ctx.set_verkey(vkb[0], vkb[1])
        dev = torch.device("cuda", 0)
        to = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)  # noqa: E731
        P = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
        calls = []
        for rev in sets:
            cases = [c for c in F.make_pok_cases(vk, rev) if c["name"] in ("random", "resp_small", "rev_small")]
            b = F.pok_batch_inputs(oc, vk, cases, rev)
            D = {k: to(b[k]) for k in ("s1", "s2", "J", "T", "resp", "chal", "rev")}
            calls.append((b, D, F.oracle_pok(oc, vk, vkb, b)))
        ctx.set_concurrency(2)
        try:
            streams = [torch.cuda.Stream(dev) for _ in range(2)]
            # the outputs are zero-filled on the current stream, the calls run on side streams: every fill
            # has ended (synchronize) before the first call is queued, so no fill can land on a result
            outs = [(torch.zeros(b["n"], dtype=torch.uint8, device=dev),
                     torch.zeros(b["n"] * 576, dtype=torch.uint8, device=dev)) for b, _, _ in calls]
            torch.cuda.synchronize()
            for k, (b, D, _) in enumerate(calls):
                n, r = b["n"], len(b["revealed"])
                v, gt = outs[k]
                st = streams[k % 2]
                st.wait_stream(torch.cuda.current_stream(dev))
                ridx = (ctypes.c_uint64 * max(r, 1))(*b["revealed"])
                assert _lib.lib.cc_pok_verify_batch_device(ctx.h, n, q, r, b["nresp"], P(D["s1"]), P(D["s2"]), P(D["J"]),
                                                           P(D["T"]), P(D["resp"]), P(D["chal"]), ridx, P(D["rev"]),
                                                           P(v), P(gt), ctypes.c_void_p(st.cuda_stream)) == 0
            torch.cuda.synchronize()
            for k, ((b, _, want), (v, gt)) in enumerate(zip(calls, outs)):
                v, gt = v.cpu().numpy(), bytes(gt.cpu().numpy())
                assert any(w[0] for w in want)  # each call has proofs that only its own index set accepts
                for i, name in enumerate(b["names"]):
                    assert v[i] == want[i][0], (k, b["revealed"], name)
                    if want[i][1] is not None:
                        assert gt[576 * i:576 * (i + 1)] == want[i][1], (k, b["revealed"], name)
        finally:
            ctx.set_concurrency(1)
    finally:
        ctx.close()
