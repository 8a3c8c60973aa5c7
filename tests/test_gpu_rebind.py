"""GPU tests of rebinding Params and Verkey on a live context, and of a g~ that does not decode, both group
modes, byte-exact against the oracle (tests/rebind_cases.py; its inputs are checked on the CPU by
tests/test_rebind_model.py).

cc_set_params under an existing verkey patches the verkey block's g~ slot, recomputes the subgroup status and
rebuilds the tables; every other GPU test follows it with cc_set_verkey, which rewrites all of that before a
kernel reads it.  Here every reader of a g~-derived buffer is observed after every single rebind:

    gtilde_aff                    verify at n = 8 (k_miller_wide2), 136 (k_miller_wide), 2056 (past
                                  kFexpWideMax); per-verkey verify and PoK
    gtilde_lz / gtilde_lines      verify at n = 4104 (past kWideMax: the pair-lane k_miller)
    vk_aff / vk_inf slot q + 1,   PoK verify at n = 8 and 1032 (past kPrepWideMax), the PoK provers (J and T
    base q of the table           use g~'s table)
    rlc_pw, the X~ table base     the RLC engine on its own (fixed seed, no fallback), verify_batch(rlc=True),
                                  the locate modes
    vk_subgroup                   the RLC engine under a g~ outside the subgroup

through the C ABI (no Python cache between the test and cc_set_params / cc_set_verkey) and again through the
Context methods; then with concurrency slots in flight, after failed calls, and with every degenerate g~.
The contexts are the tests' own, their tables forced to 8 bits unless a step says otherwise."""
import ctypes
import functools

import numpy as np
import pytest

import rebind_cases as RC

pytestmark = pytest.mark.gpu

MODES = sorted(RC.MODES)
VERIFY_N = (8, 136, 2056, 4104)
PERVK_N = (8, 1032)
POK_N = (8, 1032)
RLC_N = (8, 4104)
ERR_LEN, ERR_DECODE = -1, -4


def _lib():
    from coconut import _lib
    return _lib.lib


def _new_ctx(mode, bits=8):
    import coconut
    ctx = coconut.Context(0, coconut.GroupMode(RC.MODES[mode]))
    ctx.set_table_bits(bits, 0)
    return ctx


def _set_params(ctx, how, g):
    if how == "abi":
        assert _lib().cc_set_params(ctx.h, g) == 0
        ctx._gtilde = g
    else:
        ctx.set_params(g)


def _set_verkey(ctx, how, mode, X, Y):
    if how == "abi":
        assert _lib().cc_set_verkey(ctx.h, X, Y, len(Y) // RC.sizes(mode)[1]) == 0
        ctx._vk = (X, Y)
    else:
        ctx.set_verkey(X, Y)


def _bind(ctx, how, mode, st):
    _set_params(ctx, how, st[0])
    _set_verkey(ctx, how, mode, st[1], st[2])


def _same(tag, got_v, got_gt, want_v, want_gt):
    """Verdicts, and GT bytes wherever the oracle has some (a PoK rejected before the pairing has none)."""
    got_v = [int(x) for x in got_v]
    assert got_v == list(want_v), (tag, [i for i, (a, b) in enumerate(zip(got_v, want_v)) if a != b][:8])
    if isinstance(want_gt, bytes):
        if got_gt != want_gt:
            bad = [i for i in range(len(want_v)) if got_gt[576 * i:576 * (i + 1)] != want_gt[576 * i:576 * (i + 1)]]
            raise AssertionError((tag, "GT rows", bad[:8], len(bad)))
    else:
        bad = [i for i, w in enumerate(want_gt) if w is not None and got_gt[576 * i:576 * (i + 1)] != w]
        assert not bad, (tag, "GT rows", bad[:8], len(bad))


def _pok_args(t):
    return (t["n"], t["q"], t["revealed"], t["nresp"], t["ps1"], t["ps2"], t["J"], t["T"], t["resp"], t["chal"], t["rev"])


def checks(ctx, mode, st, where, proofs="pok", verify_n=VERIFY_N, pervk_n=PERVK_N, pok_n=POK_N, plain=True,
           prove=False):
    """[(tag, check)]: every consumer under state st against the oracle, for the batch whose q the bound verkey
    has; the other world's q is refused.  plain=False: the PoK consumers only (a second set of proofs over the
    same rows); prove: the provers' bytes equal the oracle's proofs (the proofs must have been made under st's
    g~).  A check asserts; the tags name what a failure report is about."""
    from coconut import (pok_gen_proof_batch, pok_init_batch, pok_verify_batch, pok_verify_batch_locate, verify_batch,
                         verify_batch_locate)
    from test_gpu_rlc_fold_direct import rlc_engine_accepts
    name = RC.world_of(mode, st)
    e = RC.observed(mode, st, proofs)
    b = RC.batch(mode, name, proofs)
    q = b["q"]
    tiled = functools.lru_cache(None)(lambda n: RC.tile_batch(b, n))
    out = []

    def add(*tag):
        return lambda fn: out.append(((where,) + tag, fn))

    def verify(n, form):
        t = tiled(n)
        vk = (t["vkX"], t["vkY"]) if form == "verify_pervk" else None
        v, gt = verify_batch(ctx, n, q, t["s1"], t["s2"], t["msgs"], vk=vk, want_gt=True)
        _same((where, form, n), v, gt, *RC.tile_expect(e[form], n))

    def pok(n, form):
        t = tiled(n)
        v, gt = pok_verify_batch(ctx, *_pok_args(t), want_gt=True, vk=(t["vkX"], t["vkY"]) if form == "pok_pervk" else None)
        _same((where, form, n), v, gt, *RC.tile_expect(e[form], n))

    def verdicts(n, form):
        t = tiled(n)
        if form == "rlc":
            v = verify_batch(ctx, n, q, t["s1"], t["s2"], t["msgs"], rlc=True)
        elif form == "locate":
            v, _ = verify_batch_locate(ctx, n, q, t["s1"], t["s2"], t["msgs"], seg=4)
        else:
            v, _ = pok_verify_batch_locate(ctx, *_pok_args(t), seg=4)
        want = RC.tile_expect(e["pok" if form == "pok_locate" else "verify"], n)[0]
        assert [int(x) for x in v] == want, (where, form, n)

    def provers():
        s1, s2, J, T, rand = pok_init_batch(ctx, 8, q, b["revealed"], b["s1"], b["s2"], b["msgs"], b["rand"])
        assert (s1, s2, J, T) == (b["ps1"], b["ps2"], b["J"], b["T"]), (where, "pok_init")
        assert pok_gen_proof_batch(ctx, 8, q, b["revealed"], b["msgs"], rand, b["chal"]) == b["resp"], (where, "gen_proof")

    def engine():
        assert rlc_engine_accepts(ctx, RC.VALID, q, *RC.valid_rows(b)) is e["engine"], (where, "engine", e["engine"])

    def other_q():  # the other world's q is not the bound verkey's
        o = RC.batch(mode, "B" if name == "A" else "A")
        res = np.zeros(8, dtype=np.uint8)
        P = ctypes.c_void_p(res.ctypes.data)
        assert _lib().cc_verify_batch(ctx.h, 8, o["q"], o["s1"], o["s2"], o["msgs"], None, None, P, None, 0) == ERR_LEN, where
        idx = (ctypes.c_uint64 * len(o["revealed"]))(*o["revealed"])
        assert _lib().cc_pok_verify_batch(ctx.h, 8, o["q"], len(o["revealed"]), o["nresp"], o["ps1"], o["ps2"], o["J"],
                                          o["T"], o["resp"], o["chal"], idx, o["rev"], P, None) == ERR_LEN, where

    if plain:
        for n in verify_n:
            add("verify", n)(functools.partial(verify, n, "verify"))
        for n in pervk_n:
            add("verify_pervk", n)(functools.partial(verify, n, "verify_pervk"))
    for n in pok_n:
        add("pok", n)(functools.partial(pok, n, "pok"))
    add("pok_pervk", 8)(functools.partial(pok, 8, "pok_pervk"))
    add("pok_locate", 8)(functools.partial(verdicts, 8, "pok_locate"))
    if prove:
        add("provers", 8)(provers)
    if plain:
        for n in RLC_N:
            add("rlc", n)(functools.partial(verdicts, n, "rlc"))
            add("locate", n)(functools.partial(verdicts, n, "locate"))
        add("engine", RC.VALID)(engine)
        add("other_q", 8)(other_q)
    return out


def observe(ctx, mode, st, where, **kw):
    for _, check in checks(ctx, mode, st, where, **kw):
        check()


@pytest.mark.parametrize("how", ["abi", "methods"])
@pytest.mark.parametrize("mode", MODES)
def test_every_consumer_after_every_rebind(mode, how):
    """The sequence of rebind_cases.SEQUENCE, one call a step: only what changed is bound again, so steps 1
    and 4 run cc_set_params' verkey branch alone and step 4 leaves the valid state it built."""
    ctx = _new_ctx(mode)
    try:
        bound, bits = (None, None, None), 8
        for label, (gw, vw) in RC.SEQUENCE:
            st = RC.state(mode, gw, vw)
            if label in RC.SAME_STATE_STEPS:  # the same key at another width
                assert st == bound
                ctx.set_table_bits(12, 0)
                _set_verkey(ctx, how, mode, st[1], st[2])
                bits = 12
            else:
                assert (st[0] != bound[0]) != (st[1:] != bound[1:]) or bound[0] is None, label
                if st[0] != bound[0]:
                    _set_params(ctx, how, st[0])
                if st[1:] != bound[1:]:
                    _set_verkey(ctx, how, mode, st[1], st[2])
            bound = st
            assert ctx.table_bits()[0] == bits, label
            observe(ctx, mode, st, label, prove=gw == vw)
    finally:
        ctx.close()


def _degenerate_params():
    return [pytest.param(m, name, id="%s-%s" % (m, name)) for m in MODES for name, _, _ in RC.degenerate_forms(m)]


@pytest.mark.parametrize("mode,form", _degenerate_params())
def test_degenerate_g_tilde_under_a_bound_verkey(mode, form):
    """cc_set_params(form) with vkA bound: an encoding that decodes to the identity makes pair 1 contribute
    factor 1 on every path (the pr = O row is then ACCEPTED), coordinates >= p are the honest point, a
    small-order point goes through the pairing as it is; the RLC on its own accepts only under a g~ in the
    subgroup; cc_set_params(gA) afterwards restores step 0's results."""
    enc, kind = {name: (enc, kind) for name, enc, kind in RC.degenerate_forms(mode)}[form]
    honest = RC.state(mode, "A", "A")
    st = (enc,) + honest[1:]
    small = dict(verify_n=(8, 4104), pervk_n=(8,), pok_n=(8,))
    ctx = _new_ctx(mode)
    try:
        _bind(ctx, "methods", mode, honest)
        ctx.set_params(enc)
        assert RC.observed(mode, st)["engine"] is (kind == "alias")
        observe(ctx, mode, st, form, prove=kind == "alias", **small)
        # the proofs made under g~ = O: their Schnorr check holds under an identity g~, so the pairing runs
        observe(ctx, mode, st, form + " / proofs under O", proofs="pok_id", plain=False, prove=kind == "identity",
                **small)
        ctx.set_params(honest[0])
        observe(ctx, mode, honest, form + " / back to gA", prove=True, **small)
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", MODES)
def test_rebind_waits_for_the_slots_in_flight(mode):
    """cc_set_concurrency(2): a batch queued under (gA, vkA) on one stream, the context rebound to (gB, vkB)
    with no synchronisation, a batch queued under it on another stream.  cc_set_params / cc_set_verkey wait for
    the slots' batches, so each batch carries the expectation of the state it was queued under: plain verify at
    n = 4104, PoK verify at n = 1032."""
    import torch
    lib = _lib()
    dev = torch.device("cuda", 0)
    to = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)  # noqa: E731
    P = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    ob = RC.sizes(mode)[1]
    states = {w: RC.state(mode, w, w) for w in "AB"}
    plain = {w: RC.tile_batch(RC.batch(mode, w), 4104) for w in "AB"}
    pok = {w: RC.tile_batch(RC.batch(mode, w), 1032) for w in "AB"}
    keys = ("s1", "s2", "msgs", "ps1", "ps2", "J", "T", "resp", "chal", "rev")
    D = {(kind, w): {k: to(t[w][k]) for k in keys} for kind, t in (("plain", plain), ("pok", pok)) for w in "AB"}
    idx = {w: (ctypes.c_uint64 * len(plain[w]["revealed"]))(*plain[w]["revealed"]) for w in "AB"}
    ctx = _new_ctx(mode)
    try:
        ctx.set_concurrency(2)
        streams = {w: torch.cuda.Stream(dev) for w in "AB"}
        for kind in ("plain", "pok"):
            outs = {}
            torch.cuda.synchronize()
            for w in "AB":
                g, X, Y = states[w]
                assert lib.cc_set_params(ctx.h, g) == 0
                assert lib.cc_set_verkey(ctx.h, X, Y, len(Y) // ob) == 0
                t, d = (plain if kind == "plain" else pok)[w], D[(kind, w)]
                v = torch.zeros(t["n"], dtype=torch.uint8, device=dev)
                gt = torch.zeros(t["n"] * 576, dtype=torch.uint8, device=dev)
                sp = ctypes.c_void_p(streams[w].cuda_stream)
                streams[w].wait_stream(torch.cuda.current_stream(dev))  # the zeroed outputs; no host wait
                if kind == "plain":
                    assert lib.cc_verify_batch_device(ctx.h, t["n"], t["q"], P(d["s1"]), P(d["s2"]), P(d["msgs"]), P(v),
                                                      P(gt), sp) == 0
                else:
                    assert lib.cc_pok_verify_batch_device(ctx.h, t["n"], t["q"], len(t["revealed"]), t["nresp"],
                                                          P(d["ps1"]), P(d["ps2"]), P(d["J"]), P(d["T"]), P(d["resp"]),
                                                          P(d["chal"]), idx[w], P(d["rev"]), P(v), P(gt), sp) == 0
                outs[w] = (v, gt)
            torch.cuda.synchronize()
            for w in "AB":
                e = RC.observed(mode, states[w])["verify" if kind == "plain" else "pok"]
                v, gt = outs[w]
                _same((kind, w), v.cpu().numpy(), bytes(gt.cpu().numpy()), *RC.tile_expect(e, len(v)))
        ctx.set_concurrency(1)
        assert ctx.concurrency() == 1
        ctx._gtilde, ctx._vk = states["B"][0], states["B"][1:]
        observe(ctx, mode, states["B"], "after the slots", verify_n=(8,), pervk_n=(8,), pok_n=(8,), prove=True)
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", MODES)
def test_refused_rebinds_leave_the_bound_state(mode):
    """cc_set_params(NULL) and cc_set_verkey with q > 4096 are refused before anything is touched: step 0's
    results still hold."""
    lib = _lib()
    st = RC.state(mode, "A", "A")
    ctx = _new_ctx(mode)
    try:
        _bind(ctx, "abi", mode, st)
        assert lib.cc_set_params(ctx.h, None) == ERR_DECODE
        assert lib.cc_set_verkey(ctx.h, st[1], st[2], 4097) == ERR_DECODE
        assert ctx.table_bits()[0] == 8
        observe(ctx, mode, st, "after the refused calls", verify_n=(8, 4104), pervk_n=(8,), pok_n=(8,), prove=True)
    finally:
        ctx.close()
