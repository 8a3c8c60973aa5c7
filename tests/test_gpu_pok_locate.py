"""GPU tests of the PoK RLC locate mode: cc_pok_rlc_partial_seg_device (one PoK RLC partial per segment of the
batch, in one pass), cc_rlc_finish_each_device on those partials, and the cc_pok_verify_batch_locate drivers,
which verify per proof only the segments whose own RLC check failed.  Reference semantics are per proof (ps_sig
PoKOfSignatureProof::verify): the verdicts must always equal pok_verify_batch(rlc=False).  The inputs are
tests/pok_locate_cases.py's, checked on the CPU by tests/test_pok_locate_model.py."""
import ctypes

import numpy as np
import pytest

import pok_locate_cases as P
from conftest import golden
from test_gpu_parity import MODES

pytestmark = pytest.mark.gpu

DECODE, LEN, STATE, BASES = -4, -1, -7, -2  # CC_ERR_DECODE, _LEN, _STATE, _BASES_EXPS (coconut_hip.h)
FLAG = 144
MAX_BATCH = 1 << 26


@pytest.fixture(scope="module")
def ctxs():
    import coconut
    c = {m: coconut.Context(0, coconut.GroupMode(v)) for m, v in MODES.items()}
    yield c
    for x in c.values():
        x.close()


def _bind(ctx, b):
    ctx.set_params(b["g_tilde"])
    ctx.set_verkey(b["X"], b["Y"])


def _to_dev(b):
    import torch
    dev = torch.device("cuda", 0)
    # one spare byte so an empty array still has a device pointer
    return {k: torch.frombuffer(bytearray(b[k] + b"\0"), dtype=torch.uint8).to(dev) for k in P.KEYS}


def _engine(ctx, b, D, lo=0, hi=None, base_index=0, stream=None):
    """A PokDeviceEngine over proofs [lo, hi) of the device batch D (fixed seed)."""
    from coconut.dist import PokDeviceEngine
    hi = b["n"] if hi is None else hi
    w = P.widths(b["mode"], b["nresp"], len(b["revealed"]))
    s = {k: D[k][lo * w[k]:] for k in P.KEYS}
    return PokDeviceEngine(ctx, hi - lo, b["q"], b["revealed"], s["s1"], s["s2"], s["J"], s["T"], s["resp"], s["chal"],
                           s["rev"], base_index=base_index, seed=P.SEED, stream=stream)


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _per_proof(ctx, b):
    from coconut import pok_verify_batch
    return pok_verify_batch(ctx, b["n"], b["q"], b["revealed"], b["nresp"], *(b[k] for k in P.KEYS), rlc=False)


def _finish_one(ctx, part):
    """cc_rlc_finish_device(1, part) -> (accept, GT bytes)."""
    import torch
    from coconut._lib import lib
    part = part.contiguous()
    acc = torch.zeros(1, dtype=torch.uint8, device=part.device)
    gt = torch.zeros(576, dtype=torch.uint8, device=part.device)
    torch.cuda.synchronize()
    assert lib.cc_rlc_finish_device(ctx.h, 1, ctypes.c_void_p(part.data_ptr()), ctypes.c_void_p(acc.data_ptr()),
                                    ctypes.c_void_p(gt.data_ptr()), None) == 0
    torch.cuda.synchronize()
    return int(acc.item()), gt.cpu().numpy().tobytes()


# ---------------------------------------------------------------- 1. partials against the existing path
@pytest.mark.parametrize("mode", ["G2", "G1"])
@pytest.mark.parametrize("n,seg", P.SHAPES)
def test_segment_partials_equal_the_slices_partials(ctxs, mode, n, seg):
    """Partial s of cc_pok_rlc_partial_seg_device equals, word for word, cc_pok_rlc_partial_device on the slice
    [s seg, min(n, (s + 1) seg)) with base_index + s seg: the same Miller values (two proofs a loop) through the
    same tree level, and affine window sums.  Base index 0 and a non-zero one wider than 32 bits."""
    import torch
    ctx = ctxs[mode]
    b = P.batch(MODES[mode], n)
    _bind(ctx, b)
    D = _to_dev(b)
    S = -(-n // seg)
    for base in (0, P.BASE_INDEX):
        parts = _engine(ctx, b, D, base_index=base).partial_seg(seg)
        torch.cuda.synchronize()
        assert tuple(parts.shape) == (S, 929)
        got = _words(parts)
        for s in range(S):
            lo, hi = s * seg, min(n, (s + 1) * seg)
            want = _words(_engine(ctx, b, D, lo, hi, base_index=base + lo).partial().clone())
            diff = np.flatnonzero(got[s] != want)
            assert diff.size == 0, (base, s, diff[:8])
            assert got[s][FLAG] == 0


# ---------------------------------------------------------------- 2. each failure kind alone
@pytest.mark.parametrize("mode", ["G2", "G1"])
@pytest.mark.parametrize("kind", P.KINDS)
def test_each_failure_kind_flags_and_rejects_its_segment_only(ctxs, mode, kind):
    """One fixture bad proof at index 70 of (150, 16): only segment 4's accept byte is clear; its partial's flag
    word is 1 for a failed Schnorr relation (bad_chal, bad_response, bad_J) and an identity sigma'_1, 0 for
    bad_revealed (only the pairing product catches it); every other segment's flag word is 0, so a Schnorr
    failure no longer flags the batch.  finish_each's bytes equal cc_rlc_finish_device(1, partial)'s."""
    ctx = ctxs[mode]
    b = P.batch(MODES[mode], P.N, ((P.KIND_AT, kind),))
    _bind(ctx, b)
    e = _engine(ctx, b, _to_dev(b))
    parts = e.partial_seg(P.SEG).clone()
    S, at = -(-P.N // P.SEG), P.KIND_AT // P.SEG
    assert list(_words(parts)[:, FLAG]) == [int(s == at and kind in P.FLAGGED) for s in range(S)]
    acc, gts = e.finish_each(parts, S, want_gt=True)
    assert list(acc) == [int(s != at) for s in range(S)]
    for s in range(S):
        a, gt = _finish_one(ctx, parts[s])
        assert (a, gt) == (int(acc[s]), gts[576 * s:576 * (s + 1)]), s
    v, st = e.locate(P.SEG)
    assert st == (S, 1, P.SEG)
    assert np.array_equal(v, b["expect"]) and np.array_equal(_per_proof(ctx, b), b["expect"])


# ---------------------------------------------------------------- 3. positions
@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_one_bad_proof_at_the_edge_positions(ctxs, mode):
    """A bad_revealed proof (no flag: the segment's product alone rejects) at the first and last index of a
    segment, at both positions of a twin loop, at the tail segment's last index with n odd, and either side of
    the PoK prep's block edge: that segment alone is rechecked and the verdicts equal the per-proof path's."""
    ctx = ctxs[mode]
    for n, seg, i, seg_no, length in P.LOCATE_ONE:
        b = P.batch(MODES[mode], n, ((i, "bad_revealed"),))
        _bind(ctx, b)
        e = _engine(ctx, b, _to_dev(b))
        S = -(-n // seg)
        parts = e.partial_seg(seg)
        assert not _words(parts)[:, FLAG].any(), (n, i)
        assert list(e.finish_each(parts, S)) == [int(s != seg_no) for s in range(S)], (n, i)
        v, st = e.locate(seg)
        assert st == (S, 1, length), (n, i)
        per = _per_proof(ctx, b)
        assert np.array_equal(per, b["expect"]) and np.array_equal(v, per), (n, i)


# ---------------------------------------------------------------- 4. several bad proofs, the sentinel
def _locate_with_sentinel(ctx, b, seg):
    """locate() into a verdict buffer with 64 sentinel bytes behind the n verdicts."""
    import torch
    e = _engine(ctx, b, _to_dev(b))
    e.verdicts = torch.full((b["n"] + 64,), 0xA5, dtype=torch.uint8, device=e.dev)
    v, st = e.locate(seg)
    assert (v[b["n"]:] == 0xA5).all()
    return v[:b["n"]], st


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_adjacent_distant_and_every_segment_bad(ctxs, mode):
    """Two rejected segments side by side (one merged run), two far apart (two runs compacted side by side),
    and a bad proof in every segment (the batch verified in place): verdicts, stats, and the bytes of
    d_verdicts beyond n untouched."""
    ctx = ctxs[mode]
    for bad, segs, rechecked in P.LOCATE_TWO:
        b = P.batch(MODES[mode], P.N, tuple((i, "bad_revealed") for i in bad))
        _bind(ctx, b)
        v, st = _locate_with_sentinel(ctx, b, P.SEG)
        assert st == (10, len(segs), rechecked), bad
        per = _per_proof(ctx, b)
        assert np.array_equal(per, b["expect"]) and np.array_equal(v, per), bad
    # mixed kinds far apart: a flagged segment and an unflagged one in the same plan
    b = P.batch(MODES[mode], P.N, ((10, "bad_chal"), (100, "bad_revealed"), (149, "sigma1_inf")))
    v, st = _locate_with_sentinel(ctx, b, P.SEG)
    assert st == (10, 3, 16 + 16 + 6)
    assert np.array_equal(v, b["expect"]) and np.array_equal(_per_proof(ctx, b), b["expect"])
    b = P.batch(MODES[mode], P.EVERY_N, tuple((i, "bad_revealed") for i in P.EVERY_BAD))
    v, st = _locate_with_sentinel(ctx, b, P.EVERY_SEG)
    assert st == (5, 5, P.EVERY_N)
    assert np.array_equal(v, b["expect"]) and np.array_equal(_per_proof(ctx, b), b["expect"])
    b = P.batch(MODES[mode], P.N)
    v, st = _locate_with_sentinel(ctx, b, P.SEG)
    assert st == (10, 0, 0) and v.all()


# ---------------------------------------------------------------- 5. batch-wide causes
def _outside(group):
    return next(bytes.fromhex(r["point"]) for r in golden("subgroup.json")[group] if int(r["status"]) == 1)


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_a_verkey_component_outside_the_subgroup_flags_every_segment(ctxs, mode):
    """Y~_0 replaced by a curve point outside the order-r subgroup: the linear-combination argument does not
    hold, every segment carries the flag, the batch is verified in place and the verdicts equal the per-proof
    path's.  Rebinding the verkey clears the flags."""
    ctx = ctxs[mode]
    m = MODES[mode]
    b = P.batch(m, 40)
    D = _to_dev(b)
    bad_Y = [_outside("G1" if m == 0 else "G2")] + b["Y"][1:]
    assert len(bad_Y[0]) == len(b["Y"][0])
    try:
        for Y, flagged in ((b["Y"], False), (bad_Y, True), (b["Y"], False)):
            ctx.set_params(b["g_tilde"])
            ctx.set_verkey(b["X"], Y)
            e = _engine(ctx, b, D)
            assert list(_words(e.partial_seg(8))[:, FLAG]) == [int(flagged)] * 5
            v, st = e.locate(8)
            assert st == ((5, 5, 40) if flagged else (5, 0, 0))
            per = _per_proof(ctx, b)
            assert np.array_equal(v, per)
            assert flagged or per.all()
    finally:
        _bind(ctx, b)


def test_a_small_order_component_in_verkey_or_g_tilde_sigg2(ctxs):
    """SigG2, the point (0, 2) of order 3 added to a revealed message's Y~ or to g~.  Y~_3 + (0, 2): the pairing
    is cofactor-blind on its G1 side and Y~_3 is in no Schnorr relation, so every proof still verifies, but
    every segment is flagged and the batch is verified in place.  g~ + (0, 2): a proof's Schnorr sum moves by
    resp_0 (0, 2), so exactly the proofs whose first response is a multiple of 3 still verify; the verdicts are
    the per-proof path's either way."""
    from oracle import bls12_381 as B
    ctx = ctxs["G2"]
    b = P.batch(0, 40)
    D = _to_dev(b)
    t3 = (0, 2)
    assert B.G1.on_curve(t3) and B.G1.mul_any(t3, 3) is None
    shift = lambda enc: B.g1_to_bytes(B.G1.add(B.g1_from_bytes(enc), t3))  # noqa: E731
    i = b["revealed"][0]
    Y_bad = b["Y"][:i] + [shift(b["Y"][i])] + b["Y"][i + 1:]
    rw = b["nresp"] * 48
    resp0_mod3 = np.array([int.from_bytes(b["resp"][k * rw:k * rw + 48], "big") % 3 == 0 for k in range(40)], np.uint8)
    try:
        for g, Y, want in ((b["g_tilde"], Y_bad, np.ones(40, np.uint8)), (shift(b["g_tilde"]), b["Y"], resp0_mod3)):
            ctx.set_params(g)
            ctx.set_verkey(b["X"], Y)
            e = _engine(ctx, b, D)
            assert list(_words(e.partial_seg(8))[:, FLAG]) == [1] * 5
            v, st = e.locate(8)
            assert st == (5, 5, 40)
            per = _per_proof(ctx, b)
            assert np.array_equal(v, per)
            assert np.array_equal(per, want)
    finally:
        _bind(ctx, b)


# ---------------------------------------------------------------- 6. the four-proof route
def test_batch_past_the_two_proof_loop():
    """65,667 proofs at seg 16,384: past the twin limit the segmented partial takes the four-proof loop
    (cck_miller4_seg_lz_g2 / cck_miller4_lz_g1), five segments with a tail of 131.  All valid: every accept
    byte is 1.  Proof n - 2 with its neighbour's sigma'_2: only the last segment is rejected, and locate
    rechecks its 131 proofs.  (Accept bytes and verdicts, not partial words: the slices' own partials would
    take the two-proof loop and group the products differently.)  Both modes in this one test, the only large
    one."""
    import bench_modes
    import coconut
    n, seg = 65664 + 3, 16384
    for mode in (0, 1):
        ctx = coconut.Context(0, coconut.GroupMode(mode))
        try:
            b = bench_modes.make_pok_batch(ctx, mode, n, q=6, revealed=[1, 4], seed=61, bad_every=0)
            _bind(ctx, b)
            e = _engine(ctx, b, _to_dev(b))
            parts = e.partial_seg(seg)
            assert not _words(parts)[:, FLAG].any(), mode
            assert list(e.finish_each(parts, 5)) == [1] * 5, mode
            w = P.widths(mode, b["nresp"], len(b["revealed"]))["s2"]
            s2 = bytearray(b["s2"])
            s2[(n - 2) * w:(n - 1) * w] = b["s2"][(n - 1) * w:n * w]
            c = dict(b, s2=bytes(s2))
            e = _engine(ctx, c, _to_dev(c))
            assert list(e.finish_each(e.partial_seg(seg), 5)) == [1, 1, 1, 1, 0], mode
            v, st = e.locate(seg)
            assert st == (5, 1, 131), mode
            expect = np.ones(n, np.uint8)
            expect[n - 2] = 0
            assert np.array_equal(v, expect), mode
        finally:
            ctx.close()


# ---------------------------------------------------------------- 7. the host form
@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_host_form_with_the_default_segment(ctxs, mode):
    from coconut import pok_verify_batch_locate
    ctx = ctxs[mode]
    b = P.batch(MODES[mode], P.N, ((P.KIND_AT, "bad_revealed"),))
    _bind(ctx, b)
    args = (b["n"], b["q"], b["revealed"], b["nresp"], *(b[k] for k in P.KEYS))
    v, st = pok_verify_batch_locate(ctx, *args)          # seg = 0: one segment at this size
    assert st == (1, 1, P.N)
    assert np.array_equal(v, _per_proof(ctx, b)) and np.array_equal(v, b["expect"])
    v, st = pok_verify_batch_locate(ctx, *args, seg=P.SEG)
    assert st == (10, 1, P.SEG) and np.array_equal(v, b["expect"])
    good = P.batch(MODES[mode], P.N)
    v, st = pok_verify_batch_locate(ctx, good["n"], good["q"], good["revealed"], good["nresp"],
                                    *(good[k] for k in P.KEYS))
    assert st == (1, 0, 0) and v.all()


# ---------------------------------------------------------------- 8. argument errors
def test_argument_errors(ctxs):
    """The checks of cc_pok_rlc_partial_device in its order (NULL context / buffers, no verkey, q, a bad revealed
    index, nresp), then the segment length (no power of two, below 4, above CC_MAX_BATCH; 0 only for the partial
    call) and S > CC_MAX_PARTS, by all three entry points before anything is launched (the buffers here are far
    smaller than the counts claim); n = 0 writes nothing and returns zero stats."""
    import coconut
    import torch
    lib = coconut._lib.lib
    ctx = ctxs["G2"]
    b = P.batch(0, 8)
    _bind(ctx, b)
    t = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    p = ctypes.c_void_p(t.data_ptr())
    host = bytes(4096)
    stats = (ctypes.c_uint32 * 3)()
    N = None
    idx = (ctypes.c_uint64 * 2)(3, 5)

    def calls(h, n, q, r, nresp, seg, ptr=p, hptr=host, ix=idx, seed=P.SEED):
        a = (ptr,) * 6 + (ix, ptr)
        ha = (hptr,) * 6 + (ix, hptr)
        return (lib.cc_pok_rlc_partial_seg_device(h, n, q, r, nresp, seg, 0, seed, *a, ptr, N),
                lib.cc_pok_verify_batch_locate_device(h, n, q, r, nresp, seg, seed, *a, ptr, stats, N),
                lib.cc_pok_verify_batch_locate(h, n, q, r, nresp, seg, *ha, hptr, stats))

    assert calls(N, 8, 6, 2, 5, 16) == (DECODE,) * 3
    assert calls(ctx.h, 8, 6, 2, 5, 16, ptr=N, hptr=N) == (DECODE,) * 3
    assert calls(ctx.h, 8, 6, 2, 5, 16, ix=N) == (DECODE,) * 3
    assert calls(ctx.h, 8, 6, 2, 5, 16, seed=N)[:2] == (DECODE,) * 2
    bare = coconut.Context(0, coconut.GroupMode(0))
    try:
        assert calls(bare.h, 8, 6, 2, 5, 16) == (STATE,) * 3
        bare.set_params(b["g_tilde"])
        assert calls(bare.h, 8, 6, 2, 5, 3) == (STATE,) * 3     # the verkey before the segment length
    finally:
        bare.close()
    assert calls(ctx.h, 8, 7, 2, 6, 16) == (LEN,) * 3
    assert calls(ctx.h, 8, 7, 2, 6, 3) == (LEN,) * 3            # q before the segment length
    assert calls(ctx.h, 8, 6, 2, 5, 16, ix=(ctypes.c_uint64 * 2)(3, 6)) == (LEN,) * 3      # index >= q
    assert calls(ctx.h, 8, 6, 2, 5, 16, ix=(ctypes.c_uint64 * 2)(3, 3)) == (DECODE,) * 3   # repeated index
    assert calls(ctx.h, 8, 6, 2, 4, 16) == (BASES,) * 3
    assert calls(ctx.h, 8, 6, 2, 4, 3) == (BASES,) * 3          # nresp before the segment length
    for seg in (3, 6, 2, 1, 2 * MAX_BATCH):
        assert calls(ctx.h, 8, 6, 2, 5, seg) == (DECODE,) * 3, seg
    a = (p,) * 6 + (idx, p)
    assert lib.cc_pok_rlc_partial_seg_device(ctx.h, 8, 6, 2, 5, 0, 0, P.SEED, *a, p, N) == DECODE   # no default here
    assert calls(ctx.h, 4 * (1 << 16) + 1, 6, 2, 5, 4) == (DECODE,) * 3       # S = CC_MAX_PARTS + 1
    assert calls(ctx.h, MAX_BATCH + 1, 6, 2, 5, 1 << 20) == (DECODE,) * 3     # n > CC_MAX_BATCH
    torch.cuda.synchronize()
    assert not t.any()
    # n = 0: nothing written, zero stats
    canary = torch.full((929,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    c = ctypes.c_void_p(canary.data_ptr())
    stats[0] = stats[1] = stats[2] = 9
    na = (N,) * 6 + (idx, N)
    assert lib.cc_pok_rlc_partial_seg_device(ctx.h, 0, 6, 2, 5, 16, 0, P.SEED, *na, c, N) == 0
    assert lib.cc_pok_verify_batch_locate_device(ctx.h, 0, 6, 2, 5, 0, P.SEED, *na, c, stats, N) == 0
    assert list(stats) == [0, 0, 0]
    stats[0] = 9
    assert lib.cc_pok_verify_batch_locate(ctx.h, 0, 6, 2, 5, 0, *na, N, stats) == 0
    assert list(stats) == [0, 0, 0]
    assert lib.cc_pok_verify_batch_locate(ctx.h, 0, 6, 2, 4, 0, *na, N, stats) == BASES
    torch.cuda.synchronize()
    assert (canary == 0x5A5A5A5A).all()


# ---------------------------------------------------------------- 9. a caller stream, and the older paths after
@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_caller_stream_and_the_existing_paths_afterwards(ctxs, mode):
    """The device form on a non-default caller stream gives the same verdicts; afterwards the unsegmented PoK
    partial, its finish and pok_verify_batch(rlc=True) on the same context give their usual results (the new
    calls share their workspaces)."""
    import torch
    from coconut import pok_verify_batch
    ctx = ctxs[mode]
    b = P.batch(MODES[mode], P.N, ((66, "bad_revealed"), (5, "bad_response")))
    good = P.batch(MODES[mode], P.N)
    _bind(ctx, b)
    D = _to_dev(b)
    ok = _engine(ctx, good, _to_dev(good))
    before = _words(ok.partial().clone())
    v0, st0 = _engine(ctx, b, D).locate(P.SEG)
    v1, st1 = _engine(ctx, b, D, stream=torch.cuda.Stream(torch.device("cuda", 0))).locate(P.SEG)
    assert st0 == st1 == (10, 2, 32)
    assert np.array_equal(v0, b["expect"]) and np.array_equal(v1, b["expect"])
    args = lambda x: (x["n"], x["q"], x["revealed"], x["nresp"], *(x[k] for k in P.KEYS))  # noqa: E731
    assert np.array_equal(pok_verify_batch(ctx, *args(b), rlc=True), b["expect"])
    assert pok_verify_batch(ctx, *args(good), rlc=True).all()
    part = ok.partial().clone()
    assert np.array_equal(_words(part), before)
    assert ok.finish(part.reshape(1, -1), 1) is True
    bad = _engine(ctx, b, D)
    assert bad.finish(bad.partial().clone().reshape(1, -1), 1) is False
