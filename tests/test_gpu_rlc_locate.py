"""GPU tests of the RLC locate mode: cc_rlc_partial_seg_device (one RLC partial per segment of the batch, in
one pass), cc_rlc_finish_each_device (one accept byte per partial) and the cc_verify_batch_locate drivers,
which verify per credential only the segments whose own RLC check failed.  Reference semantics are per
credential (Signature::verify, src/signature.rs:473-478): the verdicts must always equal
verify_batch(rlc=False).  The inputs are tests/rlc_locate_cases.py's, checked against the C oracle on the CPU
by tests/test_rlc_locate_model.py."""
import ctypes

import numpy as np
import pytest

import rlc_locate_cases as L
from conftest import golden
from test_gpu_parity import MODES, _cat

pytestmark = pytest.mark.gpu

DECODE, LEN, STATE = -4, -1, -7  # CC_ERR_DECODE, CC_ERR_LEN, CC_ERR_STATE (coconut_hip.h)
FLAG = 144


@pytest.fixture(scope="module")
def ctxs():
    import coconut
    c = {m: coconut.Context(0, coconut.GroupMode(v)) for m, v in MODES.items()}
    yield c
    for x in c.values():
        x.close()


def _bind(ctx, mode):
    b = L.batch(mode)
    ctx.set_params(b["g_tilde"])
    ctx.set_verkey(b["X"], b["Y"])


def _dev(x):
    import torch
    return torch.frombuffer(bytearray(x) if len(x) else bytearray(1), dtype=torch.uint8)[:len(x)].to(torch.device("cuda", 0))


def _engine(ctx, n, s1, s2, ms, q=L.Q, base_index=0, lo=0, hi=None):
    """A DeviceEngine over credentials [lo, hi) of the device arrays (fixed seed)."""
    from coconut.dist import DeviceEngine
    hi = n if hi is None else hi
    sb = ctx.mode.sig_bytes
    return DeviceEngine(ctx, hi - lo, q, s1[lo * sb:hi * sb], s2[lo * sb:hi * sb], ms[lo * q * 48:hi * q * 48],
                        base_index=base_index, seed=L.SEED)


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _finish_one(ctx, part):
    """cc_rlc_finish_device(1, part) -> (accept, GT bytes)."""
    import torch
    lib = __import__("coconut")._lib.lib
    part = part.contiguous()
    acc = torch.zeros(1, dtype=torch.uint8, device=part.device)
    gt = torch.zeros(576, dtype=torch.uint8, device=part.device)
    torch.cuda.synchronize()
    assert lib.cc_rlc_finish_device(ctx.h, 1, ctypes.c_void_p(part.data_ptr()), ctypes.c_void_p(acc.data_ptr()),
                                    ctypes.c_void_p(gt.data_ptr()), None) == 0
    torch.cuda.synchronize()
    return int(acc.item()), gt.cpu().numpy().tobytes()


def _per_credential(ctx, n, s1, s2, ms, q=L.Q):
    from coconut import verify_batch
    return verify_batch(ctx, n, q, s1, s2, ms)


# ---------------------------------------------------------------- partials against the existing path
@pytest.mark.parametrize("mode", ["G2", "G1"])
@pytest.mark.parametrize("n,seg", L.SHAPES + L.WIDE_SHAPES)
def test_segment_partials_equal_the_slices_partials(ctxs, mode, n, seg):
    """Partial s of cc_rlc_partial_seg_device equals, word for word, cc_rlc_partial_device on the slice
    [s seg, min(n, (s + 1) seg)) with base_index + s seg: the same Miller values through the same tree level,
    and affine window sums.  Base index 0 and a non-zero one wider than 32 bits."""
    import torch
    m = MODES[mode]
    ctx = ctxs[mode]
    _bind(ctx, m)
    s1, s2, ms = map(_dev, L.head(m, n))
    S = -(-n // seg)
    for base in (0, L.BASE_INDEX):
        parts = _engine(ctx, n, s1, s2, ms, base_index=base).partial_seg(seg)
        torch.cuda.synchronize()
        assert tuple(parts.shape) == (S, 929)
        got = _words(parts)
        for s in range(S):
            lo, hi = s * seg, min(n, (s + 1) * seg)
            want = _words(_engine(ctx, n, s1, s2, ms, base_index=base + lo, lo=lo, hi=hi).partial().clone())
            diff = np.flatnonzero(got[s] != want)
            assert diff.size == 0, (base, s, diff[:8])
            assert got[s][FLAG] == 0


def test_segmented_partial_of_an_empty_batch_writes_nothing(ctxs):
    import torch
    ctx = ctxs["G2"]
    _bind(ctx, 0)
    z = _dev(b"")
    e = _engine(ctx, 0, z, z, z)
    assert tuple(e.partial_seg(16).shape) == (0, 929)
    lib = __import__("coconut")._lib.lib
    canary = torch.full((929,), 0x5A5A5A5A, dtype=torch.int32, device=z.device)
    torch.cuda.synchronize()
    assert lib.cc_rlc_partial_seg_device(ctx.h, 0, L.Q, 16, 0, L.SEED, None, None, None,
                                         ctypes.c_void_p(canary.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert (canary == 0x5A5A5A5A).all()
    v, st = e.locate(16)
    assert v.size == 0 and st == (0, 0, 0)


# ---------------------------------------------------------------- the per-partial finish
@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_finish_each_equals_one_finish_per_partial(ctxs, mode):
    """Accept and GT bytes of every partial — the ten segment partials of a batch with one bad credential,
    a neutral partial (an empty shard's) and an unsegmented partial of the whole batch — equal
    cc_rlc_finish_device(1, that partial); and one finish over all segment partials decides as the finish
    of the unsegmented partial does, on the valid batch and on the corrupted one."""
    import torch
    m = MODES[mode]
    ctx = ctxs[mode]
    _bind(ctx, m)
    for bad in ((), (70,)):
        s1h, s2h, msh, _ = L.swap_sigma2(m, L.N, bad)
        s1, s2, ms = _dev(s1h), _dev(s2h), _dev(msh)
        e = _engine(ctx, L.N, s1, s2, ms)
        seg_parts = e.partial_seg(L.SEG).clone()
        whole = e.partial().clone()
        z = s1[:0]
        neutral = _engine(ctx, 0, z, z, z).partial().clone()
        stack = torch.cat([seg_parts, neutral.reshape(1, -1), whole.reshape(1, -1)]).contiguous()
        k = stack.shape[0]
        acc, gts = e.finish_each(stack, k, want_gt=True)
        want_acc = [0 if (s < 10 and bad and s == bad[0] // L.SEG) else 1 for s in range(k)]
        want_acc[-1] = 0 if bad else 1
        assert list(acc) == want_acc
        for r in range(k):
            a, gt = _finish_one(ctx, stack[r])
            assert (a, gt) == (int(acc[r]), gts[576 * r:576 * (r + 1)]), (bad, r)
        S = seg_parts.shape[0]
        assert e.finish(seg_parts, S) == e.finish(whole.reshape(1, -1), 1) == (not bad)


# ---------------------------------------------------------------- locating bad credentials
@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_one_bad_credential_rejects_its_segment_only(ctxs, mode):
    """A swapped sigma_2 at the first and at the last credential of a segment, at each of the four quad
    positions and in the 6-credential tail segment: exactly that segment's accept byte clears, the stats are
    (S, 1, the segment's length), and the verdicts equal construction and verify_batch(rlc=False)."""
    m = MODES[mode]
    ctx = ctxs[mode]
    _bind(ctx, m)
    S = -(-L.N // L.SEG)
    for i, seg_no, length in L.LOCATE_ONE:
        s1h, s2h, msh, expect = L.swap_sigma2(m, L.N, (i,))
        e = _engine(ctx, L.N, _dev(s1h), _dev(s2h), _dev(msh))
        acc = e.finish_each(e.partial_seg(L.SEG), S)
        assert list(acc) == [0 if s == seg_no else 1 for s in range(S)], i
        v, st = e.locate(L.SEG)
        assert st == (S, 1, length), i
        assert np.array_equal(v, expect), i
        assert np.array_equal(_per_credential(ctx, L.N, s1h, s2h, msh), expect), i


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_two_bad_credentials_adjacent_and_far_apart(ctxs, mode):
    """Two rejected segments side by side are rechecked as one merged run, two far apart as two runs
    compacted side by side; either way 32 credentials are rechecked and the verdicts are exact."""
    m = MODES[mode]
    ctx = ctxs[mode]
    _bind(ctx, m)
    for bad, segs, _runs in L.LOCATE_TWO:
        s1h, s2h, msh, expect = L.swap_sigma2(m, L.N, bad)
        e = _engine(ctx, L.N, _dev(s1h), _dev(s2h), _dev(msh))
        v, st = e.locate(L.SEG)
        assert st == (10, len(segs), 32), bad
        assert np.array_equal(v, expect), bad
        assert np.array_equal(_per_credential(ctx, L.N, s1h, s2h, msh), expect), bad


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_every_segment_bad_is_verified_in_place(ctxs, mode):
    """Every credential bad (each sigma_2 replaced by its successor's): every segment is rejected, the batch
    is verified where it lies, every verdict is 0."""
    m = MODES[mode]
    ctx = ctxs[mode]
    _bind(ctx, m)
    n = 40
    s1h, s2h, msh, expect = L.swap_sigma2(m, n, range(n))
    assert not expect.any()
    v, st = _engine(ctx, n, _dev(s1h), _dev(s2h), _dev(msh)).locate(8)
    assert st == (5, 5, n) and not v.any()
    assert not _per_credential(ctx, n, s1h, s2h, msh).any()


# ---------------------------------------------------------------- per-segment fall-back flags
@pytest.mark.parametrize("mode", ["G2", "G1"])
@pytest.mark.parametrize("kind", L.FLAG_KINDS)
def test_identity_or_non_subgroup_sigma_flags_its_segment_only(ctxs, mode, kind):
    """An identity sigma_1 / sigma_2 and a curve point outside the subgroup as sigma_1 / sigma_2 at
    credential 21 of 64 (segment 1 of 4): only partial 1 carries the fall-back flag and only segment 1 is
    rejected.  SigG2's sigma_1 test comes from the Miller loop's own T: one word for the whole launch would
    flag all four segments here."""
    m = MODES[mode]
    ctx = ctxs[mode]
    _bind(ctx, m)
    s1h, s2h, msh, expect = L.flag_case(m, kind)
    e = _engine(ctx, L.FLAG_N, _dev(s1h), _dev(s2h), _dev(msh))
    parts = e.partial_seg(L.FLAG_SEG)
    assert list(_words(parts)[:, FLAG]) == [0, 1, 0, 0]
    assert list(e.finish_each(parts, 4)) == [1, 0, 1, 1]
    v, st = e.locate(L.FLAG_SEG)
    assert st == (4, 1, L.FLAG_SEG)
    per = _per_credential(ctx, L.FLAG_N, s1h, s2h, msh)
    assert np.array_equal(per, expect) and np.array_equal(v, per)


def test_a_g_tilde_outside_the_subgroup_flags_every_segment(ctxs):
    """g~' = g~ + T (T of order dividing the G1 cofactor) under the same verkey, as in
    test_rlc_subgroup_status_follows_a_rebound_g_tilde: the linear-combination argument does not hold, so
    every segment carries the flag and the whole batch is verified per credential — every honest credential
    still verifies there (SigG2's g~ is the cofactor-blind P side).  Rebinding g~ clears the flags."""
    from oracle import bls12_381 as B
    from oracle.subgroup import random_curve_point
    d = golden("verify_g2_q6.json")
    good = [c for c in d["creds"] if c["verdict"] == 1]
    n, q = len(good), 6
    args = (_cat(c["sigma1"] for c in good), _cat(c["sigma2"] for c in good), _cat(m for c in good for m in c["msgs"]))
    g = B.g1_from_bytes(bytes.fromhex(d["g_tilde"]))
    h1 = 0x396C8C005555E1568C00AAAB0000AAAB  # G1 cofactor (x - 1)^2 / 3
    T = B.G1.mul_any(random_curve_point(B.G1, 0x5EED), B.R * pow(B.R, -1, h1))
    assert T is not None and B.G1.mul_any(T, h1) is None
    g_bad, g_ok = B.g1_to_bytes(B.G1.add(g, T)), bytes.fromhex(d["g_tilde"])
    vk = (bytes.fromhex(d["vk"]["X"]), [bytes.fromhex(y) for y in d["vk"]["Y"]])
    ctx = ctxs["G2"]
    S = -(-n // 4)
    dv = [_dev(a) for a in args]
    try:
        for g_bytes, flagged in ((g_ok, False), (g_bad, True), (g_ok, False)):
            ctx.set_params(g_bytes)
            ctx.set_verkey(*vk)
            e = _engine(ctx, n, *dv, q=q)
            flags = list(_words(e.partial_seg(4))[:, FLAG])
            assert flags == [int(flagged)] * S
            v, st = e.locate(4)
            assert st == ((S, S, n) if flagged else (S, 0, 0))
            assert v.all() and _per_credential(ctx, n, *args, q=q).all()
    finally:
        ctx.set_params(g_ok)
        ctx.set_verkey(*vk)


# ---------------------------------------------------------------- the segmented fold's edges
@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_segmented_fold_edge_batches(ctxs, mode):
    """64 copies of one credential at seg 16 (in every segment each bucket sums a repeated point: the
    doubling branch of the additions); the same with one copy's sigma_2 corrupted; and a tail segment of one
    credential (127 of each window's 128 buckets empty), valid and corrupted."""
    from coconut import verify_batch_locate
    d = golden(f"verify_{mode.lower()}_q6.json")
    ctx = ctxs[mode]
    ctx.set_params(bytes.fromhex(d["g_tilde"]))
    ctx.set_verkey(bytes.fromhex(d["vk"]["X"]), [bytes.fromhex(y) for y in d["vk"]["Y"]])
    good = next(c for c in d["creds"] if c["verdict"] == 1)
    other = next(c for c in d["creds"] if c["verdict"] == 1 and c["sigma2"] != good["sigma2"])
    k = 64
    s1, s2, ms = _cat([good["sigma1"]] * k), _cat([good["sigma2"]] * k), _cat(list(good["msgs"]) * k)
    v, st = verify_batch_locate(ctx, k, 6, s1, s2, ms, seg=16)
    assert v.all() and st == (4, 0, 0)
    sb = len(bytes.fromhex(good["sigma2"]))
    bad = bytearray(s2)
    bad[37 * sb:38 * sb] = bytes.fromhex(other["sigma2"])
    v, st = verify_batch_locate(ctx, k, 6, s1, bytes(bad), ms, seg=16)
    assert st == (4, 1, 16) and v[37] == 0 and v.sum() == k - 1
    # 17 credentials at seg 16: the tail segment holds one
    n = 17
    v, st = verify_batch_locate(ctx, n, 6, s1[:n * sb], s2[:n * sb], ms[:n * 6 * 48], seg=16)
    assert v.all() and st == (2, 0, 0)
    bad = bytearray(s2[:n * sb])
    bad[16 * sb:17 * sb] = bytes.fromhex(other["sigma2"])
    v, st = verify_batch_locate(ctx, n, 6, s1[:n * sb], bytes(bad), ms[:n * 6 * 48], seg=16)
    assert st == (2, 1, 1) and list(v) == [1] * 16 + [0]


# ---------------------------------------------------------------- the other call paths
@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_host_form_default_segment_device_set_and_sharded(ctxs, mode):
    """The host form (a fresh seed per call), seg = 0 (the library default: one segment at this size), a
    device-set context over {GPU 0}, and verify_sharded(rlc="locate")."""
    import coconut
    from coconut import verify_batch_locate
    from coconut.dist import verify_sharded
    m = MODES[mode]
    ctx = ctxs[mode]
    _bind(ctx, m)
    good = L.head(m, L.N)
    s1h, s2h, msh, expect = L.swap_sigma2(m, L.N, (47, 48))
    v, st = verify_batch_locate(ctx, L.N, L.Q, *good, seg=L.SEG)
    assert v.all() and st == (10, 0, 0)
    v, st = verify_batch_locate(ctx, L.N, L.Q, s1h, s2h, msh, seg=L.SEG)
    assert np.array_equal(v, expect) and st == (10, 2, 32)
    v, st = verify_batch_locate(ctx, L.N, L.Q, *good)
    assert v.all() and st == (1, 0, 0)
    v, st = verify_batch_locate(ctx, L.N, L.Q, s1h, s2h, msh)
    assert np.array_equal(v, expect) and st == (1, 1, L.N)
    e = _engine(ctx, L.N, _dev(s1h), _dev(s2h), _dev(msh))
    assert np.array_equal(verify_sharded(e, rlc="locate"), expect)
    assert np.array_equal(verify_sharded(e, rlc=True), expect) and np.array_equal(verify_sharded(e, rlc=False), expect)
    b = L.batch(m)
    multi = coconut.Context(mode=coconut.GroupMode(m), devices=[0])
    try:
        multi.set_params(b["g_tilde"])
        multi.set_verkey(b["X"], b["Y"])
        v, st = verify_batch_locate(multi, L.N, L.Q, s1h, s2h, msh, seg=L.SEG)
        assert np.array_equal(v, expect) and st == (10, 2, 32)
        v, st = verify_batch_locate(multi, L.N, L.Q, *good, seg=L.SEG)
        assert v.all() and st == (10, 0, 0)
    finally:
        multi.close()


def test_argument_errors(ctxs):
    """A segment length that is no power of two or below 4, more segments than CC_MAX_PARTS, a wrong q, a
    context without a verkey and null pointers are refused by all three device entry points and the host
    form before anything is launched (the buffers here are far smaller than the counts claim)."""
    import coconut
    import torch
    lib = coconut._lib.lib
    for code, word in ((DECODE, "bad buffer"), (LEN, "NoOfMessages"), (STATE, "not set")):
        assert word in lib.cc_status_str(code).decode()
    ctx = ctxs["G2"]
    _bind(ctx, 0)
    t = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    p = ctypes.c_void_p(t.data_ptr())
    host = bytes(4096)
    stats = (ctypes.c_uint32 * 3)()
    N = None

    def calls(h, n, q, seg, ptr=p, hptr=host):
        return (lib.cc_rlc_partial_seg_device(h, n, q, seg, 0, L.SEED, ptr, ptr, ptr, ptr, N),
                lib.cc_verify_batch_locate_device(h, n, q, seg, L.SEED, ptr, ptr, ptr, ptr, stats, N),
                lib.cc_verify_batch_locate(h, n, q, seg, hptr, hptr, hptr, hptr, stats))

    for seg in (3, 6, 2, 1, (1 << 26) * 2):
        assert calls(ctx.h, 8, L.Q, seg) == (DECODE,) * 3, seg
    assert lib.cc_rlc_partial_seg_device(ctx.h, 8, L.Q, 0, 0, L.SEED, p, p, p, p, N) == DECODE  # no default here
    assert calls(ctx.h, 4 * (1 << 16) + 1, L.Q, 4) == (DECODE,) * 3       # S = CC_MAX_PARTS + 1
    assert calls(ctx.h, (1 << 26) + 1, L.Q, 1 << 20) == (DECODE,) * 3     # n > CC_MAX_BATCH
    assert calls(ctx.h, 8, L.Q + 1, 16) == (LEN,) * 3
    assert calls(ctx.h, 8, L.Q, 16, ptr=N, hptr=N) == (DECODE,) * 3
    assert lib.cc_rlc_partial_seg_device(ctx.h, 8, L.Q, 16, 0, N, p, p, p, p, N) == DECODE
    assert lib.cc_verify_batch_locate_device(ctx.h, 8, L.Q, 16, N, p, p, p, p, stats, N) == DECODE
    assert calls(N, 8, L.Q, 16) == (DECODE,) * 3
    for args in ((0, p, p), (1 << 17, p, p), (4, N, p), (4, p, N)):
        assert lib.cc_rlc_finish_each_device(ctx.h, args[0], args[1], args[2], N, N) == DECODE, args[0]
    bare = coconut.Context(0, coconut.GroupMode(0))
    try:
        assert calls(bare.h, 8, L.Q, 16) == (STATE,) * 3
        assert lib.cc_rlc_finish_each_device(bare.h, 4, p, p, N, N) == STATE
        bare.set_params(L.batch(0)["g_tilde"])
        assert calls(bare.h, 8, L.Q, 16) == (STATE,) * 3
    finally:
        bare.close()
    torch.cuda.synchronize()
    assert not t.any()


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_existing_rlc_paths_after_the_new_calls(ctxs, mode):
    """The new calls share the RLC workspaces and the finish's buffers: after them verify_batch(rlc=True),
    cc_rlc_partial_device and cc_rlc_finish_device on the same context give their usual results."""
    from coconut import verify_batch
    m = MODES[mode]
    ctx = ctxs[mode]
    _bind(ctx, m)
    s1h, s2h, msh, expect = L.swap_sigma2(m, L.N, (66,))
    bad = _engine(ctx, L.N, _dev(s1h), _dev(s2h), _dev(msh))
    ok = _engine(ctx, L.N, *map(_dev, L.head(m, L.N)))
    before = _words(ok.partial().clone())
    assert np.array_equal(bad.locate(L.SEG)[0], expect)
    assert list(ok.finish_each(ok.partial_seg(4), -(-L.N // 4))) == [1] * 38
    assert np.array_equal(verify_batch(ctx, L.N, L.Q, s1h, s2h, msh, rlc=True), expect)
    assert verify_batch(ctx, L.N, L.Q, *L.head(m, L.N), rlc=True).all()
    p = ok.partial().clone()
    assert np.array_equal(_words(p), before)
    assert ok.finish(p.reshape(1, -1), 1) is True
    assert bad.finish(bad.partial().clone().reshape(1, -1), 1) is False
