"""GPU tests of the RLC batch mode's g~-side fold (csrc/fold.hip) and of the finish's own side (rlc.hip
k_rlc_gather, fold.hip k_fold_fixed, miller_wide.hip's window pairs) against an independent model: the
window words of cc_rlc_partial_device and cc_rlc_partial_seg_device, the accept byte and the GT bytes of
cc_rlc_finish_device are compared, exactly, with tests/rlc_fold_cases.py (the Python key stream, curve and
pairing; checked on the CPU by tests/test_rlc_fold_model.py).  Every engine has a fixed seed and base index,
and nothing here goes through verify_batch(rlc=True), whose per-credential fallback would hide a wrong fold
behind right verdicts."""
import ctypes

import numpy as np
import pytest

import rlc_fold_cases as F

pytestmark = pytest.mark.gpu

MODES = {"G2": 0, "G1": 1}
CASES = sorted(F.cases("G2"))
assert CASES == sorted(F.cases("G1"))


@pytest.fixture(scope="module")
def ctxs():
    import coconut
    c = {}
    for m, v in MODES.items():
        d = F.fixture(m)
        c[m] = coconut.Context(0, coconut.GroupMode(v))
        c[m].set_params(bytes.fromhex(d["g_tilde"]))
        c[m].set_verkey(bytes.fromhex(d["vk"]["X"]), [bytes.fromhex(y) for y in d["vk"]["Y"]])
    yield c
    for x in c.values():
        x.close()


def _dev(x):
    import torch
    return torch.frombuffer(bytearray(x), dtype=torch.uint8).to(torch.device("cuda", 0))


def _words(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def rlc_engine_accepts(ctx, n, q, s1, s2, msgs, base_index=0, seed=F.SEED):
    """The RLC check itself on host bytes, with a fixed seed and no fallback behind it: partial -> finish.
    Other GPU tests use it next to their verify_batch(rlc=True) assertions."""
    from coconut.dist import DeviceEngine
    e = DeviceEngine(ctx, n, q, _dev(s1), _dev(s2), _dev(msgs), base_index=base_index, seed=seed)
    return e.finish(e.partial().reshape(1, -1), 1)


_INPUTS = {}


def _inputs(ctxs, mode, case):
    """Device (sigma_1, sigma_2, msgs) of a case: the Python oracle's multiples up to 64 credentials; above
    that the product's own fixed-base multiplication of the base credential's points, eight of them checked
    against the Python oracle."""
    key = (mode, case.name)
    if key not in _INPUTS:
        if case.n <= 64:
            host = F.inputs(mode, case.ks)
        else:
            import coconut
            c = F.valid_creds(mode)[0]
            sc = b"".join(k.to_bytes(48, "big") for k in case.ks)
            group = 2 if mode == "G2" else 1
            s1 = coconut.fixed_base_mul(ctxs[mode], group, bytes.fromhex(c["sigma1"]), sc)
            s2 = coconut.fixed_base_mul(ctxs[mode], group, bytes.fromhex(c["sigma2"]), sc)
            sb = len(s1) // case.n
            for i in (0, 1, 15, 16, 17, 1024, case.n - 2, case.n - 1):
                want = F.cred_bytes(mode, case.ks[i])
                assert (s1[i * sb:(i + 1) * sb], s2[i * sb:(i + 1) * sb]) == want, i
            host = (s1, s2, F.base_msgs(mode) * case.n)
        _INPUTS[key] = tuple(_dev(x) for x in host)
    return _INPUTS[key]


def _engine(ctxs, mode, case):
    from coconut.dist import DeviceEngine
    return DeviceEngine(ctxs[mode], case.n, F.Q, *_inputs(ctxs, mode, case), base_index=case.base_index, seed=F.SEED)


def _explain(mode, case, lo, hi, w, got):
    """What a failing window held, for the report: the digits and units (lanes in SigG1, lane pairs in SigG2)
    of a short slice, the bucket counts of a long one."""
    dig = [d[w] for d in case.dig(lo, hi)]
    if hi - lo <= 8:
        where = [(d, F.unit_of(mode, d), (abs(d) - 1) % F.CK[mode]) if d else (0, None, None) for d in dig]
        body = f"(digit, unit, bucket in unit) = {where}, multipliers k_i = {[hex(k)[:12] for k in case.ks[lo:hi]]}"
    else:
        cnt = {}
        for d in dig:
            if d:
                cnt[abs(d)] = cnt.get(abs(d), 0) + 1
        body = f"{len(cnt)} buckets populated, counts {sorted(set(cnt.values()))}"
    return (f"window {w} of {case.name} [{lo}, {hi}) at base index {case.base_index + lo}: device identity flag "
            f"{int(got[48])}, {body}")


def _check_partial(mode, case, part, lo=0, hi=None):
    """One partial against the model of credentials [lo, hi) at base_index + lo."""
    hi = case.n if hi is None else hi
    part = np.asarray(part)
    assert part.size == F.PART_WORDS
    assert part[F.FLAG] == 0, (case, lo)
    got = part[F.WIN_OFF:].reshape(F.FW, F.WIN_WORDS)
    want = case.expected(mode, lo, hi).reshape(F.FW, F.WIN_WORDS)
    bad = [w for w in range(F.FW) if not np.array_equal(got[w], want[w])]
    assert not bad, "; ".join(_explain(mode, case, lo, hi, w, got[w]) for w in bad)
    for w in range(F.FW):
        F.window_point(mode, got[w])   # every stored coordinate < p, flag 0 / 1, zeros where zeros belong


def _finish(ctx, parts, k):
    """cc_rlc_finish_device(k, parts) -> (accept, GT bytes)."""
    import torch
    lib = __import__("coconut")._lib.lib
    parts = parts.contiguous()
    acc = torch.full((1,), 7, dtype=torch.uint8, device=parts.device)
    gt = torch.zeros(576, dtype=torch.uint8, device=parts.device)
    torch.cuda.synchronize()
    assert lib.cc_rlc_finish_device(ctx.h, k, ctypes.c_void_p(parts.data_ptr()), ctypes.c_void_p(acc.data_ptr()),
                                    ctypes.c_void_p(gt.data_ptr()), None) == 0
    torch.cuda.synchronize()
    return int(acc.item()), gt.cpu().numpy().tobytes()


# ---------------------------------------------------------------- the fold
@pytest.mark.parametrize("mode", ["G2", "G1"])
@pytest.mark.parametrize("name", CASES)
def test_partial_windows_equal_the_model(ctxs, mode, name):
    """cc_rlc_partial_device: words [145, 929) are the model's 16 windows, the flag word is clear, every
    coordinate is canonical, and the finish accepts this very partial."""
    case = F.cases(mode)[name]
    e = _engine(ctxs, mode, case)
    part = e.partial().clone()
    _check_partial(mode, case, _words(part))
    assert e.finish(part.reshape(1, -1), 1) is True


@pytest.mark.parametrize("mode", ["G2", "G1"])
@pytest.mark.parametrize("name", CASES)
def test_segmented_partials_equal_the_model(ctxs, mode, name):
    """cc_rlc_partial_seg_device (the k_fold_*_seg kernels) on the same inputs: as one segment (seg >= n), and
    cut into at least two, segment s against the model of its slice at base_index + s seg; the finish over
    all of a batch's segment partials accepts."""
    case = F.cases(mode)[name]
    seg = 4
    while seg < case.n:
        seg *= 2
    e = _engine(ctxs, mode, case)
    parts = e.partial_seg(seg).clone()
    assert tuple(parts.shape) == (1, F.PART_WORDS)
    _check_partial(mode, case, _words(parts)[0])
    assert e.finish(parts, 1) is True
    sp = case.split()
    if sp is None:
        return
    cut, seg = sp
    e = _engine(ctxs, mode, cut)
    parts = e.partial_seg(seg).clone()
    S = -(-cut.n // seg)
    assert S >= 2 and tuple(parts.shape) == (S, F.PART_WORDS)
    got = _words(parts)
    for s in range(S):
        _check_partial(mode, cut, got[s], s * seg, min(cut.n, (s + 1) * seg))
    assert e.finish(parts, S) is True


# ---------------------------------------------------------------- rejecting batches
@pytest.mark.parametrize("mode", ["G2", "G1"])
@pytest.mark.parametrize("name", sorted(F.REJECTS))
def test_rejecting_batches_give_the_models_windows_and_gt(ctxs, mode, name):
    """Valid fixture credentials with one / two bad ones: the windows are the model's, the finish rejects
    and its GT bytes are prod_{bad i} gt_i^(delta_i mod r) -- through the whole partial and through the
    batch's two segment partials gathered."""
    from coconut.dist import DeviceEngine
    cr, bad = F.reject_creds(mode, name)
    n = len(cr)
    e = DeviceEngine(ctxs[mode], n, F.Q, *map(_dev, F.reject_inputs(mode, name)), base_index=F.REJECT_BASE, seed=F.SEED)
    part = e.partial().clone()
    w = _words(part)
    assert w[F.FLAG] == 0
    diff = np.flatnonzero(w[F.WIN_OFF:] != F.reject_windows(mode, name))
    assert diff.size == 0, sorted({int(x) // F.WIN_WORDS for x in diff})
    assert e.finish(part.reshape(1, -1), 1) is False
    assert _finish(ctxs[mode], part, 1) == (0, F.reject_gt(mode, name))
    parts = e.partial_seg(4).clone()
    assert parts.shape[0] == 2
    assert _finish(ctxs[mode], parts, 2) == (0, F.reject_gt(mode, name))


# ---------------------------------------------------------------- the finish over hand-built partials
@pytest.mark.parametrize("mode", ["G2", "G1"])
@pytest.mark.parametrize("names", F.HAND_PAIRS, ids="+".join)
def test_finish_over_hand_built_partials(ctxs, mode, names):
    """Two gathered partials whose Miller product is one and whose windows are chosen multiples of one point:
    GT = e(sum_w 256^w S_w, g~) of the Python oracle (k_rlc_gather's operands and skip flags, the fixed
    points 256^w g~, the wide Miller loop's window pairs), accept only where that sum is the identity."""
    import torch
    parts = torch.from_numpy(F.hand_partials(mode, names).view(np.int32)).to(torch.device("cuda", 0))
    want_gt, want_acc = F.hand_gt(mode, names)
    assert _finish(ctxs[mode], parts, 2) == (want_acc, want_gt)
    if names[1] == "neutral":   # and the first alone
        assert _finish(ctxs[mode], parts[:1], 1) == (want_acc, want_gt)
