"""CPU checks of tests/rlc_fold_cases.py: every case reaches the branch of the fold (csrc/fold.hip) it is
named after -- through the mirror of the fold's structure, on the committed base indices -- the window-sum
model agrees with a second implementation (the C oracle's oc_msm), and the GT the finish must give for the
rejecting batches equals the Python oracle's full weighted product.  No product code runs here;
tests/test_gpu_rlc_fold_direct.py compares the device with the same model."""
import ctypes

import pytest

import rlc_fold_cases as F
from oracle import bls12_381 as B
from oracle import coconut_ref as C

R = F.R
MODES = F.MODES


def _events(win, stage):
    return [(wh, kd) for s, wh, kd in win["events"] if s == stage]


def _two(mode, name):
    c = F.cases(mode)[name]
    da, db = (d[c.wstar] for d in c.dig())
    return c, da, db, F.mirror(mode, c.ks, c.dig())[c.wstar]


# ---------------------------------------------------------------- the encoding
def test_storage_form_and_window_words_round_trip():
    assert F._fp_words(1) == list(F.ONE_WORDS)   # 2^406 mod p, as an empty shard's partial shows it
    for mode in MODES:
        pt = F.X(mode)
        ws = F.partial_words(mode, pt)
        assert len(ws) == 49 and ws[48] == 0 and F.window_point(mode, ws) == pt
        if mode == "G1":
            assert not any(ws[24:48])
        assert F.partial_words(mode, None) == [0] * 48 + [1] and F.window_point(mode, [0] * 48 + [1]) is None
        bad = list(ws)
        bad[:12] = [(F.P >> (32 * k)) & 0xFFFFFFFF for k in range(12)]   # p itself: not canonical
        with pytest.raises(AssertionError):
            F.window_point(mode, bad)
    p = F.hand_partial("G2", [None] * 16)
    assert p.size == 929 and list(p[:12]) == list(F.ONE_WORDS) and not p[12:145].any()


def test_digits_are_the_key_streams_and_the_nonce_word_counts():
    d = F.digits(F.SEED, 5, 3)
    assert len(d) == 3 and all(len(r) == 16 and all(-128 <= x <= 127 for x in r) for r in d)
    assert F.digits(F.SEED, 6, 1)[0] == d[1]
    assert F.deltas(F.SEED, 5, 1)[0] == sum(x << (8 * w) for w, x in enumerate(d[0]))
    assert F.digits(F.SEED, F.HIGH + 5, 1)[0] != d[0]


# ---------------------------------------------------------------- the reach of every case
@pytest.mark.parametrize("mode", MODES)
def test_single_launches_reach_identity_window_top_bucket_and_the_uv_doubling(mode):
    rows = {b: F.digits(F.SEED, b, 1)[0] for b in F.SINGLE_BASES}
    seen = {x for r in rows.values() for x in r}
    big = 2 * F.CK[mode]                      # |d| = 4 (SigG1) / 8 (SigG2): u = v in unit 1
    assert {0, -128, 127, 1, -1} <= seen and (big in seen or -big in seen)
    ident = top = dbl = False
    for b, r in rows.items():
        c = F.cases(mode)[f"single_{b}"]
        assert c.n == 1 and c.base_index == b
        for w, win in enumerate(F.mirror(mode, c.ks, c.dig())):
            if r[w] == 0:
                ident |= win["S"] == 0 and not any(win["counts"])
            if r[w] == -128:   # bucket 128 holds the sign - only: the top digit of the last unit
                top |= win["counts"][127] == 1 and win["buckets"][127] == R - 1
                assert win["shares"][F.UNITS[mode] - 1] == (-128) % R
            if abs(r[w]) == big:
                dbl |= (1, "dbl") in _events(win, "uv")
            elif r[w]:
                assert "dbl" not in [kd for _, kd in _events(win, "uv")]
            if r[w] and (abs(r[w]) - 1) % F.CK[mode]:   # a populated bucket over an empty one: u + run doubles
                assert ((F.unit_of(mode, r[w]), (abs(r[w]) - 1) % F.CK[mode] - 1), "dbl") in _events(win, "u")
    assert ident and top and dbl


@pytest.mark.parametrize("mode", MODES)
def test_same_bucket_cases_double_and_cancel_in_the_mixed_addition(mode):
    for tag, kind in (("eq", "dbl"), ("op", "inf")):
        c, da, db, win = _two(mode, f"same_bucket_{tag}")
        assert da == db != 0 and c.ks == (1, 1 if tag == "eq" else R - 1)
        b = abs(da) - 1
        assert win["counts"][b] == 2 and sum(win["counts"]) == 2
        assert _events(win, "sum") == [((b, 0, 1), kind)]   # acc = the point / minus the point
        assert win["buckets"][b] == (2 * F.sgn(da) % R if tag == "eq" else 0)
        assert (win["S"] == 0) == (tag == "op")             # op: the identity window with a non-empty bucket


@pytest.mark.parametrize("mode", MODES)
def test_same_lane_cases_meet_equal_and_opposite_operands_inside_one_unit(mode):
    ck = F.CK[mode]
    for tag in ("eq", "op"):
        c, da, db, win = _two(mode, f"same_lane_{tag}")
        t = F.unit_of(mode, da)
        assert t == F.unit_of(mode, db) and abs(da) != abs(db)
        assert sorted(b for b, n in enumerate(win["counts"]) if n) == sorted((abs(da) - 1, abs(db) - 1))
        assert da % R == (1 if tag == "eq" else -1) * db * c.ks[1] % R   # d_b X_b = +-d_a X_a
        assert [s for s in win["shares"] if s] == ([2 * da % R] if tag == "eq" else [])
        if tag == "op":   # u = -v: the unit's final addition goes to the identity
            assert (t, "inf") in _events(win, "uv") and win["S"] == 0
        # B_hi = +-B_lo: the running sum adds equal / opposite buckets, and u then adds to what it holds
        c, da, db, win = _two(mode, f"same_lane_run_{tag}")
        k_lo = (min(abs(da), abs(db)) - 1) % ck
        assert ((t, k_lo), "dbl" if tag == "eq" else "inf") in _events(win, "run")
        hi, lo = (abs(da) - 1, abs(db) - 1) if abs(da) > abs(db) else (abs(db) - 1, abs(da) - 1)
        assert win["buckets"][hi] == (win["buckets"][lo] if tag == "eq" else R - win["buckets"][lo]) != 0
        assert win["S"] == (win["buckets"][hi] * (hi + 1) + win["buckets"][lo] * (lo + 1)) % R != 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["partner_hi", "partner_lo", "high_index"])
def test_partner_cases_meet_in_the_butterfly_at_the_named_step(mode, name):
    ul = F.UNIT_LANES[mode]
    for tag, kind in (("eq", "dbl"), ("op", "inf")):
        c, da, db, win = _two(mode, f"{name}_{tag}")
        ta, tb = F.unit_of(mode, da), F.unit_of(mode, db)
        assert ta != tb
        m = F.meeting_step(ta, tb) * ul   # in lanes, as the kernels count it
        assert m == 32 if name != "partner_lo" else m <= 2
        assert win["shares"][ta] == da % R != 0
        assert win["shares"][tb] == (da % R if tag == "eq" else -da % R)
        ev = _events(win, "bfly")
        assert ev and all(wh[0] == m and kd == kind for wh, kd in ev if wh[0] >= m)
        assert sum(1 for wh, _ in ev if wh[0] == m) >= 1
        assert win["S"] == (2 * da % R if tag == "eq" else 0)
        if name == "high_index":   # the key stream's nonce word: other digits than at the index's low 32 bits
            assert c.base_index >> 40 == 1
            assert F.digits(F.SEED, c.base_index - F.HIGH, 2) != c.dig()


@pytest.mark.parametrize("mode", MODES)
def test_neighbouring_base_indices_lack_the_patterns(mode):
    """The committed indices matter: for each searched pattern a base index within 8 of the committed one
    does not have it, and the committed one does (so a replaced index fails the tests above or here)."""
    finds = {"same_bucket": F.find_same_bucket, "same_lane": F.find_same_lane,
             "partner_hi": lambda m, a, b: F.find_partner(m, a, b, True),
             "high_index": lambda m, a, b: F.find_partner(m, a, b, True)}
    for key, find in finds.items():
        base = F.BASES[mode][key]
        assert base >= 4 and find(mode, *F.digits(F.SEED, base, 2)) is not None
        near = [j for j in range(base - 8, base + 9) if j >= 4 and find(mode, *F.digits(F.SEED, j, 2)) is None]
        assert near, key
    a, b = F.digits(F.SEED, F.BASES[mode]["partner_lo"], 2)
    assert F.find_partner(mode, a, b, False) is not None
    for nb in F.SINGLE_BASES:   # the neighbours of the single launches miss a digit the set needs
        need = [{0}, {-128}, {127}, {1}, {-1}, {4, -4}, {8, -8}]
        have = {x for b2 in F.SINGLE_BASES if b2 != nb for x in F.digits(F.SEED, b2, 1)[0]}
        have |= set(F.digits(F.SEED, nb + 1, 1)[0])
        assert not all(s & have for s in need)


@pytest.mark.parametrize("mode", MODES)
def test_copies_every_bucket_is_a_small_multiple_of_one_point(mode):
    c = F.cases(mode)["copies"]
    assert c.n == 64 and c.ks == (1, R - 1) * 32
    zero = two = 0
    for win in F.mirror(mode, c.ks, c.dig()):
        for n, v in zip(win["counts"], win["buckets"]):
            mult = v if v <= R // 2 else v - R
            assert abs(mult) <= n and (mult - n) % 2 == 0
            zero += n > 0 and mult == 0
            two += abs(mult) >= 2
        kinds = {kd for _, kd in _events(win, "sum")}
        assert {"dbl", "inf"} <= kinds
    assert zero >= 16 and two >= 16


@pytest.mark.parametrize("mode", MODES)
def test_chunks_hits_the_chunk_boundaries(mode):
    c = F.cases(mode)["chunks"]
    assert c.n == F.CHUNKS_N and len(set(c.ks)) == c.n and 0 not in c.ks
    mir = F.mirror(mode, c.ks, c.dig())
    counts = {n for win in mir for n in win["counts"]}
    assert set(F.CHUNK_COUNTS) <= counts
    assert F.FS * 2 < max(counts) <= F.FS * 4
    # the buckets' chunk partials: one, two and three chunks are reduced
    nchunks = {-(-n // F.FS) for n in counts if n}
    assert {1, 2, 3} <= nchunks
    assert any(kd == "add" for win in mir for _, kd in _events(win, "reduce"))
    # one index fewer loses the count the search stopped at
    fewer = {n for win in F.mirror(mode, c.ks[:-1], c.dig(0, c.n - 1)) for n in win["counts"]}
    assert not set(F.CHUNK_COUNTS) <= fewer


def test_split_forms():
    for mode in MODES:
        for c in F.cases(mode).values():
            sp = c.split()
            if c.n == 1:
                assert sp is None
                continue
            s, seg = sp
            assert seg >= 4 and seg & (seg - 1) == 0 and -(-s.n // seg) >= 2
            if c.n == 2:   # segment 1 is the case itself, at its own base index
                assert s.base_index + seg == c.base_index and s.ks[seg:] == c.ks and s.dig(seg, s.n) == c.dig()


# ---------------------------------------------------------------- the model against other implementations
def _fold_points(mode, ks):
    dec = F._codec(mode)[0]
    cv = F.curve(mode)
    return [cv.neg(dec(F.cred_bytes(mode, k)[1])) for k in ks]


@pytest.mark.parametrize("mode", MODES)
def test_window_sums_recombine_to_the_c_oracles_msm(oc, mode):
    """sum_w 256^w S_w = sum_i (delta_i mod r) (-sigma_2,i) with the right side from oc_msm over the encoded
    fold points, for every case the Python oracle builds; the multiples-of-X shortcut equals the
    point-by-point window sums; and every re-randomised credential verifies (the first of each multiplier)."""
    cv, enc = F.curve(mode), F._codec(mode)[1]
    group = 2 if mode == "G2" else 1
    eb = 192 if mode == "G2" else 97
    grp = C.Groups(mode)
    d = F.fixture(mode)
    vk = (grp.oth_from_bytes(bytes.fromhex(d["vk"]["X"])), [grp.oth_from_bytes(bytes.fromhex(y)) for y in d["vk"]["Y"]])
    g_tilde = grp.oth_from_bytes(bytes.fromhex(d["g_tilde"]))
    msgs = [B.fr_from_bytes(bytes.fromhex(m)) for m in F.valid_creds(mode)[0]["msgs"]]
    checked = set()
    for c in F.small_cases(mode):
        pts = _fold_points(mode, c.ks)
        dig = c.dig()
        sums = F.window_sums(mode, pts, dig)
        assert sums == F.window_sums_of_multiples(mode, c.ks, dig), c
        total = None
        for w, S in enumerate(sums):
            total = cv.add(total, F.smul(cv, S, 1 << (8 * w)))
        dl = F.deltas(F.SEED, c.base_index, c.n)
        out = ctypes.create_string_buffer(eb)
        oc.oc_msm(group, ctypes.c_size_t(c.n), b"".join(enc(p) for p in pts),
                  b"".join(B.fr_to_bytes(x % R) for x in dl), out)
        assert out.raw == enc(total), c
        for k in c.ks:
            if k in checked or len(checked) >= 6:
                continue
            checked.add(k)
            dec = F._codec(mode)[0]
            sig = tuple(dec(x) for x in F.cred_bytes(mode, k))
            assert C.verify(grp, sig, msgs, vk, g_tilde), (c, k)


@pytest.mark.parametrize("mode", MODES)
def test_chunks_points_spot_check(mode):
    """Eight of the chunks case's multipliers through the Python oracle: distinct points, and the window
    scalar of the model is the sum of their digits' multiples."""
    c = F.cases(mode)["chunks"]
    idx = (0, 1, 15, 16, 17, 1024, c.n - 2, c.n - 1)
    pts = _fold_points(mode, [c.ks[i] for i in idx])
    assert len(set(pts)) == 8 and all(F.curve(mode).on_curve(p) for p in pts)
    dig = [c.dig()[i] for i in idx]
    assert F.window_sums(mode, pts, dig) == F.window_sums_of_multiples(mode, [c.ks[i] for i in idx], dig)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(F.REJECTS))
def test_reject_gt_is_the_bad_credentials_gt_power(mode, name):
    """prod_i e(sigma_1,i, delta_i pr_i) e(-delta_i sigma_2,i, g~), pr = X~ + sum m_j Y~_j, after the final
    exponentiation, equals prod_{bad i} gt_i^(delta_i mod r) with the fixture's per-credential GT bytes."""
    cr, bad = F.reject_creds(mode, name)
    assert len(cr) == 6 + len(bad) and bad == tuple(sorted(F.REJECTS[name]))
    grp = C.Groups(mode)
    d = F.fixture(mode)
    Xt = grp.oth_from_bytes(bytes.fromhex(d["vk"]["X"]))
    Y = [grp.oth_from_bytes(bytes.fromhex(y)) for y in d["vk"]["Y"]]
    g_tilde = grp.oth_from_bytes(bytes.fromhex(d["g_tilde"]))
    ml = (lambda s, o: B.miller_loop(s, o)) if mode == "G2" else (lambda s, o: B.miller_loop(o, s))
    f = B.f12_one()
    for c, delta in zip(cr, F.deltas(F.SEED, F.REJECT_BASE, len(cr))):
        s1 = grp.sig_from_bytes(bytes.fromhex(c["sigma1"]))
        s2 = grp.sig_from_bytes(bytes.fromhex(c["sigma2"]))
        pr = Xt
        for y, m in zip(Y, c["msgs"]):
            pr = grp.other.add(pr, grp.other.mul(y, B.fr_from_bytes(bytes.fromhex(m))))
        f = B.f12_mul(f, ml(s1, grp.other.mul(pr, delta % R)))
        f = B.f12_mul(f, ml(grp.sig.neg(grp.sig.mul(s2, delta % R)), g_tilde))
    gt = B.final_exp(f)
    assert B.gt_to_bytes(gt) == F.reject_gt(mode, name)
    assert not B.f12_is_one(gt)


@pytest.mark.parametrize("mode", MODES)
def test_hand_built_sets(mode):
    for names in F.HAND_PAIRS:
        gt, acc = F.hand_gt(mode, names)
        assert acc == int(names == ("cancels", "neutral"))
        assert (gt == B.gt_to_bytes(B.f12_one())) == bool(acc)
    assert all(F.HAND["all_finite"]) and F.HAND["only_15"][:15] == [0] * 15
    assert [bool(s) for s in F.HAND["interleaved"]] == [True, False] * 8
    assert len(set(F.HAND["same_point"])) == 1
    # the pairing is bilinear in the window weights: e(256 S, g~) = e(S, g~)^256 for the oracle's pairing
    S = F.multiple_of_X(mode, F.HAND["only_15"][15])
    g = bytes.fromhex(F.fixture(mode)["g_tilde"])
    one = B.pairing(B.g1_from_bytes(g), S) if mode == "G2" else B.pairing(S, B.g2_from_bytes(g))
    assert B.gt_to_bytes(B.f12_pow(one, pow(256, 15, R))) == F.hand_gt(mode, ("only_15", "neutral"))[0]
