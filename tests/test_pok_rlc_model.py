"""CPU model of the PoK RLC batch check (csrc/pok_rlc.hip): the delta key stream restated in Python
(fr.h rlc_delta_signed: one ChaCha20 block per proof, its first 16 bytes read as signed base-256
digits) and the equation the kernels implement, evaluated with the oracle's pure-Python pairing on the
q = 6 fixture:

    prod_i e(sigma'_1,i, delta_i J'_i) * e(-delta_i sigma'_2,i, g~),  J' = X~ + J + sum_revealed m_i Y~_i

after the final exponentiation equals gt_bad^(delta mod r) for a batch whose only failing proof is
Schnorr-valid with a wrong revealed message (gt_bad: that proof's own GT from the fixture)."""
import struct

from conftest import golden
from oracle import bls12_381 as B
from oracle import coconut_ref as C


def _rotl(x, n):
    return ((x << n) | (x >> (32 - n))) & 0xFFFFFFFF


def _qr(x, a, b, c, d):
    x[a] = (x[a] + x[b]) & 0xFFFFFFFF; x[d] = _rotl(x[d] ^ x[a], 16)  # noqa: E702
    x[c] = (x[c] + x[d]) & 0xFFFFFFFF; x[b] = _rotl(x[b] ^ x[c], 12)  # noqa: E702
    x[a] = (x[a] + x[b]) & 0xFFFFFFFF; x[d] = _rotl(x[d] ^ x[a], 8)   # noqa: E702
    x[c] = (x[c] + x[d]) & 0xFFFFFFFF; x[b] = _rotl(x[b] ^ x[c], 7)   # noqa: E702


def chacha20_block(key_words, counter, n0, n1, n2):
    """RFC 8439 block function over 32-bit words (fr.h chacha20_block): 16 output words."""
    s = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574, *key_words, counter, n0, n1, n2]
    x = list(s)
    for _ in range(10):
        _qr(x, 0, 4, 8, 12); _qr(x, 1, 5, 9, 13); _qr(x, 2, 6, 10, 14); _qr(x, 3, 7, 11, 15)  # noqa: E702
        _qr(x, 0, 5, 10, 15); _qr(x, 1, 6, 11, 12); _qr(x, 2, 7, 8, 13); _qr(x, 3, 4, 9, 14)  # noqa: E702
    return [(a + b) & 0xFFFFFFFF for a, b in zip(x, s)]


def rlc_delta_signed(seed32: bytes, g: int):
    """(delta, digits) of global proof index g under the 32-byte seed: the block with counter = low 32
    bits of g and nonce (high 32 bits of g, 0, 0); its first 16 bytes are the int8 digits d_w,
    delta = sum_w d_w 256^w (fr.h rlc_delta_signed; the device works with delta mod r)."""
    key = struct.unpack("<8I", seed32)
    blk = chacha20_block(key, g & 0xFFFFFFFF, (g >> 32) & 0xFFFFFFFF, 0, 0)
    dig = list(struct.unpack("<16b", struct.pack("<4I", *blk[:4])))
    return sum(d << (8 * w) for w, d in enumerate(dig)), dig


def test_chacha20_block_known_answer():
    """RFC 8439 section 2.3.2: key 00..1f, nonce 00:00:00:09:00:00:00:4a:00:00:00:00, block counter 1."""
    key = struct.unpack("<8I", bytes(range(32)))
    out = chacha20_block(key, 1, 0x09000000, 0x4A000000, 0)
    assert out == [0xE4E7F110, 0x15593BD1, 0x1FDD0F50, 0xC47120A3, 0xC7F4D1C7, 0x0368C033, 0x9AAA2204, 0x4E6CD4C3,
                   0x466482D2, 0x09AA9F07, 0x05D7C214, 0xA2028BD9, 0xD19C12B5, 0xB94E16DE, 0xE883D0CB, 0x4E3C50A2]


def test_delta_digits_are_the_key_stream_bytes():
    seed = bytes(range(100, 132))
    for g in (0, 7, (1 << 32) + 3):
        delta, dig = rlc_delta_signed(seed, g)
        assert len(dig) == 16 and all(-128 <= d <= 127 for d in dig)
        assert abs(delta) < 1 << 136
        assert delta == sum(d * 256 ** w for w, d in enumerate(dig))
    assert rlc_delta_signed(seed, 3)[0] != rlc_delta_signed(seed, (1 << 32) + 3)[0]  # the nonce word counts


SEED = bytes((37 * k + 11) & 0xFF for k in range(32))
BASE_INDEX = 5


def sub_batch(d):
    """[valid, valid, bad_revealed, valid] of a PoK fixture: every Schnorr relation holds."""
    pr = d["proofs"]
    valid = [p for p in pr if p["kind"] == "valid"]
    bad = next(p for p in pr if p["kind"] == "bad_revealed")
    return [valid[0], valid[1], bad, valid[2]]


def expected_gt(d, seed=SEED, base_index=BASE_INDEX):
    """GT bytes the finish must produce for sub_batch(d): gt_bad^(delta mod r), delta of global index
    base_index + 2."""
    bad = sub_batch(d)[2]
    delta, _ = rlc_delta_signed(seed, base_index + 2)
    return B.gt_to_bytes(B.f12_pow(B.gt_from_bytes(bytes.fromhex(bad["gt"])), delta % B.R))


def test_weighted_product_equals_the_bad_proofs_gt_power():
    d = golden("pok_g2_q6.json")
    grp = C.Groups(d["mode"])
    X = grp.oth_from_bytes(bytes.fromhex(d["vk"]["X"]))
    Y = [grp.oth_from_bytes(bytes.fromhex(y)) for y in d["vk"]["Y"]]
    gt_ = grp.oth_from_bytes(bytes.fromhex(d["g_tilde"]))
    f = B.f12_one()
    for i, p in enumerate(sub_batch(d)):
        delta = rlc_delta_signed(SEED, BASE_INDEX + i)[0] % B.R
        s1 = grp.sig_from_bytes(bytes.fromhex(p["sigma1"]))
        s2 = grp.sig_from_bytes(bytes.fromhex(p["sigma2"]))
        j = grp.other.add(X, grp.oth_from_bytes(bytes.fromhex(p["J"])))
        for idx, m in zip(d["revealed"], p["revealed_msgs"]):
            j = grp.other.add(j, grp.other.mul(Y[idx], B.fr_from_bytes(bytes.fromhex(m))))
        # SigG2: sigma' in G2 (the Miller loop's Q), J' and g~ in G1 (its P)
        f = B.f12_mul(f, B.miller_loop(s1, grp.other.mul(j, delta)))
        f = B.f12_mul(f, B.miller_loop(grp.sig.neg(grp.sig.mul(s2, delta)), gt_))
    assert B.gt_to_bytes(B.final_exp(f)) == expected_gt(d)
    assert not B.f12_is_one(B.final_exp(f))
