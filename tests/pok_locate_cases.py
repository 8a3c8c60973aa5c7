"""Inputs shared by tests/test_gpu_pok_locate.py (GPU) and tests/test_pok_locate_model.py (CPU): the shapes, the
PoK batches and where the bad proofs go.  Batches come from the golden fixtures pok_g2_q6.json / pok_g1_q6.json
(3 valid proofs and 5 corruption kinds each, with the per-proof verdicts recorded when they were generated): the
three valid proofs tiled to n (identical proofs get different deltas, so a tiled batch is a sound RLC input) with
fixture bad proofs placed at chosen indices.  Inputs only: no GPU here."""
import functools

import numpy as np

import rlc_locate_cases as L
from conftest import golden

Q = 6
N, SEG = L.N, L.SEG                 # 150 proofs: 9 full segments of 16 and a tail of 6
SEED, BASE_INDEX = L.SEED, L.BASE_INDEX
# (n, seg) of the partial comparison: rlc_locate_cases' shapes, and one wide segment (the segmented fold sizes its
# lane groups by seg: one lane or lane pair a bucket up to 2,048, two from 4,096)
SHAPES = L.SHAPES + ((150, 4096),)
KEYS = ("s1", "s2", "J", "T", "resp", "chal", "rev")
KINDS = ("bad_chal", "bad_response", "bad_J", "sigma1_inf", "bad_revealed")
# what raises a fall-back flag (a failed Schnorr relation: bad_chal, bad_response, bad_J; an identity sigma'_1) and
# what only the pairing product catches: as tests/test_gpu_pok_rlc.py test_each_failure_kind_alone_is_rejected
# asserts for the unsegmented partial's one word
FLAGGED = ("bad_chal", "bad_response", "bad_J", "sigma1_inf")
UNFLAGGED = ("bad_revealed",)
KIND_AT = 70                        # the failure kinds one at a time: proof 70 of (150, 16), segment 4

# one bad_revealed proof at a time: (n, seg, index, segment it must clear, that segment's length)
LOCATE_ONE = (
    (150, 16, 32, 2, 16),    # the first proof of a segment
    (150, 16, 47, 2, 16),    # the last proof of a segment
    (150, 16, 64, 4, 16), (150, 16, 65, 4, 16),   # both positions of a twin loop (k_miller<SIG, true>)
    (149, 16, 148, 9, 5),    # n odd: the tail segment's last proof, whose loop skips its second pair
    (129, 64, 127, 1, 64),   # the last proof of the PoK prep's first block
    (129, 64, 128, 2, 1),    # the first proof of the second block, alone in the tail segment
)
# several at a time in the (150, 16) batch: (indices, rejected segments, proofs rechecked)
LOCATE_TWO = (
    ((47, 48), (2, 3), 32),      # adjacent segments: one merged run
    ((10, 100), (0, 6), 32),     # far apart: two runs compacted side by side
)
EVERY_N, EVERY_SEG, EVERY_BAD = 40, 8, (3, 11, 19, 27, 35)   # a bad proof in each of the 5 segments: in place


def mode_name(mode):
    return "G2" if mode == 0 else "G1"


def widths(mode, nresp, r):
    """Bytes per proof of the seven arrays."""
    sb, ob = (192, 97) if mode == 0 else (97, 192)
    return dict(s1=sb, s2=sb, J=ob, T=ob, resp=nresp * 48, chal=48, rev=r * 48)


@functools.lru_cache(maxsize=None)
def fixture(mode):
    d = golden(f"pok_{mode_name(mode).lower()}_q6.json")
    assert d["q"] == Q
    return d


def _row(p):
    h = bytes.fromhex
    return dict(s1=h(p["sigma1"]), s2=h(p["sigma2"]), J=h(p["J"]), T=h(p["T"]),
                resp=b"".join(h(x) for x in p["responses"]), chal=h(p["chal"]),
                rev=b"".join(h(x) for x in p["revealed_msgs"]))


def proofs_of(mode, n, bad=()):
    """The fixture proofs of an n-proof batch: valid proof i % 3 at index i, the fixture's bad proof of `kind`
    at every (index, kind) of `bad`."""
    d = fixture(mode)
    valid = [p for p in d["proofs"] if p["kind"] == "valid"]
    by_kind = {p["kind"]: p for p in d["proofs"] if p["kind"] != "valid"}
    out = [valid[i % len(valid)] for i in range(n)]
    for i, kind in bad:
        out[i] = by_kind[kind]
    return out


def batch(mode, n, bad=()):
    """The batch as one dict in bench_modes.make_pok_batch's layout, with the verkey, and `expect`: the
    fixture's recorded verdict of every placed proof."""
    d = fixture(mode)
    pr = proofs_of(mode, n, bad)
    rows = [_row(p) for p in pr]
    b = dict(mode=mode, n=n, q=Q, revealed=list(d["revealed"]), nresp=len(pr[0]["responses"]) if pr else Q - 1,
             g_tilde=bytes.fromhex(d["g_tilde"]), X=bytes.fromhex(d["vk"]["X"]),
             Y=[bytes.fromhex(y) for y in d["vk"]["Y"]],
             expect=np.array([p["verdict"] for p in pr], np.uint8))
    for k in KEYS:
        b[k] = b"".join(r[k] for r in rows)
    return b


def slice_of(b, lo, hi):
    """Proofs [lo, hi) of batch b."""
    w = widths(b["mode"], b["nresp"], len(b["revealed"]))
    return dict(b, n=hi - lo, expect=b["expect"][lo:hi], **{k: b[k][lo * w[k]:hi * w[k]] for k in KEYS})


def twin_values(n):
    """The proofs of every Miller value of the two-proof loop: value j holds proofs 2 j and 2 j + 1."""
    return [list(range(2 * j, min(n, 2 * j + 2))) for j in range((n + 1) // 2)]
