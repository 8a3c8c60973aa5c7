"""Shared inputs and oracle expectations of the holder-side issuance tests (test_sigreq_prove_abi.py: the
model check on the CPU; test_gpu_sigreq_prove.py: the same inputs through cc_sigreq_new_batch /
cc_sigreq_pok_init_batch / cc_sigreq_pok_gen_proof_batch).

Everything expected here comes from oracle/issuance.py (signature_request_new / compute_h /
sigreq_pok_init / sigreq_gen_proof); the scalars the reference draws (r, k_i; the blindings) are fixed per
row and replayed into the oracle (pok_prove_cases.Replay), so the GPU is given the very same scalars as
`rand` and `blind`.  A world is one Params (g, h_0 .. h_{q-1}) with the points its encodings decode to;
a row is one request under it."""
import functools

from oracle import coconut_ref as C
from oracle import issuance as I
from pok_prove_cases import Replay, be48, fr, off_curve  # noqa: F401

R = C.R
SHAPES = ((3, 0), (3, 1), (4, 2), (3, 3), (6, 5))
ONES252 = (1 << 252) - 1          # every fixed-table window below bit 252 all ones (8-, 13- and 16-bit tables)
TOP252 = 1 << 252                 # a single digit in the top window of each width
N8 = int("8" * 63, 16)            # signed radix-16 recoding: every nibble 8 (the carry threshold)
N7 = int("7" * 63, 16)            # every nibble 7 (one below it)


class World:
    """Params for q messages: points (None = the identity) and the encodings handed to the library, which
    may differ from to_bytes of the point (an off-curve encoding decodes to the identity)."""

    def __init__(self, mode, q, seed, h=None, g=None, h_enc=None):
        self.mode, self.q = mode, q
        self.grp = grp = C.Groups(mode)
        rng = C.Drbg(f"sigreq-world-{mode}-{seed}")
        hp = [grp.sig.mul(grp.sig.gen, rng.fr()) for _ in range(q)]
        gp = grp.sig.mul(grp.sig.gen, rng.fr())
        if h is not None:
            hp = h(hp)
        self.h = hp
        self.g = gp if g is None else g(hp)
        self.g_enc = grp.sig_to_bytes(self.g)
        self.h_enc = [grp.sig_to_bytes(p) for p in hp]
        if h_enc is not None:  # {index: function of the point's encoding}; the point becomes the identity
            for j, f in h_enc.items():
                self.h_enc[j] = f(self.h_enc[j])
                self.h[j] = None
        self.g_tilde = grp.other.mul(grp.other.gen, rng.fr())

    def params(self):
        return {"g": self.g, "h": self.h}


def oracle_row(w, row):
    """The oracle's request, proof record and to_bytes for one row (dict: k, msgs, pk point, rand, blind,
    sk, chal as integers, possibly >= r: reduced here as the ABI reduces them)."""
    grp, k, q = w.grp, row["k"], w.q
    se = grp.sig_to_bytes
    msgs = [m % R for m in row["msgs"]]
    rand = [v % R for v in row["rand"]]
    blind = [v % R for v in row["blind"]]
    chal, sk = row["chal"] % R, row["sk"] % R
    req, randomness = I.signature_request_new(grp, msgs, k, row["pk"], w.params(), Replay(rand))
    assert randomness == rand
    h = I.compute_h(grp, req["commitment"], req["known"])  # for k = 0 as well: the issuer computes it
    pok = I.sigreq_pok_init(grp, req, row["pk"], w.params(), Replay(blind))
    proof = I.sigreq_gen_proof(pok, msgs[:k], randomness, sk, chal)
    T = dict(sk=se(pok["sk"]["T"]), comm=se(pok["comm"]["T"]), cts=[(se(a["T"]), se(b["T"])) for a, b in pok["cts"]])
    rec = T["sk"] + fr(proof["sk"]["responses"][0]) + T["comm"] + b"".join(fr(v) for v in proof["comm"]["responses"])
    rec0 = T["sk"] + bytes(48) + T["comm"] + bytes(48 * (k + 1))
    for (t1, t2), (p1, p2) in zip(T["cts"], proof["cts"]):
        rec += t1 + fr(p1["responses"][0]) + t2 + fr(p2["responses"][0]) + fr(p2["responses"][1])
        rec0 += t1 + bytes(48) + t2 + bytes(96)
    pk_enc = row["pk_enc"]
    g = w.g_enc
    tb = g + T["sk"] + b"".join(w.h_enc[:k]) + g + T["comm"]
    for t1, t2 in T["cts"]:
        tb += g + t1 + pk_enc + se(h) + t2
    return dict(req=req, h_pt=h, proof=proof, commitment=se(req["commitment"]), h=se(h),
                cts=b"".join(se(a) + se(b) for a, b in req["ciphertexts"]), init=rec0, record=rec, to_bytes=tb)


def _row(w, rng, k, name, msgs=None, rand=None, blind=None, pk=None, pk_enc=None, valid=True):
    sk = rng.fr()
    pkp = w.grp.sig.mul(w.g, sk) if pk is None else pk[0]
    return dict(name=name, k=k, msgs=[rng.fr() for _ in range(w.q)] if msgs is None else msgs,
                rand=[rng.fr() for _ in range(k + 1)] if rand is None else rand,
                blind=[rng.fr() for _ in range(3 * k + 2)] if blind is None else blind, sk=sk, chal=rng.fr(),
                pk=pkp, pk_enc=pk_enc if pk_enc is not None else w.grp.sig_to_bytes(pkp),
                # valid: pk = sk g, so the request proof verifies and the issuance flow gives a signature
                valid=valid and pk is None)


@functools.lru_cache(maxsize=None)
def shape_batches(mode):
    """One world and two random rows for each (q, k) of SHAPES."""
    out = []
    for q, k in SHAPES:
        w = World(mode, q, f"shape-{q}")
        rng = C.Drbg(f"sigreq-shape-{mode}-{q}-{k}")
        out.append((f"q{q}k{k}", w, k, [_row(w, rng, k, f"q{q}k{k}#{i}") for i in range(2)]))
    return out


def _blind(k, b_sk, hb, b_r, pairs):
    return [b_sk] + list(hb) + [b_r] + [v for p in pairs for v in p]


@functools.lru_cache(maxsize=None)
def edge_batches(mode):
    """[(name, world, k, [row ...])]: the edge scalars and the related bases of the issue, the rows that
    share a world and a k in one batch."""
    grp = C.Groups(mode)
    rng = C.Drbg("sigreq-edges-" + mode)
    f = rng.fr
    out = []
    w = World(mode, 3, "edges")
    k = 3
    a = [
        _row(w, rng, k, "m=0,1,r-1", msgs=[0, 1, R - 1]),
        # r = 0: the commitment has no g term; k_0 = 0: c1_0 is the identity; m_0 = 0 as well: c2_0 too;
        # a hidden message handed over as r + 7 is reduced
        _row(w, rng, k, "r=0,k0=0,m0=0,m2>=r", msgs=[0, f(), R + 7], rand=[0, 0, f(), f()]),
        _row(w, rng, k, "blindings=0", blind=[0] * (3 * k + 2)),
        _row(w, rng, k, "recoding edges", msgs=[N7, R - 1, 8], rand=[N8, 8, N8, R - 1],
             blind=_blind(k, 8, [N8, N7, R - 1], N7, [(N8, N7), (R - 1, 8), (N7, N8)])),
        _row(w, rng, k, "table digit edges", msgs=[TOP252, ONES252, 1 << 248], rand=[ONES252, TOP252, ONES252, 1],
             blind=_blind(k, ONES252, [TOP252, ONES252, 1], TOP252, [(ONES252, TOP252), (TOP252, ONES252), (1, 1)])),
    ]
    out.append(("edge scalars", w, k, a))
    # a known message >= r hashes as its reduced value (k = 0: no ciphertexts at all)
    out.append(("known m>=r", w, 0, [_row(w, rng, 0, "known m0=r+5", msgs=[R + 5, f(), f()])]))
    # elgamal_pk related to the request's own h, k_0 = m_0 (and b2_0 = hb_0): the two-base accumulator
    # doubles (pk = h), cancels (pk = -h) or meets 2h's table (pk = 2h); pk is then no key of sk, so the
    # request proof is not valid, only byte-exact
    k = 1
    rel = []
    for name, mk in (("pk=h", lambda h: h), ("pk=-h", lambda h: grp.sig.neg(h)), ("pk=2h", lambda h: grp.sig.add(h, h))):
        m0, r0, hb0 = f(), f(), f()
        msgs = [m0, f(), f()]
        comm = grp.sig.msm([w.h[0], w.g], [m0, r0])
        h = I.compute_h(grp, comm, msgs[1:])
        rel.append(_row(w, rng, k, name, msgs=msgs, rand=[r0, m0], blind=_blind(k, f(), [hb0], f(), [(f(), hb0)]),
                        pk=(mk(h),)))
    good = grp.sig.mul(w.g, f())
    rel.append(_row(w, rng, k, "pk=identity", pk=(None,)))
    rel.append(_row(w, rng, k, "pk off-curve", pk=(None,), pk_enc=off_curve(grp.sig_to_bytes(good))))
    out.append(("related pk", w, k, rel))
    k = 2
    mm = f()
    w1 = World(mode, 3, "h1=h0", h=lambda hp: [hp[0], hp[0], hp[2]])
    # one-window scalars: the second term is the very table entry the sum stands at (a doubling)
    out.append(("h1=h0", w1, k, [_row(w1, rng, k, "h1=h0, equal messages", msgs=[5, 5, f()],
                                      blind=_blind(k, f(), [7, 7], f(), [(f(), f()), (f(), f())]))]))
    w2 = World(mode, 3, "h1=-h0", h=lambda hp: [hp[0], grp.sig.neg(hp[0]), hp[2]])
    out.append(("h1=-h0", w2, k, [_row(w2, rng, k, "h1=-h0, equal messages", msgs=[mm, mm, f()],
                                       blind=_blind(k, f(), [mm, mm], f(), [(f(), f()), (f(), f())]))]))
    w3 = World(mode, 3, "g=h0", g=lambda hp: hp[0])
    out.append(("g=h0", w3, k, [_row(w3, rng, k, "g=h0")]))
    ident = grp.sig_to_bytes(None)
    w4 = World(mode, 3, "h-identity", h_enc={0: lambda e: ident, 1: off_curve})
    out.append(("h0 identity, h1 off-curve", w4, k, [_row(w4, rng, k, "h0 identity, h1 off-curve")]))
    return out


@functools.lru_cache(maxsize=None)
def expected(mode, which):
    """shape_batches / edge_batches with every row's oracle bytes added (key `want`)."""
    src = shape_batches(mode) if which == "shapes" else edge_batches(mode)
    return [(name, w, k, [dict(r, want=oracle_row(w, r)) for r in rows]) for name, w, k, rows in src]


def inputs(w, k, rows):
    """The flat byte strings of a batch: msgs, pk, rand, blind, sk, chal (scalars unreduced, as given)."""
    return dict(msgs=b"".join(be48(m) for r in rows for m in r["msgs"]), pk=b"".join(r["pk_enc"] for r in rows),
                rand=b"".join(be48(v) for r in rows for v in r["rand"]),
                blind=b"".join(be48(v) for r in rows for v in r["blind"]),
                sk=b"".join(be48(r["sk"]) for r in rows), chal=b"".join(be48(r["chal"]) for r in rows))
