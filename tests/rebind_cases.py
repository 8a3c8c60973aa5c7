"""Inputs and oracle expectations for rebinding Params and Verkey on a live context, and for a g~ that does
not decode (test_rebind_model.py: conditions on these inputs, on the CPU; test_gpu_rebind.py: the same inputs
through cc_set_params / cc_set_verkey and every consumer of the context's g~-derived buffers).  TEST
INFRASTRUCTURE ONLY, importable without a GPU.

WORLDS.  Two per group mode from pok_prove_cases.World, with different seeds and so different g~ and keys:
A has q = 6 and reveals (3, 5), B has q = 3 and reveals (1,).  Each world has 8 distinct rows:

    rows 0..5  valid credentials over random messages;
    row 6      a valid credential's sigma_2 shown with another first message;
    row 7      messages solved for pr = X~ + sum m_j Y~_j = O (the world keeps its secret key) under an
               arbitrary pair sigma = (h, k h).  With an honest g~ it is one more bad credential; with a g~
               that decodes to the identity the check is e(sigma_1, pr) = 1 and the oracle ACCEPTS it, so a
               device that lets a degenerate g~ into the pairing gets a verdict wrong, not only GT bytes.

Every row carries its PoKOfSignature proof from the Python oracle (pok_prove_cases.oracle_proof, fixed draws
and challenge; init's J and T use g~ as a base).  World A's rows carry a second proof made with g~ = O, whose
Schnorr check holds under every identity-decoding g~, so the pairing half of PoK verify is reached there.

STATES.  A state is (g~ encoding, X~ encoding, Y~ encodings joined): whatever cc_set_params / cc_set_verkey
last bound.  expect(mode, state, world) asks the C oracle (oc_verify_batch shared and per_cred_vk = 1,
oc_pok_verify) for the 8 rows of a world under a state; the per-verkey forms give every row the world's own
verkey and take only g~ from the state.  tile() repeats the 8 rows, and the expectations alike, to any
multiple of 8.
"""
import ctypes
import functools

from conftest import oracle_lib
from oracle import coconut_ref as C

import keygen_deal_cases as KD
from pok_prove_cases import World, fr, oracle_proof
from torsion_edges import fixture as torsion_fixture

R = C.R
MODES = {"G2": 0, "G1": 1}
WORLDS = {"A": (6, (3, 5)), "B": (3, (1,))}
ROWS, VALID = 8, 6
PR_O_ROW = 7
# one small-order point per OtherGroup (tests/golden/torsion.json): on the curve, outside the subgroup
TORSION = {"G2": ("G1", "T11"), "G1": ("G2", "T13")}
# the steps of test_gpu_rebind's sequence as (label, (g~ world, verkey world) bound after the step)
SEQUENCE = (("0 bind (gA, vkA)", ("A", "A")), ("1 set_params(gB)", ("B", "A")), ("2 set_verkey(vkB)", ("B", "B")),
            ("3 set_verkey(vkA)", ("B", "A")), ("4 set_params(gA)", ("A", "A")), ("5 12-bit tables", ("A", "A")),
            ("6a set_verkey(vkB)", ("A", "B")), ("6b set_params(gB)", ("B", "B")))
SAME_STATE_STEPS = ("5 12-bit tables",)  # the key is bound again at another width: nothing may change
CONSUMERS = ("verify", "verify_pervk", "pok", "pok_pervk", "engine")


def _sz(n):
    return ctypes.c_size_t(n)


def sizes(mode):
    """(SignatureGroup bytes, OtherGroup bytes)."""
    return (192, 97) if mode == "G2" else (97, 192)


@functools.lru_cache(None)
def world(mode, name):
    q, _ = WORLDS[name]
    return World(mode, q, "rebind-%s-%s" % (name, mode))


class _IdentityParams:
    """A world's verkey under g~ = O: what the prover sees when Params.g_tilde does not decode."""

    def __init__(self, w):
        self.grp, self.vk, self.g_tilde, self.q = w.grp, w.vk, None, w.q


def _proof_fields(w, pok, proof):
    e, o = w.grp.sig_to_bytes, w.grp.oth_to_bytes
    return dict(s1=e(pok["sig"][0]), s2=e(pok["sig"][1]), J=o(pok["J"]), T=o(pok["T"]),
                resp=b"".join(fr(v) for v in proof["responses"]))


@functools.lru_cache(None)
def rows(mode, name):
    """The 8 rows of a world: dicts of points, integers and encodings."""
    w = world(mode, name)
    q, revealed = WORLDS[name]
    grp = w.grp
    rng = C.Drbg("rebind-rows-%s-%s" % (name, mode))
    nresp = q - len(revealed) + 1
    out = []
    for i in range(ROWS):
        msgs = [rng.fr() for _ in range(q)]
        if i < VALID:
            sig = w.sign(msgs)
        elif i == 6:
            sig = w.sign([(msgs[0] + 1) % R] + msgs[1:])
        else:
            # x + sum y_j m_j = 0 (mod r): the last message from the others
            part = (w.x + sum(a * b for a, b in zip(w.y[:-1], msgs[:-1]))) % R
            msgs[-1] = (-part * pow(w.y[-1], -1, R)) % R
            assert (w.x + sum(a * b for a, b in zip(w.y, msgs))) % R == 0
            h = grp.sig.mul(grp.sig.gen, rng.fr())
            sig = (h, grp.sig.mul(h, rng.fr()))
        rand = [rng.fr() for _ in range(nresp + 2)]
        chal = rng.fr()
        row = dict(msgs=msgs, sig=sig, rand=rand, chal=chal, s1=grp.sig_to_bytes(sig[0]), s2=grp.sig_to_bytes(sig[1]))
        row["pok"] = _proof_fields(w, *oracle_proof(w, sig, msgs, revealed, rand, chal))
        if name == "A":
            row["pok_id"] = _proof_fields(w, *oracle_proof(_IdentityParams(w), sig, msgs, revealed, rand, chal))
        out.append(row)
    assert len({r["s1"] for r in out}) == ROWS
    return out


@functools.lru_cache(None)
def batch(mode, name, proofs="pok"):
    """The 8 rows as the byte buffers of the C ABI; proofs: "pok" (made under the world's g~) or "pok_id"
    (world A: made under g~ = O)."""
    w = world(mode, name)
    q, revealed = WORLDS[name]
    rs = rows(mode, name)
    g, X, Y = w.vk_bytes()
    cat = lambda f: b"".join(f(r) for r in rs)  # noqa: E731
    return dict(mode=mode, world=name, q=q, revealed=list(revealed), nresp=q - len(revealed) + 1, n=ROWS,
                s1=cat(lambda r: r["s1"]), s2=cat(lambda r: r["s2"]),
                msgs=cat(lambda r: b"".join(fr(m) for m in r["msgs"])),
                rand=cat(lambda r: b"".join(fr(v) for v in r["rand"])), chal=cat(lambda r: fr(r["chal"])),
                rev=cat(lambda r: b"".join(fr(r["msgs"][i]) for i in revealed)),
                ps1=cat(lambda r: r[proofs]["s1"]), ps2=cat(lambda r: r[proofs]["s2"]), J=cat(lambda r: r[proofs]["J"]),
                T=cat(lambda r: r[proofs]["T"]), resp=cat(lambda r: r[proofs]["resp"]),
                vkX=X * ROWS, vkY=b"".join(Y) * ROWS)


def valid_rows(b):
    """The batch of a world's 6 valid credentials (s1, s2, msgs): what the RLC engine is asked to accept."""
    sb = len(b["s1"]) // ROWS
    return b["s1"][:VALID * sb], b["s2"][:VALID * sb], b["msgs"][:VALID * b["q"] * 48]


# ---------------------------------------------------------------- states
def state(mode, g_world, vk_world):
    """(g~, X~, Y~) encodings: g~ of one world, the verkey of another."""
    g = world(mode, g_world).vk_bytes()[0]
    _, X, Y = world(mode, vk_world).vk_bytes()
    return g, X, b"".join(Y)


def state_q(mode, st):
    return len(st[2]) // sizes(mode)[1]


def world_of(mode, st):
    """The world whose q the state's verkey has: its batch is the one the bound verkey can be asked about."""
    return {q: name for name, (q, _) in WORLDS.items()}[state_q(mode, st)]


@functools.lru_cache(None)
def degenerate_forms(mode):
    """[(name, g~ encoding, kind)] of world A's g~: kind "identity" (decodes to the identity), "alias" (a
    coordinate >= p: the honest point) or "torsion" (a small-order point of the OtherGroup's curve)."""
    w = world(mode, "A")
    forms = KD.g1_forms(w.g_tilde) if mode == "G2" else KD.g2_forms(w.g_tilde)
    out = [(name, enc, "identity" if dec is None else "alias") for name, enc, dec in forms]
    grp, tname = TORSION[mode]
    out.append((tname, torsion_fixture()[grp][tname]["point"], "torsion"))
    return out


# ---------------------------------------------------------------- the oracle
def _oracle_verify(mode, b, X, Y, per_cred, g):
    n = b["n"]
    ver = ctypes.create_string_buffer(n)
    gts = ctypes.create_string_buffer(576 * n)
    oracle_lib().oc_verify_batch(MODES[mode], _sz(n), _sz(b["q"]), b["s1"], b["s2"], b["msgs"], X, Y, int(per_cred), g,
                                 ver, gts, 1)
    return list(ver.raw), gts.raw


def _oracle_pok(mode, b, X, Y, g):
    """([verdict], [GT bytes or None]): oc_pok_verify leaves no GT where it rejects before the pairing."""
    oc = oracle_lib()
    sb, ob = sizes(mode)
    q, r, nr = b["q"], len(b["revealed"]), b["nresp"]
    idx = (ctypes.c_uint64 * max(r, 1))(*b["revealed"])
    vs, gts = [], []
    for i in range(b["n"]):
        gt = ctypes.create_string_buffer(576)
        v = oc.oc_pok_verify(MODES[mode], _sz(q), _sz(r), b["ps1"][i * sb:(i + 1) * sb], b["ps2"][i * sb:(i + 1) * sb],
                             b["J"][i * ob:(i + 1) * ob], b["T"][i * ob:(i + 1) * ob],
                             b["resp"][i * nr * 48:(i + 1) * nr * 48], _sz(nr), b["chal"][48 * i:48 * (i + 1)], idx,
                             b["rev"][i * r * 48:(i + 1) * r * 48], X, Y, g, gt)
        vs.append(v)
        gts.append(gt.raw if any(gt.raw) else None)
    return vs, gts


@functools.lru_cache(None)
def in_subgroup(mode, enc):
    """Whether an OtherGroup encoding decodes to a point of order r (the identity does not count: the
    library's RLC refuses it, as cc_subgroup_check's status 0 says)."""
    curve, _, dec, _ = KD.oth(mode)
    pt = dec(enc)
    return pt is not None and curve.mul_any(pt, R) is None


@functools.lru_cache(None)
def expect(mode, st, name, proofs="pok"):
    """The oracle's results for the 8 rows of world `name` under state st = (g~, X~, Y~):
    verify (verdicts, GT) with the shared verkey, verify_pervk with the world's own verkey per row, pok
    (verdicts, [GT or None]), pok_pervk, and engine: whether the RLC on its own may accept the 6 valid rows
    (all of them verify and g~ and the verkey are in the subgroup)."""
    g, X, Y = st
    b = batch(mode, name, proofs)
    assert state_q(mode, st) == b["q"], "the shared-verkey forms need the batch of the bound q"
    out = {"verify": _oracle_verify(mode, b, X, Y, 0, g),
           "verify_pervk": _oracle_verify(mode, b, b["vkX"], b["vkY"], 1, g),
           "pok": _oracle_pok(mode, b, X, Y, g),
           "pok_pervk": _oracle_pok(mode, b, b["vkX"][:len(X)], b["vkY"][:len(Y)], g)}
    ob = sizes(mode)[1]
    pts = [g, X] + [Y[j * ob:(j + 1) * ob] for j in range(len(Y) // ob)]
    out["engine"] = all(v == 1 for v in out["verify"][0][:VALID]) and all(in_subgroup(mode, p) for p in pts)
    return out


def observed(mode, st, proofs="pok"):
    """What test_gpu_rebind compares the device with under a state: expect() for the bound verkey's world."""
    return expect(mode, st, world_of(mode, st), proofs)


# ---------------------------------------------------------------- tiling
def tile(buf, n):
    """A buffer of 8 rows repeated to n rows (n a multiple of 8)."""
    assert n % ROWS == 0
    return buf * (n // ROWS)


def tile_batch(b, n):
    out = dict(b, n=n)
    for k in ("s1", "s2", "msgs", "rand", "chal", "rev", "ps1", "ps2", "J", "T", "resp", "vkX", "vkY"):
        out[k] = tile(b[k], n)
    return out


def tile_expect(e, n):
    """(verdicts, GT) of 8 rows repeated to n rows; GT a byte string (verify) or a list (PoK)."""
    v, gt = e
    return tile(v, n), tile(gt, n)
