"""Shared inputs and oracle expectations of the holder-side tests (test_pok_prove_abi.py: the model check
on the CPU; test_gpu_pok_prove.py: the same inputs through cc_pok_init_batch / cc_pok_gen_proof_batch).

Everything expected here comes from oracle/coconut_ref.py (pok_init / pok_to_bytes / pok_gen_proof /
pok_verify_gt) and oracle/issuance.py (unblind); the randomness init draws (r1, r2, b_0 ..) is fixed per
case and replayed into the oracle, so the GPU is given the very same scalars as `rand`."""
import functools

from oracle import coconut_ref as C

R = C.R
CONFIG5_REVEALED = (3, 5, 7, 11, 13, 17, 19, 23)  # the eight revealed indices of bench config 5 (bench_modes.REVEALED)


def fr(v):
    return (v % R).to_bytes(48, "big")


def be48(v):
    """48 bytes big-endian WITHOUT reduction (the ABI reduces a value >= r itself)."""
    return v.to_bytes(48, "big")


class Replay:
    """Stands in for the Drbg pok_init draws from: hands out the recorded scalars in order."""

    def __init__(self, vals):
        self.vals = list(vals)

    def fr(self):
        return self.vals.pop(0)


class World:
    """One verkey with its secret key, so that signatures over any messages can be made."""

    def __init__(self, mode, q, seed, y=None):
        self.mode, self.q = mode, q
        self.grp = grp = C.Groups(mode)
        self.rng = rng = C.Drbg(seed)
        self.g_tilde = grp.other.mul(grp.other.gen, rng.fr())
        self.x = rng.fr()
        self.y = [rng.fr() for _ in range(q)] if y is None else [v if v is not None else rng.fr() for v in y]
        self.vk = (grp.other.mul(self.g_tilde, self.x), [grp.other.mul(self.g_tilde, v) for v in self.y])

    def sign(self, msgs, k=None):
        grp = self.grp
        h = grp.sig.mul(grp.sig.gen, self.rng.fr() if k is None else k)
        return C.sign(grp, (self.x, self.y), msgs, h)

    def vk_bytes(self):
        e = self.grp.oth_to_bytes
        return e(self.g_tilde), e(self.vk[0]), [e(v) for v in self.vk[1]]


def oracle_proof(w, sig, msgs, revealed, rand, chal, sig_pts=None):
    """pok_init with the draws `rand` (reduced mod r as the ABI reduces them), then gen_proof.
    sig_pts: the points the sigma encodings decode to (an off-curve encoding decodes to the identity)."""
    grp = w.grp
    pok = C.pok_init(grp, sig if sig_pts is None else sig_pts, w.vk, w.g_tilde, [m % R for m in msgs], set(revealed),
                     Replay([v % R for v in rand]))
    proof = C.pok_gen_proof(pok, chal % R)
    return pok, proof


def proof_bytes(grp, pok, proof):
    return dict(s1=grp.sig_to_bytes(pok["sig"][0]), s2=grp.sig_to_bytes(pok["sig"][1]), J=grp.oth_to_bytes(pok["J"]),
                T=grp.oth_to_bytes(pok["T"]), resp=b"".join(fr(v) for v in proof["responses"]),
                to_bytes=C.pok_to_bytes(grp, pok))


def off_curve(enc):
    """A SignatureGroup encoding with y + 1: not on the curve, decodes to the identity."""
    b = bytearray(enc)
    b[-1] ^= 1
    return bytes(b)


@functools.lru_cache(maxsize=None)
def edge_batches(mode):
    """The edge cases as batches [(name, world, revealed, [case ...])]; a case is a dict with the inputs
    (sig encodings s1 / s2, msgs, rand = [r1, r2, b_0 ..] as integers, possibly >= r, chal) and `valid`:
    whether ps_sig's verifier accepts the proof init and gen_proof make from them."""
    q = 3
    grp = C.Groups(mode)
    se = grp.sig_to_bytes
    rng = C.Drbg("pok-prove-edges-" + mode)
    out = []

    def case(name, w, revealed, valid, sig=None, msgs=None, rand=None, s1=None, s2=None, sig_pts=None, chal=None):
        msgs = [rng.fr() for _ in range(w.q)] if msgs is None else msgs
        sig = w.sign(msgs) if sig is None else sig
        nresp = w.q - len(revealed) + 1
        rand = [rng.fr() for _ in range(nresp + 2)] if rand is None else rand(nresp)
        return dict(name=name, valid=valid, sig=sig, sig_pts=sig_pts, s1=s1 or se(sig[0]), s2=s2 or se(sig[1]),
                    msgs=msgs, rand=rand, chal=rng.fr() if chal is None else chal)

    def draws(nresp, **fix):
        v = [rng.fr() for _ in range(nresp + 2)]
        for k, x in fix.items():
            v[{"r1": 0, "r2": 1}[k]] = x
        return v

    w = World(mode, q, "edge-vk-" + mode)
    rev = (1,)
    h = grp.sig.mul(grp.sig.gen, rng.fr())
    m0 = [rng.fr() for _ in range(q)]
    real = w.sign(m0)
    a = [
        # r1 = 0: both sigma' are the identity and the verifier says no
        case("r1=0", w, rev, False, rand=lambda n: draws(n, r1=0)),
        case("r2=0", w, rev, True, rand=lambda n: draws(n, r2=0)),
        case("r1=r-1", w, rev, True, rand=lambda n: draws(n, r1=R - 1)),
        # (h, h) is no signature; with r2 = r - 1 sigma'_2 = r1 (h - h) is the identity
        case("s2=s1,r2=r-1", w, rev, False, sig=(h, h), rand=lambda n: draws(n, r2=R - 1)),
        # (h, h) with r2 = 1: B's two terms meet in a doubling inside every window where the digits agree
        case("s2=s1,r2=1", w, rev, False, sig=(h, h), rand=lambda n: draws(n, r2=1)),
        case("s2=-s1,r2=1", w, rev, False, sig=(h, grp.sig.neg(h)), rand=lambda n: draws(n, r2=1)),
        case("s1=identity", w, rev, False, sig=(None, real[1])),
        case("s1 off-curve", w, rev, False, sig=real, msgs=m0, s1=off_curve(se(real[0])), sig_pts=(None, real[1])),
        case("blindings=0", w, rev, True, rand=lambda n: draws(n)[:2] + [0] * n),
        case("hidden m=0", w, rev, True, msgs=[0, rng.fr(), rng.fr()]),
        # a scalar handed over as r + 5 in 48 bytes is reduced
        case("r1=r+5", w, rev, True, rand=lambda n: draws(n, r1=R + 5)),
    ]
    out.append(("scalars and sigma", w, rev, a))
    y0 = rng.fr()
    mm = rng.fr()
    w1 = World(mode, q, "edge-vk1-" + mode, y=[y0, y0, None])
    out.append(("Y1=Y0", w1, (), [case("Y1=Y0, equal messages", w1, (), True, msgs=[mm, mm, rng.fr()])]))
    w2 = World(mode, q, "edge-vk2-" + mode, y=[y0, R - y0, None])
    out.append(("Y1=-Y0", w2, (), [case("Y1=-Y0, equal messages", w2, (), True, msgs=[mm, mm, rng.fr()])]))
    w3 = World(mode, q, "edge-vk3-" + mode, y=[None, None, 0])
    out.append(("Y2=identity", w3, (0,), [case("Y2 identity", w3, (0,), True)]))
    out.append(("r=0", w, (), [case("nothing revealed", w, (), True)]))
    out.append(("r=q", w, (0, 1, 2), [case("all revealed", w, (0, 1, 2), True)]))
    return out


@functools.lru_cache(maxsize=None)
def edge_expected(mode):
    """edge_batches with every case's oracle proof bytes added (key `want`) and its revealed messages."""
    res = []
    for name, w, rev, cases in edge_batches(mode):
        done = []
        for c in cases:
            pok, proof = oracle_proof(w, c["sig"], c["msgs"], rev, c["rand"], c["chal"], c["sig_pts"])
            done.append(dict(c, want=proof_bytes(w.grp, pok, proof), proof=proof))
        res.append((name, w, rev, done))
    return res


@functools.lru_cache(maxsize=None)
def drbg_batch(mode, q, revealed, n, seed):
    """n credentials under one verkey; each proof's draws come from its own Drbg, which the oracle is
    given seeded the same way (test 1 of the issue)."""
    w = World(mode, q, f"vk-{mode}-{q}-{seed}")
    rng = C.Drbg(f"msgs-{mode}-{q}-{seed}")
    nresp = q - len(revealed) + 1
    rows = []
    for i in range(n):
        msgs = [rng.fr() for _ in range(q)]
        sig = w.sign(msgs)
        chal = rng.fr()
        d = C.Drbg(f"draws-{mode}-{q}-{seed}-{i}")
        rand = [d.fr() for _ in range(nresp + 2)]
        pok = C.pok_init(w.grp, sig, w.vk, w.g_tilde, msgs, set(revealed), C.Drbg(f"draws-{mode}-{q}-{seed}-{i}"))
        proof = C.pok_gen_proof(pok, chal)
        rows.append(dict(sig=sig, s1=w.grp.sig_to_bytes(sig[0]), s2=w.grp.sig_to_bytes(sig[1]), msgs=msgs, rand=rand,
                         chal=chal, want=proof_bytes(w.grp, pok, proof)))
    return w, rows


def response_cases():
    """(b, chal, secret) triples for gen_proof against plain integers."""
    rng = C.Drbg("responses")
    c, s = rng.fr(), rng.fr()
    return [("chal=0", rng.fr(), 0, rng.fr()), ("chal=r-1", rng.fr(), R - 1, rng.fr()), ("secret=0", rng.fr(), c, 0),
            ("b<chal*secret", (c * s - 1) % R, c, s), ("b=chal*secret", c * s % R, c, s), ("b=0", 0, c, s),
            ("unreduced", R + 3, R + 1, R + 2)]
