"""Edge-case inputs for the issuer's and the dealer's rows: cc_sigreq_verify_batch (issue.hip
k_sigreq_checks, k_sigreq_combine) and cc_vss_verify_batch (k_vss_verify), with a model of the ladder both
kernels share, and the inputs of compute_h's canonicalisation (k_h_input_canon).

Plain Python, the C oracle (oc_msm, oc_gen_mul: sums over ENCODED points with possibly non-canonical
scalars) and the Python oracle (oracle/issuance.py compute_h, oracle/bls12_381.py curve arithmetic); no
product code and no context.

THE LADDER.  Both kernels decode their bases into per-lane scratch with a finite flag, walk MSB-first from
bit 254 with one doubling per bit and, per bit, add in entry order every finite base whose bit is set
(curve.h jac_add_aff); k_sigreq_checks then adds -T where T decodes to a finite point and accepts when the
sum is the identity.  ladder() restates the walk on affine points and names the branch every addition takes
(the CHAIN names of tests/fixed_edges.py):

    fresh          the accumulator is the identity because nothing was added yet
    from-identity  the accumulator is the identity again after a to-identity: the sum restarts from the base
    doubling       the accumulator equals the base            (h == 0, r == 0)
    to-identity    the accumulator is the base's negative     (h == 0, r != 0)
    general
    skipped        the base decoded to the identity (flag 0): never added, whatever its scalar

REQUEST PROOFS.  A Schnorr check accepts any responses and challenge once T = sum resp_j B_j + chal C, so
every case chooses bases, responses and challenge freely and takes T from oc_msm over the encodings it
sends.  elgamal_pk, the commitment and the ciphertexts are per request; g and h_j are per call (a "call"
below is one cc_sigreq_verify_batch); h = compute_h(commitment, known) is fixed by the request, so the cases
relate elgamal_pk and c2 to it.  The four check kinds (KINDS) and their ladder entries, in order:

    sk    g: r_sk, elgamal_pk: chal                          T_sk
    comm  h_0: r_comm[0] .. h_(k-1): r_comm[k-1], g: r_comm[k], commitment: chal      T_comm
    ct1   g: r_1[i], c1_i: chal                              T_1[i]
    ct2   elgamal_pk: r_2a[i], h: r_2b[i], c2_i: chal        T_2[i]

and k_sigreq_combine's rule r_2b[i] == r_comm[i] (mod r).

VSS SHARES.  Everything lives in the group spanned by g and h: C_k = a_k g + b_k h by oc_msm, and a share of
id is valid exactly when s = sum a_k id^k, s' = sum b_k id^k (mod r).  The ladder's entries: g: -s, h: -s'
("gh"), then C_k: id^k ("C").

EXPECTATIONS come from the C oracle (expect_request, expect_share): oc_msm over the encodings sent, with
the oracle's decode rules (off-curve or bad prefix -> identity, scalars mod r, coordinates mod p), compared
with the decoded T or between the two sides.  Every case also carries the verdict its construction intends;
tests/test_issuer_edges_model.py asserts that the two and the Python oracle's sigreq_proof_verify /
verify_share agree and that every named case reaches its branch, tests/test_gpu_issuer_edges.py runs the
cases on the device.
"""
import ctypes
import functools
import random

from conftest import host_threads
from fixed_edges import CHAIN, G1_IDENTITY, G2_IDENTITY, P, R, be48, gen_mul
from torsion_edges import fixture as torsion_fixture

BRANCHES = CHAIN + ("skipped",)
KINDS = ("sk", "comm", "ct1", "ct2")
MODES = {"G2": 0, "G1": 1}
TOP = 1 << 200  # related-base cases: two scalars whose top set bit is this one, every other scalar below
EDGE_SCALARS = (("zero", 0), ("one", 1), ("r_minus_1", R - 1), ("r", R), ("r_plus_1", R + 1),
                ("max", (1 << 384) - 1), ("bit254", 1 << 254))
SHAPES = ((3, 0), (3, 1), (3, 3), (6, 2), (18, 17))  # (q, k)
# sub-batches of a call's list: one request, exactly 64 lanes of k_sigreq_checks (n (2 + 2 k) = 64), one
# more, and with k = 2 / k = 17 a request whose lanes straddle two blocks (6 and 36 lanes a request)
SLICES = {(3, 0): (1, 32, 33), (3, 1): (1, 16, 17), (3, 3): (1, 8, 9), (6, 2): (1, 11), (18, 17): (1, 2)}


# the requests that go with a call's own case where g or an h_j is special (accepting and rejecting ones)
SPECIAL_KEEP = {"valid_random", "scalars_mixed", "scalars_all_zero", "valid_distinct_bytes", "T_negated_ct2",
                "T_identity_ct2", "T_off_curve_ct2", "combine_v_and_v_plus_1_0", "combine_v_and_v_plus_r_1",
                "flip_challenge_sk"}


class Env:
    """One group (1 or 2) through the oracles: encodings in, encodings out."""

    def __init__(self, oc, group):
        from oracle import bls12_381 as B
        from oracle import coconut_ref as C
        self.oc, self.group = oc, group
        self.sb = 97 if group == 1 else 192
        self.identity = G1_IDENTITY if group == 1 else G2_IDENTITY
        self.grp = C.Groups("G1" if group == 1 else "G2")  # the assignment whose SignatureGroup this is
        self.curve = B.G1 if group == 1 else B.G2
        self._dec = B.g1_from_bytes if group == 1 else B.g2_from_bytes
        self._enc = B.g1_to_bytes if group == 1 else B.g2_to_bytes
        self._pool = []

    def muls(self, ks):
        raw = gen_mul(self.oc, self.group, list(ks))
        return [raw[i * self.sb:(i + 1) * self.sb] for i in range(len(ks))]

    def rand_pt(self, rng):
        """A random multiple of the generator (drawn 256 at a time on the host's threads)."""
        if not self._pool:
            ks = b"".join(be48(rng.randrange(1 << 250, R)) for _ in range(256))
            out = ctypes.create_string_buffer(self.sb * 256)
            self.oc.oc_gen_mul_mt(self.group, ctypes.c_size_t(256), ks, out, host_threads())
            self._pool = [out.raw[i * self.sb:(i + 1) * self.sb] for i in range(256)]
        return self._pool.pop()

    def msm(self, pts, scalars):
        """sum k_i P_i over encodings and encoded (unreduced) scalars, canonical bytes (oc_msm)."""
        assert len(pts) == len(scalars) and all(len(p) == self.sb for p in pts)
        out = ctypes.create_string_buffer(self.sb)
        self.oc.oc_msm(self.group, ctypes.c_size_t(len(pts)), b"".join(pts), b"".join(be48(s) for s in scalars), out)
        return out.raw

    def canon(self, pt):
        """What the oracle decodes pt to, re-encoded (the identity encoding for an off-curve pt)."""
        return self.msm([pt], [1])

    def neg(self, pt):
        return self.msm([pt], [R - 1])

    def dec(self, pt):
        return self._dec(pt)

    def enc(self, point):
        return self._enc(point)

    def off_curve(self, pt):
        """pt with the lowest bit of its last coordinate flipped."""
        return pt[:-1] + bytes([pt[-1] ^ 1])

    def bad_prefix(self, pt):
        assert self.group == 1
        return b"\x03" + pt[1:]

    def shifted(self, pt, j):
        """pt with j p added to every coordinate (j = 'max': the largest that still fits 48 bytes)."""
        head, body = (pt[:1], pt[1:]) if self.group == 1 else (b"", pt)
        out = []
        for o in range(0, len(body), 48):
            v = int.from_bytes(body[o:o + 48], "big")
            jj = ((1 << 384) - 1 - v) // P if j == "max" else j
            assert jj >= 1 and v + jj * P < 1 << 384
            out.append(be48(v + jj * P))
        return head + b"".join(out)

    def identity_forms(self, rng):
        """[(name, an encoding that decodes to the identity)]."""
        forms = [("identity", self.identity), ("off_curve", self.off_curve(self.rand_pt(rng)))]
        if self.group == 1:
            forms.append(("bad_prefix", self.bad_prefix(self.rand_pt(rng))))
        return forms


# ---------------------------------------------------------------- the model of the ladder
def ladder(curve, entries, T=False):
    """entries: [(affine point or None, scalar, tag)] in the kernel's order; T: the decoded T (None: it
    decoded to the identity; False: the walk has no last step, as in k_vss_verify).
    Returns dict(sum: the point before the last step, log: [(tag, branch)], final: the branch of the
    addition of -T or 'skipped', ok: the kernel's verdict)."""
    ent = [(pt, s % R, tag) for pt, s, tag in entries]
    log = [(tag, "skipped") for pt, _, tag in ent if pt is None]
    st = dict(acc=None, seen=False)

    def add(pt, tag, log):
        acc = st["acc"]
        if acc is None:
            b = "from-identity" if st["seen"] else "fresh"
        elif acc == pt:
            b = "doubling"
        elif acc == curve.neg(pt):
            b = "to-identity"
        else:
            b = "general"
        st["seen"] = True
        st["acc"] = curve.add(acc, pt)
        log.append((tag, b))
        return b

    for bit in range(254, -1, -1):
        st["acc"] = curve.add(st["acc"], st["acc"])
        for pt, s, tag in ent:
            if pt is not None and (s >> bit) & 1:
                add(pt, tag, log)
    total = st["acc"]
    final = None
    if T is not False:
        final = "skipped" if T is None else add(curve.neg(T), "T", [])
    return dict(sum=total, log=log, final=final, ok=st["acc"] is None)


# ---------------------------------------------------------------- request proofs
def check_list(call, req):
    """[((kind, i), bases, scalars, C)] of one request: its 2 + 2 k Schnorr checks in lane order."""
    k, g = call["k"], call["g"]
    out = [(("sk", 0), [g], [req["r_sk"]], req["pk"]),
           (("comm", 0), list(call["hvec"][:k]) + [g], list(req["r_comm"]), req["commitment"])]
    for i in range(k):
        out.append((("ct1", i), [g], [req["r1"][i]], req["cts"][i][0]))
        out.append((("ct2", i), [req["pk"], req["h"]], [req["r2a"][i], req["r2b"][i]], req["cts"][i][1]))
    return out


def _finish(env, call, req):
    """Resolve the fields that depend on h, then T of every check from the oracle, then the overrides."""
    from oracle import issuance as I
    h = env.enc(I.compute_h(env.grp, env.dec(req["commitment"]), [m % R for m in req["known"]]))
    req["h"] = h
    if callable(req["pk"]):
        req["pk"] = req["pk"](h)
    req["cts"] = [[c(h) if callable(c) else c for c in pair] for pair in req["cts"]]
    req["T"] = {}
    for key, bases, scal, C in check_list(call, req):
        t = env.msm(bases + [C], scal + [req["T_chal"].get(key, req["chal"])])
        req["T"][key] = req["T_mod"][key](t) if key in req["T_mod"] else t
    for f in req["post"]:
        f(req)
    return req


def proof_bytes(call, req):
    """The record cc_sigreq_verify_batch reads (sigreq_layout.h):
    T_sk | r_sk | T_comm | r_comm[0..k] | k x (T_1 | r_1 | T_2 | r_2a | r_2b)."""
    T = req["T"]
    out = [T[("sk", 0)], be48(req["r_sk"]), T[("comm", 0)]] + [be48(v) for v in req["r_comm"]]
    for i in range(call["k"]):
        out += [T[("ct1", i)], be48(req["r1"][i]), T[("ct2", i)], be48(req["r2a"][i]), be48(req["r2b"][i])]
    return b"".join(out)


def expect_checks(env, call, req):
    """{(kind, i): 0 / 1} from the C oracle: the sum over the encodings equals what T decodes to."""
    return {key: int(env.msm(bases + [C], scal + [req["chal"]]) == env.canon(req["T"][key]))
            for key, bases, scal, C in check_list(call, req)}


def expect_request(env, call, req):
    """SignatureRequestProof::verify's verdict from the C oracle's sums and the response-equality rule."""
    ok = all(expect_checks(env, call, req).values())
    return int(ok and all(a % R == b % R for a, b in zip(req["r2b"], req["r_comm"])))


def trace_check(env, call, req, key):
    """ladder() of one check of a request, on the decoded points."""
    for kk, bases, scal, C in check_list(call, req):
        if kk == key:
            ent = [(env.dec(b), s, key[0]) for b, s in zip(bases + [C], scal + [req["chal"]])]
            return ladder(env.curve, ent, env.dec(req["T"][key]))
    raise KeyError(key)


def python_verdict(env, call, req):
    """oracle/issuance.py sigreq_proof_verify on the decoded inputs."""
    from oracle import issuance as I
    k, T = call["k"], req["T"]
    d = env.dec
    proof = {"sk": {"T": d(T[("sk", 0)]), "responses": [req["r_sk"] % R]},
             "comm": {"T": d(T[("comm", 0)]), "responses": [v % R for v in req["r_comm"]]},
             "cts": [({"T": d(T[("ct1", i)]), "responses": [req["r1"][i] % R]},
                      {"T": d(T[("ct2", i)]), "responses": [req["r2a"][i] % R, req["r2b"][i] % R]}) for i in range(k)]}
    rq = {"known": [m % R for m in req["known"]], "commitment": d(req["commitment"]),
          "ciphertexts": [(d(a), d(b)) for a, b in req["cts"]]}
    params = {"g": d(call["g"]), "h": [d(x) for x in call["hvec"]]}
    return int(I.sigreq_proof_verify(env.grp, proof, rq, d(req["pk"]), req["chal"] % R, params))


def _distinct_scalar(rng):
    """A 48-byte value whose bytes are pairwise different (a misread at any offset changes it)."""
    return int.from_bytes(bytes(rng.sample(range(256), 48)), "big")


def request_cases(env, call, rng, short=False, keep=None):
    """The named requests of one call, finished (T from the oracle).  Each: dict(name, intent: the verdict
    the construction means, reach: [(kind, branch)] the model must report (branch 'final:<b>': the
    addition of -T), + the fields sent).  short: without the cases that do not depend on the call's g and h_j;
    keep: a predicate on the names."""
    q, k, g = call["q"], call["k"], call["g"]
    fr = lambda: rng.randrange(1 << 250, R)  # noqa: E731
    out = []

    def new(name, intent, *reach):
        rc = [fr() for _ in range(k + 1)]
        req = dict(name=name, intent=intent, reach=list(reach), pk=env.rand_pt(rng),
                   commitment=env.rand_pt(rng), known=[fr() for _ in range(q - k)],
                   cts=[[env.rand_pt(rng), env.rand_pt(rng)] for _ in range(k)], r_sk=fr(), r_comm=rc,
                   r1=[fr() for _ in range(k)], r2a=[fr() for _ in range(k)], r2b=list(rc[:k]), chal=fr(),
                   T_mod={}, T_chal={}, post=[])
        out.append(req)
        return req

    def set_all(req, vals):
        """Every response and the challenge from the cycle vals (r_2b follows r_comm: the combine rule)."""
        it = iter(vals * (3 * k + 3))
        req["r_sk"], req["chal"] = next(it), next(it)
        req["r_comm"] = [next(it) for _ in range(k + 1)]
        req["r1"], req["r2a"] = [next(it) for _ in range(k)], [next(it) for _ in range(k)]
        req["r2b"] = list(req["r_comm"][:k])

    def small(req, but=()):
        """Every response and the challenge below TOP (nonzero, different), except the names in `but`."""
        if "r_sk" not in but:
            req["r_sk"] = 3
        if "chal" not in but:
            req["chal"] = (1 << 100) + 7
        req["r_comm"] = [11 + 2 * j for j in range(k + 1)]
        req["r1"], req["r2a"] = [5 + j for j in range(k)], [(1 << 90) + j for j in range(k)]
        req["r2b"] = list(req["r_comm"][:k])

    keys = [("sk", 0), ("comm", 0)] + ([("ct1", k - 1), ("ct2", k - 1)] if k else [])
    last = k - 1

    new("valid_random", 1)
    # ---- responses and challenge at the edges of fr_from_be48 and of the walk
    for nm, v in EDGE_SCALARS:
        set_all(new(f"scalars_all_{nm}", 1), [v])  # zero / r: every sum is the identity, T its encoding
    set_all(new("scalars_mixed", 1), [v for _, v in EDGE_SCALARS])
    set_all(new("valid_distinct_bytes", 1), [_distinct_scalar(rng) for _ in range(3 * k + 3)])
    if not short:
        for key in keys:  # identity sum, T sent as something else
            r0 = new(f"zero_sum_finite_T_{key[0]}", 0)
            set_all(r0, [0, R])
            pt = env.rand_pt(rng)
            r0["T_mod"][key] = lambda t, pt=pt: pt
        r0 = new("zero_sum_off_curve_T", 1)
        set_all(r0, [0])
        for key in keys:
            r0["T_mod"][key] = lambda t, pt=env.off_curve(env.rand_pt(rng)): pt
        if env.group == 1:
            r0 = new("zero_sum_bad_prefix_T", 1)
            set_all(r0, [R, 0])
            for key in keys:
                r0["T_mod"][key] = lambda t, pt=env.bad_prefix(env.rand_pt(rng)): pt
    # ---- T, on a check that is otherwise valid
    tforms = [("identity", lambda t: env.identity, "final:skipped"), ("off_curve", env.off_curve, "final:skipped"),
              ("negated", env.neg, "final:doubling")]
    if env.group == 1:
        tforms.append(("bad_prefix", env.bad_prefix, "final:skipped"))
    for key in keys if not short else keys[-1:]:
        for nm, f, br in tforms:
            new(f"T_{nm}_{key[0]}", 0, (key[0], br))["T_mod"][key] = f
    # ---- related bases among the per-request inputs
    ng = env.neg(g)
    r0 = new("pk_eq_g", 1, ("sk", "doubling"))
    small(r0, ("r_sk", "chal"))
    r0.update(pk=g, r_sk=TOP + 5, chal=TOP + 3)
    r0 = new("pk_eq_neg_g", 1, ("sk", "to-identity"), ("sk", "from-identity"))
    small(r0, ("r_sk", "chal"))
    r0.update(pk=ng, r_sk=TOP + 4, chal=TOP + 1)
    r0 = new("commitment_eq_g", 1, ("comm", "doubling"))
    small(r0, ("chal",))
    r0.update(commitment=g, chal=TOP + 3)
    r0["r_comm"][k] = TOP + 5
    r0 = new("commitment_eq_neg_g", 1, ("comm", "to-identity"), ("comm", "from-identity"))
    small(r0, ("chal",))
    r0.update(commitment=ng, chal=TOP + 1)
    r0["r_comm"][k] = TOP + 4
    if k:
        r0 = new("c1_eq_g", 1, ("ct1", "doubling"))
        small(r0, ("chal",))
        r0["cts"][last][0], r0["r1"][last], r0["chal"] = g, TOP + 5, TOP + 3
        r0 = new("c1_eq_neg_g", 1, ("ct1", "to-identity"), ("ct1", "from-identity"))
        small(r0, ("chal",))
        r0["cts"][last][0], r0["r1"][last], r0["chal"] = ng, TOP + 4, TOP + 1
        r0 = new("pk_eq_h", 1, ("ct2", "doubling"))
        small(r0)
        r0["pk"], r0["r2a"][last] = (lambda h: h), TOP + 5
        r0["r2b"][last] = r0["r_comm"][last] = TOP + 3
        r0 = new("pk_eq_neg_h", 1, ("ct2", "to-identity"), ("ct2", "from-identity"))
        small(r0)
        r0["pk"], r0["r2a"][last] = env.neg, TOP + 4
        r0["r2b"][last] = r0["r_comm"][last] = TOP + 1
        r0 = new("c2_eq_h", 1, ("ct2", "doubling"))
        small(r0, ("chal",))
        r0["cts"][last][1], r0["chal"] = (lambda h: h), TOP + 3
        r0["r2b"][last] = r0["r_comm"][last] = TOP + 5
    # ---- per-request bases that decode to the identity
    for nm, form in env.identity_forms(rng)[1 if short else 0:2 if short else None]:
        new(f"pk_{nm}", 1, ("sk", "skipped"), *([("ct2", "skipped")] if k else []))["pk"] = form
        new(f"commitment_{nm}", 1, ("comm", "skipped"))["commitment"] = form  # h: of the decoded point
        if k:
            new(f"c1_{nm}", 1, ("ct1", "skipped"))["cts"][last][0] = form
            new(f"c2_{nm}", 1, ("ct2", "skipped"))["cts"][0][1] = form
    # ---- coordinates >= p: T from the canonical encodings, the shifted ones sent
    if not short:
        for j in (1, "max"):
            r0 = new(f"pk_coords_plus_{j}p", 1)

            def shift_pk(req, j=j):
                req["pk"] = env.shifted(req["pk"], j)
            r0["post"].append(shift_pk)
            if k:
                r0 = new(f"ct_coords_plus_{j}p", 1)

                def shift_ct(req, j=j):
                    req["cts"][0] = [env.shifted(c, j) for c in req["cts"][0]]
                r0["post"].append(shift_ct)
        # ---- points of small order as elgamal_pk (the decoders test the curve equation alone)
        tor = torsion_fixture()["G1" if env.group == 1 else "G2"]
        for nm in ("T3", "-T3") if env.group == 1 else ("T13", "-T13"):
            new(f"pk_{nm}", 1)["pk"] = tor[nm]["point"]
    # ---- k_sigreq_combine alone: every Schnorr check valid, the two copies of a hidden response differ
    for i in sorted({0, last}) if k else []:
        v = fr()
        r0 = new(f"combine_v_and_v_plus_r_{i}", 1)
        r0["r_comm"][i], r0["r2b"][i] = v, v + R
        r0 = new(f"combine_v_plus_r_and_v_{i}", 1)
        r0["r_comm"][i], r0["r2b"][i] = v + R, v
        r0 = new(f"combine_v_and_v_plus_1_{i}", 0)
        r0["r_comm"][i], r0["r2b"][i] = v, v + 1
    # ---- one flipped bit per field of the layout, scalars of pairwise different bytes
    for key in keys if not short else keys[:1]:
        kind, i = key
        r0 = new(f"flip_response_{kind}", 0)
        set_all(r0, [_distinct_scalar(rng) for _ in range(3 * k + 3)])
        # T of this check from the unflipped response (for ct2 / comm the flipped one is a response the
        # combine rule does not read: r_2a, r_comm[k])
        name, idx = {"sk": ("r_sk", None), "comm": ("r_comm", k), "ct1": ("r1", i), "ct2": ("r2a", i)}[kind]

        def flip(req, name=name, idx=idx):
            if idx is None:
                req[name] ^= 1 << 59
            else:
                req[name][idx] ^= 1 << 59
        r0["post"].append(flip)
        r0 = new(f"flip_T_{kind}", 0)
        set_all(r0, [_distinct_scalar(rng) for _ in range(3 * k + 3)])
        r0["T_mod"][key] = lambda t: t[:env.sb // 2] + bytes([t[env.sb // 2] ^ 0x10]) + t[env.sb // 2 + 1:]
        r0 = new(f"flip_challenge_{kind}", 0)  # this check's T alone is of the other challenge
        set_all(r0, [_distinct_scalar(rng) for _ in range(3 * k + 3)])
        r0["T_chal"][key] = r0["chal"] ^ (1 << 59)
    return [_finish(env, call, r) for r in out if keep is None or keep(r["name"])]


def _params(env, q, seed):
    rng = random.Random(seed)
    return env.rand_pt(rng), [env.rand_pt(rng) for _ in range(q)]


@functools.lru_cache(maxsize=None)
def _sigreq_calls(oc_key, mode):
    oc = _OC[oc_key]
    env = Env(oc, 2 if mode == "G2" else 1)
    seed0 = 100 * MODES[mode]
    calls = []
    for q, k in SHAPES:
        g, hvec = _params(env, q, seed0 + 10 * q + k)
        call = dict(name=f"q{q}k{k}", q=q, k=k, g=g, hvec=hvec, slices=SLICES[(q, k)])
        # k = 17 (36 lanes a request, 19 ladder entries): the combine rule at i = 0 and i = 16, a few others
        wide = (lambda nm: nm.startswith(("valid_", "scalars_mixed", "combine_", "flip_", "T_negated", "pk_eq_neg_h")))
        call["reqs"] = request_cases(env, call, random.Random(seed0 + q + k), short=k == 17,
                                     keep=wide if k == 17 else None)
        calls.append(call)
    # per-call bases: g and one h_j as the identity, related h_j; k = 2, 11 requests = 66 lanes
    q, k = 6, 2
    g0, h0 = _params(env, q, seed0 + 77)
    rng = random.Random(seed0 + 78)
    special = [(f"g_{nm}", form, h0, None) for nm, form in env.identity_forms(rng)]
    special += [(f"h1_{nm}", g0, [h0[0], form] + h0[2:], None) for nm, form in env.identity_forms(rng)]
    special += [("h1_eq_h0", g0, [h0[0], h0[0]] + h0[2:], (TOP + 5, TOP + 3, 13, "doubling")),
                ("h1_eq_neg_h0", g0, [h0[0], env.neg(h0[0])] + h0[2:], (TOP + 4, TOP + 1, 13, "to-identity")),
                ("h0_eq_g", g0, [g0] + h0[1:], (TOP + 5, 9, TOP + 3, "doubling"))]
    for nm, g, hvec, rel in special:
        call = dict(name=nm, q=q, k=k, g=g, hvec=hvec, slices=())
        reqs = request_cases(env, call, random.Random(seed0 + 79), short=True, keep=SPECIAL_KEEP.__contains__)
        assert len(reqs) == 10
        call["reqs"] = reqs
        # the call's own case: the base that is special here, in the check that reads it
        r0 = dict(reqs[0], name=nm, intent=1, T_mod={}, T_chal={}, post=[])
        if rel:
            r0.update(r_comm=list(rel[:3]), r2b=list(rel[:2]), chal=(1 << 100) + 7,
                      reach=[("comm", rel[3])] + ([("comm", "from-identity")] if rel[3] == "to-identity" else []))
        else:
            r0["reach"] = [("comm", "skipped")]
            if nm.startswith("g_"):
                r0["reach"] += [("sk", "skipped"), ("ct1", "skipped")]
        call["reqs"].append(_finish(env, call, r0))
        calls.append(call)
    return calls


_OC = {}


def sigreq_calls(oc, mode):
    """The calls of one group mode ('G2' / 'G1'): [dict(name, q, k, g, hvec, reqs, slices)], shared between
    tests, not to be modified."""
    _OC[id(oc)] = oc
    return _sigreq_calls(id(oc), mode)


def call_args(call, reqs):
    """The arguments of coconut.sigreq_verify_batch after ctx, for the given requests of a call."""
    return (call["q"], call["k"], call["g"], call["hvec"], [r["commitment"] for r in reqs],
            [[be48(m) for m in r["known"]] for r in reqs], [[tuple(p) for p in r["cts"]] for r in reqs],
            [r["pk"] for r in reqs], [proof_bytes(call, r) for r in reqs], [be48(r["chal"]) for r in reqs])


def permutation(n, seed=5):
    """A fixed order of range(n) other than the identity."""
    p = list(range(n))
    random.Random(seed + n).shuffle(p)
    if p == list(range(n)) and n > 1:
        p = p[1:] + p[:1]
    return p


# ---------------------------------------------------------------- Pedersen VSS shares
VSS_T = (1, 2, 3, 5, 33)
VSS_IDS = (0, 1, 2, (1 << 32) - 1, 1 << 32, (1 << 64) - 1)
VSS_H = ("rand", "identity", "off_curve", "eq_g", "neg_g")
VSS_SIZES = (1, 64, 65, 130)


def _poly(c, x):
    return sum(a * pow(x, k, R) for k, a in enumerate(c)) % R


def vss_call(oc, t, hkind="rand"):
    """One cc_vss_verify_batch: dict(t, g, h, sets: [[C_k encodings]], cases: [dict(name, set, id, s, st
    (encoded, possibly >= r), intent, reach: [('gh' / 'C', branch)])], gk, hk, logs: [[dlog of C_k as the
    oracle decodes it]]).  The intent is the share equation in discrete logarithms."""
    _OC[id(oc)] = oc
    return _vss_call(id(oc), t, hkind)


@functools.lru_cache(maxsize=None)
def _vss_call(oc_key, t, hkind):
    env = Env(_OC[oc_key], 1)
    rng = random.Random(9000 + 10 * t + VSS_H.index(hkind))
    fr = lambda: rng.randrange(1 << 250, R)  # noqa: E731
    gk, hr = fr(), fr()
    g, hpt = env.muls([gk, hr])
    h, hk = {"rand": (hpt, hr), "identity": (env.identity, 0), "off_curve": (env.off_curve(hpt), 0),
             "eq_g": (g, gk), "neg_g": (env.neg(g), R - gk)}[hkind]
    sets, cases = [], []

    def add_set(name, coef, off=()):
        """C_k = a_k g + b_k h over the encodings sent; off: indices sent off-curve (they decode to the
        identity: the coefficient pair counts as zero)."""
        enc = [env.msm([g, h], [a, b]) for a, b in coef]
        eff = list(coef)
        for k in off:
            assert enc[k] != env.identity
            enc[k], eff[k] = env.off_curve(enc[k]), (0, 0)
        sets.append(dict(name=name, enc=enc, a=[a for a, _ in eff], b=[b for _, b in eff]))
        return len(sets) - 1

    def case(name, si, i, s, st, *reach, at=None):
        at = si if at is None else at  # the set the share is pointed at
        S = sets[at]
        lhs = (s * gk + st * hk) % R
        rhs = sum((a * gk + b * hk) * pow(i, k, R) for k, (a, b) in enumerate(zip(S["a"], S["b"]))) % R
        cases.append(dict(name=f"{sets[si]['name']}/{name}", set=at, id=i, s=s, st=st, intent=int(lhs == rhs),
                          reach=list(reach)))

    def valid(si, i):
        return _poly(sets[si]["a"], i), _poly(sets[si]["b"], i)

    rand = [(fr(), fr()) for _ in range(t)]
    rel, off = [(fr(), fr()) for _ in range(t)], ()
    if t >= 2:
        rel[1] = rel[0]
    if t >= 3:
        rel[2] = (R - rel[0][0], R - rel[0][1])
    if t >= 5:
        rel[3], off = (0, 0), (4,)
    gs = [(fr(), fr()) for _ in range(t)]
    gs[0] = (1, 0)
    if t >= 2:
        gs[1] = (R - 1, 0)
    s_rand, s_rel, s_g = add_set("rand", rand), add_set("rel", rel, off), add_set("C0_eq_g", gs)
    for si in (s_rand, s_rel, s_g):
        for i in VSS_IDS:
            case(f"valid_id_{i:x}", si, i, *valid(si, i))
    for i in (2, (1 << 64) - 1):
        s, st = valid(s_rand, i)
        case(f"s_plus_1_id_{i:x}", s_rand, i, (s + 1) % R, st)
        case(f"st_plus_1_id_{i:x}", s_rand, i, s, (st + 1) % R)
        case(f"negated_id_{i:x}", s_rand, i, (R - s) % R, (R - st) % R)
        case(f"wrongid_id_{i:x}", s_rand, 1, s, st)  # a valid share under another id
        case(f"other_set_id_{i:x}", s_rand, i, s, st, at=s_rel)
    # the C_k entries alone (share 0, 0: g and h are never added), id = 1: every id^k is 1
    sk = [("C", "skipped")] if t >= 5 else []
    case("zero_share_id_1", s_rel, 1, 0, 0, *([("C", "doubling")] if t >= 2 else []), *sk)
    case("zero_share_id_1", s_g, 1, 0, 0, *([("C", "to-identity")] if t >= 2 else []),
         *([("C", "from-identity")] if t >= 3 else []))
    # the g / h entries: id = 0 leaves C_0 alone at bit 0
    if hkind == "eq_g":
        case("gh_doubling", s_rand, 0, R - (TOP + 5), R - (TOP + 3), ("gh", "doubling"))
    elif hkind == "neg_g":
        case("gh_cancel", s_rand, 0, R - (TOP + 4), R - (TOP + 1), ("gh", "to-identity"), ("gh", "from-identity"))
    elif hkind != "rand":
        cases[0]["reach"].append(("gh", "skipped"))
    # shares at the edges of fr_from_be48 and of the negation: a set per target, a_0 and b_0 solved for it
    for nm, i, sv, stv, se, ste in (("s_zero", 1, 0, fr(), 0, None), ("st_zero", 2, fr(), 0, None, 0),
                                    ("both_zero", 1 << 32, 0, 0, 0, 0),
                                    ("r_minus_1", (1 << 64) - 1, R - 1, R - 1, R - 1, R - 1),
                                    ("r_and_r_plus_1", 1, 0, 1, R, R + 1),
                                    ("max", (1 << 32) - 1, ((1 << 384) - 1) % R, ((1 << 384) - 1) % R,
                                     (1 << 384) - 1, (1 << 384) - 1)):
        coef = [(fr(), fr()) for _ in range(t)]
        coef[0] = (0, 0)
        a0 = (sv - _poly([a for a, _ in coef], i)) % R
        b0 = (stv - _poly([b for _, b in coef], i)) % R
        coef[0] = (a0, b0)
        si = add_set(nm, coef)
        case("valid", si, i, sv if se is None else se, stv if ste is None else ste)
        assert valid(si, i) == (sv, stv)
    return dict(t=t, hkind=hkind, g=g, h=h, gk=gk, hk=hk, sets=[s["enc"] for s in sets], cases=cases)


def vss_batch(call, n, order=0):
    """n shares of a call: its cases round-robin over the sets, repeated as far as needed, the last share
    pointed at the last set; order 1: the same in a second fixed order.  Returns the case list."""
    seen, keyed = {}, []
    for c in call["cases"]:
        seen[c["set"]] = seen.get(c["set"], -1) + 1
        keyed.append((seen[c["set"]], c["set"], len(keyed)))
    cs = [call["cases"][z] for _, _, z in sorted(keyed)]
    tail = next(c for c in reversed(call["cases"]) if c["set"] == len(call["sets"]) - 1)
    head = [cs[i % len(cs)] for i in range(n - 1)]
    if order:
        head = [head[i] for i in permutation(len(head), seed=11)]
    return head + [tail]


def vss_args(call, batch):
    """The arguments of coconut.vss_verify_batch after ctx."""
    return (call["t"], call["g"], call["h"], call["sets"], [c["set"] for c in batch], [c["id"] for c in batch],
            [(be48(c["s"]), be48(c["st"])) for c in batch])


def expect_share(env, call, c):
    """verify_share's verdict from the C oracle: s g + s' h == sum id^k C_k over the encodings."""
    C = call["sets"][c["set"]]
    return int(env.msm([call["g"], call["h"]], [c["s"], c["st"]]) ==
               env.msm(C, [pow(c["id"], k, R) for k in range(call["t"])]))


def trace_share(env, call, c):
    """ladder() of one share as k_vss_verify walks it."""
    ent = [(env.dec(call["g"]), (R - c["s"] % R) % R, "gh"), (env.dec(call["h"]), (R - c["st"] % R) % R, "gh")]
    ent += [(env.dec(C), pow(c["id"], k, R), "C") for k, C in enumerate(call["sets"][c["set"]])]
    return ladder(env.curve, ent)


def python_share(env, call, c):
    """oracle/keygen.py verify_share on the decoded inputs."""
    from oracle import keygen as K
    comm = [env.dec(x) for x in call["sets"][c["set"]]]
    return int(K.verify_share(call["t"], c["id"], (c["s"] % R, c["st"] % R), comm, env.dec(call["g"]),
                              env.dec(call["h"])))


# ---------------------------------------------------------------- compute_h's input canonicalisation
def compute_h_inputs(env, q, k, rng):
    """[(name, commitment sent, known sent (encoded ints))] for cc_blind_sign_batch: every row must give the
    h, c~1, c~2 of its canonical form (the decoded commitment re-encoded, the messages mod r)."""
    fr = lambda: rng.randrange(1 << 250, R)  # noqa: E731
    kn = q - k
    jmax = lambda m: ((1 << 384) - 1 - m) // R  # noqa: E731
    rows = [("canonical", env.rand_pt(rng), [fr() for _ in range(kn)])]
    rows += [(f"commitment_{nm}", form, [fr() for _ in range(kn)]) for nm, form in env.identity_forms(rng)]
    for j in (1, "max"):
        rows.append((f"commitment_coords_plus_{j}p", env.shifted(env.rand_pt(rng), j), [fr() for _ in range(kn)]))
    m = [fr() for _ in range(kn)]
    rows.append(("known_plus_r", env.rand_pt(rng), [v + R for v in m]))
    rows.append(("known_plus_max_r", env.rand_pt(rng), [v + jmax(v) * R for v in m]))
    rows.append(("known_edges", env.rand_pt(rng), [((1 << 384) - 1, R, 0, R - 1, R + 1, 1)[j % 6] for j in range(kn)]))
    rows.append(("known_edges_rotated", env.rand_pt(rng),
                 [(R, 0, (1 << 384) - 1, 1 << 255, R - 1)[j % 5] for j in range(kn)]))
    return rows
