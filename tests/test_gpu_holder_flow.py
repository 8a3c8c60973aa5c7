"""The reference's test_PoK_sig (src/pok_sig.rs:17-106) with the holder's side on the GPU as well:
BlindSignature::unblind (cc_unblind_batch), PoKOfSignature::init / to_bytes / gen_proof
(cc_pok_init_batch, cc_pok_gen_proof_batch) and the challenge (cc_hash_msg) run through the Python API,
on top of the issuer- and verifier-side steps test_gpu_reference_flows.py already runs there.  Only
SignatureRequest::new and SignatureRequestPoK (the request and its proof) stay on the oracle."""
import pytest

from test_gpu_reference_flows import Flow, _fr, ctxs  # noqa: F401  (ctxs: the module's context fixture)

pytestmark = pytest.mark.gpu


class HolderFlow(Flow):
    def blind_signatures(self, msgs, k, signers):
        """Flow.blind_signatures with the last step on the GPU: one unblind_batch over the signers' blind
        signatures (the same ElGamal key for each)."""
        from oracle import issuance as I
        grp, P = self.grp, self.pts
        sk, pk = I.elgamal_keygen(grp, P, self.rng)
        req, rnd = I.signature_request_new(grp, msgs, k, pk, P, self.rng)
        pok = I.sigreq_pok_init(grp, req, pk, P, self.rng)
        se = grp.sig_to_bytes
        pok_bytes = se(pok["sk"]["T"]) + se(pok["comm"]["T"]) + b"".join(se(a["T"]) + se(b["T"]) for a, b in pok["cts"])
        chal = int.from_bytes(self.co.hash_msg(self.ctx, [pok_bytes])[0], "big")
        proof = I.sigreq_gen_proof(pok, msgs[:k], rnd, sk, chal)
        pb = se(proof["sk"]["T"]) + _fr(proof["sk"]["responses"][0]) + se(proof["comm"]["T"])
        pb += b"".join(_fr(v) for v in proof["comm"]["responses"])
        for p1, p2 in proof["cts"]:
            pb += se(p1["T"]) + _fr(p1["responses"][0]) + se(p2["T"]) + _fr(p2["responses"][0]) + _fr(p2["responses"][1])
        cm = se(req["commitment"])
        known = [_fr(m) for m in req["known"]]
        cts = [(se(a), se(b)) for a, b in req["ciphertexts"]]
        t = len(signers)
        v = self.co.sigreq_verify_batch(self.ctx, self.q, k, self.params.g, self.params.h, [cm] * t, [known] * t,
                                        [cts] * t, [se(pk)] * t, [pb] * t, [_fr(chal)] * t)
        assert v.all()
        hs, c1s, c2s = [], [], []
        for s in signers:
            h, c1, c2 = self.co.blind_sign_batch(self.ctx, self.q, k, [cm], [known], [cts], _fr(s["x"]),
                                                 [_fr(y) for y in s["y"]])
            hs.append(h[0])
            c1s.append(c1[0])
            c2s.append(c2[0])
        s2s = self.co.unblind_batch(self.ctx, c1s, c2s, [_fr(sk)] * t)
        return [self.co.Signature(h, s2) for h, s2 in zip(hs, s2s)]


@pytest.mark.parametrize("mode", ["G2", "G1"])
def test_PoK_sig_holder_on_gpu(ctxs, mode):  # noqa: F811
    """t = 3 of 5, q = 6, 2 hidden at issuance, messages {3, 5} revealed in the showing: the proof made by
    PoKOfSignature.init / gen_proof verifies under the aggregated verkey with the challenge hashed from
    to_bytes, and not with a changed revealed message."""
    f = HolderFlow(ctxs[mode], mode, seed=811, q=6)
    _, _, signers = f.sss_keygen(3, 5)
    msgs = [f.rng.fr() for _ in range(6)]
    sigs = f.blind_signatures(msgs, 2, signers[:3])
    f.verify_each(sigs, msgs, signers[:3])
    aggr_sig = f.co.Signature.aggregate(3, [(s["id"], sig) for s, sig in zip(signers, sigs)], ctx=f.ctx)
    aggr_vk = f.co.Verkey.aggregate(3, [(s["id"], s["vk"]) for s in signers], ctx=f.ctx)
    f.verify_aggregate(aggr_sig, msgs, aggr_vk)
    revealed = {3, 5}
    pok = f.co.PoKOfSignature.init(aggr_sig, aggr_vk, f.params, msgs, revealed=revealed, ctx=f.ctx)
    tb = pok.to_bytes()
    assert len(tb) == 2 * f.sb + f.ob * (2 + 1 + 4)  # sigma', J, [g~, four hidden Y~], T
    chal = int.from_bytes(f.co.hash_msg(f.ctx, [tb])[0], "big")
    assert f.co.pok_challenge_batch(f.ctx, 1, 6, sorted(revealed), f.params.g_tilde, aggr_vk.Y_tilde, pok.sigma_1,
                                    pok.sigma_2, pok.J, pok.commitment) == chal.to_bytes(48, "big")
    proof = pok.gen_proof(chal)
    assert len(proof.responses) == 5
    rev = {i: msgs[i] for i in revealed}
    assert proof.verify(aggr_vk, f.params, rev, chal, ctx=f.ctx)
    rev[5] += 1
    assert not proof.verify(aggr_vk, f.params, rev, chal, ctx=f.ctx)
    # a second showing of the same credential is a different proof (fresh r1, r2, blindings)
    again = f.co.PoKOfSignature.init(aggr_sig, aggr_vk, f.params, msgs, revealed=revealed, ctx=f.ctx)
    assert again.sigma_1 != pok.sigma_1 and again.commitment != pok.commitment
