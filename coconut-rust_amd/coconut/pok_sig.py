"""PoKOfSignature::init / gen_proof and PoKOfSignatureProof::verify — host mirror of the ps_sig 0.1.2 API [EXT] the reference exercises
in src/pok_sig.rs:85-105 (`proof.verify(&ps_verkey, &ps_params, revealed_msgs, &chal)`).

Responses are ordered as ps_sig builds them: [r2 for g~, m_i for each hidden i ascending]
(pok_sig init bases g~, Y~_hidden).  The revealed map is keyed by message index; iteration order
does not matter (the sum is order-independent), so indices are sorted here.
"""
from __future__ import annotations

import ctypes
import secrets
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Union

import numpy as np

from ._lib import buf, check, lib, need
from .errors import CoconutError
from .signature import GT_BYTES, R_ORDER, Context, Params, Signature, Verkey, fr_bytes, hash_msg


@dataclass
class PoKOfSignatureProof:
    sigma_1: bytes          # sigma'_1 (SignatureGroup)
    sigma_2: bytes          # sigma'_2
    J: bytes                # OtherGroup
    commitment: bytes       # Schnorr commitment T (OtherGroup)
    responses: List[bytes]  # 48-byte Fr each

    def verify(self, vk: Verkey, params: Params, revealed_msgs: Dict[int, Union[int, bytes]],
               chal: Union[int, bytes], ctx: Context = None) -> bool:
        ctx = ctx or Context.default()
        ctx.set_params(params.g_tilde)
        ctx.set_verkey(vk.X_tilde, vk.Y_tilde)
        idx = sorted(revealed_msgs)
        v = pok_verify_batch(ctx, 1, len(vk.Y_tilde), idx, len(self.responses), self.sigma_1, self.sigma_2,
                             self.J, self.commitment, b"".join(self.responses), fr_bytes(chal),
                             b"".join(fr_bytes(revealed_msgs[i]) for i in idx))
        return bool(v[0])


def pok_verify_batch(ctx: Context, n: int, q: int, revealed_idx, nresp: int, sigma1: bytes, sigma2: bytes,
                     J: bytes, T: bytes, responses: bytes, chal: bytes, revealed_msgs: bytes,
                     want_gt: bool = False, rlc: bool = False, vk=None):
    """Batch PoK verify against the context's params and shared verkey.

    vk=(X_bytes, Y_bytes) checks proof i against ITS OWN verkey instead (cc_pok_verify_batch_pervk):
    X_bytes n x OtherGroup, Y_bytes n x q x OtherGroup.  The context then needs its params only, and
    revealed_idx may be in any order (revealed_msgs follow it).  There is no RLC form of it.

    rlc=True checks the whole batch with one random-linear-combination pairing product first
    (cc_pok_verify_batch_rlc) and falls back to the per-proof path on reject, so the verdicts are the
    same; it has no GT output."""
    if rlc and want_gt:
        raise ValueError("rlc=True has no per-proof GT output (want_gt=True)")
    if rlc and vk is not None:
        raise ValueError("rlc=True needs the shared verkey (vk=None)")
    r = len(revealed_idx)
    sb, ob = ctx.mode.sig_bytes, ctx.mode.other_bytes
    for v, nb, what in ((sigma1, n * sb, "sigma'_1"), (sigma2, n * sb, "sigma'_2"), (J, n * ob, "J"),
                        (T, n * ob, "commitment"), (responses, n * nresp * 48, "responses"),
                        (chal, n * 48, "challenges"), (revealed_msgs, n * r * 48, "revealed messages")):
        need(v, nb, what)
    if vk is not None:
        vk_X, vk_Y = vk
        need(vk_X, n * ob, "verkey X~ (one per proof)")
        need(vk_Y, n * q * ob, "verkey Y~ (q per proof)")
    idx = np.ascontiguousarray(np.asarray(revealed_idx, dtype=np.uint64)) if r else np.zeros(1, np.uint64)
    verdicts = np.zeros(max(n, 1), dtype=np.uint8)
    gts = np.zeros(max(n, 1) * GT_BYTES, dtype=np.uint8) if want_gt else None
    keep = [buf(x) for x in (sigma1, sigma2, J, T, responses, chal, revealed_msgs)]
    ptrs = [k[0] for k in keep]
    if vk is not None:
        kv = [buf(x) for x in (vk_X, vk_Y)]
        st = lib.cc_pok_verify_batch_pervk(ctx.h, n, q, r, nresp, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5],
                                           ctypes.c_void_p(idx.ctypes.data), ptrs[6], kv[0][0], kv[1][0],
                                           ctypes.c_void_p(verdicts.ctypes.data),
                                           ctypes.c_void_p(gts.ctypes.data) if want_gt else None)
    elif rlc:
        st = lib.cc_pok_verify_batch_rlc(ctx.h, n, q, r, nresp, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5],
                                         ctypes.c_void_p(idx.ctypes.data), ptrs[6],
                                         ctypes.c_void_p(verdicts.ctypes.data))
    else:
        st = lib.cc_pok_verify_batch(ctx.h, n, q, r, nresp, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5],
                                     ctypes.c_void_p(idx.ctypes.data), ptrs[6], ctypes.c_void_p(verdicts.ctypes.data),
                                     ctypes.c_void_p(gts.ctypes.data) if want_gt else None)
    if st != 0:
        raise CoconutError(st, lib.cc_status_str(st).decode())
    if want_gt:
        return verdicts[:n], gts[:n * GT_BYTES].tobytes()
    return verdicts[:n]


def pok_verify_batch_locate(ctx: Context, n: int, q: int, revealed_idx, nresp: int, sigma1: bytes, sigma2: bytes,
                            J: bytes, T: bytes, responses: bytes, chal: bytes, revealed_msgs: bytes, seg: int = 0):
    """Batch PoK verify through the RLC locate mode (cc_pok_verify_batch_locate; shared verkey): the batch is
    checked in segments of `seg` proofs (a power of two >= 4; 0: the library's default) and only the rejected
    segments are verified per proof.  Returns (verdicts uint8[n], stats) with stats = (segments, rejected
    segments, proofs rechecked); the verdicts equal pok_verify_batch's."""
    r = len(revealed_idx)
    sb, ob = ctx.mode.sig_bytes, ctx.mode.other_bytes
    for v, nb, what in ((sigma1, n * sb, "sigma'_1"), (sigma2, n * sb, "sigma'_2"), (J, n * ob, "J"),
                        (T, n * ob, "commitment"), (responses, n * nresp * 48, "responses"),
                        (chal, n * 48, "challenges"), (revealed_msgs, n * r * 48, "revealed messages")):
        need(v, nb, what)
    idx = np.ascontiguousarray(np.asarray(revealed_idx, dtype=np.uint64)) if r else np.zeros(1, np.uint64)
    verdicts = np.zeros(max(n, 1), dtype=np.uint8)
    stats = np.zeros(3, dtype=np.uint32)
    keep = [buf(x) for x in (sigma1, sigma2, J, T, responses, chal, revealed_msgs)]
    ptrs = [k[0] for k in keep]
    check(lib.cc_pok_verify_batch_locate(ctx.h, n, q, r, nresp, seg, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4],
                                         ptrs[5], ctypes.c_void_p(idx.ctypes.data), ptrs[6],
                                         ctypes.c_void_p(verdicts.ctypes.data), ctypes.c_void_p(stats.ctypes.data)),
          "cc_pok_verify_batch_locate")
    return verdicts[:n], tuple(int(x) for x in stats)


def _fresh_scalars(count: int) -> bytes:
    """count scalars from the OS generator: 48 random bytes each, reduced mod r (bias < 2^-128)."""
    return b"".join((int.from_bytes(secrets.token_bytes(48), "big") % R_ORDER).to_bytes(48, "big")
                    for _ in range(count))


def _idx_array(revealed_idx):
    r = len(revealed_idx)
    return np.ascontiguousarray(np.asarray(revealed_idx, dtype=np.uint64)) if r else np.zeros(1, np.uint64)


def pok_init_batch(ctx: Context, n: int, q: int, revealed_idx, sigma1: bytes, sigma2: bytes, msgs: bytes,
                   rand: Optional[bytes] = None):
    """PoKOfSignature::init for n credentials under the context's params and shared verkey
    (cc_pok_init_batch).  rand: n x (q - r + 3) x 48 B = r1 | r2 | b_0 .. per credential (b_0 blinds r2,
    b_{1+j} the j-th hidden message, ascending index); None draws it from `secrets`.
    Returns (sigma'_1, sigma'_2, J, T, rand): four byte strings of n encodings and the randomness
    gen_proof needs."""
    r = len(revealed_idx)
    nresp = q - r + 1
    sb, ob = ctx.mode.sig_bytes, ctx.mode.other_bytes
    if rand is None:
        rand = _fresh_scalars(n * max(nresp + 2, 0))
    for v, nb, what in ((sigma1, n * sb, "sigma_1"), (sigma2, n * sb, "sigma_2"), (msgs, n * q * 48, "messages"),
                        (rand, n * (nresp + 2) * 48, "randomness")):
        need(v, nb, what)
    idx = _idx_array(revealed_idx)
    outs = [np.zeros(max(n, 1) * w, dtype=np.uint8) for w in (sb, sb, ob, ob)]
    keep = [buf(x) for x in (sigma1, sigma2, msgs, rand)]
    check(lib.cc_pok_init_batch(ctx.h, n, q, r, nresp, keep[0][0], keep[1][0], keep[2][0],
                                ctypes.c_void_p(idx.ctypes.data), keep[3][0],
                                *[ctypes.c_void_p(o.ctypes.data) for o in outs]), "cc_pok_init_batch")
    s1, s2, J, T = (o.tobytes()[:n * w] for o, w in zip(outs, (sb, sb, ob, ob)))
    return s1, s2, J, T, bytes(rand)


def pok_gen_proof_batch(ctx: Context, n: int, q: int, revealed_idx, msgs: bytes, rand: bytes, chal: bytes) -> bytes:
    """gen_proof for n committed proofs (cc_pok_gen_proof_batch): n x (q - r + 1) responses of 48 B,
    responses[0] = b_0 - chal r2, responses[1 + j] = b_{1+j} - chal m_hidden_j."""
    r = len(revealed_idx)
    nresp = q - r + 1
    for v, nb, what in ((msgs, n * q * 48, "messages"), (rand, n * (nresp + 2) * 48, "randomness"),
                        (chal, n * 48, "challenges")):
        need(v, nb, what)
    idx = _idx_array(revealed_idx)
    out = np.zeros(max(n * max(nresp, 0), 1) * 48, dtype=np.uint8)
    keep = [buf(x) for x in (msgs, rand, chal)]
    check(lib.cc_pok_gen_proof_batch(ctx.h, n, q, r, nresp, keep[0][0], ctypes.c_void_p(idx.ctypes.data), keep[1][0],
                                     keep[2][0], ctypes.c_void_p(out.ctypes.data)), "cc_pok_gen_proof_batch")
    return out.tobytes()[:n * nresp * 48]


def pok_to_bytes_batch(ctx: Context, n: int, q: int, revealed_idx, g_tilde: bytes, Y: Sequence[bytes], sigma1: bytes,
                       sigma2: bytes, J: bytes, T: bytes) -> List[bytes]:
    """PoKOfSignature::to_bytes per proof: sigma'_1 || sigma'_2 || J || g~ || Y~_hidden.. || T."""
    sb, ob = ctx.mode.sig_bytes, ctx.mode.other_bytes
    for v, nb, what in ((sigma1, n * sb, "sigma'_1"), (sigma2, n * sb, "sigma'_2"), (J, n * ob, "J"),
                        (T, n * ob, "commitment")):
        need(v, nb, what)
    hidden = set(int(i) for i in revealed_idx)
    bases = bytes(g_tilde) + b"".join(bytes(Y[i]) for i in range(q) if i not in hidden)
    return [sigma1[i * sb:(i + 1) * sb] + sigma2[i * sb:(i + 1) * sb] + J[i * ob:(i + 1) * ob] + bases +
            T[i * ob:(i + 1) * ob] for i in range(n)]


def pok_challenge_batch(ctx: Context, n: int, q: int, revealed_idx, g_tilde: bytes, Y: Sequence[bytes],
                        sigma1: bytes, sigma2: bytes, J: bytes, T: bytes) -> bytes:
    """The reference's challenge (src/pok_sig.rs:94: FieldElement::from_msg_hash(&pok.to_bytes())) for n
    committed proofs: the to_bytes rows through hash_msg on the GPU; n x 48 B."""
    return b"".join(hash_msg(ctx, pok_to_bytes_batch(ctx, n, q, revealed_idx, g_tilde, Y, sigma1, sigma2, J, T)))


@dataclass
class PoKOfSignature:
    """ps_sig PoKOfSignature [EXT] (reference src/pok_sig.rs:80-100): the committed state between init
    and gen_proof."""
    sigma_1: bytes           # sigma'_1
    sigma_2: bytes           # sigma'_2
    J: bytes
    commitment: bytes        # T
    bases: List[bytes]       # g~, Y~_i for hidden i ascending
    revealed: List[int]
    msgs: bytes              # the q messages (48 B each)
    rand: bytes              # r1 | r2 | b_0 .. (secret)
    ctx: Context = None

    @staticmethod
    def init(sig: Signature, vk: Verkey, params: Params, msgs: Sequence[Union[int, bytes]],
             blindings: Optional[Sequence[Union[int, bytes]]] = None, revealed=(), ctx: Context = None,
             rand: Optional[Sequence[Union[int, bytes]]] = None) -> "PoKOfSignature":
        """blindings: one per hidden message (ascending index), as ps_sig takes them; the rest (r1, r2
        and r2's blinding) is drawn from `secrets`.  rand = [r1, r2, b_0, b_1 ..] fixes every draw
        (replaying a recorded proof)."""
        ctx = ctx or Context.default()
        q = len(vk.Y_tilde)
        if len(msgs) != q:
            raise CoconutError(-1, f"Verkey valid for {q} messages but given {len(msgs)}")
        idx = sorted(set(int(i) for i in revealed))
        hidden = q - len(idx)
        if rand is not None:
            if len(rand) != hidden + 3:
                raise CoconutError(-2, f"rand holds {len(rand)} scalars, init draws {hidden + 3}")
            rb = b"".join(fr_bytes(x) for x in rand)
        else:
            if blindings is not None and len(blindings) != hidden:
                raise CoconutError(-2, f"{len(blindings)} blindings for {hidden} hidden messages")
            rb = _fresh_scalars(3) + (b"".join(fr_bytes(b) for b in blindings) if blindings is not None
                                      else _fresh_scalars(hidden))
        ctx.set_params(params.g_tilde)
        ctx.set_verkey(vk.X_tilde, vk.Y_tilde)
        mb = b"".join(fr_bytes(m) for m in msgs)
        s1, s2, J, T, rb = pok_init_batch(ctx, 1, q, idx, sig.sigma_1, sig.sigma_2, mb, rb)
        rev = set(idx)
        bases = [bytes(params.g_tilde)] + [bytes(vk.Y_tilde[i]) for i in range(q) if i not in rev]
        return PoKOfSignature(s1, s2, J, T, bases, idx, mb, rb, ctx)

    def to_bytes(self) -> bytes:
        return self.sigma_1 + self.sigma_2 + self.J + b"".join(self.bases) + self.commitment

    def gen_proof(self, chal: Union[int, bytes]) -> PoKOfSignatureProof:
        ctx = self.ctx or Context.default()
        q = len(self.msgs) // 48
        resp = pok_gen_proof_batch(ctx, 1, q, self.revealed, self.msgs, self.rand, fr_bytes(chal))
        return PoKOfSignatureProof(self.sigma_1, self.sigma_2, self.J, self.commitment,
                                   [resp[k:k + 48] for k in range(0, len(resp), 48)])
