"""Keygen — host mirror of reference src/keygen.rs: trusted_party_SSS_keygen (53-71),
trusted_party_PVSS_keygen (74-122) with keygen_from_shares (17-45), and the final sums of the decentralized
keygen (124-205), for whole batches of keygens through include/coconut_hip.h (cc_keygen_deal_batch,
cc_keygen_combine_batch).  The polynomials are the caller's, or drawn here from the OS generator."""
from __future__ import annotations

import ctypes
import secrets
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from ._lib import buf, check, lib, need
from .issuance import _dev_need, _dev_ptr, _fresh_scalars, _stream_ptr
from .signature import Context, Params, Verkey


@dataclass
class Sigkey:
    """signature.rs:40-43."""
    x: bytes
    y: List[bytes]


@dataclass
class Signer:
    """keygen.rs:10-14."""
    id: int
    sigkey: Sigkey
    verkey: Verkey


def _out(nbytes: int):
    return np.zeros(max(nbytes, 1), dtype=np.uint8)


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _sizes(ctx: Context, m: int, q: int, t: int, total: int):
    """Bytes of x, y, xt, yt, comm, X, Y for m keygens."""
    ob = ctx.mode.other_bytes
    return (m * total * 48, m * total * q * 48, m * total * 48, m * total * q * 48, m * (q + 1) * t * 97,
            m * total * ob, m * total * q * ob)


def keygen_deal_batch(ctx: Context, m: int, q: int, t: int, total: int, coeffs: bytes,
                      coeffs_t: Optional[bytes] = None):
    """m trusted-party keygens under the context's keygen params (Context.set_keygen_params;
    cc_keygen_deal_batch).  coeffs m x (q + 1) x t x 48: polynomial 0 shares x, 1 + j shares y_j, coefficient
    0 is the secret; coeffs_t the blinding polynomials in the same layout (None: Shamir).
    Returns (x, y, xt, yt, comm, X, Y) as bytes in the header's layouts; xt, yt and comm are None for Shamir."""
    cb = m * (q + 1) * t * 48
    need(coeffs, cb, "coefficients")
    ped = coeffs_t is not None
    if ped:
        need(coeffs_t, cb, "blinding coefficients")
    sizes = _sizes(ctx, m, q, t, total)
    outs = [_out(s) if (ped or i not in (2, 3, 4)) else None for i, s in enumerate(sizes)]
    keep = [buf(coeffs), buf(coeffs_t)]
    check(lib.cc_keygen_deal_batch(ctx.h, m, q, t, total, keep[0][0], keep[1][0], *[_ptr(o) for o in outs]),
          "cc_keygen_deal_batch")
    return tuple(None if o is None else o.tobytes()[:s] for o, s in zip(outs, sizes))


def keygen_combine_batch(ctx: Context, m: int, d: int, q: int, t: int, total: int, x: bytes, y: bytes,
                         xt: Optional[bytes] = None, yt: Optional[bytes] = None, comm: Optional[bytes] = None):
    """The decentralized keygen's last step for m groups of d dealers (cc_keygen_combine_batch): the inputs
    are the outputs of keygen_deal_batch with m x d keygens; every output is the sum over a group's dealers.
    Returns (x, y, xt, yt, comm, X, Y); xt, yt and comm are None unless the three inputs are given."""
    ped = xt is not None or yt is not None or comm is not None
    sizes = _sizes(ctx, m, q, t, total)
    ins = (x, y, xt, yt, comm)
    for v, s, what in zip(ins, sizes, ("x shares", "y shares", "x blinding shares", "y blinding shares",
                                        "commitments")):
        if ped or what in ("x shares", "y shares"):
            need(v, d * s, what)
    outs = [_out(s) if (ped or i not in (2, 3, 4)) else None for i, s in enumerate(sizes)]
    keep = [buf(v) for v in ins]
    check(lib.cc_keygen_combine_batch(ctx.h, m, d, q, t, total, *[k[0] for k in keep], *[_ptr(o) for o in outs]),
          "cc_keygen_combine_batch")
    return tuple(None if o is None else o.tobytes()[:s] for o, s in zip(outs, sizes))


def keygen_deal_batch_device(ctx: Context, m: int, q: int, t: int, total: int, coeffs, coeffs_t=None, stream=None):
    """keygen_deal_batch with the coefficients in HBM (cc_keygen_deal_batch_device): torch.uint8 CUDA tensors
    in, the tensors (x, y, xt, yt, comm, X, Y) out (xt, yt, comm None for Shamir).  Asynchronous on `stream`
    (a torch.cuda.Stream; None: the context's)."""
    import torch
    cb = m * (q + 1) * t * 48
    ped = coeffs_t is not None
    _dev_need(((coeffs, cb, "coefficients"), (coeffs_t, cb if ped else 0, "blinding coefficients")))
    dev = coeffs.device if m else None
    outs = [torch.empty(s, dtype=torch.uint8, device=dev) if (ped or i not in (2, 3, 4)) else None
            for i, s in enumerate(_sizes(ctx, m, q, t, total))]
    check(lib.cc_keygen_deal_batch_device(ctx.h, m, q, t, total, _dev_ptr(coeffs), _dev_ptr(coeffs_t),
                                          *[_dev_ptr(o) for o in outs], _stream_ptr(stream)),
          "cc_keygen_deal_batch_device")
    return tuple(outs)


def keygen_combine_batch_device(ctx: Context, m: int, d: int, q: int, t: int, total: int, x, y, xt=None, yt=None,
                                comm=None, stream=None):
    """keygen_combine_batch on tensors in HBM (cc_keygen_combine_batch_device), the outputs of
    keygen_deal_batch_device with m x d keygens.  Returns the tensors (x, y, xt, yt, comm, X, Y)."""
    import torch
    ped = xt is not None or yt is not None or comm is not None
    sizes = _sizes(ctx, m, q, t, total)
    _dev_need([(v, d * s if (ped or i < 2) else 0, what) for i, (v, s, what) in enumerate(zip(
        (x, y, xt, yt, comm), sizes, ("x shares", "y shares", "x blinding shares", "y blinding shares",
                                      "commitments")))])
    dev = x.device if m else None
    outs = [torch.empty(s, dtype=torch.uint8, device=dev) if (ped or i not in (2, 3, 4)) else None
            for i, s in enumerate(sizes)]
    check(lib.cc_keygen_combine_batch_device(ctx.h, m, d, q, t, total, *[_dev_ptr(v) for v in (x, y, xt, yt, comm)],
                                             *[_dev_ptr(o) for o in outs], _stream_ptr(stream)),
          "cc_keygen_combine_batch_device")
    return tuple(outs)


def keygen_verify_shares_device(ctx: Context, m: int, q: int, t: int, total: int, x, y, xt, yt, comm,
                                rlc: bool = False, seed: Optional[bytes] = None, stream=None):
    """PedersenVSS::verify_share for every share of m keygens, read in place from the tensors
    keygen_deal_batch_device / keygen_combine_batch_device returned (cc_keygen_verify_shares_batch_device).
    Verdict (keygen (q + 1) + p) total + signer belongs to polynomial p (0: x, 1 + j: y_j) and signer index
    0 .. total - 1.  rlc: one random-linear-combination check a (keygen, polynomial) first, keyed by `seed` (32
    bytes; None: drawn here).  The call synchronises `stream` once.  Returns (verdict tensor, stats) with
    stats = (sets, sets the RLC check rejected, irregular sets, shares verified per share)."""
    import torch
    sx, sy, _, _, sc, _, _ = _sizes(ctx, m, q, t, total)
    _dev_need(((x, sx, "x shares"), (y, sy, "y shares"), (xt, sx, "x blinding shares"),
               (yt, sy, "y blinding shares"), (comm, sc, "commitments")))
    if rlc and seed is None:
        seed = secrets.token_bytes(32)
    if seed is not None:
        need(seed, 32, "seed")
    keep = buf(bytes(seed)) if seed is not None else (None, None)
    n = m * (q + 1) * total
    v = torch.empty(n, dtype=torch.uint8, device=x.device if n else None)
    st = np.zeros(4, dtype=np.uint32)
    check(lib.cc_keygen_verify_shares_batch_device(ctx.h, m, q, t, total, *[_dev_ptr(a) for a in (x, y, xt, yt, comm)],
                                                   1 if rlc else 0, keep[0], _dev_ptr(v),
                                                   ctypes.c_void_p(st.ctypes.data), _stream_ptr(stream)),
          "cc_keygen_verify_shares_batch_device")
    return v, tuple(int(s) for s in st)


def _signers(ctx: Context, q: int, total: int, x: bytes, y: bytes, X: bytes, Y: bytes) -> List[Signer]:
    """keygen_from_shares' result for one keygen's slices."""
    ob = ctx.mode.other_bytes
    out = []
    for i in range(total):
        ys = [y[(i * q + j) * 48:(i * q + j + 1) * 48] for j in range(q)]
        Ys = [Y[(i * q + j) * ob:(i * q + j + 1) * ob] for j in range(q)]
        out.append(Signer(i + 1, Sigkey(x[i * 48:(i + 1) * 48], ys), Verkey(X[i * ob:(i + 1) * ob], Ys)))
    return out


def _secrets(coeffs: bytes, q: int, t: int):
    """Coefficient 0 of every polynomial: (secret of polynomial 0, [secrets of polynomials 1 .. q])."""
    s = [coeffs[p * t * 48:p * t * 48 + 48] for p in range(q + 1)]
    return s[0], s[1:]


def trusted_party_SSS_keygen(threshold: int, total: int, params: Params, ctx: Context = None,
                             coeffs: Optional[bytes] = None):
    """keygen.rs:53-71: (secret_x, secret_y, signers).  coeffs fixes the (q + 1) x threshold coefficients."""
    ctx = ctx or Context.default()
    q = params.msg_count()
    if coeffs is None:
        coeffs = _fresh_scalars((q + 1) * threshold)
    ctx.set_keygen_params(params.g_tilde)
    x, y, _, _, _, X, Y = keygen_deal_batch(ctx, 1, q, threshold, total, coeffs)
    sx, sy = _secrets(coeffs, q, threshold)
    return sx, sy, _signers(ctx, q, total, x, y, X, Y)


def trusted_party_PVSS_keygen(threshold: int, total: int, params: Params, g: bytes, h: bytes, ctx: Context = None,
                              coeffs: Optional[bytes] = None, coeffs_t: Optional[bytes] = None):
    """keygen.rs:74-122, the reference's eleven values in its order: secret_x, secret_y, signers, secret_x_t,
    comm_coeff_x, x_shares, x_t_shares, secret_y_t, comm_coeff_y, y_shares, y_t_shares.  The share maps are
    keyed by signer id (1 .. total), the commitment maps by coefficient index (0 .. threshold - 1)."""
    ctx = ctx or Context.default()
    q, t = params.msg_count(), threshold
    if coeffs is None:
        coeffs = _fresh_scalars((q + 1) * t)
    if coeffs_t is None:
        coeffs_t = _fresh_scalars((q + 1) * t)
    ctx.set_keygen_params(params.g_tilde, g, h)
    x, y, xt, yt, comm, X, Y = keygen_deal_batch(ctx, 1, q, t, total, coeffs, coeffs_t)
    sx, sy = _secrets(coeffs, q, t)
    sxt, syt = _secrets(coeffs_t, q, t)
    cm = lambda p: {i: comm[(p * t + i) * 97:(p * t + i + 1) * 97] for i in range(t)}  # noqa: E731
    xs = lambda b: {i + 1: b[i * 48:(i + 1) * 48] for i in range(total)}  # noqa: E731
    ys = lambda b, j: {i + 1: b[(i * q + j) * 48:(i * q + j + 1) * 48] for i in range(total)}  # noqa: E731
    return (sx, sy, _signers(ctx, q, total, x, y, X, Y), sxt, cm(0), xs(x), xs(xt), syt,
            [cm(1 + j) for j in range(q)], [ys(y, j) for j in range(q)], [ys(yt, j) for j in range(q)])
