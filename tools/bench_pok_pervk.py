"""PoKOfSignatureProof::verify with one verkey per proof (cc_pok_verify_batch_pervk_device) against the only
route a caller had for distinct verkeys before it, in one process on one context, inputs resident in HBM
(by default 65,536 proofs, q = 32, 8 revealed, every proof under its own verkey, 1/16 corrupted):

  N  cc_pok_verify_batch_pervk_device on the whole batch
  P  the earlier route on a sample of the same proofs: per proof one cc_set_verkey (8-bit tables, the
     cheapest to build) and one cc_pok_verify_batch_device call of size 1
  S  reference point: cc_pok_verify_batch_device on a shared-verkey batch of the same shape
  V  reference point: cc_verify_batch_pervk_device (Signature::verify, one verkey per credential) at the same q,
     on credentials under the verkeys of N

One batch in flight, alternating blocks (N P S V N P S V ...) after a warm-up of each; each call is timed
with a host clock around a stream synchronise.  Before anything is printed every path's verdicts are
checked against construction.  One JSON line: the rates, their spread over blocks, N's phase times from
cc_last_timing (prep, Miller, final exponentiation), the latency of N on one proof, and N / P (which must
exceed 1).

    python tools/bench_pok_pervk.py [--g1] [--n 65536] [--q 32] [--sample 256] [--blocks 3] [--reps 3]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "coconut-rust_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))  # pok_pervk_cases: the distinct-verkey batch builder


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g1", action="store_true", help="SigG1 (signatures in G1, the verkeys in G2)")
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--q", type=int, default=32)
    ap.add_argument("--sample", type=int, default=256, help="proofs of the earlier route per timed call")
    ap.add_argument("--blocks", type=int, default=3, help="timed blocks of each path (at least 3)")
    ap.add_argument("--reps", type=int, default=3, help="calls per block (the earlier route: one)")
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if args.blocks < 3:
        ap.error("--blocks must be at least 3")
    import numpy as np
    import torch
    import coconut
    import pok_pervk_cases as C
    from bench_modes import REVEALED, R, make_pok_batch
    lib = coconut._lib.lib
    mode = 1 if args.g1 else 0
    og, sg = C.groups(mode)
    ob, sb = (97, 192) if mode == 0 else (192, 97)
    dev = torch.device("cuda", 0)
    ctx = coconut.Context(0, coconut.GroupMode(mode))
    revealed = [i for i in REVEALED if i < args.q]
    n, q, r = args.n, args.q, len(revealed)
    ns = min(args.sample, n)
    mul = C.gpu_mul(ctx)
    b = C.distinct_batch(mul, mode, n, q, revealed, seed=5, bad_every=16)
    nresp = b["nresp"]
    ctx.set_params(b["g"])
    # V's credentials under the same verkeys: sigma = (k G, k (x + sum y_j m_j) G), 1/16 with sigma_2 off by G
    rng = np.random.default_rng(6)
    fr = lambda: int.from_bytes(rng.bytes(32), "big") % R  # noqa: E731
    e1, e2, mb, vexp = [], [], [], np.ones(n, np.uint8)
    for i, key in enumerate(b["keys"]):
        m = [fr() for _ in range(q)]
        k = fr() or 1
        bad = i % 16 == 15
        vexp[i] = not bad
        e1.append(k)
        e2.append(k * (key[0] + sum(y * mm for y, mm in zip(key[1:], m))) + bad)
        mb.append(b"".join(C.be48(v) for v in m))
    cred = dict(s1=mul(sg, e1), s2=mul(sg, e2), msgs=b"".join(mb))
    # S's batch: the same shape under one verkey (a context holds one g~: S rebinds the params)
    s = make_pok_batch(ctx, mode, n, q=q, revealed=revealed, seed=5, bad_every=16)
    to = lambda x: torch.frombuffer(bytearray(x + b"\0"), dtype=torch.uint8).to(dev)  # noqa: E731
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    keys = ("s1", "s2", "J", "T", "resp", "chal", "rev")
    D = {k: to(b[k]) for k in keys + ("X", "Y")}
    S = {k: to(s[k]) for k in keys}
    V = {k: to(cred[k]) for k in ("s1", "s2", "msgs")}
    idx = (ctypes.c_uint64 * max(r, 1))(*revealed)
    out = {k: torch.zeros(n, dtype=torch.uint8, device=dev) for k in "NPSV"}
    stream = torch.cuda.Stream(dev)
    sh = ctypes.c_void_p(stream.cuda_stream)
    torch.cuda.synchronize(dev)

    def ck(st, what):
        if st != 0:
            raise RuntimeError(f"{what}: {lib.cc_status_str(st).decode()}")

    def bind_b():  # untimed: the params (and, for P, the table width) a path runs under
        ctx.set_table_bits(0, 0)
        ctx.set_params(b["g"])

    def bind_p():
        ctx.set_table_bits(8, 0)
        ctx.set_params(b["g"])

    def bind_s():
        ctx.set_table_bits(0, 0)
        ctx.set_params(s["g_tilde"])
        ctx.set_verkey(s["X"], s["Y"])

    def run_n():
        ck(lib.cc_pok_verify_batch_pervk_device(ctx.h, n, q, r, nresp, *[P(D[k]) for k in keys[:6]], idx, P(D["rev"]),
                                                P(D["X"]), P(D["Y"]), P(out["N"]), None, sh),
           "cc_pok_verify_batch_pervk_device")

    item = {"s1": sb, "s2": sb, "J": ob, "T": ob, "resp": nresp * 48, "chal": 48, "rev": r * 48}

    def run_p():
        for i in range(ns):
            ctx.set_verkey(b["X"][i * ob:(i + 1) * ob], b["Y"][i * q * ob:(i + 1) * q * ob])
            a = [ctypes.c_void_p(D[k].data_ptr() + i * item[k]) for k in keys]
            ck(lib.cc_pok_verify_batch_device(ctx.h, 1, q, r, nresp, *a[:6], idx, a[6],
                                              ctypes.c_void_p(out["P"].data_ptr() + i), None, sh),
               "cc_pok_verify_batch_device (one proof)")

    def run_s():
        ck(lib.cc_pok_verify_batch_device(ctx.h, n, q, r, nresp, *[P(S[k]) for k in keys[:6]], idx, P(S["rev"]),
                                          P(out["S"]), None, sh), "cc_pok_verify_batch_device")

    def run_v():
        ck(lib.cc_verify_batch_pervk_device(ctx.h, n, q, P(V["s1"]), P(V["s2"]), P(V["msgs"]), P(D["X"]), P(D["Y"]),
                                            P(out["V"]), None, sh), "cc_verify_batch_pervk_device")

    def timed(f, bind=None):
        if bind:
            bind()
            torch.cuda.synchronize(dev)
        stream.synchronize()
        t0 = time.perf_counter()
        f()
        stream.synchronize()
        return time.perf_counter() - t0

    paths = (("N", run_n, bind_b, n, args.reps), ("P", run_p, bind_p, ns, 1), ("S", run_s, bind_s, n, args.reps),
             ("V", run_v, bind_b, n, args.reps))
    for _ in range(args.warmup):
        for _, f, bind, _, _ in paths:
            timed(f, bind)

    def gate():
        want = {"N": np.asarray(b["expect"], np.uint8), "P": np.asarray(b["expect"][:ns], np.uint8),
                "S": np.asarray(s["expect"], np.uint8), "V": vexp}
        for k, w in want.items():
            got = out[k].cpu().numpy()[:len(w)]
            if not np.array_equal(got, w):
                raise SystemExit(f"path {k}: {int((got != w).sum())} verdicts differ from construction")

    gate()
    ctx.timing(True)
    timed(run_n, bind_b)
    phases = ctx.last_timing()
    ctx.timing(False)
    blocks = {k: [] for k, _, _, _, _ in paths}
    for _ in range(args.blocks):
        for k, f, bind, cnt, reps in paths:
            first = timed(f, bind)  # (binding is outside the clock)
            blocks[k].append(cnt / statistics.median([first] + [timed(f) for _ in range(reps - 1)]))
    gate()
    # single-call latency of the new entry point (recorded, not a goal: one prep path serves every n)
    one = torch.zeros(1, dtype=torch.uint8, device=dev)

    def run_1():
        ck(lib.cc_pok_verify_batch_pervk_device(ctx.h, 1, q, r, nresp, *[P(D[k]) for k in keys[:6]], idx, P(D["rev"]),
                                                P(D["X"]), P(D["Y"]), P(one), None, sh),
           "cc_pok_verify_batch_pervk_device (one proof)")

    timed(run_1, bind_b)
    single_ms = statistics.median([timed(run_1) for _ in range(20)]) * 1e3
    if int(one.item()) != b["expect"][0]:
        raise SystemExit("the single-proof call's verdict differs from construction")
    rate = {k: statistics.median(v) for k, v in blocks.items()}
    spread = {k: (max(v) - min(v)) / statistics.median(v) for k, v in blocks.items()}
    if rate["N"] <= rate["P"]:
        raise SystemExit(f"the new call ({rate['N']:.1f}/s) does not beat the earlier route ({rate['P']:.1f}/s)")
    res = {
        "tool": "bench_pok_pervk", "mode": "SigG1" if mode else "SigG2", "n": n, "q": q, "revealed": r, "sample": ns,
        "blocks": args.blocks, "reps": args.reps, "version": coconut.version(),
        "pervk_per_s": round(rate["N"], 1), "earlier_route_per_s": round(rate["P"], 1),
        "ratio_pervk_over_earlier_route": round(rate["N"] / rate["P"], 1),
        "shared_verkey_per_s": round(rate["S"], 1), "verify_pervk_per_s": round(rate["V"], 1),
        "pervk_single_proof_ms": round(single_ms, 3),
        "pervk_phase_ms": {"prep": round(phases[0], 3), "miller": round(phases[1], 3), "fexp": round(phases[2], 3)},
        "blocks_per_s": {k: [round(x, 1) for x in v] for k, v in blocks.items()},
        "spread": {k: round(v, 4) for k, v in spread.items()},
    }
    ctx.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
