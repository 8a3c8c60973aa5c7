"""Holder-side issuance on one context, inputs resident in HBM (by default 65,536 requests, q = 6
messages of which k = 3 hidden, library-default request tables):

  N  cc_sigreq_new_batch_device                                          (SignatureRequest::new)
  P  cc_sigreq_pok_init_batch_device + cc_sigreq_pok_gen_proof_batch_device  (SignatureRequestPoK, challenge given)
  V  cc_sigreq_verify_batch on the requests and proofs N and P produced      (the yardstick, same run)

V has a host form only, so its time includes staging its inputs from host memory; N and P read and write
device buffers.  The gate: before any number is printed, what N and P wrote goes through
cc_sigreq_verify_batch and every request must be accepted.  The three run in alternating blocks (N P V N
P V ...) after a warm-up, one batch in flight, each call timed with a host clock around a stream
synchronise.  One JSON line: requests/s of each, the N/V and P/V ratios and the spread over blocks.

    python tools/bench_sigreq_prove.py [--g1] [--n 65536] [--q 6] [--k 3] [--blocks 3] [--reps 3] [--warmup 1]
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

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g1", action="store_true", help="SigG1 (requests in G1)")
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--q", type=int, default=6)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--bits", type=int, default=0, help="request table window width (0: chosen by memory)")
    ap.add_argument("--blocks", type=int, default=3, help="timed blocks of each path (at least 3)")
    ap.add_argument("--reps", type=int, default=3, help="calls per block")
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if args.blocks < 3:
        ap.error("--blocks must be at least 3")
    if not 0 <= args.k <= args.q or args.q < 1:
        ap.error("need 0 <= k <= q and q >= 1")
    import secrets
    import numpy as np
    import torch
    import coconut
    lib = coconut._lib.lib
    mode = 1 if args.g1 else 0
    dev = torch.device("cuda", 0)
    ctx = coconut.Context(0, coconut.GroupMode(mode))
    n, q, k = args.n, args.q, args.k
    sg = 2 if mode == 0 else 1
    gen = {1: coconut.G1_GENERATOR, 2: coconut.G2_GENERATOR}[sg]
    sb = ctx.mode.sig_bytes
    pb = coconut.sigreq_proof_bytes(ctx, k)
    be = lambda v: v.to_bytes(48, "big")  # noqa: E731
    scal = lambda c: b"".join(be(int.from_bytes(secrets.token_bytes(48), "big") % R) for _ in range(c))  # noqa: E731
    bases = coconut.fixed_base_mul(ctx, sg, gen, scal(q + 1))
    g, hv = bases[:sb], bases[sb:]
    t0 = time.perf_counter()
    ctx.set_request_params(g, hv, args.bits)
    table_s = time.perf_counter() - t0
    host = dict(msgs=scal(n * q), rand=scal(n * (k + 1)), blind=scal(n * (3 * k + 2)), sk=scal(n), chal=scal(n))
    host["pk"] = coconut.fixed_base_mul(ctx, sg, g, host["sk"])
    D = {key: torch.frombuffer(bytearray(v + b"\0"), dtype=torch.uint8).to(dev) for key, v in host.items()}
    for key, w in (("commitment", sb), ("h", sb), ("cts", k * 2 * sb), ("proofs", pb)):
        D[key] = torch.zeros(n * w + 16, dtype=torch.uint8, device=dev)
    P = {key: ctypes.c_void_p(t.data_ptr()) for key, t in D.items()}
    stream = torch.cuda.Stream(dev)
    sh = ctypes.c_void_p(stream.cuda_stream)
    torch.cuda.synchronize(dev)

    def ck(st, what):
        if st != 0:
            raise RuntimeError(f"{what}: {lib.cc_status_str(st).decode()}")

    def run_n():
        ck(lib.cc_sigreq_new_batch_device(ctx.h, n, q, k, P["msgs"], P["pk"], P["rand"], P["commitment"], P["h"],
                                          P["cts"], sh), "cc_sigreq_new_batch_device")

    def run_p():
        ck(lib.cc_sigreq_pok_init_batch_device(ctx.h, n, q, k, P["h"], P["pk"], P["blind"], P["proofs"], sh),
           "cc_sigreq_pok_init_batch_device")
        ck(lib.cc_sigreq_pok_gen_proof_batch_device(ctx.h, n, q, k, P["msgs"], P["rand"], P["blind"], P["sk"],
                                                    P["chal"], P["proofs"], sh), "cc_sigreq_pok_gen_proof_batch_device")

    V = {}
    verdicts = np.zeros(n, dtype=np.uint8)

    def stage_v():
        """The host copies cc_sigreq_verify_batch reads: what N and P last wrote."""
        stream.synchronize()
        for key, w in (("commitment", sb), ("cts", k * 2 * sb), ("proofs", pb)):
            V[key] = np.ascontiguousarray(D[key][:max(n * w, 1)].cpu().numpy())
        msgs = np.frombuffer(host["msgs"], dtype=np.uint8).reshape(n, q * 48)
        V["known"] = np.ascontiguousarray(msgs[:, k * 48:]) if q > k else np.zeros(1, np.uint8)
        V["pk"] = np.frombuffer(host["pk"], dtype=np.uint8)
        V["chal"] = np.frombuffer(host["chal"], dtype=np.uint8)
        V["g"] = np.frombuffer(g, dtype=np.uint8)
        V["hv"] = np.frombuffer(hv, dtype=np.uint8)

    def run_v():
        p = lambda key: ctypes.c_void_p(V[key].ctypes.data)  # noqa: E731
        ck(lib.cc_sigreq_verify_batch(ctx.h, n, q, k, p("g"), p("hv"), p("commitment"), p("known") if q > k else None,
                                      p("cts") if k else None, p("pk"), p("proofs"), p("chal"),
                                      ctypes.c_void_p(verdicts.ctypes.data)), "cc_sigreq_verify_batch")

    def timed(f):
        stream.synchronize()
        t0 = time.perf_counter()
        f()
        stream.synchronize()
        return time.perf_counter() - t0

    for _ in range(args.warmup):
        timed(run_n)
        timed(run_p)
    stage_v()
    timed(run_v)
    # the gate: every request and proof the device produced is accepted by the device's verifier
    bad = int(n - int(verdicts.sum()))
    if bad:
        raise SystemExit(f"cc_sigreq_verify_batch rejected {bad} of {n} produced proofs")
    blocks = {"N": [], "P": [], "V": []}
    for _ in range(args.blocks):
        for name, f in (("N", run_n), ("P", run_p), ("V", run_v)):
            ts = [timed(f) for _ in range(args.reps)]
            blocks[name].append(n / statistics.median(ts))
    stage_v()
    verdicts[:] = 0
    run_v()
    if int(verdicts.sum()) != n:
        raise SystemExit("a timed call changed a verdict")
    rate = {key: statistics.median(v) for key, v in blocks.items()}
    spread = {key: (max(v) - min(v)) / statistics.median(v) for key, v in blocks.items()}
    out = {
        "tool": "bench_sigreq_prove", "mode": "SigG1" if mode else "SigG2", "n": n, "q": q, "k": k,
        "table_bits_asked": args.bits, "table_build_s": round(table_s, 3), "blocks": args.blocks, "reps": args.reps,
        "version": coconut.version(),
        "new_per_s": round(rate["N"], 1), "prove_per_s": round(rate["P"], 1), "verify_per_s": round(rate["V"], 1),
        "ratio_new_over_verify": round(rate["N"] / rate["V"], 4),
        "ratio_prove_over_verify": round(rate["P"] / rate["V"], 4),
        "new_blocks": [round(x, 1) for x in blocks["N"]], "prove_blocks": [round(x, 1) for x in blocks["P"]],
        "verify_blocks": [round(x, 1) for x in blocks["V"]],
        "new_spread": round(spread["N"], 4), "prove_spread": round(spread["P"], 4),
        "verify_spread": round(spread["V"], 4),
    }
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
