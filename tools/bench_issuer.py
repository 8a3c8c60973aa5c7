"""Issuer side of issuance on one context (by default 65,536 requests, q = 6 messages of which k = 3 hidden,
library-default request tables).  Requests and proofs are made by the device prover calls
(cc_sigreq_new_batch_device, cc_sigreq_pok_init_batch_device, cc_sigreq_pok_gen_proof_batch_device); a few
proofs are then corrupted.  Legs, each timed with a host clock around a stream synchronise:

  V_host        cc_sigreq_verify_batch, inputs in host memory            (the yardstick, same run)
  V_dev         cc_sigreq_verify_batch_device, inputs in HBM
  V_dev+stage   upload of the same host inputs, the device call, download of the verdicts (like for like with V_host)
  B_host        cc_blind_sign_batch
  B_dev         cc_blind_sign_batch_device, h hashed by the call
  step_reuse    device verify writing h, then device sign reading it      (the issuer's step)
  step_twice    device verify, then device sign hashing h again

The gate, before any number is printed: V_dev's verdicts equal V_host's on the batch (the corrupted proofs
refused, every other accepted) and B_dev's h, c~1, c~2 equal B_host's.  The legs run in alternating blocks
after a warm-up, one batch in flight.  One JSON line: requests/s of each leg, the ratios over V_host / B_host,
the saving from reusing h and the spread over blocks.

    python tools/bench_issuer.py [--g1] [--n 65536] [--q 6] [--k 3] [--blocks 3] [--reps 3] [--warmup 1]
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
LEGS = ("V_host", "V_dev", "V_dev+stage", "B_host", "B_dev", "step_reuse", "step_twice")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g1", action="store_true", help="SigG1 (requests in G1)")
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--q", type=int, default=6)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--bits", type=int, default=0, help="request table window width (0: chosen by memory)")
    ap.add_argument("--blocks", type=int, default=3, help="timed blocks of each leg (at least 3)")
    ap.add_argument("--reps", type=int, default=3, help="calls per block")
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if args.blocks < 3:
        ap.error("--blocks must be at least 3")
    if not 0 <= args.k <= args.q or args.q < 1 or args.n < 8:
        ap.error("need 0 <= k <= q, q >= 1 and n >= 8")
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
    ctx.set_request_params(g, hv, args.bits)
    host = dict(msgs=scal(n * q), rand=scal(n * (k + 1)), blind=scal(n * (3 * k + 2)), sk=scal(n), chal=scal(n))
    host["pk"] = coconut.fixed_base_mul(ctx, sg, g, host["sk"])
    x, y = scal(1), scal(q)
    D = {key: torch.frombuffer(bytearray(v + b"\0"), dtype=torch.uint8).to(dev) for key, v in host.items()}
    for key, w in (("commitment", sb), ("h", sb), ("cts", k * 2 * sb), ("proofs", pb)):
        D[key] = torch.zeros(n * w + 16, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)
    sh = ctypes.c_void_p(stream.cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    torch.cuda.synchronize(dev)

    def ck(st, what):
        if st != 0:
            raise RuntimeError(f"{what}: {lib.cc_status_str(st).decode()}")

    # ---- the batch: requests and proofs from the device prover, a few proofs corrupted
    ck(lib.cc_sigreq_new_batch_device(ctx.h, n, q, k, ptr(D["msgs"]), ptr(D["pk"]), ptr(D["rand"]), ptr(D["commitment"]),
                                      ptr(D["h"]), ptr(D["cts"]), sh), "cc_sigreq_new_batch_device")
    ck(lib.cc_sigreq_pok_init_batch_device(ctx.h, n, q, k, ptr(D["h"]), ptr(D["pk"]), ptr(D["blind"]), ptr(D["proofs"]),
                                           sh), "cc_sigreq_pok_init_batch_device")
    ck(lib.cc_sigreq_pok_gen_proof_batch_device(ctx.h, n, q, k, ptr(D["msgs"]), ptr(D["rand"]), ptr(D["blind"]),
                                                ptr(D["sk"]), ptr(D["chal"]), ptr(D["proofs"]), sh),
       "cc_sigreq_pok_gen_proof_batch_device")
    stream.synchronize()
    corrupted = sorted({3, n // 2, n - 1})
    for i in corrupted:
        D["proofs"][i * pb + sb + 47] ^= 1  # r_sk of request i
    msgs = np.frombuffer(host["msgs"], dtype=np.uint8).reshape(n, q * 48)
    known = np.ascontiguousarray(msgs[:, k * 48:]).reshape(-1) if q > k else np.zeros(0, np.uint8)
    D["known"] = torch.from_numpy(np.concatenate([known, np.zeros(16, np.uint8)])).to(dev)
    torch.cuda.synchronize(dev)
    # the host copies the host forms read, and the device buffers the staged leg uploads them to
    H = {"commitment": D["commitment"][:n * sb], "known": D["known"][:n * (q - k) * 48], "cts": D["cts"][:n * k * 2 * sb],
         "pk": D["pk"][:n * sb], "proofs": D["proofs"][:n * pb], "chal": D["chal"][:n * 48]}
    H = {key: np.ascontiguousarray(t.cpu().numpy()) for key, t in H.items()}
    S = {key: torch.zeros(v.size + 16, dtype=torch.uint8, device=dev) for key, v in H.items()}
    G = {"g": np.frombuffer(g, dtype=np.uint8), "hv": np.frombuffer(hv, dtype=np.uint8),
         "x": np.frombuffer(x, dtype=np.uint8), "y": np.frombuffer(y, dtype=np.uint8)}
    hp = lambda a: ctypes.c_void_p(a.ctypes.data) if a.size else None  # noqa: E731
    dp = lambda t, size=1: ptr(t) if size else None  # noqa: E731
    v_host, v_dev = np.zeros(n, dtype=np.uint8), torch.zeros(n, dtype=torch.uint8, device=dev)
    v_stage = torch.zeros(n, dtype=torch.uint8, device=dev)
    bh = [np.zeros(n * sb, dtype=np.uint8) for _ in range(3)]
    bd = [torch.zeros(n * sb, dtype=torch.uint8, device=dev) for _ in range(3)]
    d_h = torch.zeros(n * sb, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)

    def verify_dev(src, verdicts, out_h):
        ck(lib.cc_sigreq_verify_batch_device(ctx.h, n, q, k, ptr(src["commitment"]), dp(src["known"], q - k),
                                             dp(src["cts"], k), ptr(src["pk"]), ptr(src["proofs"]), ptr(src["chal"]),
                                             ptr(verdicts), out_h, sh), "cc_sigreq_verify_batch_device")

    def sign_dev(h_in):
        ck(lib.cc_blind_sign_batch_device(ctx.h, n, q, k, ptr(D["commitment"]), dp(D["known"], q - k), dp(D["cts"], k),
                                          h_in, hp(G["x"]), hp(G["y"]), ptr(bd[0]), ptr(bd[1]), ptr(bd[2]), sh),
           "cc_blind_sign_batch_device")

    DV = {"commitment": D["commitment"], "known": D["known"], "cts": D["cts"], "pk": D["pk"], "proofs": D["proofs"],
          "chal": D["chal"]}

    def run_v_host():
        ck(lib.cc_sigreq_verify_batch(ctx.h, n, q, k, hp(G["g"]), hp(G["hv"]), hp(H["commitment"]), hp(H["known"]),
                                      hp(H["cts"]), hp(H["pk"]), hp(H["proofs"]), hp(H["chal"]), hp(v_host)),
           "cc_sigreq_verify_batch")

    def run_v_dev():
        verify_dev(DV, v_dev, None)

    staged = {}

    def run_v_stage():
        with torch.cuda.stream(stream):
            for key, a in H.items():
                if a.size:
                    S[key][:a.size].copy_(torch.from_numpy(a), non_blocking=True)
        verify_dev(S, v_stage, None)
        with torch.cuda.stream(stream):
            staged["v"] = v_stage.cpu()

    def run_b_host():
        ck(lib.cc_blind_sign_batch(ctx.h, n, q, k, hp(H["commitment"]), hp(H["known"]), hp(H["cts"]), hp(G["x"]),
                                   hp(G["y"]), hp(bh[0]), hp(bh[1]), hp(bh[2])), "cc_blind_sign_batch")

    def run_b_dev():
        sign_dev(None)

    def run_step_reuse():
        verify_dev(DV, v_dev, ptr(d_h))
        sign_dev(ptr(d_h))

    def run_step_twice():
        verify_dev(DV, v_dev, None)
        sign_dev(None)

    legs = dict(zip(LEGS, (run_v_host, run_v_dev, run_v_stage, run_b_host, run_b_dev, run_step_reuse, run_step_twice)))

    def timed(f):
        stream.synchronize()
        t0 = time.perf_counter()
        f()
        stream.synchronize()
        return time.perf_counter() - t0

    for _ in range(max(args.warmup, 1)):
        for f in legs.values():
            timed(f)

    # ---- the gate
    def gate(when):
        want = np.ones(n, dtype=np.uint8)
        want[corrupted] = 0
        if not (v_host == want).all():
            raise SystemExit(f"{when}: cc_sigreq_verify_batch gave {int((v_host != want).sum())} unexpected verdicts")
        for name, t in (("V_dev", v_dev.cpu().numpy()), ("V_dev+stage", staged["v"].numpy())):
            if not (t == v_host).all():
                raise SystemExit(f"{when}: {name} differs from V_host in {int((t != v_host).sum())} verdicts")
        for name, a, b in zip(("h", "c1", "c2"), bh, bd):
            if not (b.cpu().numpy() == a).all():
                raise SystemExit(f"{when}: B_dev's {name} differs from B_host's")

    timed(run_step_reuse)  # B_dev's outputs from the reused h
    gate("before timing (h reused)")
    timed(run_b_dev)
    gate("before timing")
    blocks = {name: [] for name in LEGS}
    for _ in range(args.blocks):
        for name, f in legs.items():
            ts = [timed(f) for _ in range(args.reps)]
            blocks[name].append(n / statistics.median(ts))
    gate("after timing")
    rate = {key: statistics.median(v) for key, v in blocks.items()}
    spread = {key: (max(v) - min(v)) / statistics.median(v) for key, v in blocks.items()}
    gain = rate["V_dev+stage"] / rate["V_host"] - 1.0
    noise = max(spread["V_dev+stage"], spread["V_host"])
    out = {
        "tool": "bench_issuer", "mode": "SigG1" if mode else "SigG2", "n": n, "q": q, "k": k,
        "table_bits_asked": args.bits, "blocks": args.blocks, "reps": args.reps, "corrupted": len(corrupted),
        "version": coconut.version(),
        "per_s": {key: round(v, 1) for key, v in rate.items()},
        "blocks_per_s": {key: [round(x, 1) for x in v] for key, v in blocks.items()},
        "spread": {key: round(v, 4) for key, v in spread.items()},
        "ratio_v_dev_over_v_host": round(rate["V_dev"] / rate["V_host"], 4),
        "ratio_v_dev_stage_over_v_host": round(rate["V_dev+stage"] / rate["V_host"], 4),
        "ratio_b_dev_over_b_host": round(rate["B_dev"] / rate["B_host"], 4),
        "step_reuse_over_step_twice": round(rate["step_reuse"] / rate["step_twice"], 4),
        "v_dev_stage_gain": round(gain, 4), "spread_to_clear": round(noise, 4),
        "v_dev_stage_clears_spread": bool(gain > noise),
    }
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
