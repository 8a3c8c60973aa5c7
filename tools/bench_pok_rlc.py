"""Per-proof PoK verification against the RLC batch mode, in one process on one context and one
all-valid batch resident in HBM (the config-5 size by default: 65,536 proofs, q = 32, 8 revealed):

  A  cc_pok_verify_batch_device                          (a two-pair Miller loop and a final exponentiation per proof)
  B  cc_pok_rlc_partial_device + cc_rlc_finish_device    (one pair per proof, one final exponentiation per batch)

Both run with one batch in flight, in alternating blocks (A B A B ...), after a warm-up of both; each
call is timed with a host clock around a stream synchronise.  A's verdicts and B's accept bit are
checked before anything is printed.  One JSON line: both rates, their ratio and the spread over blocks.

    python tools/bench_pok_rlc.py [--g1] [--n 65536] [--q 32] [--blocks 3] [--reps 5] [--warmup 2]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g1", action="store_true", help="SigG1 (signatures in G1, the verkey in G2)")
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--q", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=3, help="timed blocks of each path (at least 3)")
    ap.add_argument("--reps", type=int, default=5, help="calls per block")
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if args.blocks < 3:
        ap.error("--blocks must be at least 3")
    import torch
    import coconut
    from bench_modes import REVEALED, make_pok_batch
    lib = coconut._lib.lib
    mode = 1 if args.g1 else 0
    dev = torch.device("cuda", 0)
    ctx = coconut.Context(0, coconut.GroupMode(mode))
    revealed = [i for i in REVEALED if i < args.q]
    b = make_pok_batch(ctx, mode, args.n, q=args.q, revealed=revealed, seed=5, bad_every=0)
    ctx.set_params(b["g_tilde"])
    ctx.set_verkey(b["X"], b["Y"])
    n, q, r, nresp = args.n, args.q, len(revealed), b["nresp"]
    D = [torch.frombuffer(bytearray(b[k] + b"\0"), dtype=torch.uint8).to(dev)
         for k in ("s1", "s2", "J", "T", "resp", "chal", "rev")]
    P = [ctypes.c_void_p(t.data_ptr()) for t in D]
    idx = (ctypes.c_uint64 * max(r, 1))(*revealed)
    verdicts = torch.zeros(n, dtype=torch.uint8, device=dev)
    part = torch.zeros(coconut.dist.PARTIAL_WORDS, dtype=torch.int32, device=dev)
    accept = torch.zeros(1, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)
    sh = ctypes.c_void_p(stream.cuda_stream)
    torch.cuda.synchronize(dev)

    def ck(st, what):
        if st != 0:
            raise RuntimeError(f"{what}: {lib.cc_status_str(st).decode()}")

    def run_a():
        ck(lib.cc_pok_verify_batch_device(ctx.h, n, q, r, nresp, P[0], P[1], P[2], P[3], P[4], P[5], idx, P[6],
                                          ctypes.c_void_p(verdicts.data_ptr()), None, sh), "cc_pok_verify_batch_device")

    def run_b():
        ck(lib.cc_pok_rlc_partial_device(ctx.h, n, q, r, nresp, 0, os.urandom(32), P[0], P[1], P[2], P[3], P[4], P[5],
                                         idx, P[6], ctypes.c_void_p(part.data_ptr()), sh), "cc_pok_rlc_partial_device")
        ck(lib.cc_rlc_finish_device(ctx.h, 1, ctypes.c_void_p(part.data_ptr()), ctypes.c_void_p(accept.data_ptr()),
                                    None, sh), "cc_rlc_finish_device")

    def timed(f):
        stream.synchronize()
        t0 = time.perf_counter()
        f()
        stream.synchronize()
        return time.perf_counter() - t0

    for _ in range(args.warmup):
        timed(run_a)
        timed(run_b)
    # the gate: every per-proof verdict is 1 and the batch check accepts
    if not bool(verdicts.cpu().numpy().all()):
        raise SystemExit("per-proof path rejected a valid proof")
    if int(accept.item()) != 1:
        raise SystemExit("RLC batch check rejected the all-valid batch")
    blocks = {"A": [], "B": []}
    for _ in range(args.blocks):
        for name, f in (("A", run_a), ("B", run_b)):
            ts = [timed(f) for _ in range(args.reps)]
            blocks[name].append(n / statistics.median(ts))
    if not bool(verdicts.cpu().numpy().all()) or int(accept.item()) != 1:
        raise SystemExit("a timed call changed the decision")
    rate = {k: statistics.median(v) for k, v in blocks.items()}
    spread = {k: (max(v) - min(v)) / statistics.median(v) for k, v in blocks.items()}
    out = {
        "tool": "bench_pok_rlc", "mode": "SigG1" if mode else "SigG2", "n": n, "q": q, "revealed": r,
        "blocks": args.blocks, "reps": args.reps, "version": coconut.version(),
        "per_proof_per_s": round(rate["A"], 1), "rlc_per_s": round(rate["B"], 1),
        "ratio_rlc_over_per_proof": round(rate["B"] / rate["A"], 4),
        "per_proof_blocks": [round(x, 1) for x in blocks["A"]], "rlc_blocks": [round(x, 1) for x in blocks["B"]],
        "per_proof_spread": round(spread["A"], 4), "rlc_spread": round(spread["B"], 4),
    }
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
