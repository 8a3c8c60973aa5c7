"""Pedersen VSS verify_share on one context, at tools/bench_keygen.py's two shapes: 4,096 committees of (t = 3,
total = 5, q = 6) and 8 committees of BASELINE config 4's (t = 67, total = 100, q = 32).  The shares are dealt
on the device (cc_keygen_deal_batch_device) and every share of every (committee, polynomial) set is verified:
143,360 shares in 28,672 sets, and 26,400 shares in 264 sets.  Legs, each timed with a host clock around a
stream synchronise:

  old          cc_vss_verify_batch on the repacked rows in host memory, uploads included (the yardstick)
  sets_host    cc_vss_verify_sets, rlc = 0, on the same host rows: the same uploads, old's like-for-like pair
  exact        cc_keygen_verify_shares_batch_device, rlc = 0, on the deal's outputs in HBM
  rlc_valid    the same with rlc = 1, every share valid
  rlc_one_bad  rlc = 1, one altered share in one set
  rlc_1pct     rlc = 1, one altered share in 1 % of the sets

The gate, before any number is printed and again after timing: every leg's verdicts equal old's on the same
shares (old runs on the clean rows and on both altered variants), the clean verdicts are all ones, and the altered
variants reject exactly the altered rows.  The legs run in alternating blocks after a warm-up, one batch in
flight.  One JSON line: milliseconds per block, shares/s, spreads over blocks, and the ratios sets_host / old,
exact / old and rlc_valid / exact with the spread each has to clear.

    python tools/bench_vss_verify.py [--g1] [--bits 0] [--blocks 3] [--reps 2] [--warmup 1] [--inner 4] [--small]
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
LEGS = ("old", "sets_host", "exact", "rlc_valid", "rlc_one_bad", "rlc_1pct")
SHAPES = (("committees", 4096, 3, 5, 6), ("config4", 8, 67, 100, 32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g1", action="store_true", help="SigG1 (verkeys in G2)")
    ap.add_argument("--bits", type=int, default=0, help="keygen table window width (0: chosen by memory)")
    ap.add_argument("--blocks", type=int, default=3, help="timed blocks of each leg (at least 3)")
    ap.add_argument("--reps", type=int, default=2, help="timed windows per block (the block's value: their median)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--inner", type=int, default=4, help="calls per timed window of a device leg (host legs: one)")
    ap.add_argument("--small", action="store_true", help="64 committees instead of 4,096 (a quick check)")
    args = ap.parse_args()
    if args.blocks < 3:
        ap.error("--blocks must be at least 3")
    import secrets
    import numpy as np
    import torch
    import coconut
    lib = coconut._lib.lib
    mode = 1 if args.g1 else 0
    dev = torch.device("cuda", 0)
    ctx = coconut.Context(0, coconut.GroupMode(mode))
    og = 1 if mode == 0 else 2
    be = lambda v: v.to_bytes(48, "big")  # noqa: E731
    scal = lambda c: b"".join(be(int.from_bytes(secrets.token_bytes(48), "big") % R) for _ in range(c))  # noqa: E731
    gt = coconut.fixed_base_mul(ctx, og, {1: coconut.G1_GENERATOR, 2: coconut.G2_GENERATOR}[og], scal(1))
    gh = coconut.fixed_base_mul(ctx, 1, coconut.G1_GENERATOR, scal(2))
    g, h = gh[:97], gh[97:]
    ctx.set_keygen_params(gt, g, h, args.bits)
    stream = torch.cuda.Stream(dev)
    up = lambda b: torch.frombuffer(bytearray(b + b"\0"), dtype=torch.uint8).to(dev)  # noqa: E731
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    seed = secrets.token_bytes(32)

    def ck(st, what):
        if st != 0:
            raise RuntimeError(f"{what}: {lib.cc_status_str(st).decode()}")

    def timed(f, calls=1):
        """Seconds per call of `calls` back-to-back calls, one synchronise at the end."""
        stream.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            f()
        stream.synchronize()
        return (time.perf_counter() - t0) / calls

    result = {"tool": "bench_vss_verify", "mode": "SigG1" if mode else "SigG2", "table_bits_asked": args.bits,
              "blocks": args.blocks, "reps": args.reps, "inner": args.inner, "version": coconut.version(),
              "device_call": "cc_keygen_verify_shares_batch_device", "shapes": {}}
    for name, m, t, total, q in SHAPES:
        if args.small and m > 64:
            m = 64
        nc, ns = m * (q + 1) * t, m * (q + 1)
        n = ns * total
        cf, ct = up(scal(nc)), up(scal(nc))
        torch.cuda.synchronize(dev)
        x, y, xt, yt, comm, _, _ = coconut.keygen_deal_batch_device(ctx, m, q, t, total, cf, ct, stream=stream)
        stream.synchronize()

        # the altered variants: signer 1's share of set j (p = 0: x, p = 1 + k: y_k) with its last byte flipped
        def altered(sets_hit):
            x2, y2 = x.clone(), y.clone()
            for j in sets_hit:
                kg, p = divmod(j, q + 1)
                o = (kg * total) if p == 0 else (kg * total * q + p - 1)
                buf = x2 if p == 0 else y2
                buf[o * 48 + 47] = buf[o * 48 + 47] ^ 1
            return x2, y2
        hit = {"clean": [], "one_bad": [ns // 2], "pct": list(range(0, ns, 100))}
        var = {"clean": (x, y)}
        var["one_bad"], var["pct"] = altered(hit["one_bad"]), altered(hit["pct"])
        torch.cuda.synchronize(dev)

        # the same shares as host rows in the verdict order (committee, polynomial, signer)
        def rows_of(xv, yv):
            a = lambda v, inner: np.frombuffer(v.cpu().numpy().tobytes(), dtype=np.uint8)[:m * total * inner * 48]  # noqa: E731
            X, Xt = (a(v, 1).reshape(m, 1, total, 48) for v in (xv, xt))
            Y, Yt = (a(v, q).reshape(m, total, q, 48).transpose(0, 2, 1, 3) for v in (yv, yt))
            s, st = np.concatenate([X, Y], axis=1), np.concatenate([Xt, Yt], axis=1)
            return np.ascontiguousarray(np.concatenate([s, st], axis=-1).reshape(n, 96))
        rows = {k: rows_of(*v) for k, v in var.items()}
        ids = np.ascontiguousarray(np.tile(np.arange(1, total + 1, dtype=np.uint64), ns))
        set_of = np.ascontiguousarray(np.repeat(np.arange(ns, dtype=np.uint32), total))
        begin = np.ascontiguousarray(np.arange(ns + 1, dtype=np.uint64) * total)
        hcomm = np.frombuffer(comm.cpu().numpy().tobytes(), dtype=np.uint8)[:ns * t * 97].copy()
        out = {leg: np.zeros(n, dtype=np.uint8) for leg in ("old", "sets_host")}
        dout = {leg: torch.zeros(n, dtype=torch.uint8, device=dev) for leg in LEGS[2:]}
        stats = {leg: np.zeros(4, dtype=np.uint32) for leg in LEGS[1:]}
        dp = lambda v: ctypes.c_void_p(v.data_ptr())  # noqa: E731
        sp = ctypes.c_void_p(stream.cuda_stream)

        def run_old(which="clean", into=None):
            ck(lib.cc_vss_verify_batch(ctx.h, n, t, g, h, ptr(hcomm), ns, ptr(set_of), ptr(ids), ptr(rows[which]),
                                       ptr(out["old"] if into is None else into)), "cc_vss_verify_batch")

        def run_sets_host():
            ck(lib.cc_vss_verify_sets(ctx.h, n, t, ns, ptr(begin), ptr(hcomm), ptr(ids), ptr(rows["clean"]), 0,
                                      ptr(out["sets_host"]), ptr(stats["sets_host"])), "cc_vss_verify_sets")

        def device_leg(leg, which, rlc):
            xv, yv = var[which]

            def f():
                ck(lib.cc_keygen_verify_shares_batch_device(ctx.h, m, q, t, total, dp(xv), dp(yv), dp(xt), dp(yt),
                                                            dp(comm), rlc, seed, dp(dout[leg]), ptr(stats[leg]), sp),
                   "cc_keygen_verify_shares_batch_device")
            return f
        legs = {"old": run_old, "sets_host": run_sets_host, "exact": device_leg("exact", "clean", 0),
                "rlc_valid": device_leg("rlc_valid", "clean", 1), "rlc_one_bad": device_leg("rlc_one_bad", "one_bad", 1),
                "rlc_1pct": device_leg("rlc_1pct", "pct", 1)}
        variant = {"old": "clean", "sets_host": "clean", "exact": "clean", "rlc_valid": "clean",
                   "rlc_one_bad": "one_bad", "rlc_1pct": "pct"}
        # old's verdicts on the three variants, once: the yardstick of the gate
        ref = {}
        for which in var:
            ref[which] = np.zeros(n, dtype=np.uint8)
            run_old(which, ref[which])
            want = np.ones(n, dtype=np.uint8)
            want[[j * total for j in hit[which]]] = 0
            if not (ref[which] == want).all():
                raise SystemExit(f"{name}: cc_vss_verify_batch does not reject exactly the altered rows ({which})")
        for _ in range(max(args.warmup, 1)):
            for f in legs.values():
                timed(f)

        def gate(when):
            stream.synchronize()
            for leg in LEGS:
                got = out[leg] if leg in out else dout[leg].cpu().numpy()
                if not (got == ref[variant[leg]]).all():
                    raise SystemExit(f"{name} {when}: {leg}'s verdicts differ from cc_vss_verify_batch's")

        gate("before timing")
        blocks = {leg: [] for leg in LEGS}
        for _ in range(args.blocks):
            for leg, f in legs.items():
                calls = 1 if leg in out else args.inner
                blocks[leg].append(statistics.median(timed(f, calls) for _ in range(args.reps)))
        gate("after timing")
        med = {leg: statistics.median(v) for leg, v in blocks.items()}
        spread = {leg: (max(v) - min(v)) / med[leg] for leg, v in blocks.items()}

        def ratio(num, den):  # how many times faster num's leg is than den's, and the spread it has to clear twice
            return {"ratio": round(med[den] / med[num], 3), "spread": round(max(spread[num], spread[den]), 4)}
        result["shapes"][name] = {
            "m": m, "t": t, "total": total, "q": q, "sets": ns, "shares": n,
            "ms": {leg: [round(1e3 * v, 3) for v in b] for leg, b in blocks.items()},
            "ms_median": {leg: round(1e3 * v, 3) for leg, v in med.items()},
            "shares_per_s": {leg: round(n / v, 1) for leg, v in med.items()},
            "spread": {leg: round(v, 4) for leg, v in spread.items()},
            "stats4": {leg: [int(v) for v in s] for leg, s in stats.items()},
            "sets_host_over_old": ratio("sets_host", "old"), "exact_over_old": ratio("exact", "old"),
            "rlc_valid_over_exact": ratio("rlc_valid", "exact"),
        }
    ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
