"""Device keygen on one context, at two shapes: 4,096 committees of (t = 3, total = 5, q = 6) and 8 committees
of BASELINE config 4's (t = 67, total = 100, q = 32).  Coefficients are drawn on the host once and live in HBM;
library-default table widths unless --bits.  Legs, each timed with a host clock around a stream synchronise:

  deal         cc_keygen_deal_batch_device, Pedersen (shares, blinding shares, commitments, verkeys)
  deal_sss     the same, Shamir (no f', no commitments)
  combine      cc_keygen_combine_batch_device over the deal's outputs read as groups of d = 5 dealers
  derive       the derivation alone: cc_keygen_combine_batch_device with d = 1 and no Pedersen buffers, whose
               sums are copies, on exactly the deal's shares
  derive_old   cc_fixed_base_mul on the same scalars from host memory (the yardstick, same run): the one route to
               g~ * share before the keygen entry points; it builds an 8-bit table on every call

The gate, before any number is printed: the deal's verkeys equal cc_fixed_base_mul's on its shares; deal_sss and
derive give the deal's shares and verkeys; a sample of the dealt (s, s') pairs passes cc_vss_verify_batch
against the dealt commitments, and one altered share does not; the combined shares are the sums (host big
integers), their verkeys equal cc_fixed_base_mul's, and a sample of them passes cc_vss_verify_batch against the
combined commitments.  The legs run in alternating blocks after a warm-up, one batch in flight.  One JSON line:
keygens/s of deal, deal_sss and combine (groups/s), scalars/s of derive and derive_old, their ratio and the
spread over blocks.

A timed window is --inner back-to-back calls (a single call is about a millisecond, too short to time alone).

    python tools/bench_keygen.py [--g1] [--bits 0] [--blocks 3] [--reps 3] [--warmup 1] [--inner 32] [--small]
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
LEGS = ("deal", "deal_sss", "combine", "derive", "derive_old")
SHAPES = (("committees", 4096, 3, 5, 6), ("config4", 8, 67, 100, 32))
D = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g1", action="store_true", help="SigG1 (verkeys in G2)")
    ap.add_argument("--bits", type=int, default=0, help="keygen table window width (0: chosen by memory)")
    ap.add_argument("--blocks", type=int, default=3, help="timed blocks of each leg (at least 3)")
    ap.add_argument("--reps", type=int, default=3, help="calls per block")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--inner", type=int, default=32,
                    help="calls per timed window of a device leg (derive_old: an eighth), so a window is tens of ms")
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
    ob = ctx.mode.other_bytes
    be = lambda v: v.to_bytes(48, "big")  # noqa: E731
    scal = lambda c: b"".join(be(int.from_bytes(secrets.token_bytes(48), "big") % R) for _ in range(c))  # noqa: E731
    gt = coconut.fixed_base_mul(ctx, og, {1: coconut.G1_GENERATOR, 2: coconut.G2_GENERATOR}[og], scal(1))
    gh = coconut.fixed_base_mul(ctx, 1, coconut.G1_GENERATOR, scal(2))
    g, h = gh[:97], gh[97:]
    ctx.set_keygen_params(gt, g, h, args.bits)
    stream = torch.cuda.Stream(dev)
    up = lambda b: torch.frombuffer(bytearray(b + b"\0"), dtype=torch.uint8).to(dev)  # noqa: E731
    host = lambda t: None if t is None else bytes(t.cpu().numpy())  # noqa: E731

    def timed(f, calls=1):
        """Seconds per call of `calls` back-to-back calls, one synchronise at the end."""
        stream.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            f()
        stream.synchronize()
        return (time.perf_counter() - t0) / calls

    result = {"tool": "bench_keygen", "mode": "SigG1" if mode else "SigG2", "table_bits_asked": args.bits,
              "blocks": args.blocks, "reps": args.reps, "inner": args.inner, "d": D, "version": coconut.version(), "shapes": {}}
    for name, m, t, total, q in SHAPES:
        if args.small and m > 64:
            m = 64
        mg = m // D  # combine: groups of D dealers
        nc, ns = m * (q + 1) * t, m * total * (q + 1)
        cf, ct = up(scal(nc)), up(scal(nc))
        torch.cuda.synchronize(dev)
        out = {}

        def run_deal():
            out["deal"] = coconut.keygen_deal_batch_device(ctx, m, q, t, total, cf, ct, stream=stream)

        def run_deal_sss():
            out["deal_sss"] = coconut.keygen_deal_batch_device(ctx, m, q, t, total, cf, None, stream=stream)

        timed(run_deal)
        dx, dy, dxt, dyt, dcomm, dX, dY = out["deal"]
        shares_host = np.frombuffer(host(dx) + host(dy), dtype=np.uint8)
        old = np.zeros(ns * ob, dtype=np.uint8)

        def run_combine():
            out["combine"] = coconut.keygen_combine_batch_device(ctx, mg, D, q, t, total, dx, dy, dxt, dyt, dcomm,
                                                                 stream=stream)

        def run_derive():
            out["derive"] = coconut.keygen_combine_batch_device(ctx, m, 1, q, t, total, dx, dy, stream=stream)

        def run_derive_old():
            st = lib.cc_fixed_base_mul(ctx.h, og, gt, ns, ctypes.c_void_p(shares_host.ctypes.data),
                                       ctypes.c_void_p(old.ctypes.data))
            if st != 0:
                raise RuntimeError(f"cc_fixed_base_mul: {lib.cc_status_str(st).decode()}")

        legs = dict(zip(LEGS, (run_deal, run_deal_sss, run_combine, run_derive, run_derive_old)))
        for _ in range(max(args.warmup, 1)):
            for f in legs.values():
                timed(f)

        def sample_verifies(x, xt, y, yt, comm, groups, alter):
            """cc_vss_verify_batch on signer 1 and signer `total` of every polynomial of up to 8 keygens."""
            hx, hxt, hy, hyt, hc = (host(v) for v in (x, xt, y, yt, comm))
            ks = sorted({0, groups // 2, groups - 1} | set(range(min(groups, 5))))
            sets, set_of, ids, sh = [], [], [], []
            for k in ks:
                for p in range(q + 1):
                    s = k * (q + 1) + p
                    sets.append([hc[(s * t + i) * 97:(s * t + i + 1) * 97] for i in range(t)])
                    for i in sorted({0, total - 1}):
                        o = (k * total + i) if p == 0 else ((k * total + i) * q + p - 1)
                        a, b = (hx, hxt) if p == 0 else (hy, hyt)
                        set_of.append(len(sets) - 1)
                        ids.append(i + 1)
                        sh.append((a[o * 48:(o + 1) * 48], b[o * 48:(o + 1) * 48]))
            v = coconut.vss_verify_batch(ctx, t, g, h, sets, set_of, ids, sh)
            if not v.all():
                return False
            if alter:
                sh[1] = (be((int.from_bytes(sh[1][0], "big") + 1) % R), sh[1][1])
                v = coconut.vss_verify_batch(ctx, t, g, h, sets, set_of, ids, sh)
                return v[1] == 0 and v.sum() == len(ids) - 1
            return True

        def gate(when):
            deal = [host(v) for v in out["deal"]]
            if bytes(old) != deal[5] + deal[6]:
                raise SystemExit(f"{name} {when}: the deal's verkeys differ from cc_fixed_base_mul's")
            sss, der = [host(v) for v in out["deal_sss"]], [host(v) for v in out["derive"]]
            for what, got in (("deal_sss", sss), ("derive", der)):
                if [got[i] for i in (0, 1, 5, 6)] != [deal[i] for i in (0, 1, 5, 6)] or got[2:5] != [None] * 3:
                    raise SystemExit(f"{name} {when}: {what} differs from the deal")
            if not sample_verifies(dx, dxt, dy, dyt, dcomm, m, True):
                raise SystemExit(f"{name} {when}: dealt shares do not verify against the dealt commitments")
            cx, cy, cxt, cyt, ccomm, cX, cY = out["combine"]
            for buf, src, inner in ((cx, deal[0], total), (cy, deal[1], total * q), (cxt, deal[2], total),
                                    (cyt, deal[3], total * q)):
                v = [int.from_bytes(src[i * 48:(i + 1) * 48], "big") for i in range(mg * D * inner)]
                want = b"".join(be(sum(v[(gr * D + dd) * inner + e] for dd in range(D)) % R)
                                for gr in range(mg) for e in range(inner))
                if host(buf) != want:
                    raise SystemExit(f"{name} {when}: a combined share is not the sum of the dealers'")
            cs = host(cx) + host(cy)
            chk = coconut.fixed_base_mul(ctx, og, gt, cs)
            if chk != host(cX) + host(cY):
                raise SystemExit(f"{name} {when}: the combined verkeys differ from cc_fixed_base_mul's")
            if not sample_verifies(cx, cxt, cy, cyt, ccomm, mg, False):
                raise SystemExit(f"{name} {when}: combined shares do not verify against the combined commitments")

        gate("before timing")
        blocks = {leg: [] for leg in LEGS}
        for _ in range(args.blocks):
            for leg, f in legs.items():
                calls = max(1, args.inner // 8) if leg == "derive_old" else args.inner
                blocks[leg].append(statistics.median(timed(f, calls) for _ in range(args.reps)))
        gate("after timing")
        units = {"deal": m, "deal_sss": m, "combine": mg, "derive": ns, "derive_old": ns}
        rate = {leg: units[leg] / statistics.median(v) for leg, v in blocks.items()}
        spread = {leg: (max(v) - min(v)) / statistics.median(v) for leg, v in blocks.items()}
        ratio = rate["derive"] / rate["derive_old"]
        noise = max(spread["derive"], spread["derive_old"])
        result["shapes"][name] = {
            "m": m, "t": t, "total": total, "q": q, "groups": mg, "derive_scalars": ns,
            "per_s": {leg: round(v, 1) for leg, v in rate.items()},
            "ms": {leg: [round(1e3 * x, 3) for x in v] for leg, v in blocks.items()},
            "spread": {leg: round(v, 4) for leg, v in spread.items()},
            "derive_over_derive_old": round(ratio, 3), "spread_to_clear": round(noise, 4),
            "derive_not_slower": bool(ratio >= 1.0 - noise),
            "deal_ms_minus_derive_ms": round(1e3 * (statistics.median(blocks["deal"]) - statistics.median(blocks["derive"])), 3),
        }
    ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
