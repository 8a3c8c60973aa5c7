"""The PoK RLC batch mode's accept and reject paths against the PoK locate mode and the per-proof path, in one
process on one context and one batch resident in HBM (config 5's shape by default: 65,536 proofs, q = 32, 8
revealed), per group mode, one call in flight, library-default tables:

  P  cc_pok_verify_batch_device alone, all valid                                  (the per-proof path)
  A  cc_pok_rlc_partial_device + cc_rlc_finish_device, all valid                  (today's accept path)
  B  cc_pok_verify_batch_locate_device, all valid                                 (per seg)
  C  A, then cc_pok_verify_batch_device over the whole batch, one bad proof       (today's reject path)
  D  cc_pok_verify_batch_locate_device, the same bad proof                        (per seg)
  E  cc_pok_verify_batch_locate_device, one bad in each of 8 evenly spaced segments   (per seg)

A bad proof carries its successor's sigma'_2: its Schnorr relation holds, only the pairing equation fails.  The
legs run alternately (P, A, C, then B D E for every seg, and again) in --blocks blocks of --reps calls after a
warm-up of each; a call is timed with a host clock around a stream synchronise.  Every leg's outputs are checked
before anything is printed: verdicts against the per-proof path's on the same arrays (which must equal
construction), accept bits, the locate statistics.  One JSON line a mode: each leg's rate (proofs/s, median of
the block medians) and spread over blocks, B/A, D/C and D/P per seg, whether D beats C by more than twice the
run's spread, and the seg the rule of CC_LOCATE_SEG_DEFAULT_* picks: the best D among the segs whose B/A loss
is within twice the run's spread, else the smallest loss.

    python tools/bench_pok_locate.py [--modes g2,g1] [--n 65536] [--q 32] [--segs 1024,...] [--blocks 3] [--reps 3]
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

KEYS = ("s1", "s2", "J", "T", "resp", "chal", "rev")


def run_mode(args, mode):
    import numpy as np
    import torch
    import coconut
    from bench_modes import REVEALED, make_pok_batch
    lib = coconut._lib.lib
    dev = torch.device("cuda", 0)
    ctx = coconut.Context(0, coconut.GroupMode(mode))
    n, q, segs = args.n, args.q, args.segs
    revealed = [i for i in REVEALED if i < q]
    b = make_pok_batch(ctx, mode, n, q=q, revealed=revealed, seed=5, bad_every=0)
    ctx.set_params(b["g_tilde"])
    ctx.set_verkey(b["X"], b["Y"])
    r, nresp = len(revealed), b["nresp"]
    sb = 192 if mode == 0 else 97

    def swapped(bad):  # sigma'_2 of every index in bad replaced by its successor's
        s2 = bytearray(b["s2"])
        expect = np.ones(n, np.uint8)
        for i in bad:
            s2[i * sb:(i + 1) * sb] = b["s2"][(i + 1) * sb:(i + 2) * sb]
            expect[i] = 0
        return bytes(s2), expect

    one = [n * 19 // 32 + 3]
    eight = [n * k // 8 + 5 for k in range(8)]
    s2_one, exp_one = swapped(one)
    s2_eight, exp_eight = swapped(eight)
    to_dev = lambda x: torch.frombuffer(bytearray(x + b"\0"), dtype=torch.uint8).to(dev)  # noqa: E731
    D = {k: to_dev(b[k]) for k in KEYS}
    d_s2 = {"ok": D["s2"], "one": to_dev(s2_one), "eight": to_dev(s2_eight)}
    expect = {"ok": np.ones(n, np.uint8), "one": exp_one, "eight": exp_eight}
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    idx = (ctypes.c_uint64 * max(r, 1))(*revealed)
    verdicts = torch.zeros(n, dtype=torch.uint8, device=dev)
    part = torch.zeros(coconut.dist.PARTIAL_WORDS, dtype=torch.int32, device=dev)
    accept = torch.zeros(1, dtype=torch.uint8, device=dev)
    stats = (ctypes.c_uint32 * 3)()
    stream = torch.cuda.Stream(dev)
    sh = ctypes.c_void_p(stream.cuda_stream)
    torch.cuda.synchronize(dev)

    def ck(st, what):
        if st != 0:
            raise RuntimeError(f"{what}: {lib.cc_status_str(st).decode()}")

    def arrays(which):
        return (ptr(D["s1"]), ptr(d_s2[which]), ptr(D["J"]), ptr(D["T"]), ptr(D["resp"]), ptr(D["chal"]), idx,
                ptr(D["rev"]))

    def per_proof(which):
        ck(lib.cc_pok_verify_batch_device(ctx.h, n, q, r, nresp, *arrays(which), ptr(verdicts), None, sh),
           "cc_pok_verify_batch_device")

    def rlc(which):
        ck(lib.cc_pok_rlc_partial_device(ctx.h, n, q, r, nresp, 0, os.urandom(32), *arrays(which), ptr(part), sh),
           "cc_pok_rlc_partial_device")
        ck(lib.cc_rlc_finish_device(ctx.h, 1, ptr(part), ptr(accept), None, sh), "cc_rlc_finish_device")

    def run_p():
        per_proof("ok")

    def run_a():
        rlc("ok")

    def run_c():  # the caller's fall-back: read the accept bit, then verify everything per proof
        rlc("one")
        stream.synchronize()
        if int(accept.item()) == 0:
            per_proof("one")

    def locate(which, seg):
        def f():
            ck(lib.cc_pok_verify_batch_locate_device(ctx.h, n, q, r, nresp, seg, os.urandom(32), *arrays(which),
                                                     ptr(verdicts), stats, sh), "cc_pok_verify_batch_locate_device")
        return f

    def timed(f):
        stream.synchronize()
        t0 = time.perf_counter()
        f()
        stream.synchronize()
        return time.perf_counter() - t0

    # the reference of every check: the per-proof path's verdicts on each of the three inputs
    ref = {}
    for which in ("ok", "one", "eight"):
        verdicts.zero_()
        per_proof(which)
        stream.synchronize()
        ref[which] = verdicts.cpu().numpy().copy()
        if not np.array_equal(ref[which], expect[which]):
            raise SystemExit(f"per-proof path on '{which}': verdicts differ from construction")

    def check(name, which, seg=None):  # after a call of the leg: its outputs against the per-proof path's
        if name == "A":
            ok = int(accept.item()) == 1
        elif name == "P":
            ok = np.array_equal(verdicts.cpu().numpy(), ref["ok"])
        elif name == "C":
            ok = int(accept.item()) == 0 and np.array_equal(verdicts.cpu().numpy(), ref["one"])
        else:
            S = -(-n // seg)
            rej = {int(i) // seg for i in np.flatnonzero(ref[which] == 0)}
            want = (S, len(rej), sum(min(n, (s + 1) * seg) - s * seg for s in rej))
            ok = tuple(stats) == want and np.array_equal(verdicts.cpu().numpy(), ref[which])
        if not ok:
            raise SystemExit(f"leg {name} seg {seg}: outputs differ from the per-proof path's")

    legs = [("P", None, run_p, "ok"), ("A", None, run_a, "ok"), ("C", None, run_c, "one")]
    for seg in segs:
        legs += [("B", seg, locate("ok", seg), "ok"), ("D", seg, locate("one", seg), "one"),
                 ("E", seg, locate("eight", seg), "eight")]
    for name, seg, f, which in legs:  # warm-up (workspaces grow here) and the gate
        for _ in range(args.warmup):
            verdicts.zero_()
            timed(f)
        check(name, which, seg)
    blocks = {(name, seg): [] for name, seg, _, _ in legs}
    for _ in range(args.blocks):
        for name, seg, f, which in legs:
            verdicts.zero_()
            ts = [timed(f) for _ in range(args.reps)]
            check(name, which, seg)
            blocks[(name, seg)].append(n / statistics.median(ts))
    rate = {k: statistics.median(v) for k, v in blocks.items()}
    spread = {k: (max(v) - min(v)) / statistics.median(v) for k, v in blocks.items()}
    run_spread = max(spread.values())
    p, a, c = rate[("P", None)], rate[("A", None)], rate[("C", None)]
    per_seg = {}
    for seg in segs:
        d = rate[("D", seg)]
        per_seg[str(seg)] = {
            "B_per_s": round(rate[("B", seg)], 1), "D_per_s": round(d, 1), "E_per_s": round(rate[("E", seg)], 1),
            "B_spread": round(spread[("B", seg)], 4), "D_spread": round(spread[("D", seg)], 4),
            "E_spread": round(spread[("E", seg)], 4),
            "B_over_A": round(rate[("B", seg)] / a, 4), "D_over_C": round(d / c, 4), "D_over_P": round(d / p, 4),
            "D_beats_C": bool(d / c - 1 > 2 * run_spread),
        }
    loss = {seg: 1 - rate[("B", seg)] / a for seg in segs}
    within = [seg for seg in segs if loss[seg] <= 2 * run_spread]
    pick = max(within, key=lambda s: rate[("D", s)]) if within else min(segs, key=lambda s: loss[s])
    out = {
        "tool": "bench_pok_locate", "mode": "SigG1" if mode else "SigG2", "n": n, "q": q, "revealed": r,
        "blocks": args.blocks, "reps": args.reps, "version": coconut.version(),
        "P_per_s": round(p, 1), "P_spread": round(spread[("P", None)], 4),
        "A_per_s": round(a, 1), "A_spread": round(spread[("A", None)], 4),
        "C_per_s": round(c, 1), "C_spread": round(spread[("C", None)], 4),
        "A_over_P": round(a / p, 4), "run_spread": round(run_spread, 4), "segs": per_seg,
        "picked_seg": pick, "picked_by": "best D within twice the spread" if within else "smallest B/A loss",
        "picked_B_over_A_loss": round(loss[pick], 4), "picked_D_over_C": per_seg[str(pick)]["D_over_C"],
        "picked_D_over_P": per_seg[str(pick)]["D_over_P"], "picked_D_beats_C": per_seg[str(pick)]["D_beats_C"],
    }
    ctx.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="g2,g1")
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--q", type=int, default=32)
    ap.add_argument("--segs", default="1024,2048,4096,8192,16384")
    ap.add_argument("--blocks", type=int, default=3, help="timed blocks of each leg (at least 3)")
    ap.add_argument("--reps", type=int, default=3, help="calls per block")
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if args.blocks < 3:
        ap.error("--blocks must be at least 3")
    args.segs = [int(s) for s in args.segs.split(",")]
    for m in args.modes.split(","):
        run_mode(args, {"g2": 0, "g1": 1}[m])


if __name__ == "__main__":
    main()
