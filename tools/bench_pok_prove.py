"""Holder-side proving on one context, inputs resident in HBM (the config-5 shape by default: 65,536
credentials, q = 32, 8 revealed, library-default tables):

  P  cc_pok_init_batch_device + cc_pok_gen_proof_batch_device   (PoKOfSignature::init + gen_proof, challenge given)
  I  cc_pok_init_batch_device alone
  V  cc_pok_verify_batch_device on the proofs P produced          (the yardstick, same run)

The gate: before any number is printed, the proofs P wrote go through cc_pok_verify_batch_device and
every one must be accepted.  The three run in alternating blocks (P I V P I V ...) after a warm-up, one
batch in flight, each call timed with a host clock around a stream synchronise.  One JSON line:
proofs/s of each and the spread over blocks.

    python tools/bench_pok_prove.py [--g1] [--n 65536] [--q 32] [--blocks 3] [--reps 5] [--warmup 2]
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


def make_credentials(ctx, mode, n, q, seed=5):
    """n valid credentials with known discrete logs (as bench_modes.make_pok_batch builds its proofs):
    vk = gk (x, y) G~, sigma_1 = k G, sigma_2 = k (x + sum y_i m_i) G, points by cc_fixed_base_mul."""
    import numpy as np
    import coconut
    from bench_modes import _be, _fr
    rng = np.random.default_rng(seed)
    og, sg = (1, 2) if mode == 0 else (2, 1)
    gen = {1: coconut.G1_GENERATOR, 2: coconut.G2_GENERATOR}
    ob = 97 if og == 1 else 192
    x, y, gk = _fr(rng), [_fr(rng) for _ in range(q)], _fr(rng) or 1
    vk = coconut.fixed_base_mul(ctx, og, gen[og], b"".join(_be(v * gk) for v in [x] + y + [1]))
    e1, e2, msgs = [], [], []
    for _ in range(n):
        m = [_fr(rng) for _ in range(q)]
        k = _fr(rng) or 1
        e1.append(_be(k))
        e2.append(_be(k * (x + sum(a * b for a, b in zip(y, m)))))
        msgs.append(m)
    return dict(X=vk[:ob], Y=vk[ob:ob * (q + 1)], g_tilde=vk[ob * (q + 1):],
                s1=coconut.fixed_base_mul(ctx, sg, gen[sg], b"".join(e1)),
                s2=coconut.fixed_base_mul(ctx, sg, gen[sg], b"".join(e2)), msgs=msgs)


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
    import secrets
    import torch
    import coconut
    from bench_modes import REVEALED, _be
    lib = coconut._lib.lib
    mode = 1 if args.g1 else 0
    dev = torch.device("cuda", 0)
    ctx = coconut.Context(0, coconut.GroupMode(mode))
    n, q = args.n, args.q
    revealed = [i for i in REVEALED if i < q]
    r, nresp = len(revealed), q - len(revealed) + 1
    c = make_credentials(ctx, mode, n, q)
    ctx.set_params(c["g_tilde"])
    ctx.set_verkey(c["X"], c["Y"])
    sb, ob = ctx.mode.sig_bytes, ctx.mode.other_bytes
    scal = lambda k: b"".join(_be(int.from_bytes(secrets.token_bytes(48), "big") % R) for _ in range(k))  # noqa: E731
    host = dict(s1=c["s1"], s2=c["s2"], msgs=b"".join(_be(v) for m in c["msgs"] for v in m),
                rand=scal(n * (nresp + 2)), chal=scal(n),
                rev=b"".join(_be(m[i]) for m in c["msgs"] for i in revealed))
    D = {k: torch.frombuffer(bytearray(v + b"\0"), dtype=torch.uint8).to(dev) for k, v in host.items()}
    for k, w in (("o1", sb), ("o2", sb), ("J", ob), ("T", ob), ("resp", nresp * 48), ("verdicts", 1)):
        D[k] = torch.zeros(n * w, dtype=torch.uint8, device=dev)
    P = {k: ctypes.c_void_p(t.data_ptr()) for k, t in D.items()}
    idx = (ctypes.c_uint64 * max(r, 1))(*revealed)
    stream = torch.cuda.Stream(dev)
    sh = ctypes.c_void_p(stream.cuda_stream)
    torch.cuda.synchronize(dev)

    def ck(st, what):
        if st != 0:
            raise RuntimeError(f"{what}: {lib.cc_status_str(st).decode()}")

    def run_i():
        ck(lib.cc_pok_init_batch_device(ctx.h, n, q, r, nresp, P["s1"], P["s2"], P["msgs"], idx, P["rand"], P["o1"],
                                        P["o2"], P["J"], P["T"], sh), "cc_pok_init_batch_device")

    def run_p():
        run_i()
        ck(lib.cc_pok_gen_proof_batch_device(ctx.h, n, q, r, nresp, P["msgs"], idx, P["rand"], P["chal"], P["resp"], sh),
           "cc_pok_gen_proof_batch_device")

    def run_v():
        ck(lib.cc_pok_verify_batch_device(ctx.h, n, q, r, nresp, P["o1"], P["o2"], P["J"], P["T"], P["resp"], P["chal"],
                                          idx, P["rev"], P["verdicts"], None, sh), "cc_pok_verify_batch_device")

    def timed(f):
        stream.synchronize()
        t0 = time.perf_counter()
        f()
        stream.synchronize()
        return time.perf_counter() - t0

    for _ in range(args.warmup):
        timed(run_p)
        timed(run_i)
        timed(run_v)
    # the gate: every proof the device produced is accepted by the device's verifier
    bad = int(n - int(D["verdicts"].sum().item()))
    if bad:
        raise SystemExit(f"cc_pok_verify_batch_device rejected {bad} of {n} produced proofs")
    blocks = {"P": [], "I": [], "V": []}
    for _ in range(args.blocks):
        for name, f in (("P", run_p), ("I", run_i), ("V", run_v)):
            ts = [timed(f) for _ in range(args.reps)]
            blocks[name].append(n / statistics.median(ts))
    if int(D["verdicts"].sum().item()) != n:
        raise SystemExit("a timed call changed a verdict")
    rate = {k: statistics.median(v) for k, v in blocks.items()}
    spread = {k: (max(v) - min(v)) / statistics.median(v) for k, v in blocks.items()}
    vb = ctypes.c_int()
    ib = ctypes.c_int()
    lib.cc_table_bits(ctx.h, ctypes.byref(vb), ctypes.byref(ib))
    out = {
        "tool": "bench_pok_prove", "mode": "SigG1" if mode else "SigG2", "n": n, "q": q, "revealed": r,
        "table_bits": vb.value, "blocks": args.blocks, "reps": args.reps, "version": coconut.version(),
        "prove_per_s": round(rate["P"], 1), "init_per_s": round(rate["I"], 1), "verify_per_s": round(rate["V"], 1),
        "ratio_prove_over_verify": round(rate["P"] / rate["V"], 4),
        "prove_blocks": [round(x, 1) for x in blocks["P"]], "init_blocks": [round(x, 1) for x in blocks["I"]],
        "verify_blocks": [round(x, 1) for x in blocks["V"]],
        "prove_spread": round(spread["P"], 4), "init_spread": round(spread["I"], 4),
        "verify_spread": round(spread["V"], 4),
    }
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
