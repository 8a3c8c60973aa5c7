"""Multi-GPU batch verification: one process per GPU over torch.distributed (backend "nccl" is RCCL
on ROCm, riding xGMI between the GPUs of a node).  SURVEY.md §8e.

The batch shards by credential (credentials are independent):

* per-credential mode — every rank verifies its own contiguous slice; no collective on the data
  path (verdicts stay with the rank that owns the slice);
* RLC mode — every rank reduces its slice to one 929-word partial (the Fp12 Miller product of its
  delta-weighted pairs, a fall-back flag and its 16 fold window sums, ``cc_rlc_partial_device``); ONE
  all-gather of the partials (3,716 B per rank) is the only exchange; every rank pairs the gathered
  window sums with the fixed multiples of g~, multiplies everything and runs the single final
  exponentiation (``cc_rlc_finish_device``), so all ranks reach the same accept/reject
  decision without a second collective.  On reject every rank falls back to per-credential
  verification of its own slice, so verdicts always equal the reference's
  (``Signature::verify``, reference src/signature.rs:473-478, per credential).

Engines decouple this control flow from the device: ``DeviceEngine`` drives libcoconut_hip.so on
device-resident tensors; tests substitute a CPU engine to exercise the same sharding, gather and
decision logic over the gloo backend.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import numpy as np

# 144 Fp12 Montgomery words, fall-back flag, 16 x (48-word affine window sum + identity flag):
# CC_RLC_PARTIAL_WORDS of include/coconut_hip.h (= cc_rlc_partial_words(), checked by tests/test_capi.py)
PARTIAL_WORDS = 929
PARTIAL_FLAG = 144


def shard_bounds(n: int, world: int, rank: int):
    """Contiguous slice [lo, hi) of an n-credential batch owned by `rank` of `world`."""
    return n * rank // world, n * (rank + 1) // world


def _dist():
    import torch.distributed as dist
    return dist if dist.is_available() and dist.is_initialized() else None


def gather_partials(part, group=None):
    """All-gather the per-rank partials (one tensor of PARTIAL_WORDS int32 each) -> (stacked, k).
    Over RCCL ("nccl") the device tensors are gathered in place (3,716 B per rank over xGMI); over gloo
    (CPU transport: tests, hosts without RCCL) a device partial crosses through host memory and the
    gathered partials return to its device."""
    import torch
    dist = _dist()
    world = dist.get_world_size(group) if dist else 1
    if world == 1:
        return part.reshape(1, -1), 1
    dev = part.device
    host = dev.type != "cpu" and dist.get_backend(group) == "gloo"
    src = part.cpu() if host else part
    parts = [torch.empty_like(src) for _ in range(world)]
    dist.all_gather(parts, src, group=group)
    out = torch.stack(parts)
    return (out.to(dev) if host else out), world


def rlc_accept(engine, group=None) -> bool:
    """One RLC decision for the whole (sharded) batch: partial -> all-gather -> finish."""
    part = engine.partial()
    allp, k = gather_partials(part, group)
    return engine.finish(allp, k)


def verify_sharded(engine, rlc=True, group=None) -> np.ndarray:
    """Verdicts (uint8) for this rank's slice; RLC first when requested, per-credential fallback.
    rlc="locate": every rank locates inside its own slice (``engine.locate``: segments with their own RLC
    checks, per-credential verification of the rejected ones only); no collective at all."""
    if rlc == "locate":
        return engine.locate()[0]
    if rlc and rlc_accept(engine, group):
        return np.ones(engine.n, dtype=np.uint8)
    return engine.per_credential()


class DeviceEngine:
    """One rank's slice, resident in HBM as torch tensors, checked through the C ABI."""

    def __init__(self, ctx, n: int, q: int, d_s1, d_s2, d_msgs, base_index: int = 0,
                 seed: Optional[bytes] = None, stream=None):
        import torch
        from ._lib import lib
        self.lib, self.ctx, self.n, self.q = lib, ctx, n, q
        self.d_s1, self.d_s2, self.d_msgs = d_s1, d_s2, d_msgs
        self.base_index = base_index
        self.seed = seed
        self.dev = d_s1.device
        # a real (non-null) stream: a NULL handle would select the context's own non-blocking stream,
        # which is not ordered against torch's default stream
        self.stream = stream if stream is not None else torch.cuda.Stream(self.dev)
        self._sh = ctypes.c_void_p(self.stream.cuda_stream)
        # two partial / accept buffers: a pipelined caller's finish of batch i (finish_async, on its own
        # stream) may still read one while the next partial writes the other.  A third partial issued
        # before batch i's finish has run reuses batch i's slot: partial() then makes the engine's stream
        # wait (on the device) for that finish's event, so the slot is never overwritten while read.
        self._parts = [torch.empty(PARTIAL_WORDS, dtype=torch.int32, device=self.dev) for _ in range(2)]
        self._accepts = [torch.zeros(1, dtype=torch.uint8, device=self.dev) for _ in range(2)]
        self._slot_ev = [None, None]
        self._slot = 0
        self.part = self._parts[0]
        self.accept = self._accepts[0]
        self._fin_stream = None
        self.verdicts = torch.zeros(n, dtype=torch.uint8, device=self.dev)

    def _enter(self):
        import torch
        self.stream.wait_stream(torch.cuda.current_stream(self.dev))

    def _leave(self):
        import torch
        torch.cuda.current_stream(self.dev).wait_stream(self.stream)

    def _check(self, st, what):
        if st != 0:
            from .errors import CoconutError
            raise CoconutError(st, f"{what}: {self.lib.cc_status_str(st).decode()}")

    def partial(self):
        seed = self.seed if self.seed is not None else os.urandom(32)
        self._slot ^= 1
        self.part = self._parts[self._slot]
        self._enter()
        if self._slot_ev[self._slot] is not None:  # a finish_async still reading this slot
            self.stream.wait_event(self._slot_ev[self._slot])
            self._slot_ev[self._slot] = None
        self._check(self.lib.cc_rlc_partial_device(self.ctx.h, self.n, self.q, self.base_index, seed,
                                                   ctypes.c_void_p(self.d_s1.data_ptr()),
                                                   ctypes.c_void_p(self.d_s2.data_ptr()),
                                                   ctypes.c_void_p(self.d_msgs.data_ptr()),
                                                   ctypes.c_void_p(self.part.data_ptr()), self._sh),
                    "cc_rlc_partial_device")
        self._leave()
        return self.part

    def finish(self, allp, k: int, sync: bool = True):
        allp = allp.contiguous()
        self._enter()
        self._check(self.lib.cc_rlc_finish_device(self.ctx.h, k, ctypes.c_void_p(allp.data_ptr()),
                                                  ctypes.c_void_p(self.accept.data_ptr()), None, self._sh),
                    "cc_rlc_finish_device")
        self._leave()
        if not sync:
            return None
        return bool(self.accept.item())

    def finish_async(self, allp, k: int):
        """cc_rlc_finish_device on the engine's second stream, NOT ordered before later work on the
        engine's main stream: the next batch's partial() can overlap this batch's final exponentiation.
        Returns a callable that waits for the decision and returns it.  Any number of finishes may be
        outstanding: the library runs the finishes of one context in call order, and a partial() that
        reuses the slot of an unfinished batch waits for that batch's finish on the device."""
        import torch
        if self._fin_stream is None:
            # high priority: the finish's latency-bound launches (16 waves of window pairs per partial, the
            # product tree, one final exponentiation) take wave slots ahead of the next partial's full
            # launches instead of queueing behind them
            self._fin_stream = torch.cuda.Stream(self.dev, priority=-1)
        fs = self._fin_stream
        allp = allp.contiguous()
        fs.wait_stream(torch.cuda.current_stream(self.dev))  # the gathered partials are ready
        fs.wait_stream(self.stream)
        allp.record_stream(fs)
        acc = self._accepts[self._slot]
        self._check(self.lib.cc_rlc_finish_device(self.ctx.h, k, ctypes.c_void_p(allp.data_ptr()),
                                                  ctypes.c_void_p(acc.data_ptr()), None,
                                                  ctypes.c_void_p(fs.cuda_stream)), "cc_rlc_finish_device")
        # the decision is copied out on the finish stream, so a later batch reusing this slot cannot
        # change what result() returns
        host = torch.empty(1, dtype=torch.uint8, pin_memory=True)
        with torch.cuda.stream(fs):
            host.copy_(acc, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(fs)
        self._slot_ev[self._slot] = ev

        def result() -> bool:
            ev.synchronize()
            return bool(host[0].item())
        return result

    def _ptrs(self):
        return (ctypes.c_void_p(self.d_s1.data_ptr()), ctypes.c_void_p(self.d_s2.data_ptr()),
                ctypes.c_void_p(self.d_msgs.data_ptr()))

    def partial_seg(self, seg: int):
        """cc_rlc_partial_seg_device: one partial per segment of `seg` credentials (a power of two >= 4), a
        (ceil(n / seg), PARTIAL_WORDS) int32 tensor; partial s is what partial() gives for the slice with
        base_index + s * seg."""
        import torch
        seed = self.seed if self.seed is not None else os.urandom(32)
        nseg = -(-self.n // seg) if seg > 0 else 0
        parts = torch.empty((max(nseg, 1), PARTIAL_WORDS), dtype=torch.int32, device=self.dev)
        self._enter()
        self._check(self.lib.cc_rlc_partial_seg_device(self.ctx.h, self.n, self.q, seg, self.base_index, seed,
                                                       *self._ptrs(), ctypes.c_void_p(parts.data_ptr()), self._sh),
                    "cc_rlc_partial_seg_device")
        self._leave()
        return parts[:nseg]

    def finish_each(self, parts, k: int, want_gt: bool = False):
        """cc_rlc_finish_each_device: one decision per partial, a uint8 array of k (and, with want_gt, the
        k x 576 GT bytes); decision s is finish(parts[s:s + 1], 1)'s."""
        import torch
        parts = parts.contiguous()
        acc = torch.zeros(k, dtype=torch.uint8, device=self.dev)
        gt = torch.zeros(k * 576, dtype=torch.uint8, device=self.dev) if want_gt else None
        self._enter()
        self._check(self.lib.cc_rlc_finish_each_device(self.ctx.h, k, ctypes.c_void_p(parts.data_ptr()),
                                                       ctypes.c_void_p(acc.data_ptr()),
                                                       ctypes.c_void_p(gt.data_ptr()) if want_gt else None,
                                                       self._sh), "cc_rlc_finish_each_device")
        self._leave()
        a = acc.cpu().numpy()
        return (a, gt.cpu().numpy().tobytes()) if want_gt else a

    def locate(self, seg: int = 0):
        """cc_verify_batch_locate_device over the slice (deltas from index 0: every slice is checked on its
        own): (verdicts uint8[n], (segments, rejected segments, credentials rechecked))."""
        seed = self.seed if self.seed is not None else os.urandom(32)
        stats = np.zeros(3, dtype=np.uint32)
        self._enter()
        self._check(self.lib.cc_verify_batch_locate_device(self.ctx.h, self.n, self.q, seg, seed, *self._ptrs(),
                                                           ctypes.c_void_p(self.verdicts.data_ptr()),
                                                           ctypes.c_void_p(stats.ctypes.data), self._sh),
                    "cc_verify_batch_locate_device")
        self._leave()
        return self.verdicts.cpu().numpy(), tuple(int(x) for x in stats)

    def per_credential(self) -> np.ndarray:
        self._enter()
        self._check(self.lib.cc_verify_batch_device(self.ctx.h, self.n, self.q,
                                                    ctypes.c_void_p(self.d_s1.data_ptr()),
                                                    ctypes.c_void_p(self.d_s2.data_ptr()),
                                                    ctypes.c_void_p(self.d_msgs.data_ptr()),
                                                    ctypes.c_void_p(self.verdicts.data_ptr()), None, self._sh),
                    "cc_verify_batch_device")
        self._leave()
        return self.verdicts.cpu().numpy()


class PokDeviceEngine(DeviceEngine):
    """One rank's slice of a PoKOfSignatureProof::verify batch, resident in HBM as torch tensors: the
    interface of DeviceEngine (partial / finish / finish_async / per_credential), so rlc_accept,
    verify_sharded and gather_partials serve PoK batches unchanged.  The partial is
    ``cc_pok_rlc_partial_device`` (finished by ``cc_rlc_finish_device``, like a signature shard's), the
    per-proof path ``cc_pok_verify_batch_device``.  revealed_idx is a host sequence shared by the batch."""

    def __init__(self, ctx, n: int, q: int, revealed_idx, d_s1, d_s2, d_J, d_T, d_responses, d_chal,
                 d_revealed_msgs, base_index: int = 0, seed: Optional[bytes] = None, stream=None):
        super().__init__(ctx, n, q, d_s1, d_s2, None, base_index=base_index, seed=seed, stream=stream)
        self.r = len(revealed_idx)
        self.nresp = q - self.r + 1
        self.idx = (np.ascontiguousarray(np.asarray(revealed_idx, dtype=np.uint64)) if self.r
                    else np.zeros(1, np.uint64))
        self.d_J, self.d_T, self.d_responses, self.d_chal = d_J, d_T, d_responses, d_chal
        self.d_revealed_msgs = d_revealed_msgs

    def _proof_args(self):
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        return (p(self.d_s1), p(self.d_s2), p(self.d_J), p(self.d_T), p(self.d_responses), p(self.d_chal),
                ctypes.c_void_p(self.idx.ctypes.data), p(self.d_revealed_msgs))

    def partial(self):
        seed = self.seed if self.seed is not None else os.urandom(32)
        self._slot ^= 1
        self.part = self._parts[self._slot]
        self._enter()
        if self._slot_ev[self._slot] is not None:  # a finish_async still reading this slot
            self.stream.wait_event(self._slot_ev[self._slot])
            self._slot_ev[self._slot] = None
        self._check(self.lib.cc_pok_rlc_partial_device(self.ctx.h, self.n, self.q, self.r, self.nresp,
                                                       self.base_index, seed, *self._proof_args(),
                                                       ctypes.c_void_p(self.part.data_ptr()), self._sh),
                    "cc_pok_rlc_partial_device")
        self._leave()
        return self.part

    def partial_seg(self, seg: int):
        """cc_pok_rlc_partial_seg_device: one partial per segment of `seg` proofs (a power of two >= 4), a
        (ceil(n / seg), PARTIAL_WORDS) int32 tensor; partial s is what partial() gives for the slice with
        base_index + s * seg.  finish_each (inherited) decides them."""
        import torch
        seed = self.seed if self.seed is not None else os.urandom(32)
        nseg = -(-self.n // seg) if seg > 0 else 0
        parts = torch.empty((max(nseg, 1), PARTIAL_WORDS), dtype=torch.int32, device=self.dev)
        self._enter()
        self._check(self.lib.cc_pok_rlc_partial_seg_device(self.ctx.h, self.n, self.q, self.r, self.nresp, seg,
                                                           self.base_index, seed, *self._proof_args(),
                                                           ctypes.c_void_p(parts.data_ptr()), self._sh),
                    "cc_pok_rlc_partial_seg_device")
        self._leave()
        return parts[:nseg]

    def locate(self, seg: int = 0):
        """cc_pok_verify_batch_locate_device over the slice (deltas from index 0): (verdicts uint8[n],
        (segments, rejected segments, proofs rechecked)); seg = 0: the library's default for the mode."""
        seed = self.seed if self.seed is not None else os.urandom(32)
        stats = np.zeros(3, dtype=np.uint32)
        self._enter()
        self._check(self.lib.cc_pok_verify_batch_locate_device(self.ctx.h, self.n, self.q, self.r, self.nresp, seg,
                                                               seed, *self._proof_args(),
                                                               ctypes.c_void_p(self.verdicts.data_ptr()),
                                                               ctypes.c_void_p(stats.ctypes.data), self._sh),
                    "cc_pok_verify_batch_locate_device")
        self._leave()
        return self.verdicts.cpu().numpy(), tuple(int(x) for x in stats)

    def per_credential(self) -> np.ndarray:
        self._enter()
        self._check(self.lib.cc_pok_verify_batch_device(self.ctx.h, self.n, self.q, self.r, self.nresp,
                                                        *self._proof_args(),
                                                        ctypes.c_void_p(self.verdicts.data_ptr()), None, self._sh),
                    "cc_pok_verify_batch_device")
        self._leave()
        return self.verdicts.cpu().numpy()
