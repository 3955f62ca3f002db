"""Data-parallel gradient exchange over RCCL (torch.distributed backend "nccl" = RCCL on ROCm).

Replaces what the reference gets implicitly from `accelerator.prepare` -> torch DDP
(src/train.py:61-64): an all-reduce(sum) of every trainable gradient per step, overlapped with
the backward.  MI355X-first design:
  * the VideoMAE plugin keeps its gradients in two flat f32 buffers (VideoMAETemporal in three, its
    temporal blocks' between the head's and the encoder's); this class owns them
    (`grad_buffer`) and the model reports finished ranges during its hand-sequenced backward
    (`mark_ready`) — head first (its 77 M-param Base gradient is ready before any encoder work),
    then encoder layers in reverse order;
  * finished ranges are coalesced into buckets of >= `bucket_mb` and launched immediately with
    `async_op=True`: RCCL's stream waits on the current stream at the call, so the collective of
    bucket k runs on its own stream while the backward kernels of layer k-1 execute.  8 MB by
    default: the ViT-Tiny encoder's gradients are 22 MB in all (1.8 MB per layer), so 32-MB
    buckets left the whole encoder to one all-reduce after the last backward kernel; at 8 MB three
    of them run under the remaining layers and only the last ~6 MB is exposed.  An 8-MB ring
    all-reduce over 8 ranks still moves 1-MB pieces per xGMI hop (bandwidth-bound, not latency);
  * no 1/world scaling pass: the optimizer folds it in (`FusedAdamW(grad_scale=1/world)`);
  * like DDP's constructor, every parameter and buffer is broadcast from the group's first rank
    once at construction, so all replicas start from the same weights whatever each rank's
    initialisation seed was.
Parameters that never report ranges (e.g. the Linear plugin's per-layer tensors) are reduced
in `finish()` as one flattened call.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import torch
import torch.distributed as dist


class GradExchange:
    def __init__(self, model: torch.nn.Module, bucket_mb: float = 8.0, group=None, return_grads: bool = False,
                 ddp=None):
        """return_grads: the model's autograd Function hands the (being-reduced) sink buffers back
        to autograd as the gradients instead of installing them as `.grad` itself — the mode DDP
        needs (its reducer fires on those gradients, `attach_ddp`).  ddp: that DDP wrapper, whose
        `no_sync()` state the sink follows (gradient accumulation, see `_mode`)."""
        self.model = model
        self.group = group
        self.return_grads = return_grads
        self.ddp = ddp
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.bucket_elems = int(bucket_mb * (1 << 20) / 4)
        self._buffers: Dict[int, torch.Tensor] = {}
        self._pending: Dict[int, List[Tuple[int, int]]] = {}
        self._works = []
        self._sunk = set()
        self._accumulating = False      # a no_sync micro-step ran since the last synchronised step
        self._passthrough = set()       # ids whose gradient of this step DDP reduces itself
        self._fwd_sync = None           # DDP's require_backward_grad_sync when the last forward ran
        if self.world > 1:
            src = dist.get_global_rank(group, 0) if group is not None else 0
            with torch.no_grad():
                for t in list(model.parameters()) + list(model.buffers()):
                    dist.broadcast(t.detach(), src=src, group=group)
        # a collective's write does not bump a tensor's version: re-cast low-precision weight
        # shadows explicitly instead of trusting the version counter
        if hasattr(model, "invalidate_lp"):
            model.invalidate_lp()
        if hasattr(model, "grad_sink"):
            model.grad_sink = self
            # the flat buffers whose gradients the model hands over through this sink (a plugin with
            # more than the two names them in SUNK_BUFFERS): finish() leaves those to the buckets
            names = getattr(model, "SUNK_BUFFERS", ("enc_flat", "head_flat"))
            self._sunk = {id(getattr(model, n)) for n in names} if hasattr(model, "enc_flat") else set()

    def _mode(self) -> str:
        """'overlap' (launch bucketed all-reduces during the backward), 'local' (DDP no_sync
        micro-step: plain local gradients, no collective) or 'passthrough' (the synchronised step
        that closes an accumulation window: DDP's bucket holds the ACCUMULATED local gradients, so
        DDP's own all-reduce handles this step and nothing is launched early)."""
        if self.ddp is None or self.world == 1:
            return "overlap"
        # DDP decides at FORWARD time whether this iteration synchronises (its reducer is prepared in
        # DDP.forward); a backward run outside the no_sync() block its forward ran in must follow
        # the forward's decision, so the flag recorded by the forward pre-hook wins
        sync = self._fwd_sync if self._fwd_sync is not None else self.ddp.require_backward_grad_sync
        if not sync:
            self._accumulating = True
            return "local"
        return "passthrough" if self._accumulating else "overlap"

    # ---- sink protocol (called from the model's backward) ---------------------------------------
    def grad_buffer(self, p: torch.Tensor) -> torch.Tensor:
        mode = self._mode()
        if mode != "overlap":
            if mode == "passthrough":
                self._passthrough.add(id(p))
            buf = torch.zeros_like(p)
            if not self.return_grads:
                p.grad = buf
            self._pending[id(p)] = None
            return buf
        self._passthrough.discard(id(p))
        buf = self._buffers.get(id(p))
        if buf is None or buf.device != p.device:
            buf = torch.zeros_like(p)
            self._buffers[id(p)] = buf
        else:
            buf.zero_()
        self._pending[id(p)] = []
        if not self.return_grads:
            p.grad = buf
        return buf

    def reduced(self, p: torch.Tensor):
        """The all-reduced (summed) gradient buffer of a sink parameter, or None (also when DDP
        reduces this step's gradient itself: the step after no_sync micro-steps)."""
        if id(p) in self._passthrough:
            return None
        return self._buffers.get(id(p))

    def mark_ready(self, p: torch.Tensor, lo: int, hi: int) -> None:
        if self.world == 1 or hi <= lo or self._pending.get(id(p), []) is None:
            return            # local / passthrough step: no early collective
        pend = self._pending.setdefault(id(p), [])
        pend.append((lo, hi))
        pend.sort()
        # coalesce adjacent ranges; launch every merged span that reached the bucket size
        merged: List[Tuple[int, int]] = []
        for a, b in pend:
            if merged and merged[-1][1] == a:
                merged[-1] = (merged[-1][0], b)
            else:
                merged.append((a, b))
        keep = []
        for a, b in merged:
            if b - a >= self.bucket_elems or (a == 0 and b == p.numel()):
                self._launch(self._buffers[id(p)][a:b])
            else:
                keep.append((a, b))
        self._pending[id(p)] = keep

    def _launch(self, t: torch.Tensor) -> None:
        self._works.append(dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group, async_op=True))

    # ---- end of backward ------------------------------------------------------------------------
    def end_backward(self) -> None:
        """Called by the model when its backward has handed over every gradient: the forward's
        recorded DDP sync decision has been consumed (a stale flag could steer a later
        backward whose forward bypassed the DDP wrapper)."""
        self._fwd_sync = None

    def finish(self) -> None:
        """Flush partial buckets, reduce the non-sink gradients, and make the current stream wait."""
        if self.world > 1:
            for pid, spans in self._pending.items():
                if spans is None:
                    continue
                for a, b in spans:
                    self._launch(self._buffers[pid][a:b])
                spans.clear()
            rest = [] if self.return_grads else [p for p in self.model.parameters()   # DDP reduces those
                                                 if p.grad is not None and id(p) not in self._sunk]
            if rest:
                flat = torch.cat([p.grad.reshape(-1) for p in rest])
                dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group)
                off = 0
                for p in rest:
                    n = p.grad.numel()
                    p.grad.copy_(flat[off:off + n].view_as(p.grad))
                    off += n
        for w in self._works:
            w.wait()
        self._works.clear()


# ------------------------------------------------------------------------------------------------
# Under accelerate / torch DDP (the reference's caller: src/train.py:61-64 `accelerator.prepare`,
# src/trainer/base.py:150 `accelerator.backward`).
#
# Without anything from this module the plugins already train correctly under DDP: the VideoMAE
# autograd Function returns the two flat gradients at the end of its hand-sequenced backward and
# DDP's reducer all-reduces (averages) them — but only then, with no overlap, because to autograd
# the whole backward is one node.  `attach_ddp(ddp_model)` restores the overlap without replacing
# DDP: a GradExchange sink launches the bucketed all-reduces DURING the backward (head first, then
# encoder layers in reverse), and a DDP communication hook hands DDP those already-reduced
# gradients (averaged) instead of starting its own all-reduce.  Parameters without a sink range
# (e.g. the Linear plugin's) take DDP's default all-reduce in the same hook.
# ------------------------------------------------------------------------------------------------
def _overlap_hook(exchange: "GradExchange", bucket):
    import torch.distributed.algorithms.ddp_comm_hooks.default_hooks as dh
    params = bucket.parameters()
    if not all(exchange.reduced(p) is not None for p in params):
        if any(id(p) in exchange._passthrough for p in params):
            exchange._accumulating = False      # this synchronised step closes the no_sync window
        return dh.allreduce_hook(exchange.group, bucket)
    exchange.finish()                      # this step's early all-reduces have landed (stream order)
    buf = bucket.buffer()
    off = 0
    for p in params:
        n = p.numel()
        buf[off:off + n].copy_(exchange.reduced(p).reshape(-1)).div_(exchange.world)
        off += n
    fut = torch.futures.Future()
    fut.set_result(buf)
    return fut


def attach_ddp(ddp_model, bucket_mb: float = 8.0) -> "GradExchange":
    """Overlap the gradient all-reduce with the backward for a DDP-wrapped vspike plugin (e.g. the
    module `accelerator.prepare` returned).  Returns the exchange; nothing else changes in the
    caller: DDP still averages, the optimizer keeps grad_scale 1.  Gradient accumulation with
    `ddp_model.no_sync()` keeps DDP's semantics: no_sync micro-steps produce local gradients only,
    and the synchronised step that follows is reduced by DDP itself (from the accumulated
    gradients, without the early overlap); steps with no accumulation overlap as usual."""
    module = ddp_model.module
    ex = GradExchange(module, bucket_mb=bucket_mb, group=ddp_model.process_group, return_grads=True, ddp=ddp_model)
    if hasattr(module, "grad_sink"):
        module.grad_sink = ex
    ddp_model.register_comm_hook(ex, _overlap_hook)

    def _record_sync(mod, args):
        ex._fwd_sync = bool(mod.require_backward_grad_sync)
    ddp_model.register_forward_pre_hook(_record_sync)
    return ex
