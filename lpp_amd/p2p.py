"""Inter-stage point-to-point activation/gradient exchange over RCCL/xGMI.

Native replacement for the p2p DeepSpeed's PipelineEngine performs inside
``train_batch``.  Differences by design:

- ONE tensor per hop: the bf16 hidden state [mbs, S, H].  The reference
  ships (hidden, [B,1,S,S] fp16 mask, position_ids int64) per microbatch —
  at seq 4096 the mask alone is 32 MiB/hop of pure overhead; we ship 0.
  With sequence packing (``doc_shape``) a second static-shape message follows
  the hidden state on the forward channel: ``doc_start`` int32 [mbs, S], 4
  bytes per token against 2 x hidden for the activation.  It is posted and
  sent in the same order as the hidden state, so the pre-posted-receive
  discipline holds unchanged; the backward channel carries gradients only.
  Without packing no second message exists.
- Static shapes: the engine knows (mbs, S, H) up front, so there is no
  per-tensor meta handshake on the wire; recv buffers come from the caching
  allocator.
- TWO dedicated communicators (topology.pipe_fwd_group / pipe_bwd_group):
  activation traffic and gradient traffic ride separate RCCL comms, i.e.
  separate internal streams.  That makes pre-posted receives safe — a recv
  for the NEXT microbatch's activation enqueued on the fwd channel can
  never serialize behind this microbatch's gradient send on the bwd
  channel, which is the stream-ordering hazard that deadlocks an overlapped
  1F1B schedule on a single comm stream.
- Asynchronous primitives (``irecv_forward`` etc.) return a ``Pending``
  handle; the engine posts receives one microbatch ahead and waits only at
  the point of use, overlapping the xGMI transfer with compute
  (SURVEY.md hard-part #2; the reference delegates this to DeepSpeed's
  double-buffered p2p behind trainer_base_ds_mp.py:354).

On a single fully-connected xGMI node every stage pair is one hop; the
neighbour-only PP pattern gives each stage boundary a dedicated link
(~153 GB/s each way, full duplex).
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.distributed as dist

from .topology import ProcessGrid


class Pending:
    """An in-flight p2p operation: ``wait()`` blocks (stream-orders, on
    RCCL) until complete and returns the received buffer (None for sends).
    Holds a reference to the tensor so the caching allocator cannot reuse
    the storage while the transfer is in flight."""

    __slots__ = ("req", "buf")

    def __init__(self, req, buf: Optional[torch.Tensor]):
        self.req = req
        self.buf = buf

    def wait(self) -> Optional[torch.Tensor]:
        if self.req is not None:
            self.req.wait()
            self.req = None
        return self.buf


class PendingGroup:
    """Several in-flight operations posted together; ``wait()`` completes them
    in posting order and returns their buffers as a tuple."""

    __slots__ = ("parts",)

    def __init__(self, *parts: Pending):
        self.parts = parts

    def wait(self):
        return tuple(p.wait() for p in self.parts)


class PipeP2P:
    def __init__(self, grid: ProcessGrid, act_shape: Tuple[int, ...], dtype: torch.dtype,
                 device: torch.device, doc_shape: Optional[Tuple[int, ...]] = None):
        self.grid = grid
        self.act_shape = tuple(act_shape)
        self.dtype = dtype
        self.device = device
        # sequence packing: shape [mbs, S] of the int32 doc_start message that
        # follows every hidden state on the forward channel (None: no such message)
        self.doc_shape = tuple(doc_shape) if doc_shape is not None else None
        self.fwd_messages_sent = 0  # forward-channel sends posted by this stage
        # channel groups (None outside an initialized process group, e.g.
        # single-process tests — p2p is a no-op there anyway)
        self._fwd_group = grid.pipe_fwd_group
        self._bwd_group = grid.pipe_bwd_group

    def _empty(self) -> torch.Tensor:
        return torch.empty(self.act_shape, dtype=self.dtype, device=self.device)

    def warmup_channels(self) -> None:
        """One tiny ring exchange per channel so the RCCL communicators for
        pipe_fwd/pipe_bwd initialize at a controlled point (engine init)
        instead of lazily inside the overlapped 1F1B schedule — communicator
        creation is collective per group, and first-use inside a schedule
        interleaves two groups' inits across ranks."""
        if not dist.is_initialized() or self.grid.num_stages <= 1:
            return
        t = torch.ones(1, dtype=self.dtype, device=self.device)
        for send_rank, recv_rank, group in (
            (self.grid.next_rank, self.grid.prev_rank, self._fwd_group),
            (self.grid.prev_rank, self.grid.next_rank, self._bwd_group),
        ):
            reqs = []
            if recv_rank is not None:
                buf = torch.empty(1, dtype=self.dtype, device=self.device)
                reqs.append(dist.irecv(buf, recv_rank, group=group))
            if send_rank is not None:
                reqs.append(dist.isend(t, send_rank, group=group))
            for r in reqs:
                r.wait()

    # -- async primitives (the engine's hot path) ---------------------------
    def isend_forward(self, tensor: torch.Tensor,
                      doc_start: Optional[torch.Tensor] = None):
        """Post the activation send to the next stage on the fwd channel;
        with packing, ``doc_start`` right after it."""
        if self.grid.next_rank is None:
            return None
        if (doc_start is not None) != (self.doc_shape is not None):
            raise ValueError("doc_start is sent exactly when the channel was built "
                             "with doc_shape")
        t = tensor.contiguous()
        req = dist.isend(t, self.grid.next_rank, group=self._fwd_group)
        self.fwd_messages_sent += 1
        if doc_start is None:
            return Pending(req, t)
        d = doc_start.contiguous()
        if tuple(d.shape) != self.doc_shape or d.dtype is not torch.int32:
            raise ValueError(f"doc_start must be int32 {self.doc_shape}, got "
                             f"{d.dtype} {tuple(d.shape)}")
        dreq = dist.isend(d, self.grid.next_rank, group=self._fwd_group)
        self.fwd_messages_sent += 1
        return PendingGroup(Pending(req, t), Pending(dreq, d))

    def irecv_forward(self):
        """Post the activation receive; with packing also the ``doc_start``
        receive, and ``wait()`` returns (hidden, doc_start)."""
        if self.grid.prev_rank is None:
            return None
        buf = self._empty()
        req = dist.irecv(buf, self.grid.prev_rank, group=self._fwd_group)
        if self.doc_shape is None:
            return Pending(req, buf)
        dbuf = torch.empty(self.doc_shape, dtype=torch.int32, device=self.device)
        dreq = dist.irecv(dbuf, self.grid.prev_rank, group=self._fwd_group)
        return PendingGroup(Pending(req, buf), Pending(dreq, dbuf))

    def isend_backward(self, grad: torch.Tensor) -> Optional[Pending]:
        """Post the gradient send to the previous stage on the bwd channel."""
        if self.grid.prev_rank is None:
            return None
        t = grad.contiguous()
        req = dist.isend(t, self.grid.prev_rank, group=self._bwd_group)
        return Pending(req, t)

    def irecv_backward(self) -> Optional[Pending]:
        if self.grid.next_rank is None:
            return None
        buf = self._empty()
        req = dist.irecv(buf, self.grid.next_rank, group=self._bwd_group)
        return Pending(req, buf)

    # -- blocking convenience (eval/generation; not the training hot path) --
    def send_forward(self, tensor: Optional[torch.Tensor],
                     doc_start: Optional[torch.Tensor] = None) -> None:
        if tensor is None or self.grid.next_rank is None:
            return
        p = self.isend_forward(tensor, doc_start)
        if p is not None:
            p.wait()

    def recv_forward(self):
        """The hidden state, or (hidden, doc_start) with packing; None on the
        first stage."""
        p = self.irecv_forward()
        return p.wait() if p is not None else None

    def send_backward(self, grad: torch.Tensor) -> None:
        p = self.isend_backward(grad)
        if p is not None:
            p.wait()

    def recv_backward(self) -> Optional[torch.Tensor]:
        p = self.irecv_backward()
        return p.wait() if p is not None else None

    # -- combined (legacy blocking 1F1B steady state) ------------------------
    def send_forward_recv_backward(self, tensor: torch.Tensor) -> Optional[torch.Tensor]:
        if self.grid.next_rank is None:
            return None
        s = self.isend_forward(tensor)
        r = self.irecv_backward()
        s.wait()
        return r.wait()

    def send_backward_recv_forward(self, grad: torch.Tensor) -> Optional[torch.Tensor]:
        if self.grid.prev_rank is None:
            return None
        s = self.isend_backward(grad)
        r = self.irecv_forward()
        s.wait()
        return r.wait()
