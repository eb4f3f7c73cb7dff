"""GPU delivery engine — HBM-resident rings via the _swarmq HIP extension.

Implements the :class:`Engine` contract over ``DeviceQueue``
(csrc/swarmq_device_queue.h): the message log, inbox rings, read cursors,
status words, visibility bitmaps and load counters all live in MI355X
HBM3E; every hot operation is one H2D staging copy + one CDNA4 kernel.

Fails loudly if the extension is missing or no GPU is visible — there is
no silent eager fallback (use CpuEngine explicitly for CPU runs).
"""

from __future__ import annotations

import sys
import threading
import time
from typing import Dict, List, Optional, Tuple

import numpy as np

from ..core.config import QueueConfig
from .device_plane import (
    MAX_DISPATCH_BACKENDS, DeviceContext, DeviceDelivery, DeviceDispatch,
    check_context_args, check_context_shared, check_dispatch_args,
    check_reply_fields, check_row_stride, delivery_stride,
)
from .engine import (
    FETCH_DTYPE, FLAG_DERIVED_ID, REC_DTYPE, ST_DELETED, ST_PROCESSED, Engine,
)

_NO_PINS = np.empty(0, dtype=np.int32)  # dispatch_delivery without pins


def _load_ext():
    try:
        from .. import _swarmq  # type: ignore
    except ImportError as e:  # pragma: no cover
        raise RuntimeError(
            "the _swarmq HIP extension is not built — run "
            "`python build_ext.py` (hipcc, gfx950). The GPU engine has no "
            "eager fallback by design."
        ) from e
    return _swarmq


class GpuEngine(Engine):
    def __init__(self, config: Optional[QueueConfig] = None):
        self.cfg = config or QueueConfig()
        c = self.cfg
        # torch carries a HIP runtime of its own, and it only finds the
        # GPU if it initialises BEFORE this extension's runtime does
        # (measured: the other order ends in "No HIP GPUs are available").
        # A process that already imported torch — any consumer of
        # receive_to_device has — gets that order here; torch stays
        # optional and is never imported on behalf of a caller without it
        torch = sys.modules.get("torch")
        if torch is not None and torch.cuda.is_available():
            torch.cuda.init()
        self._torch_dev = None  # set by _torch_device on first use
        self._out_plans: Dict[type, tuple] = {}  # see _check_out_tensors
        ext = _load_ext()
        if ext.device_count() == 0:  # pragma: no cover
            raise RuntimeError(
                "no HIP device visible — GpuEngine requires an MI355X"
            )
        if c.max_agents % 64 != 0:
            raise ValueError("max_agents must be a multiple of 64")
        self._lock = threading.RLock()
        self.q = ext.DeviceQueue(
            num_slots=c.num_slots,
            slot_bytes=c.slot_bytes,
            max_agents=c.max_agents,
            inbox_capacity=c.inbox_capacity,
            # visibility bitmaps live in an epoch-tagged ring pool:
            # alloc_bitmap returns a handle; split_bitmap_handles maps it
            # to (pool slot, epoch) and the dequeue kernel HIDES any
            # message whose slot was recycled — visibility is exact at
            # every pool depth (a recycled bitmap is never consulted)
            num_bitmaps=c.num_bitmaps,
            num_backends=c.num_backends,
            staging_batch=c.staging_batch,
            device=c.device_index,
            recv_window=c.recv_window,
        )
        self._staging = c.staging_batch
        self._slot_bytes = c.slot_bytes
        self._num_bitmaps = c.num_bitmaps
        # host-side receive-event log (processing_rate probe); one entry
        # per poll tick, pruned by age (see receive_many)
        self._recv_events: List[Tuple[float, np.ndarray, np.ndarray]] = []
        self._RECV_EVENT_RETAIN_S = 600.0  # max supported probe window

    # --- registry ---

    def register_agent(self, agent_idx: int) -> None:
        self.q.register_agent(agent_idx)

    def deregister_agent(self, agent_idx: int) -> None:
        self.q.deregister_agent(agent_idx)

    def active_agents(self) -> np.ndarray:
        return self.q.active_agents().astype(bool)

    def _chunks(self, n: int):
        """(start, stop) pairs that cover ``range(n)`` in pieces of at most
        ``staging_batch``, the most one binding call takes."""
        for start in range(0, n, self._staging):
            yield start, min(start + self._staging, n)

    # --- send plane ---

    def _pack_aligned(self, recs: np.ndarray, payloads: bytes):
        """Ensure 16-B aligned staging offsets (the enqueue kernel copies
        uint4 chunks). Repacks only when the caller's offsets aren't
        aligned already."""
        offs = recs["payload_off"]
        lens = recs["payload_len"]
        if len(recs) and (offs % 16 == 0).all():
            slack = (np.int64(len(payloads)) - (offs.astype(np.int64) + lens)).min() if len(recs) else 0
            # kernel may over-read up to the 16B round-up of each payload
            pad_needed = int(((lens + 15) // 16 * 16 - lens).max()) if len(recs) else 0
            if slack >= pad_needed:
                return recs, payloads
        aligned_lens = (lens.astype(np.int64) + 15) // 16 * 16
        new_offs = np.zeros(len(recs), dtype=np.int64)
        np.cumsum(aligned_lens[:-1], out=new_offs[1:])
        buf = np.zeros(int(aligned_lens.sum()) + 16, dtype=np.uint8)
        src = np.frombuffer(payloads, dtype=np.uint8)
        for i in range(len(recs)):
            o, l, no = int(offs[i]), int(lens[i]), int(new_offs[i])
            buf[no : no + l] = src[o : o + l]
        out = recs.copy()
        out["payload_off"] = new_offs.astype(np.uint64)
        return out, buf.tobytes()

    def split_bitmap_handles(self, recs: np.ndarray) -> np.ndarray:
        """Map raw bitmap HANDLES (what alloc_bitmap returns and callers
        put in rec['bitmap']) to (pool slot, epoch) for the kernels.
        Returns a copy when any row needs the split."""
        bm = recs["bitmap"]
        mask = (recs["vis_mode"] != 0) & (bm != 0xFFFFFFFF)
        if not mask.any():
            return recs
        out = recs.copy()
        out["bitmap_epoch"][mask] = bm[mask]
        out["bitmap"][mask] = bm[mask] % np.uint32(self._num_bitmaps)
        return out

    def unsplit_bitmap_handles(self, recs: np.ndarray) -> np.ndarray:
        """Inverse of split_bitmap_handles for records FETCHED from the
        device (e.g. migration handoff): restore the raw handle (the
        epoch IS the allocation counter) so a later enqueue re-splits
        it."""
        bm = recs["bitmap"]
        mask = (recs["vis_mode"] != 0) & (bm != 0xFFFFFFFF)
        if not mask.any():
            return recs
        out = recs.copy()
        out["bitmap"][mask] = out["bitmap_epoch"][mask]
        out["bitmap_epoch"][mask] = 0
        return out

    def enqueue_batch(self, recs: np.ndarray, payloads: bytes) -> np.ndarray:
        n = len(recs)
        if n == 0:
            return np.empty(0, dtype=np.uint64)
        recs = self.split_bitmap_handles(np.ascontiguousarray(recs))
        recs, payloads = self._pack_aligned(recs, payloads)
        pay_view = np.frombuffer(payloads, dtype=np.uint8)
        with self._lock:
            seqs = np.empty(n, dtype=np.uint64)
            for a, b in self._chunks(n):
                sub = recs[a:b]
                # offsets need not be monotonic: bound the slice by the
                # actual extremes
                lo = int(sub["payload_off"].min())
                hi = int(
                    (sub["payload_off"] + sub["payload_len"]).max()
                )
                if a or lo:
                    sub = sub.copy()
                    sub["payload_off"] -= np.uint64(lo)
                # numpy views via the buffer protocol: no bytes copies
                base = self.q.enqueue_batch(
                    sub, pay_view[lo : min(hi + 16, len(pay_view))], b - a
                )
                seqs[a:b] = np.arange(base, base + b - a, dtype=np.uint64)
            return seqs

    def alloc_bitmap(self, bits: np.ndarray) -> int:
        words = np.packbits(
            bits.astype(bool), bitorder="little"
        ).view(np.uint64)
        return int(self.q.alloc_bitmap(words.tobytes()))

    # --- receive plane ---

    def receive(
        self, agent_idx: int, max_messages: int, priority_order: bool = False
    ) -> np.ndarray:
        counts, seqs = self.receive_many(
            np.array([agent_idx], dtype=np.uint32), max_messages, priority_order
        )
        return seqs[: counts[0]]

    def receive_many(
        self,
        agent_idxs: np.ndarray,
        max_per_agent: int,
        priority_order: bool = False,
    ) -> Tuple[np.ndarray, np.ndarray]:
        agent_idxs = np.ascontiguousarray(agent_idxs, dtype=np.uint32)
        with self._lock:
            counts, flat = self.q.receive_many(
                agent_idxs, int(max_per_agent), bool(priority_order)
            )
        counts = counts.astype(np.int64)
        total = int(counts.sum())
        if total == 0:
            return counts, np.empty(0, dtype=np.uint64)
        # vectorized compaction of the dense [n_agents, K] output
        mat = flat.reshape(len(agent_idxs), max_per_agent)
        mask = np.arange(max_per_agent)[None, :] < counts[:, None]
        seqs = mat[mask]
        self._note_receive(agent_idxs, counts)
        return counts, seqs

    def _note_receive(self, agent_idxs: np.ndarray, counts: np.ndarray) -> None:
        # O(1)-per-tick receive-rate bookkeeping (processing_rate probe).
        # Prune by AGE, not entry count: a fixed-count prune truncated the
        # 60 s probe window under sustained polling (>~17 ticks/s). The
        # retention bound is _RECV_EVENT_RETAIN_S — the largest window
        # recv_rate_window supports exactly.
        now = time.time()
        self._recv_events.append((now, agent_idxs, counts))
        cutoff = now - self._RECV_EVENT_RETAIN_S
        if self._recv_events[0][0] < cutoff:
            i = 0
            for i, (t, _, _) in enumerate(self._recv_events):
                if t >= cutoff:
                    break
            del self._recv_events[:i]

    def _torch_device(self):
        """(torch, device) of the queue's GPU for the device-resident
        delivery path; a clear error when torch cannot see the GPU."""
        if self._torch_dev is None:
            import torch

            if not torch.cuda.is_available():
                raise RuntimeError(
                    "torch sees no HIP device: import torch before "
                    "constructing GpuEngine, so that torch's HIP runtime "
                    "initialises first"
                )
            self._torch_dev = (
                torch, torch.device("cuda", self.cfg.device_index))
        return self._torch_dev

    def receive_to_device(
        self,
        agent_idxs: np.ndarray,
        max_per_agent: int,
        priority_order: bool = False,
        max_payload: int = 0,
        out: Optional[DeviceDelivery] = None,
    ) -> DeviceDelivery:
        """Dequeue + device prefix scan + packed delivery into torch
        tensors on the queue's GPU, one stream-ordered submission; only
        the per-agent counts cross PCIe. The engine's stream is not one
        of torch's, so the caller's current torch stream is drained
        first (pending consumers of reused or recycled buffers) and the
        submission is synchronized before return: the tensors are safe on
        any torch stream afterwards."""
        torch, dev = self._torch_device()
        agent_idxs = np.ascontiguousarray(agent_idxs, dtype=np.uint32)
        na, K = len(agent_idxs), int(max_per_agent)
        if K < 0:
            raise ValueError("max_per_agent must be >= 0")
        stride = delivery_stride(max_payload, self._slot_bytes)
        rows = na * K
        p = {"na": na, "stride": stride, "rows": rows}
        # every refusal happens here or in the binding's own checks —
        # before the dequeue kernel moves a cursor
        if na > self.cfg.max_agents:
            raise ValueError("more polled agents than max_agents")
        if rows > self.q.out_pool():
            raise ValueError("receive batch exceeds output pool")
        if out is not None:
            # placement only, not _check_out_tensors: its dtype, rank and
            # alignment tests cost 2-4 us on every tick that reuses `out`
            buf = DeviceDelivery.reuse(
                out, p, self._check_out_placement, placement_only=True)
        else:
            buf = DeviceDelivery.fresh(p, self._make_tensor)
        torch.cuda.current_stream(dev).synchronize()
        with self._lock:
            counts = self.q.receive_to_device(
                agent_idxs, K, bool(priority_order), stride,
                buf["payload"].data_ptr(), buf["headers"].data_ptr(),
                buf["seqs"].data_ptr(), buf["lengths"].data_ptr(),
                buf["agent_row"].data_ptr(), buf["offsets"].data_ptr(),
                int(buf["payload"].shape[0]),
            )
        counts = counts.astype(np.int64)
        total = int(counts.sum())
        if total:
            self._note_receive(agent_idxs, counts)
        return DeviceDelivery(counts=counts, stride=stride, total=total, **buf)

    def ack_device(
        self, seqs, n: Optional[int] = None, status: int = ST_PROCESSED
    ) -> None:
        """One kernel over an int64 device tensor of seqs (contiguous, on
        the queue's GPU — e.g. ``delivery.seqs`` or a selection of it);
        anything else is converted to one first. Skip rules as in
        :meth:`Engine.ack_device`."""
        torch, dev = self._torch_device()
        if not isinstance(seqs, torch.Tensor):
            seqs = torch.from_numpy(
                np.ascontiguousarray(seqs).astype(np.int64).reshape(-1)
            )
        t = seqs.to(device=dev, dtype=torch.int64).contiguous().reshape(-1)
        n = t.numel() if n is None else int(n)
        if not 0 <= n <= t.numel():
            raise ValueError("n must be within 0..len(seqs)")
        if n == 0:
            return
        # the seqs may come from kernels still running on torch's stream
        torch.cuda.current_stream(dev).synchronize()
        with self._lock:
            self.q.ack_device(t.data_ptr(), n, int(status))

    # --- device-resident send ---

    def _check_device_tensor(self, name: str, t, dtype, ndim: int,
                             align: int) -> None:
        """Refuse (ValueError) anything but a contiguous, aligned tensor
        of the given dtype and rank on the queue's GPU."""
        torch, dev = self._torch_device()
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor on {dev}")
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, the queue is on {dev}")
        if t.dtype != dtype or t.dim() != ndim:
            raise ValueError(f"{name} must be {dtype} with {ndim} dimension(s)")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if t.data_ptr() % align:
            raise ValueError(f"{name} must be {align}-byte aligned")

    # array maker and array-kind tests of the result tables (DeviceResult)
    def _make_tensor(self, shape, f):
        """A fresh tensor on the queue's GPU, zeroed where the table says."""
        torch, dev = self._torch_device()
        make = torch.zeros if f.gpu_zero else torch.empty
        return make(shape, dtype=getattr(torch, f.dtype), device=dev)

    def _check_out_tensors(self, cls, tensors) -> None:
        """:meth:`_check_device_tensor` for every buffer of a ``cls``, its
        arguments resolved once per class and its tests run in line: this
        is on the tick path. A failing tensor is handed over for its message."""
        torch, dev = self._torch_device()
        plan = self._out_plans.get(cls)
        if plan is None:
            plan = self._out_plans[cls] = tuple(
                ("out." + f.name, getattr(torch, f.dtype), f.ndim, f.align)
                for f in cls.BUFFERS)
        for (name, dtype, ndim, align), t in zip(plan, tensors):
            if not (isinstance(t, torch.Tensor) and t.device == dev
                    and t.dtype == dtype and t.dim() == ndim
                    and t.is_contiguous() and t.data_ptr() % align == 0):
                self._check_device_tensor(name, t, dtype, ndim, align)

    def _check_out_placement(self, cls, tensors) -> None:
        torch, dev = self._torch_device()
        for f, t in zip(cls.BUFFERS, tensors):
            if not (isinstance(t, torch.Tensor) and t.device == dev
                    and t.is_contiguous()):
                raise ValueError(
                    f"out.{f.name} must be a contiguous tensor on {dev}")

    def _check_delivery_tensors(self, delivery: DeviceDelivery, total: int,
                                need_seqs: bool) -> None:
        """Refuse (ValueError) a delivery whose ``headers`` and
        ``agent_row`` (and ``seqs``, for a call that reads them) are not
        device tensors of at least ``total`` rows."""
        torch, _ = self._torch_device()
        if need_seqs:
            self._check_device_tensor(
                "delivery.seqs", delivery.seqs, torch.int64, 1, 8)
        self._check_device_tensor(
            "delivery.headers", delivery.headers, torch.uint8, 2, 16)
        self._check_device_tensor(
            "delivery.agent_row", delivery.agent_row, torch.int32, 1, 4)
        if (delivery.headers.shape[0] < total
                or delivery.headers.shape[1] != REC_DTYPE.itemsize
                or delivery.agent_row.shape[0] < total
                or (need_seqs and delivery.seqs.shape[0] < total)):
            raise ValueError("delivery tensors hold fewer rows than its total")

    def enqueue_from_device(self, headers, payload, n: Optional[int] = None):
        """k_stage_device + the enqueue kernels over torch tensors on the
        queue's GPU (see :meth:`Engine.enqueue_from_device`): no staging
        copy, nothing but the launches crosses PCIe. The caller's current
        torch stream is drained first (the tensors may still be being
        written) and the engine stream is synchronized before return, so
        the tensors may be overwritten at once."""
        torch, dev = self._torch_device()
        self._check_device_tensor("headers", headers, torch.uint8, 2, 16)
        self._check_device_tensor("payload", payload, torch.uint8, 2, 16)
        cap = int(headers.shape[0])
        if headers.shape[1] != REC_DTYPE.itemsize:
            raise ValueError("headers must be uint8 [cap, 48]")
        if payload.shape[0] < cap:
            raise ValueError("payload holds fewer rows than headers")
        stride = int(payload.shape[1])
        check_row_stride(stride, self._slot_bytes)
        n = cap if n is None else int(n)
        if not 0 <= n <= cap:
            raise ValueError("n must be within 0..cap")
        if n == 0:
            return np.empty(0, dtype=np.uint64)
        torch.cuda.current_stream(dev).synchronize()
        hp, pp = headers.data_ptr(), payload.data_ptr()
        with self._lock:
            base = 0
            for a, b in self._chunks(n):
                first = self.q.enqueue_from_device(
                    hp + a * REC_DTYPE.itemsize, pp + a * stride, b - a, stride,
                )
                base = base if a else first
        return np.arange(base, base + n, dtype=np.uint64)

    def reply_to_device(
        self,
        delivery: DeviceDelivery,
        agent_idxs: np.ndarray,
        payload,
        lengths,
        type_code: int,
        priority: Optional[int] = None,
        flags: int = FLAG_DERIVED_ID,
        timestamp: Optional[float] = None,
    ) -> np.ndarray:
        """k_build_replies + the enqueue kernels over the delivery's own
        tensors and the caller's reply tensors (see
        :meth:`Engine.reply_to_device`). Only the polled agents go to
        the device and only the reply count comes back (4 B per
        ``staging_batch`` rows). Stream contract as in
        :meth:`enqueue_from_device`."""
        torch, dev = self._torch_device()
        agent_idxs = np.ascontiguousarray(agent_idxs, dtype=np.uint32)
        total = int(delivery.total)
        if len(agent_idxs) != len(delivery.counts):
            raise ValueError("agent_idxs must be the polled list of the delivery")
        if len(agent_idxs) and int(agent_idxs.max()) >= self.cfg.max_agents:
            raise ValueError("agent index out of range")
        self._check_delivery_tensors(delivery, total, need_seqs=False)
        self._check_device_tensor("payload", payload, torch.uint8, 2, 16)
        self._check_device_tensor("lengths", lengths, torch.int32, 1, 4)
        if payload.shape[0] < total or lengths.shape[0] < total:
            raise ValueError(
                "payload / lengths hold fewer rows than the delivery")
        rstride = int(payload.shape[1])
        check_row_stride(rstride, self._slot_bytes)
        code, prio, flags = check_reply_fields(type_code, priority, flags)
        ts = time.time() if timestamp is None else float(timestamp)
        if total == 0:
            return np.empty(0, dtype=np.uint64)
        torch.cuda.current_stream(dev).synchronize()
        hp, rp = delivery.headers.data_ptr(), delivery.agent_row.data_ptr()
        lp, pp = lengths.data_ptr(), payload.data_ptr()
        with self._lock:
            base = m = 0
            for a, b in self._chunks(total):
                first, mc = self.q.reply_from_device(
                    hp + a * REC_DTYPE.itemsize, rp + a * 4, lp + a * 4,
                    pp + a * rstride, b - a, rstride,
                    agent_idxs, code, prio, flags, ts,
                )
                base = base if a else first
                m += int(mc)
        return np.arange(base, base + m, dtype=np.uint64)

    def peek_inbox(self, agent_idx: int) -> np.ndarray:
        _, entries = self.q.inbox_window(int(agent_idx))
        entries = np.asarray(entries, dtype=np.uint64)
        if len(entries) == 0:
            return entries
        entries = np.sort(entries)
        eb = self.q.evict_base()
        entries = entries[entries >= eb]
        if len(entries) == 0:
            return entries
        # drop tombstoned
        return entries[self.statuses(entries) != ST_DELETED]

    def unread_count(self, agent_idx: int) -> int:
        out = self.q.unread_counts(np.array([agent_idx], dtype=np.uint32))
        return int(out[0])

    # --- message store ---

    def _fetch(self, seqs: np.ndarray, keep) -> np.ndarray:
        """Headers, statuses and seqs of ``seqs`` as one FETCH_DTYPE
        array, a chunk at a time; ``keep(a, b, hdr, pay_b)`` takes each
        chunk's payload rows (``slot_bytes`` apart in ``pay_b``)."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint64)
        out = np.zeros(len(seqs), dtype=FETCH_DTYPE)
        for a, b in self._chunks(len(seqs)):
            hdr_b, status, pay_b = self.q.fetch(seqs[a:b])
            hdr = np.frombuffer(hdr_b, dtype=REC_DTYPE, count=b - a)
            for name in REC_DTYPE.names:
                out[name][a:b] = hdr[name]
            out["status"][a:b] = status.astype(np.uint8)
            out["seq"][a:b] = seqs[a:b]
            keep(a, b, hdr, pay_b)
        return out

    def fetch(self, seqs: np.ndarray) -> Tuple[np.ndarray, List[bytes]]:
        pays: List[bytes] = []
        sb = self._slot_bytes

        def keep(a, b, hdr, pay_b):
            lens = hdr["payload_len"]
            pays.extend(
                pay_b[i * sb : i * sb + int(lens[i])] for i in range(b - a)
            )

        return self._fetch(seqs, keep), pays

    def fetch_raw_chunks(self, seqs: np.ndarray):
        """Device gather + one pinned D2H per chunk; no per-message
        Python objects (the binary-checkpoint hot path)."""
        stride = self._slot_bytes
        flat = np.empty((len(seqs), stride), dtype=np.uint8)

        def keep(a, b, hdr, pay_b):
            flat[a:b] = np.frombuffer(
                pay_b, dtype=np.uint8, count=(b - a) * stride
            ).reshape(b - a, stride)

        return self._fetch(seqs, keep), flat.reshape(-1), stride

    def read_bitmap(self, slot: int, epoch: int):
        ep, words = self.q.get_bitmap(int(slot))
        if int(ep) != int(epoch):
            return None
        bits = np.unpackbits(
            np.frombuffer(words, dtype=np.uint8), bitorder="little"
        )
        return bits.astype(bool)[: self.cfg.max_agents]

    def deliver_payloads(
        self, seqs: np.ndarray, max_payload: int = 0, synchronize: bool = True
    ) -> int:
        """Gather + D2H the payloads of `seqs` into pinned host memory
        (the delivery step of the hot path) without building per-message
        Python objects. `max_payload` (if known) tightens the D2H stride
        below slot_bytes. With synchronize=False the D2H stays in flight
        on the copy stream and overlaps the next tick's H2D (full-duplex
        PCIe); call delivery_sync() (or any sync'd delivery) to drain.
        Returns bytes landed (an upper bound when async)."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint64)
        n = len(seqs)
        total = 0
        for a, b in self._chunks(n):
            total += int(
                self.q.fetch_raw(
                    seqs[a:b], int(max_payload), synchronize and b >= n
                )
            )
        return total

    def delivery_sync(self) -> None:
        self.q.delivery_sync()

    def set_status(self, seq: int, status: int) -> None:
        self.q.set_status(int(seq), int(status))

    def get_status(self, seq: int) -> int:
        return int(self.q.get_status(int(seq)))

    def set_statuses(self, seqs: np.ndarray, statuses: np.ndarray) -> None:
        seqs = np.ascontiguousarray(seqs, dtype=np.uint64)
        statuses = np.ascontiguousarray(statuses, dtype=np.uint32)
        for a, b in self._chunks(len(seqs)):
            self.q.set_statuses(seqs[a:b], statuses[a:b])

    def statuses(self, seqs: np.ndarray) -> np.ndarray:
        seqs = np.ascontiguousarray(seqs, dtype=np.uint64)
        out = np.empty(len(seqs), dtype=np.uint8)
        for a, b in self._chunks(len(seqs)):
            out[a:b] = self.q.get_statuses(seqs[a:b]).astype(np.uint8)
        return out

    def query(
        self,
        sender: Optional[int] = None,
        receiver: Optional[int] = None,
        type_code: Optional[int] = None,
        status: Optional[int] = None,
        after: Optional[float] = None,
        before: Optional[float] = None,
        limit: int = 100,
    ) -> np.ndarray:
        mask = 0
        if sender is not None:
            mask |= 1
        if receiver is not None:
            mask |= 2
        if type_code is not None:
            mask |= 4
        if status is not None:
            mask |= 8
        if after is not None:
            mask |= 16
        if before is not None:
            mask |= 32
        limit = min(int(limit), self._staging)
        args = (
            -1 if sender is None else int(sender),
            -1 if receiver is None else int(receiver),
            -1 if type_code is None else int(type_code),
            -1 if status is None else int(status),
            0.0 if after is None else float(after),
            0.0 if before is None else float(before),
            mask,
            self._staging,
        )
        return self._scan_newest_first(
            lambda lo, hi: self.q.query_range(lo, hi, *args),
            max(1 << 20, limit), limit, np.sort,
        )

    def search(self, needle: bytes, case_sensitive: bool, limit: int) -> np.ndarray:
        # the linear-scan kernel may report a message once per matching
        # chunk: np.unique dedups as it sorts
        return self._scan_newest_first(
            lambda lo, hi: self.q.search_range(
                lo, hi, needle, not case_sensitive, self._staging
            ),
            1 << 20, min(int(limit), self._staging), np.unique,
        )

    def _scan_newest_first(self, scan, window: int, limit: int, order):
        """Up to ``limit`` matches of ``scan(lo, hi)``, newest first.
        Windows of ``window`` seqs are scanned from the newest down until
        the limit fills; if a window overflows the match buffer the subset
        is arbitrary, so the window shrinks until it fits (newest-first
        stays exact). ``order`` sorts one window's matches ascending."""
        eb = self.q.evict_base()
        hi = self.q.total_messages()
        found: List[np.ndarray] = []
        nfound = 0
        while hi > eb and nfound < limit:
            lo = max(eb, hi - window)
            seqs = scan(lo, hi)
            if len(seqs) >= self._staging and hi - lo > 1:
                window = max(1, window // 4)
                continue
            seqs = order(np.asarray(seqs, dtype=np.uint64))[::-1]
            found.append(seqs)
            nfound += len(seqs)
            hi = lo
        if not found:
            return np.empty(0, dtype=np.uint64)
        return np.concatenate(found)[:limit]

    def delete(self, seq: int) -> bool:
        if self.get_status(seq) == ST_DELETED:
            return False
        self.set_status(int(seq), ST_DELETED)
        return True

    # --- counters / stats ---

    def total_messages(self) -> int:
        return int(self.q.total_messages())

    def evict_base(self) -> int:
        return int(self.q.evict_base())

    def stats_arrays(self) -> Dict[str, np.ndarray]:
        c = self.q.counters()
        return {
            "by_type": np.asarray(c["by_type"], dtype=np.int64),
            "by_status": np.asarray(c["by_status"], dtype=np.int64),
            "sent": np.asarray(c["sent"], dtype=np.int64),
            "received": np.asarray(c["received"], dtype=np.int64),
            # inbox-ring overwrites of unexamined entries (slow-consumer
            # loss — the CPU engine's unbounded inboxes never drop)
            "dropped": int(c["dropped"]),
        }

    def recv_rate_window(self, agent_idx: int, window_s: float) -> int:
        cutoff = time.time() - window_s
        total = 0
        for t, agents, counts in reversed(self._recv_events):
            if t < cutoff:
                break
            hit = counts[agents == agent_idx]
            if len(hit):
                total += int(hit.sum())
        return total

    # --- load balancer ---

    def backend_add_load(self, backend_idx: int, delta: int) -> None:
        self.q.backend_add_load(int(backend_idx), int(delta))

    def backend_loads(self) -> np.ndarray:
        return np.asarray(self.q.backend_loads(), dtype=np.int64)

    def least_loaded_backend(self, n_backends: int) -> int:
        loads = self.backend_loads()[:n_backends]
        return int(np.argmin(loads))

    def dispatch_batch(self, requests: int, n_backends: int) -> np.ndarray:
        """Batched exact least-loaded dispatch — the wavefront min-reduce
        kernel (BASELINE config 5)."""
        return np.asarray(
            self.q.lb_dispatch(int(requests), int(n_backends)), dtype=np.uint32
        )

    # --- device-resident dispatch ---

    def dispatch_delivery(
        self,
        delivery: DeviceDelivery,
        n_backends: int,
        weight: str = "requests",
        type_code: Optional[int] = None,
        pinned=None,
        out: Optional[DeviceDispatch] = None,
    ) -> DeviceDispatch:
        """k_dispatch_rows + k_dispatch_scatter over the delivery's own
        tensors (see :meth:`Engine.dispatch_delivery`): the serial greedy
        walk runs in one wavefront on the balancer's stream, the result
        stays in torch tensors on the queue's GPU. Only ``pinned`` goes to
        the device and only the per-backend row counts come back. The
        caller's current torch stream is drained first (the delivery's
        tensors may still be being written) and the balancer's stream is
        synchronized before return."""
        torch, dev = self._torch_device()
        na = len(delivery.counts)
        total = int(delivery.total)
        nb, by_tokens, code, pins = check_dispatch_args(
            n_backends, self.cfg.num_backends, weight, type_code, pinned, na
        )
        if na > self.cfg.max_agents:
            raise ValueError("more polled agents than max_agents")
        self._check_delivery_tensors(delivery, total, need_seqs=False)
        p = {"n_backends": nb, "rows": total}
        if out is not None:
            buf = DeviceDispatch.reuse(out, p, self._check_out_tensors)
        else:
            p["rows"] = int(delivery.agent_row.shape[0])
            buf = DeviceDispatch.fresh(p, self._make_tensor)
        torch.cuda.current_stream(dev).synchronize()
        with self._lock:
            counts = self.q.dispatch_from_device(
                delivery.headers.data_ptr(), delivery.agent_row.data_ptr(),
                total, pins if pins is not None else _NO_PINS,
                pins is not None, nb, code, by_tokens,
                buf["backend"].data_ptr(), buf["rank"].data_ptr(),
                buf["order"].data_ptr(), buf["offsets"].data_ptr(),
                buf["added"].data_ptr(),
            )
        counts = np.asarray(counts, dtype=np.int64)
        return DeviceDispatch(
            counts=counts, n_backends=nb, total=total, m=int(counts.sum()),
            **buf)

    def release_dispatch(self, dispatch: DeviceDispatch) -> None:
        """k_release_loads over the dispatch's own ``added`` tensor, on
        the balancer's stream (see :meth:`Engine.release_dispatch`)."""
        torch, dev = self._torch_device()
        if dispatch.released:
            raise ValueError("dispatch was already released")
        nb = int(dispatch.n_backends)
        if not 1 <= nb <= min(MAX_DISPATCH_BACKENDS, self.cfg.num_backends):
            raise ValueError("dispatch has an unusable n_backends")
        self._check_device_tensor(
            "dispatch.added", dispatch.added, torch.int64, 1, 8)
        if dispatch.added.shape[0] != nb:
            raise ValueError("dispatch.added must hold n_backends entries")
        torch.cuda.current_stream(dev).synchronize()
        with self._lock:
            self.q.release_dispatch(dispatch.added.data_ptr(), nb)
        dispatch.released = True

    # --- device-resident conversation context ---

    def context_to_device(
        self,
        delivery: DeviceDelivery,
        agent_idxs: np.ndarray,
        depth: int,
        lookback: int,
        type_code: Optional[int] = None,
        max_payload: int = 0,
        out: Optional[DeviceContext] = None,
        group: int = 0,
        *,
        shared: bool = False,
    ) -> DeviceContext:
        """k_context_find + k_context_gather over the delivery's own
        tensors and the HBM-resident log (see
        :meth:`Engine.context_to_device`): the result stays in torch
        tensors on the queue's GPU, only the polled agents go to the
        device and no byte comes back. ``group`` picks the delivery rows
        one workgroup shares a log pass among (0: the built default,
        ``_swarmq.CONTEXT_GROUP``, one row per wavefront; 16: four, for
        measurement). ``shared`` picks the instantiation that checks
        visibility against the bitmap pool and its epochs in the kernel;
        with the default ``False`` the kernel that runs is the one that
        always ran. The caller's current torch stream is drained first
        (the delivery's tensors may still be being written) and the
        engine's stream is synchronized before return."""
        torch, dev = self._torch_device()
        shared = check_context_shared(shared)
        total = int(delivery.total)
        depth, lookback, code, agents = check_context_args(
            depth, lookback, type_code, agent_idxs, len(delivery.counts),
            self.cfg.max_agents,
        )
        stride = delivery_stride(max_payload, self._slot_bytes)
        self._check_delivery_tensors(delivery, total, need_seqs=True)
        ext = _load_ext()
        if group not in (0, ext.CONTEXT_GROUP, ext.CONTEXT_GROUP_WIDE):
            raise ValueError("group must be 0, 4 or 16")
        D = depth
        p = {"depth": D, "stride": stride, "rows": total}
        if out is not None:
            buf = DeviceContext.reuse(out, p, self._check_out_tensors)
        else:
            p["rows"] = int(delivery.agent_row.shape[0])
            buf = DeviceContext.fresh(p, self._make_tensor)
        if total:
            torch.cuda.current_stream(dev).synchronize()
            with self._lock:
                self.q.context_to_device(
                    delivery.seqs.data_ptr(), delivery.agent_row.data_ptr(),
                    delivery.headers.data_ptr(), total, agents, D, lookback,
                    code, stride, buf["counts"].data_ptr(),
                    buf["seqs"].data_ptr(), buf["lengths"].data_ptr(),
                    buf["headers"].data_ptr(), buf["payload"].data_ptr(),
                    int(group), shared,
                )
        return DeviceContext(depth=D, stride=stride, total=total, **buf)

    # --- lifecycle ---

    def close(self) -> None:
        self.q.release()
