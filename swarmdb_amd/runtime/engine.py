"""Delivery-engine interface + shared record layout.

The engine is the MI355X-native replacement for the reference's Kafka tier
(librdkafka producer/consumer + broker, reference swarmdb/ main.py:192-207,
334-345, 476-484, 553-571). It owns:

- the message slot store (payload bytes + binary routing header),
- per-agent inbox rings with read cursors,
- delivery status words,
- visibility bitmaps for restricted broadcasts,
- per-agent / per-backend load counters.

Two engines implement it: :class:`~swarmdb_amd.runtime.cpu_engine.CpuEngine`
(numpy, runs anywhere — the permanent test double, BASELINE config 1) and
:class:`~swarmdb_amd.runtime.gpu_engine.GpuEngine` (HBM-resident rings with
HIP kernels via the ``_swarmq`` extension).

The batch record layout (``REC_DTYPE``) is the host-side staging format:
callers build arrays of records + one contiguous payload buffer, and the
engine enqueues the whole batch in one shot (one pinned-memcpy + one kernel
on GPU). This replaces the reference's per-message produce path
(swarmdb/ main.py:466-484) with a batched one.
"""

from __future__ import annotations

import abc
import time
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

# ---- wire constants (must match csrc/swarmq_common.h) ----

BROADCAST = 0xFFFFFFFF  # receiver index meaning "broadcast"
NO_BITMAP = 0xFFFFFFFF  # bitmap index meaning "no visibility restriction"

# status codes (device status word). Order matters: the reference lifecycle
# pending -> delivered -> read -> processed, + failed (swarmdb/ main.py:44-51)
ST_PENDING = 0
ST_DELIVERED = 1
ST_READ = 2
ST_PROCESSED = 3
ST_FAILED = 4
ST_DELETED = 5  # tombstone (delete_message / flush_old_messages)

STATUS_NAMES = ["pending", "delivered", "read", "processed", "failed", "deleted"]

# message type codes (index into TYPE_NAMES = MessageType order)
TYPE_NAMES = [
    "chat",
    "command",
    "function_call",
    "function_result",
    "system",
    "error",
    "status",
]
TYPE_CODES = {n: i for i, n in enumerate(TYPE_NAMES)}

# visibility modes
VIS_ALL = 0      # no restriction (visible_to empty)
VIS_BITMAP = 1   # restricted: agent must be set in the bitmap (inbox entry
#                  still lands in every inbox, filtered at dequeue — the
#                  reference's broadcast-listing behavior)
VIS_GROUP = 2    # group fan-out: inbox entries land ONLY in member inboxes
#                  (one slot per group message; the fan-out kernel filters)

# record flags
FLAG_HAS_EXTRAS = 1   # payload tail carries an extras-JSON blob
FLAG_JSON_CONTENT = 2  # content bytes are JSON (dict/list), else raw utf-8 str
FLAG_DERIVED_ID = 4   # message id is derived from (rank, seq), no extras id
FLAG_OVERFLOW = 8     # payload exceeds the slot capacity and lives in the
#                       facade's host-side overflow store (device slot empty;
#                       not visible to the device search kernel)

# per-message batch record (host staging). 48 bytes, 8-byte aligned.
# Payload layout: [content bytes (content_len)][extras JSON (rest)] —
# search scans only the content window (reference searches the content
# field only, swarmdb/ main.py:742-781). Enqueue stores content_len =
# min(content_len, payload_len): see Engine's docstring.
REC_DTYPE = np.dtype(
    {
        "names": [
            "sender", "receiver", "type", "priority", "vis_mode", "flags",
            "token_count", "timestamp", "payload_off", "payload_len", "bitmap",
            "content_len", "bitmap_epoch",
        ],
        "formats": [
            np.uint32, np.uint32, np.uint8, np.uint8, np.uint8, np.uint8,
            np.uint32, np.float64, np.uint64, np.uint32, np.uint32,
            np.uint32, np.uint32,
        ],
        "offsets": [0, 4, 8, 9, 10, 11, 12, 16, 24, 32, 36, 40, 44],
        "itemsize": 48,
    }
)


def _to_numpy(x: Any) -> np.ndarray:
    """Host copy of a numpy array or of a torch tensor (duck-typed: torch
    is optional and must not be imported on the CPU path)."""
    if hasattr(x, "detach"):
        return x.detach().cpu().numpy()
    return np.array(x, copy=True)


@dataclass
class DeviceDelivery:
    """One poll tick delivered as packed, engine-resident arrays.

    Message ``i`` of polled agent ``b`` sits in row ``r = offsets[b] + i``;
    rows ``[0, total)`` are defined, the buffers may be longer (capacity
    ``len(counts) * max_per_agent``). On the GPU engine every array but
    ``counts`` is a ``torch.Tensor`` in HBM on the queue's device — a
    model on the same GPU reads its inbox without a PCIe crossing; on the
    CPU engine they are numpy arrays with the same dtypes and layout.
    ``counts`` is the one thing the GPU engine brings to the host
    (``4 * len(counts)`` bytes), so it is a host int64 array on both.

    - ``counts``     int64 [na]      messages delivered per polled agent
    - ``offsets``    int32 [na + 1]  exclusive prefix sum, ``[na] == total``
    - ``seqs``       int64 [rows]    sequence numbers
    - ``lengths``    int32 [rows]    ``min(payload_len, stride)``
    - ``agent_row``  int32 [rows]    position ``b`` in the polled list
    - ``headers``    uint8 [rows,48] REC_DTYPE records, ``payload_off``
      rebased to ``r * stride`` (into ``payload``, flattened)
    - ``payload``    uint8 [rows, stride], zero from ``lengths[r]`` on
    """

    counts: Any
    offsets: Any
    seqs: Any
    lengths: Any
    agent_row: Any
    headers: Any
    payload: Any
    stride: int
    total: int

    def to_host(self) -> "DeviceDelivery":
        """Copy with numpy arrays, trimmed to ``total`` rows; ``headers``
        comes back as a REC_DTYPE array."""
        t = self.total
        headers = np.ascontiguousarray(_to_numpy(self.headers[:t]))
        return DeviceDelivery(
            counts=_to_numpy(self.counts),
            offsets=_to_numpy(self.offsets),
            seqs=_to_numpy(self.seqs[:t]),
            lengths=_to_numpy(self.lengths[:t]),
            agent_row=_to_numpy(self.agent_row[:t]),
            headers=headers.view(REC_DTYPE).reshape(-1),
            payload=_to_numpy(self.payload[:t]),
            stride=self.stride,
            total=t,
        )


@dataclass
class DeviceDispatch:
    """The rows of a :class:`DeviceDelivery` dispatched to LLM backends
    (:meth:`Engine.dispatch_delivery`). On the GPU engine every array but
    ``counts`` is a ``torch.Tensor`` in HBM on the queue's device; on the
    CPU engine they are numpy arrays with the same dtypes. ``counts`` is
    the one thing the GPU engine brings to the host (``4 * n_backends``
    bytes).

    - ``backend``  int32 [rows]  chosen backend per row, ``-1`` for a row
      the type filter skipped; defined for ``[0, total)``
    - ``order``    int32 [rows]  the dispatched rows grouped by backend, in
      row order within a backend; defined for ``[0, m)``
    - ``offsets``  int32 [n_backends + 1]  exclusive prefix sum:
      ``order[offsets[k]:offsets[k+1]]`` are backend ``k``'s rows,
      ``offsets[n_backends] == m``
    - ``added``    int64 [n_backends]  load this dispatch put on each backend
    - ``counts``   host int64 [n_backends]  rows per backend
    - ``rank``     int32 [rows]  scratch: a row's position within its backend

    ``backend[total:]``, ``order[m:]`` and ``rank`` past ``total`` are
    unspecified. ``released`` is set by :meth:`Engine.release_dispatch`;
    ``backend_ids`` (the backend names in index order) by the facade.
    """

    backend: Any
    order: Any
    offsets: Any
    added: Any
    counts: Any
    rank: Any
    n_backends: int
    total: int
    m: int
    released: bool = False
    backend_ids: Optional[List[str]] = None

    def to_host(self) -> "DeviceDispatch":
        """Copy with numpy arrays, trimmed to the defined ranges."""
        return DeviceDispatch(
            backend=_to_numpy(self.backend[: self.total]),
            order=_to_numpy(self.order[: self.m]),
            offsets=_to_numpy(self.offsets[: self.n_backends + 1]),
            added=_to_numpy(self.added[: self.n_backends]),
            counts=_to_numpy(self.counts),
            rank=_to_numpy(self.rank[: self.total]),
            n_backends=self.n_backends,
            total=self.total,
            m=self.m,
            released=self.released,
            backend_ids=self.backend_ids,
        )


MAX_DISPATCH_BACKENDS = 64  # one wavefront lane per backend

DISPATCH_WEIGHTS = ("requests", "tokens")


def check_dispatch_args(
    n_backends: int,
    num_backends: int,
    weight: str,
    type_code: Optional[int],
    pinned: Any,
    n_agents: int,
) -> Tuple[int, bool, int, Optional[np.ndarray]]:
    """(n_backends, by_tokens, type code or -1 for 'no filter', pinned as
    int32 [n_agents] or None) of :meth:`Engine.dispatch_delivery`, or
    ValueError."""
    nb = int(n_backends)
    if not 1 <= nb <= min(MAX_DISPATCH_BACKENDS, int(num_backends)):
        raise ValueError(
            f"n_backends must be within 1.."
            f"{min(MAX_DISPATCH_BACKENDS, int(num_backends))}"
        )
    if weight not in DISPATCH_WEIGHTS:
        raise ValueError(f"weight must be one of {DISPATCH_WEIGHTS}")
    code = -1
    if type_code is not None:
        code = int(type_code)
        if not 0 <= code <= 255:
            raise ValueError("type_code is one byte")
    pins = None
    if pinned is not None:
        raw = np.asarray(pinned)
        if raw.ndim != 1 or len(raw) != n_agents:
            raise ValueError(
                "pinned must hold one entry per polled agent of the delivery"
            )
        if raw.dtype.kind not in "iu":
            raise ValueError("pinned must be an integer array")
        if len(raw) and (raw.min() < -1 or raw.max() >= nb):
            raise ValueError(f"pinned entries must be within -1..{nb - 1}")
        pins = np.ascontiguousarray(raw, dtype=np.int32)
    return nb, weight == "tokens", code, pins


def check_dispatch_out(out: "DeviceDispatch", n_backends: int, total: int) -> None:
    """Refuse (ValueError) a reused dispatch built for another
    ``n_backends`` or with fewer than ``total`` rows."""
    if not isinstance(out, DeviceDispatch):
        raise ValueError("out must be a DeviceDispatch")
    if out.n_backends != n_backends or len(out.offsets) != n_backends + 1 \
            or len(out.added) != n_backends:
        raise ValueError(
            f"out was built for {out.n_backends} backends, "
            f"this call needs {n_backends}"
        )
    for name in ("backend", "order", "rank"):
        if len(getattr(out, name)) < total:
            raise ValueError(
                f"out.{name} holds {len(getattr(out, name))} rows, "
                f"this call needs {total}"
            )


@dataclass
class DeviceContext:
    """The conversation context of every row of a :class:`DeviceDelivery`
    (:meth:`Engine.context_to_device`): for row ``r``, the newest
    ``depth`` messages exchanged between the polled agent and the row's
    sender, oldest first. Slots are fixed — row ``r``, slot ``j`` — so
    there is no prefix sum and no count to read back. On the GPU engine
    every array is a ``torch.Tensor`` in HBM on the queue's device; on the
    CPU engine they are numpy arrays with the same dtypes and layout.

    - ``counts``   int32 [rows]        defined slots of the row
    - ``seqs``     int64 [rows, D]     ascending; ``-1`` from ``counts[r]`` on
    - ``lengths``  int32 [rows, D]     ``min(payload_len, stride)``; ``0``
      in undefined slots
    - ``headers``  uint8 [rows, D, 48] REC_DTYPE records, ``payload_off``
      rebased to ``(r * D + j) * stride`` (into ``payload``, flattened)
    - ``payload``  uint8 [rows, D, stride], zero from ``lengths[r, j]`` on

    ``headers`` and ``payload`` of undefined slots, and everything at rows
    ``>= total``, are unspecified.

    A gathered header is the log's record as stored. With ``shared=True``
    a slot may hold a message of restricted visibility: on the GPU engine
    its ``bitmap`` is the pool slot and its ``bitmap_epoch`` the
    :meth:`Engine.alloc_bitmap` handle, on the CPU engine ``bitmap`` is
    the index and ``bitmap_epoch`` is 0 — the two fields in which the
    engines' contexts of the same traffic legitimately differ.
    """

    counts: Any
    seqs: Any
    lengths: Any
    headers: Any
    payload: Any
    depth: int
    stride: int
    total: int

    def to_host(self) -> "DeviceContext":
        """Copy with numpy arrays, trimmed to ``total`` rows; ``headers``
        comes back as a REC_DTYPE array ``[total, D]``."""
        t = self.total
        headers = np.ascontiguousarray(_to_numpy(self.headers[:t]))
        if headers.dtype != REC_DTYPE:
            headers = headers.view(REC_DTYPE)
        return DeviceContext(
            counts=_to_numpy(self.counts[:t]),
            seqs=_to_numpy(self.seqs[:t]),
            lengths=_to_numpy(self.lengths[:t]),
            headers=headers.reshape(t, self.depth),
            payload=_to_numpy(self.payload[:t]),
            depth=self.depth,
            stride=self.stride,
            total=t,
        )


MAX_CONTEXT_DEPTH = 64  # one wavefront lane per context slot


def check_context_args(
    depth: int,
    lookback: int,
    type_code: Optional[int],
    agent_idxs: Any,
    n_polled: int,
    max_agents: int,
) -> Tuple[int, int, int, np.ndarray]:
    """(depth, lookback, type code or -1 for 'no filter', polled agents as
    uint32 [na]) of :meth:`Engine.context_to_device`, or ValueError."""
    depth, lookback = int(depth), int(lookback)
    if not 1 <= depth <= MAX_CONTEXT_DEPTH:
        raise ValueError(f"depth must be within 1..{MAX_CONTEXT_DEPTH}")
    if not 1 <= lookback <= 2 ** 31 - 1:
        raise ValueError("lookback must be within 1..2**31-1")
    code = -1
    if type_code is not None:
        code = int(type_code)
        if not 0 <= code <= 255:
            raise ValueError("type_code is one byte")
    raw = np.asarray(agent_idxs)
    if raw.ndim != 1 or len(raw) != n_polled:
        raise ValueError("agent_idxs must be the polled list of the delivery")
    if len(raw) > max_agents:
        raise ValueError("more polled agents than max_agents")
    if len(raw) and raw.dtype.kind not in "iu":
        raise ValueError("agent_idxs must be an integer array")
    if len(raw) and (raw.min() < 0 or raw.max() > 0xFFFFFFFF):
        raise ValueError("agent index out of range")
    return depth, lookback, code, np.ascontiguousarray(raw, dtype=np.uint32)


def check_context_shared(shared: Any) -> bool:
    """``shared`` of :meth:`Engine.context_to_device`: a ``bool`` and
    nothing else (``1`` or ``"yes"`` is a ValueError — the flag picks
    another rule, so a truthy accident must not)."""
    if not isinstance(shared, (bool, np.bool_)):
        raise ValueError("shared must be a bool")
    return bool(shared)


def check_context_out(
    out: "DeviceContext", depth: int, stride: int, total: int
) -> None:
    """Refuse (ValueError) a reused context built for another ``depth`` or
    ``stride``, or with fewer than ``total`` rows."""
    if not isinstance(out, DeviceContext):
        raise ValueError("out must be a DeviceContext")
    if out.depth != depth or out.stride != stride:
        raise ValueError(
            f"out was built for depth {out.depth} and stride {out.stride}, "
            f"this call needs {depth} and {stride}"
        )
    shapes = {
        "counts": (), "seqs": (depth,), "lengths": (depth,),
        "headers": (depth, REC_DTYPE.itemsize), "payload": (depth, stride),
    }
    for name, tail in shapes.items():
        a = getattr(out, name)
        shape = tuple(getattr(a, "shape", ()))
        if len(shape) != len(tail) + 1 or shape[1:] != tail:
            want = ", ".join(["rows"] + [str(d) for d in tail])
            raise ValueError(f"out.{name} must have shape [{want}]")
        if shape[0] < total:
            raise ValueError(
                f"out.{name} holds {shape[0]} rows, this call needs {total}"
            )


def delivery_stride(max_payload: int, slot_bytes: int) -> int:
    """Row stride of a device-resident delivery: ``max_payload`` rounded up
    to 16 B when it tightens the row below ``slot_bytes``."""
    if 0 < max_payload < slot_bytes:
        return (int(max_payload) + 15) // 16 * 16
    return int(slot_bytes)


def check_delivery_out(
    out: DeviceDelivery, n_agents: int, rows: int, stride: int
) -> None:
    """Refuse (ValueError) a reused delivery whose buffers cannot hold a
    poll of ``n_agents`` x ``rows / n_agents``. Runs BEFORE any dequeue."""
    if out.stride != stride:
        raise ValueError(
            f"out has stride {out.stride}, this call needs {stride}"
        )
    if len(out.offsets) < n_agents + 1:
        raise ValueError("out.offsets is too small for the polled agents")
    for name in ("seqs", "lengths", "agent_row", "headers", "payload"):
        if len(getattr(out, name)) < rows:
            raise ValueError(
                f"out.{name} holds {len(getattr(out, name))} rows, "
                f"this call needs {rows}"
            )


# payload_len a device-side record is staged with when its length does
# not fit its payload row: above every slot_bytes, so the enqueue's own
# validation parks it in the error lane
OVERSIZE_LEN = 0xFFFFFFFF


def check_row_stride(stride: int, slot_bytes: int) -> None:
    """Row-stride rule of the device-resident planes (ValueError)."""
    if stride < 16 or stride > slot_bytes or stride % 16:
        raise ValueError(
            f"stride {stride} is not a multiple of 16 in 16..{slot_bytes}"
        )


def check_send_arrays(
    headers: Any, payload: Any, n: Optional[int], slot_bytes: int
) -> Tuple[np.ndarray, np.ndarray, int, int]:
    """Host-array form of the :meth:`Engine.enqueue_from_device`
    arguments: (REC_DTYPE records [cap], uint8 payload [cap, stride], n,
    stride), or ValueError."""
    for name, a in (("headers", headers), ("payload", payload)):
        if not isinstance(a, np.ndarray) or not a.flags.c_contiguous:
            raise ValueError(f"{name} must be a contiguous numpy array")
    if headers.dtype == REC_DTYPE and headers.ndim == 1:
        recs = headers
    elif (headers.dtype == np.uint8 and headers.ndim == 2
          and headers.shape[1] == REC_DTYPE.itemsize):
        recs = headers.view(REC_DTYPE).reshape(-1)
    else:
        raise ValueError("headers must be uint8 [cap, 48] or REC_DTYPE [cap]")
    if payload.dtype != np.uint8 or payload.ndim != 2:
        raise ValueError("payload must be uint8 [cap, stride]")
    cap = len(recs)
    if payload.shape[0] < cap:
        raise ValueError("payload holds fewer rows than headers")
    check_row_stride(int(payload.shape[1]), slot_bytes)
    n = cap if n is None else int(n)
    if not 0 <= n <= cap:
        raise ValueError("n must be within 0..cap")
    return recs, payload, n, int(payload.shape[1])


def check_reply_arrays(
    payload: Any, lengths: Any, total: int, slot_bytes: int
) -> Tuple[np.ndarray, np.ndarray, int]:
    """Host-array form of the reply tensors of
    :meth:`Engine.reply_to_device`: (uint8 payload [>= total, rstride],
    int32 lengths [>= total], rstride), or ValueError."""
    for name, a in (("payload", payload), ("lengths", lengths)):
        if not isinstance(a, np.ndarray) or not a.flags.c_contiguous:
            raise ValueError(f"{name} must be a contiguous numpy array")
    if payload.dtype != np.uint8 or payload.ndim != 2:
        raise ValueError("payload must be uint8 [rows, rstride]")
    if lengths.dtype != np.int32 or lengths.ndim != 1:
        raise ValueError("lengths must be int32 [rows]")
    if payload.shape[0] < total or lengths.shape[0] < total:
        raise ValueError("payload / lengths hold fewer rows than the delivery")
    check_row_stride(int(payload.shape[1]), slot_bytes)
    return payload, lengths, int(payload.shape[1])


def check_reply_fields(
    type_code: int, priority: Optional[int], flags: int
) -> Tuple[int, int, int]:
    """(type, priority or -1 for 'inherit', flags) as the one-byte record
    fields they become, or ValueError."""
    code, flags = int(type_code), int(flags)
    prio = -1 if priority is None else int(priority)
    if not (0 <= code <= 255 and 0 <= flags <= 255 and -1 <= prio <= 255):
        raise ValueError("type, priority and flags are one byte each")
    return code, prio, flags


class Engine(abc.ABC):
    """Abstract delivery engine. All indices are dense agent indices
    assigned by :meth:`register_agent`; the facade maps agent-id strings
    to indices.

    A message's payload is ``[content (content_len)][extras JSON (rest)]``
    and :meth:`search` scans ``payload[:content_len]`` only. Every enqueue
    path — host batch, staged and graph ticks, device send and replies,
    router ingest, checkpoint load — stores ``content_len =
    min(content_len, payload_len)`` for a good record and 0 for an
    error-lane one, so the window never reaches past the bytes the record
    itself wrote: not into what the slot's previous occupant left behind,
    not into the next slot. :meth:`fetch` returns the stored value."""

    # --- registry ---

    @abc.abstractmethod
    def register_agent(self, agent_idx: int) -> None:
        """Activate an agent slot (idempotent)."""

    @abc.abstractmethod
    def deregister_agent(self, agent_idx: int) -> None:
        """Deactivate an agent slot. Inbox/messages survive (reference
        behavior, swarmdb/ main.py:351-372 — SURVEY.md §8.15)."""

    @abc.abstractmethod
    def active_agents(self) -> np.ndarray:
        """Bool array [max_agents] of active flags."""

    # --- send plane ---

    @abc.abstractmethod
    def enqueue_batch(self, recs: np.ndarray, payloads: bytes) -> np.ndarray:
        """Enqueue a batch. ``recs`` is a REC_DTYPE array whose
        payload_off/len index into ``payloads``. Returns the assigned
        sequence numbers (uint64 array). Status of each message is
        DELIVERED once this returns (the enqueue-ack — replaces the Kafka
        delivery callback, swarmdb/ main.py:374-391)."""

    @abc.abstractmethod
    def alloc_bitmap(self, bits: np.ndarray) -> int:
        """Store a visibility bitmap (bool array [max_agents]); returns an
        allocation HANDLE for REC_DTYPE.bitmap. On the GPU engine the
        pool is an epoch-tagged ring: the engine splits the handle into
        (pool slot, epoch) at enqueue time, and dequeue hides any message
        whose pool slot was recycled (exact visibility — never filtered
        against the wrong bitmap). The CPU engine's pool never recycles,
        so handle == index there."""

    # --- receive plane ---

    @abc.abstractmethod
    def receive(
        self, agent_idx: int, max_messages: int, priority_order: bool = False
    ) -> np.ndarray:
        """Drain up to max_messages deliverable entries from the agent's
        inbox cursor. Applies the visibility filter (reference
        swarmdb/ main.py:579-585) engine-side — per-agent cursors replace
        the reference's every-consumer-scans-everything model (SURVEY.md
        §8.7). Marks returned messages READ. Returns uint64 seq array."""

    def receive_many(
        self,
        agent_idxs: np.ndarray,
        max_per_agent: int,
        priority_order: bool = False,
    ) -> Tuple[np.ndarray, np.ndarray]:
        """Drain many agents at once. Returns (counts[len(agent_idxs)],
        concatenated seqs). Default: loop over :meth:`receive`; the GPU
        engine overrides this with a single dequeue kernel (one launch for
        the whole poll tick)."""
        counts = np.zeros(len(agent_idxs), dtype=np.int64)
        chunks = []
        for i, a in enumerate(agent_idxs):
            s = self.receive(int(a), max_per_agent, priority_order)
            counts[i] = len(s)
            if len(s):
                chunks.append(s)
        seqs = (
            np.concatenate(chunks) if chunks else np.empty(0, dtype=np.uint64)
        )
        return counts, seqs

    def _packed_rows(
        self, seqs: np.ndarray, stride: int, slots: np.ndarray
    ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Packed rows of ``seqs`` for the numpy doubles, from
        :meth:`fetch_raw_chunks`: the payload rows (uint8 ``[n, stride]``,
        zero at and past each row's length), the REC_DTYPE records with
        ``payload_off`` rebased to ``slots * stride``, and the lengths
        (``payload_len`` clamped to the stride)."""
        n = len(seqs)
        hdrs, flat, fstride = self.fetch_raw_chunks(seqs)
        flat = flat.reshape(n, fstride)
        lens = np.minimum(hdrs["payload_len"], stride).astype(np.int32)
        w = min(stride, fstride)
        rows = np.zeros((n, stride), dtype=np.uint8)
        rows[:, :w] = flat[:, :w]
        rows[np.arange(stride, dtype=np.int32)[None, :] >= lens[:, None]] = 0
        recs = np.zeros(n, dtype=REC_DTYPE)
        for name in REC_DTYPE.names:
            recs[name] = hdrs[name]
        recs["payload_off"] = slots.astype(np.uint64) * np.uint64(stride)
        return rows, recs, lens

    def receive_to_device(
        self,
        agent_idxs: np.ndarray,
        max_per_agent: int,
        priority_order: bool = False,
        max_payload: int = 0,
        out: Optional[DeviceDelivery] = None,
    ) -> DeviceDelivery:
        """Drain many agents into packed engine-resident arrays (see
        :class:`DeviceDelivery`). ``max_payload`` (if known) tightens the
        row stride below slot_bytes; longer payloads are truncated in the
        delivery (``lengths`` says to what) while the header keeps the
        true ``payload_len``. ``out`` reuses the buffers of an earlier
        delivery; one that is too small raises ValueError before anything
        is dequeued. Default: the CPU double on :meth:`receive_many` +
        :meth:`fetch_raw_chunks`, same layout and zero tails as the GPU
        engine's single stream-ordered submission."""
        agent_idxs = np.ascontiguousarray(agent_idxs, dtype=np.uint32)
        na, K = len(agent_idxs), int(max_per_agent)
        if K < 0:
            raise ValueError("max_per_agent must be >= 0")
        stride = delivery_stride(
            max_payload, self.cfg.slot_bytes  # type: ignore[attr-defined]
        )
        rows = na * K
        if out is not None:
            check_delivery_out(out, na, rows, stride)
            offsets = out.offsets[: na + 1]
            seqs_o, lengths, agent_row = out.seqs, out.lengths, out.agent_row
            headers, payload = out.headers, out.payload
        else:
            offsets = np.zeros(na + 1, dtype=np.int32)
            seqs_o = np.zeros(rows, dtype=np.int64)
            lengths = np.zeros(rows, dtype=np.int32)
            agent_row = np.zeros(rows, dtype=np.int32)
            headers = np.zeros((rows, REC_DTYPE.itemsize), dtype=np.uint8)
            payload = np.zeros((rows, stride), dtype=np.uint8)
        counts, seqs = self.receive_many(agent_idxs, K, priority_order)
        counts = np.asarray(counts, dtype=np.int64)
        total = int(counts.sum())
        offsets[0] = 0
        offsets[1:] = np.cumsum(counts)
        if total:
            payload[:total], recs, lens = self._packed_rows(
                seqs, stride, np.arange(total)
            )
            headers[:total] = recs.view(np.uint8).reshape(
                total, REC_DTYPE.itemsize
            )
            seqs_o[:total] = seqs.astype(np.int64)
            lengths[:total] = lens
            agent_row[:total] = np.repeat(
                np.arange(na, dtype=np.int32), counts
            )
        return DeviceDelivery(
            counts=counts, offsets=offsets, seqs=seqs_o, lengths=lengths,
            agent_row=agent_row, headers=headers, payload=payload,
            stride=stride, total=total,
        )

    def ack_device(
        self, seqs: Any, n: Optional[int] = None, status: int = ST_PROCESSED
    ) -> None:
        """Mark the first ``n`` (default: all) of ``seqs`` — the int64
        ``seqs`` array of a :class:`DeviceDelivery`, or a selection of it —
        with ``status``. A seq below the retention horizon is skipped (its
        slot holds a newer message), as is one never assigned; a deleted
        message stays deleted. Default: a host loop (the CPU double); the
        GPU engine reads the seqs straight from HBM in one kernel."""
        arr = np.asarray(_to_numpy(seqs), dtype=np.int64).reshape(-1)
        n = len(arr) if n is None else int(n)
        if not 0 <= n <= len(arr):
            raise ValueError("n must be within 0..len(seqs)")
        lo, hi = self.evict_base(), self.total_messages()
        for s in arr[:n].tolist():
            if s < lo or s >= hi or self.get_status(s) == ST_DELETED:
                continue
            self.set_status(s, int(status))

    # --- device-resident send ---

    def enqueue_from_device(
        self, headers: Any, payload: Any, n: Optional[int] = None
    ) -> np.ndarray:
        """Enqueue the first ``n`` (default: all ``cap``) records of
        ``headers`` — uint8 ``[cap, 48]`` holding REC_DTYPE records —
        with row ``i`` of ``payload`` (uint8 ``[cap, stride]``, stride a
        multiple of 16 in ``16..slot_bytes``) as record ``i``'s payload.
        Returns the seqs ``base..base+n``. On the GPU engine both are
        torch tensors in HBM and nothing but the launch crosses PCIe.

        The records are device data the host never sees, so only what
        the host can bound is followed: a record's own ``payload_off``
        is ignored, and ``payload_len > stride`` takes the error lane
        like any malformed record (FAILED, stored ``payload_len ==
        content_len == 0``, no inbox entry). ``bitmap`` carries the raw
        :meth:`alloc_bitmap` handle as for :meth:`enqueue_batch`; the GPU
        engine splits it on the device and overwrites ``bitmap_epoch``.
        Someone forwarding DELIVERED headers of restricted-visibility
        messages must restore the handle first (``bitmap =
        bitmap_epoch``, as ``GpuEngine.unsplit_bitmap_handles`` does).
        Broadcasts and VIS_GROUP fan out as in any batch. Every refusal
        (dtype, device, contiguity, alignment, stride, ``n``) is a
        ValueError raised before anything is enqueued.

        Default: the CPU double on :meth:`enqueue_batch`; it also takes a
        REC_DTYPE array for ``headers``."""
        recs, pay, n, stride = check_send_arrays(
            headers, payload, n, self.cfg.slot_bytes  # type: ignore[attr-defined]
        )
        if n == 0:
            return np.empty(0, dtype=np.uint64)
        recs = recs[:n].copy()
        recs["payload_off"] = np.arange(n, dtype=np.uint64) * np.uint64(stride)
        recs["payload_len"][recs["payload_len"] > stride] = OVERSIZE_LEN
        recs["bitmap_epoch"] = 0
        return self.enqueue_batch(recs, pay[:n].tobytes())

    def reply_to_device(
        self,
        delivery: DeviceDelivery,
        agent_idxs: np.ndarray,
        payload: Any,
        lengths: Any,
        type_code: int,
        priority: Optional[int] = None,
        flags: int = FLAG_DERIVED_ID,
        timestamp: Optional[float] = None,
    ) -> np.ndarray:
        """Answer the rows of ``delivery`` (polled with ``agent_idxs``)
        from engine-resident arrays: row ``r < delivery.total`` gets a
        reply iff ``lengths[r] >= 0`` (int32 ``[>= total]``), with the
        first ``lengths[r]`` bytes of row ``r`` of ``payload`` (uint8
        ``[>= total, rstride]``, the stride rules of
        :meth:`enqueue_from_device`) as payload and content.

        The reply goes from the POLLED agent of the row
        (``agent_idxs[agent_row[r]]`` — the delivered receiver may be
        BROADCAST) to the delivered message's sender, with type
        ``type_code``, ``priority`` (default: the delivered message's),
        ``flags``, the one ``timestamp`` (default: now), no visibility
        restriction and ``token_count`` 0. ``lengths[r] > rstride`` takes
        the error lane. Replies are numbered in row order — the j-th
        answered row gets ``base + j`` — and their seqs are returned;
        nothing is enqueued when no row is answered. On the GPU engine
        the count of replies is the one word that crosses PCIe.

        Default: the CPU double on :meth:`enqueue_batch`."""
        agent_idxs = np.ascontiguousarray(agent_idxs, dtype=np.uint32)
        total = int(delivery.total)
        if len(agent_idxs) != len(delivery.counts):
            raise ValueError("agent_idxs must be the polled list of the delivery")
        pay, lens, rstride = check_reply_arrays(
            payload, lengths, total, self.cfg.slot_bytes  # type: ignore[attr-defined]
        )
        code, prio, flags = check_reply_fields(type_code, priority, flags)
        lens = lens[:total].astype(np.int64)
        rows = np.flatnonzero(lens >= 0)
        m = len(rows)
        if m == 0:
            return np.empty(0, dtype=np.uint64)
        hdr = np.ascontiguousarray(_to_numpy(delivery.headers[:total]))
        if hdr.dtype != REC_DTYPE:
            hdr = hdr.view(REC_DTYPE).reshape(-1)
        hdr = hdr[rows]
        arow = np.asarray(_to_numpy(delivery.agent_row[:total]))[rows]
        known = (arow >= 0) & (arow < len(agent_idxs))
        recs = np.zeros(m, dtype=REC_DTYPE)
        recs["sender"] = BROADCAST  # a row of no polled agent: error lane
        recs["sender"][known] = agent_idxs[arow[known]]
        recs["receiver"] = hdr["sender"]
        recs["type"] = code
        recs["priority"] = hdr["priority"] if prio < 0 else prio
        recs["vis_mode"] = VIS_ALL
        recs["flags"] = flags
        recs["timestamp"] = time.time() if timestamp is None else timestamp
        recs["payload_off"] = rows.astype(np.uint64) * np.uint64(rstride)
        recs["payload_len"] = np.where(lens[rows] > rstride, OVERSIZE_LEN,
                                       lens[rows])
        recs["content_len"] = lens[rows]
        recs["bitmap"] = NO_BITMAP
        return self.enqueue_batch(recs, pay[:total].tobytes())

    @abc.abstractmethod
    def peek_inbox(self, agent_idx: int) -> np.ndarray:
        """All seqs ever appended to the agent's inbox (oldest first),
        tombstones excluded — backs get_agent_messages."""

    @abc.abstractmethod
    def unread_count(self, agent_idx: int) -> int:
        """Inbox entries in DELIVERED state (reference
        swarmdb/ main.py:1026-1047)."""

    # --- message store ---

    @abc.abstractmethod
    def fetch(self, seqs: np.ndarray) -> Tuple[np.ndarray, List[bytes]]:
        """Return (headers REC-like structured array incl. status + seq,
        payload bytes list) for the given seqs."""

    def fetch_raw_chunks(
        self, seqs: np.ndarray
    ) -> Tuple[np.ndarray, np.ndarray, int]:
        """Bulk fetch WITHOUT per-message Python objects: returns
        (headers structured array incl. status+seq, flat uint8 payload
        array laid out [n, stride], stride). The binary checkpoint path
        uses this to move the log at device-gather speed."""
        hdrs, pays = self.fetch(seqs)
        stride = int(self.cfg.slot_bytes)  # type: ignore[attr-defined]
        flat = np.zeros((len(seqs), stride), dtype=np.uint8)
        for i, p in enumerate(pays):
            flat[i, : len(p)] = np.frombuffer(p, dtype=np.uint8)
        return hdrs, flat.reshape(-1), stride

    def read_bitmap(self, slot: int, epoch: int) -> Optional[np.ndarray]:
        """Bit array of a visibility-bitmap pool slot if the epoch still
        matches (i.e. the referencing record's visibility set is still
        live); None when the slot was recycled."""
        return None

    @abc.abstractmethod
    def set_status(self, seq: int, status: int) -> None: ...

    def set_statuses(self, seqs: np.ndarray, statuses: np.ndarray) -> None:
        """Batched status restore (one kernel on GPU)."""
        for s, st in zip(seqs, statuses):
            self.set_status(int(s), int(st))

    @abc.abstractmethod
    def get_status(self, seq: int) -> int: ...

    def statuses(self, seqs: np.ndarray) -> np.ndarray:
        """Batched status lookup (one kernel + one D2H on GPU)."""
        return np.fromiter(
            (self.get_status(int(s)) for s in seqs), dtype=np.uint8,
            count=len(seqs),
        )

    @abc.abstractmethod
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
        """Filtered scan over all messages, newest-first (reference
        swarmdb/ main.py:671-740). Returns seq array."""

    @abc.abstractmethod
    def search(self, needle: bytes, case_sensitive: bool, limit: int) -> np.ndarray:
        """Substring scan over payloads, newest-first (reference
        swarmdb/ main.py:742-781). Returns seq array."""

    @abc.abstractmethod
    def delete(self, seq: int) -> bool:
        """Tombstone a message (reference swarmdb/ main.py:1132-1157)."""

    # --- counters / stats ---

    @abc.abstractmethod
    def total_messages(self) -> int: ...

    def evict_base(self) -> int:
        """Lowest seq still retained (slot-ring retention horizon). 0 on
        engines that never evict (the CPU log is append-only)."""
        return 0

    @abc.abstractmethod
    def stats_arrays(self) -> Dict[str, np.ndarray]:
        """Running counters: by_type [7], by_status [6], sent [max_agents],
        received [max_agents] (replaces the reference's O(N) scans,
        swarmdb/ main.py:973-1024 — SURVEY.md §5.5)."""

    @abc.abstractmethod
    def recv_rate_window(self, agent_idx: int, window_s: float) -> int:
        """Messages received by the agent in the last window (backs
        get_agent_load's processing_rate, swarmdb/ main.py:1069-1093)."""

    # --- load balancer ---

    @abc.abstractmethod
    def backend_add_load(self, backend_idx: int, delta: int) -> None: ...

    @abc.abstractmethod
    def backend_loads(self) -> np.ndarray: ...

    @abc.abstractmethod
    def least_loaded_backend(self, n_backends: int) -> int:
        """argmin over per-backend load counters (CDNA4 reduction kernel on
        GPU — BASELINE config 5; the mechanism the reference lacks,
        SURVEY.md §2.2 'LLM load balancing')."""

    def dispatch_batch(self, requests: int, n_backends: int) -> np.ndarray:
        """Exact sequential least-loaded dispatch of `requests` requests:
        each pick increments the chosen backend's in-flight count. One
        wavefront-shuffle reduction kernel on GPU; returns the chosen
        backend index per request."""
        out = np.empty(requests, dtype=np.uint32)
        for i in range(requests):
            b = self.least_loaded_backend(n_backends)
            self.backend_add_load(b, 1)
            out[i] = b
        return out

    # --- device-resident dispatch ---

    def dispatch_delivery(
        self,
        delivery: DeviceDelivery,
        n_backends: int,
        weight: str = "requests",
        type_code: Optional[int] = None,
        pinned: Any = None,
        out: Optional[DeviceDispatch] = None,
    ) -> DeviceDispatch:
        """Dispatch the rows of ``delivery`` to ``n_backends`` LLM backends
        where the engine keeps them. Rows ``r = 0 .. total-1`` are taken in
        row order against the per-backend load counters of
        :meth:`backend_add_load` / :meth:`dispatch_batch` (int64, compared
        as signed)::

            if type_code is not None and header[r].type != type_code:
                backend[r] = -1                  # row not dispatched
                continue
            cost = 1 if weight == "requests" else max(token_count[r], 1)
            b = agent_row[r]
            p = pinned[b] if pinned is not None and 0 <= b < na else -1
            k = p if p >= 0 else argmin(load[0:n_backends])  # ties: lowest
            load[k] += cost;  added[k] += cost;  backend[r] = k

        ``pinned`` is a host int32 array, one entry per polled agent of
        the delivery: ``-1`` or a backend index. ``agent_row`` and
        ``headers`` may have been written to by the consumer: an
        ``agent_row`` outside the polled list means "not pinned" and is
        never used as an index; ``type`` and ``token_count`` are values.
        The result (see :class:`DeviceDispatch`) stays in engine memory;
        on the GPU engine only the per-backend row counts cross PCIe.
        ``out`` reuses the buffers of an earlier dispatch. With
        ``weight="requests"`` and neither filter nor pins,
        ``backend[:total]`` equals ``dispatch_batch(total, n_backends)``.
        Hand the result to :meth:`release_dispatch` when the batch is done.

        Every refusal (``n_backends`` outside ``1..min(64, num_backends)``,
        an unknown ``weight``, a ``type_code`` outside one byte, a
        ``pinned`` of the wrong length or range, unusable arrays, an
        ``out`` that is too small or built for another ``n_backends``) is
        a ValueError raised before any load changes.

        Default: the CPU double, a numpy loop over :meth:`backend_loads`
        applied through :meth:`backend_add_load`."""
        na = len(delivery.counts)
        total = int(delivery.total)
        nb, by_tokens, code, pins = check_dispatch_args(
            n_backends, self.cfg.num_backends,  # type: ignore[attr-defined]
            weight, type_code, pinned, na,
        )
        hdr, arow = delivery.headers, delivery.agent_row
        for name, a in (("delivery.headers", hdr), ("delivery.agent_row", arow)):
            if not isinstance(a, np.ndarray) or not a.flags.c_contiguous:
                raise ValueError(f"{name} must be a contiguous numpy array")
        if hdr.dtype == np.uint8 and hdr.ndim == 2 \
                and hdr.shape[1] == REC_DTYPE.itemsize:
            hdr = hdr.view(REC_DTYPE).reshape(-1)
        elif not (hdr.dtype == REC_DTYPE and hdr.ndim == 1):
            raise ValueError(
                "delivery.headers must be uint8 [rows, 48] or REC_DTYPE [rows]")
        if arow.dtype != np.int32 or arow.ndim != 1:
            raise ValueError("delivery.agent_row must be int32 [rows]")
        if len(hdr) < total or len(arow) < total:
            raise ValueError("delivery arrays hold fewer rows than its total")
        if out is not None:
            check_dispatch_out(out, nb, total)
            for name in ("backend", "order", "rank", "offsets", "added"):
                if not isinstance(getattr(out, name), np.ndarray):
                    raise ValueError(f"out.{name} must be a numpy array")
            backend, order, rank = out.backend, out.order, out.rank
            offsets, added = out.offsets, out.added
        else:
            rows = len(arow)
            backend = np.zeros(rows, dtype=np.int32)
            order = np.zeros(rows, dtype=np.int32)
            rank = np.zeros(rows, dtype=np.int32)
            offsets = np.zeros(nb + 1, dtype=np.int32)
            added = np.zeros(nb, dtype=np.int64)

        load = np.asarray(self.backend_loads(), dtype=np.int64)[:nb].copy()
        types = hdr["type"][:total]
        tokens = hdr["token_count"][:total].astype(np.int64)
        cost = np.maximum(tokens, 1) if by_tokens else np.ones(total, np.int64)
        add = np.zeros(nb, dtype=np.int64)
        cnt = np.zeros(nb, dtype=np.int64)
        for r in range(total):
            if code >= 0 and int(types[r]) != code:
                backend[r] = -1
                rank[r] = 0
                continue
            b = int(arow[r])
            k = int(pins[b]) if pins is not None and 0 <= b < na else -1
            if k < 0:
                k = int(np.argmin(load))
            load[k] += cost[r]
            add[k] += cost[r]
            backend[r] = k
            rank[r] = cnt[k]
            cnt[k] += 1
        m = int(cnt.sum())
        chosen = backend[:total]
        rows_of = np.flatnonzero(chosen >= 0)
        order[:m] = rows_of[np.argsort(chosen[rows_of], kind="stable")]
        offsets[0] = 0
        offsets[1:] = np.cumsum(cnt)
        added[:] = add
        for k in range(nb):
            if add[k]:
                self.backend_add_load(k, int(add[k]))
        return DeviceDispatch(
            backend=backend, order=order, offsets=offsets, added=added,
            counts=cnt, rank=rank, n_backends=nb, total=total, m=m,
        )

    def release_dispatch(self, dispatch: DeviceDispatch) -> None:
        """Take the load of a finished dispatch off its backends:
        ``load[k] -= added[k]`` — the batch form of completing requests
        one by one. A second release of the same object is a
        ValueError."""
        if dispatch.released:
            raise ValueError("dispatch was already released")
        added = np.asarray(_to_numpy(dispatch.added), dtype=np.int64)
        for k in range(int(dispatch.n_backends)):
            if added[k]:
                self.backend_add_load(k, -int(added[k]))
        dispatch.released = True

    # --- device-resident conversation context ---

    def _context_window(self, lo: int, hi: int) -> Tuple[np.ndarray, np.ndarray]:
        """(headers, statuses) of the seqs ``[lo, hi)`` for the context
        double. Default: through :meth:`fetch_raw_chunks`."""
        hdrs, _, _ = self.fetch_raw_chunks(np.arange(lo, hi, dtype=np.uint64))
        return hdrs, np.asarray(hdrs["status"])

    def _context_visibility(
        self, wh: np.ndarray, ok: np.ndarray
    ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The part of ``sees`` that does not depend on the reader, for
        the window records ``wh`` that are candidates (``ok``): ``ok``
        without the records nobody can see, per record the row of its
        live bitmap in ``bits`` (``-1``: visible to all), and ``bits``
        (bool ``[k, max_agents]``, ``k >= 1``). Each distinct (bitmap,
        epoch) is read once, through :meth:`read_bitmap`."""
        max_agents = int(self.cfg.max_agents)  # type: ignore[attr-defined]
        vis = wh["vis_mode"]
        ok = ok.copy()
        pool = np.full(len(wh), -1, dtype=np.int64)
        rows: List[np.ndarray] = []
        known: Dict[Tuple[int, int], int] = {}
        restricted = ok & ((vis == VIS_BITMAP) | (vis == VIS_GROUP))
        for i in np.flatnonzero(restricted).tolist():
            bm = int(wh["bitmap"][i])
            if bm == NO_BITMAP:
                if vis[i] == VIS_GROUP and wh["receiver"][i] == BROADCAST:
                    ok[i] = False  # fanned out to nobody
                continue
            key = (bm, int(wh["bitmap_epoch"][i]))
            row = known.get(key)
            if row is None:
                try:
                    b = self.read_bitmap(*key)
                except IndexError:  # outside the pool
                    b = None
                row = -1
                if b is not None:
                    row = len(rows)
                    full = np.zeros(max_agents, dtype=bool)
                    b = np.asarray(b, dtype=bool)[:max_agents]
                    full[:len(b)] = b
                    rows.append(full)
                known[key] = row
            if row < 0:
                ok[i] = False  # recycled: hidden for good
            else:
                pool[i] = row
        bits = np.stack(rows) if rows else np.zeros((1, max_agents), bool)
        return ok, pool, bits

    def context_to_device(
        self,
        delivery: DeviceDelivery,
        agent_idxs: np.ndarray,
        depth: int,
        lookback: int,
        type_code: Optional[int] = None,
        max_payload: int = 0,
        out: Optional[DeviceContext] = None,
        *,
        shared: bool = False,
    ) -> DeviceContext:
        """Gather the conversation context of every row of ``delivery``
        (polled with ``agent_idxs``) from the log into engine-resident
        arrays (see :class:`DeviceContext`). For each row ``r <
        delivery.total``, independently of the other rows::

            a  = agent_idxs[agent_row[r]]  if 0 <= agent_row[r] < na  else none
            s  = headers[r].sender
            hi = min(max(seqs[r], 0), total_messages())   # exclusive
            lo = max(evict_base(), hi - lookback)
            if a is none or s >= max_agents:  count[r] = 0
            else:
              match(q) := status(q) not in {DELETED, FAILED}
                      and hdr(q).vis_mode == VIS_ALL
                      and (   (hdr(q).sender == s and hdr(q).receiver == a)
                           or (hdr(q).sender == a and hdr(q).receiver == s))
                      and (type_code is None or hdr(q).type == type_code)
              M = the `depth` largest q in [lo, hi) with match(q)
              count[r] = |M|;  slot j holds the j-th smallest q of M

        The row's own message is never part of its context (``hi`` is
        exclusive). Broadcasts never match (``receiver`` is BROADCAST),
        and messages with restricted visibility (VIS_BITMAP, VIS_GROUP)
        never appear: the context does not show a message whose visibility
        nobody checked. ``delivery.seqs``, ``agent_row`` and ``headers``
        may have been written to by the consumer and are values: an
        out-of-range ``agent_row`` or ``sender`` gives ``count == 0``, an
        out-of-range seq is clamped. ``max_payload`` tightens the slot
        stride as in :meth:`receive_to_device`. Only queue state is read:
        no cursor, status, counter or load changes.

        With ``shared=True`` (keyword-only, opt-in) the context of a row
        holds the newest messages one of the two parties wrote and the
        other party was allowed to see: broadcasts and group messages are
        included, and visibility is checked exactly as delivery checks
        it. ``a``, ``s``, ``lo``, ``hi``, ``depth`` and the slot order
        are as above; only ``match`` changes::

            sees(x, q) := what a poll by agent x does with q once q is in
                          x's inbox (k_receive):
              vis_mode(q) not in {VIS_BITMAP, VIS_GROUP}  -> True
              bitmap(q) == NO_BITMAP        -> True, except for a VIS_GROUP
                                               broadcast (receiver ==
                                               BROADCAST): k_fanout gives it
                                               to no inbox -> False
              bitmap(q) >= num_bitmaps      -> False
              the pool slot's epoch != bitmap_epoch(q)
                                            -> False  (recycled: hidden
                                                       for good)
              otherwise                     -> bit x of that bitmap

            match(q) := status(q) not in {DELETED, FAILED}
                    and (type_code is None or hdr(q).type == type_code)
                    and (   (hdr(q).sender == s
                             and hdr(q).receiver in {a, BROADCAST}
                             and sees(a, q))
                         or (hdr(q).sender == a
                             and hdr(q).receiver in {s, BROADCAST}
                             and sees(s, q)))

        The bit tested is always the other party's, never the author's (a
        facade broadcast leaves the sender's own bit clear, and that does
        not matter); with ``a == s`` the two lines say the same thing.
        Whether an agent was registered when a broadcast was sent cannot
        be recovered from the log and is not considered: a broadcast one
        party sent before the other registered still appears. An ``a``
        that is no agent index (``>= max_agents``) has no bit and sees
        nothing restricted. The delivered row's own ``bitmap`` fields are
        never used, only log records are. With ``shared=False`` every
        call behaves as it always did.

        Every refusal (``depth`` outside ``1..64``, ``lookback`` outside
        ``1..2**31-1``, a ``type_code`` outside one byte, an
        ``agent_idxs`` of another length than the delivery's or longer
        than ``max_agents``, a ``shared`` that is not a ``bool``, unusable
        delivery arrays, an ``out`` built for another ``depth`` or stride
        or with too few rows) is a ValueError raised before anything is
        gathered.

        Default: the CPU double, plain numpy over the log window (bitmaps
        through :meth:`read_bitmap`, where ``None`` — recycled — means
        hidden); ``Engine.context_to_device(gpu_engine, delivery.to_host(),
        ...)`` runs it over a GPU engine's own log."""
        cfg = self.cfg  # type: ignore[attr-defined]
        shared = check_context_shared(shared)
        total = int(delivery.total)
        depth, lookback, code, agents = check_context_args(
            depth, lookback, type_code, agent_idxs, len(delivery.counts),
            cfg.max_agents,
        )
        na = len(agents)
        stride = delivery_stride(max_payload, cfg.slot_bytes)
        dseq, arow, hdr = delivery.seqs, delivery.agent_row, delivery.headers
        for name, a in (("delivery.seqs", dseq), ("delivery.agent_row", arow),
                        ("delivery.headers", hdr)):
            if not isinstance(a, np.ndarray) or not a.flags.c_contiguous:
                raise ValueError(f"{name} must be a contiguous numpy array")
        if hdr.dtype == np.uint8 and hdr.ndim == 2 \
                and hdr.shape[1] == REC_DTYPE.itemsize:
            hdr = hdr.view(REC_DTYPE).reshape(-1)
        elif not (hdr.dtype == REC_DTYPE and hdr.ndim == 1):
            raise ValueError(
                "delivery.headers must be uint8 [rows, 48] or REC_DTYPE [rows]")
        if dseq.dtype != np.int64 or dseq.ndim != 1:
            raise ValueError("delivery.seqs must be int64 [rows]")
        if arow.dtype != np.int32 or arow.ndim != 1:
            raise ValueError("delivery.agent_row must be int32 [rows]")
        if len(hdr) < total or len(arow) < total or len(dseq) < total:
            raise ValueError("delivery arrays hold fewer rows than its total")
        D = depth
        if out is not None:
            check_context_out(out, D, stride, total)
            for name in ("counts", "seqs", "lengths", "headers", "payload"):
                if not isinstance(getattr(out, name), np.ndarray):
                    raise ValueError(f"out.{name} must be a numpy array")
            counts, seqs, lengths = out.counts, out.seqs, out.lengths
            headers, payload = out.headers, out.payload
        else:
            rows = len(arow)
            counts = np.zeros(rows, dtype=np.int32)
            seqs = np.full((rows, D), -1, dtype=np.int64)
            lengths = np.zeros((rows, D), dtype=np.int32)
            headers = np.zeros((rows, D, REC_DTYPE.itemsize), dtype=np.uint8)
            payload = np.zeros((rows, D, stride), dtype=np.uint8)
        result = DeviceContext(
            counts=counts, seqs=seqs, lengths=lengths, headers=headers,
            payload=payload, depth=D, stride=stride, total=total,
        )
        if total == 0:
            return result

        count, base = int(self.total_messages()), int(self.evict_base())
        hi = np.clip(dseq[:total], 0, count)
        lo = np.maximum(base, hi - lookback)
        ar = arow[:total].astype(np.int64)
        known = (ar >= 0) & (ar < na)
        a_of = np.full(total, -1, dtype=np.int64)
        a_of[known] = agents[ar[known]]
        s_of = hdr["sender"][:total].astype(np.int64)
        live = known & (s_of < cfg.max_agents) & (lo < hi)

        counts[:total] = 0
        seqs[:total] = -1
        lengths[:total] = 0
        if live.any():
            # one pass over the union window; the matches of each
            # (agent, sender) pair, ascending, serve all its rows
            wlo, whi = int(lo[live].min()), int(hi[live].max())
            wh, wst = self._context_window(wlo, whi)
            ok = (wst != ST_DELETED) & (wst != ST_FAILED)
            if code >= 0:
                ok &= wh["type"] == code
            snd = wh["sender"].astype(np.int64)
            rcv = wh["receiver"].astype(np.int64)
            if shared:
                ok, pool, bits = self._context_visibility(wh, ok)
            else:
                ok &= wh["vis_mode"] == VIS_ALL
            matches: Dict[Tuple[int, int], np.ndarray] = {}
            for r in np.flatnonzero(live).tolist():
                a, s = int(a_of[r]), int(s_of[r])
                m = matches.get((a, s))
                if m is None and shared:
                    to_a = (snd == s) & ((rcv == a) | (rcv == BROADCAST))
                    to_s = (snd == a) & ((rcv == s) | (rcv == BROADCAST))
                    free = pool < 0
                    sees_a = free | bits[pool, a] if a < bits.shape[1] else free
                    pair = (to_a & sees_a) | (to_s & (free | bits[pool, s]))
                    m = matches[(a, s)] = np.flatnonzero(ok & pair) + wlo
                elif m is None:
                    pair = ((snd == s) & (rcv == a)) | ((snd == a) & (rcv == s))
                    m = matches[(a, s)] = np.flatnonzero(ok & pair) + wlo
                i0 = int(np.searchsorted(m, lo[r]))
                i1 = int(np.searchsorted(m, hi[r]))
                took = m[max(i0, i1 - D):i1]
                counts[r] = len(took)
                seqs[r, :len(took)] = took
        rr, jj = np.nonzero(seqs[:total] >= 0)
        if len(rr):
            q = seqs[:total][rr, jj].astype(np.uint64)
            payload[rr, jj], recs, lengths[rr, jj] = self._packed_rows(
                q, stride, rr * D + jj)
            headers[rr, jj] = recs.view(np.uint8).reshape(
                len(q), REC_DTYPE.itemsize)
        return result

    # --- lifecycle ---

    def close(self) -> None:  # noqa: B027
        pass
