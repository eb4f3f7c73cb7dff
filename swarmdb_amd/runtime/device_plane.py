"""The device plane's result types and argument rules.

A call of the device plane leaves its result where the engine keeps it:
torch tensors in HBM on the GPU engine, numpy arrays of the same layout on
the CPU double. The layout of each result is written down once, as the
``FIELDS`` table of its class; fresh allocation, the check of a reused
``out=``, ``to_host()`` and the layout test all read that table. The
argument checkers both engines share live here too. No torch import.
"""

from __future__ import annotations

import dataclasses
import functools
import operator
from dataclasses import dataclass
from typing import Any, Callable, ClassVar, Dict, List, Optional, Tuple

import numpy as np

from .engine import REC_DTYPE


def _to_numpy(x: Any) -> np.ndarray:
    """Host copy of a numpy array or of a torch tensor (duck-typed: torch
    is optional and must not be imported on the CPU path)."""
    if hasattr(x, "detach"):
        return x.detach().cpu().numpy()
    return np.array(x, copy=True)


def check_host_array(name: str, a: Any) -> None:
    """Array kind of the CPU double (ValueError)."""
    if not isinstance(a, np.ndarray) or not a.flags.c_contiguous:
        raise ValueError(f"{name} must be a contiguous numpy array")


def as_records(a: np.ndarray, name: str) -> np.ndarray:
    """A contiguous host array seen as REC_DTYPE records: a REC_DTYPE array
    as it is, uint8 ``[..., 48]`` with the last axis folded into the
    record. Anything else is a ValueError."""
    if a.dtype == REC_DTYPE:
        return a
    if a.dtype == np.uint8 and a.ndim >= 2 \
            and a.shape[-1] == REC_DTYPE.itemsize:
        return a.view(REC_DTYPE).reshape(a.shape[:-1])
    raise ValueError(f"{name} must be uint8 [..., 48] or REC_DTYPE")


# ---- the field tables ----


class Field:
    """One array of a result. An extent is ``(name, plus)``. ``lead``: the
    leading extent a call needs, from its parameters ``p`` ("rows": the
    rows to allocate, or to define); ``tail``: the trailing shape, sizes
    or names in ``p``; ``keep``: the extent ``to_host()`` keeps, from the
    result's attributes (None: all). ``fill``: what the double's fresh
    array holds; the GPU engine's is ``torch.empty`` unless ``gpu_zero``.
    A reused array holds at least ``lead`` entries; ``exact``: no more;
    ``prefix``: the call uses its first ``lead``. ``host``: made on the
    host by the call, never allocated, never part of ``out=``."""

    def __init__(self, name: str, dtype: str, lead: Tuple[str, int],
                 tail: Tuple[Any, ...], keep: Optional[Tuple[str, int]],
                 fill: int = 0, gpu_zero: bool = False, exact: bool = False,
                 prefix: bool = False, host: bool = False):
        self.name, self.dtype = name, dtype  # dtype by name, as numpy takes it
        self.lead, self.tail, self.keep = lead, tail, keep
        self.fill, self.gpu_zero = fill, gpu_zero
        self.exact, self.prefix, self.host = exact, prefix, host
        self.ndim = 1 + len(tail)
        # byte rows move as 16 B chunks, everything else as its own item
        self.align = 16 if dtype == U8 else np.dtype(dtype).itemsize

    def tail_in(self, p: Dict[str, int]) -> Tuple[int, ...]:
        return tuple(map(p.get, self.tail, self.tail))  # a size stays itself

    def shape(self, p: Dict[str, int]) -> Tuple[int, ...]:
        return (p[self.lead[0]] + self.lead[1],) + self.tail_in(p)


I32, I64, U8 = "int32", "int64", "uint8"
ROWS, TOTAL = ("rows", 0), ("total", 0)


def numpy_array(shape: Tuple[int, ...], f: Field) -> np.ndarray:
    """The double's array maker for :meth:`DeviceResult.fresh`."""
    return np.full(shape, f.fill, dtype=f.dtype)


def check_host_fields(cls: type, arrays: List[Any]) -> None:
    """The double's array-kind test for :meth:`DeviceResult.reuse`."""
    for f, a in zip(cls.BUFFERS, arrays):
        check_host_array("out." + f.name, a)
        if a.dtype != f.dtype:
            raise ValueError(f"out.{f.name} must be {f.dtype}")


@functools.lru_cache(maxsize=64)
def _tails(cls: type, built: Any) -> Tuple[Tuple[int, ...], ...]:
    """Trailing shapes of the buffers of a ``cls`` built for ``built``, the
    values of ``BUILT_FOR``: all a tail may name."""
    p = dict(zip(cls.BUILT_FOR, built if len(cls.BUILT_FOR) > 1 else [built]))
    return tuple(f.tail_in(p) for f in cls.BUFFERS)


class DeviceResult:
    """What the three results share: everything that follows from the
    ``FIELDS`` table (in allocation order) and from ``BUILT_FOR``, the
    attributes a reused result must have been built with."""

    FIELDS: ClassVar[Tuple[Field, ...]] = ()
    BUFFERS: ClassVar[Tuple[Field, ...]] = ()  # FIELDS without the host's
    BUILT_FOR: ClassVar[Tuple[str, ...]] = ()

    def __init_subclass__(cls) -> None:
        cls.BUFFERS = tuple(f for f in cls.FIELDS if not f.host)
        # what reuse() reads per buffer, flat: it runs on every tick
        cls._PLAN = tuple(
            (f.name, f.lead[0], f.lead[1], f.exact, f.prefix, f.ndim)
            for f in cls.BUFFERS)
        # BUILT_FOR's values in a result and in a call's p (one, or a tuple)
        cls._built_of = operator.attrgetter(*cls.BUILT_FOR)
        cls._built_in = operator.itemgetter(*cls.BUILT_FOR)

    @classmethod
    def fresh(cls, p: Dict[str, int], make: Callable) -> Dict[str, Any]:
        """Fresh arrays for the parameters ``p``, by name, from the array
        maker ``make(shape, field)``."""
        return {f.name: make(f.shape(p), f) for f in cls.BUFFERS}

    @classmethod
    def reuse(cls, out: Any, p: Dict[str, int], kind: Callable,
              placement_only: bool = False) -> Dict[str, Any]:
        """The arrays of ``out``, by name, for a call with the parameters
        ``p``; ValueError if ``out`` was built for others, or the arrays
        fail ``kind(cls, arrays)``, or one has the wrong shape or is too
        short. With ``placement_only`` nothing is tested but
        ``BUILT_FOR``, ``kind`` and the leading extents."""
        if not placement_only and not isinstance(out, cls):
            raise ValueError(f"out must be a {cls.__name__}")
        built = cls._built_in(p)
        if cls._built_of(out) != built:
            raise ValueError(
                f"out was built for another {cls.BUILT_FOR}, not {built}")
        plan = cls._PLAN
        arrays = [getattr(out, row[0]) for row in plan]
        kind(cls, arrays)
        tails = plan if placement_only else _tails(cls, built)
        got = {}
        for (name, key, plus, exact, prefix, ndim), tail, a in zip(
                plan, tails, arrays):
            shape = a.shape
            if not placement_only and (
                    len(shape) != ndim or (tail and shape[1:] != tail)):
                raise ValueError(
                    f"out.{name} must have shape [rows, *{tail}]")
            n, have = p[key] + plus, shape[0]
            if have < n or (exact and have != n):
                raise ValueError(
                    f"out.{name} holds {have} rows, this call needs {n}")
            got[name] = a[:n] if prefix else a
        return got

    def to_host(self):
        """Copy with numpy arrays, each trimmed to the extent its field
        keeps (the defined range); ``headers``, where there is one, comes
        back as a REC_DTYPE array."""
        h = {}
        for f in self.FIELDS:
            end = f.keep and getattr(self, f.keep[0]) + f.keep[1]
            h[f.name] = _to_numpy(getattr(self, f.name)[:end])
        if "headers" in h:
            h["headers"] = as_records(
                np.ascontiguousarray(h["headers"]), "headers")
        return dataclasses.replace(self, **h)  # type: ignore[type-var]


@dataclass
class DeviceDelivery(DeviceResult):
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

    BUILT_FOR = ("stride",)
    FIELDS = (
        Field("offsets", I32, ("na", 1), (), None, gpu_zero=True, prefix=True),
        Field("seqs", I64, ROWS, (), TOTAL),
        Field("lengths", I32, ROWS, (), TOTAL),
        Field("agent_row", I32, ROWS, (), TOTAL),
        Field("headers", U8, ROWS, (REC_DTYPE.itemsize,), TOTAL),
        Field("payload", U8, ROWS, ("stride",), TOTAL),
        Field("counts", I64, ("na", 0), (), None, host=True),
    )


@dataclass
class DeviceDispatch(DeviceResult):
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
    unspecified, and :meth:`to_host` trims them away. ``released`` is set
    by :meth:`Engine.release_dispatch`; ``backend_ids`` (the backend names
    in index order) by the facade.
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

    BUILT_FOR = ("n_backends",)
    FIELDS = (
        Field("backend", I32, ROWS, (), TOTAL),
        Field("order", I32, ROWS, (), ("m", 0)),
        Field("rank", I32, ROWS, (), TOTAL),
        Field("offsets", I32, ("n_backends", 1), (), ("n_backends", 1),
              exact=True),
        Field("added", I64, ("n_backends", 0), (), ("n_backends", 0),
              exact=True),
        Field("counts", I64, ("n_backends", 0), (), None, host=True),
    )


@dataclass
class DeviceContext(DeviceResult):
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
    ``>= total``, are unspecified; :meth:`to_host` trims to ``total`` rows
    and gives ``headers`` as REC_DTYPE ``[total, D]``.

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

    BUILT_FOR = ("depth", "stride")
    FIELDS = (
        Field("counts", I32, ROWS, (), TOTAL),
        Field("seqs", I64, ROWS, ("depth",), TOTAL, fill=-1),
        Field("lengths", I32, ROWS, ("depth",), TOTAL),
        Field("headers", U8, ROWS, ("depth", REC_DTYPE.itemsize), TOTAL),
        Field("payload", U8, ROWS, ("depth", "stride"), TOTAL),
    )


# ---- a delivery as input ----


def delivery_host_view(
    delivery: DeviceDelivery, total: int, need_seqs: bool = False
) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]:
    """The host-array form of a delivery a call reads: (``headers`` as
    REC_DTYPE ``[rows]``, ``agent_row``, ``seqs`` or None), each of at
    least ``total`` rows, or ValueError — the numpy counterpart of
    ``GpuEngine._check_delivery_tensors``."""
    check_host_array("delivery.headers", delivery.headers)
    hdr = as_records(delivery.headers, "delivery.headers")
    if hdr.ndim != 1:
        raise ValueError(
            "delivery.headers must be uint8 [rows, 48] or REC_DTYPE [rows]")
    read = {"agent_row": I32, "seqs": I64} if need_seqs else {"agent_row": I32}
    for name, dtype in read.items():
        a = getattr(delivery, name)
        check_host_array(f"delivery.{name}", a)
        if a.dtype != dtype or a.ndim != 1:
            raise ValueError(f"delivery.{name} must be {dtype} [rows]")
        if len(a) < total or len(hdr) < total:
            raise ValueError("delivery arrays hold fewer rows than its total")
    return hdr, delivery.agent_row, delivery.seqs if need_seqs else None


# ---- argument rules ----

MAX_DISPATCH_BACKENDS = 64  # one wavefront lane per backend

DISPATCH_WEIGHTS = ("requests", "tokens")

MAX_CONTEXT_DEPTH = 64  # one wavefront lane per context slot

# payload_len a device-side record is staged with when its length does
# not fit its payload row: above every slot_bytes, so the enqueue's own
# validation parks it in the error lane
OVERSIZE_LEN = 0xFFFFFFFF


def _type_filter(type_code: Optional[int]) -> int:
    """``type_code`` as the kernels take it: -1 for 'no filter'."""
    if type_code is None:
        return -1
    code = int(type_code)
    if not 0 <= code <= 255:
        raise ValueError("type_code is one byte")
    return code


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
    code = _type_filter(type_code)
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
    code = _type_filter(type_code)
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


def delivery_stride(max_payload: int, slot_bytes: int) -> int:
    """Row stride of a device-resident delivery: ``max_payload`` rounded up
    to 16 B when it tightens the row below ``slot_bytes``."""
    if 0 < max_payload < slot_bytes:
        return (int(max_payload) + 15) // 16 * 16
    return int(slot_bytes)


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
    check_host_array("headers", headers)
    check_host_array("payload", payload)
    recs = as_records(headers, "headers")
    if recs.ndim != 1:
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
    check_host_array("payload", payload)
    check_host_array("lengths", lengths)
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
