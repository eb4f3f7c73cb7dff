"""The device plane's contract and its numpy doubles.

The docstring of each method here specifies a call of the device plane;
the body under it is the reference implementation in plain numpy over the
engine's host-visible calls. :class:`~swarmdb_amd.runtime.engine.Engine`
inherits them as defaults: the CPU engine runs them under its lock, the
GPU engine overrides each with kernels, and ``Engine.<call>(gpu_engine,
...)`` runs a double over a GPU engine's own log.
"""

from __future__ import annotations

import time
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from .device_plane import (
    OVERSIZE_LEN, DeviceContext, DeviceDelivery, DeviceDispatch, _to_numpy,
    check_context_args, check_context_shared, check_dispatch_args,
    check_host_fields, check_reply_arrays, check_reply_fields,
    check_send_arrays, delivery_host_view, delivery_stride, numpy_array,
)
from .engine import (
    BROADCAST, FLAG_DERIVED_ID, NO_BITMAP, REC_DTYPE, ST_DELETED, ST_FAILED,
    ST_PROCESSED, VIS_ALL, VIS_BITMAP, VIS_GROUP,
)


class DeviceDoubles:
    """Mixin base of :class:`~swarmdb_amd.runtime.engine.Engine`."""

    cfg: Any  # the engine's QueueConfig

    # --- device-resident delivery ---

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
        self, agent_idxs: np.ndarray, max_per_agent: int,
        priority_order: bool = False, max_payload: int = 0,
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
        stride = delivery_stride(max_payload, self.cfg.slot_bytes)
        p = {"na": na, "stride": stride, "rows": na * K}
        if out is not None:
            buf = DeviceDelivery.reuse(out, p, check_host_fields)
        else:
            buf = DeviceDelivery.fresh(p, numpy_array)
        counts, seqs = self.receive_many(agent_idxs, K, priority_order)
        counts = np.asarray(counts, dtype=np.int64)
        total = int(counts.sum())
        buf["offsets"][0] = 0
        buf["offsets"][1:] = np.cumsum(counts)
        if total:
            buf["payload"][:total], recs, lens = self._packed_rows(
                seqs, stride, np.arange(total))
            buf["headers"][:total] = recs.view(np.uint8).reshape(total, -1)
            buf["seqs"][:total] = seqs.astype(np.int64)
            buf["lengths"][:total] = lens
            buf["agent_row"][:total] = np.repeat(
                np.arange(na, dtype=np.int32), counts)
        return DeviceDelivery(counts=counts, stride=stride, total=total, **buf)

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
            headers, payload, n, self.cfg.slot_bytes)
        if n == 0:
            return np.empty(0, dtype=np.uint64)
        recs = recs[:n].copy()
        recs["payload_off"] = np.arange(n, dtype=np.uint64) * np.uint64(stride)
        recs["payload_len"][recs["payload_len"] > stride] = OVERSIZE_LEN
        recs["bitmap_epoch"] = 0
        return self.enqueue_batch(recs, pay[:n].tobytes())

    def reply_to_device(
        self, delivery: DeviceDelivery, agent_idxs: np.ndarray, payload: Any,
        lengths: Any, type_code: int, priority: Optional[int] = None,
        flags: int = FLAG_DERIVED_ID, timestamp: Optional[float] = None,
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
        hdr, arow, _ = delivery_host_view(delivery, total)
        pay, lens, rstride = check_reply_arrays(
            payload, lengths, total, self.cfg.slot_bytes)
        code, prio, flags = check_reply_fields(type_code, priority, flags)
        lens = lens[:total].astype(np.int64)
        rows = np.flatnonzero(lens >= 0)
        m = len(rows)
        if m == 0:
            return np.empty(0, dtype=np.uint64)
        hdr, arow = hdr[rows], arow[rows]
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

    # --- device-resident dispatch ---

    def dispatch_delivery(
        self, delivery: DeviceDelivery, n_backends: int,
        weight: str = "requests", type_code: Optional[int] = None,
        pinned: Any = None, out: Optional[DeviceDispatch] = None,
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
            n_backends, self.cfg.num_backends, weight, type_code, pinned, na)
        hdr, arow, _ = delivery_host_view(delivery, total)
        p = {"n_backends": nb, "rows": total}
        if out is not None:
            buf = DeviceDispatch.reuse(out, p, check_host_fields)
        else:
            p["rows"] = len(arow)
            buf = DeviceDispatch.fresh(p, numpy_array)
        backend, order, rank = buf["backend"], buf["order"], buf["rank"]

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
        buf["offsets"][0] = 0
        buf["offsets"][1:] = np.cumsum(cnt)
        buf["added"][:] = add
        for k in range(nb):
            if add[k]:
                self.backend_add_load(k, int(add[k]))
        return DeviceDispatch(
            counts=cnt, n_backends=nb, total=total, m=m, **buf)

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
        max_agents = int(self.cfg.max_agents)
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
        self, delivery: DeviceDelivery, agent_idxs: np.ndarray, depth: int,
        lookback: int, type_code: Optional[int] = None, max_payload: int = 0,
        out: Optional[DeviceContext] = None, *, shared: bool = False,
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
        cfg = self.cfg
        shared = check_context_shared(shared)
        total = int(delivery.total)
        depth, lookback, code, agents = check_context_args(
            depth, lookback, type_code, agent_idxs, len(delivery.counts),
            cfg.max_agents,
        )
        na = len(agents)
        stride = delivery_stride(max_payload, cfg.slot_bytes)
        hdr, arow, dseq = delivery_host_view(delivery, total, need_seqs=True)
        D = depth
        p = {"depth": D, "stride": stride, "rows": total}
        if out is not None:
            buf = DeviceContext.reuse(out, p, check_host_fields)
        else:
            p["rows"] = len(arow)
            buf = DeviceContext.fresh(p, numpy_array)
        counts, seqs, lengths = buf["counts"], buf["seqs"], buf["lengths"]
        headers, payload = buf["headers"], buf["payload"]
        result = DeviceContext(depth=D, stride=stride, total=total, **buf)
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
            headers[rr, jj] = recs.view(np.uint8).reshape(len(q), -1)
        return result
