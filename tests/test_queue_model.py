"""The bounded queue against a line-by-line model of its kernels.

``QueueModel`` below is plain Python, one statement per kernel statement,
of k_enqueue_meta + k_fanout, k_receive, k_unread, k_statuses,
k_set_status(es) and k_gather (csrc/swarmq_kernels.h), with the bounds the
CPU engine does not have: a log ring of ``num_slots``, inbox rings of
``inbox_capacity``, a dequeue window of ``recv_window`` and a recycling
bitmap pool. It shares no code with either engine.

Chain (tests/README.md): hand-computed cases -> QueueModel -> CpuEngine
(bounds out of reach, so the two must agree on everything) -> GPU (bounds
biting). Everything compared is an integer, an integer sequence or bytes:
no tolerance anywhere.

The GPU settles two orders with atomics: one agent's directs within a
batch, and the batch's broadcasts in ``bcast_list``. ``QueueModel.adopt``
checks what the ring may legally hold after a batch and takes the observed
order over; counters, ``wpos`` and ``dropped`` never depend on it and are
always predicted. The deterministic-batch tests use no adoption at all.

The model counts the branches it takes (``events``); each fuzz
configuration asserts that every branch it is meant to reach was reached,
per seed, and the GPU configurations are first run model-alone on the CPU
with the same seeds and sizes.

The file holds CPU and GPU tests, so GPU tests carry the marker one by
one.
"""

import collections

import numpy as np
import pytest

from swarmdb_amd import QueueConfig
from swarmdb_amd.runtime.cpu_engine import CpuEngine
from swarmdb_amd.runtime.engine import (
    BROADCAST,
    NO_BITMAP,
    REC_DTYPE,
    ST_DELETED,
    ST_DELIVERED,
    ST_FAILED,
    ST_PENDING,
    ST_PROCESSED,
    ST_READ,
    VIS_ALL,
    VIS_BITMAP,
    VIS_GROUP,
)

EPOCH_NONE = 0xFFFFFFFF
N_TYPES = 7
N_STATUS = 6
SEQ_MASK = (1 << 48) - 1
T0 = 1.7e9  # timestamps T0 + i are exact doubles

ZERO_HDR = {name: 0 for name in REC_DTYPE.names}


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------


class QueueModel:
    """The device queue's state and kernels, statement by statement.

    An inbox is the unbounded list of every seq ever appended; ring
    position ``p`` is ``inbox[a][p]``, and only positions ``>= wpos -
    inbox_capacity`` are ever read, as on the device where older ones are
    overwritten."""

    def __init__(self, *, max_agents, num_slots, slot_bytes, inbox_capacity,
                 recv_window, num_bitmaps):
        self.max_agents = max_agents
        self.num_slots = num_slots
        self.slot_bytes = slot_bytes
        self.cap = inbox_capacity
        self.window = recv_window
        self.num_bitmaps = num_bitmaps

        self.count = 0
        self.hdr = [dict(ZERO_HDR) for _ in range(num_slots)]
        self.status = [ST_PENDING] * num_slots
        self.payload = [b""] * num_slots

        self.inbox = [[] for _ in range(max_agents)]
        self.rpos = [0] * max_agents
        self.carry = [[] for _ in range(max_agents)]
        self.active = [False] * max_agents

        self.bitmaps = [None] * num_bitmaps
        self.epochs = [EPOCH_NONE] * num_bitmaps
        self.next_handle = 0

        self.by_type = [0] * N_TYPES
        self.by_status = [0] * N_STATUS
        self.sent = [0] * max_agents
        self.received = [0] * max_agents
        self.dropped = 0

        self.events = collections.Counter()
        self.was_active = set()
        # the last batch, for adopt()
        self._b_wpos = [0] * max_agents
        self._b_directs = collections.defaultdict(list)
        self._b_bcasts = collections.defaultdict(list)
        self._b_seen = []

    # --- whole-queue state ---

    @property
    def evict_base(self):
        return max(0, self.count - self.num_slots)

    def register(self, a):
        self.active[a] = True
        self.was_active.add(a)

    def deregister(self, a):
        self.active[a] = False

    def alloc_bitmap(self, bits):
        handle = self.next_handle
        self.next_handle += 1
        idx = handle % self.num_bitmaps
        self.bitmaps[idx] = [bool(b) for b in bits]
        self.epochs[idx] = handle
        return handle

    # --- k_enqueue_meta, k_enqueue_payload, k_fanout ---

    def _append(self, a, seq, book):
        pos = len(self.inbox[a])
        if pos - self.rpos[a] >= self.cap:
            self.dropped += 1
            self.events["dropped_append"] += 1
        if pos >= self.cap:
            self.events["ring_wrapped"] += 1
        self.inbox[a].append(seq)
        book[a].append(seq)

    def enqueue(self, recs, buf=b""):
        """One batch (at most staging_batch records, raw bitmap handles in
        ``bitmap`` as the engine takes them). Returns the base seq."""
        base = self.count
        self._b_wpos = [len(ib) for ib in self.inbox]
        self._b_directs = collections.defaultdict(list)
        self._b_bcasts = collections.defaultdict(list)
        self._b_seen = []
        bcast_list = []
        for i in range(len(recs)):
            r = {name: recs[name][i].item() for name in REC_DTYPE.names}
            # the engine's split of a handle into (pool slot, epoch)
            if r["vis_mode"] != VIS_ALL and r["bitmap"] != NO_BITMAP:
                r["bitmap_epoch"] = r["bitmap"]
                r["bitmap"] = r["bitmap"] % self.num_bitmaps
            seq = base + i
            slot = seq % self.num_slots
            bad = (
                r["type"] >= N_TYPES
                or r["priority"] > 3
                or r["payload_len"] > self.slot_bytes
                or (r["receiver"] != BROADCAST
                    and r["receiver"] >= self.max_agents)
                or r["sender"] >= self.max_agents
                or (r["vis_mode"] != VIS_ALL and r["bitmap"] != NO_BITMAP
                    and r["bitmap"] >= self.num_bitmaps)
            )
            off, plen = r["payload_off"], r["payload_len"]
            r["payload_off"] = slot * self.slot_bytes
            if bad:
                r["payload_len"] = 0
                r["content_len"] = 0
                self.hdr[slot] = r
                self.status[slot] = ST_FAILED
                self.by_status[ST_FAILED] += 1
                continue
            r["content_len"] = min(r["content_len"], r["payload_len"])
            self.hdr[slot] = r
            self.status[slot] = ST_DELIVERED
            if plen:
                self.payload[slot] = bytes(buf[off:off + plen])
            self.by_type[r["type"]] += 1
            self.by_status[ST_DELIVERED] += 1
            self.sent[r["sender"]] += 1
            if r["receiver"] == BROADCAST:
                bcast_list.append(seq)
            else:
                self._append(r["receiver"], seq, self._b_directs)
        self.count = base + len(recs)

        for a in range(self.max_agents):
            if not bcast_list:
                break
            for seq in bcast_list:
                h = self.hdr[seq % self.num_slots]
                if not self.active[a]:
                    # counted for a deregistered member only, not for the
                    # registry's never-used rows
                    if (a in self.was_active
                            and h["vis_mode"] == VIS_GROUP
                            and h["bitmap"] != NO_BITMAP
                            and self.epochs[h["bitmap"]] == h["bitmap_epoch"]
                            and self.bitmaps[h["bitmap"]][a]):
                        self.events["group_skip_inactive"] += 1
                    continue
                if h["vis_mode"] == VIS_GROUP:
                    if h["bitmap"] == NO_BITMAP:
                        self.events["group_skip_nobitmap"] += 1
                        continue
                    if self.epochs[h["bitmap"]] != h["bitmap_epoch"]:
                        self.events["group_skip_recycled"] += 1
                        continue
                    if not self.bitmaps[h["bitmap"]][a]:
                        self.events["group_skip_nonmember"] += 1
                        continue
                self._append(a, seq, self._b_bcasts)
        return base

    # --- the order one batch leaves in a ring ---

    def batch_start(self, a):
        """``wpos`` of agent ``a`` before the last batch."""
        return self._b_wpos[a]

    def adopt(self, a, wpos, window, device=True):
        """Check the ring of agent ``a`` as observed after the last batch
        (``window`` = the ``len(window)`` entries that end at ``wpos``),
        then take its order over. ``device``: the two orders only the GPU
        fixes, directs before broadcasts and one common broadcast order."""
        window = [int(s) for s in window]
        ib = self.inbox[a]
        assert wpos == len(ib), (a, wpos, len(ib))
        start = wpos - len(window)
        assert start >= 0
        if device:
            assert len(window) == min(wpos, self.cap), a
        b0 = self._b_wpos[a]
        n_old = max(0, b0 - start)
        assert window[:n_old] == ib[start:b0], f"agent {a}: old entries moved"
        first = max(b0, start)
        new = window[n_old:]
        seen, mine = collections.Counter(new), collections.Counter(ib[b0:])
        assert not seen - mine, f"agent {a}: entries nobody appended"
        if start <= b0:
            assert seen == mine, f"agent {a}: batch entries lost"
        if device:
            directs = set(self._b_directs[a])
            bcasts = set(self._b_bcasts[a])
            nd = len(self._b_directs[a])
            for p, s in enumerate(new, first):
                assert s in (directs if p < b0 + nd else bcasts), (a, p, s)
            self._b_seen.append([s for s in new if s in bcasts])
        ib[first:] = new

    def check_common_order(self):
        """The adopted rings' broadcasts fit one total order (bcast_list's):
        their consecutive pairs form no cycle."""
        succ = collections.defaultdict(set)
        indeg = collections.Counter()
        nodes = set()
        for seqs in self._b_seen:
            nodes.update(seqs)
            for x, y in zip(seqs, seqs[1:]):
                if y not in succ[x]:
                    succ[x].add(y)
                    indeg[y] += 1
        ready = [s for s in nodes if indeg[s] == 0]
        done = 0
        while ready:
            s = ready.pop()
            done += 1
            for t in succ[s]:
                indeg[t] -= 1
                if indeg[t] == 0:
                    ready.append(t)
        assert done == len(nodes), "broadcast order differs between rings"

    # --- k_receive ---

    def _visible(self, h, a):
        if (h["vis_mode"] in (VIS_BITMAP, VIS_GROUP)
                and h["bitmap"] != NO_BITMAP):
            if self.epochs[h["bitmap"]] != h["bitmap_epoch"]:
                self.events["recycled_hidden"] += 1
                return False
            if not self.bitmaps[h["bitmap"]][a]:
                self.events["hidden_nonmember"] += 1
                return False
        return True

    def receive(self, a, K, priority=False):
        eb = self.evict_base
        r = self.rpos[a]
        w = len(self.inbox[a])
        carry = self.carry[a]
        nc = len(carry)
        room = self.window - nc
        avail = w - r
        if avail > self.cap:
            r = w - self.cap
            avail = self.cap
            self.events["overflow_skip"] += 1
        fresh = min(avail, room)
        if fresh < avail:
            self.events["window_cut"] += 1
            if nc:
                self.events["window_cut_by_carry"] += 1
        total = nc + fresh
        if total > 256:
            self.events["examined_gt_256"] += 1
        if total and total & (total - 1):
            self.events["total_not_pow2"] += 1
        keys = []
        for i, seq in enumerate(carry + self.inbox[a][r:r + fresh]):
            if seq < eb:
                self.events["evicted_carry" if i < nc else "evicted_inbox"] += 1
                continue
            slot = seq % self.num_slots
            if self.status[slot] == ST_DELETED:
                self.events["deleted_examined"] += 1
                continue
            h = self.hdr[slot]
            if not self._visible(h, a):
                continue
            keys.append(((3 - h["priority"]) << 48 | seq) if priority else seq)
        keys.sort()
        if K == 0 and keys:
            self.events["k0_visible"] += 1
        if nc and fresh:
            self.events["carry_mixed_with_fresh"] += 1
        out = [k & SEQ_MASK for k in keys[:K]]
        self.carry[a] = [k & SEQ_MASK for k in keys[K:]]
        if self.carry[a]:
            self.events["carry_left"] += 1
        self.rpos[a] = r + fresh
        for seq in out:
            slot = seq % self.num_slots
            if self.status[slot] == ST_DELIVERED:
                self.status[slot] = ST_READ
                self.by_status[ST_READ] += 1
                self.by_status[ST_DELIVERED] -= 1
        self.received[a] += len(out)
        return out

    def receive_many(self, agents, K, priority=False):
        return [self.receive(int(a), K, priority) for a in agents]

    # --- k_unread, peek, k_statuses, k_set_status(es), k_gather ---

    def _retained(self, a):
        w = len(self.inbox[a])
        return self.inbox[a][max(0, w - self.cap):w]

    def unread(self, a):
        eb = self.evict_base
        return sum(
            1 for seq in self._retained(a)
            if seq >= eb and self.status[seq % self.num_slots] == ST_DELIVERED
        )

    def peek(self, a):
        eb = self.evict_base
        return [s for s in sorted(self._retained(a))
                if s >= eb and self.get_status(s) != ST_DELETED]

    def get_status(self, seq):
        if seq < self.evict_base or seq >= self.count:
            return ST_DELETED
        return self.status[seq % self.num_slots]

    def set_status(self, seq, new):
        if seq < self.evict_base or seq >= self.count:
            return
        slot = seq % self.num_slots
        old = self.status[slot]
        if old != new:
            self.by_status[old] -= 1
            self.by_status[new] += 1
            self.status[slot] = new

    def set_statuses(self, seqs, sts):
        for s, st in zip(seqs, sts):
            self.set_status(int(s), int(st))

    def delete(self, seq):
        if self.get_status(seq) == ST_DELETED:
            return False
        self.set_status(seq, ST_DELETED)
        return True

    def fetch(self, seq):
        """(header, status, payload bytes) of a seq below ``count``."""
        if seq < self.evict_base:
            return dict(ZERO_HDR), ST_DELETED, b""
        slot = seq % self.num_slots
        h = self.hdr[slot]
        return h, self.status[slot], self.payload[slot][:h["payload_len"]]


# ---------------------------------------------------------------------------
# records
# ---------------------------------------------------------------------------


def records(specs):
    """REC_DTYPE records + payload buffer from dicts of fields (``payload``
    holds the bytes). Every payload starts 16 B aligned with 16 B of slack
    behind the last, as the enqueue kernel's chunk copy wants."""
    recs = np.zeros(len(specs), dtype=REC_DTYPE)
    recs["vis_mode"] = VIS_ALL
    recs["bitmap"] = NO_BITMAP
    buf = bytearray()
    for i, spec in enumerate(specs):
        pay = spec.get("payload", b"")
        recs["payload_off"][i] = len(buf)
        recs["payload_len"][i] = len(pay)
        recs["content_len"][i] = len(pay)
        buf += pay + b"\x00" * (-len(pay) % 16)
        for name, v in spec.items():
            if name != "payload":
                recs[name][i] = v
    buf += b"\x00" * 16
    return recs, bytes(buf)


def direct(receiver, sender=0, **kw):
    return dict(sender=sender, receiver=receiver, **kw)


def bcast(sender=0, vis=VIS_ALL, handle=NO_BITMAP, **kw):
    return dict(sender=sender, receiver=BROADCAST, vis_mode=vis,
                bitmap=handle, **kw)


def bits(max_agents, *members):
    b = np.zeros(max_agents, dtype=bool)
    b[list(members)] = True
    return b


TINY = dict(max_agents=64, num_slots=8, slot_bytes=64, inbox_capacity=4,
            recv_window=4, num_bitmaps=2)
SMALL = dict(max_agents=64, num_slots=256, slot_bytes=64, inbox_capacity=64,
             recv_window=64, num_bitmaps=4)
BIG = dict(max_agents=64, num_slots=4096, slot_bytes=64, inbox_capacity=1024,
           recv_window=512, num_bitmaps=4)
# the CPU engine's bounds, as far as it has any: nothing evicts, overflows
# or recycles within a fuzz run
UNBOUNDED = dict(max_agents=64, num_slots=1 << 20, slot_bytes=64,
                 inbox_capacity=1 << 20, recv_window=64, num_bitmaps=1 << 16)


# ---------------------------------------------------------------------------
# the model on its own, bounds biting: expected lists written by hand
# ---------------------------------------------------------------------------


def test_model_overflow_skip_and_dropped():
    m = QueueModel(**TINY)
    m.register(1)
    # seqs 0..5 land at ring positions 0..5 of a 4-entry ring nobody has
    # read: positions 4 and 5 overwrite the unread 0 and 1
    m.enqueue(records([direct(1)] * 6)[0])
    assert m.dropped == 2
    assert m.unread(1) == 4 and m.peek(1) == [2, 3, 4, 5]
    # w - r = 6 > 4: skip to position 2
    assert m.receive(1, 10) == [2, 3, 4, 5]
    assert m.rpos[1] == 6 and m.carry[1] == []
    # positions 6, 7, 8 against rpos 6: nothing unread is overwritten
    m.enqueue(records([direct(1)] * 3)[0])
    assert m.dropped == 2
    assert m.evict_base == 1
    assert m.receive(1, 2) == [6, 7] and m.carry[1] == [8]
    assert m.receive(1, 2) == [8] and m.carry[1] == []
    assert m.received[1] == 7
    assert m.events["overflow_skip"] == 1
    assert m.events["dropped_append"] == 2
    assert m.by_status == [0, 2, 7, 0, 0, 0]  # 0 and 1 were never read


def test_model_eviction_of_unread_and_carried_entries():
    m = QueueModel(**TINY)
    for a in (1, 2, 3):
        m.register(a)
    m.enqueue(records([direct(1), direct(1), direct(1), direct(3)])[0])
    assert m.receive(1, 1) == [0]
    assert m.carry[1] == [1, 2] and m.rpos[1] == 3
    # seqs 4..11: count 12, evict_base 4; the carried 1 and 2 and agent
    # 3's unread 3 are gone from the log
    m.enqueue(records([direct(2)] * 8)[0])
    assert m.evict_base == 4
    assert m.dropped == 4  # agent 2's positions 4..7
    assert m.unread(3) == 0 and m.peek(3) == []
    assert m.receive(1, 10) == [] and m.carry[1] == []
    assert m.receive(3, 10) == [] and m.rpos[3] == 1
    assert m.events["evicted_carry"] == 2
    assert m.events["evicted_inbox"] == 1
    assert m.receive(2, 10) == [8, 9, 10, 11]
    assert m.get_status(0) == ST_DELETED  # evicted, though it was READ
    assert m.get_status(4) == ST_DELIVERED and m.get_status(8) == ST_READ
    assert m.fetch(3) == (ZERO_HDR, ST_DELETED, b"")
    # lifetime tally: 12 enqueued, 0 and 8..11 read; the overwritten
    # 1..3 are still counted DELIVERED
    assert m.by_status == [0, 7, 5, 0, 0, 0]
    assert m.received[:4] == [0, 1, 4, 0]


def test_model_recycled_epoch_hides_from_everybody():
    m = QueueModel(**TINY)
    for a in (0, 1, 2):
        m.register(a)
    h0 = m.alloc_bitmap(bits(64, 1))
    m.enqueue(records([bcast(0, VIS_BITMAP, h0)])[0])  # seq 0
    assert [len(m.inbox[a]) for a in (0, 1, 2)] == [1, 1, 1]
    h1 = m.alloc_bitmap(bits(64, 2))
    h2 = m.alloc_bitmap(bits(64, 1))  # pool slot 0 again: h0 is recycled
    assert (h0, h1, h2) == (0, 1, 2)
    assert m.receive(1, 10) == [] and m.receive(2, 10) == []
    assert m.events["recycled_hidden"] == 2
    assert m.get_status(0) == ST_DELIVERED
    # unread has no visibility test; the entry is still in the ring
    assert m.unread(1) == 1 and m.peek(1) == [0]
    # group fan-out: a stale handle and NO_BITMAP reach nobody, a current
    # one its members only
    m.enqueue(records([bcast(0, VIS_GROUP, h0), bcast(0, VIS_GROUP),
                       bcast(0, VIS_GROUP, h1)])[0])  # seqs 1, 2, 3
    assert [m.inbox[a] for a in (0, 1, 2)] == [[0], [0], [0, 3]]
    assert m.events["group_skip_recycled"] == 3
    assert m.events["group_skip_nobitmap"] == 3
    assert m.events["group_skip_nonmember"] == 2
    assert m.receive(2, 10) == [3]
    assert m.receive(0, 10) == [] and m.rpos[0] == 1
    assert m.dropped == 0


def test_model_status_write_outside_the_live_window_is_a_no_op():
    m = QueueModel(**TINY)
    m.register(1)
    m.enqueue(records([direct(1)] * 5)[0])
    m.enqueue(records([direct(1)] * 5)[0])
    assert (m.count, m.evict_base) == (10, 2)
    m.set_status(1, ST_PROCESSED)   # evicted: slot 1 holds seq 9
    m.set_status(12, ST_PROCESSED)  # unassigned: slot 4 holds seq 4
    assert m.get_status(9) == ST_DELIVERED and m.get_status(4) == ST_DELIVERED
    assert m.get_status(1) == ST_DELETED and m.get_status(12) == ST_DELETED
    assert m.by_status == [0, 10, 0, 0, 0, 0]
    m.set_status(4, ST_PROCESSED)
    assert not m.delete(1) and not m.delete(12)
    assert m.delete(5) and not m.delete(5)
    m.set_status(5, ST_READ)  # a tombstone is overwritten, as on both engines
    assert m.by_status == [0, 8, 1, 1, 0, 0]
    assert [m.get_status(s) for s in range(2, 10)] == [1, 1, 3, 2, 1, 1, 1, 1]


def test_model_adopt_checks_what_a_ring_may_hold():
    m = QueueModel(**TINY)
    m.register(1)
    m.enqueue(records([direct(1)])[0])
    m.enqueue(records([direct(1), bcast(0), direct(1)])[0])
    assert m.inbox[1] == [0, 1, 3, 2]
    m.adopt(1, 4, [0, 3, 1, 2])
    assert m.inbox[1] == [0, 3, 1, 2]
    for wpos, window in ((3, [0, 1, 3]),      # wpos is predicted
                         (4, [1, 0, 3, 2]),   # an earlier batch moved
                         (4, [0, 1, 1, 2]),   # not what was appended
                         (4, [0, 1, 2, 3])):  # broadcast before a direct
        with pytest.raises(AssertionError):
            m.adopt(1, wpos, window)
    m.adopt(1, 4, [0, 1, 2, 3], device=False)


# ---------------------------------------------------------------------------
# the fuzz driver: one traffic script for the model alone, CPU and GPU
# ---------------------------------------------------------------------------

K_SET = (0, 1, 3, 17, 64, 200)
N_ACTIVE = 24
HOT = 0
GONE = 5  # deregistered a third of the way in
COLD = 11  # the deterministic script's late reader


def make_engine(kind, geom, staging_batch=256):
    cfg = dict(geom, staging_batch=staging_batch, num_backends=16,
               auto_save=False)
    if kind == "gpu":
        # torch's HIP runtime must come up before the extension's, for the
        # tests below that hand torch tensors to the queue
        import torch  # noqa: F401

        from swarmdb_amd.runtime.gpu_engine import GpuEngine

        return GpuEngine(QueueConfig(use_gpu=True, **cfg))
    return CpuEngine(QueueConfig(use_gpu=False, **cfg))


def close(eng):
    if eng is not None and hasattr(eng, "close"):
        eng.close()


def observe(eng, m, a):
    """(wpos, window) of agent ``a``'s ring: the device's retained ring, or
    what the last batch appended to the CPU engine's."""
    if isinstance(eng, CpuEngine):
        ring = eng._inbox.get(a)
        if ring is None:
            return 0, []
        return ring.n, ring.view()[m.batch_start(a):].tolist()
    w, entries = eng.q.inbox_window(a)
    return int(w), entries.tolist()


def adopt_all(eng, m):
    device = not isinstance(eng, CpuEngine)
    for a in range(N_ACTIVE + 2):
        m.adopt(a, *observe(eng, m, a), device=device)
    if device:
        m.check_common_order()


class Traffic:
    """The seeded traffic script. Every choice comes from ``rng`` and the
    model, never from an engine, so the script is the same with or without
    one."""

    def __init__(self, seed, m, eng, *, p_new, hot_share, stale, group_nobitmap):
        self.rng = np.random.default_rng(seed)
        self.m, self.eng = m, eng
        self.p_new, self.hot_share = p_new, hot_share
        self.stale, self.group_nobitmap = stale, group_nobitmap
        self.handles = []
        self.stamp = 0

    def _bitmap(self, vis):
        rng, m = self.rng, self.m
        u = rng.random()
        if not self.handles or u < self.p_new:
            members = rng.random(m.max_agents) < 0.5
            h = m.alloc_bitmap(members)
            if self.eng is not None:
                assert self.eng.alloc_bitmap(members) == h
            self.handles.append(h)
            return h
        u = rng.random()
        if u < 0.1 and (vis == VIS_BITMAP or self.group_nobitmap):
            return NO_BITMAP
        if u < 0.3 and self.stale and len(self.handles) > m.num_bitmaps:
            return self.handles[-m.num_bitmaps - 1]  # recycled for certain
        return self.handles[-1]

    def batch(self, n):
        rng, m = self.rng, self.m
        specs = []
        for _ in range(n):
            s = dict(
                sender=int(rng.integers(0, N_ACTIVE)),
                type=int(rng.integers(0, N_TYPES)),
                priority=int(rng.integers(0, 4)),
                flags=int(rng.integers(0, 256)),
                token_count=int(rng.integers(0, 1 << 20)),
                timestamp=T0 + self.stamp,
                vis_mode=VIS_ALL,
                bitmap=NO_BITMAP,
            )
            self.stamp += 1
            if rng.random() < 0.12:
                s["receiver"] = BROADCAST
                s["vis_mode"] = (VIS_ALL, VIS_BITMAP, VIS_GROUP)[
                    int(rng.integers(0, 3))]
            else:
                s["receiver"] = (HOT if rng.random() < self.hot_share
                                 else int(rng.integers(0, N_ACTIVE)))
                if rng.random() < 0.03:
                    s["vis_mode"] = VIS_BITMAP
            if s["vis_mode"] != VIS_ALL:
                s["bitmap"] = self._bitmap(s["vis_mode"])
            plen = int(rng.integers(0, m.slot_bytes + 1))
            if rng.random() < 0.03:  # the error lane, five ways in
                how = int(rng.integers(0, 5))
                if how == 0:
                    s["type"] = 7 + int(rng.integers(0, 200))
                elif how == 1:
                    s["priority"] = 4 + int(rng.integers(0, 200))
                elif how == 2:
                    s["receiver"] = m.max_agents + int(rng.integers(0, 1000))
                elif how == 3:
                    s["sender"] = m.max_agents + int(rng.integers(0, 1000))
                else:
                    plen = m.slot_bytes + 16
            s["payload"] = rng.integers(0, 256, plen, dtype=np.uint8).tobytes()
            specs.append(s)
        recs, buf = records(specs)
        # a content window the sender overstates is clamped at enqueue
        recs["content_len"] = [int(rng.integers(0, len(s["payload"]) + 9))
                               for s in specs]
        return recs, buf


def check_counters(eng, m, with_dropped):
    st = eng.stats_arrays()
    assert st["by_type"].tolist() == m.by_type
    assert st["by_status"].tolist() == m.by_status
    assert st["sent"].tolist() == m.sent
    assert st["received"].tolist() == m.received
    if with_dropped:
        assert st["dropped"] == m.dropped


def check_inboxes(eng, m):
    agents = range(N_ACTIVE + 2)
    if isinstance(eng, CpuEngine):
        unread = [eng.unread_count(a) for a in agents]
    else:
        unread = eng.q.unread_counts(
            np.arange(N_ACTIVE + 2, dtype=np.uint32)).tolist()
    assert unread == [m.unread(a) for a in agents]
    for a in agents:
        assert eng.peek_inbox(a).tolist() == m.peek(a), a


def check_fetch(eng, m, seqs):
    hdrs, pays = eng.fetch(np.array(seqs, dtype=np.uint64))
    for i, seq in enumerate(seqs):
        h, st, pay = m.fetch(seq)
        got = {name: hdrs[name][i].item() for name in REC_DTYPE.names}
        assert got == h, seq
        assert int(hdrs["status"][i]) == st, seq
        assert bytes(pays[i]) == pay, seq


def check_device_state(eng, m, rng):
    """Everything the device exposes, against the model."""
    eb, count = m.evict_base, m.count
    assert (eng.evict_base(), eng.total_messages()) == (eb, count)
    seqs = np.arange(max(0, eb - 8), count, dtype=np.uint64)
    assert eng.statuses(seqs).tolist() == [m.get_status(int(s)) for s in seqs]
    check_counters(eng, m, with_dropped=True)
    check_inboxes(eng, m)
    if count:
        want = {eb, count - 1, *rng.integers(eb, count, 5).tolist()}
        if eb:
            want.add(eb - 1)
        check_fetch(eng, m, sorted(want))


def fuzz(seed, geom, kind, *, rounds, nmax, nmin=1, p_new=0.25, hot_share=0.3,
         hot_poll=0.35, stale=True, group_nobitmap=True, check_every=5):
    """Run the traffic script against the model and, if ``kind`` names one,
    an engine; returns the model's event counts."""
    m = QueueModel(**geom)
    eng = make_engine(kind, geom) if kind else None
    t = Traffic(seed, m, eng, p_new=p_new, hot_share=hot_share, stale=stale,
                group_nobitmap=group_nobitmap)
    rng = t.rng
    check_rng = np.random.default_rng(seed + 1000)
    try:
        for a in range(N_ACTIVE):
            m.register(a)
            if eng:
                eng.register_agent(a)
        for rnd in range(rounds):
            if rnd == rounds // 3:
                m.deregister(GONE)
                if eng:
                    eng.deregister_agent(GONE)
            recs, buf = t.batch(int(rng.integers(nmin, nmax + 1)))
            base = m.enqueue(recs, buf)
            if eng:
                seqs = eng.enqueue_batch(recs, buf)
                assert seqs.tolist() == list(range(base, base + len(recs)))
                adopt_all(eng, m)

            for _ in range(int(rng.integers(0, 4))):
                s = int(rng.integers(max(0, m.evict_base - 4), m.count + 2))
                deleted = m.delete(s)
                if eng:
                    assert eng.delete(s) == deleted, s

            for _ in range(2):
                polled = [a for a in range(N_ACTIVE + 2)
                          if rng.random() < (hot_poll if a == HOT else 0.5)]
                rng.shuffle(polled)
                K = int(rng.choice(K_SET))
                prio = bool(rng.random() < 0.5)
                want = m.receive_many(polled, K, prio)
                if eng and polled:
                    counts, got = eng.receive_many(
                        np.array(polled, dtype=np.uint32), K, prio)
                    assert counts.tolist() == [len(x) for x in want], rnd
                    assert got.tolist() == [s for x in want for s in x], rnd

            if kind == "cpu":
                check_inboxes(eng, m)
            elif kind == "gpu" and rnd % check_every == check_every - 1:
                check_device_state(eng, m, check_rng)
        if kind == "cpu":
            seqs = np.arange(m.count, dtype=np.uint64)
            assert eng.statuses(seqs).tolist() == [
                m.get_status(s) for s in range(m.count)]
            check_counters(eng, m, with_dropped=False)
        elif kind == "gpu":
            check_device_state(eng, m, check_rng)
    finally:
        close(eng)
    return m.events


def assert_reached(events, names):
    missing = [n for n in names if not events[n]]
    assert not missing, f"branches never taken: {missing} ({dict(events)})"


# what each configuration is meant to reach
CPU_EVENTS = (
    "window_cut_by_carry", "carry_left", "carry_mixed_with_fresh",
    "deleted_examined", "hidden_nonmember", "group_skip_nonmember",
    "group_skip_inactive", "k0_visible", "total_not_pow2",
)
BOUND_EVENTS = (
    "ring_wrapped", "overflow_skip", "dropped_append", "evicted_inbox",
    "evicted_carry", "recycled_hidden", "group_skip_recycled",
    "group_skip_nobitmap",
)
SMALL_EVENTS = CPU_EVENTS + BOUND_EVENTS
BIG_EVENTS = CPU_EVENTS + ("examined_gt_256", "window_cut", "recycled_hidden",
                           "group_skip_recycled", "group_skip_nobitmap",
                           "ring_wrapped", "evicted_carry")

CPU_FUZZ = dict(rounds=40, nmin=5, nmax=120, p_new=0.6, stale=False,
                group_nobitmap=False)  # CpuEngine has no group NO_BITMAP
SMALL_FUZZ = dict(rounds=60, nmax=200)
BIG_FUZZ = dict(rounds=60, nmax=200, hot_share=0.5, hot_poll=0.15)

CPU_SEEDS = (1, 2, 3, 4)
GPU_SEEDS = (11, 12, 13)
BIG_SEED = 21


@pytest.mark.parametrize("seed", CPU_SEEDS)
def test_cpu_engine_against_model(seed):
    """CpuEngine at recv_window=64 and the model with its bounds out of
    reach agree on every call, status, counter, unread count and peek."""
    events = fuzz(seed, UNBOUNDED, "cpu", **CPU_FUZZ)
    assert_reached(events, CPU_EVENTS)
    # nothing evicted, overflowed or recycled: the bounds were out of reach
    assert not [n for n in BOUND_EVENTS if events[n]]


@pytest.mark.parametrize("seed", GPU_SEEDS)
def test_model_alone_reaches_every_branch_small(seed):
    assert_reached(fuzz(seed, SMALL, None, **SMALL_FUZZ), SMALL_EVENTS)


def test_model_alone_reaches_every_branch_big():
    assert_reached(fuzz(BIG_SEED, BIG, None, **BIG_FUZZ), BIG_EVENTS)


def test_cpu_status_writes_outside_the_log():
    """CpuEngine.set_status(es) skip a seq never assigned, as the model
    (and the kernels) do; live seqs, tombstones included, are written."""
    m = QueueModel(**UNBOUNDED)
    cpu = make_engine("cpu", UNBOUNDED)
    m.register(1)
    cpu.register_agent(1)
    recs, buf = records([direct(1, payload=b"x" * 20)] * 10)
    m.enqueue(recs, buf)
    cpu.enqueue_batch(recs, buf)
    m.delete(3)
    cpu.delete(3)
    for e in (m, cpu):
        e.set_status(15, ST_PROCESSED)  # count + 5
        e.set_status(10, ST_PROCESSED)  # count
        e.set_status(2, ST_PROCESSED)
        e.set_statuses(np.array([0, 11, 3, 4000, 7], dtype=np.uint64),
                       np.array([ST_READ, ST_READ, ST_FAILED, ST_READ,
                                 ST_DELETED], dtype=np.uint32))
    assert cpu.statuses(np.arange(10)).tolist() == [
        m.get_status(s) for s in range(10)] == [2, 1, 3, 4, 1, 1, 1, 5, 1, 1]
    check_counters(cpu, m, with_dropped=False)
    assert m.by_status == [0, 6, 1, 1, 1, 1]
    assert cpu.receive(1, 100).tolist() == m.receive(1, 100)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("seed", GPU_SEEDS)
def test_gpu_fuzz_small(seed):
    """The smallest geometry where every branch is reachable: the log wraps
    a dozen times, rings overflow, epochs recycle."""
    assert_reached(fuzz(seed, SMALL, "gpu", **SMALL_FUZZ), SMALL_EVENTS)


@pytest.mark.gpu
def test_gpu_fuzz_big():
    """recv_window=512: k_receive's strided loops and the sort stages
    above 256 keys."""
    assert_reached(fuzz(BIG_SEED, BIG, "gpu", **BIG_FUZZ), BIG_EVENTS)


def deterministic_script(m, eng, rounds=150):
    """Batches of at most one direct per receiver and at most one
    broadcast: no order is left to the atomics, so rings, calls and state
    are compared with the model's own prediction, nothing adopted. Agent
    HOT is polled in round 100 (K=1: its ring has overflowed, and nearly
    a window's worth is carried) and from round 130 on (the carry cuts the
    fresh window, and part of it has left the log); agent COLD from round
    140 on, when what its ring holds has left the log."""
    rng = np.random.default_rng(7)
    n_agents = 12
    for a in range(n_agents):
        m.register(a)
        if eng:
            eng.register_agent(a)
    h = None
    for rnd in range(rounds):
        if rnd % 9 == 0:
            members = rng.random(m.max_agents) < 0.5
            h = m.alloc_bitmap(members)
            if eng:
                assert eng.alloc_bitmap(members) == h
        specs = [
            direct(a, sender=int(rng.integers(0, n_agents)),
                   priority=int(rng.integers(0, 4)),
                   payload=bytes([a, rnd % 256]) * int(rng.integers(0, 33)))
            for a in range(n_agents) if a == HOT or rng.random() < 0.25
        ]
        if rng.random() < 0.7:
            vis = (VIS_ALL, VIS_BITMAP, VIS_GROUP)[int(rng.integers(0, 3))]
            specs.append(bcast(1, vis, NO_BITMAP if vis == VIS_ALL else h))
        order = rng.permutation(len(specs))
        recs, buf = records([specs[i] for i in order])
        m.enqueue(recs, buf)
        tomb = int(rng.integers(m.evict_base, m.count)) if rnd % 5 == 2 else None
        quiet = {HOT: 130, COLD: 140}
        polled = [a for a in range(n_agents)
                  if rnd >= quiet.get(a, 0) and rng.random() < 0.3]
        K = int(rng.choice((0, 1, 2, 5, 16)))
        if rnd == 100:
            polled, K = [HOT], 1
        prio = bool(rnd % 2)
        yield recs, buf, tomb, polled, K, prio


def test_model_deterministic_script_bites():
    m = QueueModel(**SMALL)
    for _, _, tomb, polled, K, prio in deterministic_script(m, None):
        if tomb is not None:
            m.delete(tomb)
        m.receive_many(polled, K, prio)
    assert_reached(m.events, (
        "ring_wrapped", "overflow_skip", "dropped_append", "evicted_inbox",
        "evicted_carry", "window_cut_by_carry", "carry_left",
        "deleted_examined", "recycled_hidden", "group_skip_nonmember",
        "hidden_nonmember", "k0_visible"))


@pytest.mark.gpu
def test_gpu_deterministic_batches():
    m = QueueModel(**SMALL)
    eng = make_engine("gpu", SMALL)
    rng = np.random.default_rng(8)
    try:
        for rnd, (recs, buf, tomb, polled, K, prio) in enumerate(
                deterministic_script(m, eng)):
            eng.enqueue_batch(recs, buf)
            if tomb is not None:
                assert eng.delete(tomb) == m.delete(tomb)
            for a in range(12):
                w, entries = eng.q.inbox_window(a)
                assert w == len(m.inbox[a])
                assert entries.tolist() == m._retained(a), (rnd, a)
            want = m.receive_many(polled, K, prio)
            if polled:
                counts, got = eng.receive_many(
                    np.array(polled, dtype=np.uint32), K, prio)
                assert counts.tolist() == [len(x) for x in want], rnd
                assert got.tolist() == [s for x in want for s in x], rnd
            if rnd % 25 == 24:
                check_device_state(eng, m, rng)
        check_device_state(eng, m, rng)
    finally:
        close(eng)


SORT_TOTALS = (0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256,
               257, 511, 512)


@pytest.mark.gpu
@pytest.mark.parametrize("half", (False, True), ids=("full", "half"))
@pytest.mark.parametrize("prio", (True, False), ids=("priority", "seq"))
def test_gpu_sort_sweep(prio, half):
    """One agent per window total around every power of two up to the
    512-key window, random priorities, one tombstone each: the pad to
    npad, the bitonic stages and the carry round trip."""
    m = QueueModel(**BIG)
    eng = make_engine("gpu", BIG, staging_batch=4096)
    rng = np.random.default_rng(5)
    try:
        specs = []
        for a, total in enumerate(SORT_TOTALS):
            m.register(a)
            eng.register_agent(a)
            specs += [direct(a, priority=int(rng.integers(0, 4)))
                      for _ in range(total)]
        recs, buf = records([specs[i] for i in rng.permutation(len(specs))])
        m.enqueue(recs, buf)
        eng.enqueue_batch(recs, buf)
        for a, total in enumerate(SORT_TOTALS):
            assert len(m.inbox[a]) == total
            if total >= 2:
                s = m.inbox[a][int(rng.integers(0, total))]
                assert m.delete(s) and eng.delete(s)
        agents = np.arange(len(SORT_TOTALS), dtype=np.uint32)
        if not half:
            steps = [(agents, 512)]
        else:  # K = total // 2 for each agent alone, then one drain
            steps = [(agents[a:a + 1], t // 2)
                     for a, t in enumerate(SORT_TOTALS)]
            steps.append((agents, 512))
        for polled, K in steps:
            want = m.receive_many(polled, K, prio)
            counts, got = eng.receive_many(polled, K, prio)
            assert counts.tolist() == [len(x) for x in want]
            assert got.tolist() == [s for x in want for s in x]
        assert all(not c for c in m.carry)
        # in the half mode every agent whose live entries (one tombstone
        # off from 2 up) exceed total // 2 carried the rest once
        assert m.events["carry_left"] == (
            sum(1 for t in SORT_TOTALS if t - (t >= 2) > t // 2)
            if half else 0)
        check_counters(eng, m, with_dropped=True)
        seqs = np.arange(m.count, dtype=np.uint64)
        assert eng.statuses(seqs).tolist() == [
            m.get_status(s) for s in range(m.count)]
    finally:
        close(eng)


TICK_N, TICK_K, TICK_AGENTS = 64, 16, 16
TICK_EVENTS = ("ring_wrapped", "overflow_skip", "dropped_append",
               "evicted_carry", "window_cut_by_carry", "carry_left")


def tick_batches():
    """Twelve 64-record batches for 16 agents, half of the directs to HOT:
    at K=16 its backlog outgrows the window, the ring and the log."""
    rng = np.random.default_rng(9)
    for tick in range(12):
        specs = []
        for i in range(TICK_N):
            if rng.random() < 0.1:
                specs.append(bcast(int(rng.integers(0, TICK_AGENTS))))
            else:
                to = HOT if rng.random() < 0.5 else int(
                    rng.integers(0, TICK_AGENTS))
                specs.append(direct(to, payload=bytes([tick, i]) * 8))
        yield records(specs)


def test_model_tick_script_bites():
    m = QueueModel(**SMALL)
    for a in range(TICK_AGENTS):
        m.register(a)
    for recs, buf in tick_batches():
        m.enqueue(recs, buf)
        m.receive_many(range(TICK_AGENTS), TICK_K)
    assert_reached(m.events, TICK_EVENTS)


@pytest.mark.gpu
def test_gpu_captured_tick_over_a_wrapping_ring():
    """build_tick / run_tick: the captured enqueue + dequeue, which reads
    evict_base from dyn[1], twelve times over a 256-slot log with agent
    HOT backlogged. The ring a tick leaves is adopted before the model
    dequeues (the dequeue does not write the ring)."""
    m = QueueModel(**SMALL)
    eng = make_engine("gpu", SMALL)
    n, K, n_agents = TICK_N, TICK_K, TICK_AGENTS
    try:
        for a in range(n_agents):
            m.register(a)
            eng.register_agent(a)
        agents = np.arange(n_agents, dtype=np.uint32)
        eng.q.build_tick(n, agents, K, False)
        for tick, (recs, buf) in enumerate(tick_batches()):
            slot = tick & 1
            eng.q.stage_fill(slot, recs, np.frombuffer(buf, np.uint8), n)
            eng.q.prefetch_staged(slot)
            counts, flat = eng.q.run_tick(slot)
            m.enqueue(recs, buf)
            for a in range(n_agents):
                w, entries = eng.q.inbox_window(a)
                m.adopt(a, int(w), entries.tolist())
            m.check_common_order()
            want = m.receive_many(agents, K, False)
            assert counts.tolist() == [len(x) for x in want], tick
            flat = flat.reshape(n_agents, K)
            for a in range(n_agents):
                assert flat[a, :counts[a]].tolist() == want[a], (tick, a)
        assert_reached(m.events, TICK_EVENTS)
        check_device_state(eng, m, np.random.default_rng(9))
    finally:
        close(eng)


@pytest.mark.gpu
def test_gpu_status_writes_across_the_horizon():
    """set_status / set_statuses of an evicted or never-assigned seq are
    no-ops: the slot's current occupant keeps its status and by_status
    does not move; get_statuses of an unassigned seq reads DELETED."""
    m = QueueModel(**SMALL)
    eng = make_engine("gpu", SMALL)
    try:
        m.register(1)
        eng.register_agent(1)
        for _ in range(3):  # 300 messages: one wrap, evict_base 44
            recs, buf = records([direct(1, payload=b"p" * 16)] * 100)
            m.enqueue(recs, buf)
            eng.enqueue_batch(recs, buf)
        eb, count = m.evict_base, m.count
        assert (eb, count) == (44, 300)
        live = np.arange(eb, count, dtype=np.uint64)

        def same():
            assert eng.statuses(live).tolist() == [
                m.get_status(int(s)) for s in live]
            check_counters(eng, m, with_dropped=True)

        for e in (m, eng):
            e.set_status(eb - 1, ST_PROCESSED)    # slot of live seq 299
            e.set_status(count + 5, ST_PROCESSED)  # slot of live seq 49
            e.set_status(count, ST_PROCESSED)      # slot of live seq 44
        assert m.by_status == [0, 300, 0, 0, 0, 0]
        same()
        seqs = np.array([eb, 3, count + 1, 120, eb - 1, 1 << 40, count - 1],
                        dtype=np.uint64)
        sts = np.array([ST_READ, ST_FAILED, ST_FAILED, ST_PROCESSED,
                        ST_DELETED, ST_READ, ST_DELETED], dtype=np.uint32)
        for e in (m, eng):
            e.set_statuses(seqs, sts)
            e.set_status(count - 1, ST_PROCESSED)  # over a tombstone
        assert m.by_status == [0, 297, 1, 2, 0, 0]
        same()
        out = eng.q.get_statuses(
            np.array([eb - 1, eb, count - 1, count, count + 7, 1 << 40],
                     dtype=np.uint64))
        assert out.tolist() == [ST_DELETED, ST_READ, ST_PROCESSED,
                                ST_DELETED, ST_DELETED, ST_DELETED]
        assert eng.get_status(count) == ST_DELETED
    finally:
        close(eng)


@pytest.mark.gpu
def test_gpu_poll_refusals_leave_the_queue_alone():
    """A polled list that is too long, holds an index >= max_agents or an
    agent twice, or a negative max_per_agent, is a ValueError at every
    entry that uploads the list, before anything is launched."""
    import torch

    m = QueueModel(**SMALL)
    eng = make_engine("gpu", SMALL)
    try:
        for a in range(6):
            m.register(a)
            eng.register_agent(a)
        recs, buf = records(
            [direct(i % 5, payload=bytes([i]) * 10) for i in range(23)]
            + [bcast(2)])
        m.enqueue(recs, buf)
        eng.enqueue_batch(recs, buf)
        adopt_all(eng, m)
        counts, got = eng.receive_many(np.array([1, 2], dtype=np.uint32), 2)
        want = m.receive_many([1, 2], 2)
        assert counts.tolist() == [2, 2]
        assert got.tolist() == want[0] + want[1]
        q = eng.q
        dev = torch.device("cuda", 0)
        rows = 64 * 4
        t = dict(
            payload=torch.zeros((rows, 64), dtype=torch.uint8, device=dev),
            headers=torch.zeros((rows, 48), dtype=torch.uint8, device=dev),
            seqs=torch.zeros(rows, dtype=torch.int64, device=dev),
            lengths=torch.zeros(rows, dtype=torch.int32, device=dev),
            agent_row=torch.zeros(rows, dtype=torch.int32, device=dev),
            offsets=torch.zeros(65, dtype=torch.int32, device=dev),
        )
        ptrs = tuple(t[k].data_ptr() for k in (
            "payload", "headers", "seqs", "lengths", "agent_row", "offsets"))

        def u32(*xs):
            return np.array(xs, dtype=np.uint32)

        too_long = np.arange(65, dtype=np.uint32) % 64
        twice = u32(3, 1, 3)
        bad_lists = (too_long, u32(1, 64), u32(0xFFFFFFFF), twice)

        def untouched():
            check_counters(eng, m, with_dropped=True)
            for a in range(6):
                w, entries = q.inbox_window(a)
                assert (w, entries.tolist()) == (
                    len(m.inbox[a]), m._retained(a))
            assert (eng.total_messages(), eng.evict_base()) == (m.count, 0)

        for agents in bad_lists:
            with pytest.raises(ValueError):
                q.receive_many(agents, 2, False)
            with pytest.raises(ValueError):
                eng.receive_many(agents, 2)
            with pytest.raises(ValueError):
                q.receive_to_device(agents, 2, False, 64, *ptrs, rows)
            with pytest.raises(ValueError):
                q.build_tick(4, agents, 2, False)
            if agents is not twice:  # k_unread only reads: allowed
                with pytest.raises(ValueError):
                    q.unread_counts(agents)
            untouched()
        assert q.unread_counts(twice).tolist() == [
            m.unread(3), m.unread(1), m.unread(3)]
        good = u32(3, 1)
        with pytest.raises(ValueError):
            q.receive_many(good, -1, False)
        with pytest.raises(ValueError):
            q.receive_to_device(good, -1, False, 64, *ptrs, rows)
        with pytest.raises(ValueError):
            q.build_tick(4, good, -1, False)
        untouched()

        # nothing moved: an ordinary receive is what the model says
        polled = u32(0, 1, 2, 3, 4, 5)
        want = m.receive_many(polled, 64)
        counts, got = eng.receive_many(polled, 64)
        assert counts.tolist() == [len(x) for x in want]
        assert got.tolist() == [s for x in want for s in x]
        check_device_state(eng, m, np.random.default_rng(0))
    finally:
        close(eng)
