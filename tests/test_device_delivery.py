"""Device-resident delivery: receive_to_device / ack_device.

The CPU engine's implementation is the plain-numpy double; it is checked
against the classic receive_many + fetch path, and the HIP kernels
(k_scan_counts, k_deliver_device, k_ack_device) are checked against it.
Every comparison is byte-exact / integer-exact.

The file holds CPU and GPU tests, so GPU tests carry the marker one by
one.
"""

import numpy as np
import pytest

from swarmdb_amd import MessageStatus, QueueConfig, SwarmsDB
from swarmdb_amd.runtime.cpu_engine import CpuEngine
from swarmdb_amd.runtime.engine import (
    BROADCAST,
    NO_BITMAP,
    REC_DTYPE,
    ST_DELETED,
    ST_DELIVERED,
    ST_PROCESSED,
    ST_READ,
    VIS_ALL,
    VIS_BITMAP,
    DeviceDelivery,
)

# header columns compared across engines (bitmap / bitmap_epoch are split
# into (pool slot, epoch) on the GPU; payload_off is checked on its own)
HDR_COLS = ("sender", "receiver", "type", "priority", "vis_mode", "flags",
            "token_count", "timestamp", "payload_len", "content_len")


def small_cfg(**kw):
    base = dict(
        use_gpu=True,
        max_agents=256,
        num_slots=1 << 14,
        slot_bytes=512,
        inbox_capacity=1 << 12,
        staging_batch=4096,
        num_backends=16,
        auto_save=False,
    )
    base.update(kw)
    return QueueConfig(**base)


def gpu_and_twin(**kw):
    from swarmdb_amd.runtime.gpu_engine import GpuEngine

    return GpuEngine(small_cfg(**kw)), CpuEngine(small_cfg(use_gpu=False, **kw))


def make_recs(receivers, payloads, sender=0, priority=None):
    """REC batch + payload buffer (16-B aligned offsets) for explicit
    per-message receivers and payload bytes; deterministic headers."""
    n = len(receivers)
    recs = np.zeros(n, dtype=REC_DTYPE)
    recs["sender"] = sender
    recs["receiver"] = np.asarray(receivers, dtype=np.uint32)
    recs["type"] = np.arange(n) % 7
    recs["priority"] = (np.arange(n) % 4) if priority is None else priority
    recs["flags"] = np.arange(n) % 3
    recs["token_count"] = np.arange(n) + 100
    recs["timestamp"] = 1.7e9 + np.arange(n) * 0.25
    recs["vis_mode"] = VIS_ALL
    recs["bitmap"] = NO_BITMAP
    buf = bytearray()
    for i, p in enumerate(payloads):
        recs["payload_off"][i] = len(buf)
        recs["payload_len"][i] = len(p)
        recs["content_len"][i] = len(p)
        # non-zero padding: whatever a 16-B staging copy drags along past
        # payload_len must not show up in a delivered row
        buf += p + b"\xee" * (-len(p) % 16)
    buf += b"\xee" * 16
    return recs, bytes(buf)


def pattern(n, salt):
    """n non-zero payload bytes (a zero tail must come from the kernel)."""
    return bytes(1 + (i * 7 + salt) % 255 for i in range(n))


def assert_layout(d):
    """Properties every delivery has, whichever engine made it."""
    h = d.to_host()
    na = len(h.counts)
    assert h.total == int(h.counts.sum())
    np.testing.assert_array_equal(
        h.offsets[: na + 1], np.concatenate([[0], np.cumsum(h.counts)])
    )
    assert int(h.offsets[na]) == h.total
    assert h.payload.shape == (h.total, h.stride)
    np.testing.assert_array_equal(
        h.headers["payload_off"],
        np.arange(h.total, dtype=np.uint64) * np.uint64(h.stride),
    )
    np.testing.assert_array_equal(
        h.lengths, np.minimum(h.headers["payload_len"], h.stride)
    )
    np.testing.assert_array_equal(
        h.agent_row, np.repeat(np.arange(na), h.counts)
    )
    cols = np.arange(h.stride)[None, :]
    assert not h.payload[cols >= h.lengths[:, None]].any(), "non-zero row tail"
    return h


def assert_same_delivery(a, b):
    """Field-for-field equality of two host deliveries."""
    np.testing.assert_array_equal(a.counts, b.counts)
    np.testing.assert_array_equal(a.offsets, b.offsets)
    np.testing.assert_array_equal(a.seqs, b.seqs)
    np.testing.assert_array_equal(a.lengths, b.lengths)
    np.testing.assert_array_equal(a.agent_row, b.agent_row)
    np.testing.assert_array_equal(a.payload, b.payload)
    assert a.stride == b.stride and a.total == b.total
    for col in HDR_COLS:
        np.testing.assert_array_equal(a.headers[col], b.headers[col], col)


# ---------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------


def test_cpu_receive_to_device_matches_receive_many_and_fetch():
    cfg = small_cfg(use_gpu=False)
    eng, twin = CpuEngine(cfg), CpuEngine(cfg)
    lens = [0, 1, 15, 16, 17, 100, 511, 512, 33, 64, 5, 300]
    receivers = [i % 5 for i in range(len(lens))]
    pays = [pattern(n, i) for i, n in enumerate(lens)]
    recs, buf = make_recs(receivers, pays)
    for e in (eng, twin):
        for a in range(6):
            e.register_agent(a)
        e.enqueue_batch(recs, buf)
    agents = np.array([3, 0, 5, 1, 2, 4], dtype=np.uint32)  # 5: empty inbox

    for _ in range(2):  # K=2: the second call delivers what the first left
        d = eng.receive_to_device(agents, 2)
        counts, seqs = twin.receive_many(agents, 2)
        hdrs, fetched = twin.fetch(seqs)
        assert isinstance(d, DeviceDelivery)
        assert isinstance(d.payload, np.ndarray)
        assert d.stride == 512 and d.payload.shape == (len(agents) * 2, 512)
        h = assert_layout(d)
        assert h.total > 0
        np.testing.assert_array_equal(h.counts, counts)
        np.testing.assert_array_equal(h.seqs, seqs.astype(np.int64))
        np.testing.assert_array_equal(h.lengths, hdrs["payload_len"])
        for r, p in enumerate(fetched):
            assert h.payload[r, : len(p)].tobytes() == p
        for col in HDR_COLS:
            np.testing.assert_array_equal(h.headers[col], hdrs[col], col)
        np.testing.assert_array_equal(eng.statuses(seqs), twin.statuses(seqs))
    assert eng.receive_to_device(agents, 2).total == 0


def test_cpu_stride_out_reuse_and_ack_rules():
    cfg = small_cfg(use_gpu=False)
    eng = CpuEngine(cfg)
    for a in range(2):
        eng.register_agent(a)
    recs, buf = make_recs([0, 0, 1], [pattern(300, 1), pattern(7, 2),
                                      pattern(40, 3)])
    seqs = eng.enqueue_batch(recs, buf)
    agents = np.array([0, 1], dtype=np.uint32)

    small = eng.receive_to_device(agents[:1], 1, max_payload=100)
    assert small.stride == 112 and small.total == 1
    with pytest.raises(ValueError):  # one agent x 1 row cannot hold 2 x 4
        eng.receive_to_device(agents, 4, max_payload=100, out=small)
    with pytest.raises(ValueError):  # stride differs
        eng.receive_to_device(agents[:1], 1, out=small)

    big = eng.receive_to_device(agents, 4, max_payload=100)
    h = assert_layout(big)
    assert h.seqs.tolist() == [1, 2]  # the refusals dequeued nothing
    again = eng.receive_to_device(agents, 4, max_payload=100, out=big)
    assert again.payload is big.payload and again.total == 0

    # ack: deleted stays deleted, unknown seqs are ignored, n limits
    eng.delete(int(seqs[1]))
    eng.ack_device(np.array([0, 1, 2, 99], dtype=np.int64), n=0)
    assert eng.statuses(seqs).tolist() == [ST_READ, ST_DELETED, ST_READ]
    eng.ack_device(np.array([0, 1, 2, 99], dtype=np.int64))
    assert eng.statuses(seqs).tolist() == [
        ST_PROCESSED, ST_DELETED, ST_PROCESSED]
    assert int(eng.stats_arrays()["by_status"].sum()) == 3


def _msg_key(m):
    return (m.id, m.sender_id, m.receiver_id, m.content, m.type, m.priority,
            m.metadata)


def facade_roundtrip(db, twin):
    """Shared by the CPU and the GPU facade test: the same Message
    objects go into both dbs; `db` is read through the device path,
    `twin` through receive_messages."""
    names = ["alice", "bob", "carol", "dave"]
    for d in (db, twin):
        for a in names:
            d.register_agent(a)
    cap = db.config.slot_bytes
    msgs = [
        db.make_message("alice", "plain string", receiver_id="bob",
                        metadata={"k": 1}),
        db.make_message("alice", {"json": [1, 2, {"x": "y"}]},
                        receiver_id="carol", message_type="command",
                        priority=3),
        db.make_message("alice", "only bob and carol", receiver_id=None,
                        visible_to=["bob", "carol"]),
        db.make_message("dave", "z" * (cap + 100), receiver_id="bob",
                        metadata={"big": True}),
        db.make_message("bob", "to be deleted", receiver_id="dave"),
    ]
    ids = db.send_messages_bulk(msgs)
    assert twin.send_messages_bulk(msgs) == ids

    polled = ["bob", "carol", "dave", "erin"]  # erin: auto-registered
    delivery = db.receive_device(polled)
    assert "erin" in db.registered_agents
    got = db.messages_from_delivery(delivery)
    want = [twin.receive_messages(a, timeout=0) for a in polled]
    assert [len(g) for g in got] == [3, 2, 1, 0]
    assert [[_msg_key(m) for m in g] for g in got] == [
        [_msg_key(m) for m in w] for w in want
    ]
    assert got[0][2].content == "z" * (cap + 100)  # from the overflow store

    doomed_seq = db._seq_of(ids[4])
    assert db.delete_message(ids[4])
    db.ack_device(delivery)
    for mid in ids[:4]:
        assert db.get_message(mid).status == MessageStatus.PROCESSED
    assert db.get_message(ids[4]) is None
    assert db.engine.get_status(doomed_seq) == ST_DELETED
    return delivery


def test_facade_device_delivery_cpu(tmp_db, tmp_path):
    cfg = QueueConfig(use_gpu=False, save_dir=str(tmp_path / "twin"),
                      max_agents=512, auto_save=False)
    twin = SwarmsDB(config=cfg)
    try:
        delivery = facade_roundtrip(tmp_db, twin)
        assert isinstance(delivery.payload, np.ndarray)
    finally:
        twin.close()


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------


@pytest.mark.gpu
def test_gpu_parity_with_cpu_double():
    import torch

    gpu, cpu = gpu_and_twin()
    try:
        lens = [0, 1, 15, 16, 17, 31, 32, 33, 511, 512]
        receivers = [i % 8 for i in range(len(lens))] + [9] * 7
        pays = [pattern(n, i) for i, n in enumerate(lens)]
        pays += [pattern(20 + k, 50 + k) for k in range(7)]
        recs, buf = make_recs(receivers, pays)
        for e in (gpu, cpu):
            for a in range(10):
                e.register_agent(a)
            e.enqueue_batch(recs, buf)
        # agent 8 has an empty inbox; agent 9 holds 7 messages, K=4
        agents = np.array([9, 3, 8, 0, 1, 2, 4, 5, 6, 7], dtype=np.uint32)
        for want_total in (4 + 10, 3):
            d = gpu.receive_to_device(agents, 4)
            for t in (d.offsets, d.seqs, d.lengths, d.agent_row, d.headers,
                      d.payload):
                assert isinstance(t, torch.Tensor) and t.is_cuda
            assert d.seqs.dtype == torch.int64
            assert d.payload.shape == (len(agents) * 4, 512)
            g = assert_layout(d)
            c = assert_layout(cpu.receive_to_device(agents, 4))
            assert g.total == want_total
            assert_same_delivery(g, c)
            seqs = g.seqs.astype(np.uint64)
            assert (gpu.statuses(seqs) == ST_READ).all()
        np.testing.assert_array_equal(
            gpu.stats_arrays()["by_status"], cpu.stats_arrays()["by_status"]
        )
        np.testing.assert_array_equal(
            gpu.stats_arrays()["received"], cpu.stats_arrays()["received"]
        )
    finally:
        gpu.close()


@pytest.mark.gpu
def test_gpu_stale_tail_after_ring_wrap():
    from swarmdb_amd.runtime.gpu_engine import GpuEngine

    eng = GpuEngine(small_cfg(num_slots=64, inbox_capacity=256))
    try:
        eng.register_agent(0)
        agents = np.array([0], dtype=np.uint32)
        recs, buf = make_recs([0] * 64, [b"\xff" * 512] * 64)
        eng.enqueue_batch(recs, buf)
        first = eng.receive_to_device(agents, 64).to_host()
        assert first.total == 64 and (first.payload == 0xFF).all()

        cyc = [0, 1, 5, 15, 16, 17]
        lens = [cyc[i % len(cyc)] for i in range(64)]
        recs, buf = make_recs([0] * 64, [b"\x41" * n for n in lens])
        eng.enqueue_batch(recs, buf)  # every slot is reused
        h = assert_layout(eng.receive_to_device(agents, 64))
        assert h.total == 64
        np.testing.assert_array_equal(h.lengths, lens)
        cols = np.arange(h.stride)[None, :]
        live = cols < h.lengths[:, None]
        assert (h.payload[live] == 0x41).all()
        assert not h.payload[~live].any()
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("na", (1, 63, 64, 65, 255, 256, 257, 1000))
def test_gpu_scan_shapes(na):
    from swarmdb_amd.runtime.gpu_engine import GpuEngine

    eng = GpuEngine(small_cfg(max_agents=1024, inbox_capacity=64,
                              slot_bytes=64))
    try:
        receivers, pays = [], []
        for i in range(na):
            for k in range(i % 4):
                receivers.append(i)
                pays.append(np.array([i, k], dtype=np.uint64).tobytes())
        if receivers:
            recs, buf = make_recs(receivers, pays)
            eng.enqueue_batch(recs, buf)
        agents = np.random.default_rng(na).permutation(na).astype(np.uint32)
        h = assert_layout(eng.receive_to_device(agents, 4, max_payload=16))
        assert h.stride == 16
        np.testing.assert_array_equal(h.counts, agents % 4)
        assert int(h.offsets[na]) == h.total == int(h.counts.sum())
        assert h.total == len(receivers)
        decoded = h.payload.view(np.uint64).reshape(h.total, 2)
        np.testing.assert_array_equal(decoded[:, 0], agents[h.agent_row])
        np.testing.assert_array_equal(
            decoded[:, 1], np.arange(h.total) - h.offsets[h.agent_row]
        )
        np.testing.assert_array_equal(h.headers["receiver"], decoded[:, 0])
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_priority_and_visibility_order():
    gpu, cpu = gpu_and_twin()
    try:
        prio = [0, 3, 1, 3, 2, 0, 2, 1, 3, 0, 1, 2]
        receivers = [i % 3 for i in range(len(prio))]
        recs, buf = make_recs(receivers, [pattern(24, i) for i in range(12)],
                              priority=prio)
        # one restricted broadcast in the middle: agents 0 and 2 only
        recs["receiver"][5] = BROADCAST
        recs["vis_mode"][5] = VIS_BITMAP
        recs["priority"][5] = 3
        bits = np.zeros(256, dtype=bool)
        bits[[0, 2]] = True
        for e in (gpu, cpu):
            for a in range(4):
                e.register_agent(a)
            r = recs.copy()
            r["bitmap"][5] = e.alloc_bitmap(bits)
            e.enqueue_batch(r, buf)
        agents = np.array([2, 0, 3, 1], dtype=np.uint32)
        per_agent = {int(a): [] for a in agents}
        for _ in range(2):  # K=3 leaves a carry for the second call
            g = assert_layout(gpu.receive_to_device(agents, 3, True))
            c = assert_layout(cpu.receive_to_device(agents, 3, True))
            assert g.total > 0
            assert_same_delivery(g, c)
            for b, a in enumerate(agents):
                per_agent[int(a)] += g.seqs[g.offsets[b]:g.offsets[b + 1]].tolist()
        assert gpu.receive_to_device(agents, 3, True).total == 0
        # first call: highest priority first, FIFO within a level; the
        # restricted broadcast (seq 5) reached agents 0 and 2 only
        assert per_agent[0][:3] == [3, 5, 6]
        assert 5 in per_agent[2] and 5 not in per_agent[1]
        assert per_agent[3] == []
    finally:
        gpu.close()


@pytest.mark.gpu
def test_gpu_truncation_at_max_payload():
    gpu, cpu = gpu_and_twin()
    try:
        recs, buf = make_recs([0, 0, 0], [pattern(300, 1), pattern(112, 2),
                                          pattern(99, 3)])
        for e in (gpu, cpu):
            e.register_agent(0)
            e.enqueue_batch(recs, buf)
        agents = np.array([0], dtype=np.uint32)
        d = gpu.receive_to_device(agents, 8, max_payload=100)
        assert d.stride == 112 and d.payload.shape == (8, 112)
        g = assert_layout(d)
        assert g.lengths.tolist() == [112, 112, 99]
        assert g.headers["payload_len"].tolist() == [300, 112, 99]
        assert g.payload[0].tobytes() == pattern(300, 1)[:112]
        assert_same_delivery(
            g, cpu.receive_to_device(agents, 8, max_payload=100).to_host()
        )
    finally:
        gpu.close()


@pytest.mark.gpu
def test_gpu_refusal_leaves_state_alone():
    from swarmdb_amd.runtime.gpu_engine import GpuEngine

    eng = GpuEngine(small_cfg(max_agents=1024, inbox_capacity=64))
    try:
        receivers = [i % 5 for i in range(23)]
        recs, buf = make_recs(receivers, [pattern(10 + i, i) for i in range(23)])
        seqs = eng.enqueue_batch(recs, buf)
        everyone = np.arange(1024, dtype=np.uint32)
        five = np.arange(5, dtype=np.uint32)
        with pytest.raises(ValueError):  # 1024 x 4097 > the 4 Mi output pool
            eng.receive_to_device(everyone, 4097)
        empty = eng.receive_to_device(np.array([7], dtype=np.uint32), 2)
        assert empty.total == 0
        with pytest.raises(ValueError):  # 2 rows cannot hold 5 x 8
            eng.receive_to_device(five, 8, out=empty)
        # the binding refuses on its own, before any launch
        q, p = eng.q, empty
        ptrs = (p.payload.data_ptr(), p.headers.data_ptr(), p.seqs.data_ptr(),
                p.lengths.data_ptr(), p.agent_row.data_ptr(),
                p.offsets.data_ptr())
        with pytest.raises(ValueError):  # capacity_rows < na * K
            q.receive_to_device(five[:1], 8, False, 512, *ptrs, 2)
        with pytest.raises(ValueError):  # output pool
            q.receive_to_device(everyone, 4097, False, 512, *ptrs, 1 << 30)
        for stride in (0, 8, 24, 528):  # not a multiple of 16 in 16..512
            with pytest.raises(ValueError):
                q.receive_to_device(five[:1], 2, False, stride, *ptrs, 2)
        with pytest.raises(ValueError):  # na > max_agents
            q.receive_to_device(np.zeros(1025, dtype=np.uint32), 0, False,
                                512, *ptrs, 2)

        assert (eng.statuses(seqs) == ST_DELIVERED).all()
        counts, got = eng.receive_many(five, 8)
        assert counts.tolist() == [5, 5, 5, 4, 4]
        assert sorted(got.tolist()) == seqs.tolist()
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_ack_device():
    import torch

    gpu, cpu = gpu_and_twin(num_slots=64, inbox_capacity=256)
    try:
        receivers = [i % 3 for i in range(40)]
        recs, buf = make_recs(receivers, [pattern(8, i) for i in range(40)])
        # one broadcast: its seq shows up in several agents' rows
        recs["receiver"][11] = BROADCAST
        for e in (gpu, cpu):
            for a in range(3):
                e.register_agent(a)
            e.enqueue_batch(recs, buf)
        agents = np.arange(3, dtype=np.uint32)
        d = gpu.receive_to_device(agents, 32)
        c = cpu.receive_to_device(agents, 32)
        assert d.total == c.total == 42
        all_seqs = np.arange(40, dtype=np.uint64)

        gpu.ack_device(d.seqs, n=0)  # no-op
        assert (gpu.statuses(all_seqs) == ST_READ).all()

        assert d.seqs.is_cuda and d.seqs.dtype == torch.int64
        gpu.ack_device(d.seqs, n=d.total)
        cpu.ack_device(c.seqs, n=c.total)
        assert (gpu.statuses(all_seqs) == ST_PROCESSED).all()
        np.testing.assert_array_equal(
            gpu.stats_arrays()["by_status"], cpu.stats_arrays()["by_status"]
        )

        # wrap the 64-slot ring: seqs 40..71 evict 0..7 and reuse slots 0..7
        recs2, buf2 = make_recs([0] * 32, [pattern(8, i) for i in range(32)])
        gpu.enqueue_batch(recs2, buf2)
        assert gpu.evict_base() == 8
        gpu.set_status(30, ST_READ)
        assert gpu.delete(20)
        before = gpu.stats_arrays()["by_status"].copy()
        # 3: evicted (slot 3 now holds seq 67); 20: tombstone; 30: live;
        # 500: never assigned
        gpu.ack_device(np.array([3, 20, 30, 500], dtype=np.int64))
        assert gpu.get_status(67) == ST_DELIVERED
        assert gpu.get_status(20) == ST_DELETED
        assert gpu.get_status(30) == ST_PROCESSED
        after = gpu.stats_arrays()["by_status"]
        before[ST_READ] -= 1
        before[ST_PROCESSED] += 1
        np.testing.assert_array_equal(after, before)
    finally:
        gpu.close()


@pytest.mark.gpu
def test_facade_device_delivery_gpu(tmp_path):
    from swarmdb_amd.runtime.gpu_engine import GpuEngine

    cfg = small_cfg(save_dir=str(tmp_path / "gpu"))
    tcfg = small_cfg(use_gpu=False, save_dir=str(tmp_path / "twin"))
    db = SwarmsDB(config=cfg, engine=GpuEngine(cfg))
    twin = SwarmsDB(config=tcfg)
    try:
        delivery = facade_roundtrip(db, twin)
        assert delivery.payload.is_cuda
        assert delivery.payload.device.index == cfg.device_index
    finally:
        db.close()
        twin.close()
