"""Device-resident send: enqueue_from_device / reply_to_device.

The CPU engine's implementation is the plain-numpy double; it is checked
against the classic enqueue_batch path, and the HIP kernels
(k_stage_device, k_reply_count, k_build_replies) are checked against it
on a twin engine fed the same inputs. Every comparison is byte-exact /
integer-exact.

The file holds CPU and GPU tests, so GPU tests carry the marker one by
one.
"""

import numpy as np
import pytest

from swarmdb_amd import (
    MessagePriority,
    MessageStatus,
    MessageType,
    QueueConfig,
    SwarmsDB,
)
from swarmdb_amd.core.wire import derived_id
from swarmdb_amd.runtime.cpu_engine import CpuEngine
from swarmdb_amd.runtime.engine import (
    BROADCAST,
    FLAG_DERIVED_ID,
    NO_BITMAP,
    REC_DTYPE,
    ST_DELIVERED,
    ST_FAILED,
    ST_READ,
    TYPE_CODES,
    VIS_ALL,
    VIS_BITMAP,
)

# header columns compared across engines (bitmap / bitmap_epoch are split
# into (pool slot, epoch) on the GPU; payload_off is the engine's own)
HDR_COLS = ("sender", "receiver", "type", "priority", "vis_mode", "flags",
            "token_count", "timestamp", "payload_len", "content_len")

LENS = [0, 1, 15, 16, 17, 100, 511, 512, 33]
GARBAGE_OFF = 2 ** 40  # what every test record carries as payload_off
PAD = 0xEE  # non-zero bytes after each payload in its row


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


def pattern(n, salt):
    """n non-zero payload bytes."""
    return bytes(1 + (i * 7 + salt) % 255 for i in range(n))


def device_batch(lens, receivers, stride, cap=None, sender=0):
    """Records + one payload row each, as a device-side producer leaves
    them: headers uint8 [cap, 48] with a garbage payload_off, payload
    uint8 [cap, stride] whose rows hold the payload followed by non-zero
    padding. A length above the stride fills the whole row."""
    n = len(lens)
    cap = n if cap is None else cap
    recs = np.zeros(cap, dtype=REC_DTYPE)
    recs["sender"][:n] = sender
    recs["receiver"][:n] = np.asarray(receivers, dtype=np.uint32)
    recs["type"][:n] = np.arange(n) % 7
    recs["priority"][:n] = np.arange(n) % 4
    recs["flags"][:n] = np.arange(n) % 3
    recs["token_count"][:n] = np.arange(n) + 100
    recs["timestamp"][:n] = 1.7e9 + np.arange(n) * 0.25
    recs["vis_mode"] = VIS_ALL
    recs["bitmap"] = NO_BITMAP
    recs["bitmap_epoch"] = 777  # must be overwritten
    recs["payload_off"] = GARBAGE_OFF
    recs["payload_len"][:n] = lens
    recs["content_len"][:n] = lens
    payload = np.full((cap, stride), PAD, dtype=np.uint8)
    for i, ln in enumerate(lens):
        w = min(ln, stride)
        payload[i, :w] = np.frombuffer(pattern(w, i), dtype=np.uint8)
    headers = recs.view(np.uint8).reshape(cap, REC_DTYPE.itemsize)
    return recs, headers, payload


def classic_batch(recs, payload, n):
    """The same n messages for enqueue_batch: offsets into the flattened
    rows."""
    out = recs[:n].copy()
    out["payload_off"] = np.arange(n, dtype=np.uint64) * np.uint64(
        payload.shape[1])
    out["bitmap_epoch"] = 0
    return out, payload[:n].tobytes() + bytes([PAD]) * 16


def snapshot(eng, n_agents):
    """Everything a send leaves behind, in host form."""
    lo, hi = eng.evict_base(), eng.total_messages()
    seqs = np.arange(lo, hi, dtype=np.uint64)
    hdrs, pays = eng.fetch(seqs)
    stats = eng.stats_arrays()
    return {
        "range": (lo, hi),
        "hdrs": hdrs,
        "pays": pays,
        "inbox": [eng.peek_inbox(a).tolist() for a in range(n_agents)],
        "stats": {k: np.asarray(stats[k]) for k in
                  ("by_type", "by_status", "sent", "received")},
        "dropped": int(stats["dropped"]),
    }


def assert_same_state(a, b, n_agents):
    sa, sb = snapshot(a, n_agents), snapshot(b, n_agents)
    assert sa["range"] == sb["range"]
    for col in HDR_COLS + ("status",):
        np.testing.assert_array_equal(sa["hdrs"][col], sb["hdrs"][col], col)
    assert sa["pays"] == sb["pays"]
    assert sa["inbox"] == sb["inbox"]
    for k in sa["stats"]:
        np.testing.assert_array_equal(sa["stats"][k], sb["stats"][k], k)
    assert sa["dropped"] == sb["dropped"] == 0
    return sa


def error_lane_case(cap):
    """stride 64; rows 1 and 2 are oversize (65, 4000), row 3 has a bad
    type, row 4 an out-of-range receiver; rows 0 and 5 are fine."""
    lens = [10, 65, 4000, 20, 30, 40]
    recs, headers, payload = device_batch(lens, [1, 1, 2, 2, 1, 2], 64, cap)
    recs["type"][3] = 9
    recs["receiver"][4] = 300
    return recs, headers, payload, len(lens)


def check_error_lane(eng, seqs):
    assert seqs.tolist() == list(range(6))
    hdrs, pays = eng.fetch(seqs)
    assert hdrs["status"].tolist() == [
        ST_DELIVERED, ST_FAILED, ST_FAILED, ST_FAILED, ST_FAILED, ST_DELIVERED]
    assert hdrs["payload_len"].tolist() == [10, 0, 0, 0, 0, 40]
    assert hdrs["content_len"].tolist() == [10, 0, 0, 0, 0, 40]
    assert pays[0] == pattern(10, 0) and pays[5] == pattern(40, 5)
    assert pays[1:5] == [b""] * 4
    by_status = eng.stats_arrays()["by_status"]
    assert by_status[ST_FAILED] == 4 and by_status[ST_DELIVERED] == 2
    assert eng.peek_inbox(1).tolist() == [0]
    assert eng.peek_inbox(2).tolist() == [5]


def reply_case(eng):
    """Agents 1 and 3 (and 0, 4, 5) are active, 7 is not. Four messages:
    5->1, 4->everyone, 5->1, 0->3. Polling [1, 7, 3] gives counts
    [3, 0, 2]; rows 1 and 3 are the broadcast."""
    for a in (0, 1, 3, 4, 5):
        eng.register_agent(a)
    recs = np.zeros(4, dtype=REC_DTYPE)
    recs["sender"] = [5, 4, 5, 0]
    recs["receiver"] = [1, BROADCAST, 1, 3]
    recs["type"] = [0, 1, 2, 4]
    recs["priority"] = [0, 2, 3, 1]
    recs["bitmap"] = NO_BITMAP
    recs["timestamp"] = 1.7e9
    recs["payload_off"] = np.arange(4) * 16
    recs["payload_len"] = recs["content_len"] = 16
    eng.enqueue_batch(recs, b"".join(pattern(16, i) for i in range(4))
                      + b"\0" * 16)
    agents = np.array([1, 7, 3], dtype=np.uint32)
    d = eng.receive_to_device(agents, 4)
    assert d.counts.tolist() == [3, 0, 2] and d.total == 5
    return d, agents


REPLY_LENGTHS = np.array([5, -1, 0, 64, -1], dtype=np.int32)


def reply_rows(rows, rstride, seed):
    return np.random.default_rng(seed).integers(
        1, 256, size=(rows, rstride), dtype=np.uint8)


# ---------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------


def test_cpu_enqueue_from_device_matches_enqueue_batch():
    cfg = small_cfg(use_gpu=False)
    eng, rec_eng, twin = CpuEngine(cfg), CpuEngine(cfg), CpuEngine(cfg)
    recs, headers, payload = device_batch(LENS, [i % 4 for i in range(9)], 512)
    for e in (eng, rec_eng, twin):
        for a in range(5):
            e.register_agent(a)
    seqs = eng.enqueue_from_device(headers, payload)
    np.testing.assert_array_equal(
        seqs, twin.enqueue_batch(*classic_batch(recs, payload, 9)))
    assert seqs.dtype == np.uint64 and seqs.tolist() == list(range(9))
    s = assert_same_state(eng, twin, 5)
    assert s["hdrs"]["payload_len"].tolist() == LENS
    assert s["pays"] == [pattern(n, i) for i, n in enumerate(LENS)]
    # a REC_DTYPE array is taken too; n limits the batch
    np.testing.assert_array_equal(
        rec_eng.enqueue_from_device(recs, payload, n=4), seqs[:4])
    assert rec_eng.total_messages() == 4
    assert rec_eng.enqueue_from_device(recs, payload, n=0).tolist() == []
    for bad_n in (-1, 10):
        with pytest.raises(ValueError):
            rec_eng.enqueue_from_device(recs, payload, n=bad_n)
    with pytest.raises(ValueError):  # stride 40
        rec_eng.enqueue_from_device(recs, payload[:, :40].copy())
    assert rec_eng.total_messages() == 4


def test_cpu_error_lane():
    eng = CpuEngine(small_cfg(use_gpu=False))
    for a in range(3):
        eng.register_agent(a)
    _, headers, payload, n = error_lane_case(cap=6)
    check_error_lane(eng, eng.enqueue_from_device(headers, payload, n))


def test_cpu_reply_to_device():
    eng = CpuEngine(small_cfg(use_gpu=False))
    d, agents = reply_case(eng)
    pay = reply_rows(d.payload.shape[0], 64, seed=3)
    seqs = eng.reply_to_device(d, agents, pay, REPLY_LENGTHS,
                               TYPE_CODES["function_result"], timestamp=1.8e9)
    assert seqs.tolist() == [4, 5, 6]  # m == 3, row order
    hdrs, pays = eng.fetch(seqs)
    want = np.zeros(3, dtype=REC_DTYPE)
    want["sender"] = [1, 1, 3]    # the polled agent, also for the broadcast
    want["receiver"] = [5, 5, 4]  # the original sender
    want["type"] = TYPE_CODES["function_result"]
    want["priority"] = [0, 3, 2]  # inherited
    want["vis_mode"] = VIS_ALL
    want["flags"] = FLAG_DERIVED_ID
    want["timestamp"] = 1.8e9
    want["payload_len"] = want["content_len"] = [5, 0, 64]
    for col in HDR_COLS:
        np.testing.assert_array_equal(hdrs[col], want[col], col)
    assert (hdrs["bitmap"] == NO_BITMAP).all()
    assert (hdrs["status"] == ST_DELIVERED).all()
    assert pays == [pay[0, :5].tobytes(), b"", pay[3].tobytes()]
    assert eng.peek_inbox(5).tolist() == [1, 4, 5]
    assert eng.peek_inbox(4).tolist() == [1, 6]

    seqs = eng.reply_to_device(d, agents, pay, REPLY_LENGTHS, 0, priority=1)
    assert eng.fetch(seqs)[0]["priority"].tolist() == [1, 1, 1]

    before = eng.total_messages()
    none = eng.reply_to_device(d, agents, pay,
                               np.full(5, -1, dtype=np.int32), 0)
    assert none.tolist() == [] and none.dtype == np.uint64
    assert eng.total_messages() == before
    with pytest.raises(ValueError):  # not the polled list
        eng.reply_to_device(d, agents[:2], pay, REPLY_LENGTHS, 0)
    with pytest.raises(ValueError):  # lengths shorter than total
        eng.reply_to_device(d, agents, pay, REPLY_LENGTHS[:4].copy(), 0)
    assert eng.total_messages() == before


def numpy_reply(delivery):
    """Reply = the content bytes, each plus one."""
    hdr = delivery.headers.view(REC_DTYPE).reshape(-1)
    return delivery.payload[:, :64] + np.uint8(1), hdr["content_len"].astype(
        np.int32)


def facade_loop(db, make_reply):
    """send A->B, A->C; device poll of [B, C]; reply from the delivery;
    the caller reads A's inbox. Returns the expected reply contents."""
    ida = db.send_message("ann", "hello-bob", receiver_id="bob",
                          priority=MessagePriority.HIGH)
    idb = db.send_message("ann", "hi-cy", receiver_id="cy",
                          priority=MessagePriority.CRITICAL)
    d = db.receive_device(["bob", "cy"])
    assert d.counts.tolist() == [1, 1]
    pay, lengths = make_reply(d)
    before = db.engine.total_messages()
    with pytest.raises(ValueError):
        db.reply_device(d, ["bob"], pay, lengths)
    with pytest.raises(ValueError):
        db.reply_device(d, ["bob", "nobody"], pay, lengths)
    assert "nobody" not in db.registered_agents
    assert db.engine.total_messages() == before
    seqs = db.reply_device(d, ["bob", "cy"], pay, lengths)
    assert seqs.tolist() == [before, before + 1]
    db.ack_device(d)
    for mid in (ida, idb):
        assert db.get_message(mid).status == MessageStatus.PROCESSED
    return seqs, ["ifmmp.cpc", "ij.dz"]


def check_replies(db, msgs, seqs, contents):
    assert [m.content for m in msgs] == contents
    assert [m.sender_id for m in msgs] == ["bob", "cy"]
    assert [m.receiver_id for m in msgs] == ["ann", "ann"]
    assert all(m.type == MessageType.FUNCTION_RESULT for m in msgs)
    assert [m.priority for m in msgs] == [
        MessagePriority.HIGH, MessagePriority.CRITICAL]
    assert [m.id for m in msgs] == [
        derived_id(db.config.rank, int(s)) for s in seqs]


def test_facade_device_send_cpu(tmp_db):
    seqs, contents = facade_loop(tmp_db, numpy_reply)
    check_replies(tmp_db, tmp_db.receive_messages("ann", timeout=0), seqs,
                  contents)
    # send_device: the engine call behind the facade
    _, headers, payload = device_batch([3, 4], [0, 0], 16)
    sent = tmp_db.send_device(headers, payload)
    assert sent.tolist() == [int(seqs[-1]) + 1, int(seqs[-1]) + 2]


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------


def dev(arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr)).cuda()


@pytest.mark.gpu
def test_gpu_enqueue_from_device_parity():
    gpu, cpu = gpu_and_twin()
    try:
        for e in (gpu, cpu):
            for a in range(5):
                e.register_agent(a)
        base = 0
        # thread-per-record block edges, 4-waves-per-block payload edges
        for n in (1, 63, 64, 65, 255, 256, 257):
            lens = [LENS[i % len(LENS)] for i in range(n)]
            _, headers, payload = device_batch(
                lens, [i % 5 for i in range(n)], 512)
            seqs = gpu.enqueue_from_device(dev(headers), dev(payload))
            np.testing.assert_array_equal(
                seqs, cpu.enqueue_from_device(headers, payload))
            assert seqs.dtype == np.uint64
            assert seqs.tolist() == list(range(base, base + n))
            base += n
            assert_same_state(gpu, cpu, 5)
        lens = list(range(49))  # 0..48 in rows of 48
        _, headers, payload = device_batch(lens, [i % 5 for i in range(49)],
                                           48, cap=53)
        seqs = gpu.enqueue_from_device(dev(headers), dev(payload), n=49)
        np.testing.assert_array_equal(
            seqs, cpu.enqueue_from_device(headers, payload, n=49))
        s = assert_same_state(gpu, cpu, 5)
        assert s["hdrs"]["payload_len"][base:].tolist() == lens
        assert (s["hdrs"]["status"] == ST_DELIVERED).all()
    finally:
        gpu.close()


@pytest.mark.gpu
def test_gpu_chunking_and_broadcast_fanout():
    gpu, cpu = gpu_and_twin(staging_batch=256)
    try:
        for e in (gpu, cpu):
            for a in range(4):
                e.register_agent(a)
        n = 600
        receivers = [BROADCAST if i % 3 == 0 else i % 4 for i in range(n)]
        _, headers, payload = device_batch(
            [(i * 5) % 65 for i in range(n)], receivers, 64, sender=1)
        seqs = gpu.enqueue_from_device(dev(headers), dev(payload))
        assert seqs.tolist() == list(range(n))  # contiguous across chunks
        np.testing.assert_array_equal(
            seqs, cpu.enqueue_from_device(headers, payload))
        s = assert_same_state(gpu, cpu, 4)  # also: nothing dropped
        bcasts = [i for i in range(n) if i % 3 == 0]
        for a in range(4):
            inbox = s["inbox"][a]
            assert len(inbox) == len(set(inbox))
            assert [q for q in inbox if q % 3 == 0] == bcasts
    finally:
        gpu.close()


@pytest.mark.gpu
def test_gpu_ring_wrap():
    from swarmdb_amd.runtime.gpu_engine import GpuEngine

    # the CPU log never evicts, so the twin is a GPU engine fed through
    # the classic path
    gpu = GpuEngine(small_cfg(num_slots=256))
    twin = GpuEngine(small_cfg(num_slots=256))
    try:
        for e in (gpu, twin):
            for a in range(3):
                e.register_agent(a)
        for k in range(3):
            lens = [LENS[(i + k) % len(LENS)] for i in range(200)]
            recs, headers, payload = device_batch(
                lens, [i % 3 for i in range(200)], 512)
            seqs = gpu.enqueue_from_device(dev(headers), dev(payload))
            np.testing.assert_array_equal(
                seqs, twin.enqueue_batch(*classic_batch(recs, payload, 200)))
        assert gpu.evict_base() == twin.evict_base() == 600 - 256
        s = assert_same_state(gpu, twin, 3)
        assert len(s["pays"]) == 256
        want = [LENS[(i + 2) % len(LENS)] for i in range(200)]
        assert s["hdrs"]["payload_len"][-200:].tolist() == want
        assert s["pays"][-1] == pattern(want[-1], 199)
    finally:
        gpu.close()
        twin.close()


@pytest.mark.gpu
def test_gpu_bitmap_handle_split_on_device():
    from swarmdb_amd.runtime.gpu_engine import GpuEngine

    pool = 8
    eng = GpuEngine(small_cfg(num_bitmaps=pool))
    try:
        for a in range(4):
            eng.register_agent(a)
        bits = np.zeros(256, dtype=bool)
        for _ in range(pool + 3):  # push the handle past the pool depth
            eng.alloc_bitmap(bits)
        bits[[0, 2]] = True
        handle = eng.alloc_bitmap(bits)
        assert handle == pool + 3  # pool slot 3: handle != slot

        def send_copy():
            recs, headers, payload = device_batch([8], [BROADCAST], 16)
            recs["vis_mode"] = VIS_BITMAP
            recs["bitmap"] = handle  # headers is a view of recs
            return int(eng.enqueue_from_device(dev(headers), dev(payload))[0])

        first = send_copy()
        assert eng.get_status(first) == ST_DELIVERED  # not the error lane
        got = [eng.receive(a, 10).tolist() for a in range(4)]
        assert got == [[first], [], [first], []]
        hdrs, _ = eng.fetch(np.array([first], dtype=np.uint64))
        assert int(hdrs["bitmap"][0]) == handle % pool
        assert int(hdrs["bitmap_epoch"][0]) == handle

        second = send_copy()
        for _ in range(pool):  # recycle the pool slot
            eng.alloc_bitmap(np.ones(256, dtype=bool))
        assert [eng.receive(a, 10).tolist() for a in range(4)] == [[]] * 4
        assert eng.get_status(second) == ST_DELIVERED  # hidden, unread
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_error_lane():
    gpu, cpu = gpu_and_twin()
    try:
        for e in (gpu, cpu):
            for a in range(3):
                e.register_agent(a)
        # 8 rows, 6 sent: the oversize rows sit in the middle of a tensor
        # with spare rows, so an unbounded read would stay inside it and
        # show up as content
        _, headers, payload, n = error_lane_case(cap=8)
        seqs = gpu.enqueue_from_device(dev(headers), dev(payload), n)
        check_error_lane(gpu, seqs)
        check_error_lane(cpu, cpu.enqueue_from_device(headers, payload, n))
        assert_same_state(gpu, cpu, 3)
    finally:
        gpu.close()


def reply_both(gpu, cpu, dg, dc, agents, pay, lengths, **kw):
    a = gpu.reply_to_device(dg, agents, dev(pay), dev(lengths), 3,
                            timestamp=1.8e9, **kw)
    b = cpu.reply_to_device(dc, agents, pay, lengths, 3, timestamp=1.8e9,
                            **kw)
    np.testing.assert_array_equal(a, b)
    assert a.dtype == np.uint64
    return a


@pytest.mark.gpu
def test_gpu_reply_case_parity():
    gpu, cpu = gpu_and_twin()
    try:
        dg, agents = reply_case(gpu)
        dc, _ = reply_case(cpu)
        pay = reply_rows(12, 64, seed=3)
        seqs = reply_both(gpu, cpu, dg, dc, agents, pay, REPLY_LENGTHS)
        assert seqs.tolist() == [4, 5, 6]
        hdrs, _ = gpu.fetch(seqs)
        assert hdrs["sender"].tolist() == [1, 1, 3]
        assert hdrs["receiver"].tolist() == [5, 5, 4]
        assert_same_state(gpu, cpu, 8)
        reply_both(gpu, cpu, dg, dc, agents, pay, REPLY_LENGTHS, priority=1)
        before = gpu.total_messages()
        none = reply_both(gpu, cpu, dg, dc, agents, pay,
                          np.full(5, -1, dtype=np.int32))  # m == 0
        assert none.tolist() == [] and gpu.total_messages() == before
        assert_same_state(gpu, cpu, 8)
    finally:
        gpu.close()


@pytest.mark.gpu
def test_gpu_reply_compaction_across_waves_and_blocks():
    import torch

    gpu, cpu = gpu_and_twin()
    try:
        K, na = 80, 4
        recs, headers, payload = device_batch(
            [16 + i % 40 for i in range(na * K)],
            [i % na for i in range(na * K)], 64)
        recs["sender"] = 4 + np.arange(na * K) % 4  # headers views recs
        for e in (gpu, cpu):
            for a in range(8):
                e.register_agent(a)
            e.enqueue_from_device(headers if e is cpu else dev(headers),
                                  payload if e is cpu else dev(payload))
        agents = np.array([2, 0, 3, 1], dtype=np.uint32)
        dg = gpu.receive_to_device(agents, K, max_payload=64)
        dc = cpu.receive_to_device(agents, K, max_payload=64)
        assert dg.total == dc.total == na * K
        r = np.arange(na * K)
        pay = reply_rows(na * K, 64, seed=5)

        pattern_len = np.where(r % 3 != 1, (r * 7) % 65, -1).astype(np.int32)
        pattern_len[10] = 100  # above rstride: the error lane
        seqs = reply_both(gpu, cpu, dg, dc, agents, pay, pattern_len)
        assert len(seqs) == int((pattern_len >= 0).sum())
        assert gpu.get_status(int(seqs[7])) == ST_FAILED  # row 10: 8th kept
        assert_same_state(gpu, cpu, 8)

        every = ((r * 3) % 65).astype(np.int32)
        assert len(reply_both(gpu, cpu, dg, dc, agents, pay, every)) == na * K
        last = np.full(na * K, -1, dtype=np.int32)
        last[-1] = 33
        assert len(reply_both(gpu, cpu, dg, dc, agents, pay, last)) == 1
        assert_same_state(gpu, cpu, 8)

        # the reply comes out of torch kernels queued just before the
        # call, no sync: the engine drains the caller's stream itself
        t = dg.payload[: na * K]
        for _ in range(8):
            t = torch.bitwise_xor(t, 0x5A).roll(1, dims=1)
        want = dc.payload[: na * K]
        for _ in range(8):
            want = np.roll(want ^ np.uint8(0x5A), 1, axis=1)
        a = gpu.reply_to_device(dg, agents, t, dev(every), 3, timestamp=1.8e9)
        b = cpu.reply_to_device(dc, agents, np.ascontiguousarray(want), every,
                                3, timestamp=1.8e9)
        np.testing.assert_array_equal(a, b)
        assert_same_state(gpu, cpu, 8)
    finally:
        gpu.close()


@pytest.mark.gpu
def test_gpu_refusals_leave_state_alone():
    import torch

    gpu, _ = gpu_and_twin()
    try:
        for a in range(3):
            gpu.register_agent(a)
        _, headers, payload = device_batch([8] * 6, [1] * 6, 64)
        h, p = dev(headers), dev(payload)
        gpu.enqueue_from_device(h, p)
        agents = np.array([1], dtype=np.uint32)
        d = gpu.receive_to_device(agents, 8)
        before = gpu.total_messages()
        assert before == d.total == 6
        bad_sends = [
            (torch.from_numpy(headers), p),              # host tensor
            (h, torch.from_numpy(payload)),
            (h.to(torch.int8), p),                       # wrong dtype
            (h, p.to(torch.int32)),
            (h, dev(np.zeros((6, 128), np.uint8))[:, :64]),  # non-contiguous
            (h, dev(np.zeros((6, 40), np.uint8))),       # stride 40
            (h, dev(np.zeros((6, 528), np.uint8))),      # above slot_bytes
        ]
        for hh, pp in bad_sends:
            with pytest.raises(ValueError):
                gpu.enqueue_from_device(hh, pp)
        with pytest.raises(ValueError):  # n > cap
            gpu.enqueue_from_device(h, p, n=7)
        with pytest.raises(ValueError):  # misaligned rows
            gpu.enqueue_from_device(
                dev(np.zeros(7 * 48 + 8, np.uint8))[8:].view(7, 48)[:6], p)

        rp, lens = dev(reply_rows(8, 64, 1)), dev(np.zeros(8, np.int32))
        bad_replies = [
            (rp.cpu(), lens),                            # host tensor
            (rp, lens.cpu()),
            (rp, lens.to(torch.int64)),                  # wrong dtype
            (dev(np.zeros((8, 128), np.uint8))[:, :64], lens),
            (dev(np.zeros((8, 40), np.uint8)), lens),    # stride 40
            (dev(np.zeros((8, 528), np.uint8)), lens),   # above slot_bytes
            (rp, lens[:5]),                              # shorter than total
            (rp[:5], lens),
        ]
        for pp, ll in bad_replies:
            with pytest.raises(ValueError):
                gpu.reply_to_device(d, agents, pp, ll, 3)
        with pytest.raises(ValueError):  # not the polled list
            gpu.reply_to_device(d, np.array([1, 2], np.uint32), rp, lens, 3)
        # the binding refuses on its own, before any launch
        q = gpu.q
        with pytest.raises(ValueError):
            q.enqueue_from_device(h.data_ptr(), p.data_ptr(), 4097, 64)
        with pytest.raises(ValueError):
            q.enqueue_from_device(h.data_ptr(), p.data_ptr() + 8, 6, 64)
        with pytest.raises(ValueError):
            q.enqueue_from_device(0, p.data_ptr(), 6, 64)
        for stride in (0, 8, 40, 528):
            with pytest.raises(ValueError):
                q.enqueue_from_device(h.data_ptr(), p.data_ptr(), 6, stride)
        with pytest.raises(ValueError):
            q.reply_from_device(d.headers.data_ptr(), d.agent_row.data_ptr(),
                                lens.data_ptr() + 2, rp.data_ptr(), 6, 64,
                                agents, 3, -1, 4, 0.0)
        assert gpu.total_messages() == before
        assert (gpu.statuses(np.arange(6, dtype=np.uint64)) == ST_READ).all()
        assert gpu.peek_inbox(1).tolist() == list(range(6))
    finally:
        gpu.close()


def torch_reply(delivery):
    import torch

    # content_len: the int32 at byte 40 of each 48-B header
    lengths = delivery.headers.view(torch.int32)[:, 10].contiguous()
    return (delivery.payload[:, :64] + 1).contiguous(), lengths


@pytest.mark.gpu
def test_facade_device_send_gpu(tmp_path):
    from swarmdb_amd.runtime.gpu_engine import GpuEngine

    cfg = small_cfg(save_dir=str(tmp_path / "gpu"))
    db = SwarmsDB(config=cfg, engine=GpuEngine(cfg))
    try:
        seqs, contents = facade_loop(db, torch_reply)
        inbox = db.receive_device(["ann"])
        assert inbox.payload.is_cuda and inbox.total == 2
        check_replies(db, db.messages_from_delivery(inbox)[0], seqs, contents)
    finally:
        db.close()
