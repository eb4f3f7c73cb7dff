"""Device-resident conversation context: context_to_device.

The CPU engine's implementation is the plain-numpy double; it is checked
against an independent naive loop written here on Python ints, following
the contract line by line, and the HIP kernels (k_context_find,
k_context_gather) are checked against the double on a twin engine fed the
same batches. Every comparison is integer- or byte-exact.

The file holds CPU and GPU tests, so GPU tests carry the marker one by
one.
"""

import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest

from swarmdb_amd import DeviceContext, MessageType, QueueConfig, SwarmsDB
from swarmdb_amd.runtime.cpu_engine import CpuEngine
from swarmdb_amd.runtime.engine import (
    BROADCAST,
    NO_BITMAP,
    REC_DTYPE,
    ST_DELETED,
    ST_FAILED,
    VIS_ALL,
    VIS_BITMAP,
)

G = 4  # rows per workgroup of k_context_find (csrc: CONTEXT_GROUP)
G_WIDE = 16  # the alternative it is also built with (CONTEXT_GROUP_WIDE)
N_AGENTS = 6
SLOT = 48  # payload stride of the batches built here (16..48 B payloads)


def small_cfg(**kw):
    base = dict(
        use_gpu=True,
        max_agents=256,
        num_slots=1 << 14,
        slot_bytes=512,
        inbox_capacity=1 << 12,
        staging_batch=4096,
        num_backends=64,
        auto_save=False,
    )
    base.update(kw)
    return QueueConfig(**base)


def cpu_engine(**kw):
    return CpuEngine(small_cfg(use_gpu=False, **kw))


def gpu_and_twin(**kw):
    from swarmdb_amd.runtime.gpu_engine import GpuEngine

    return GpuEngine(small_cfg(**kw)), cpu_engine(**kw)


def register(engines, n=N_AGENTS):
    for e in engines:
        for a in range(n):
            e.register_agent(a)


def batch(senders, receivers, rng, types=None, priority=None):
    """REC_DTYPE records + payload buffer: 16..48 random bytes each."""
    n = len(senders)
    recs = np.zeros(n, dtype=REC_DTYPE)
    recs["sender"] = senders
    recs["receiver"] = receivers
    recs["type"] = rng.integers(0, 3, n) if types is None else types
    recs["priority"] = 1 if priority is None else priority
    recs["token_count"] = rng.integers(0, 100, n)
    recs["timestamp"] = 1.7e9 + rng.integers(0, 10 ** 6, n)
    recs["vis_mode"] = VIS_ALL
    recs["bitmap"] = NO_BITMAP
    recs["payload_off"] = np.arange(n, dtype=np.uint64) * SLOT
    recs["payload_len"] = rng.integers(16, SLOT + 1, n)
    recs["content_len"] = recs["payload_len"]
    buf = rng.integers(1, 256, n * SLOT + 16, dtype=np.uint8).tobytes()
    return recs, buf


def enqueue(engines, recs, buf, bitmap_rows=()):
    """The same batch on every engine; rows in ``bitmap_rows`` get a
    visibility bitmap allocated on each engine (agents 0 and 1)."""
    seqs = None
    for e in engines:
        r = recs.copy()
        for i in bitmap_rows:
            bits = np.zeros(e.cfg.max_agents, dtype=bool)
            bits[[0, 1]] = True
            r["bitmap"][i] = e.alloc_bitmap(bits)
        seqs = e.enqueue_batch(r, buf)
    return seqs


def traffic_mix(engines, n=150, seed=7):
    """Fixed-seed traffic among 6 agents: p2p in both directions, messages
    to oneself, plain broadcasts, one VIS_BITMAP p2p message, one record
    that takes the error lane (FAILED), one deleted message, three types.
    Returns the seqs of (bitmap, failed, deleted) messages."""
    rng = np.random.default_rng(seed)
    register(engines)
    snd = rng.integers(0, N_AGENTS, n)
    rcv = rng.integers(0, N_AGENTS, n)
    # a dense dialogue between 0 and 1 and between 2 and 3, both ways
    for i in range(0, n, 3):
        snd[i], rcv[i] = (0, 1) if (i // 3) % 2 else (1, 0)
    for i in range(1, n, 5):
        snd[i], rcv[i] = (2, 3) if (i // 5) % 2 else (3, 2)
    snd[10], rcv[10] = 1, 1  # to oneself
    snd[40], rcv[40] = 2, 2
    recs, buf = batch(snd, rcv, rng, priority=rng.integers(0, 4, n))
    for i in (20, 50, 80):  # plain broadcasts from a partner
        recs["sender"][i], recs["receiver"][i] = 0, BROADCAST
    i_bm, i_bad, i_del = 33, 63, 93  # all on the 0 <-> 1 dialogue
    recs["vis_mode"][i_bm] = VIS_BITMAP
    recs["type"][i_bad] = 9  # unknown type: the error lane
    assert {tuple(sorted((int(recs["sender"][i]), int(recs["receiver"][i]))))
            for i in (i_bm, i_bad, i_del)} == {(0, 1)}
    seqs = enqueue(engines, recs, buf, bitmap_rows=(i_bm,))
    base = int(seqs[0])
    for e in engines:
        assert e.delete(base + i_del)
        assert e.get_status(base + i_bad) == ST_FAILED
    return base + i_bm, base + i_bad, base + i_del


def host_log(eng, lo=0):
    """Host copy of the log [lo, total_messages()) as plain Python lists
    (what the naive loop reads) plus the arrays the expectation is built
    from."""
    hi = eng.total_messages()
    hdrs, flat, stride = eng.fetch_raw_chunks(np.arange(lo, hi, dtype=np.uint64))
    return SimpleNamespace(
        lo=lo, hi=hi, hdrs=hdrs, payload=flat.reshape(hi - lo, stride),
        sender=hdrs["sender"].tolist(), receiver=hdrs["receiver"].tolist(),
        type=hdrs["type"].tolist(), vis=hdrs["vis_mode"].tolist(),
        status=[int(x) for x in eng.statuses(
            np.arange(lo, hi, dtype=np.uint64))],
    )


def naive(log, d, agents, depth, lookback, code, base, count, max_agents):
    """The contract's pseudo-code on Python ints: the seqs of every row's
    context, ascending."""
    na, out = len(agents), []
    hdr = d.headers
    if hdr.dtype != REC_DTYPE:
        hdr = np.ascontiguousarray(hdr).view(REC_DTYPE).reshape(-1)
    for r in range(d.total):
        b = int(d.agent_row[r])
        a = int(agents[b]) if 0 <= b < na else None
        s = int(hdr["sender"][r])
        hi = min(max(int(d.seqs[r]), 0), count)
        lo = max(base, hi - lookback)
        if a is None or s >= max_agents:
            out.append([])
            continue
        m = []
        for q in range(hi - 1, lo - 1, -1):
            if len(m) == depth:
                break
            i = q - log.lo
            if log.status[i] in (ST_DELETED, ST_FAILED):
                continue
            if log.vis[i] != VIS_ALL:
                continue
            sn, rc = log.sender[i], log.receiver[i]
            if not ((sn == s and rc == a) or (sn == a and rc == s)):
                continue
            if code is not None and log.type[i] != code:
                continue
            m.append(q)
        out.append(m[::-1])
    return out


def assert_context(ctx, want, log):
    """A context against the naive loop's seqs and the log's records:
    counts, seqs, lengths, and headers + payload of defined slots."""
    h = ctx.to_host()
    D, stride = h.depth, h.stride
    assert h.counts.dtype == np.int32 and h.seqs.dtype == np.int64
    assert h.lengths.dtype == np.int32 and h.payload.dtype == np.uint8
    assert h.headers.dtype == REC_DTYPE
    assert h.seqs.shape == (h.total, D) and h.lengths.shape == (h.total, D)
    assert h.payload.shape == (h.total, D, stride)
    assert len(want) == h.total
    for r, m in enumerate(want):
        c = len(m)
        assert h.counts[r] == c, (r, h.counts[r], m)
        assert h.seqs[r, :c].tolist() == m, r
        assert (h.seqs[r, c:] == -1).all() and (h.lengths[r, c:] == 0).all()
        for j, q in enumerate(m):
            src = log.hdrs[q - log.lo]
            got = h.headers[r, j]
            plen = int(src["payload_len"])
            n = min(plen, stride)
            assert h.lengths[r, j] == n
            for name in REC_DTYPE.names:
                if name == "payload_off":
                    assert got[name] == (r * D + j) * stride
                else:
                    assert got[name] == src[name], (r, j, name)
            row = np.zeros(stride, dtype=np.uint8)
            row[:n] = log.payload[q - log.lo, :n]
            np.testing.assert_array_equal(h.payload[r, j], row)


def assert_same_context(g, c):
    """GPU result against the CPU twin's: counts, seqs and lengths whole,
    headers and payload (zero tails included) in defined slots."""
    hg, hc = g.to_host(), c.to_host()
    assert (hg.total, hg.depth, hg.stride) == (hc.total, hc.depth, hc.stride)
    for name in ("counts", "seqs", "lengths"):
        a, b = getattr(hg, name), getattr(hc, name)
        assert a.dtype == b.dtype and a.shape == b.shape, name
        np.testing.assert_array_equal(a, b, name)
    live = hc.seqs >= 0
    assert (live.sum(axis=1) == hc.counts).all()
    np.testing.assert_array_equal(
        hg.headers[live].view(np.uint8), hc.headers[live].view(np.uint8))
    np.testing.assert_array_equal(hg.payload[live], hc.payload[live])


def to_numpy_delivery(d):
    """Host numpy copy of a delivery, headers as uint8 [rows, 48]."""
    h = d.to_host()
    return dataclasses.replace(
        h, headers=h.headers.view(np.uint8).reshape(h.total, 48).copy())


POLLED = np.array([1, 2, 0, 3], dtype=np.uint32)


def mix_delivery(engines, **kw):
    """traffic_mix + one poll of POLLED on every engine."""
    marks = traffic_mix(engines)
    ds = [e.receive_to_device(POLLED, 200, **kw) for e in engines]
    assert all(d.total == ds[0].total and d.total > 60 for d in ds)
    return marks, ds


def expect(eng, d, agents, depth, lookback, code=None, base=None):
    log = host_log(eng)
    want = naive(
        log, to_numpy_delivery(d), agents, depth, lookback, code,
        eng.evict_base() if base is None else base, eng.total_messages(),
        eng.cfg.max_agents)
    return want, log


# ---------------------------------------------------------------- CPU


@pytest.mark.parametrize("depth,lookback", [(1, 1000), (3, 40), (8, 1000),
                                            (64, 1000), (8, 1)])
def test_double_matches_naive_loop(depth, lookback):
    eng = cpu_engine()
    (bm, bad, dele), (d,) = mix_delivery([eng])
    ctx = eng.context_to_device(d, POLLED, depth, lookback)
    assert isinstance(ctx, DeviceContext)
    assert (ctx.depth, ctx.stride, ctx.total) == (depth, 512, d.total)
    want, log = expect(eng, d, POLLED, depth, lookback)
    assert_context(ctx, want, log)
    if (depth, lookback) == (64, 1000):
        shown = {q for m in want for q in m}
        assert not shown & {bm, bad, dele}
        assert not any(log.receiver[q] == BROADCAST for q in shown)
        assert any(log.sender[q] == log.receiver[q] for q in shown)
        assert {log.type[q] for q in shown} == {0, 1, 2}
        assert max(len(m) for m in want) > 8 and min(len(m) for m in want) == 0


def test_double_priority_order_rows():
    """Rows in priority order: non-monotonic seqs, every row its own hi."""
    eng = cpu_engine()
    _, (d,) = mix_delivery([eng], priority_order=True)
    assert (np.diff(d.seqs[:d.counts[0]]) < 0).any()
    ctx = eng.context_to_device(d, POLLED, 4, 50)
    want, log = expect(eng, d, POLLED, 4, 50)
    assert_context(ctx, want, log)
    for r, m in enumerate(want):
        assert all(q < d.seqs[r] for q in m)


def dialogue(engines, n_before, extra=0):
    """n_before messages 0 -> 1 (drained), then one 0 -> 1 trigger that
    is delivered as the only row; `extra` unrelated messages in between."""
    rng = np.random.default_rng(n_before)
    register(engines)
    snd = [0] * n_before + [4] * extra
    rcv = [1] * n_before + [5] * extra
    if snd:
        enqueue(engines, *batch(snd, rcv, rng))
    agents = np.array([1], dtype=np.uint32)
    for e in engines:
        e.receive_to_device(agents, 4096)
    enqueue(engines, *batch([0], [1], rng))
    return agents, [e.receive_to_device(agents, 4) for e in engines]


@pytest.mark.parametrize("n_before", [0, 5, 9])
def test_ordering_and_truncation(n_before):
    """depth 5 against zero, exactly depth, and more matches than depth:
    the newest `depth`, ascending."""
    eng = cpu_engine()
    agents, (d,) = dialogue([eng], n_before, extra=3)
    assert d.total == 1 and d.seqs[0] == n_before + 3
    ctx = eng.context_to_device(d, agents, 5, 1000)
    keep = list(range(n_before))[-5:]
    assert ctx.counts[0] == len(keep)
    assert ctx.seqs[0].tolist() == keep + [-1] * (5 - len(keep))
    want, log = expect(eng, d, agents, 5, 1000)
    assert want == [keep]
    assert_context(ctx, want, log)


def test_type_code_filter():
    eng = cpu_engine()
    _, (d,) = mix_delivery([eng])
    plain = eng.context_to_device(d, POLLED, 8, 1000).to_host()
    for code in (0, 2, 6):
        ctx = eng.context_to_device(d, POLLED, 8, 1000, type_code=code)
        want, log = expect(eng, d, POLLED, 8, 1000, code)
        assert_context(ctx, want, log)
        h = ctx.to_host()
        live = h.seqs >= 0
        assert (h.headers["type"][live] == code).all()
        assert live.any() == (code != 6)
    assert len(set(plain.headers["type"][plain.seqs >= 0].tolist())) == 3


def test_max_payload_truncates_rows_not_headers():
    eng = cpu_engine()
    _, (d,) = mix_delivery([eng])
    ctx = eng.context_to_device(d, POLLED, 8, 1000, max_payload=20)
    assert ctx.stride == 32 and ctx.payload.shape[2] == 32
    want, log = expect(eng, d, POLLED, 8, 1000)
    assert_context(ctx, want, log)
    h = ctx.to_host()
    live = h.seqs >= 0
    plen = h.headers["payload_len"][live]
    assert (plen > 32).any() and (plen <= 32).any()
    np.testing.assert_array_equal(h.lengths[live], np.minimum(plen, 32))


def tamper(d, total_messages, na, max_agents):
    """Overwrite rows 0..5 of a numpy delivery with the out-of-range
    values of the contract; returns the rows."""
    hdr = d.headers.view(REC_DTYPE).reshape(-1)
    d.seqs[0] = -5
    d.seqs[1] = total_messages + 1000
    d.agent_row[2] = -1
    d.agent_row[3] = na
    hdr["sender"][4] = max_agents
    hdr["sender"][5] = BROADCAST
    return [0, 1, 2, 3, 4, 5]


def test_tampered_inputs_are_values():
    eng = cpu_engine()
    _, (d,) = mix_delivery([eng])
    d = to_numpy_delivery(d)
    rows = tamper(d, eng.total_messages(), len(POLLED), eng.cfg.max_agents)
    ctx = eng.context_to_device(d, POLLED, 8, 1000)
    want, log = expect(eng, d, POLLED, 8, 1000)
    assert_context(ctx, want, log)
    assert [len(want[r]) for r in rows[:1] + rows[2:]] == [0] * 5
    # the seq above the log is clamped to its end: the newest 8 of the pair
    assert len(want[1]) == 8


def snapshot(eng):
    st = eng.stats_arrays()
    n = eng.total_messages()
    lo = eng.evict_base()
    return (
        {k: np.array(v) for k, v in st.items()},
        eng.statuses(np.arange(lo, n, dtype=np.uint64)).copy(),
        eng.backend_loads().copy(),
    )


def assert_read_only(eng, other):
    """`eng` and `other` hold the same traffic, both polled once with a
    small K; only `eng` gathers a context. Nothing observable moves, and
    the next poll delivers on both what it would have."""
    traffic_mix([eng, other])
    d, d_other = (e.receive_to_device(POLLED, 10) for e in (eng, other))
    eng.backend_add_load(1, 7)
    before = snapshot(eng)
    ctx = eng.context_to_device(d, POLLED, 8, 1000)
    assert int(ctx.to_host().counts.sum()) > 0
    after = snapshot(eng)
    for k in before[0]:
        np.testing.assert_array_equal(before[0][k], after[0][k], k)
    np.testing.assert_array_equal(before[1], after[1])
    np.testing.assert_array_equal(before[2], after[2])
    n1, n2 = (e.receive_to_device(POLLED, 200).to_host() for e in (eng, other))
    assert n1.total == n2.total > 0
    np.testing.assert_array_equal(n1.counts, n2.counts)
    np.testing.assert_array_equal(n1.seqs, n2.seqs)
    assert d.total == d_other.total


def test_read_only_cpu():
    assert_read_only(cpu_engine(), cpu_engine())


def arg_refusals(eng, d):
    """The refusals that need no array of the wrong kind."""
    good = dict(agent_idxs=POLLED, depth=8, lookback=100)
    bad = [
        dict(depth=0), dict(depth=65), dict(depth=-1),
        dict(lookback=0), dict(lookback=2 ** 31), dict(lookback=-3),
        dict(type_code=256), dict(type_code=-1),
        dict(agent_idxs=POLLED[:3]),
        dict(agent_idxs=np.append(POLLED, 4).astype(np.uint32)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            eng.context_to_device(d, **{**good, **kw})
    wide = np.arange(eng.cfg.max_agents + 1, dtype=np.uint32)
    many = dataclasses.replace(
        d, counts=np.zeros(len(wide), dtype=np.int64))
    with pytest.raises(ValueError):  # na > max_agents
        eng.context_to_device(many, wide, 8, 100)


def test_refusals_cpu():
    eng = cpu_engine()
    _, (d,) = mix_delivery([eng])
    arg_refusals(eng, d)
    wrong = [
        dataclasses.replace(d, seqs=d.seqs.astype(np.int32)),
        dataclasses.replace(d, agent_row=d.agent_row.astype(np.int64)),
        dataclasses.replace(d, headers=d.headers[:, :40]),
        dataclasses.replace(d, agent_row=d.agent_row.tolist()),
        dataclasses.replace(d, seqs=d.seqs[::2]),
        dataclasses.replace(d, agent_row=d.agent_row[:d.total - 1]),
        dataclasses.replace(d, seqs=d.seqs.reshape(-1, 1)),
    ]
    for w in wrong:
        with pytest.raises(ValueError):
            eng.context_to_device(w, POLLED, 8, 100)
    good = eng.context_to_device(d, POLLED, 8, 100)
    fresh = good.to_host()
    outs = [
        dataclasses.replace(good, depth=4),
        dataclasses.replace(good, stride=256),
        dataclasses.replace(good, seqs=good.seqs[:d.total - 1]),
        dataclasses.replace(good, payload=good.payload[:, :, :64]),
        dataclasses.replace(good, counts=good.counts.tolist()),
        d,
    ]
    for o in outs:
        with pytest.raises(ValueError):
            eng.context_to_device(d, POLLED, 8, 100, out=o)
    with pytest.raises(ValueError):  # built for another depth
        eng.context_to_device(d, POLLED, 4, 100, out=good)
    with pytest.raises(ValueError):  # built for another stride
        eng.context_to_device(d, POLLED, 8, 100, max_payload=32, out=good)
    good.seqs[:] = 77
    good.payload[:] = 0xEE
    again = eng.context_to_device(d, POLLED, 8, 100, out=good)
    assert again.seqs is good.seqs and again.payload is good.payload
    assert_same_context(again, fresh)


def facade_round_trip(db):
    """A dialogue of fewer than `depth` unrestricted p2p messages per
    direction, nothing deleted: the context of the trigger's row is
    get_conversation's newest `depth`, oldest first."""
    for i in range(5):
        db.send_message("ann", f"ann-{i}", receiver_id="bob")
        db.send_message("bob", {"n": i}, receiver_id="ann",
                        message_type=MessageType.COMMAND)
        db.send_message("cy", f"noise-{i}", receiver_id="bob")
        if i == 2:
            db.send_message("ann", "to all")
    db.receive_device(["bob"])  # drained: the next poll has the trigger only
    conv = db.get_conversation("bob", "ann", sort=True)
    assert len(conv) == 10
    db.send_message("ann", "trigger", receiver_id="bob")
    d = db.receive_device(["bob"])
    assert d.total == 1
    ctx = db.context_device(d, ["bob"])
    assert ctx.depth == 8 and ctx.to_host().counts.tolist() == [8]
    got = db.messages_from_context(ctx, 0)

    def key(m):
        return (m.id, m.sender_id, m.receiver_id, m.content, m.type,
                m.timestamp)

    assert [key(m) for m in got] == [key(m) for m in conv[-8:]]
    only = db.context_device(d, ["bob"], depth=3,
                             message_type=MessageType.COMMAND)
    assert [m.content for m in db.messages_from_context(only, 0)] == [
        {"n": 2}, {"n": 3}, {"n": 4}]
    again = db.context_device(d, ["bob"], out=ctx)
    assert again.seqs is ctx.seqs
    with pytest.raises(ValueError):
        db.context_device(d, ["bob", "ann"])
    with pytest.raises(ValueError):
        db.context_device(d, ["nobody"])
    with pytest.raises(ValueError):
        db.messages_from_context(ctx, 1)
    cut = db.context_device(d, ["bob"], max_payload=16)
    with pytest.raises(ValueError):
        db.messages_from_context(cut, 0)


def test_facade_context_cpu(tmp_db):
    facade_round_trip(tmp_db)


# ---------------------------------------------------------------- GPU


@pytest.mark.gpu
def test_gpu_parity_on_the_mix():
    """Depths and lookbacks that straddle the 64-entry ballot and the
    256-seq tile, on the CPU tests' traffic, with and without the type
    filter and the tighter stride."""
    import torch  # noqa: F401  (before GpuEngine: torch's HIP runtime first)

    from swarmdb_amd import _swarmq

    assert _swarmq.CONTEXT_GROUP == G
    assert _swarmq.CONTEXT_GROUP_WIDE == G_WIDE
    gpu, cpu = gpu_and_twin()
    try:
        # a longer log than the CPU mix alone, so that lookbacks up to
        # 1000 see more than one tile
        for seed in (1, 2, 3):
            traffic_mix([gpu, cpu], n=150, seed=seed)
        for e in (gpu, cpu):
            e.receive_to_device(POLLED, 4096)
        _, (dg, dc) = mix_delivery([gpu, cpu])
        np.testing.assert_array_equal(dg.seqs[:dg.total].cpu().numpy(),
                                      dc.seqs[:dc.total])
        for depth in (1, 3, 8, 64):
            for lookback in (1, 63, 64, 65, 255, 256, 257, 1000):
                g = gpu.context_to_device(dg, POLLED, depth, lookback)
                c = cpu.context_to_device(dc, POLLED, depth, lookback)
                for t in (g.counts, g.seqs, g.lengths, g.headers, g.payload):
                    assert t.is_cuda
                assert_same_context(g, c)
        g = gpu.context_to_device(dg, POLLED, 8, 257, type_code=1,
                                  max_payload=20)
        c = cpu.context_to_device(dc, POLLED, 8, 257, type_code=1,
                                  max_payload=20)
        assert g.stride == 32
        assert_same_context(g, c)
        assert int(c.counts.sum()) > 0
        # four rows per wavefront: the same answer
        for depth, lookback in ((8, 257), (64, 1000), (3, 65)):
            gw = gpu.context_to_device(dg, POLLED, depth, lookback,
                                       group=G_WIDE)
            assert_same_context(
                gw, cpu.context_to_device(dc, POLLED, depth, lookback))
        with pytest.raises(ValueError):
            gpu.context_to_device(dg, POLLED, 8, 257, group=8)
    finally:
        gpu.close()


def split3(total):
    a, b = total * 2 // 5, total // 4
    return [a, b, total - a - b]


@pytest.mark.gpu
@pytest.mark.parametrize("G", [G, G_WIDE])
def test_gpu_row_count_boundaries(G):
    """delivery.total around the rows-per-workgroup G, three polled agents
    with uneven counts: a workgroup's rows span two agents."""
    import torch  # noqa: F401

    gpu, cpu = gpu_and_twin()
    try:
        traffic_mix([gpu, cpu])
        everyone = np.arange(N_AGENTS, dtype=np.uint32)
        agents = np.array([1, 2, 3], dtype=np.uint32)
        for total in (0, 1, G - 1, G, G + 1, 4 * G + 1):
            for e in (gpu, cpu):
                e.receive_to_device(everyone, 4096)
            counts = split3(total)
            rng = np.random.default_rng(total)
            rcv = np.repeat(agents, counts)
            if total:
                enqueue([gpu, cpu],
                        *batch(rng.integers(0, N_AGENTS, total), rcv, rng))
            dg = gpu.receive_to_device(agents, max(max(counts), 1))
            dc = cpu.receive_to_device(agents, max(max(counts), 1))
            assert dg.counts.tolist() == dc.counts.tolist() == counts
            g = gpu.context_to_device(dg, agents, 8, 1000, group=G)
            c = cpu.context_to_device(dc, agents, 8, 1000)
            assert g.total == total
            assert_same_context(g, c)
            if total > G:
                arow = dc.agent_row[:total].tolist()
                assert any(len(set(arow[k:k + G])) > 1
                           for k in range(0, total, G))
                assert int(c.counts[:total].sum()) > 0
    finally:
        gpu.close()


@pytest.mark.gpu
def test_gpu_matches_at_tile_edges():
    """Matches at hi-1, hi-64, hi-65, hi-256, hi-257, exactly lo and
    lo-1 of one row; each depth makes another of them the last one taken,
    and lo-1 never appears."""
    import torch  # noqa: F401

    gpu, cpu = gpu_and_twin()
    try:
        register([gpu, cpu])
        hi, lookback = 700, 600
        at = [hi - 1, hi - 64, hi - 65, hi - 256, hi - 257, hi - 600, hi - 601]
        snd = np.full(hi, 4)
        rcv = np.full(hi, 5)
        for k, q in enumerate(at):  # both directions of the 0 <-> 1 pair
            snd[q], rcv[q] = (0, 1) if k % 2 else (1, 0)
        rng = np.random.default_rng(0)
        enqueue([gpu, cpu], *batch(snd, rcv, rng))
        agents = np.array([1], dtype=np.uint32)
        for e in (gpu, cpu):
            e.receive_to_device(agents, 4096)
        enqueue([gpu, cpu], *batch([0], [1], rng))
        dg = gpu.receive_to_device(agents, 4)
        dc = cpu.receive_to_device(agents, 4)
        assert dc.total == 1 and dc.seqs[0] == hi
        for depth in range(1, 8):
            g = gpu.context_to_device(dg, agents, depth, lookback)
            c = cpu.context_to_device(dc, agents, depth, lookback)
            assert_same_context(g, c)
            keep = sorted(at[:6])[-depth:]
            got = g.to_host()
            assert got.counts[0] == len(keep)
            assert got.seqs[0, :len(keep)].tolist() == keep
    finally:
        gpu.close()


@pytest.mark.gpu
def test_gpu_rows_of_one_block_have_their_own_windows():
    """Priority-ordered delivery: the seqs within a workgroup's rows are
    not monotonic, and every row honours its own hi."""
    import torch  # noqa: F401

    gpu, cpu = gpu_and_twin()
    try:
        _, (dg, dc) = mix_delivery([gpu, cpu], priority_order=True)
        np.testing.assert_array_equal(dg.seqs[:dg.total].cpu().numpy(),
                                      dc.seqs[:dc.total])
        for rows in (G, G_WIDE):  # workgroups whose rows go back in seq
            assert sum((np.diff(dc.seqs[k:k + rows]) < 0).any()
                       for k in range(0, dc.total, rows)) >= 4
        for depth, lookback, group in ((4, 50, G), (8, 1000, G_WIDE),
                                       (64, 20, G), (8, 300, G_WIDE)):
            g = gpu.context_to_device(dg, POLLED, depth, lookback,
                                      group=group)
            c = cpu.context_to_device(dc, POLLED, depth, lookback)
            assert_same_context(g, c)
            h = g.to_host()
            own = dc.seqs[:dc.total, None]
            assert ((h.seqs < own) | (h.seqs == -1)).all()
            assert ((h.seqs >= own - lookback) | (h.seqs == -1)).all()
    finally:
        gpu.close()


@pytest.mark.gpu
def test_gpu_eviction():
    """num_slots 256 and 700 messages: the ring wrapped twice. The twin
    retains everything, so the expectation is the naive loop over the
    twin's log with lo clamped to the GPU engine's evict_base()."""
    import torch  # noqa: F401

    gpu, cpu = gpu_and_twin(num_slots=256)
    try:
        register([gpu, cpu])
        rng = np.random.default_rng(5)
        for _ in range(7):
            snd = rng.integers(0, 3, 100)
            rcv = rng.integers(0, 3, 100)
            enqueue([gpu, cpu], *batch(snd, rcv, rng))
        base = gpu.evict_base()
        assert base == 700 - 256 and gpu.total_messages() == 700
        agents = np.array([0, 1, 2], dtype=np.uint32)
        dg = gpu.receive_to_device(agents, 300)
        assert dg.total > 100
        g = gpu.context_to_device(dg, agents, 8, 1000)
        log = host_log(cpu)
        want = naive(log, to_numpy_delivery(dg), agents, 8, 1000, None, base,
                     700, gpu.cfg.max_agents)
        assert_context(g, want, log)
        h = g.to_host()
        assert ((h.seqs >= base) | (h.seqs == -1)).all()
        assert any(len(m) < 8 for m in want) and any(len(m) == 8 for m in want)
    finally:
        gpu.close()


def fill_batch(senders, receivers, lens, fill, slot=512):
    """REC_DTYPE records + payload buffer: payload i is lens[i] bytes of
    `fill`, at offset i * slot of a buffer that holds nothing else."""
    n = len(senders)
    recs = np.zeros(n, dtype=REC_DTYPE)
    recs["sender"] = senders
    recs["receiver"] = receivers
    recs["priority"] = 1
    recs["timestamp"] = 1.7e9
    recs["vis_mode"] = VIS_ALL
    recs["bitmap"] = NO_BITMAP
    recs["payload_off"] = np.arange(n, dtype=np.uint64) * slot
    recs["payload_len"] = lens
    recs["content_len"] = lens
    buf = np.zeros(n * slot + 16, dtype=np.uint8)
    for i, ln in enumerate(lens):
        buf[i * slot:i * slot + ln] = fill
    return recs, buf.tobytes()


@pytest.mark.gpu
def test_gpu_stale_tail_after_ring_wrap():
    """The twin of the delivery test of this name: every slot of a 64-slot
    ring first holds 512 bytes of 0xFF and is then reused by a payload of
    0..33 bytes of 0x41. A context slot shows the new payload, zeros from
    its length to the stride, and never the previous occupant's bytes —
    also where the stride (16) cuts a payload short."""
    import torch  # noqa: F401

    gpu, cpu = gpu_and_twin(num_slots=64, inbox_capacity=256)
    try:
        register([gpu, cpu], 2)
        both = np.array([0, 1], dtype=np.uint32)
        snd = np.arange(64) % 2  # 0 -> 1, 1 -> 0, ...
        enqueue([gpu, cpu], *fill_batch(snd, 1 - snd, [512] * 64, 0xFF))
        for e in (gpu, cpu):
            assert e.receive_to_device(both, 64).total == 64
        cyc = [0, 1, 5, 15, 16, 17, 31, 32, 33]
        lens = [cyc[i % len(cyc)] for i in range(64)]
        seqs = enqueue([gpu, cpu], *fill_batch(snd, 1 - snd, lens, 0x41))
        assert seqs.tolist() == list(range(64, 128))  # every slot is reused
        assert gpu.evict_base() == 64
        # the twin's log has no ring: what the ring evicted is deleted there
        for q in range(64):
            assert cpu.delete(q)
        agents = np.array([1], dtype=np.uint32)
        dg = gpu.receive_to_device(agents, 64)
        dc = cpu.receive_to_device(agents, 64)
        assert dg.total == dc.total == 32
        len_of = dict(zip(seqs.tolist(), lens))
        for max_payload, stride in ((0, 512), (16, 16)):
            g = gpu.context_to_device(dg, agents, 8, 128,
                                      max_payload=max_payload)
            c = cpu.context_to_device(dc, agents, 8, 128,
                                      max_payload=max_payload)
            assert g.stride == stride
            h = g.to_host()
            live = h.seqs >= 0
            assert live.sum() == sum(min(8, 2 * r) for r in range(32))
            assert h.seqs[live].min() == 64
            plen = np.array([len_of[q] for q in h.seqs[live].tolist()])
            assert set(plen.tolist()) == set(cyc)
            np.testing.assert_array_equal(h.headers["payload_len"][live], plen)
            np.testing.assert_array_equal(
                h.lengths[live], np.minimum(plen, stride))
            rows = h.payload[live]
            below = np.arange(stride)[None, :] < h.lengths[live][:, None]
            assert (rows[below] == 0x41).all()
            assert not rows[~below].any()
            assert_same_context(g, c)
    finally:
        gpu.close()


@pytest.mark.gpu
def test_gpu_status_filter_and_tampered_rows():
    """A match deleted and another marked FAILED after the delivery never
    appear; out-of-range seqs, agent rows and senders are values."""
    import torch

    gpu, cpu = gpu_and_twin()
    try:
        _, (dg, dc) = mix_delivery([gpu, cpu])
        first = cpu.context_to_device(dc, POLLED, 8, 1000).to_host()
        r = int(np.argmax(first.counts))
        gone, failed = int(first.seqs[r, 7]), int(first.seqs[r, 5])
        for e in (gpu, cpu):
            assert e.delete(gone)
            e.set_status(failed, ST_FAILED)
        g = gpu.context_to_device(dg, POLLED, 8, 1000)
        c = cpu.context_to_device(dc, POLLED, 8, 1000)
        assert_same_context(g, c)
        shown = g.to_host().seqs
        assert not np.isin(shown, [gone, failed]).any()
        assert first.seqs[r, 6] in shown[r]

        dn = to_numpy_delivery(dc)
        rows = tamper(dn, cpu.total_messages(), len(POLLED),
                      cpu.cfg.max_agents)
        dev = dg.seqs.device
        dg.seqs[:dg.total] = torch.from_numpy(dn.seqs).to(dev)
        dg.agent_row[:dg.total] = torch.from_numpy(dn.agent_row).to(dev)
        dg.headers[:dg.total] = torch.from_numpy(dn.headers).to(dev)
        g = gpu.context_to_device(dg, POLLED, 8, 1000)
        c = cpu.context_to_device(dn, POLLED, 8, 1000)
        assert_same_context(g, c)
        hc = c.to_host()
        assert hc.counts[rows].tolist() == [0, 8, 0, 0, 0, 0]
    finally:
        gpu.close()


@pytest.mark.gpu
def test_gpu_out_reuse_and_refusals():
    import torch

    gpu, cpu = gpu_and_twin()
    try:
        _, (dg, dc) = mix_delivery([gpu, cpu])
        arg_refusals(gpu, dg)
        wrong = [
            dataclasses.replace(dg, seqs=dg.seqs.to(torch.int32)),
            dataclasses.replace(dg, agent_row=dg.agent_row.to(torch.int64)),
            dataclasses.replace(dg, headers=dg.headers.to(torch.int8)),
            dataclasses.replace(dg, seqs=dg.seqs.cpu()),
            dataclasses.replace(dg, headers=dg.headers.cpu()),
            dataclasses.replace(dg, agent_row=dg.agent_row[::2]),
            dataclasses.replace(dg, headers=dg.headers[:, :40]),
            dataclasses.replace(dg, seqs=dg.seqs[:dg.total - 1]),
            dataclasses.replace(dg, seqs=dg.seqs.cpu().numpy()),
        ]
        for w in wrong:
            with pytest.raises(ValueError):
                gpu.context_to_device(w, POLLED, 8, 100)
        g = gpu.context_to_device(dg, POLLED, 8, 100)
        c = cpu.context_to_device(dc, POLLED, 8, 100)
        assert_same_context(g, c)
        outs = [
            dataclasses.replace(g, seqs=g.seqs.to(torch.int32)),
            dataclasses.replace(g, payload=g.payload.cpu()),
            dataclasses.replace(g, lengths=g.lengths[::2]),
            dataclasses.replace(g, counts=g.counts[:dg.total - 1]),
            dataclasses.replace(g, depth=4),
            dataclasses.replace(g, stride=256),
        ]
        for o in outs:
            with pytest.raises(ValueError):
                gpu.context_to_device(dg, POLLED, 8, 100, out=o)
        with pytest.raises(ValueError):  # built for another depth
            gpu.context_to_device(dg, POLLED, 4, 100, out=g)

        # a second, smaller delivery into the same buffers
        for e in (gpu, cpu):
            e.receive_to_device(POLLED, 4096)
        rng = np.random.default_rng(11)
        enqueue([gpu, cpu], *batch([0, 1, 0, 3, 1], [1, 0, 1, 2, 0], rng))
        dg2 = gpu.receive_to_device(POLLED, 200)
        dc2 = cpu.receive_to_device(POLLED, 200)
        assert dg2.total == dc2.total == 5
        g2 = gpu.context_to_device(dg2, POLLED, 8, 100, out=g)
        c2 = cpu.context_to_device(dc2, POLLED, 8, 100, out=c)
        assert g2.seqs is g.seqs and g2.total == 5
        assert_same_context(g2, c2)
        assert int(c2.counts[:5].sum()) > 0
    finally:
        gpu.close()


@pytest.mark.gpu
def test_read_only_gpu():
    import torch  # noqa: F401

    gpu, cpu = gpu_and_twin()
    try:
        assert_read_only(gpu, cpu)
    finally:
        gpu.close()


@pytest.mark.gpu
def test_facade_context_gpu(tmp_path):
    import torch  # noqa: F401

    from swarmdb_amd.runtime.gpu_engine import GpuEngine

    cfg = small_cfg(save_dir=str(tmp_path / "gpu"))
    db = SwarmsDB(config=cfg, engine=GpuEngine(cfg))
    try:
        facade_round_trip(db)
        d = db.receive_device(["bob"])
        assert d.total == 0
        ctx = db.context_device(d, ["bob"])
        assert ctx.seqs.is_cuda and ctx.total == 0
        assert ctx.to_host().seqs.shape == (0, 8)
    finally:
        db.close()
