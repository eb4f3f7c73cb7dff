"""Visibility-checked conversation context: context_to_device(shared=True).

With ``shared=True`` the context of a row holds what one of the two
parties wrote and the other was allowed to see — broadcasts and group
messages included, visibility checked as delivery checks it. The chain is
the one of test_device_context.py: a naive loop written here on Python
ints from the contract's pseudo-code (bitmaps through ``read_bitmap``),
then the numpy double, then the HIP kernel, which is compared byte for
byte with the double run over the GPU engine's own log. Every comparison
is integer- or byte-exact.

The file holds CPU and GPU tests, so GPU tests carry the marker one by
one.
"""

import numpy as np
import pytest

from swarmdb_amd import MessageType, SwarmsDB
from swarmdb_amd.runtime.engine import (
    BROADCAST,
    NO_BITMAP,
    REC_DTYPE,
    ST_DELETED,
    ST_FAILED,
    VIS_ALL,
    VIS_BITMAP,
    VIS_GROUP,
    Engine,
)
from test_device_context import (
    G,
    G_WIDE,
    POLLED,
    assert_context,
    assert_same_context,
    batch,
    cpu_engine,
    gpu_and_twin,
    host_log,
    naive as naive_plain,
    register,
    small_cfg,
    snapshot,
    tamper,
    to_numpy_delivery,
)

N_AGENTS = 8


# ------------------------------------------------------------ the contract


def shared_log(eng, lo=0):
    """host_log plus the two record fields the visibility check reads."""
    log = host_log(eng, lo)
    log.bitmap = log.hdrs["bitmap"].tolist()
    log.epoch = log.hdrs["bitmap_epoch"].tolist()
    return log


def sees(eng, log, i, x, cache):
    """What a poll by agent x does with log entry i once it is in x's
    inbox."""
    vis = log.vis[i]
    if vis not in (VIS_BITMAP, VIS_GROUP):
        return True
    bm = log.bitmap[i]
    if bm == NO_BITMAP:
        return not (vis == VIS_GROUP and log.receiver[i] == BROADCAST)
    if bm >= eng.cfg.num_bitmaps:
        return False
    key = (bm, log.epoch[i])
    if key not in cache:
        cache[key] = eng.read_bitmap(*key)
    bits = cache[key]
    if bits is None:  # recycled: hidden for good
        return False
    return x < len(bits) and bool(bits[x])


def naive(eng, log, d, agents, depth, lookback, code, base, count):
    """The contract's pseudo-code for shared=True on Python ints: the seqs
    of every row's context, ascending. ``eng`` owns the bitmaps the log's
    records name."""
    na, out, cache = len(agents), [], {}
    hdr = d.headers
    if hdr.dtype != REC_DTYPE:
        hdr = np.ascontiguousarray(hdr).view(REC_DTYPE).reshape(-1)
    for r in range(d.total):
        b = int(d.agent_row[r])
        a = int(agents[b]) if 0 <= b < na else None
        s = int(hdr["sender"][r])
        hi = min(max(int(d.seqs[r]), 0), count)
        lo = max(base, hi - lookback)
        if a is None or s >= eng.cfg.max_agents:
            out.append([])
            continue
        m = []
        for q in range(hi - 1, lo - 1, -1):
            if len(m) == depth:
                break
            i = q - log.lo
            if log.status[i] in (ST_DELETED, ST_FAILED):
                continue
            if code is not None and log.type[i] != code:
                continue
            sn, rc = log.sender[i], log.receiver[i]
            if sn == s and rc in (a, BROADCAST) and sees(eng, log, i, a, cache):
                m.append(q)
            elif sn == a and rc in (s, BROADCAST) \
                    and sees(eng, log, i, s, cache):
                m.append(q)
        out.append(m[::-1])
    return out


def expect(eng, d, agents, depth, lookback, code=None, base=None, log=None):
    """Naive seqs of ``d`` over ``eng``'s own log and bitmaps."""
    log = shared_log(eng, eng.evict_base()) if log is None else log
    want = naive(
        eng, log, to_numpy_delivery(d), agents, depth, lookback, code,
        eng.evict_base() if base is None else base, eng.total_messages())
    return want, log


def double_over(eng, d, agents, depth, lookback, **kw):
    """The numpy double run over ``eng``'s own log (a GPU engine's too)."""
    return Engine.context_to_device(
        eng, to_numpy_delivery(d), agents, depth, lookback, shared=True, **kw)


def assert_same_as_twin(g, c):
    """GPU result against the CPU twin's where no bitmap was recycled:
    counts, seqs and lengths whole; headers of defined slots without
    ``bitmap`` and ``bitmap_epoch`` (pool slot and handle on the GPU
    engine, index and 0 on the CPU engine), and their payload."""
    hg, hc = g.to_host(), c.to_host()
    assert (hg.total, hg.depth, hg.stride) == (hc.total, hc.depth, hc.stride)
    for name in ("counts", "seqs", "lengths"):
        np.testing.assert_array_equal(
            getattr(hg, name), getattr(hc, name), name)
    live = hc.seqs >= 0
    for name in REC_DTYPE.names:
        if name not in ("bitmap", "bitmap_epoch"):
            np.testing.assert_array_equal(
                hg.headers[name][live], hc.headers[name][live], name)
    np.testing.assert_array_equal(hg.payload[live], hc.payload[live])


# ---------------------------------------------------------------- traffic


def bits_of(eng, agents):
    b = np.zeros(eng.cfg.max_agents, dtype=bool)
    b[list(agents)] = True
    return b


def enqueue(engines, recs, buf, bitmaps=None):
    """The same batch on every engine; row i of ``bitmaps`` ({row: agents})
    gets a visibility bitmap with those agents' bits, allocated on each
    engine in row order."""
    seqs = None
    for e in engines:
        r = recs.copy()
        for i in sorted(bitmaps or {}):
            r["bitmap"][i] = e.alloc_bitmap(bits_of(e, bitmaps[i]))
        seqs = e.enqueue_batch(r, buf)
    return seqs


# label -> (sender, receiver, vis_mode, bitmap agents | None, must appear,
#           the visible message it is otherwise identical to | None)
# All on the dense 0 <-> 1 and 2 <-> 3 dialogues; agent 7 sends nothing
# else, so it is a third party to every row, and 100 is nobody. A
# broadcast also reaches its author's own inbox, and in that row (a == s)
# the author's bit is the one tested: the hidden broadcasts therefore set
# nobody's bit here, and the tile-edge and bit-edge tests set the author's.
CATEGORIES = {
    "1 plain bcast from 0": (0, BROADCAST, VIS_ALL, None, True, None),
    "1 plain bcast from 1": (1, BROADCAST, VIS_ALL, None, True, None),
    "2 bitmap bcast from 0, 1 set": (0, BROADCAST, VIS_BITMAP, (1, 100), True, None),
    "2 bitmap bcast from 0, 1 clear": (
        0, BROADCAST, VIS_BITMAP, (100,), False, "2 bitmap bcast from 0, 1 set"),
    "2 bitmap bcast from 1, 0 set": (1, BROADCAST, VIS_BITMAP, (0, 100), True, None),
    "2 bitmap bcast from 1, 0 clear": (
        1, BROADCAST, VIS_BITMAP, (100,), False, "2 bitmap bcast from 1, 0 set"),
    "3 author's own bit clear": (3, BROADCAST, VIS_BITMAP, (2, 100), True, None),
    "4 group, 3 a member": (2, BROADCAST, VIS_GROUP, (3, 6), True, None),
    "4 group, 3 not a member": (
        2, BROADCAST, VIS_GROUP, (100,), False, "4 group, 3 a member"),
    "5 bitmap p2p, receiver set": (0, 1, VIS_BITMAP, (1,), True, None),
    "5 bitmap p2p, receiver clear": (
        0, 1, VIS_BITMAP, (0,), False, "5 bitmap p2p, receiver set"),
    "6 restricted p2p, no bitmap": (1, 0, VIS_BITMAP, None, True, None),
    "7 third party's bcast": (
        7, BROADCAST, VIS_BITMAP, (0, 1, 2, 3), False,
        "2 bitmap bcast from 0, 1 set"),
    "8 deleted bcast": (0, BROADCAST, VIS_ALL, None, False, "1 plain bcast from 0"),
    "8 failed bcast": (0, BROADCAST, VIS_ALL, None, False, "1 plain bcast from 0"),
    "9 to oneself, own bit set": (2, 2, VIS_BITMAP, (2,), True, None),
    "9 to oneself, own bit clear": (
        2, 2, VIS_BITMAP, (3,), False, "9 to oneself, own bit set"),
}


def shared_mix(engines, n=200, seed=11):
    """Fixed-seed traffic among 8 agents (7 sends nothing of its own):
    random p2p, the dense 0 <-> 1 and 2 <-> 3 dialogues, two messages of
    2 to itself, and one message of every CATEGORIES entry in the first
    half, so that later rows of its dialogue have it in their window.
    Returns {label: seq}."""
    rng = np.random.default_rng(seed)
    register(engines, N_AGENTS)
    snd = rng.integers(0, N_AGENTS - 1, n)
    # never to oneself: the rows with a == s are the ones placed below
    rcv = (snd + rng.integers(1, N_AGENTS - 1, n)) % (N_AGENTS - 1)
    for i in range(0, n, 3):
        snd[i], rcv[i] = (0, 1) if (i // 3) % 2 else (1, 0)
    for i in range(1, n, 5):
        snd[i], rcv[i] = (2, 3) if (i // 5) % 2 else (3, 2)
    for i in (140, 185):  # rows whose polled agent is their sender
        snd[i], rcv[i] = 2, 2
    recs, buf = batch(snd, rcv, rng, priority=rng.integers(0, 4, n))
    at, bitmaps = {}, {}
    free = [i for i in range(4, n // 2) if i % 3 and i % 5 != 1]
    for k, (label, spec) in enumerate(CATEGORIES.items()):
        i = free[2 * k]  # on neither dialogue's stride
        s, r, vis, agents, _, _ = spec
        recs["sender"][i], recs["receiver"][i] = s, r
        recs["vis_mode"][i] = vis
        if agents is not None:
            bitmaps[i] = agents
        at[label] = i
    seqs = enqueue(engines, recs, buf, bitmaps)
    base = int(seqs[0])
    at = {label: base + i for label, i in at.items()}
    for e in engines:
        assert e.delete(at["8 deleted bcast"])
        e.set_status(at["8 failed bcast"], ST_FAILED)
    return at


def mix_delivery(engines, **kw):
    at = shared_mix(engines)
    ds = [e.receive_to_device(POLLED, 200, **kw) for e in engines]
    assert all(d.total == ds[0].total and d.total > 80 for d in ds)
    return at, ds


def plain_expect(eng, d, depth, lookback, code=None):
    """The rule of shared=False: test_device_context's naive loop."""
    log = host_log(eng)
    return naive_plain(
        log, to_numpy_delivery(d), POLLED, depth, lookback, code,
        eng.evict_base(), eng.total_messages(), eng.cfg.max_agents), log


# ---------------------------------------------------------------- CPU


@pytest.mark.parametrize("depth", [1, 3, 8, 64])
@pytest.mark.parametrize("lookback", [40, 1000])
def test_double_matches_naive_loop(depth, lookback):
    eng = cpu_engine()
    _, (d,) = mix_delivery([eng])
    ctx = eng.context_to_device(d, POLLED, depth, lookback, shared=True)
    assert (ctx.depth, ctx.stride, ctx.total) == (depth, 512, d.total)
    want, log = expect(eng, d, POLLED, depth, lookback)
    assert_context(ctx, want, log)
    assert any(len(m) == min(depth, 8) for m in want)


def test_every_category_is_exercised():
    """Each category that must appear makes some row's context differ
    between shared=True and shared=False; each that must not is absent
    from every row while the visible message it is otherwise identical to
    is present. Computed from the naive loops, then held against the
    double."""
    eng = cpu_engine()
    at, (d,) = mix_delivery([eng])
    want, log = expect(eng, d, POLLED, 64, 1000)
    plain, _ = plain_expect(eng, d, 64, 1000)
    assert_context(
        eng.context_to_device(d, POLLED, 64, 1000, shared=True), want, log)
    assert_context(
        eng.context_to_device(d, POLLED, 64, 1000, shared=False), plain, log)
    shown = {q for m in want for q in m}
    shown_plain = {q for m in plain for q in m}
    assert shown_plain < shown
    for label, (s, r, vis, agents, appears, twin) in CATEGORIES.items():
        q = at[label]
        i = q - log.lo
        assert (log.sender[i], log.receiver[i], log.vis[i]) == (s, r, vis)
        assert (log.bitmap[i] == NO_BITMAP) == (agents is None), label
        assert q not in shown_plain, label
        if appears:
            rows = [k for k, m in enumerate(want) if q in m]
            assert rows and all(q not in plain[k] for k in rows), label
        else:
            assert q not in shown, label
            assert CATEGORIES[twin][4] and at[twin] in shown, label
    # the rows that see a party's broadcast are rows of both directions
    hdr = d.headers.view(REC_DTYPE).reshape(-1)
    q = at["2 bitmap bcast from 0, 1 set"]
    pairs = {(int(POLLED[d.agent_row[k]]), int(hdr["sender"][k]))
             for k, m in enumerate(want) if q in m}
    assert pairs == {(1, 0), (0, 1)}
    # a row whose polled agent is its sender
    q = at["9 to oneself, own bit set"]
    assert {(int(POLLED[d.agent_row[k]]), int(hdr["sender"][k]))
            for k, m in enumerate(want) if q in m} == {(2, 2)}


def test_type_code_filter():
    eng = cpu_engine()
    _, (d,) = mix_delivery([eng])
    seen = set()
    for code in (0, 1, 2, 6):
        ctx = eng.context_to_device(
            d, POLLED, 8, 1000, type_code=code, shared=True)
        want, log = expect(eng, d, POLLED, 8, 1000, code)
        assert_context(ctx, want, log)
        h = ctx.to_host()
        live = h.seqs >= 0
        assert (h.headers["type"][live] == code).all()
        assert live.any() == (code != 6)
        seen |= set(h.headers["vis_mode"][live].tolist())
    assert seen == {VIS_ALL, VIS_BITMAP, VIS_GROUP}


@pytest.mark.parametrize("depth,lookback", [(3, 40), (64, 1000)])
def test_default_is_the_old_rule(depth, lookback):
    """shared=False, and no ``shared`` at all, on this mix: the present
    predicate, whole arrays."""
    eng = cpu_engine()
    _, (d,) = mix_delivery([eng])
    plain, log = plain_expect(eng, d, depth, lookback)
    off = eng.context_to_device(d, POLLED, depth, lookback, shared=False)
    assert_context(off, plain, log)
    assert_same_context(off, eng.context_to_device(d, POLLED, depth, lookback))
    h = off.to_host()
    live = h.seqs >= 0
    assert (h.headers["vis_mode"][live] == VIS_ALL).all()
    assert (h.headers["receiver"][live] != BROADCAST).all()


def test_tampered_inputs_are_values():
    eng = cpu_engine()
    _, (d,) = mix_delivery([eng])
    d = to_numpy_delivery(d)
    rows = tamper(d, eng.total_messages(), len(POLLED), eng.cfg.max_agents)
    # the delivered rows' own bitmap fields are never consulted
    hdr = d.headers.view(REC_DTYPE).reshape(-1)
    hdr["bitmap"][6:] = 3
    hdr["bitmap_epoch"][6:] = 12345
    hdr["vis_mode"][6:] = VIS_BITMAP
    ctx = eng.context_to_device(d, POLLED, 8, 1000, shared=True)
    want, log = expect(eng, d, POLLED, 8, 1000)
    assert_context(ctx, want, log)
    assert [len(want[r]) for r in rows[:1] + rows[2:]] == [0] * 5
    assert len(want[1]) == 8  # a seq above the log is clamped to its end


def test_read_only_cpu():
    eng, other = cpu_engine(), cpu_engine()
    assert_read_only(eng, other)


def assert_read_only(eng, other):
    """As in test_device_context, with shared=True: nothing observable
    moves, and the next poll delivers what it would have."""
    shared_mix([eng, other])
    d, d_other = (e.receive_to_device(POLLED, 10) for e in (eng, other))
    eng.backend_add_load(1, 7)
    before = snapshot(eng)
    ctx = eng.context_to_device(d, POLLED, 8, 1000, shared=True)
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


def refusals(eng, d):
    """Every refused call raises before anything is gathered: the queue
    and a reused ``out`` are as they were."""
    good = eng.context_to_device(d, POLLED, 8, 100, shared=True)
    keep = good.to_host()
    before = snapshot(eng)
    bad = [
        dict(shared=1), dict(shared=0), dict(shared="yes"),
        dict(shared=None), dict(shared=np.int32(1)),
        dict(depth=0, shared=True), dict(depth=65, shared=True),
        dict(lookback=0, shared=True), dict(lookback=2 ** 31, shared=True),
        dict(type_code=256, shared=True),
        dict(agent_idxs=POLLED[:3], shared=True),
    ]
    base = dict(agent_idxs=POLLED, depth=8, lookback=100, out=good)
    for kw in bad:
        with pytest.raises(ValueError):
            eng.context_to_device(d, **{**base, **kw})
    with pytest.raises(TypeError):  # keyword-only
        eng.context_to_device(d, POLLED, 8, 100, None, 0, None, 0, True)
    after = snapshot(eng)
    for k in before[0]:
        np.testing.assert_array_equal(before[0][k], after[0][k], k)
    np.testing.assert_array_equal(before[1], after[1])
    assert_same_context(good, keep)


def test_refusals_cpu():
    eng = cpu_engine()
    _, (d,) = mix_delivery([eng])
    refusals(eng, d)


def facade_shared(db):
    """broadcast_message, send_to_group_fast and send_message(visible_to=)
    traffic: context_device(shared=True) shows each message to the agents
    allowed and to nobody else, messages_from_context decodes them, and
    shared=False shows none."""
    for a in ("ann", "bob", "cy", "dee"):
        db.register_agent(a)
    db.add_agent_group("team", ["ann", "bob", "cy"])
    db.send_message("ann", "p2p", receiver_id="bob")
    db.broadcast_message("ann", "to all but dee", exclude_agents=["dee"])
    db.send_to_group_fast("team", "ann", {"group": 1},
                          message_type=MessageType.COMMAND)
    db.send_message("ann", "for cy only", visible_to=["cy"])
    db.send_message("ann", "for bob and dee", visible_to=["bob", "dee"])
    db.send_message("ann", "whisper", receiver_id="bob", visible_to=["bob"])
    db.send_message("ann", "lost", receiver_id="bob", visible_to=["cy"])
    db.broadcast_message("bob", "bob to all")
    db.broadcast_message("cy", "a third party")
    everyone = ["bob", "cy", "dee", "ann"]
    db.receive_device(everyone)  # drained: the next poll has triggers only
    for who in ("bob", "cy", "dee"):
        db.send_message("ann", "trigger", receiver_id=who)
    db.send_message("bob", "trigger", receiver_id="ann")
    d = db.receive_device(everyone)
    assert d.counts.tolist() == [1, 1, 1, 1]
    ctx = db.context_device(d, everyone, shared=True)
    want = {
        "bob": ["p2p", "to all but dee", {"group": 1}, "for bob and dee",
                "whisper", "bob to all"],
        # what cy itself broadcast, ann may see: it is part of the exchange
        "cy": ["to all but dee", {"group": 1}, "for cy only",
               "a third party"],
        "dee": ["for bob and dee"],
        # ann's row was sent by bob: the same exchange from the other side
        "ann": ["p2p", "to all but dee", {"group": 1}, "for bob and dee",
                "whisper", "bob to all", "trigger"],
    }
    for row, who in enumerate(everyone):
        got = db.messages_from_context(ctx, row)
        assert [m.content for m in got] == want[who], who
        for m in got:
            assert m.sender_id in (who, "bob" if who == "ann" else "ann")
    by_text = {m.content: m for m in db.messages_from_context(ctx, 0)
               if isinstance(m.content, str)}
    assert by_text["to all but dee"].visible_to == ["bob", "cy"]
    assert by_text["to all but dee"].receiver_id is None
    assert by_text["for bob and dee"].visible_to == ["bob", "dee"]
    assert by_text["whisper"].visible_to == ["bob"]
    assert by_text["p2p"].visible_to == []
    group = db.messages_from_context(ctx, 0)[2]
    assert group.visible_to == ["bob", "cy"]
    assert group.type == MessageType.COMMAND
    assert group.metadata == {"group": "team"}
    only = db.context_device(d, everyone, shared=True,
                             message_type=MessageType.COMMAND)
    assert [m.content for m in db.messages_from_context(only, 1)] == [
        {"group": 1}]
    for off in (db.context_device(d, everyone, shared=False),
                db.context_device(d, everyone)):
        assert [[m.content for m in db.messages_from_context(off, row)]
                for row in range(4)] == [["p2p"], [], [], ["p2p", "trigger"]]
    again = db.context_device(d, everyone, shared=True, out=ctx)
    assert again.seqs is ctx.seqs
    with pytest.raises(ValueError):
        db.context_device(d, everyone, shared="yes")


def test_facade_shared_cpu(tmp_db):
    facade_shared(tmp_db)


# ---------------------------------------------------------------- GPU


@pytest.mark.gpu
@pytest.mark.parametrize("group", [G, G_WIDE])
def test_gpu_parity_on_the_mix(group):
    import torch  # noqa: F401  (before GpuEngine: torch's HIP runtime first)

    gpu, cpu = gpu_and_twin()
    try:
        at, (dg, dc) = mix_delivery([gpu, cpu])
        np.testing.assert_array_equal(dg.seqs[:dg.total].cpu().numpy(),
                                      dc.seqs[:dc.total])
        for depth in (1, 8, 64):
            for lookback in (40, 1000):
                g = gpu.context_to_device(dg, POLLED, depth, lookback,
                                          group=group, shared=True)
                for t in (g.counts, g.seqs, g.lengths, g.headers, g.payload):
                    assert t.is_cuda
                assert_same_context(
                    g, double_over(gpu, dg, POLLED, depth, lookback))
                assert_same_as_twin(g, cpu.context_to_device(
                    dc, POLLED, depth, lookback, shared=True))
        # the naive loop over the GPU engine's own log and pool
        g = gpu.context_to_device(dg, POLLED, 64, 1000, group=group,
                                  shared=True)
        want, log = expect(gpu, dg, POLLED, 64, 1000)
        assert_context(g, want, log)
        shown = set(g.to_host().seqs.ravel().tolist())
        for label, spec in CATEGORIES.items():
            assert (at[label] in shown) == spec[4], label
        g = gpu.context_to_device(dg, POLLED, 8, 1000, type_code=1,
                                  max_payload=20, group=group, shared=True)
        assert g.stride == 32
        assert_same_context(g, double_over(
            gpu, dg, POLLED, 8, 1000, type_code=1, max_payload=20))
        # shared=False is the instantiation that was there
        off = gpu.context_to_device(dg, POLLED, 64, 1000, group=group,
                                    shared=False)
        assert_same_context(off, cpu.context_to_device(dc, POLLED, 64, 1000))
        assert_same_context(off, gpu.context_to_device(
            dg, POLLED, 64, 1000, group=group))
    finally:
        gpu.close()


EDGE_AGENTS = (0, 63, 64, 127, 128, 255)  # first and last bit of each word


@pytest.mark.gpu
@pytest.mark.parametrize("group", [G, G_WIDE])
def test_gpu_bitmap_word_and_bit_edges(group):
    """Both parties drawn from the agents at the word edges of a 256-bit
    bitmap; every bitmap sets exactly one of those bits, or all but one. A
    wrong word index or shift shows here and nowhere else."""
    import torch  # noqa: F401

    gpu, cpu = gpu_and_twin()
    try:
        for e in (gpu, cpu):
            for a in EDGE_AGENTS:
                e.register_agent(a)
        rng = np.random.default_rng(3)
        snd, rcv, bitmaps, one, allbut = [], [], {}, {}, {}
        everyone = set(range(256))
        for x in EDGE_AGENTS:
            for y in EDGE_AGENTS:
                one[x, y] = len(snd)
                bitmaps[len(snd)] = (y,)
                snd.append(x), rcv.append(BROADCAST)
                allbut[x, y] = len(snd)
                bitmaps[len(snd)] = tuple(everyone - {y})
                snd.append(x), rcv.append(BROADCAST)
        recs, buf = batch(snd, rcv, rng)
        recs["vis_mode"] = VIS_BITMAP
        enqueue([gpu, cpu], recs, buf, bitmaps)
        agents = np.array(EDGE_AGENTS, dtype=np.uint32)
        for e in (gpu, cpu):
            e.receive_to_device(agents, 4096)
        # one trigger per ordered pair, itself included
        pairs = [(x, y) for x in EDGE_AGENTS for y in EDGE_AGENTS]
        enqueue([gpu, cpu], *batch([x for x, _ in pairs],
                                   [y for _, y in pairs], rng))
        dg = gpu.receive_to_device(agents, 16)
        dc = cpu.receive_to_device(agents, 16)
        assert dg.total == dc.total == len(pairs)
        g = gpu.context_to_device(dg, agents, 64, 1000, group=group,
                                  shared=True)
        assert_same_context(g, double_over(gpu, dg, agents, 64, 1000))
        assert_same_as_twin(
            g, cpu.context_to_device(dc, agents, 64, 1000, shared=True))
        want, log = expect(gpu, dg, agents, 64, 1000)
        assert_context(g, want, log)
        h = dg.to_host()
        for r in range(h.total):
            y = int(agents[h.agent_row[r]])  # the polled agent
            x = int(h.headers["sender"][r])
            got = set(want[r])
            # what x wrote, judged by y's bit; what y wrote, by x's bit
            for author, reader in ((x, y), (y, x)):
                for z in EDGE_AGENTS:
                    assert (one[author, z] in got) == (z == reader)
                    assert (allbut[author, z] in got) == (z != reader)
            assert len(got) == (12 if x != y else 6) + \
                sum(1 for q in got if q >= len(snd))
    finally:
        gpu.close()


@pytest.mark.gpu
def test_gpu_recycled_pool_slot():
    """num_bitmaps 4: message A's handle is the first, four more
    allocations wrap onto its slot, message B uses the newest handle of
    that slot. A is in no context whatever the new bitmap says, B is
    judged by its own bits. The CPU twin never recycles and is not
    consulted."""
    import torch  # noqa: F401

    from swarmdb_amd.runtime.gpu_engine import GpuEngine

    gpu = GpuEngine(small_cfg(num_bitmaps=4))
    try:
        register([gpu], 2)
        rng = np.random.default_rng(4)
        agent1 = np.array([1], dtype=np.uint32)

        def bcast(handle):
            recs, buf = batch([0], [BROADCAST], rng)
            recs["vis_mode"] = VIS_BITMAP
            recs["bitmap"] = handle
            return int(gpu.enqueue_batch(recs, buf)[0])

        h_a = gpu.alloc_bitmap(bits_of(gpu, (1,)))
        a = bcast(h_a)
        gpu.enqueue_batch(*batch([0], [1], rng))
        d0 = gpu.receive_to_device(agent1, 16)
        assert d0.total == 2  # A was delivered while its bitmap was live
        before = gpu.context_to_device(d0, agent1, 8, 100, shared=True)
        assert before.to_host().seqs[1].tolist()[:1] == [a]

        h_c = gpu.alloc_bitmap(bits_of(gpu, (1,)))   # slot 1: stays live
        h_d = gpu.alloc_bitmap(bits_of(gpu, (0,)))   # slot 2: 1's bit clear
        gpu.alloc_bitmap(bits_of(gpu, (0, 1)))       # slot 3
        h_b = gpu.alloc_bitmap(bits_of(gpu, (1, 5)))  # slot 0 again
        assert (h_a % 4, h_b % 4, h_b - h_a) == (0, 0, 4)
        assert gpu.read_bitmap(0, h_a) is None
        assert gpu.read_bitmap(0, h_b)[[0, 1, 5]].tolist() == [False, True, True]
        c, dd, b = bcast(h_c), bcast(h_d), bcast(h_b)
        h_e = gpu.alloc_bitmap(bits_of(gpu, (0,)))   # slot 1 again
        assert h_e % 4 == h_c % 4
        gpu.receive_to_device(agent1, 16)
        trigger = int(gpu.enqueue_batch(*batch([0], [1], rng))[0])
        d = gpu.receive_to_device(agent1, 16)
        assert d.total == 1 and int(d.seqs[0]) == trigger
        for group in (G, G_WIDE):
            g = gpu.context_to_device(d, agent1, 8, 100, group=group,
                                      shared=True)
            h = g.to_host()
            # A and C recycled, D hidden by its own bits, B visible
            assert h.counts.tolist() == [2]
            assert h.seqs[0, :2].tolist() == [a + 1, b]
            assert h.headers["bitmap"][0, 1] == 0
            assert h.headers["bitmap_epoch"][0, 1] == h_b
            assert_same_context(g, double_over(gpu, d, agent1, 8, 100))
            want, log = expect(gpu, d, agent1, 8, 100)
            assert want == [[a + 1, b]]
            assert_context(g, want, log)
        assert not {a, c, dd} & set(want[0])
    finally:
        gpu.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flip", [0, 1])
def test_gpu_tile_and_ballot_edges(flip):
    """Restricted messages at distances 63, 64, 65, 255, 256, 257, 511 and
    512 below a row's hi, visible and hidden alternating (``flip`` swaps
    them); each depth makes another of them the last one taken."""
    import torch  # noqa: F401

    gpu, cpu = gpu_and_twin()
    try:
        register([gpu, cpu])
        hi, lookback = 700, 600
        dist = [63, 64, 65, 255, 256, 257, 511, 512]
        snd = np.full(hi, 4)
        rcv = np.full(hi, 5)
        bitmaps, visible = {}, []
        for k, dd in enumerate(dist):
            q = hi - dd
            snd[q], rcv[q] = k % 2, BROADCAST  # from s and from a in turn
            other = 1 - k % 2
            if (k + flip) % 2:
                bitmaps[q] = (other, 3)
                visible.append(q)
            else:
                bitmaps[q] = (k % 2, 3)  # the author's bit, not the other's
        rng = np.random.default_rng(flip)
        recs, buf = batch(snd, rcv, rng)
        recs["vis_mode"][sorted(bitmaps)] = VIS_BITMAP
        enqueue([gpu, cpu], recs, buf, bitmaps)
        agents = np.array([1], dtype=np.uint32)
        for e in (gpu, cpu):
            e.receive_to_device(agents, 4096)
        enqueue([gpu, cpu], *batch([0], [1], rng))
        dg = gpu.receive_to_device(agents, 4)
        dc = cpu.receive_to_device(agents, 4)
        assert dc.total == 1 and dc.seqs[0] == hi
        assert len(visible) == 4
        for group in (G, G_WIDE):
            for depth in (1, 2, 3, 4, 8):
                g = gpu.context_to_device(dg, agents, depth, lookback,
                                          group=group, shared=True)
                assert_same_context(
                    g, double_over(gpu, dg, agents, depth, lookback))
                assert_same_as_twin(g, cpu.context_to_device(
                    dc, agents, depth, lookback, shared=True))
                keep = sorted(visible)[-depth:]
                got = g.to_host()
                assert got.counts[0] == len(keep)
                assert got.seqs[0, :len(keep)].tolist() == keep
    finally:
        gpu.close()


@pytest.mark.gpu
def test_gpu_group_broadcast_without_bitmap():
    """A VIS_GROUP broadcast whose bitmap is NO_BITMAP is enqueued and
    fanned out to nobody: it is in no context. The CPU engine cannot
    enqueue this record, so the double runs over the GPU log only."""
    import torch  # noqa: F401

    from swarmdb_amd.runtime.gpu_engine import GpuEngine

    gpu = GpuEngine(small_cfg())
    try:
        register([gpu], 2)
        rng = np.random.default_rng(6)
        recs, buf = batch([0, 0, 1, 0], [BROADCAST, BROADCAST, BROADCAST, 1],
                          rng)
        recs["vis_mode"][:3] = VIS_GROUP
        seqs = enqueue([gpu], recs, buf, {1: (1,), 2: (0,)})
        lone, member, back, trigger = (int(q) for q in seqs)
        agent1 = np.array([1], dtype=np.uint32)
        d = gpu.receive_to_device(agent1, 16)
        # only the member broadcast and the trigger reached the inbox
        assert d.seqs[:d.total].tolist() == [member, trigger]
        for group in (G, G_WIDE):
            g = gpu.context_to_device(d, agent1, 8, 100, group=group,
                                      shared=True)
            assert_same_context(g, double_over(gpu, d, agent1, 8, 100))
            h = g.to_host()
            assert h.counts.tolist() == [0, 2]
            assert h.seqs[1, :2].tolist() == [member, back]
            assert lone not in h.seqs
        want, log = expect(gpu, d, agent1, 8, 100)
        assert want == [[], [member, back]]
        assert log.bitmap[lone] == NO_BITMAP and log.vis[lone] == VIS_GROUP
    finally:
        gpu.close()


@pytest.mark.gpu
def test_gpu_rows_of_one_block_get_their_own_verdict():
    """Priority-ordered delivery, sixteen rows per workgroup: rows with
    different (a, s) and different windows test the same restricted
    entries of one tile, each with its own bit."""
    import torch  # noqa: F401

    gpu, cpu = gpu_and_twin()
    try:
        at, (dg, dc) = mix_delivery([gpu, cpu], priority_order=True)
        np.testing.assert_array_equal(dg.seqs[:dg.total].cpu().numpy(),
                                      dc.seqs[:dc.total])
        h = dc.to_host()
        pair = list(zip(POLLED[h.agent_row].tolist(),
                        h.headers["sender"].tolist()))
        blocks = range(0, h.total, G_WIDE)
        assert sum(len(set(pair[k:k + G_WIDE])) >= 4 for k in blocks) >= 4
        assert sum((np.diff(h.seqs[k:k + G_WIDE]) < 0).any()
                   for k in blocks) >= 4
        for depth, lookback in ((4, 50), (8, 1000), (64, 120)):
            g = gpu.context_to_device(dg, POLLED, depth, lookback,
                                      group=G_WIDE, shared=True)
            assert_same_context(
                g, double_over(gpu, dg, POLLED, depth, lookback))
            assert_same_as_twin(g, cpu.context_to_device(
                dc, POLLED, depth, lookback, shared=True))
        # one restricted entry, two verdicts within one workgroup
        g = gpu.context_to_device(dg, POLLED, 64, 1000, group=G_WIDE,
                                  shared=True).to_host()
        q = at["4 group, 3 a member"]
        took = (g.seqs == q).any(axis=1)
        later = h.seqs > q
        assert any(took[k:k + G_WIDE].any()
                   and (later[k:k + G_WIDE] & ~took[k:k + G_WIDE]).any()
                   for k in blocks)
    finally:
        gpu.close()


@pytest.mark.gpu
def test_gpu_eviction():
    """num_slots 256 and 700 messages with restricted broadcasts among
    them: the ring wrapped twice. Against the double over the GPU log,
    and against the naive loop over the twin's log (which retains
    everything, and whose bitmap indices equal the GPU engine's handles)
    with lo clamped to the GPU engine's evict_base()."""
    import torch  # noqa: F401

    gpu, cpu = gpu_and_twin(num_slots=256)
    try:
        register([gpu, cpu], 4)
        rng = np.random.default_rng(5)
        for _ in range(7):
            snd = rng.integers(0, 3, 100)
            rcv = rng.integers(0, 3, 100)
            recs, buf = batch(snd, rcv, rng)
            rows = rng.choice(100, 20, replace=False)
            recs["receiver"][rows] = BROADCAST
            recs["vis_mode"][rows] = VIS_BITMAP
            bitmaps = {int(i): tuple(rng.choice(4, 2, replace=False).tolist())
                       for i in rows}
            enqueue([gpu, cpu], recs, buf, bitmaps)
        base = gpu.evict_base()
        assert base == 700 - 256 and gpu.total_messages() == 700
        agents = np.array([0, 1, 2], dtype=np.uint32)
        dg = gpu.receive_to_device(agents, 300)
        assert dg.total > 100
        for group in (G, G_WIDE):
            g = gpu.context_to_device(dg, agents, 8, 1000, group=group,
                                      shared=True)
            assert_same_context(g, double_over(gpu, dg, agents, 8, 1000))
            log = shared_log(cpu)
            want = naive(cpu, log, to_numpy_delivery(dg), agents, 8, 1000,
                         None, base, 700)
            h = g.to_host()
            assert [m + [-1] * (8 - len(m)) for m in want] == h.seqs.tolist()
            assert ((h.seqs >= base) | (h.seqs == -1)).all()
            live = h.seqs >= 0
            assert (h.headers["vis_mode"][live] == VIS_BITMAP).any()
            assert any(len(m) < 8 for m in want)
            assert any(len(m) == 8 for m in want)
    finally:
        gpu.close()


@pytest.mark.gpu
def test_gpu_out_reuse_tampered_rows_and_refusals():
    import torch

    gpu, cpu = gpu_and_twin()
    try:
        _, (dg, dc) = mix_delivery([gpu, cpu])
        refusals(gpu, dg)
        with pytest.raises(ValueError):
            gpu.context_to_device(dg, POLLED, 8, 100, group=8, shared=True)
        # one set of buffers, the two rules in turn
        on = gpu.context_to_device(dg, POLLED, 8, 1000, shared=True)
        want_on = double_over(gpu, dg, POLLED, 8, 1000)
        want_off = cpu.context_to_device(dc, POLLED, 8, 1000)
        assert_same_context(on, want_on)
        off = gpu.context_to_device(dg, POLLED, 8, 1000, shared=False, out=on)
        assert off.seqs is on.seqs
        assert_same_context(off, want_off)
        assert not np.array_equal(want_on.to_host().seqs,
                                  want_off.to_host().seqs)
        again = gpu.context_to_device(dg, POLLED, 8, 1000, shared=True,
                                      out=off)
        assert again.payload is on.payload
        assert_same_context(again, want_on)

        dn = to_numpy_delivery(dc)
        rows = tamper(dn, cpu.total_messages(), len(POLLED),
                      cpu.cfg.max_agents)
        hdr = dn.headers.view(REC_DTYPE).reshape(-1)
        hdr["bitmap"][6:] = 3  # the rows' own bitmap fields are not used
        hdr["bitmap_epoch"][6:] = 12345
        dev = dg.seqs.device
        dg.seqs[:dg.total] = torch.from_numpy(dn.seqs).to(dev)
        dg.agent_row[:dg.total] = torch.from_numpy(dn.agent_row).to(dev)
        dg.headers[:dg.total] = torch.from_numpy(dn.headers).to(dev)
        g = gpu.context_to_device(dg, POLLED, 8, 1000, shared=True)
        assert_same_context(g, double_over(gpu, dg, POLLED, 8, 1000))
        assert_same_as_twin(
            g, cpu.context_to_device(dn, POLLED, 8, 1000, shared=True))
        assert g.to_host().counts[rows].tolist() == [0, 8, 0, 0, 0, 0]
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
def test_facade_shared_gpu(tmp_path):
    import torch  # noqa: F401

    from swarmdb_amd.runtime.gpu_engine import GpuEngine

    cfg = small_cfg(save_dir=str(tmp_path / "gpu"))
    db = SwarmsDB(config=cfg, engine=GpuEngine(cfg))
    try:
        facade_shared(db)
    finally:
        db.close()
