"""Device-resident LLM dispatch: dispatch_delivery / release_dispatch.

The CPU engine's implementation is the plain-numpy double; it is checked
against an independent naive loop written here and against
dispatch_batch, and the HIP kernels (k_dispatch_rows, k_dispatch_scatter,
k_release_loads) are checked against it on a twin engine fed the same
inputs. Every comparison is integer-exact.

The file holds CPU and GPU tests, so GPU tests carry the marker one by
one.
"""

import numpy as np
import pytest

from swarmdb_amd import DeviceDispatch, MessageType, QueueConfig, SwarmsDB
from swarmdb_amd.runtime.cpu_engine import CpuEngine
from swarmdb_amd.runtime.engine import NO_BITMAP, REC_DTYPE, VIS_ALL

TOKENS = np.array([0, 1, 7, 1000, 2 ** 32 - 1], dtype=np.uint64)
TOTALS = [0, 1, 63, 64, 65, 129, 257]  # 64-row chunks, 256-thread blocks


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


def split3(total):
    """Uneven per-agent counts of three polled agents; from 65 rows on the
    middle agent's rows straddle the first 64-row chunk boundary."""
    a, b = total * 2 // 5, total // 4
    return [a, b, total - a - b]


def fill(engines, counts, seed=0):
    """Enqueue counts[b] messages for agent b + 1 (sender 0) on every
    engine, with types 0..2 and token counts drawn from TOKENS by a
    fixed-seed generator. Returns (polled agents, types, tokens) in
    delivery row order."""
    rng = np.random.default_rng(seed)
    n = int(sum(counts))
    recv = np.repeat(np.arange(1, len(counts) + 1), counts)
    recs = np.zeros(n, dtype=REC_DTYPE)
    recs["sender"] = 0
    recs["receiver"] = recv
    recs["type"] = rng.integers(0, 3, n)
    recs["token_count"] = rng.choice(TOKENS, n).astype(np.uint32)
    if n >= 2:  # both extremes are always there
        recs["token_count"][0] = 2 ** 32 - 1
        recs["token_count"][n - 1] = 0
    recs["timestamp"] = 1.7e9 + np.arange(n)
    recs["vis_mode"] = VIS_ALL
    recs["bitmap"] = NO_BITMAP
    recs["payload_off"] = np.arange(n, dtype=np.uint64) * 16
    recs["payload_len"] = 16
    recs["content_len"] = 16
    buf = bytes(range(1, 17)) * n + b"\xee" * 16
    for e in engines:
        for a in range(len(counts) + 1):
            e.register_agent(a)
        if n:
            e.enqueue_batch(recs, buf)
    agents = np.arange(1, len(counts) + 1, dtype=np.uint32)
    return agents, recs["type"].astype(int), recs["token_count"].astype(int)


def deliver(eng, agents, counts):
    d = eng.receive_to_device(agents, max(max(counts), 1), max_payload=16)
    assert d.counts.tolist() == list(counts)
    return d


def preload(engines, loads):
    for e in engines:
        for k, v in enumerate(loads):
            if v:
                e.backend_add_load(k, int(v))


def naive(loads, nb, types, tokens, arow, weight, code, pinned):
    """The issue's loop, on Python ints and lists."""
    load = [int(x) for x in loads[:nb]]
    added, backend = [0] * nb, []
    for r in range(len(types)):
        if code is not None and types[r] != code:
            backend.append(-1)
            continue
        cost = 1 if weight == "requests" else max(int(tokens[r]), 1)
        b = int(arow[r])
        p = pinned[b] if pinned is not None and 0 <= b < len(pinned) else -1
        if p >= 0:
            k = p
        else:
            k = 0
            for i in range(1, nb):
                if load[i] < load[k]:
                    k = i
        load[k] += cost
        added[k] += cost
        backend.append(k)
    return backend, added, load


def assert_grouped(h):
    """order / offsets / counts against backend, on a host copy."""
    assert h.offsets[0] == 0 and h.offsets[h.n_backends] == h.m
    np.testing.assert_array_equal(h.counts, np.diff(h.offsets))
    for k in range(h.n_backends):
        np.testing.assert_array_equal(
            h.order[h.offsets[k]:h.offsets[k + 1]],
            np.flatnonzero(h.backend == k),
        )
    assert h.m == int((h.backend >= 0).sum())


def assert_same_dispatch(g, c):
    """GPU result against the CPU twin's, defined ranges only."""
    hg, hc = g.to_host(), c.to_host()
    assert (hg.total, hg.m, hg.n_backends) == (hc.total, hc.m, hc.n_backends)
    for name in ("backend", "order", "offsets", "added", "counts"):
        a, b = getattr(hg, name), getattr(hc, name)
        assert a.dtype == b.dtype, name
        np.testing.assert_array_equal(a, b, name)
    assert_grouped(hg)


# ---------------------------------------------------------------- CPU


@pytest.mark.parametrize("weight", ["requests", "tokens"])
def test_double_matches_naive_loop(weight):
    counts = [7, 0, 19, 4]
    pre = [3, -5, 0, 0, 2, 0]
    for code, pinned in ((None, None), (1, None), (None, [-1, 2, 5, -1]),
                         (2, [0, -1, -1, 4])):
        eng = cpu_engine()
        agents, types, tokens = fill([eng], counts)
        assert set(tokens.tolist()) == set(TOKENS.tolist())
        preload([eng], pre)
        d = deliver(eng, agents, counts)
        got = eng.dispatch_delivery(d, 6, weight, code, pinned)
        assert isinstance(got, DeviceDispatch) and not got.released
        backend, added, load = naive(
            pre, 6, types, tokens, d.agent_row[:d.total], weight, code, pinned)
        assert got.backend[:got.total].tolist() == backend
        assert got.added.tolist() == added
        assert eng.backend_loads()[:6].tolist() == load
        assert got.backend.dtype == got.order.dtype == np.int32
        assert got.offsets.dtype == np.int32 and got.added.dtype == np.int64
        assert got.counts.dtype == np.int64
        assert_grouped(got.to_host())


def test_requests_equals_dispatch_batch():
    counts = [30, 11, 40]
    eng, twin = cpu_engine(), cpu_engine()
    agents, _, _ = fill([eng], counts)
    preload([eng, twin], [4, 0, -5, 9, 0])
    d = deliver(eng, agents, counts)
    got = eng.dispatch_delivery(d, 5)
    want = twin.dispatch_batch(d.total, 5)
    np.testing.assert_array_equal(got.backend[:d.total], want.astype(np.int32))
    np.testing.assert_array_equal(eng.backend_loads(), twin.backend_loads())


def test_grouping_is_stable():
    counts = split3(129)
    eng = cpu_engine()
    agents, _, _ = fill([eng], counts)
    d = deliver(eng, agents, counts)
    got = eng.dispatch_delivery(d, 3, "tokens", pinned=[-1, 1, -1])
    h = got.to_host()
    assert_grouped(h)
    assert h.m == h.total == 129 and h.counts.sum() == 129
    for k in range(3):
        grp = h.order[h.offsets[k]:h.offsets[k + 1]]
        assert (np.diff(grp) > 0).all()


def test_type_filter_skips_rows():
    counts = [20, 25]
    eng = cpu_engine()
    agents, types, tokens = fill([eng], counts)
    d = deliver(eng, agents, counts)
    got = eng.dispatch_delivery(d, 4, "tokens", type_code=1)
    h = got.to_host()
    skipped = types != 1
    assert skipped.any() and (~skipped).any()
    assert (h.backend[skipped] == -1).all() and (h.backend[~skipped] >= 0).all()
    assert not np.isin(np.flatnonzero(skipped), h.order).any()
    assert h.m == int((~skipped).sum())
    assert h.added.sum() == int(np.maximum(tokens[~skipped], 1).sum())
    assert eng.backend_loads()[:4].tolist() == h.added.tolist()


def test_pinned_agents_keep_their_backend():
    counts = [10, 12, 8]
    eng = cpu_engine()
    agents, _, _ = fill([eng], counts)
    d = deliver(eng, agents, counts)
    got = eng.dispatch_delivery(d, 4, pinned=np.array([-1, 3, -1]))
    h = got.to_host()
    arow = d.agent_row[:d.total]
    assert (h.backend[arow == 1] == 3).all()
    assert h.counts[3] >= 12 and h.added[3] == h.counts[3]
    assert eng.backend_loads()[3] == h.added[3]
    # the pinned load is seen by the unpinned rows that follow
    # (10 rows round-robin, 12 pinned, then 8 that avoid the loaded one)
    assert (h.backend[arow == 2] != 3).all()
    assert h.counts.tolist() == [6, 5, 5, 14]


def test_release_restores_loads():
    counts = [9, 9]
    eng = cpu_engine()
    agents, _, _ = fill([eng], counts)
    preload([eng], [5, -5, 2 ** 40])
    before = eng.backend_loads()
    d = deliver(eng, agents, counts)
    got = eng.dispatch_delivery(d, 3, "tokens")
    assert (eng.backend_loads() != before).any()
    eng.release_dispatch(got)
    assert got.released
    np.testing.assert_array_equal(eng.backend_loads(), before)
    with pytest.raises(ValueError):
        eng.release_dispatch(got)
    np.testing.assert_array_equal(eng.backend_loads(), before)


def facade_round_trip(db):
    """receive_device -> dispatch_device -> complete_device; returns what
    the checks below look at."""
    for b in ("alpha", "beta", "gamma"):
        db.register_llm_backend(b)
    db.assign_llm_backend("bob", "gamma")
    for i in range(6):
        db.send_message("ann", f"to-bob-{i}", receiver_id="bob")
        db.send_message("ann", f"to-cy-{i}", receiver_id="cy",
                        message_type=MessageType.COMMAND)
    start = db.engine.backend_loads().copy()
    d = db.receive_device(["bob", "cy"])
    assert d.counts.tolist() == [6, 6]

    pinned = db.dispatch_device(d, ["bob", "cy"])
    assert pinned.backend_ids == ["alpha", "beta", "gamma"]
    hp = pinned.to_host()
    db.complete_device(pinned)
    after_pinned = db.engine.backend_loads().copy()

    db.set_llm_load_balancing(True)
    free = db.dispatch_device(d, ["bob", "cy"])
    hf = free.to_host()
    db.complete_device(free)

    only = db.dispatch_device(d, ["bob", "cy"], weight="tokens",
                              message_type=MessageType.COMMAND)
    ho = only.to_host()
    db.complete_device(only)
    with pytest.raises(ValueError):
        db.complete_device(only)
    np.testing.assert_array_equal(after_pinned, start)
    np.testing.assert_array_equal(db.engine.backend_loads(), start)

    # balancing off: bob's rows (0..5) are pinned to gamma
    assert hp.backend[:6].tolist() == [2] * 6
    assert hp.backend[6:].tolist() == [0, 1, 0, 1, 0, 1]
    # balancing on: nothing is pinned
    assert hf.backend.tolist() == [0, 1, 2] * 4
    assert ho.backend[:6].tolist() == [-1] * 6 and (ho.backend[6:] >= 0).all()
    assert ho.m == 6

    with pytest.raises(ValueError):
        db.dispatch_device(d, ["bob"])
    with pytest.raises(ValueError):
        db.dispatch_device(d, ["bob", "nobody"])
    with pytest.raises(ValueError):
        db.dispatch_device(d, ["bob", "cy"], weight="bytes")
    np.testing.assert_array_equal(db.engine.backend_loads(), start)


def test_facade_dispatch_cpu(tmp_db):
    d = tmp_db.receive_device(["ann"])
    with pytest.raises(RuntimeError):
        tmp_db.dispatch_device(d, ["ann"])
    facade_round_trip(tmp_db)


def refusals(eng, d):
    """Every refusal is a ValueError and leaves the loads alone."""
    preload([eng], [1, -5, 3])
    before = eng.backend_loads().copy()
    na = len(d.counts)
    bad = [
        dict(n_backends=0),
        dict(n_backends=65),
        dict(n_backends=eng.cfg.num_backends + 1),
        dict(n_backends=4, weight="bytes"),
        dict(n_backends=4, type_code=256),
        dict(n_backends=4, type_code=-1),
        dict(n_backends=4, pinned=[-1] * (na + 1)),
        dict(n_backends=4, pinned=[-1] * (na - 1)),
        dict(n_backends=4, pinned=[4] + [-1] * (na - 1)),
        dict(n_backends=4, pinned=[-2] + [-1] * (na - 1)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            eng.dispatch_delivery(d, **kw)
        np.testing.assert_array_equal(eng.backend_loads(), before, str(kw))
    return before


def test_refusals_cpu():
    import dataclasses

    counts = [5, 6]
    eng = cpu_engine(num_backends=16)
    agents, _, _ = fill([eng], counts)
    d = deliver(eng, agents, counts)
    before = refusals(eng, d)
    good = eng.dispatch_delivery(d, 4)
    eng.release_dispatch(good)
    wrong = [
        dataclasses.replace(d, agent_row=d.agent_row.astype(np.int64)),
        dataclasses.replace(d, headers=d.headers[:, :40]),
        dataclasses.replace(d, agent_row=d.agent_row.tolist()),
        dataclasses.replace(d, agent_row=d.agent_row[:3]),
    ]
    for w in wrong:
        with pytest.raises(ValueError):
            eng.dispatch_delivery(w, 4)
    with pytest.raises(ValueError):  # built for another n_backends
        eng.dispatch_delivery(d, 5, out=good)
    small = dataclasses.replace(good, order=good.order[:d.total - 1])
    with pytest.raises(ValueError):
        eng.dispatch_delivery(d, 4, out=small)
    np.testing.assert_array_equal(eng.backend_loads(), before)
    again = eng.dispatch_delivery(d, 4, out=good)
    assert again.backend is good.backend and not again.released


# ---------------------------------------------------------------- GPU


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [1, 2, 3, 8, 64])
def test_gpu_parity_shapes(nb):
    """Chunk (64 rows) and block (256 threads) boundaries x every
    reduction depth, both weights, with and without filter + pin, from
    loads that hold ties, a negative and a 2**40."""
    import torch  # noqa: F401  (before GpuEngine: torch's HIP runtime first)

    gpu, cpu = gpu_and_twin()
    try:
        pre = [0] * nb
        pre[0] = 2 ** 40
        if nb > 2:
            pre[2] = -5
        preload([gpu, cpu], pre)
        start = cpu.backend_loads().copy()
        np.testing.assert_array_equal(gpu.backend_loads(), start)
        for total in TOTALS:
            counts = split3(total)
            agents, types, _ = fill([gpu, cpu], counts, seed=total)
            dg, dc = deliver(gpu, agents, counts), deliver(cpu, agents, counts)
            assert dg.total == dc.total == total
            pin = [-1, nb - 1, -1]
            for weight in ("requests", "tokens"):
                for code, pinned in ((None, None), (1, pin)):
                    g = gpu.dispatch_delivery(dg, nb, weight, code, pinned)
                    c = cpu.dispatch_delivery(dc, nb, weight, code, pinned)
                    assert g.backend.is_cuda and g.order.is_cuda
                    assert g.offsets.is_cuda and g.added.is_cuda
                    assert isinstance(g.counts, np.ndarray)
                    assert_same_dispatch(g, c)
                    np.testing.assert_array_equal(
                        gpu.backend_loads(), cpu.backend_loads())
                    if code is not None and total >= 129:
                        skip = np.flatnonzero(types != code)
                        assert (skip < 64).any() and (skip >= 64).any()
                        hb = g.to_host().backend
                        assert (hb[skip] == -1).all()
                        arow = dc.agent_row[:total]
                        assert (hb[(arow == 1) & (types == code)]
                                == nb - 1).all()
                    gpu.release_dispatch(g)
                    cpu.release_dispatch(c)
                    np.testing.assert_array_equal(gpu.backend_loads(), start)
                    with pytest.raises(ValueError):
                        gpu.release_dispatch(g)
    finally:
        gpu.close()


@pytest.mark.gpu
def test_gpu_ties_and_dispatch_batch_identity():
    """All-equal loads go round-robin from index 0, and the plain
    request-weighted dispatch is dispatch_batch on the GPU engine itself."""
    import torch  # noqa: F401

    gpu, cpu = gpu_and_twin()
    try:
        counts = split3(257)
        agents, _, _ = fill([gpu], counts)
        d = deliver(gpu, agents, counts)
        for nb, pre in ((8, [0] * 8), (5, [7, -5, 2 ** 40, 7, 0]),
                        (64, [3] * 64)):
            preload([gpu], pre)
            start = gpu.backend_loads().copy()
            got = gpu.dispatch_delivery(d, nb)
            h = got.to_host()
            loads_after = gpu.backend_loads().copy()
            gpu.release_dispatch(got)
            np.testing.assert_array_equal(gpu.backend_loads(), start)
            want = gpu.dispatch_batch(257, nb)
            np.testing.assert_array_equal(h.backend, want.astype(np.int32))
            np.testing.assert_array_equal(gpu.backend_loads(), loads_after)
            if len(set(pre)) == 1:
                assert h.backend.tolist() == [r % nb for r in range(257)]
            # back to zero for the next case
            for k, v in enumerate(gpu.backend_loads()[:nb]):
                gpu.backend_add_load(k, -int(v))
    finally:
        gpu.close()


@pytest.mark.gpu
def test_gpu_tampered_agent_row_reads_as_unpinned():
    import torch

    gpu, cpu = gpu_and_twin()
    try:
        counts = split3(129)
        agents, _, _ = fill([gpu, cpu], counts)
        dg, dc = deliver(gpu, agents, counts), deliver(cpu, agents, counts)
        rows = [0, 5, 63, 64, 70, 128]
        vals = [-1, 10 ** 6, -1, 10 ** 6, -(2 ** 31), 2 ** 31 - 1]
        dg.agent_row[torch.tensor(rows, device=dg.agent_row.device)] = \
            torch.tensor(vals, dtype=torch.int32, device=dg.agent_row.device)
        dc.agent_row[rows] = vals
        pin = [2, 0, 1]
        g = gpu.dispatch_delivery(dg, 3, "tokens", None, pin)
        c = cpu.dispatch_delivery(dc, 3, "tokens", None, pin)
        assert_same_dispatch(g, c)
        np.testing.assert_array_equal(gpu.backend_loads(), cpu.backend_loads())
    finally:
        gpu.close()


@pytest.mark.gpu
def test_gpu_out_reuse():
    import dataclasses

    import torch  # noqa: F401

    gpu, cpu = gpu_and_twin()
    try:
        big, small = split3(257), split3(65)
        agents, _, _ = fill([gpu, cpu], big, seed=1)
        dg, dc = deliver(gpu, agents, big), deliver(cpu, agents, big)
        g = gpu.dispatch_delivery(dg, 8, "tokens")
        c = cpu.dispatch_delivery(dc, 8, "tokens")
        assert_same_dispatch(g, c)
        fill([gpu, cpu], small, seed=2)
        dg2, dc2 = deliver(gpu, agents, small), deliver(cpu, agents, small)
        g2 = gpu.dispatch_delivery(dg2, 8, "tokens", 1, out=g)
        c2 = cpu.dispatch_delivery(dc2, 8, "tokens", 1, out=c)
        assert g2.backend is g.backend and g2.total == 65 and not g2.released
        assert_same_dispatch(g2, c2)
        np.testing.assert_array_equal(gpu.backend_loads(), cpu.backend_loads())

        before = gpu.backend_loads().copy()
        tiny = dataclasses.replace(g2, backend=g2.backend[:64])
        with pytest.raises(ValueError):
            gpu.dispatch_delivery(dg2, 8, out=tiny)
        with pytest.raises(ValueError):  # built for another n_backends
            gpu.dispatch_delivery(dg2, 4, out=g2)
        np.testing.assert_array_equal(gpu.backend_loads(), before)
    finally:
        gpu.close()


@pytest.mark.gpu
def test_gpu_refusals():
    import dataclasses

    import torch

    gpu, _ = gpu_and_twin(num_backends=16)
    try:
        counts = [5, 6]
        agents, _, _ = fill([gpu], counts)
        d = deliver(gpu, agents, counts)
        before = refusals(gpu, d)
        good = gpu.dispatch_delivery(d, 4)
        gpu.release_dispatch(good)
        wrong = [
            dataclasses.replace(d, agent_row=d.agent_row.to(torch.int64)),
            dataclasses.replace(d, headers=d.headers.to(torch.int8)),
            dataclasses.replace(d, agent_row=d.agent_row.cpu()),
            dataclasses.replace(d, headers=d.headers.cpu()),
            dataclasses.replace(d, agent_row=d.agent_row[::2]),
            dataclasses.replace(d, headers=d.headers[:, :40]),
            dataclasses.replace(d, agent_row=d.agent_row.cpu().numpy()),
        ]
        for w in wrong:
            with pytest.raises(ValueError):
                gpu.dispatch_delivery(w, 4)
            np.testing.assert_array_equal(gpu.backend_loads(), before)
        outs = [
            dataclasses.replace(good, backend=good.backend.to(torch.int64)),
            dataclasses.replace(good, order=good.order.cpu()),
            dataclasses.replace(good, added=good.added.to(torch.int32)),
        ]
        for o in outs:
            with pytest.raises(ValueError):
                gpu.dispatch_delivery(d, 4, out=o)
            np.testing.assert_array_equal(gpu.backend_loads(), before)
    finally:
        gpu.close()


@pytest.mark.gpu
def test_facade_dispatch_gpu(tmp_path):
    import torch  # noqa: F401

    from swarmdb_amd.runtime.gpu_engine import GpuEngine

    cfg = small_cfg(save_dir=str(tmp_path / "gpu"))
    db = SwarmsDB(config=cfg, engine=GpuEngine(cfg))
    try:
        facade_round_trip(db)
        d = db.receive_device(["bob"])
        assert d.total == 0
        got = db.dispatch_device(d, ["bob"])
        assert got.backend.is_cuda and got.m == 0
        assert got.to_host().offsets.tolist() == [0, 0, 0, 0]
        db.complete_device(got)
    finally:
        db.close()
