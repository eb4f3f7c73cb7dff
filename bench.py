#!/usr/bin/env python3
"""Flagship benchmark — messages/sec (whole node) + p50 send->receive
latency, 1024 agents per GPU (BASELINE.json headline metric).

Each timed step is one full delivery tick through the GPU-resident queue:

  build batch -> [N>1: RCCL all-to-all routing over xGMI] -> pinned H2D
  staging -> enqueue kernel (slot write + inbox append + DELIVERED ack)
  -> broadcast fan-out kernel -> dequeue kernel (visibility filter +
  LDS sort + READ) -> payload gather kernel -> D2H -> host holds bytes.

Latency is measured PER MESSAGE, not per tick: every message header
carries its submission timestamp (stamped when the batch is handed to
the queue — for the pipelined path that is at pinned-buffer staging, so
pipeline wait is included). A dedicated steady-state latency phase runs
immediately AFTER the timed loop (sampling drains the async delivery
pipeline, ~6% throughput, which must not contaminate the timed region):
each phase step drains the delivery D2H, records the wall-clock receive
time and keeps a random sample of delivered seqs; p50/p99 of
(receive time - submission timestamp) are computed from those headers.

Usage (driver contract):
  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
A plain run sets up, warms up, times the K steps and prints the result
line. --full additionally runs the per-message latency phase and the
GPU-busy sampler (p50/p99/n_latency_samples/gpu_busy_pct in the result
line). --dump-outputs DIR writes what the last timed step delivered as
DIR/<name>.npy (see dump_outputs below).
For N>1 the driver launches via torch.distributed.run; ranks read
RANK/LOCAL_RANK/WORLD_SIZE from the env. Scaling is weak: 1024 agents and
the same message load per GPU.

No GPU present -> falls back to the CPU engine (config-1 loopback) so the
script stays runnable in CPU CI; the driver's numbers come from MI355X.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))

from swarmdb_amd.core.config import QueueConfig  # noqa: E402
from swarmdb_amd.runtime.engine import (  # noqa: E402
    BROADCAST,
    NO_BITMAP,
    REC_DTYPE,
    VIS_ALL,
)


def build_batches(rng, n_batches, batch, agents_global, rank, world,
                  payload_bytes, bcast_frac=0.0):
    """Pre-build rotating synthetic batches (random agent ids, 1 KB chat
    messages — BASELINE 'synthetic messages, random agent IDs')."""
    stride = (payload_bytes + 15) // 16 * 16
    local_agents = np.arange(rank, agents_global, world, dtype=np.uint32)
    batches = []
    for _ in range(n_batches):
        recs = np.zeros(batch, dtype=REC_DTYPE)
        # senders are local agents; receivers uniform over the global space
        recs["sender"] = rng.choice(local_agents, batch)
        recv = rng.integers(0, agents_global, batch).astype(np.uint32)
        if bcast_frac > 0:
            recv[rng.random(batch) < bcast_frac] = BROADCAST
        recs["receiver"] = recv
        recs["type"] = 0  # chat
        recs["priority"] = rng.integers(0, 4, batch)
        recs["timestamp"] = time.time()
        recs["vis_mode"] = VIS_ALL
        recs["bitmap"] = NO_BITMAP
        recs["payload_len"] = payload_bytes
        recs["content_len"] = payload_bytes
        recs["payload_off"] = np.arange(batch, dtype=np.uint64) * stride
        payload = rng.integers(32, 127, batch * stride, dtype=np.uint8).tobytes()
        batches.append((recs, payload))
    return batches, local_agents


def dump_outputs(out_dir, engine, counts, seqs, seq_base, payload_bytes,
                 rank, world):
    """Write what the last timed step delivered as DIR/<name>.npy.

    counts       float32 [n_agents]   messages delivered to each polled agent
    seq_offsets  float64 [n_delivered] delivered seqs in agent order, relative
                                       to the first seq the step enqueued (the
                                       absolute base depends on how many
                                       warmup ticks ran)
    sample_index float64 [k]          positions in seq_offsets of a fixed,
                                       seeded sample (k <= 4096)
    headers      float32 [k, 4]       sender, receiver, priority, payload_len
                                       of the sampled messages
    payloads     float32 [k, payload] their payload bytes
    """
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    sfx = f"_rank{rank}" if world > 1 else ""
    counts = np.asarray(counts, dtype=np.int64)
    seqs = np.asarray(seqs, dtype=np.uint64)
    np.save(out / f"counts{sfx}.npy", counts.astype(np.float32))
    np.save(out / f"seq_offsets{sfx}.npy",
            seqs.astype(np.float64) - float(seq_base))
    k = min(4096, len(seqs))
    idx = np.sort(np.random.default_rng(0).choice(len(seqs), k, replace=False))
    hdr_out = np.zeros((k, 4), dtype=np.float32)
    pay_out = np.zeros((k, payload_bytes), dtype=np.float32)
    if k:
        hdrs, pays = engine.fetch(seqs[idx].copy())
        for c, name in enumerate(
            ("sender", "receiver", "priority", "payload_len")
        ):
            hdr_out[:, c] = hdrs[name]
        for r, pay in enumerate(pays):
            b = np.frombuffer(pay, dtype=np.uint8)[:payload_bytes]
            pay_out[r, : len(b)] = b
    np.save(out / f"sample_index{sfx}.npy", idx.astype(np.float64))
    np.save(out / f"headers{sfx}.npy", hdr_out)
    np.save(out / f"payloads{sfx}.npy", pay_out)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--agents", type=int, default=1024,
                    help="agents per GPU (weak scaling)")
    ap.add_argument("--batch", type=int, default=16384,
                    help="messages per step per GPU")
    ap.add_argument("--payload", type=int, default=1024,
                    help="payload bytes (1 KB chat messages)")
    ap.add_argument("--priority", action="store_true",
                    help="priority-ordered dequeue (config 3 kernel)")
    ap.add_argument("--bcast-frac", type=float, default=0.0,
                    help="fraction of messages sent as broadcasts "
                         "(each fans out to every agent)")
    ap.add_argument("--no-gather", action="store_true",
                    help="skip payload D2H gather (delivery stays device-side)")
    ap.add_argument("--dump-steps", action="store_true",
                    help="print per-step wall times (variance diagnosis)")
    ap.add_argument("--graph", action="store_true",
                    help="use the hipGraph-captured tick (measured neutral "
                         "at large batches, slower at small — default off)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed "
                         "step delivered as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run the per-message latency phase and the "
                         "GPU-busy sampler (a plain run only times the steps)")
    args = ap.parse_args()

    import torch

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    have_gpu = torch.cuda.is_available()

    dist_on = world > 1
    backend = os.environ.get(
        "SWARMDB_BENCH_BACKEND", "nccl" if have_gpu else "gloo"
    )
    if dist_on:
        import torch.distributed as dist

        if have_gpu:
            torch.cuda.set_device(local_rank % max(1, torch.cuda.device_count()))
        if backend == "nccl" and have_gpu:
            dist.init_process_group(
                backend=backend,
                device_id=torch.device(
                    "cuda", local_rank % max(1, torch.cuda.device_count())
                ),
            )
        else:
            dist.init_process_group(backend=backend)

    agents_global = args.agents * world
    max_agents = ((agents_global + 63) // 64) * 64
    rng = np.random.default_rng(1234 + rank)

    n_dev = torch.cuda.device_count() if have_gpu else 1
    cfg = QueueConfig(
        use_gpu=have_gpu,
        max_agents=max_agents,
        num_slots=max(1 << 20, 4 * args.batch * world),
        # tight slots: payload rounded to 16 B + 64 B headroom — denser
        # HBM writes and less PCIe on the gather than a fixed 2 KiB slot
        slot_bytes=max(256, ((args.payload + 15) // 16) * 16 + 64),
        inbox_capacity=1 << 16,
        # dequeue window: 4x the expected poll depth (pow2, min 256);
        # small windows keep many dequeue workgroups resident
        recv_window=min(
            4096,
            max(
                256,
                1
                << (
                    4 * max(64, 4 * args.batch * world // max(1, args.agents))
                    - 1
                ).bit_length(),
            ),
        ),
        staging_batch=max(16384, args.batch * (2 if dist_on else 1)),
        device_index=local_rank % max(1, n_dev),
        auto_save=False,
        world_size=world,
        rank=rank,
    )
    if have_gpu:
        from swarmdb_amd.runtime.gpu_engine import GpuEngine

        engine = GpuEngine(cfg)
    else:
        from swarmdb_amd.runtime.cpu_engine import CpuEngine

        engine = CpuEngine(cfg)

    batches, local_agents = build_batches(
        rng, min(8, max(2, args.steps)), args.batch, agents_global, rank,
        world, args.payload, bcast_frac=args.bcast_frac,
    )
    for a in local_agents:
        engine.register_agent(int(a))

    router = None
    grouter = None
    if dist_on:
        if have_gpu and backend == "nccl":
            # GPU-direct: pack kernel -> RCCL all-to-all over xGMI ->
            # device-side ingest (payloads never touch the host)
            from swarmdb_amd.parallel.router import GpuDirectRouter

            grouter = GpuDirectRouter(engine, torch.device("cuda", local_rank))
        else:
            # host-path exchange (gloo): engine may still be the GPU one
            from swarmdb_amd.parallel.router import CrossGpuRouter

            router = CrossGpuRouter(torch.device("cpu"))

    per_agent = args.batch * world / max(1, agents_global)
    per_agent += args.bcast_frac * args.batch * world  # every bcast hits all
    recv_K = max(64, int(4 * per_agent))
    sent_total = 0
    recv_total = 0

    # per-message latency sampling: on sampled steps the delivery D2H
    # is drained, the receive wall-time recorded, and a random subset
    # of delivered seqs kept; deltas against the header timestamps are
    # computed at the end. Sampling runs in a DEDICATED steady-state
    # phase after the timed loop (draining the async delivery pipeline
    # costs ~6% throughput, which must not contaminate the timed
    # region); the latencies are still real per-message measurements.
    sampling = {"on": False}
    # --dump-outputs: the last timed step keeps its counts and delivered
    # seqs (dense [na, K] layouts are compacted) for dump_outputs()
    capture = {"on": False, "counts": None, "seqs": None}
    lat_deltas: list = []  # per-message (t_recv - submission) seconds

    def keep_sample(t_recv: float, seqs, counts=None, K=None) -> None:
        if seqs is None or len(seqs) == 0:
            return
        seqs = np.asarray(seqs, dtype=np.uint64)
        if counts is not None:
            # dense [na, K] layout: keep only valid entries
            c64 = np.asarray(counts, dtype=np.int64)
            mat = seqs.reshape(len(c64), K)
            seqs = mat[np.arange(K)[None, :] < c64[:, None]]
            if len(seqs) == 0:
                return
        take = min(128, len(seqs))
        idx = rng.choice(len(seqs), take, replace=False)
        # fetch the headers NOW (the phase is untimed): deferring the
        # fetch lets the slot ring evict/reuse sampled seqs first
        hdrs, _ = engine.fetch(seqs[idx].copy())
        ts = np.asarray(hdrs["timestamp"], dtype=np.float64)
        d = t_recv - ts
        d = d[(ts > 0) & (d >= 0) & (d < 60.0)]
        if len(d):
            lat_deltas.append(d)

    def barrier_sync():
        if dist_on:
            import torch.distributed as dist

            dist.barrier()
        if have_gpu:
            torch.cuda.synchronize()

    def step(i: int) -> int:
        nonlocal sent_total, recv_total, grouter, router
        recs, payload = batches[i % len(batches)]
        recs["timestamp"] = time.time()  # submission stamp (per message)
        if grouter is not None:
            try:
                sent_local = grouter.route_and_enqueue(recs, payload)
            except Exception as e:
                # first-line fallback: host-path router still uses RCCL
                # for the exchange but routes via host buffers — the
                # scaling run survives a GPU-direct path failure
                if i == 0:
                    print(f"[bench] GpuDirectRouter failed ({e}); "
                          "falling back to host-path router",
                          file=sys.stderr)
                    from swarmdb_amd.parallel.router import CrossGpuRouter

                    router = CrossGpuRouter(
                        torch.device("cuda", local_rank)
                    )
                    grouter = None
                    recs2, payload2 = router.route(recs, payload)
                    engine.enqueue_batch(recs2, payload2)
                    sent_local = len(recs2)
                else:
                    raise
        else:
            if router is not None:
                recs, payload = router.route(recs, payload)
            engine.enqueue_batch(recs, payload)
            sent_local = len(recs)
        counts, seqs = engine.receive_many(
            local_agents, recv_K, priority_order=args.priority
        )
        ndel = int(counts.sum())
        if not args.no_gather and ndel:
            # payload gather + D2H: bytes land in pinned host memory
            deliver = getattr(engine, "deliver_payloads", None)
            if deliver is not None:
                deliver(seqs, args.payload)
            else:
                engine.fetch(seqs)
        if sampling["on"] and ndel:
            keep_sample(time.time(), seqs)
        if capture["on"]:
            capture["counts"] = np.asarray(counts, dtype=np.int64)
            capture["seqs"] = np.asarray(seqs, dtype=np.uint64).copy()
        sent_total += sent_local
        recv_total += ndel
        return ndel

    # single-GPU pipelined path: batches live in PINNED host buffers and
    # upload on a dedicated H2D stream, overlapping the previous tick's
    # kernels and delivery D2H — zero host copies on the send path.
    # (Never in distributed mode: the routed step above owns that case.)
    pipelined = have_gpu and not dist_on and hasattr(engine, "q")
    if pipelined:
        q = engine.q
        pinned = []
        for recs, payload in batches:
            pr = q.alloc_pinned(recs.nbytes)
            pr_view = np.frombuffer(pr, dtype=REC_DTYPE)
            pr_view[:] = recs
            pp = q.alloc_pinned(len(payload))
            np.frombuffer(pp, dtype=np.uint8)[:] = np.frombuffer(
                payload, dtype=np.uint8
            )
            pinned.append((pr, pp, len(recs), len(payload), pr_view))

        def _prefetch(slot: int, i: int) -> None:
            pr, pp, n, nbytes, pr_view = pinned[i % len(pinned)]
            # submission stamp: the moment the batch is handed to the
            # queue (upload begins) — pipeline wait counts as latency
            pr_view["timestamp"] = time.time()
            q.prefetch_from(
                slot,
                pr.__array_interface__["data"][0],
                pp.__array_interface__["data"][0],
                n,
                nbytes,
            )

        _prefetch(0, 0)

        # hipGraph-captured steady-state tick: enqueue + fanout +
        # receive + result D2H replay as ONE graph launch per step
        use_graph = args.graph and args.bcast_frac == 0
        if use_graph:
            try:
                q.build_tick(args.batch, local_agents.astype(np.uint32),
                             recv_K, bool(args.priority))
            except Exception as e:
                print(f"[bench] tick-graph capture unavailable ({e}); "
                      "using discrete launches", file=sys.stderr)
                use_graph = False

        local_agents32 = local_agents.astype(np.uint32)

        def step(i: int, _cur=[0]) -> int:  # noqa: F811
            nonlocal sent_total, recv_total
            cur = _cur[0]
            n_staged = len(batches[i % len(batches)][0])
            sampled = sampling["on"]
            seqs = None
            counts_dense = None
            if use_graph:
                # upload batch i+1 first so its H2D overlaps this tick's
                # graph execution
                _prefetch(1 - cur, i + 1)
                counts, seqs = q.run_tick(cur)
                counts_dense = counts
                ndel = int(counts.astype(np.int64).sum())
            else:
                q.enqueue_staged(cur)
                # upload batch i+1 on the H2D stream: overlaps batch i's
                # kernels and the delivery D2H (full-duplex PCIe)
                _prefetch(1 - cur, i + 1)
                want_seqs = args.bcast_frac > 0 or sampled or capture["on"]
                counts, seqs = q.receive_many(
                    local_agents32, recv_K, bool(args.priority),
                    return_seqs=want_seqs,
                )
                counts_dense = counts if want_seqs else None
                ndel = int(counts.astype(np.int64).sum())
            if not args.no_gather and ndel:
                stride16 = (args.payload + 15) // 16 * 16
                fits = ndel * stride16 <= engine.cfg.staging_batch * engine.cfg.slot_bytes
                if fits:
                    # device-side gather straight from the dequeue output
                    # buffer; D2H overlaps the next tick (bounded 2 deep)
                    c64 = counts.astype(np.int64)
                    offs = np.zeros(len(c64), dtype=np.uint32)
                    offs[1:] = np.cumsum(c64[:-1]).astype(np.uint32)
                    q.deliver_outbuf(offs, ndel, int(c64.max()),
                                     args.payload, False)
                else:
                    # fan-out-heavy tick overflows the pinned staging:
                    # chunked delivery via the seq path
                    c64 = counts.astype(np.int64)
                    mat = seqs.reshape(len(local_agents32), recv_K)
                    taken = mat[np.arange(recv_K)[None, :] < c64[:, None]]
                    engine.deliver_payloads(taken, args.payload)
            if sampled and ndel and seqs is not None:
                # drain the in-flight delivery D2H so "received" means
                # bytes are host-visible, then stamp the receive time
                engine.delivery_sync()
                keep_sample(time.time(), seqs,
                            counts=counts_dense, K=recv_K)
            if capture["on"]:
                c64 = counts.astype(np.int64)
                mat = np.asarray(seqs, dtype=np.uint64).reshape(
                    len(local_agents32), recv_K
                )
                capture["counts"] = c64
                capture["seqs"] = mat[
                    np.arange(recv_K)[None, :] < c64[:, None]
                ]
            sent_total += n_staged
            recv_total += ndel
            _cur[0] = 1 - cur
            return ndel

    # Warmup: at least args.warmup steps AND at least 150 ms of wall
    # time. The floor is clock/power stabilization: with short steps a
    # one-time ~6.5 ms reclock event otherwise lands a few steps into
    # the timed region and poisons the mean (measured; profiles/
    # r02_results.md). Warmup work never counts toward the timed total.
    it = 0
    tw = time.perf_counter()
    for _ in range(args.warmup):
        step(it)
        it += 1
    elapsed_w = time.perf_counter() - tw
    extra = 0
    if elapsed_w < 0.15 and args.warmup > 0:
        per = max(elapsed_w / args.warmup, 1e-5)
        extra = int((0.15 - elapsed_w) / per) + 1
    if dist_on:
        # every rank must run the same number of steps (collectives):
        # agree on the max. Tensor device must match the backend (nccl
        # reduces CUDA tensors only).
        import torch.distributed as dist

        t = torch.tensor(
            [extra], dtype=torch.int64,
            device="cuda" if (have_gpu and backend == "nccl") else "cpu",
        )
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        extra = int(t.item())
    # the floor makes the warmup count timing-dependent: pad it to a
    # multiple of the batch rotation so timed step j always sends batch
    # j % len(batches) (same arguments -> same inputs, run to run)
    extra += -(it + extra) % len(batches)
    for _ in range(extra):
        step(it)
        it += 1

    # warmup deliveries must not count toward the timed total
    sent_total = 0
    recv_total = 0

    # best-effort GPU-busy sampler (the driver's own sampler can miss a
    # short timed region entirely — round-1 weak item 9): read the
    # sysfs gpu_busy_percent every 50 ms on a daemon thread
    busy_samples: list = []
    stop_busy = False
    if args.full and have_gpu and rank == 0:
        import glob as _glob
        import threading as _threading

        paths = _glob.glob(
            "/sys/class/drm/card*/device/gpu_busy_percent"
        )

        def _sample_busy():
            while not stop_busy and paths:
                try:
                    with open(paths[0]) as f:
                        busy_samples.append(float(f.read().strip()))
                except OSError:
                    return
                time.sleep(0.05)

        _threading.Thread(target=_sample_busy, daemon=True).start()

    barrier_sync()
    t0 = time.perf_counter()
    step_times = []
    for j in range(args.steps):
        capture["on"] = bool(args.dump_outputs) and j == args.steps - 1
        s = time.perf_counter()
        sent_before = sent_total
        step(it)
        it += 1
        step_times.append(time.perf_counter() - s)
    barrier_sync()
    t1 = time.perf_counter()
    stop_busy = True
    capture["on"] = False

    if args.dump_outputs and capture["counts"] is not None:
        sync = getattr(engine, "delivery_sync", None)
        if sync is not None:
            sync()  # the last delivery D2H shares the fetch staging buffer
        dump_outputs(
            args.dump_outputs, engine, capture["counts"], capture["seqs"],
            engine.total_messages() - (sent_total - sent_before),
            args.payload, rank, world,
        )

    # latency phase (--full only): same steady state, sampling on,
    # UNTIMED (every rank runs the same count — the distributed step has
    # collectives); capped at 128 steps so soak-length runs don't spend
    # minutes sampling
    lat_steps = max(8, min(args.steps // 2, 128)) if args.full else 0
    # Alternate sampled/unsampled steps: a sampled step's bookkeeping
    # (drain + header fetch) runs AFTER its own receive stamp but ages
    # the NEXT step's messages — with every step sampled that observer
    # overhead compounds into the percentiles. Alternation means every
    # sampled step measures messages stamped during a clean step. Two
    # unsampled flush steps first drain the batch that was prefetched
    # (and stamped) before the end-of-loop barrier.
    lat_sent = lat_recv = 0
    for _ in range(2 if args.full else 0):
        before_s, before_r = sent_total, recv_total
        step(it)
        it += 1
        lat_sent += sent_total - before_s
        lat_recv += recv_total - before_r
    phase_times = []
    for j in range(lat_steps):
        sampling["on"] = j % 2 == 1
        before_s, before_r = sent_total, recv_total
        ps = time.perf_counter()
        step(it)
        phase_times.append(time.perf_counter() - ps)
        it += 1
        lat_sent += sent_total - before_s
        lat_recv += recv_total - before_r
    sampling["on"] = False
    if args.dump_steps and args.full and rank == 0:
        print("phase_times_ms:",
              [round(t * 1000, 3) for t in phase_times])
    sent_total -= lat_sent  # latency phase is outside the timed totals
    recv_total -= lat_recv

    elapsed = t1 - t0
    if dist_on:
        import torch.distributed as dist

        t = torch.tensor([elapsed], dtype=torch.float64,
                         device="cuda" if (have_gpu and backend == "nccl") else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        tot = torch.tensor([float(recv_total)], dtype=torch.float64,
                           device="cuda" if (have_gpu and backend == "nccl") else "cpu")
        dist.all_reduce(tot, op=dist.ReduceOp.SUM)
        recv_all = int(tot.item())
    else:
        recv_all = recv_total

    if args.dump_steps and rank == 0:
        print("step_times_ms:", [round(t * 1000, 3) for t in step_times])

    # conservation: at steady state every enqueued message is delivered
    # within the same tick (broadcasts amplify, so only LOSS warns;
    # p2p-only runs should match within 5%)
    expect = sent_total * (1 + args.bcast_frac * max(0, args.agents - 1))
    if sent_total and recv_total < 0.95 * expect:
        print(
            f"[bench] WARNING rank {rank}: delivered {recv_total} of "
            f"~{int(expect)} expected — routing/dequeue loss",
            file=sys.stderr,
        )

    msgs_per_s = recv_all / elapsed
    ms_per_step = elapsed / args.steps * 1000.0

    # per-message latency: receive wall time minus the submission stamp
    # carried in each sampled message's header
    p50_ms = p99_ms = None
    n_lat = 0
    if lat_deltas:
        alld = np.concatenate(lat_deltas)
        n_lat = int(len(alld))
        p50_ms = float(np.median(alld) * 1000.0)
        p99_ms = float(np.percentile(alld, 99) * 1000.0)
    if p50_ms is None:
        # no samples (zero deliveries in the latency phase): fall back to
        # tick-duration bound and say so via n_lat_samples = 0
        p50_ms = float(np.median(step_times) * 1000.0)
        p99_ms = float(np.percentile(step_times, 99) * 1000.0)

    if rank == 0:
        out = {
            "metric": "messages/sec (whole node), 1024 agents/GPU, "
                      "1 KB synthetic chat messages",
            "value": round(msgs_per_s, 1),
            "unit": "msg/s",
            "n_gpus": world if have_gpu else 0,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,  # reference publishes no numbers
            "dtype": "uint8",
            "data": "synthetic",
            "config": {
                "model": "gpu-mpmc-ring-queue",
                "global_batch": args.batch * world,
                "seq_len": args.payload,
                "parallelism": f"agent-sharded all-to-all x{world}"
                if world > 1
                else "single-gpu",
                "agents": agents_global,
                "engine": type(engine).__name__,
                "priority_dequeue": bool(args.priority),
                "payload_gather_d2h": not args.no_gather,
            },
        }
        if args.full:
            out["p50_latency_ms"] = round(p50_ms, 3)
            out["p99_latency_ms"] = round(p99_ms, 3)
            out["n_latency_samples"] = n_lat
            # None when sysfs gpu_busy_percent is absent or reads 0
            # throughout (the kernel evidence in profiles/ covers
            # utilization instead)
            out["gpu_busy_pct"] = (
                round(float(np.mean(busy_samples)), 1)
                if busy_samples and max(busy_samples) > 0
                else None
            )
        print(json.dumps(out))

    engine.close()
    if dist_on:
        import torch.distributed as dist

        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
