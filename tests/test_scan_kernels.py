"""The two scan kernels, k_search<P> and k_filter, against naive loops.

Chain (tests/README.md): naive reference -> CpuEngine -> GPU. The naive
references below are plain Python over the test's own record of what it
sent (a list of ``Msg``); they share no code with either engine. The CPU half runs
anywhere; the GPU half builds one small GpuEngine per test. Everything
compared is an integer set or an integer sequence: no tolerance.

``search_range`` / ``query_range`` return one window's matches unordered
(search possibly once per matching 16 B chunk), so they are compared as
sorted unique sets; ``engine.search`` / ``engine.query`` are compared
exactly, newest first. ``blocks=`` and ``loads=`` shrink the scan grid so
that a few thousand 16 B messages reach k_search's software-pipelined
loop (more than ``blocks * 256 * (loads - 1)`` chunks) and k_filter's
grid-stride loop, which the production grid enters only above 64 MB of
payload and 524288 seqs.

The file holds CPU and GPU tests, so GPU tests carry the marker one by
one.
"""

from dataclasses import dataclass

import numpy as np
import pytest

from swarmdb_amd import QueueConfig
from swarmdb_amd.runtime.cpu_engine import CpuEngine
from swarmdb_amd.runtime.engine import (
    NO_BITMAP,
    REC_DTYPE,
    ST_DELETED,
    ST_DELIVERED,
    ST_FAILED,
    ST_PROCESSED,
    ST_READ,
    VIS_ALL,
)

N_AGENTS = 8
T0 = 1.7e9  # timestamps T0 + i are exact doubles

# ASCII folding maps A-Z to a-z and nothing else.
FOLD = bytes(c + 32 if 0x41 <= c <= 0x5A else c for c in range(256))

# The small alphabet: an upper/lower pair for the needles' first and
# second characters; three pairs 0x20 apart that folding must NOT merge
# (` @, [ {, 0xC1 0xE1); and 'c' == 'b' ^ 1, which the packed first-byte
# test (haszero on w ^ splat) flags through its borrow when it sits above
# a real 'b' — the screen may pass it, the verify must not.
ALPHABET = np.frombuffer(b"bBrR`@[{\xc1\xe1c", dtype=np.uint8)

# two needles per length 1..5, over the alphabet
RANDOM_NEEDLES = [
    b"b", b"@",
    b"bR", b"[b",
    b"Br`", b"\xc1rb",
    b"bR{c", b"r@Bb",
    b"bRc`B", b"`\xe1[rb",
]
RANDOM_SEED = 5
RANDOM_N = 1500  # x 4 chunks of slot_bytes=64 stays under staging_batch


# ---------------------------------------------------------------------------
# the test's own record of the log, and the naive references
# ---------------------------------------------------------------------------


@dataclass
class Msg:
    payload: bytes          # as sent
    content_len: int        # as sent (may exceed len(payload))
    sender: int = 0
    receiver: int = 1
    type: int = 0
    timestamp: float = T0
    bad: bool = False       # malformed on purpose: takes the error lane
    status: int = ST_DELIVERED

    @property
    def stored(self) -> bytes:
        """The payload the engine keeps: none for an error-lane record."""
        return b"" if self.bad else self.payload


def naive_search(log, needle, fold, lo=0, hi=None):
    """Seqs in [lo, hi) whose content window holds the needle, newest
    first. The window is payload[:min(content_len, payload_len)]."""
    hi = len(log) if hi is None else min(hi, len(log))
    if fold:
        needle = needle.translate(FOLD)
    hits = []
    for seq in range(lo, hi):
        m = log[seq]
        if m.status == ST_DELETED:
            continue
        pay = m.stored
        window = pay[: min(m.content_len, len(pay))]
        if fold:
            window = window.translate(FOLD)
        if needle in window:
            hits.append(seq)
    return hits[::-1]


def naive_query(log, lo=0, hi=None, sender=None, receiver=None,
                type_code=None, status=None, after=None, before=None):
    """Seqs in [lo, hi) that pass the six predicates, newest first. Both
    time bounds are exclusive."""
    hi = len(log) if hi is None else min(hi, len(log))
    hits = []
    for seq in range(lo, hi):
        m = log[seq]
        if m.status == ST_DELETED:
            continue
        if sender is not None and m.sender != sender:
            continue
        if receiver is not None and m.receiver != receiver:
            continue
        if type_code is not None and m.type != type_code:
            continue
        if status is not None and m.status != status:
            continue
        if after is not None and not m.timestamp > after:
            continue
        if before is not None and not m.timestamp < before:
            continue
        hits.append(seq)
    return hits[::-1]


# ---------------------------------------------------------------------------
# engines and sending
# ---------------------------------------------------------------------------


def cfg(**kw):
    base = dict(
        use_gpu=True,
        max_agents=64,
        num_slots=4096,
        slot_bytes=64,
        inbox_capacity=1 << 12,
        staging_batch=8192,
        num_backends=16,
        auto_save=False,
    )
    base.update(kw)
    return QueueConfig(**base)


def make_engine(kind, **kw):
    if kind == "gpu":
        from swarmdb_amd.runtime.gpu_engine import GpuEngine

        eng = GpuEngine(cfg(**kw))
    else:
        eng = CpuEngine(cfg(use_gpu=False, **kw))
    for a in range(N_AGENTS):
        eng.register_agent(a)
    return eng


def close(eng):
    if hasattr(eng, "close"):
        eng.close()


def evict_base(eng, log):
    """First live seq: the CPU log never evicts."""
    if isinstance(eng, CpuEngine):
        return 0
    return max(0, len(log) - eng.cfg.num_slots)


def records(msgs):
    """REC_DTYPE records + payload bytes; every payload starts 16 B
    aligned with zero padding, as the enqueue kernel's copy wants."""
    n = len(msgs)
    recs = np.zeros(n, dtype=REC_DTYPE)
    buf = bytearray()
    for i, m in enumerate(msgs):
        recs["payload_off"][i] = len(buf)
        buf += m.payload + b"\x00" * (-len(m.payload) % 16)
    buf += b"\x00" * 16
    recs["sender"] = [m.sender for m in msgs]
    recs["receiver"] = [m.receiver for m in msgs]
    recs["type"] = [99 if m.bad else m.type for m in msgs]
    recs["timestamp"] = [m.timestamp for m in msgs]
    recs["payload_len"] = [len(m.payload) for m in msgs]
    recs["content_len"] = [m.content_len for m in msgs]
    recs["vis_mode"] = VIS_ALL
    recs["bitmap"] = NO_BITMAP
    return recs, bytes(buf)


def send(eng, log, msgs, via="batch"):
    """Enqueue msgs, through enqueue_batch or enqueue_from_device, and
    append them to the log."""
    recs, buf = records(msgs)
    if via == "batch":
        seqs = eng.enqueue_batch(recs, buf)
    else:
        stride = eng.cfg.slot_bytes
        rows = np.zeros((len(msgs), stride), dtype=np.uint8)
        for i, m in enumerate(msgs):
            rows[i, : len(m.payload)] = np.frombuffer(m.payload, dtype=np.uint8)
        headers = recs.view(np.uint8).reshape(len(msgs), REC_DTYPE.itemsize)
        if isinstance(eng, CpuEngine):
            seqs = eng.enqueue_from_device(headers, rows)
        else:
            import torch

            seqs = eng.enqueue_from_device(
                torch.from_numpy(headers).cuda(), torch.from_numpy(rows).cuda()
            )
    assert seqs.tolist() == list(range(len(log), len(log) + len(msgs)))
    for m in msgs:
        if m.bad:  # as records() sent it
            m.type, m.status = 99, ST_FAILED
        log.append(m)
    return seqs


def check_search(eng, log, needle, fold, **grid):
    """engine.search exactly, and on the GPU one search_range over the
    whole live window as a set. Returns the naive hits."""
    eb = evict_base(eng, log)
    want = naive_search(log, needle, fold, lo=eb)
    got = eng.search(needle, case_sensitive=not fold, limit=len(log) + 1)
    assert got.tolist() == want, (needle, fold)
    if not isinstance(eng, CpuEngine):
        raw = eng.q.search_range(0, len(log), needle, fold,
                                 eng.cfg.staging_batch, **grid)
        assert np.unique(raw).tolist() == sorted(want), (needle, fold, grid)
    return want


QUERY_KEYS = ("sender", "receiver", "type_code", "status", "after", "before")


def query_range(eng, lo, hi, blocks=0, **kw):
    mask = sum(1 << i for i, k in enumerate(QUERY_KEYS) if kw.get(k) is not None)
    args = [-1 if kw.get(k) is None else int(kw[k]) for k in QUERY_KEYS[:4]]
    args += [0.0 if kw.get(k) is None else float(kw[k]) for k in QUERY_KEYS[4:]]
    return eng.q.query_range(lo, hi, *args, mask, eng.cfg.staging_batch,
                             blocks=blocks)


def check_query(eng, log, **kw):
    eb = evict_base(eng, log)
    want = naive_query(log, lo=eb, **kw)
    got = eng.query(limit=len(log) + 1, **kw)
    assert got.tolist() == want, kw
    assert eng.query(limit=7, **kw).tolist() == want[:7], kw
    if not isinstance(eng, CpuEngine):
        for blocks in (0, 1, 2):
            raw = query_range(eng, 0, len(log), blocks=blocks, **kw)
            assert len(raw) == len(want), (kw, blocks)  # each seq once
            assert np.sort(raw).tolist() == sorted(want), (kw, blocks)
    return want


# ---------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------


def swap_case(b: bytes) -> bytes:
    return bytes(c ^ 0x20 if (0x41 <= c <= 0x5A or 0x61 <= c <= 0x7A) else c
                 for c in b)


def near_miss(rng, b: bytes) -> bytes:
    """One byte of b moved to its 0x20 partner where folding must not
    follow (` @ [ { 0xC1 0xE1), else to its XOR-1 neighbour."""
    i = int(rng.integers(0, len(b)))
    c = b[i]
    c = c ^ 0x20 if c in b"`@[{\xc1\xe1" else c ^ 1
    return b[:i] + bytes([c]) + b[i + 1:]


def random_msgs(rng, n, slot_bytes, needles, plants=(1, 4)):
    """Random text over ALPHABET with copies, case-swapped copies and
    near misses of the needles dropped in at random places (also across
    the end of the content window), random content_len <= payload_len <=
    slot_bytes, senders/receivers/types spread out."""
    msgs = []
    for i in range(n):
        plen = int(rng.integers(0, slot_bytes + 1))
        clen = plen if rng.random() < 0.3 else int(rng.integers(0, plen + 1))
        text = bytearray(ALPHABET[rng.integers(0, len(ALPHABET), plen)].tobytes())
        for _ in range(int(rng.integers(*plants))):
            nd = needles[int(rng.integers(0, len(needles)))]
            v = rng.random()
            if v < 0.25:
                nd = swap_case(nd)
            elif v < 0.5:
                nd = near_miss(rng, nd)
            if len(nd) <= plen:
                p = int(rng.integers(0, plen - len(nd) + 1))
                text[p : p + len(nd)] = nd
        msgs.append(Msg(bytes(text), clen, sender=i % 5, receiver=(i * 7) % 6,
                        type=i % 7, timestamp=T0 + i))
    return msgs


def random_log():
    return random_msgs(np.random.default_rng(RANDOM_SEED), RANDOM_N, 64,
                       [nd for nd in RANDOM_NEEDLES if len(nd) >= 3])


# filler bytes that occur in no planted needle
FILL = b"."
PLANT_LENGTHS = (1, 2, 3, 16, 17, 33, 256)
_letters = np.frombuffer(
    b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ", dtype=np.uint8)
PLANT_TEXT = _letters[
    np.random.default_rng(11).integers(0, len(_letters), 256)].tobytes()


def planted_msgs():
    """For each needle PLANT_TEXT[:L] and each chunk phase j in 0..15,
    three messages of slot_bytes=512 on filler: the needle at 16k+j well
    inside the content; one that ends exactly at content_len; one whose
    last byte is the first byte of the extras (no hit)."""
    msgs = []
    for L in PLANT_LENGTHS:
        nd = PLANT_TEXT[:L]
        for j in range(16):
            k = (0, 1, 7, 15)[(j + L) % 4]
            off = 16 * k + j
            assert off + L <= 512
            tail = (j * 5) % (512 - off - L + 1)  # content after the needle
            for clen, plen in (
                (off + L + tail, 512 if j % 2 else off + L + tail),
                (off + L, off + L if j % 3 == 0 else min(512, off + L + 40)),
                (off + L - 1, min(512, off + L + j)),
            ):
                text = bytearray(FILL * plen)
                text[off : off + L] = nd
                msgs.append(Msg(bytes(text), clen, receiver=1 + j % 4,
                                timestamp=T0 + len(msgs)))
    return msgs


def wrap_msgs():
    """64 + 40 messages for num_slots=64, slot_bytes=64. The first 40 are
    evicted on the GPU; each holds the needle at byte 32, where its
    slot's next occupant (16 B long) leaves it as a stale tail. Live hits
    sit at both ends of both segments: seqs 40 and 63 (slots 40, 63), 64
    and 103 (slots 0, 39)."""
    nd = b"Wrap"
    msgs = []
    for i in range(104):
        if i < 40:
            text = FILL * 32 + nd + FILL * 28
        elif i in (40, 63, 64, 103, 50, 80):
            text = FILL * 11 + nd + b"."  # 16 B, the needle across byte 12..15
        else:
            text = FILL * 16
        msgs.append(Msg(text, len(text), receiver=1 + i % 4,
                        timestamp=T0 + i))
    return nd, msgs


# ---------------------------------------------------------------------------
# scenarios, run on either engine
# ---------------------------------------------------------------------------


def run_random_texts(kind):
    log, eng = [], make_engine(kind)
    try:
        send(eng, log, random_log())
        for nd in RANDOM_NEEDLES:
            for fold in (True, False):
                want = check_search(eng, log, nd, fold)
                # hits and misses are both common, per needle and mode
                assert 0.05 * len(log) < len(want) < 0.95 * len(log), (nd, fold)
            check_search(eng, log, swap_case(nd), True)
        # a limit cuts the newest
        want = naive_search(log, b"b", True)
        assert eng.search(b"b", False, 10).tolist() == want[:10]
    finally:
        close(eng)


def run_planted(kind):
    log, eng = [], make_engine(kind, slot_bytes=512, num_slots=1024)
    try:
        msgs = planted_msgs()
        send(eng, log, msgs)
        for L in PLANT_LENGTHS:
            nd = PLANT_TEXT[:L]
            want = check_search(eng, log, nd, False)
            # at least the two hits per phase planted for this length
            assert len(want) >= 32
            check_search(eng, log, swap_case(nd), True)
            check_search(eng, log, nd, True)
            check_search(eng, log, swap_case(nd), False)
        # the planted miss of every (L, j) is a miss
        longest = set(naive_search(log, PLANT_TEXT[:256], False))
        base = 3 * 16 * PLANT_LENGTHS.index(256)
        assert longest == {base + 3 * j + c for j in range(16) for c in (0, 1)}
    finally:
        close(eng)


def run_many_matches(kind):
    log, eng = [], make_engine(kind, slot_bytes=512, num_slots=1024,
                               staging_batch=4096)
    try:
        n = 200  # x 32 chunks > staging_batch: the window has to shrink
        send(eng, log, [Msg(b"a" * 512, 512, timestamp=T0 + i)
                        for i in range(n)])
        for limit in (1, 7, 64, 65, 199, 200, 1000):
            got = eng.search(b"a", True, limit).tolist()
            assert got == list(range(n - 1, -1, -1))[:limit], limit
        assert eng.search(b"A", False, 5).tolist() == [199, 198, 197, 196, 195]
        assert eng.search(b"A", True, 5).tolist() == []
    finally:
        close(eng)


def run_wrap(kind):
    log, eng = [], make_engine(kind, num_slots=64)
    try:
        nd, msgs = wrap_msgs()
        send(eng, log, msgs[:64])
        send(eng, log, msgs[64:])
        eb = evict_base(eng, log)
        for needle, fold in ((nd, False), (nd.lower(), True), (nd.lower(), False)):
            want = check_search(eng, log, needle, fold)
            if kind == "gpu":
                assert eb == 40 and min(want, default=eb) >= eb
        if kind == "gpu":
            assert check_search(eng, log, nd, False) == [103, 80, 64, 63, 50, 40]
            for lo, hi in ((40, 104), (50, 70), (63, 65), (64, 104), (0, 1000),
                           (41, 103), (63, 64), (103, 104)):
                raw = eng.q.search_range(lo, hi, nd, False, 8192)
                assert np.unique(raw).tolist() == sorted(
                    naive_search(log, nd, False, max(lo, eb), hi)), (lo, hi)
    finally:
        close(eng)


def run_status(kind):
    log, eng = [], make_engine(kind)
    try:
        nd = b"Status"
        msgs = [Msg(FILL * (i % 16) + nd + FILL * 3, i % 16 + 9,
                    receiver=1 + i % 2, timestamp=T0 + i) for i in range(40)]
        for i in (3, 17, 18):
            msgs[i].bad = True
        send(eng, log, msgs)
        for s in (0, 5, 39):
            assert eng.delete(s)
            log[s].status = ST_DELETED
        for s in eng.receive(1, 6).tolist():  # these become READ
            log[s].status = ST_READ
        for s in (7, 8, 20):
            eng.set_status(s, ST_PROCESSED)
            log[s].status = ST_PROCESSED
        assert {m.status for m in log} == {
            ST_DELIVERED, ST_FAILED, ST_DELETED, ST_READ, ST_PROCESSED}
        want = check_search(eng, log, nd, False)
        check_search(eng, log, nd.upper(), True)
        hit_status = {log[s].status for s in want}
        assert hit_status == {ST_DELIVERED, ST_READ, ST_PROCESSED}
        assert len(want) == 40 - 3 - 3
    finally:
        close(eng)


def run_clamp(kind, via):
    """content_len above payload_len is stored clamped, so the window
    ends with the record's own bytes: not in the slot's previous occupant
    (GPU: slot reuse after a wrap), not in the next record's bytes (CPU:
    the next payload on the heap; GPU: the next slot)."""
    log, eng = [], make_engine(kind, num_slots=8)
    try:
        nd = b"Needle"
        sb = eng.cfg.slot_bytes
        # old occupants of all 8 slots: the needle's tail right after the
        # 16 B a new occupant will write, and the whole needle further on
        old = b"edle" + FILL * 10 + nd + FILL * 12
        send(eng, log, [Msg(FILL * 16 + old, 16 + len(old), timestamp=T0 + i)
                        for i in range(8)], via)
        a = Msg(FILL * 14 + b"Ne", sb)            # slot 0
        b = Msg(b"edle" + FILL * 10 + b"Ne", sb + 200)  # slot 1, not the last
        c = Msg(b"edle" + FILL * 12, 16)          # slot 2
        seqs = send(eng, log, [a, b, c], via)
        assert seqs.tolist() == [8, 9, 10]
        hdrs, pays = eng.fetch(seqs)
        assert hdrs["payload_len"].tolist() == [16, 16, 16]
        assert hdrs["content_len"].tolist() == [16, 16, 16]
        assert pays == [a.payload, b.payload, c.payload]
        for needle, fold in ((nd, False), (b"needle", True), (b"e", False)):
            want = check_search(eng, log, needle, fold)
            if needle != b"e":
                assert not set(want) & {8, 9, 10}
    finally:
        close(eng)


def filter_msgs(n):
    return [Msg(b"x" * 16, 16, sender=i % 5, receiver=(i * 7) % 6, type=i % 7,
                timestamp=T0 + i) for i in range(n)]


def run_filter(kind, n, **kw):
    log, eng = [], make_engine(kind, slot_bytes=16, **kw)
    try:
        msgs = filter_msgs(n)
        for i in range(0, n, 97):
            msgs[i].bad = True
        for a in range(0, n, 2000):
            send(eng, log, msgs[a : a + 2000])
        eb = evict_base(eng, log)
        rng = np.random.default_rng(3)
        live = np.arange(eb, n)
        st = rng.choice([ST_READ, ST_PROCESSED, ST_DELETED], len(live) // 2)
        seqs = rng.choice(live, len(st), replace=False)
        keep = np.array([not log[s].bad for s in seqs])
        seqs, st = seqs[keep], st[keep]
        eng.set_statuses(seqs.astype(np.uint64), st.astype(np.uint32))
        for s, v in zip(seqs.tolist(), st.tolist()):
            log[s].status = v
        mid = eb + (n - eb) // 2
        lo_t, hi_t = T0 + mid - 300, T0 + mid + 300  # stored timestamps
        everything = dict(sender=3, receiver=5, type_code=2,
                          status=ST_DELIVERED, after=T0 + eb + 10,
                          before=T0 + n - 10)
        cases = [
            dict(),
            dict(sender=3),
            dict(receiver=5),
            dict(type_code=2),
            dict(status=ST_READ),
            dict(status=ST_FAILED),
            dict(after=lo_t),
            dict(before=hi_t),
            dict(after=lo_t, before=hi_t),
            dict(after=T0 + n - 2),          # the newest alone
            dict(before=T0 + eb + 1),        # the oldest live alone
            dict(after=lo_t, before=lo_t + 1),  # nothing strictly between
            everything,
            dict(sender=1, type_code=1),
        ]
        for case in cases:
            want = check_query(eng, log, **case)
            if "after" in case and "before" in case and len(case) == 2:
                # both ends excluded, everything strictly between is
                # there unless deleted
                ts = [log[s].timestamp for s in want]
                assert all(case["after"] < t < case["before"] for t in ts)
        assert check_query(eng, log, after=lo_t, before=lo_t + 1) == []
        assert any(m.status == ST_DELETED for m in log[eb:])
        assert check_query(eng, log, status=ST_DELETED) == []
        assert check_query(eng, log, **everything)  # not vacuous
        assert len(check_query(eng, log, after=T0 + n - 2)) <= 1
    finally:
        close(eng)


# ---------------------------------------------------------------------------
# CPU: CpuEngine against the naive references
# ---------------------------------------------------------------------------


def test_naive_search_reference():
    """The reference itself, on cases written out by hand."""
    log = [
        Msg(b"xxAbc", 5),
        Msg(b"xxabc", 4),            # the needle's last byte is an extra
        Msg(b"xxabc", 99),           # content_len above the payload
        Msg(b"`bc @BC {bc [BC", 15),
        Msg(b"abc", 3, status=ST_DELETED),
        Msg(b"abc", 3, bad=True, status=ST_FAILED),
        Msg(b"\xc1bc", 3),
    ]
    assert naive_search(log, b"abc", False) == [2]
    assert naive_search(log, b"abc", True) == [2, 0]
    assert naive_search(log, b"ABC", True) == [2, 0]
    assert naive_search(log, b"@bc", True) == [3]
    assert naive_search(log, b"`bc", True) == [3]
    assert naive_search(log, b"[bc", True) == [3]
    assert naive_search(log, b"\xe1bc", True) == []
    assert naive_search(log, b"\xc1BC", True) == [6]
    assert naive_search(log, b"abc", True, lo=1) == [2]
    assert FOLD[0x40] == 0x40 and FOLD[0x5B] == 0x5B and FOLD[0xC1] == 0xC1
    assert FOLD[0x41] == 0x61 and FOLD[0x5A] == 0x7A


def test_cpu_search_random_texts():
    run_random_texts("cpu")


def test_cpu_search_planted_at_every_chunk_phase():
    run_planted("cpu")


def test_cpu_search_many_matches_in_one_message():
    run_many_matches("cpu")


def test_cpu_search_log_longer_than_gpu_ring():
    run_wrap("cpu")


def test_cpu_search_status():
    run_status("cpu")


@pytest.mark.parametrize("via", ["batch", "device"])
def test_cpu_content_len_clamp(via):
    run_clamp("cpu", via)


def test_cpu_query():
    run_filter("cpu", 5600)


# ---------------------------------------------------------------------------
# GPU: k_search<P> and k_filter against the naive references
# ---------------------------------------------------------------------------


@pytest.mark.gpu
def test_gpu_search_random_texts():
    run_random_texts("gpu")


@pytest.mark.gpu
def test_gpu_search_planted_at_every_chunk_phase():
    run_planted("gpu")


@pytest.mark.gpu
def test_gpu_search_needle_length_bounds():
    log, eng = [], make_engine("gpu")
    try:
        send(eng, log, [Msg(b"a" * 64, 64)])
        for bad in (b"", b"a" * 257):
            with pytest.raises(ValueError):
                eng.q.search_range(0, 1, bad, False, 8192)
            with pytest.raises(ValueError):
                eng.search(bad, True, 10)
        assert eng.search(b"a" * 64, True, 10).tolist() == [0]
        assert eng.search(b"a" * 65, True, 10).tolist() == []
        assert eng.search(b"a" * 256, True, 10).tolist() == []
    finally:
        close(eng)


@pytest.mark.gpu
def test_gpu_search_many_matches_in_one_message():
    run_many_matches("gpu")


@pytest.mark.gpu
def test_gpu_search_ring_wrap():
    run_wrap("gpu")


@pytest.mark.gpu
def test_gpu_search_status():
    run_status("gpu")


PIPE_NEEDLES = [(b"b", False), (b"B", True), (b"bR", False), (b"Br", True),
                (b"Br`", False), (b"bR`", True), (b"@", True)]
PIPE_D = (-1, 0, 1, 63, 64, 65, 255, 256, 257)


def pipe_log(slot_bytes, n):
    return random_msgs(np.random.default_rng(21), n, slot_bytes,
                       [b"bR", b"Br`", b"r@B"], plants=(0, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("loads", [2, 4, 8])
def test_gpu_search_every_exit_of_the_pipelined_loop(loads):
    """One chunk per slot and one block: a lane runs the pipelined loop k
    times and then the tail loop, and n = loads*256*k + d puts the end of
    the segment at every place relative to a group and to the wave and
    block edges inside it."""
    n_max = loads * 256 * 2 + 257
    log = []
    eng = make_engine("gpu", slot_bytes=16, num_slots=8192)
    try:
        send(eng, log, pipe_log(16, n_max))
        assert any(naive_search(log, nd, fold) for nd, fold in PIPE_NEEDLES)
        for k in (0, 1, 2):
            for d in PIPE_D:
                n = loads * 256 * k + d
                if n <= 0:
                    continue
                for nd, fold in PIPE_NEEDLES:
                    raw = eng.q.search_range(0, n, nd, fold, 8192, blocks=1,
                                             loads=loads)
                    want = naive_search(log, nd, fold, 0, n)
                    # one chunk per message: a seq comes at most once
                    assert np.sort(raw).tolist() == sorted(want), (k, d, nd)
        # two blocks: a group is 2*256*loads chunks
        for n in (loads * 512 - 1, loads * 512, loads * 512 + 257, n_max):
            for nd, fold in PIPE_NEEDLES:
                raw = eng.q.search_range(0, n, nd, fold, 8192, blocks=2,
                                         loads=loads)
                assert np.sort(raw).tolist() == sorted(
                    naive_search(log, nd, fold, 0, n)), (n, nd)
        # a window that starts inside the segment
        raw = eng.q.search_range(300, n_max - 5, b"b", True, 8192, blocks=1,
                                 loads=loads)
        assert np.sort(raw).tolist() == sorted(
            naive_search(log, b"b", True, 300, n_max - 5))
    finally:
        close(eng)


@pytest.mark.gpu
@pytest.mark.parametrize("loads", [2, 4, 8])
def test_gpu_search_pipelined_loop_four_chunks_per_slot(loads):
    """slot_bytes=64: chunk index / chunks-per-slot is no identity, and a
    message may be reported once per chunk."""
    per = loads * 256 // 4  # messages per group at blocks=1
    n_max = 4 * per + 65
    log = []
    eng = make_engine("gpu", slot_bytes=64, num_slots=4096)
    try:
        send(eng, log, pipe_log(64, n_max))
        for blocks in (1, 2):
            for n in (per - 1, per, per + 1, per + 16, 2 * per, 2 * per + 1,
                      n_max):
                n *= blocks if n != n_max else 1
                n = min(n, n_max)
                for nd, fold in PIPE_NEEDLES:
                    raw = eng.q.search_range(0, n, nd, fold, 8192,
                                             blocks=blocks, loads=loads)
                    assert np.unique(raw).tolist() == sorted(
                        naive_search(log, nd, fold, 0, n)), (blocks, n, nd)
    finally:
        close(eng)


@pytest.mark.gpu
@pytest.mark.parametrize("via", ["batch", "device"])
def test_gpu_content_len_clamp(via):
    run_clamp("gpu", via)


@pytest.mark.gpu
def test_gpu_filter():
    run_filter("gpu", 3000)


@pytest.mark.gpu
def test_gpu_filter_wrapped_ring():
    """4096 live seqs in two segments: at blocks=1 every thread of
    k_filter takes 16 turns of the grid-stride loop."""
    run_filter("gpu", 5600, num_slots=4096)


@pytest.mark.gpu
def test_gpu_scan_argument_checks():
    log, eng = [], make_engine("gpu")
    try:
        send(eng, log, random_log()[:300])
        nd = b"bR"
        want = sorted(naive_search(log, nd, True))
        assert want
        with pytest.raises(ValueError):
            eng.q.search_range(0, 300, nd, True, 8192, loads=3)
        assert np.unique(
            eng.q.search_range(0, 300, nd, True, 8192)).tolist() == want
        with pytest.raises(ValueError):
            eng.q.search_range(0, 300, nd, True, 8192, blocks=-1)
        assert np.unique(
            eng.q.search_range(0, 300, nd, True, 8192)).tolist() == want
        for loads in (1, 16, -2):
            with pytest.raises(ValueError):
                eng.q.search_range(0, 300, nd, True, 8192, loads=loads)
        # an empty window refuses them all the same
        with pytest.raises(ValueError):
            eng.q.search_range(300, 300, nd, True, 8192, loads=3)
        with pytest.raises(ValueError):
            query_range(eng, 0, 300, blocks=-1, sender=3)
        assert np.sort(query_range(eng, 0, 300, sender=3)).tolist() == sorted(
            naive_query(log, sender=3))
        assert eng.search(nd, False, 1000).tolist() == want[::-1]
    finally:
        close(eng)
