// The core queue kernels: tick, enqueue, fan-out, dequeue, host gathers,
// filter, search, unread, statuses, batch load balancer, all-to-all pack.
#pragma once

#include "swarmq_util.h"

// Enqueue, split in two for occupancy: k_enqueue_meta does the
// per-message bookkeeping THREAD-per-message (header write, status ack,
// counters, inbox append — 64 messages per wave instead of one message
// per wave with 63 idle lanes), k_enqueue_payload streams the payload
// bytes WAVE-per-message (64 lanes x 16 B = 1 KiB per vector round).
// Both read the same staged records; they are independent and the
// dequeue that needs both runs later on the same stream.
// Graph-tick prologue: advance the device-side tail and publish this
// tick's (base, evict) pair for the captured kernels to read.
__global__ void k_tick_begin(u64 *__restrict__ base_evict,
                             ull *__restrict__ tail, int n, u64 num_slots) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const u64 base = *tail;
    base_evict[0] = base;
    const u64 cnt = base + (u64)n;
    base_evict[1] = cnt > num_slots ? cnt - num_slots : 0;
    *tail = cnt;
  }
}

__global__ void k_enqueue_meta(const Rec *__restrict__ stage, int n,
                               u64 base_seq, const u64 *__restrict__ dyn,
                               Rec *__restrict__ hdr,
                               u32 *__restrict__ status,
                               u64 *__restrict__ inbox,
                               ull *__restrict__ inbox_wpos,
                               const ull *__restrict__ inbox_rpos,
                               ull *__restrict__ by_type,
                               ull *__restrict__ by_status,
                               ull *__restrict__ sent,
                               u64 *__restrict__ bcast_list,
                               u32 *__restrict__ bcast_count,
                               ull *__restrict__ dropped, QueueGeom g) {
  // per-block histograms: one global atomic per bin per block
  __shared__ u32 h_type[N_TYPES];
  __shared__ u32 h_msgs;
  __shared__ u32 h_failed;
  if (threadIdx.x < N_TYPES)
    h_type[threadIdx.x] = 0;
  if (threadIdx.x == N_TYPES)
    h_msgs = 0;
  if (threadIdx.x == N_TYPES + 1)
    h_failed = 0;
  __syncthreads();

  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const Rec r = stage[i];
    const u64 seq = (dyn ? dyn[0] : base_seq) + (u64)i;
    const u32 slot = (u32)(seq % g.num_slots);

    // error lane (reference _errors topic analog, "swarmdb/
    // main.py":260-273, 501-519): malformed records park FAILED
    const bool bad =
        r.type >= N_TYPES || r.priority > 3 ||
        r.payload_len > g.slot_bytes ||
        (r.receiver != BROADCAST && r.receiver >= g.max_agents) ||
        r.sender >= g.max_agents ||
        (r.vis_mode != VIS_ALL && r.bitmap != NO_BITMAP &&
         r.bitmap >= g.num_bitmaps);
    Rec h = r;
    h.payload_off = (u64)slot * g.slot_bytes;
    if (bad) {
      h.payload_len = 0;
      h.content_len = 0;
      hdr[slot] = h;
      status[slot] = ST_FAILED;
      atomicAdd(&h_failed, 1u);
    } else {
      // the search window is a prefix of the payload: a content_len the
      // host never saw must not reach past the bytes this record wrote
      // (into the slot's previous occupant, or the next slot)
      h.content_len = min(h.content_len, h.payload_len);
      hdr[slot] = h;
      status[slot] = ST_DELIVERED;
      atomicAdd(&h_type[r.type], 1u);
      atomicAdd(&h_msgs, 1u);
      atomicAdd(&sent[r.sender], 1ull);
      if (r.receiver == BROADCAST) {
        u32 bi = atomicAdd(bcast_count, 1u);
        bcast_list[bi] = seq;
      } else {
        ull pos = atomicAdd(&inbox_wpos[r.receiver], 1ull);
        // ring overfill: a slow consumer's unexamined entry is about to
        // be overwritten — count the loss instead of hiding it (exposed
        // via stats; the CPU engine's inboxes are unbounded, so this is
        // the one place GPU delivery can drop)
        if (pos - inbox_rpos[r.receiver] >= (ull)g.inbox_capacity)
          atomicAdd(dropped, 1ull);
        inbox[(u64)r.receiver * g.inbox_capacity + (pos % g.inbox_capacity)] =
            seq;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < N_TYPES && h_type[threadIdx.x])
    atomicAdd(&by_type[threadIdx.x], (ull)h_type[threadIdx.x]);
  if (threadIdx.x == N_TYPES && h_msgs)
    atomicAdd(&by_status[ST_DELIVERED], (ull)h_msgs);
  if (threadIdx.x == N_TYPES + 1 && h_failed)
    atomicAdd(&by_status[ST_FAILED], (ull)h_failed);
}

__global__ void k_enqueue_payload(const Rec *__restrict__ stage,
                                  const u8 *__restrict__ stage_pay, int n,
                                  u64 base_seq, const u64 *__restrict__ dyn,
                                  u8 *__restrict__ payload, QueueGeom g) {
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (wave >= n)
    return;
  const u64 payload_off = stage[wave].payload_off;
  const u32 payload_len = stage[wave].payload_len;
  if (payload_len == 0 || payload_len > g.slot_bytes)
    return;
  const u64 seq = (dyn ? dyn[0] : base_seq) + (u64)wave;
  const u32 slot = (u32)(seq % g.num_slots);
  copy_chunks(stage_pay + payload_off, payload + (u64)slot * g.slot_bytes,
              payload_len, lane);
}

// Broadcast fan-out: one thread per agent appends the batch's broadcast
// seqs to its own inbox ring — no atomics (each thread owns its agent,
// and kernels are stream-serialized). Replaces the reference's Python
// loop over all inboxes (reference "swarmdb/ main.py":457-463).
__global__ void k_fanout(const u64 *__restrict__ bcast_list,
                         const u32 *__restrict__ bcast_count,
                         const u32 *__restrict__ active,
                         const Rec *__restrict__ hdr,
                         const u64 *__restrict__ bitmaps,
                         const u32 *__restrict__ bitmap_epochs,
                         u64 *__restrict__ inbox, ull *__restrict__ inbox_wpos,
                         const ull *__restrict__ inbox_rpos,
                         ull *__restrict__ dropped, QueueGeom g) {
  const u32 a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= g.max_agents || !active[a])
    return;
  const u32 nb = *bcast_count;
  if (nb == 0)
    return;
  ull pos = inbox_wpos[a];
  const ull rpos = inbox_rpos[a];
  ull ndrop = 0;
  u64 *ib = inbox + (u64)a * g.inbox_capacity;
  for (u32 i = 0; i < nb; ++i) {
    const u64 seq = bcast_list[i];
    const Rec &h = hdr[seq % g.num_slots]; // uniform per i, L2-cached
    if (h.vis_mode == VIS_GROUP) {
      // group fan-out: only member inboxes get the entry; a recycled
      // bitmap (epoch mismatch) means membership is unknowable — skip
      // rather than misdeliver
      if (h.bitmap == NO_BITMAP ||
          bitmap_epochs[h.bitmap] != h.bitmap_epoch ||
          !((bitmaps[(u64)h.bitmap * g.bitmap_words + (a >> 6)] >>
             (a & 63)) & 1ull))
        continue;
    }
    if (pos - rpos >= (ull)g.inbox_capacity)
      ++ndrop; // ring overfill overwrites an unexamined entry
    ib[pos % g.inbox_capacity] = seq;
    ++pos;
  }
  inbox_wpos[a] = pos;
  if (ndrop)
    atomicAdd(dropped, ndrop);
}

// Dequeue: one 256-thread workgroup per polling agent. Drains the
// agent's carry buffer + fresh inbox window into LDS, applies the
// visibility filter on-device (reference's client-side filter at
// "swarmdb/ main.py":579-585 moved into the kernel — each message is
// touched O(recipients) times instead of O(agents)), bitonic-sorts the
// window (by seq for FIFO, or (3-priority)<<48|seq for priority mode —
// the priority-sort kernel of BASELINE config 3), marks the delivered
// prefix READ, and carries leftovers.
__global__ void __launch_bounds__(256)
    k_receive(const u32 *__restrict__ agents, int n_agents, int max_per_agent,
              int priority_mode, u64 evict_base,
              const u64 *__restrict__ dyn, const Rec *__restrict__ hdr,
              u32 *__restrict__ status, const u64 *__restrict__ inbox,
              ull *__restrict__ inbox_wpos, ull *__restrict__ inbox_rpos,
              u64 *__restrict__ carry, u32 *__restrict__ carry_n,
              const u64 *__restrict__ bitmaps,
              const u32 *__restrict__ bitmap_epochs,
              u64 *__restrict__ out_seqs,
              u32 *__restrict__ out_counts, ull *__restrict__ by_status,
              ull *__restrict__ received, QueueGeom g) {
  // dynamic LDS: [0..1] control words, [2..] the sort window (the
  // window size is a queue parameter — small dequeue windows keep many
  // blocks resident; the base stays 16-B aligned with no static
  // __shared__ objects, guide §6 G17)
  extern __shared__ __attribute__((aligned(16))) u64 smem[];
  u64 *keys = smem + 2;
  u32 *sh_valid = reinterpret_cast<u32 *>(smem);

  const int b = blockIdx.x;
  if (b >= n_agents)
    return;
  if (dyn)
    evict_base = dyn[1];
  const u32 a = agents[b];
  ull r = inbox_rpos[a];
  const ull w = inbox_wpos[a];
  const u32 nc = carry_n[a];
  const u32 room = g.recv_window - nc;
  ull avail = w - r;
  if (avail > (ull)g.inbox_capacity) {
    // ring overfilled since the last poll: the oldest (w - r - cap)
    // entries were overwritten (counted in `dropped` at append time) —
    // skip to the retained window instead of re-reading live slots as
    // stale duplicates
    r = w - (ull)g.inbox_capacity;
    avail = (ull)g.inbox_capacity;
  }
  const u32 fresh = (u32)(avail < (ull)room ? avail : (ull)room);
  const u32 total = nc + fresh;

  const u64 *ib = inbox + (u64)a * g.inbox_capacity;
  const u64 *cb = carry + (u64)a * g.recv_window;

  for (u32 i = threadIdx.x; i < total; i += blockDim.x) {
    const u64 seq =
        (i < nc) ? cb[i] : ib[(r + (i - nc)) % g.inbox_capacity];
    u64 key = KEY_INVALID;
    if (seq >= evict_base) {
      const u32 slot = (u32)(seq % g.num_slots);
      if (status[slot] != ST_DELETED) {
        const Rec h = hdr[slot];
        bool vis = true;
        if ((h.vis_mode == VIS_BITMAP || h.vis_mode == VIS_GROUP) &&
            h.bitmap != NO_BITMAP) {
          if (bitmap_epochs[h.bitmap] != h.bitmap_epoch) {
            // the pool slot was recycled since this message was sent:
            // the original visibility set is gone — hide the message
            // (exact semantics: never deliver against the wrong bitmap)
            vis = false;
          } else {
            const u64 wbits =
                bitmaps[(u64)h.bitmap * g.bitmap_words + (a >> 6)];
            vis = (wbits >> (a & 63)) & 1ull;
          }
        }
        if (vis)
          key = priority_mode ? prio_key(h.priority, seq) : seq;
      }
    }
    keys[i] = key;
  }
  u32 npad = 1;
  while (npad < total)
    npad <<= 1;
  if (total == 0)
    npad = 0;
  for (u32 i = threadIdx.x; i < npad; i += blockDim.x)
    if (i >= total)
      keys[i] = KEY_INVALID;
  __syncthreads();

  // bitonic sort ascending (invalid keys sink to the end)
  for (u32 k = 2; k <= npad; k <<= 1) {
    for (u32 j = k >> 1; j > 0; j >>= 1) {
      for (u32 i = threadIdx.x; i < npad; i += blockDim.x) {
        const u32 ixj = i ^ j;
        if (ixj > i) {
          const u64 x = keys[i], y = keys[ixj];
          const bool up = ((i & k) == 0);
          if ((x > y) == up) {
            keys[i] = y;
            keys[ixj] = x;
          }
        }
      }
      __syncthreads();
    }
  }

  if (threadIdx.x == 0) {
    u32 lo = 0, hi = npad;
    while (lo < hi) { // first INVALID = count of deliverable keys
      const u32 mid = (lo + hi) >> 1;
      if (keys[mid] == KEY_INVALID)
        hi = mid;
      else
        lo = mid + 1;
    }
    *sh_valid = lo;
  }
  __syncthreads();
  const u32 valid = *sh_valid;
  const u32 take = valid < (u32)max_per_agent ? valid : (u32)max_per_agent;

  for (u32 i = threadIdx.x; i < take; i += blockDim.x) {
    const u64 seq =
        priority_mode ? (keys[i] & 0xFFFFFFFFFFFFull) : keys[i];
    out_seqs[(u64)b * (u32)max_per_agent + i] = seq;
    const u32 slot = (u32)(seq % g.num_slots);
    // DELIVERED -> READ transition; CAS because two agents may read the
    // same broadcast slot concurrently (status is global, as in the
    // reference)
    const u32 old = atomicCAS(&status[slot], ST_DELIVERED, ST_READ);
    if (old == ST_DELIVERED) {
      atomicAdd(&by_status[ST_READ], 1ull);
      atomicAdd(&by_status[ST_DELIVERED], (ull)(-1ll));
    }
  }

  const u32 rest = valid - take;
  u64 *cbw = carry + (u64)a * g.recv_window;
  for (u32 i = threadIdx.x; i < rest; i += blockDim.x) {
    const u64 key = keys[take + i];
    cbw[i] = priority_mode ? (key & 0xFFFFFFFFFFFFull) : key;
  }
  if (threadIdx.x == 0) {
    carry_n[a] = rest;
    inbox_rpos[a] = r + fresh;
    out_counts[b] = take;
    if (take)
      atomicAdd(&received[a], (ull)take);
  }
}

// Gather delivered payloads straight from the dequeue output buffer
// (device-resident) into a dense D2H staging area — the delivery path
// never round-trips seqs through the host.
__global__ void k_gather_outbuf(const u64 *__restrict__ out_seqs,
                                const u32 *__restrict__ counts,
                                const u32 *__restrict__ offsets, int n_agents,
                                int K, int max_count,
                                const Rec *__restrict__ hdr,
                                const u8 *__restrict__ payload,
                                u8 *__restrict__ out_pay, u32 stride,
                                QueueGeom g) {
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int a = wave / max_count;
  const int i = wave % max_count;
  if (a >= n_agents || (u32)i >= counts[a])
    return;
  const u64 seq = out_seqs[(u64)a * K + i];
  const Rec h = hdr[seq % g.num_slots];
  u32 plen = h.payload_len;
  if (plen > stride)
    plen = stride;
  copy_chunks(payload + h.payload_off,
              out_pay + (u64)(offsets[a] + i) * stride, plen, lane);
}

// Gather message contents for the host (receive payload delivery, fetch,
// history spill): one wave per message, dense slot_bytes-strided output.
__global__ void k_gather(const u64 *__restrict__ seqs, int n,
                         const Rec *__restrict__ hdr,
                         const u32 *__restrict__ status,
                         const u8 *__restrict__ payload,
                         Rec *__restrict__ out_hdr,
                         u32 *__restrict__ out_status,
                         u8 *__restrict__ out_pay, u64 evict_base,
                         u32 out_stride, QueueGeom g) {
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (wave >= n)
    return;
  const u64 seq = seqs[wave];
  const u32 slot = (u32)(seq % g.num_slots);
  if (seq < evict_base) {
    if (lane == 0) {
      Rec z{};
      out_hdr[wave] = z;
      out_status[wave] = ST_DELETED;
    }
    return;
  }
  const Rec h = hdr[slot];
  u32 plen = h.payload_len;
  if (plen > out_stride)
    plen = out_stride;
  copy_chunks(payload + h.payload_off, out_pay + (u64)wave * out_stride, plen,
              lane);
  if (lane == 0) {
    out_hdr[wave] = h;
    out_status[wave] = status[slot];
  }
}

// Filtered scan over a seq range (query_messages engine, reference
// "swarmdb/ main.py":671-740): one thread per message, matches appended
// with a global atomic; the host sorts newest-first.
__global__ void k_filter(u64 lo, u64 hi, int f_sender, int f_receiver,
                         int f_type, int f_status, double after, double before,
                         u32 pred_mask, const Rec *__restrict__ hdr,
                         const u32 *__restrict__ status,
                         u64 *__restrict__ out, u32 *__restrict__ out_count,
                         u32 cap, QueueGeom g) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 seq = lo + blockIdx.x * blockDim.x + threadIdx.x; seq < hi;
       seq += stride) {
    const u32 slot = (u32)(seq % g.num_slots);
    const u32 st = status[slot];
    if (st == ST_DELETED)
      continue;
    const Rec h = hdr[slot];
    if ((pred_mask & 1u) && h.sender != (u32)f_sender)
      continue;
    if ((pred_mask & 2u) && h.receiver != (u32)f_receiver)
      continue;
    if ((pred_mask & 4u) && h.type != (u8)f_type)
      continue;
    if ((pred_mask & 8u) && st != (u32)f_status)
      continue;
    if ((pred_mask & 16u) && !(h.timestamp > after)) // exclusive bounds
      continue;
    if ((pred_mask & 32u) && !(h.timestamp < before))
      continue;
    const u32 i = atomicAdd(out_count, 1u);
    if (i < cap)
      out[i] = seq;
  }
}

// Substring search over message content (search_messages engine,
// reference "swarmdb/ main.py":742-781): one wave per message; lanes
// stride over candidate start positions; ASCII case-folding optional.
// The content window is payload[0:content_len] — metadata/ids never
// match.
__device__ __forceinline__ u8 fold_c(u8 c, int fold) {
  return (fold && c >= 'A' && c <= 'Z') ? (u8)(c | 0x20) : c;
}

// packed first-byte test: 0x80 in every byte of the result that equals
// the splat byte (the classic haszero trick on w ^ splat)
__device__ __forceinline__ u32 byte_eq_mask(u32 w, u32 splat) {
  const u32 x = w ^ splat;
  return (x - 0x01010101u) & ~x & 0x80808080u;
}

// compact the 0x80-bits of a byte_eq_mask result into 4 low bits
// (movemask): t*0x00204081 lands byte k's bit at position 28+k
__device__ __forceinline__ u32 movemask4(u32 t) {
  return (t * 0x00204081u) >> 28;
}

// Candidate verification (rare path): the chunk is still in REGISTERS
// (v) — build the per-byte first-char hitmask from it (no memory
// re-reads) and only the actual hit positions compare the needle tail
// against global memory (in L1/L2 — the wave just streamed it).
__device__ __forceinline__ void verify_chunk(
    u64 seq, u32 slot, u32 sub, const uint4 &v,
    const u8 *__restrict__ needle, int nlen, int fold,
    const Rec *__restrict__ hdr, const u32 *__restrict__ status,
    const u8 *__restrict__ payload, u64 *__restrict__ out,
    u32 *__restrict__ out_count, u32 cap, QueueGeom g) {
  const u8 n0 = fold_c(needle[0], fold);
  const u8 *bytes = reinterpret_cast<const u8 *>(&v);
  u32 hitmask = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j)
    hitmask |= (fold_c(bytes[j], fold) == n0) ? (1u << j) : 0u;
  if (hitmask == 0 || status[slot] == ST_DELETED)
    return;
  const Rec h = hdr[slot];
  const int nstart = (int)h.content_len - nlen + 1;
  const u8 *text = payload + (u64)slot * g.slot_bytes;
  const int base = (int)(sub << 4);
  bool found = false;
  while (hitmask && !found && nstart > 0) {
    const int j = __builtin_ctz(hitmask);
    hitmask &= hitmask - 1;
    const int p = base + j;
    if (p >= nstart)
      continue;
    bool m = true;
    for (int q = 1; q < nlen; ++q) {
      if (fold_c(text[p + q], fold) != fold_c(needle[q], fold)) {
        m = false;
        break;
      }
    }
    found = m;
  }
  if (found) {
    const u32 i = atomicAdd(out_count, 1u);
    if (i < cap)
      out[i] = seq;
  }
}

// Linear-streaming scan over ONE contiguous slot segment. The slot
// region of a seq range is always at most TWO contiguous byte ranges
// (the ring wraps at most once), so the host splits the scan and each
// launch is a PURE linear walk: addr = seg + 16*ci — the access shape
// that measures 6.2 TB/s on this chip (csrc/bench_membw.hip).
//
// Cross-group software pipeline: group k+1's P loads are ISSUED before
// group k's screens/verifies run, so the screen work (a tiered
// first-char / adjacent-pair filter whose cost the wave pays whenever
// any lane has a candidate, ~16% per lane on random text) overlaps the
// loads' HBM round-trip instead of serializing against it. A
// wave-aggregated two-phase variant (ballot-recorded candidates,
// lane-parallel verify) measured WORSE (2.0 TB/s) — its per-ballot
// phase-B overhead exceeded the screen it saved; see profiles/.
template <int P>
__global__ void k_search(const u8 *__restrict__ seg, u64 nchunks, u64 seq0,
                         u32 slot0, const u8 *__restrict__ needle, int nlen,
                         int fold, const Rec *__restrict__ hdr,
                         const u32 *__restrict__ status,
                         const u8 *__restrict__ payload,
                         u64 *__restrict__ out, u32 *__restrict__ out_count,
                         u32 cap, QueueGeom g) {
  const u8 nf = fold_c(needle[0], fold);
  const u32 s1 = (u32)nf * 0x01010101u;
  const bool two = fold && nf >= 'a' && nf <= 'z';
  const u32 s2 = two ? s1 - 0x20202020u : s1; // upper-case splat
  // second-byte screen (nlen >= 2): a chunk is only a candidate if it
  // also contains the needle's SECOND char (or its first-char hit is in
  // the final byte, whose successor lives in the next chunk)
  const u8 ng = nlen >= 2 ? fold_c(needle[1], fold) : 0;
  const u32 t1 = (u32)ng * 0x01010101u;
  const bool two2 = fold && ng >= 'a' && ng <= 'z';
  const u32 t2 = two2 ? t1 - 0x20202020u : t1;
  const u32 cps = g.slot_bytes >> 4; // chunks per slot

  // three-tier screen, costed for wave-level issue (a divergent branch
  // is paid whenever ANY lane takes it):
  //   tier 1 (every chunk): does the chunk contain the first char at
  //     all — 4-8 haszero tests;
  //   tier 2 (~16% of chunks on random text): EXACT positional check
  //     that some first-char hit is immediately followed by the second
  //     char (movemask + shifted AND) — not just "second char appears
  //     somewhere";
  //   tier 3 (~needle-density of chunks, ~0.2% random): full verify
  //     with header/status loads.
  // The approximate contains-n1 screen left ~2.4% of chunks entering
  // tier 3, whose divergent dependent loads cost ~1 TB/s (measured,
  // profiles/r02 search notes).
  auto test16 = [&](const uint4 &v) -> bool {
    u32 e0 = byte_eq_mask(v.x, s1), e1 = byte_eq_mask(v.y, s1),
        e2 = byte_eq_mask(v.z, s1), e3 = byte_eq_mask(v.w, s1);
    if (two) {
      e0 |= byte_eq_mask(v.x, s2);
      e1 |= byte_eq_mask(v.y, s2);
      e2 |= byte_eq_mask(v.z, s2);
      e3 |= byte_eq_mask(v.w, s2);
    }
    if ((e0 | e1 | e2 | e3) == 0)
      return false;
    if (nlen < 2)
      return true;
    // tier 1.5 (issued at the first-char rate, ~16%): does the SECOND
    // char appear at all — 4 more haszero tests gate the pricier
    // positional tier down to ~P(char)^2 issue rate
    u32 f0 = byte_eq_mask(v.x, t1), f1 = byte_eq_mask(v.y, t1),
        f2 = byte_eq_mask(v.z, t1), f3 = byte_eq_mask(v.w, t1);
    if (two2) {
      f0 |= byte_eq_mask(v.x, t2);
      f1 |= byte_eq_mask(v.y, t2);
      f2 |= byte_eq_mask(v.z, t2);
      f3 |= byte_eq_mask(v.w, t2);
    }
    if ((f0 | f1 | f2 | f3) == 0)
      return (e3 & 0x80000000u) != 0; // last-byte hit: pair spans chunks
    const u32 m0 = movemask4(e0) | (movemask4(e1) << 4) |
                   (movemask4(e2) << 8) | (movemask4(e3) << 12);
    const u32 m1 = movemask4(f0) | (movemask4(f1) << 4) |
                   (movemask4(f2) << 8) | (movemask4(f3) << 12);
    // bit 15 (chunk's last byte) always passes: its successor lives in
    // the next chunk and is checked by the verify's tail compare
    return (m0 & ((m1 >> 1) | 0x8000u)) != 0;
  };
  auto verify = [&](u64 ci, const uint4 &v) {
    // rare path: division happens HERE, never in the hot loop
    const u64 q = ci / cps;
    const u32 sub = (u32)(ci - q * cps);
    verify_chunk(seq0 + q, slot0 + (u32)q, sub, v, needle, nlen, fold,
                 hdr, status, payload, out, out_count, cap, g);
  };

  const u64 stride = (u64)gridDim.x * blockDim.x;
  const uint4 *src = reinterpret_cast<const uint4 *>(seg);
  const u64 group = (u64)P * stride;
  u64 ci = (u64)blockIdx.x * blockDim.x + threadIdx.x;

  uint4 v[P];
  bool have = ci + (u64)(P - 1) * stride < nchunks;
  if (have) {
#pragma unroll
    for (int p = 0; p < P; ++p)
      v[p] = src[ci + (u64)p * stride];
  }
  while (have) {
    const u64 nci = ci + group;
    const bool next = nci + (u64)(P - 1) * stride < nchunks;
    uint4 vn[P];
    if (next) {
#pragma unroll
      for (int p = 0; p < P; ++p) // next group's loads fly NOW,
        vn[p] = src[nci + (u64)p * stride]; // over this group's screens
    }
#pragma unroll
    for (int p = 0; p < P; ++p)
      if (test16(v[p]))
        verify(ci + (u64)p * stride, v[p]);
#pragma unroll
    for (int p = 0; p < P; ++p)
      v[p] = vn[p];
    ci = nci;
    have = next;
  }
  for (; ci < nchunks; ci += stride) {
    const uint4 w = src[ci];
    if (test16(w))
      verify(ci, w);
  }
}

// Unread count: one workgroup per agent scans its retained inbox window
// for entries whose global status is DELIVERED (reference "swarmdb/
// main.py":1026-1047).
__global__ void k_unread(const u32 *__restrict__ agents, int n_agents,
                         u64 evict_base, const u32 *__restrict__ status,
                         const u64 *__restrict__ inbox,
                         const ull *__restrict__ inbox_wpos,
                         u32 *__restrict__ out, QueueGeom g) {
  __shared__ u32 cnt;
  const int b = blockIdx.x;
  if (b >= n_agents)
    return;
  if (threadIdx.x == 0)
    cnt = 0;
  __syncthreads();
  const u32 a = agents[b];
  const ull w = inbox_wpos[a];
  const ull start = w > g.inbox_capacity ? w - g.inbox_capacity : 0;
  const u64 *ib = inbox + (u64)a * g.inbox_capacity;
  u32 local = 0;
  for (ull i = start + threadIdx.x; i < w; i += blockDim.x) {
    const u64 seq = ib[i % g.inbox_capacity];
    if (seq < evict_base)
      continue;
    if (status[seq % g.num_slots] == ST_DELIVERED)
      ++local;
  }
  atomicAdd(&cnt, local);
  __syncthreads();
  if (threadIdx.x == 0)
    out[b] = cnt;
}

// Batched status gather (no payload traffic). A seq outside the live
// window [evict_base, count) reads DELETED, as get_status has it: its
// slot holds another message, or none yet.
__global__ void k_statuses(const u64 *__restrict__ seqs, int n,
                           u64 evict_base, u64 count,
                           const u32 *__restrict__ status,
                           u32 *__restrict__ out, QueueGeom g) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const u64 s = seqs[i];
  out[i] = (s < evict_base || s >= count) ? ST_DELETED
                                          : status[s % g.num_slots];
}

// Batched status mutation with counter upkeep (history load restore).
// An evicted seq is skipped (its slot belongs to a newer message), so is
// one never assigned, as in k_ack_device; a tombstone IS overwritten.
__global__ void k_set_statuses(const u64 *__restrict__ seqs,
                               const u32 *__restrict__ new_status, int n,
                               u64 evict_base, u64 count,
                               u32 *__restrict__ status,
                               ull *__restrict__ by_status, QueueGeom g) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const u64 s = seqs[i];
  if (s < evict_base || s >= count)
    return;
  swap_status(status, by_status, (u32)(s % g.num_slots), new_status[i]);
}

// Status mutation with counter upkeep (mark processed / admin status
// updates / delete tombstones). Same skip rule as k_set_statuses.
__global__ void k_set_status(u64 seq, u32 new_status, u64 evict_base,
                             u64 count, u32 *__restrict__ status,
                             ull *__restrict__ by_status, QueueGeom g) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    if (seq < evict_base || seq >= count)
      return;
    swap_status(status, by_status, (u32)(seq % g.num_slots), new_status);
  }
}

// Least-loaded dispatch (BASELINE config 5): one wavefront holds all
// backend loads in registers; each request is an exact sequential
// argmin via a 64-lane shuffle min-reduce, then the winner's load is
// bumped — the CDNA4 reduction-kernel mechanism the reference never
// implemented (SURVEY.md §2.2 "LLM load balancing").
__global__ void k_lb_batch(int requests, int n_backends,
                           ull *__restrict__ loads,
                           u32 *__restrict__ choices) {
  const int lane = threadIdx.x;
  if (lane >= 64)
    return;
  long long my = (lane < n_backends) ? (long long)loads[lane]
                                     : 0x7FFFFFFFFFFFFFFFll;
  for (int r = 0; r < requests; ++r) {
    long long v = my;
    int li = lane;
    for (int o = 32; o > 0; o >>= 1) {
      const long long ov = __shfl_down(v, o, 64);
      const int ol = __shfl_down(li, o, 64);
      if (ov < v || (ov == v && ol < li)) {
        v = ov;
        li = ol;
      }
    }
    li = __shfl(li, 0, 64);
    if (lane == li)
      ++my;
    if (lane == 0 && choices != nullptr)
      choices[r] = (u32)li;
  }
  if (lane < n_backends)
    loads[lane] = (ull)my;
}

// Pack payload instances into an all-to-all send buffer (cross-GPU
// routing over xGMI, BASELINE config 4): one wave per instance, 16-B
// chunks. Offsets are host-computed (stable, no atomics).
__global__ void k_pack(const u8 *__restrict__ src_pay,
                       const u64 *__restrict__ src_off,
                       const u64 *__restrict__ dst_off,
                       const u32 *__restrict__ lens, int n,
                       u8 *__restrict__ out) {
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (wave >= n)
    return;
  copy_chunks(src_pay + src_off[wave], out + dst_off[wave], lens[wave], lane);
}

__global__ void k_add_load(int idx, long long delta, ull *__restrict__ loads) {
  if (threadIdx.x == 0 && blockIdx.x == 0)
    atomicAdd(&loads[idx], (ull)delta);
}
