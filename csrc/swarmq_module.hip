// swarmq_module.hip — MI355X-native message-queue engine.
//
// HBM-resident MPMC slot ring + per-agent inbox rings with hand-written
// CDNA4 HIP kernels (gfx950): wavefront-cooperative enqueue (64 lanes x
// 16 B = 1 KiB per copy round), broadcast fan-out, LDS-bitonic priority
// dequeue, filter/search scans, and a wavefront-shuffle least-loaded
// reduction for LLM backend dispatch.
//
// This is the native replacement for the reference's librdkafka/Kafka
// tier (reference "swarmdb/ main.py":192-207, 334-345, 466-484, 553-588;
// SURVEY.md §2.4). All kernels run on one HIP stream per queue, so
// cross-kernel visibility is stream-ordered — no inter-workgroup
// release/acquire protocol is needed inside a launch (each workgroup
// owns disjoint state: a message, or an agent).
//
// Build: hipcc --offload-arch=gfx950 (see setup.py) — no CUDA paths, no
// hipify, no Triton.

#include <hip/hip_runtime.h>

#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "swarmq_common.h"

namespace py = pybind11;
using namespace swarmq;

#define HIP_CHECK(expr)                                                        \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) {                                                    \
      throw std::runtime_error(std::string("HIP error at " __FILE__ ":") +     \
                               std::to_string(__LINE__) + ": " +               \
                               hipGetErrorString(_e));                         \
    }                                                                          \
  } while (0)

using ull = unsigned long long;

// multi-threaded host memcpy for large staging copies (a single-threaded
// 16 MB memcpy at ~12 GB/s would cost more than the H2D DMA it feeds)
#include <thread>
static void par_memcpy(void *dst, const void *src, size_t n) {
  constexpr size_t kCut = 2u << 20;
  if (n < kCut) {
    std::memcpy(dst, src, n);
    return;
  }
  const int nt = 4;
  std::thread ts[nt];
  const size_t chunk = (n + nt - 1) / nt;
  for (int t = 0; t < nt; ++t) {
    const size_t off = (size_t)t * chunk;
    const size_t len = off < n ? std::min(chunk, n - off) : 0;
    ts[t] = std::thread([=] {
      if (len)
        std::memcpy((char *)dst + off, (const char *)src + off, len);
    });
  }
  for (auto &t : ts)
    t.join();
}

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------

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
  const uint4 *src =
      reinterpret_cast<const uint4 *>(stage_pay + payload_off);
  uint4 *dst =
      reinterpret_cast<uint4 *>(payload + (u64)slot * g.slot_bytes);
  const u32 nchunk = (payload_len + 15u) >> 4;
  for (u32 c = lane; c < nchunk; c += 64)
    dst[c] = src[c];
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
  const uint4 *src = reinterpret_cast<const uint4 *>(payload + h.payload_off);
  uint4 *dst = reinterpret_cast<uint4 *>(
      out_pay + (u64)(offsets[a] + i) * stride);
  u32 plen = h.payload_len;
  if (plen > stride)
    plen = stride;
  const u32 nchunk = (plen + 15u) >> 4;
  for (u32 c = lane; c < nchunk; c += 64)
    dst[c] = src[c];
}

// Device-resident delivery, step 1: exclusive prefix sum of the dequeue
// counts, offsets[0..n] with offsets[n] = total. One 256-thread
// workgroup: a 64-lane shuffle scan per wave, the four wave totals
// combined through LDS, tiles of 256 chained by a running total (every
// thread keeps the same copy of it, so no broadcast is needed). Replaces
// the host-side cumsum of deliver_outbuf — the counts never leave HBM.
__global__ void __launch_bounds__(256)
    k_scan_counts(const u32 *__restrict__ counts, int n,
                  u32 *__restrict__ offsets) {
  // dynamic LDS: the four wave totals of the current tile
  extern __shared__ __attribute__((aligned(16))) u32 scan_wave_tot[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  u32 running = 0;
  for (int base = 0; base < n; base += 256) {
    const int i = base + (int)threadIdx.x;
    const u32 c = (i < n) ? counts[i] : 0u;
    u32 v = c; // inclusive scan within the wave
    for (int d = 1; d < 64; d <<= 1) {
      const u32 t = __shfl_up(v, d, 64);
      if (lane >= d)
        v += t;
    }
    if (lane == 63)
      scan_wave_tot[wave] = v;
    __syncthreads();
    u32 before = 0, tile = 0;
    for (int w = 0; w < 4; ++w) {
      const u32 t = scan_wave_tot[w];
      if (w < wave)
        before += t;
      tile += t;
    }
    if (i < n)
      offsets[i] = running + before + v - c;
    running += tile;
    __syncthreads(); // the next tile overwrites the wave totals
  }
  if (threadIdx.x == 0)
    offsets[n] = running;
}

// Byte mask of the 32-bit word that starts at byte `first` of a 16-B
// chunk whose first `rem` bytes are live (little-endian).
__device__ inline u32 tail_mask(u32 rem, u32 first) {
  if (rem >= first + 4)
    return ~0u;
  if (rem <= first)
    return 0u;
  return (1u << (8 * (rem - first))) - 1u;
}

// Device-resident delivery, step 2: blockIdx.x is the polled agent (the
// k_receive grid), and the four waves of a 256-thread workgroup stride
// over that agent's delivered messages, writing packed rows
// r = offsets[b] + i into caller-provided device buffers. With many
// agents and small counts one workgroup per agent has no idle waves;
// with few agents and a deep inbox (one agent draining 4096 x 1 KB
// through a single workgroup: a 1.9 ms tick, against 0.59 ms now) the
// host adds gridDim.y workgroups per agent that interleave over the
// same messages, and the ones past the agent's count exit at once (see
// profiles/device_delivery.md). Unlike the D2H gathers above,
// every row is fully defined: the last 16-B chunk is masked at
// payload_len (a slot reused after ring wrap still holds the previous
// occupant's bytes there) and the rest of the row is zero-filled. The
// header is rebased so payload_off indexes the delivered payload tensor.
__global__ void __launch_bounds__(256)
    k_deliver_device(const u64 *__restrict__ out_seqs,
                     const u32 *__restrict__ counts,
                     const u32 *__restrict__ offsets, int n_agents, int K,
                     const Rec *__restrict__ hdr,
                     const u8 *__restrict__ payload,
                     u8 *__restrict__ out_pay, uint4 *__restrict__ out_hdr,
                     long long *__restrict__ out_seq,
                     int *__restrict__ out_len, int *__restrict__ out_row,
                     u32 stride, QueueGeom g) {
  const int b = blockIdx.x;
  if (b >= n_agents)
    return;
  const u32 lane = threadIdx.x & 63;
  const u32 wave = threadIdx.x >> 6;
  const u32 cnt = counts[b];
  const u32 off = offsets[b];
  const u32 row_chunks = stride >> 4;
  for (u32 i = blockIdx.y * 4 + wave; i < cnt; i += 4 * gridDim.y) {
    const u64 seq = out_seqs[(u64)b * (u32)K + i];
    const Rec h = hdr[seq % g.num_slots];
    const u64 r = (u64)off + i;
    const u32 plen = h.payload_len < stride ? h.payload_len : stride;
    const u32 full = plen >> 4; // whole 16-B chunks
    const u32 rem = plen & 15u; // live bytes of the chunk after them
    const uint4 *src =
        reinterpret_cast<const uint4 *>(payload + h.payload_off);
    uint4 *dst = reinterpret_cast<uint4 *>(out_pay + r * stride);
    for (u32 c = lane; c < row_chunks; c += 64) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (c < full) {
        v = src[c];
      } else if (c == full && rem) {
        v = src[c];
        // keep bytes [0, rem) of the chunk: word w holds bytes 4w..4w+3
        v.x &= tail_mask(rem, 0);
        v.y &= tail_mask(rem, 4);
        v.z &= tail_mask(rem, 8);
        v.w &= tail_mask(rem, 12);
      }
      dst[c] = v;
    }
    if (lane == 0) {
      Rec hh = h;
      hh.payload_off = r * stride;
      uint4 hv[3];
      __builtin_memcpy(hv, &hh, sizeof(Rec));
      uint4 *oh = out_hdr + r * 3;
      oh[0] = hv[0];
      oh[1] = hv[1];
      oh[2] = hv[2];
    } else if (lane == 1) {
      out_seq[r] = (long long)seq;
    } else if (lane == 2) {
      out_len[r] = (int)plen;
    } else if (lane == 3) {
      out_row[r] = b;
    }
  }
}

// ---- device-resident conversation context ----
//
// For every row r of a delivery: the newest `depth` messages of the log
// window [lo, hi) that the row's polled agent a and the row's sender s
// exchanged, in fixed slots (r, j), oldest first. Both kernels only READ
// queue state and run on stream_, which serialises every mutation of the
// log: stream order is the only synchronisation.
//
// The delivery's seqs / agent_row / headers may have been written to by
// the consumer, so they are values, never indices: agent_row is range-
// checked before it picks the polled agent, the sender is compared but
// never dereferenced, the seq is clamped into [0, count].

// Rows of a delivery one workgroup of k_context_find takes (CONTEXT_GROUP
// / 4 per wavefront). 4 — one row per wavefront — measured best on a
// 4096-row tick, where the call is bound by the serial chain of tiles a
// workgroup walks and not by the log reads the wider group saves; 16 is
// built too, for the comparison in profiles/device_context.md.
constexpr int CONTEXT_GROUP = 4;
constexpr int CONTEXT_GROUP_WIDE = 16;
constexpr int CONTEXT_TILE = 256;     // seqs per tile: one per thread
constexpr int CONTEXT_MAX_DEPTH = 64; // one lane per slot

// Step 1: which seqs. The workgroup walks the union window of its G rows
// from newest to oldest in tiles of 256 seqs. Thread t loads the first
// 16 B of one record (sender, receiver, type, vis_mode) plus its status
// word and leaves (sender, receiver, ok | type) in LDS; then every
// wavefront tests its G/4 rows against the tile, 64 entries per ballot,
// newest 64 first, each row under its own [lo, hi), and takes matches
// from the high end of the mask until the row holds `depth`. One
// 16-B-per-record pass is shared by G rows: where rows of one tick have
// nearly the same window, the log headers are read ~rows/G times, not
// rows times. The next tile's loads are issued before the current one is
// tested. Every branch around a barrier depends on block-uniform values
// only (top, wlo and the block-wide vote).
template <int G>
__global__ void __launch_bounds__(256)
    k_context_find(const long long *__restrict__ d_seqs,
                   const int *__restrict__ d_agent_row,
                   const u32 *__restrict__ d_headers, // 12 words per row
                   int total, const u32 *__restrict__ agents, int na,
                   int depth, long long lookback, int type_code,
                   u64 evict_base, u64 count, const Rec *__restrict__ hdr,
                   const u32 *__restrict__ status, int *__restrict__ out_counts,
                   long long *__restrict__ out_seqs,
                   int *__restrict__ out_lengths, QueueGeom g) {
  static_assert(G % 4 == 0 && G >= 4, "G/4 rows per wavefront");
  constexpr int RPW = G / 4;
  __shared__ u32 t_sender[CONTEXT_TILE];
  __shared__ u32 t_receiver[CONTEXT_TILE];
  __shared__ u32 t_ok_type[CONTEXT_TILE]; // bit 8: candidate; bits 0..7: type
  __shared__ u32 r_a[G], r_s[G];
  __shared__ long long r_lo[G], r_hi[G]; // lo >= hi: the row takes nothing
  __shared__ long long found[G][CONTEXT_MAX_DEPTH]; // newest first

  const int tid = (int)threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const long long row0 = (long long)blockIdx.x * G;

  if (tid < G) {
    const long long r = row0 + tid;
    long long lo = 0, hi = 0;
    u32 a = 0, s = 0;
    if (r < total) {
      const int b = d_agent_row[r];
      s = d_headers[r * 12];
      if (b >= 0 && b < na && s < g.max_agents) {
        a = agents[b];
        long long q = d_seqs[r];
        q = q < 0 ? 0 : q;
        hi = q > (long long)count ? (long long)count : q;
        lo = hi - lookback;
        if (lo < (long long)evict_base)
          lo = (long long)evict_base;
      }
    }
    r_a[tid] = a;
    r_s[tid] = s;
    r_lo[tid] = lo;
    r_hi[tid] = hi;
  }
  __syncthreads();

  // this wavefront's rows, and the block's union window
  u32 ra[RPW], rs[RPW];
  long long rlo[RPW], rhi[RPW];
  int rc[RPW];
#pragma unroll
  for (int i = 0; i < RPW; ++i) {
    ra[i] = r_a[wave * RPW + i];
    rs[i] = r_s[wave * RPW + i];
    rlo[i] = r_lo[wave * RPW + i];
    rhi[i] = r_hi[wave * RPW + i];
    rc[i] = 0;
  }
  long long wlo = 0, whi = 0;
  for (int i = 0; i < G; ++i) {
    const long long l = r_lo[i], h = r_hi[i];
    if (l < h) {
      wlo = (whi == 0 || l < wlo) ? l : wlo;
      whi = h > whi ? h : whi;
    }
  }

  // Thread tid's entry of the tile that ends at t_top (exclusive): seq
  // max(t_top - 256, wlo) + tid, as the raw record words and status (the
  // caller decodes them when it needs them, so the loads stay in
  // flight). One 64-bit modulo per tile; a loaded thread has tid <
  // t_top - tlo <= whi - evict_base <= num_slots, so one conditional
  // step wraps its slot. An entry outside the tile reads as DELETED.
  auto load_tile = [&](long long t_top, uint4 &v, u32 &st) {
    v = make_uint4(0u, 0u, 0u, 0u);
    st = ST_DELETED;
    if (t_top <= wlo)
      return;
    const long long tlo =
        t_top - CONTEXT_TILE > wlo ? t_top - CONTEXT_TILE : wlo;
    if (tlo + tid >= t_top)
      return;
    u32 slot = (u32)((u64)tlo % g.num_slots) + (u32)tid;
    if (slot >= g.num_slots)
      slot -= g.num_slots;
    v = *reinterpret_cast<const uint4 *>(hdr + slot);
    st = status[slot];
  };

  long long top = whi; // exclusive end of the next tile; whi == 0: no window
  uint4 v;
  u32 st;
  load_tile(top, v, st);
  while (top > wlo) {
    const long long tlo = top - CONTEXT_TILE > wlo ? top - CONTEXT_TILE : wlo;
    const u32 type = v.z & 0xFFu;
    const u32 vis = (v.z >> 16) & 0xFFu;
    const bool ok = st != ST_DELETED && st != ST_FAILED && vis == VIS_ALL &&
                    (type_code < 0 || type == (u32)type_code);
    t_sender[tid] = v.x;
    t_receiver[tid] = v.y;
    t_ok_type[tid] = (ok ? 0x100u : 0u) | type;
    __syncthreads();
    // the next (older) tile's loads fly while this one is tested
    load_tile(tlo, v, st);

    int open = 0; // a row of this wavefront may still take older seqs
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      if (rc[i] < depth && rlo[i] < rhi[i] && rhi[i] > tlo && rlo[i] < top) {
        for (int c = CONTEXT_TILE / 64 - 1; c >= 0 && rc[i] < depth; --c) {
          const int e = c * 64 + lane;
          const long long qe = tlo + e;
          const u32 es = t_sender[e], er = t_receiver[e];
          const bool m = (t_ok_type[e] & 0x100u) && qe >= rlo[i] &&
                         qe < rhi[i] && qe < top &&
                         ((es == rs[i] && er == ra[i]) ||
                          (es == ra[i] && er == rs[i]));
          const ull mask = __ballot(m);
          if (mask) {
            // matches above this lane come first (newest first)
            const int above =
                lane == 63 ? 0 : __popcll(mask >> (lane + 1));
            const int need = depth - rc[i];
            if (m && above < need)
              found[wave * RPW + i][rc[i] + above] = qe;
            const int got = __popcll(mask);
            rc[i] += got < need ? got : need;
          }
        }
      }
      if (rc[i] < depth && rlo[i] < rhi[i] && rlo[i] < tlo)
        open = 1;
    }
    top = tlo;
    // also the barrier that lets the next tile overwrite the LDS tile
    if (!__syncthreads_or(open))
      break;
  }
  __syncthreads(); // found[] of the last tile, for the lanes that write out

#pragma unroll
  for (int i = 0; i < RPW; ++i) {
    const long long r = row0 + wave * RPW + i;
    if (r >= total)
      continue;
    const int c = rc[i];
    if (lane < depth) {
      const long long o = r * depth + lane;
      if (lane < c) {
        out_seqs[o] = found[wave * RPW + i][c - 1 - lane]; // chronological
      } else {
        out_seqs[o] = -1;
        out_lengths[o] = 0;
      }
    }
    if (lane == 0)
      out_counts[r] = c;
  }
}

// Step 2: one wavefront per (r, j) slot with a seq, as k_deliver_device
// copies a row: 16-B lanes, the last chunk masked at payload_len, zero
// tail to `stride`, the record with payload_off rebased to the slot.
// k_context_find only hands out seqs of [evict_base, count), so the
// slot holds the message that seq names.
__global__ void __launch_bounds__(256)
    k_context_gather(const long long *__restrict__ ctx_seqs, long long n_slots,
                     const Rec *__restrict__ hdr,
                     const u8 *__restrict__ payload, u8 *__restrict__ out_pay,
                     uint4 *__restrict__ out_hdr, int *__restrict__ out_len,
                     u32 stride, QueueGeom g) {
  const long long o = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const u32 lane = threadIdx.x & 63;
  if (o >= n_slots)
    return;
  const long long seq = ctx_seqs[o];
  if (seq < 0)
    return;
  const Rec h = hdr[(u64)seq % g.num_slots];
  const u32 plen = h.payload_len < stride ? h.payload_len : stride;
  const u32 full = plen >> 4;
  const u32 rem = plen & 15u;
  const u32 row_chunks = stride >> 4;
  const uint4 *src = reinterpret_cast<const uint4 *>(payload + h.payload_off);
  uint4 *dst = reinterpret_cast<uint4 *>(out_pay + (u64)o * stride);
  for (u32 c = lane; c < row_chunks; c += 64) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (c < full) {
      v = src[c];
    } else if (c == full && rem) {
      v = src[c];
      v.x &= tail_mask(rem, 0);
      v.y &= tail_mask(rem, 4);
      v.z &= tail_mask(rem, 8);
      v.w &= tail_mask(rem, 12);
    }
    dst[c] = v;
  }
  if (lane == 0) {
    Rec hh = h;
    hh.payload_off = (u64)o * stride;
    uint4 hv[3];
    __builtin_memcpy(hv, &hh, sizeof(Rec));
    uint4 *oh = out_hdr + o * 3;
    oh[0] = hv[0];
    oh[1] = hv[1];
    oh[2] = hv[2];
  } else if (lane == 1) {
    out_len[o] = (int)plen;
  }
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
  const uint4 *src = reinterpret_cast<const uint4 *>(payload + h.payload_off);
  uint4 *dst =
      reinterpret_cast<uint4 *>(out_pay + (u64)wave * out_stride);
  u32 plen = h.payload_len;
  if (plen > out_stride)
    plen = out_stride;
  const u32 nchunk = (plen + 15u) >> 4;
  for (u32 c = lane; c < nchunk; c += 64)
    dst[c] = src[c];
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

// Batched status gather (no payload traffic).
__global__ void k_statuses(const u64 *__restrict__ seqs, int n,
                           u64 evict_base, const u32 *__restrict__ status,
                           u32 *__restrict__ out, QueueGeom g) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const u64 s = seqs[i];
  out[i] = (s < evict_base) ? ST_DELETED : status[s % g.num_slots];
}

// Batched status mutation with counter upkeep (history load restore).
__global__ void k_set_statuses(const u64 *__restrict__ seqs,
                               const u32 *__restrict__ new_status, int n,
                               u32 *__restrict__ status,
                               ull *__restrict__ by_status, QueueGeom g) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const u32 slot = (u32)(seqs[i] % g.num_slots);
  const u32 ns = new_status[i];
  const u32 old = atomicExch(&status[slot], ns);
  if (old != ns) {
    if (old < N_STATUS)
      atomicAdd(&by_status[old], (ull)(-1ll));
    if (ns < N_STATUS)
      atomicAdd(&by_status[ns], 1ull);
  }
}

// Device-side ack: the consumer hands back the int64 seq tensor of a
// device-resident delivery and the seqs are read straight from its
// pointer. An evicted seq is skipped (its slot belongs to a newer
// message), so is one never assigned, and a tombstone is never
// resurrected. A broadcast delivered to several agents shows up more
// than once; the exchange makes the counter move exactly once.
__global__ void k_ack_device(const long long *__restrict__ seqs, int n,
                             u32 new_status, u64 evict_base, u64 count,
                             u32 *__restrict__ status,
                             ull *__restrict__ by_status, QueueGeom g) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const u64 s = (u64)seqs[i];
  if (s < evict_base || s >= count)
    return;
  const u32 slot = (u32)(s % g.num_slots);
  if (status[slot] == ST_DELETED)
    return;
  const u32 old = atomicExch(&status[slot], new_status);
  if (old != new_status) {
    if (old < N_STATUS)
      atomicAdd(&by_status[old], (ull)(-1ll));
    if (new_status < N_STATUS)
      atomicAdd(&by_status[new_status], 1ull);
  }
}

// ---- device-resident send ----
//
// The records of a device-side producer live in a tensor the host never
// sees, so nothing in them may steer a read. Both kernels below write
// SANITISED records into the engine's own buffer, and the unchanged
// enqueue kernels run on that copy: payload_off is always
// (engine-derived row) * stride, and a length above the stride — the
// 16-B round-up of any smaller one stays inside the row, the stride
// being a multiple of 16 — is replaced by OVERSIZE, which k_enqueue_meta
// parks FAILED and k_enqueue_payload never copies.
constexpr u32 OVERSIZE = 0xFFFFFFFFu;

__device__ inline void store_rec(Rec *dst, const Rec &r) {
  uint4 v[3];
  __builtin_memcpy(v, &r, sizeof(Rec));
  uint4 *o = reinterpret_cast<uint4 *>(dst);
  o[0] = v[0];
  o[1] = v[1];
  o[2] = v[2];
}

// Sanitise caller records: one thread per record, three 16-B loads from
// the caller's tensor. Record i owns payload row i, whatever its own
// payload_off says. The visibility-bitmap HANDLE is split here into
// (pool slot, epoch), as GpuEngine.split_bitmap_handles does on the
// host path; an incoming bitmap_epoch is never trusted.
__global__ void __launch_bounds__(256)
    k_stage_device(const uint4 *__restrict__ src, int n, u32 stride,
                   u32 num_bitmaps, Rec *__restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  uint4 v[3];
  v[0] = src[(u64)i * 3];
  v[1] = src[(u64)i * 3 + 1];
  v[2] = src[(u64)i * 3 + 2];
  Rec r;
  __builtin_memcpy(&r, v, sizeof(Rec));
  r.payload_off = (u64)i * stride;
  if (r.payload_len > stride)
    r.payload_len = OVERSIZE;
  if (r.vis_mode != VIS_ALL && r.bitmap != NO_BITMAP) {
    r.bitmap_epoch = r.bitmap;
    r.bitmap = r.bitmap % num_bitmaps;
  } else {
    r.bitmap_epoch = 0;
  }
  store_rec(dst + i, r);
}

// Replies to a device-resident delivery. Row r is answered iff
// lengths[r] >= 0, and the answers are numbered in row order, so the
// kept rows need a stable compaction across workgroups. Two passes over
// the 4-byte lengths, one thread per row in 256-thread workgroups:
// k_reply_count leaves the kept rows of each workgroup, k_scan_counts
// turns those into workgroup offsets (and the total m, the one word the
// host reads back), and k_build_replies ranks each kept row inside its
// workgroup — a ballot + popcount per wave, the four wave totals through
// LDS — and writes its record at offset + rank.
__global__ void __launch_bounds__(256)
    k_reply_count(const int *__restrict__ lengths, int total,
                  u32 *__restrict__ block_counts) {
  __shared__ u32 wave_tot[4];
  const int r = blockIdx.x * 256 + (int)threadIdx.x;
  const bool keep = r < total && lengths[r] >= 0;
  const ull mask = __ballot(keep);
  if ((threadIdx.x & 63) == 0)
    wave_tot[threadIdx.x >> 6] = (u32)__popcll(mask);
  __syncthreads();
  if (threadIdx.x == 0)
    block_counts[blockIdx.x] =
        wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
}

// The reply to delivered row r: sender = the polled agent of the row
// (agents[agent_row[r]] — not the delivered receiver, which may be
// BROADCAST), receiver = the delivered sender, payload = row r of the
// caller's reply tensor. headers and agent_row are tensors the consumer
// could have written to, so an agent_row outside the polled list gives
// sender BROADCAST (out of range: the error lane) and is never used as
// an index; every other field is copied as a value, not followed.
__global__ void __launch_bounds__(256)
    k_build_replies(const uint4 *__restrict__ headers,
                    const int *__restrict__ agent_row,
                    const int *__restrict__ lengths, int total,
                    const u32 *__restrict__ agents, int n_agents,
                    const u32 *__restrict__ block_offsets, u32 rstride,
                    u32 type_code, int priority, u32 flags, double timestamp,
                    Rec *__restrict__ dst) {
  __shared__ u32 wave_tot[4];
  const u32 lane = threadIdx.x & 63;
  const u32 wave = threadIdx.x >> 6;
  const int r = blockIdx.x * 256 + (int)threadIdx.x;
  const int len = r < total ? lengths[r] : -1;
  const bool keep = len >= 0;
  const ull mask = __ballot(keep);
  if (lane == 0)
    wave_tot[wave] = (u32)__popcll(mask);
  __syncthreads();
  if (!keep)
    return;
  u32 before = 0;
  for (u32 w = 0; w < wave; ++w)
    before += wave_tot[w];
  const u32 rank = (u32)__popcll(mask & ((1ull << lane) - 1ull));
  const u32 j = block_offsets[blockIdx.x] + before + rank;

  const uint4 h0 = headers[(u64)r * 3]; // sender .x, type/priority/.. .z
  const int b = agent_row[r];
  Rec o;
  o.sender = (b >= 0 && b < n_agents) ? agents[b] : BROADCAST;
  o.receiver = h0.x;
  o.type = (u8)type_code;
  o.priority = priority >= 0 ? (u8)priority : (u8)((h0.z >> 8) & 0xFFu);
  o.vis_mode = VIS_ALL;
  o.flags = (u8)flags;
  o.token_count = 0;
  o.timestamp = timestamp;
  o.payload_off = (u64)r * rstride;
  o.payload_len = (u32)len > rstride ? OVERSIZE : (u32)len;
  o.bitmap = NO_BITMAP;
  o.content_len = (u32)len;
  o.bitmap_epoch = 0;
  store_rec(dst + j, o);
}

// Status mutation with counter upkeep (mark processed / admin status
// updates / delete tombstones).
__global__ void k_set_status(u64 seq, u32 new_status, u32 *__restrict__ status,
                             ull *__restrict__ by_status, QueueGeom g) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const u32 slot = (u32)(seq % g.num_slots);
    const u32 old = atomicExch(&status[slot], new_status);
    if (old != new_status) {
      if (old < N_STATUS)
        atomicAdd(&by_status[old], (ull)(-1ll));
      if (new_status < N_STATUS)
        atomicAdd(&by_status[new_status], 1ull);
    }
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
  const uint4 *s = reinterpret_cast<const uint4 *>(src_pay + src_off[wave]);
  uint4 *d = reinterpret_cast<uint4 *>(out + dst_off[wave]);
  const u32 nchunk = (lens[wave] + 15u) >> 4;
  for (u32 c = lane; c < nchunk; c += 64)
    d[c] = s[c];
}

__global__ void k_add_load(int idx, long long delta, ull *__restrict__ loads) {
  if (threadIdx.x == 0 && blockIdx.x == 0)
    atomicAdd(&loads[idx], (ull)delta);
}

// Device-resident dispatch of a delivery's rows (Engine.dispatch_delivery
// has the semantics). The greedy choice is serial in the rows, so one
// wavefront walks them with lane = backend, as in k_lb_batch; what makes a
// step cheap is that nothing but the choice itself is on the serial path:
//  - lane j resolves row base+j's (skip, pin, cost) for a whole 64-row
//    chunk at once (one coalesced header load, fetched two chunks ahead;
//    the pin lookup one chunk ahead), and the inner loop only broadcasts
//    them with a readlane at the wave-uniform index j;
//  - the argmin reduces the 64-bit load alone — DPP moves inside a row of
//    16 lanes, a shuffle only above that, and only the LEVELS that
//    n_backends needs — and a ballot of "my load is the minimum" gives the
//    lowest such lane: signed comparison, ties to the lowest index;
//  - lane k counts backend k's rows, so a row's rank within its backend is
//    a readlane of the winner's count, and k_dispatch_scatter can place
//    the row without a histogram pass;
//  - choice and rank of row j stay in lane j and are stored once per chunk.
// headers and agent_row are tensors the consumer could have written to:
// an agent_row outside the polled list reads as "not pinned" and is never
// used as an index, type and token_count are copied as values. The loop
// bounds come from the host-known total alone.
constexpr int DPP_QUAD_XOR1 = 0xB1;    // quad_perm:[1,0,3,2]
constexpr int DPP_QUAD_XOR2 = 0x4E;    // quad_perm:[2,3,0,1]
constexpr int DPP_HALF_MIRROR = 0x141; // lane i <-> 7 - i of each 8
constexpr int DPP_ROW_MIRROR = 0x140;  // lane i <-> 15 - i of each 16

template <int CTRL> __device__ __forceinline__ long long dpp_min_i64(long long v) {
  // every lane of these patterns has a source lane: no fill value needed
  const int lo = __builtin_amdgcn_mov_dpp((int)(u32)(ull)v, CTRL, 0xF, 0xF, true);
  const int hi =
      __builtin_amdgcn_mov_dpp((int)(u32)((ull)v >> 32), CTRL, 0xF, 0xF, true);
  const long long o = (long long)(((ull)(u32)hi << 32) | (ull)(u32)lo);
  return o < v ? o : v;
}

constexpr int DISPATCH_SKIP = -2; // row filtered out by type
constexpr int DISPATCH_FREE = -1; // row not pinned: least-loaded backend

struct DispatchRaw {
  u32 word2; // header bytes 8..11: type is the low byte
  u32 tokens;
  int arow;
};

// Row r's header words and agent_row, with r clamped into the delivery:
// the loads are unconditional, and rows past total are never walked.
__device__ __forceinline__ DispatchRaw
dispatch_load_row(const uint4 *__restrict__ headers,
                  const int *__restrict__ agent_row, int r, int total) {
  r = r < total ? r : total - 1;
  const uint4 h0 = headers[(u64)r * 3]; // type = byte 8, token_count = .w
  return DispatchRaw{h0.z, h0.w, agent_row[r]};
}

// The pin word of the row's polled agent, or of agent 0 for a row of no
// polled agent: dispatch_resolve drops that one. Its value is only used
// once the walk of the chunk before is over.
__device__ __forceinline__ int
dispatch_load_pin(const int *__restrict__ pinned, int n_agents, int arow) {
  if (n_agents <= 0)
    return DISPATCH_FREE;
  return pinned[(arow >= 0 && arow < n_agents) ? arow : 0];
}

__device__ __forceinline__ void
dispatch_resolve(const DispatchRaw &w, int pin, int n_agents, int n_backends,
                 int type_code, int by_tokens, int &sel, u32 &cost) {
  const bool polled = w.arow >= 0 && w.arow < n_agents;
  sel = (polled && pin >= 0 && pin < n_backends) ? pin : DISPATCH_FREE;
  if (type_code >= 0 && (w.word2 & 0xFFu) != (u32)type_code)
    sel = DISPATCH_SKIP;
  cost = by_tokens ? (w.tokens ? w.tokens : 1u) : 1u;
}

template <int LEVELS>
__global__ void __launch_bounds__(64)
    k_dispatch_rows(const uint4 *__restrict__ headers,
                    const int *__restrict__ agent_row, int total,
                    const int *__restrict__ pinned, int n_agents,
                    int n_backends, int type_code, int by_tokens,
                    ull *__restrict__ loads, int *__restrict__ backend,
                    int *__restrict__ rank, ull *__restrict__ added_out,
                    u32 *__restrict__ counts_out, int *__restrict__ offsets) {
  const int lane = (int)threadIdx.x;
  const bool mine = lane < n_backends;
  const ull live = n_backends >= 64 ? ~0ull : ((1ull << n_backends) - 1ull);
  long long my = mine ? (long long)loads[lane] : 0x7FFFFFFFFFFFFFFFll;
  ull added = 0;
  int cnt = 0;

  // software pipeline over 64-row chunks: the pin lookup of chunk c + 1,
  // the header loads of chunk c + 2 and the stores of chunk c - 1 are
  // issued before chunk c is walked and are not waited for until after
  // it, when chunk c + 1 is resolved
  DispatchRaw raw1{0u, 0u, -1};
  int sel_v = DISPATCH_SKIP;
  u32 cost_v = 1u;
  if (total > 0) {
    const DispatchRaw raw0 = dispatch_load_row(headers, agent_row, lane, total);
    raw1 = dispatch_load_row(headers, agent_row, 64 + lane, total);
    dispatch_resolve(raw0, dispatch_load_pin(pinned, n_agents, raw0.arow),
                     n_agents, n_backends, type_code, by_tokens, sel_v, cost_v);
  }

  int ch = -1, rk = 0; // choice and rank of row base + lane
  for (int base = 0; base < total; base += 64) {
    const int pin1 = dispatch_load_pin(pinned, n_agents, raw1.arow);
    // base + 128 cannot wrap: the host bounds total well below 2^31
    const DispatchRaw raw2 =
        dispatch_load_row(headers, agent_row, base + 128 + lane, total);

    if (base > 0) { // the chunk before this one was a full one
      backend[base - 64 + lane] = ch;
      rank[base - 64 + lane] = rk;
    }
    ch = -1;
    rk = 0;
    const int nrow = total - base < 64 ? total - base : 64;
    for (int j = 0; j < nrow; ++j) {
      const int sel = __builtin_amdgcn_readlane(sel_v, j);
      int k = -1, pos = 0;
      if (sel != DISPATCH_SKIP) {
        const u32 cost = (u32)__builtin_amdgcn_readlane((int)cost_v, j);
        k = sel;
        if (sel < 0) {
          long long v = my;
          if constexpr (LEVELS > 0)
            v = dpp_min_i64<DPP_QUAD_XOR1>(v);
          if constexpr (LEVELS > 1)
            v = dpp_min_i64<DPP_QUAD_XOR2>(v);
          if constexpr (LEVELS > 2)
            v = dpp_min_i64<DPP_HALF_MIRROR>(v);
          if constexpr (LEVELS > 3)
            v = dpp_min_i64<DPP_ROW_MIRROR>(v);
          if constexpr (LEVELS > 4) {
            const long long o = __shfl_xor(v, 16, 64);
            v = o < v ? o : v;
          }
          if constexpr (LEVELS > 5) {
            const long long o = __shfl_xor(v, 32, 64);
            v = o < v ? o : v;
          }
          // lanes [0, 2^LEVELS) all hold the minimum of the live loads; at
          // least the lane that owns it answers the ballot
          const ull hit = __ballot(my == v) & live;
          k = __ffsll((long long)hit) - 1;
        }
        pos = __builtin_amdgcn_readlane(cnt, k);
        if (lane == k) {
          my = (long long)((ull)my + cost);
          added += cost;
          ++cnt;
        }
      }
      if (lane == j) {
        ch = k;
        rk = pos;
      }
    }
    dispatch_resolve(raw1, pin1, n_agents, n_backends, type_code, by_tokens,
                     sel_v, cost_v);
    raw1 = raw2;
  }
  if (total > 0) {
    const int last = (total - 1) & ~63;
    if (last + lane < total) {
      backend[last + lane] = ch;
      rank[last + lane] = rk;
    }
  }

  // offsets = exclusive prefix sum of the per-backend row counts
  int off = 0;
  for (int i = 0; i < n_backends; ++i) {
    const int c = __builtin_amdgcn_readlane(cnt, i);
    if (lane > i)
      off += c;
  }
  if (mine) {
    loads[lane] = (ull)my;
    added_out[lane] = added;
    counts_out[lane] = (u32)cnt;
    offsets[lane] = off;
    if (lane == n_backends - 1)
      offsets[n_backends] = off + cnt;
  }
}

// order[offsets[backend[r]] + rank[r]] = r for every dispatched row: rows
// keep their order within a backend, because the rank was counted in row
// order. backend and rank come back from caller-visible tensors, so the
// index is bounded before it is used.
__global__ void __launch_bounds__(256)
    k_dispatch_scatter(const int *__restrict__ backend,
                       const int *__restrict__ rank,
                       const int *__restrict__ offsets, int total,
                       int n_backends, int *__restrict__ order) {
  const int r = blockIdx.x * 256 + (int)threadIdx.x;
  if (r >= total)
    return;
  const int b = backend[r];
  if (b < 0 || b >= n_backends)
    return;
  const long long idx = (long long)offsets[b] + (long long)rank[r];
  if (idx >= 0 && idx < (long long)total)
    order[idx] = r;
}

// The batch form of completing requests: loads[k] -= added[k], with added
// read from the dispatch's own tensor.
__global__ void k_release_loads(ull *__restrict__ loads,
                                const ull *__restrict__ added,
                                int n_backends) {
  const int k = (int)threadIdx.x;
  if (blockIdx.x == 0 && k < n_backends)
    loads[k] -= added[k];
}

// ---------------------------------------------------------------------------
// DeviceQueue — host runtime (the librdkafka-equivalent native layer)
// ---------------------------------------------------------------------------

class DeviceQueue {
public:
  DeviceQueue(u32 num_slots, u32 slot_bytes, u32 max_agents,
              u32 inbox_capacity, u32 num_bitmaps, u32 num_backends,
              u32 staging_batch, int device, u32 recv_window = RECV_WINDOW)
      : device_(device), staging_batch_(staging_batch) {
    if (slot_bytes % 16 != 0)
      throw std::invalid_argument("slot_bytes must be a multiple of 16");
    if (max_agents % 64 != 0)
      throw std::invalid_argument("max_agents must be a multiple of 64");
    g_.num_slots = num_slots;
    g_.slot_bytes = slot_bytes;
    g_.max_agents = max_agents;
    g_.inbox_capacity = inbox_capacity;
    g_.num_bitmaps = num_bitmaps;
    g_.bitmap_words = max_agents / 64;
    g_.num_backends = num_backends;
    if (recv_window < 64 || (recv_window & (recv_window - 1)))
      throw std::invalid_argument("recv_window must be a power of two >= 64");
    g_.recv_window = recv_window;

    HIP_CHECK(hipSetDevice(device_));
    HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    HIP_CHECK(hipStreamCreateWithFlags(&copy_stream_, hipStreamNonBlocking));
    HIP_CHECK(hipStreamCreateWithFlags(&h2d_stream_, hipStreamNonBlocking));
    HIP_CHECK(hipStreamCreateWithFlags(&lb_stream_, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreateWithFlags(&ev_, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&up_ev_[0], hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&up_ev_[1], hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&d2h_ev_[0], hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&d2h_ev_[1], hipEventDisableTiming));

    // device state
    HIP_CHECK(hipMalloc(&d_hdr_, (size_t)num_slots * sizeof(Rec)));
    HIP_CHECK(hipMalloc(&d_status_, (size_t)num_slots * sizeof(u32)));
    HIP_CHECK(hipMalloc(&d_payload_, (size_t)num_slots * slot_bytes));
    HIP_CHECK(
        hipMalloc(&d_inbox_, (size_t)max_agents * inbox_capacity * sizeof(u64)));
    HIP_CHECK(hipMalloc(&d_wpos_, (size_t)max_agents * sizeof(ull)));
    HIP_CHECK(hipMalloc(&d_rpos_, (size_t)max_agents * sizeof(ull)));
    HIP_CHECK(hipMalloc(&d_carry_,
                        (size_t)max_agents * g_.recv_window * sizeof(u64)));
    HIP_CHECK(hipMalloc(&d_carry_n_, (size_t)max_agents * sizeof(u32)));
    HIP_CHECK(hipMalloc(&d_active_, (size_t)max_agents * sizeof(u32)));
    HIP_CHECK(hipMalloc(&d_bitmaps_,
                        (size_t)num_bitmaps * g_.bitmap_words * sizeof(u64)));
    HIP_CHECK(hipMalloc(&d_bitmap_epochs_, (size_t)num_bitmaps * sizeof(u32)));
    HIP_CHECK(hipMemset(d_bitmap_epochs_, 0xFF,
                        (size_t)num_bitmaps * sizeof(u32))); // all EPOCH_NONE
    HIP_CHECK(hipMalloc(&d_dropped_, sizeof(ull)));
    HIP_CHECK(hipMemset(d_dropped_, 0, sizeof(ull)));
    HIP_CHECK(hipMalloc(&d_by_type_, N_TYPES * sizeof(ull)));
    HIP_CHECK(hipMalloc(&d_by_status_, N_STATUS * sizeof(ull)));
    HIP_CHECK(hipMalloc(&d_sent_, (size_t)max_agents * sizeof(ull)));
    HIP_CHECK(hipMalloc(&d_received_, (size_t)max_agents * sizeof(ull)));
    HIP_CHECK(hipMalloc(&d_bcast_, (size_t)staging_batch * sizeof(u64)));
    HIP_CHECK(hipMalloc(&d_bcast_count_, sizeof(u32)));
    HIP_CHECK(hipMalloc(&d_backend_loads_, (size_t)num_backends * sizeof(ull)));
    HIP_CHECK(hipMalloc(&d_choices_, (size_t)staging_batch * sizeof(u32)));
    HIP_CHECK(hipMalloc(&d_lb_out_, (size_t)staging_batch * sizeof(u32)));
    HIP_CHECK(hipMalloc(&d_match_, (size_t)staging_batch * sizeof(u64)));
    HIP_CHECK(hipMalloc(&d_match_count_, sizeof(u32)));
    HIP_CHECK(hipMalloc(&d_needle_, 256));
    HIP_CHECK(hipMalloc(&d_agents_, (size_t)max_agents * sizeof(u32)));
    HIP_CHECK(hipMalloc(&d_unread_, (size_t)max_agents * sizeof(u32)));

    HIP_CHECK(hipMalloc(&d_dyn_, 2 * sizeof(u64)));
    HIP_CHECK(hipMalloc(&d_tail_, sizeof(ull)));
    HIP_CHECK(hipMemset(d_tail_, 0, sizeof(ull)));
    out_pool_ = (size_t)4 << 20; // receive output pool: 4M entries, 32 MB
    HIP_CHECK(hipMalloc(&d_out_seqs_, out_pool_ * sizeof(u64)));
    HIP_CHECK(hipMalloc(&d_out_counts_, (size_t)max_agents * sizeof(u32)));

    // staging (device side of the H2D batch), double-buffered so the
    // host can fill batch i+1 while batch i's H2D/kernels run
    stage_pay_bytes_ = (size_t)staging_batch * 1024; // grows on demand
    for (int s = 0; s < 2; ++s) {
      HIP_CHECK(hipMalloc(&d_stage_recs_[s], (size_t)staging_batch * sizeof(Rec)));
      HIP_CHECK(hipMalloc(&d_stage_pay_[s], stage_pay_bytes_));
      HIP_CHECK(hipEventCreateWithFlags(&stage_ev_[s], hipEventDisableTiming));
    }
    HIP_CHECK(hipMalloc(&d_seqs_in_, (size_t)staging_batch * sizeof(u64)));
    HIP_CHECK(hipMalloc(&d_fetch_hdr_, (size_t)staging_batch * sizeof(Rec)));
    HIP_CHECK(hipMalloc(&d_fetch_status_, (size_t)staging_batch * sizeof(u32)));
    HIP_CHECK(hipMalloc(&d_fetch_pay_, (size_t)staging_batch * slot_bytes));

    // pinned host staging
    for (int s = 0; s < 2; ++s) {
      HIP_CHECK(hipHostMalloc(&h_recs_[s], (size_t)staging_batch * sizeof(Rec)));
      HIP_CHECK(hipHostMalloc(&h_pay_[s], stage_pay_bytes_));
    }
    HIP_CHECK(hipHostMalloc(&h_out_seqs_, out_pool_ * sizeof(u64)));
    HIP_CHECK(hipHostMalloc(&h_out_counts_, (size_t)max_agents * sizeof(u32)));
    HIP_CHECK(hipHostMalloc(&h_fetch_hdr_, (size_t)staging_batch * sizeof(Rec)));
    HIP_CHECK(
        hipHostMalloc(&h_fetch_status_, (size_t)staging_batch * sizeof(u32)));
    HIP_CHECK(hipHostMalloc(&h_fetch_pay_, (size_t)staging_batch * slot_bytes));
    HIP_CHECK(hipHostMalloc(&h_choices_, (size_t)staging_batch * sizeof(u32)));

    // zero all mutable state
    HIP_CHECK(hipMemset(d_status_, 0, (size_t)num_slots * sizeof(u32)));
    HIP_CHECK(hipMemset(d_wpos_, 0, (size_t)max_agents * sizeof(ull)));
    HIP_CHECK(hipMemset(d_rpos_, 0, (size_t)max_agents * sizeof(ull)));
    HIP_CHECK(hipMemset(d_carry_n_, 0, (size_t)max_agents * sizeof(u32)));
    HIP_CHECK(hipMemset(d_active_, 0, (size_t)max_agents * sizeof(u32)));
    HIP_CHECK(hipMemset(d_by_type_, 0, N_TYPES * sizeof(ull)));
    HIP_CHECK(hipMemset(d_by_status_, 0, N_STATUS * sizeof(ull)));
    HIP_CHECK(hipMemset(d_sent_, 0, (size_t)max_agents * sizeof(ull)));
    HIP_CHECK(hipMemset(d_received_, 0, (size_t)max_agents * sizeof(ull)));
    HIP_CHECK(hipMemset(d_backend_loads_, 0, (size_t)num_backends * sizeof(ull)));

    // device-resident send: sanitised records, and the per-workgroup
    // reply counts / offsets of the compaction (256 rows per workgroup).
    // Allocated last, so that every buffer above sits where it did
    // before these existed (profiles/device_send.md)
    const size_t reply_blocks = ((size_t)staging_batch + 255) / 256;
    HIP_CHECK(hipMalloc(&d_dev_recs_, (size_t)staging_batch * sizeof(Rec)));
    HIP_CHECK(hipMalloc(&d_reply_blk_, reply_blocks * sizeof(u32)));
    HIP_CHECK(hipMalloc(&d_reply_off_, (reply_blocks + 1) * sizeof(u32)));
    HIP_CHECK(hipHostMalloc(&h_reply_m_, sizeof(u32)));

    // device-resident dispatch: the device copy of the pins (one word per
    // polled agent) and the per-backend row counts with their pinned
    // landing buffer. Last again, for the same reason
    HIP_CHECK(hipMalloc(&d_disp_pinned_, (size_t)max_agents * sizeof(int)));
    HIP_CHECK(hipMalloc(&d_disp_counts_, 64 * sizeof(u32)));
    HIP_CHECK(hipHostMalloc(&h_disp_counts_, 64 * sizeof(u32)));
  }

  ~DeviceQueue() { release(); }

  void release() {
    if (released_)
      return;
    released_ = true;
    (void)hipStreamSynchronize(stream_);
    (void)hipStreamSynchronize(copy_stream_);
    for (void *p :
         std::vector<void *>{d_hdr_, d_status_, d_payload_, d_inbox_, d_wpos_,
                             d_rpos_, d_carry_, d_carry_n_, d_active_,
                             d_bitmaps_, d_bitmap_epochs_, d_dropped_,
                             d_by_type_, d_by_status_, d_sent_,
                             d_received_, d_bcast_, d_bcast_count_,
                             d_backend_loads_, d_choices_, d_lb_out_, d_match_,
                             d_match_count_, d_needle_, d_agents_, d_unread_,
                             d_dyn_, d_tail_,
                             d_out_seqs_, d_out_counts_, d_stage_recs_[0],
                             d_stage_recs_[1], d_stage_pay_[0],
                             d_stage_pay_[1], d_seqs_in_, d_fetch_hdr_,
                             d_fetch_status_, d_fetch_pay_, d_dev_recs_,
                             d_reply_blk_, d_reply_off_, d_disp_pinned_,
                             d_disp_counts_})
      (void)hipFree(p);
    for (void *p : std::vector<void *>{h_recs_[0], h_recs_[1], h_pay_[0],
                                       h_pay_[1], h_out_seqs_,
                                       h_out_counts_, h_fetch_hdr_,
                                       h_fetch_status_, h_fetch_pay_,
                                       h_choices_, h_reply_m_,
                                       h_disp_counts_})
      (void)hipHostFree(p);
    (void)hipEventDestroy(stage_ev_[0]);
    (void)hipEventDestroy(stage_ev_[1]);
    for (int s = 0; s < 2; ++s)
      if (tick_exec_[s])
        (void)hipGraphExecDestroy(tick_exec_[s]);
    (void)hipEventDestroy(ev_);
    (void)hipEventDestroy(up_ev_[0]);
    (void)hipEventDestroy(up_ev_[1]);
    (void)hipEventDestroy(d2h_ev_[0]);
    (void)hipEventDestroy(d2h_ev_[1]);
    (void)hipStreamDestroy(stream_);
    (void)hipStreamDestroy(copy_stream_);
    (void)hipStreamDestroy(h2d_stream_);
    (void)hipStreamDestroy(lb_stream_);
  }

  // ---- registry ----

  void register_agent(u32 idx) {
    check_agent(idx);
    const u32 one = 1;
    HIP_CHECK(hipMemcpy(d_active_ + idx, &one, sizeof(u32),
                        hipMemcpyHostToDevice));
  }

  void deregister_agent(u32 idx) {
    check_agent(idx);
    const u32 zero = 0;
    HIP_CHECK(hipMemcpy(d_active_ + idx, &zero, sizeof(u32),
                        hipMemcpyHostToDevice));
  }

  py::array_t<u32> active_agents() {
    py::array_t<u32> out(g_.max_agents);
    HIP_CHECK(hipMemcpy(out.mutable_data(), d_active_,
                        g_.max_agents * sizeof(u32), hipMemcpyDeviceToHost));
    return out;
  }

  // ---- send plane ----

  // recs: n x 48 bytes (REC_DTYPE), payload_off 16-B aligned into `pay`.
  // Returns base seq. The stream sync at the end is the DELIVERED ack.
  u64 enqueue_batch(py::buffer recs, py::buffer pay, int n) {
    py::buffer_info ri = recs.request(), pi = pay.request();
    if ((size_t)ri.size * ri.itemsize < (size_t)n * sizeof(Rec))
      throw std::invalid_argument("recs buffer too small");
    if (n <= 0)
      return count_;
    if ((u32)n > staging_batch_)
      throw std::invalid_argument("batch exceeds staging_batch");
    const size_t pay_bytes = (size_t)pi.size * pi.itemsize;
    ensure_stage_pay(pay_bytes + 16);

    const u64 base = count_;
    {
      py::gil_scoped_release nogil;
      std::memcpy(h_recs_[0], ri.ptr, (size_t)n * sizeof(Rec));
      if (pay_bytes)
        par_memcpy(h_pay_[0], pi.ptr, pay_bytes);
      HIP_CHECK(hipMemcpyAsync(d_stage_recs_[0], h_recs_[0],
                               (size_t)n * sizeof(Rec),
                               hipMemcpyHostToDevice, stream_));
      if (pay_bytes)
        HIP_CHECK(hipMemcpyAsync(d_stage_pay_[0], h_pay_[0], pay_bytes,
                                 hipMemcpyHostToDevice, stream_));
      HIP_CHECK(hipEventRecord(stage_ev_[0], stream_));
      HIP_CHECK(hipMemsetAsync(d_bcast_count_, 0, sizeof(u32), stream_));
      launch_enqueue(d_stage_recs_[0], d_stage_pay_[0], n, base);
      HIP_CHECK(hipStreamSynchronize(stream_));
    }
    count_ = base + (u64)n;
    if (count_ > g_.num_slots)
      evict_base_ = count_ - g_.num_slots;
    return base;
  }

  // Async variant: fill slot 0 and launch without a sync; caller must
  // sync() (or rely on stream ordering) before reading results.
  u64 enqueue_batch_async(py::buffer recs, py::buffer pay, int n) {
    if (n <= 0)
      return count_;
    stage_fill(0, recs, pay, n);
    return enqueue_staged(0);
  }

  void sync() {
    py::gil_scoped_release nogil;
    HIP_CHECK(hipStreamSynchronize(stream_));
  }

  // ---- pipelined staging: fill one pinned set while the other's
  // H2D/kernels are in flight ----

  void stage_fill(int slot, py::buffer recs, py::buffer pay, int n) {
    if (slot < 0 || slot > 1)
      throw std::invalid_argument("slot must be 0 or 1");
    if ((u32)n > staging_batch_)
      throw std::invalid_argument("batch exceeds staging_batch");
    py::buffer_info ri = recs.request(), pi = pay.request();
    const size_t pay_bytes = (size_t)pi.size * pi.itemsize;
    ensure_stage_pay(pay_bytes + 16);
    {
      py::gil_scoped_release nogil;
      // don't overwrite pinned memory a previous H2D still reads
      HIP_CHECK(hipEventSynchronize(stage_ev_[slot]));
      std::memcpy(h_recs_[slot], ri.ptr, (size_t)n * sizeof(Rec));
      if (pay_bytes)
        par_memcpy(h_pay_[slot], pi.ptr, pay_bytes);
    }
    staged_n_[slot] = n;
    staged_pay_[slot] = pay_bytes;
  }

  // Allocate pinned host memory exposed as a numpy array (freed by the
  // array's capsule). Producers can build batches in-place and hand the
  // pointers to prefetch_from — zero host-side copies on the send path.
  static py::array alloc_pinned(size_t nbytes) {
    void *p = nullptr;
    HIP_CHECK(hipHostMalloc(&p, nbytes));
    py::capsule owner(p, [](void *q) { (void)hipHostFree(q); });
    return py::array_t<u8>({(py::ssize_t)nbytes}, {(py::ssize_t)1},
                           static_cast<u8 *>(p), owner);
  }

  // Upload a batch that ALREADY lives in pinned host memory (e.g. from
  // alloc_pinned) straight onto the H2D stream — no staging memcpy.
  // The caller must not rewrite the buffers until the upload completes
  // (one tick later with double-buffered slots).
  void prefetch_from(int slot, uintptr_t recs_ptr, uintptr_t pay_ptr, int n,
                     size_t pay_bytes) {
    if (slot < 0 || slot > 1)
      throw std::invalid_argument("slot must be 0 or 1");
    if ((u32)n > staging_batch_)
      throw std::invalid_argument("batch exceeds staging_batch");
    ensure_stage_pay(pay_bytes + 16);
    {
      py::gil_scoped_release nogil;
      HIP_CHECK(hipMemcpyAsync(d_stage_recs_[slot],
                               reinterpret_cast<void *>(recs_ptr),
                               (size_t)n * sizeof(Rec),
                               hipMemcpyHostToDevice, h2d_stream_));
      if (pay_bytes)
        HIP_CHECK(hipMemcpyAsync(d_stage_pay_[slot],
                                 reinterpret_cast<void *>(pay_ptr), pay_bytes,
                                 hipMemcpyHostToDevice, h2d_stream_));
      HIP_CHECK(hipEventRecord(stage_ev_[slot], h2d_stream_));
      HIP_CHECK(hipEventRecord(up_ev_[slot], h2d_stream_));
    }
    staged_n_[slot] = n;
    staged_pay_[slot] = pay_bytes;
    uploaded_[slot] = true;
  }

  // Upload a filled slot's staging buffers on the dedicated H2D stream
  // (overlaps the main stream's kernels and the copy stream's delivery
  // D2H — PCIe is full duplex). enqueue_staged picks the upload up.
  void prefetch_staged(int slot) {
    if (slot < 0 || slot > 1)
      throw std::invalid_argument("slot must be 0 or 1");
    const int n = staged_n_[slot];
    if (n <= 0)
      return;
    const size_t pay_bytes = staged_pay_[slot];
    py::gil_scoped_release nogil;
    HIP_CHECK(hipMemcpyAsync(d_stage_recs_[slot], h_recs_[slot],
                             (size_t)n * sizeof(Rec), hipMemcpyHostToDevice,
                             h2d_stream_));
    if (pay_bytes)
      HIP_CHECK(hipMemcpyAsync(d_stage_pay_[slot], h_pay_[slot], pay_bytes,
                               hipMemcpyHostToDevice, h2d_stream_));
    HIP_CHECK(hipEventRecord(stage_ev_[slot], h2d_stream_));
    HIP_CHECK(hipEventRecord(up_ev_[slot], h2d_stream_));
    uploaded_[slot] = true;
  }

  // Launch H2D + enqueue kernels for a previously filled slot; returns
  // the base seq. NO sync — receive_many on the same stream is ordered
  // after it.
  u64 enqueue_staged(int slot) {
    if (slot < 0 || slot > 1)
      throw std::invalid_argument("slot must be 0 or 1");
    const int n = staged_n_[slot];
    if (n <= 0)
      return count_;
    const size_t pay_bytes = staged_pay_[slot];
    const u64 base = count_;
    {
      py::gil_scoped_release nogil;
      if (uploaded_[slot]) {
        // already uploaded by prefetch_staged: order kernels after it
        HIP_CHECK(hipStreamWaitEvent(stream_, up_ev_[slot], 0));
        uploaded_[slot] = false;
      } else {
        HIP_CHECK(hipMemcpyAsync(d_stage_recs_[slot], h_recs_[slot],
                                 (size_t)n * sizeof(Rec),
                                 hipMemcpyHostToDevice, stream_));
        if (pay_bytes)
          HIP_CHECK(hipMemcpyAsync(d_stage_pay_[slot], h_pay_[slot],
                                   pay_bytes, hipMemcpyHostToDevice, stream_));
        HIP_CHECK(hipEventRecord(stage_ev_[slot], stream_));
      }
      HIP_CHECK(hipMemsetAsync(d_bcast_count_, 0, sizeof(u32), stream_));
      launch_enqueue(d_stage_recs_[slot], d_stage_pay_[slot], n, base);
    }
    count_ = base + (u64)n;
    if (count_ > g_.num_slots)
      evict_base_ = count_ - g_.num_slots;
    return base;
  }

  // ---- captured steady-state tick (hipGraph) ----
  // One graph per staging slot captures the whole delivery tick:
  // tick-begin (device tail) -> enqueue meta+payload -> fanout ->
  // receive -> counts/seqs D2H. Replay cost is one graph launch instead
  // of ~10 API calls; the H2D prefetch stays outside (its event is
  // waited on the stream before the launch).
  void build_tick(int n, py::array_t<u32> agents, int K, bool priority) {
    const int na = (int)agents.size();
    if (n <= 0 || (u32)n > staging_batch_)
      throw std::invalid_argument("bad tick batch size");
    if ((size_t)na * K > out_pool_)
      throw std::invalid_argument("tick exceeds output pool");
    for (int s = 0; s < 2; ++s)
      if (tick_exec_[s]) {
        (void)hipGraphExecDestroy(tick_exec_[s]);
        tick_exec_[s] = nullptr;
      }
    HIP_CHECK(hipStreamSynchronize(stream_));
    HIP_CHECK(hipMemcpy(d_agents_, agents.data(), na * sizeof(u32),
                        hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_tail_, &count_, sizeof(ull),
                        hipMemcpyHostToDevice));
    for (int s = 0; s < 2; ++s) {
      hipGraph_t graph;
      HIP_CHECK(hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal));
      HIP_CHECK(hipMemsetAsync(d_bcast_count_, 0, sizeof(u32), stream_));
      hipLaunchKernelGGL(k_tick_begin, dim3(1), dim3(64), 0, stream_, d_dyn_,
                         d_tail_, n, (u64)g_.num_slots);
      hipLaunchKernelGGL(k_enqueue_meta, dim3((n + 255) / 256), dim3(256), 0,
                         stream_, d_stage_recs_[s], n, 0, d_dyn_, d_hdr_,
                         d_status_, d_inbox_, d_wpos_, d_rpos_, d_by_type_,
                         d_by_status_, d_sent_, d_bcast_, d_bcast_count_,
                         d_dropped_, g_);
      hipLaunchKernelGGL(k_enqueue_payload, dim3((n + 3) / 4), dim3(256), 0,
                         stream_, d_stage_recs_[s], d_stage_pay_[s], n, 0,
                         d_dyn_, d_payload_, g_);
      hipLaunchKernelGGL(k_fanout, dim3((g_.max_agents + 255) / 256),
                         dim3(256), 0, stream_, d_bcast_, d_bcast_count_,
                         d_active_, d_hdr_, d_bitmaps_, d_bitmap_epochs_,
                         d_inbox_, d_wpos_, d_rpos_, d_dropped_, g_);
      hipLaunchKernelGGL(k_receive, dim3(na), dim3(256),
                         (g_.recv_window + 2) * sizeof(u64), stream_,
                         d_agents_, na, K, priority ? 1 : 0, 0, d_dyn_,
                         d_hdr_, d_status_, d_inbox_, d_wpos_, d_rpos_,
                         d_carry_, d_carry_n_, d_bitmaps_, d_bitmap_epochs_,
                         d_out_seqs_, d_out_counts_, d_by_status_,
                         d_received_, g_);
      HIP_CHECK(hipMemcpyAsync(h_out_counts_, d_out_counts_, na * sizeof(u32),
                               hipMemcpyDeviceToHost, stream_));
      HIP_CHECK(hipMemcpyAsync(h_out_seqs_, d_out_seqs_,
                               (size_t)na * K * sizeof(u64),
                               hipMemcpyDeviceToHost, stream_));
      HIP_CHECK(hipStreamEndCapture(stream_, &graph));
      HIP_CHECK(hipGraphInstantiate(&tick_exec_[s], graph, nullptr, nullptr, 0));
      HIP_CHECK(hipGraphDestroy(graph));
    }
    tick_n_ = n;
    tick_na_ = na;
    tick_K_ = K;
  }

  // Replay the captured tick for a slot previously uploaded with
  // prefetch_from/prefetch_staged. Returns (counts, seqs).
  py::tuple run_tick(int slot) {
    if (slot < 0 || slot > 1 || !tick_exec_[slot])
      throw std::invalid_argument("tick graph not built for this slot");
    py::array_t<u32> counts(tick_na_);
    py::array_t<u64> seqs((size_t)tick_na_ * tick_K_);
    {
      py::gil_scoped_release nogil;
      if (uploaded_[slot]) {
        HIP_CHECK(hipStreamWaitEvent(stream_, up_ev_[slot], 0));
        uploaded_[slot] = false;
      }
      HIP_CHECK(hipGraphLaunch(tick_exec_[slot], stream_));
      HIP_CHECK(hipStreamSynchronize(stream_));
    }
    count_ += (u64)tick_n_;
    if (count_ > g_.num_slots)
      evict_base_ = count_ - g_.num_slots;
    last_recv_na_ = tick_na_;
    last_recv_K_ = tick_K_;
    std::memcpy(counts.mutable_data(), h_out_counts_,
                tick_na_ * sizeof(u32));
    std::memcpy(seqs.mutable_data(), h_out_seqs_,
                (size_t)tick_na_ * tick_K_ * sizeof(u64));
    return py::make_tuple(counts, seqs);
  }

  // ---- GPU-direct cross-GPU routing support ----

  // Stage this rank's raw batch payload H2D and scatter instances into a
  // caller-provided device send buffer (a torch tensor's data_ptr). The
  // instance arrays are host-computed: src_off into the staged payload,
  // dst_off into the send buffer (both 16-B aligned). Synchronizes so
  // the collective can run on any stream afterwards.
  void pack_exchange(py::buffer pay, py::array_t<u64> src_off,
                     py::array_t<u64> dst_off, py::array_t<u32> lens,
                     uintptr_t send_ptr) {
    const int n = (int)src_off.size();
    if (n == 0)
      return;
    if ((u32)n > staging_batch_)
      throw std::invalid_argument("pack batch exceeds staging_batch");
    py::buffer_info pi = pay.request();
    const size_t pay_bytes = (size_t)pi.size * pi.itemsize;
    ensure_stage_pay(pay_bytes + 16);
    {
      py::gil_scoped_release nogil;
      HIP_CHECK(hipEventSynchronize(stage_ev_[0]));
      par_memcpy(h_pay_[0], pi.ptr, pay_bytes);
      HIP_CHECK(hipMemcpyAsync(d_stage_pay_[0], h_pay_[0], pay_bytes,
                               hipMemcpyHostToDevice, stream_));
      HIP_CHECK(hipEventRecord(stage_ev_[0], stream_));
      HIP_CHECK(hipMemcpyAsync(d_seqs_in_, src_off.data(), n * sizeof(u64),
                               hipMemcpyHostToDevice, stream_));
      HIP_CHECK(hipMemcpyAsync(d_match_, dst_off.data(), n * sizeof(u64),
                               hipMemcpyHostToDevice, stream_));
      HIP_CHECK(hipMemcpyAsync(d_choices_, lens.data(), n * sizeof(u32),
                               hipMemcpyHostToDevice, stream_));
      hipLaunchKernelGGL(k_pack, dim3((n + 3) / 4), dim3(256), 0, stream_,
                         d_stage_pay_[0], d_seqs_in_, d_match_, d_choices_, n,
                         reinterpret_cast<u8 *>(send_ptr));
      HIP_CHECK(hipStreamSynchronize(stream_));
    }
  }

  // Enqueue a batch whose records and payloads are ALREADY on the device
  // (e.g. an all-to-all receive buffer): no host staging at all.
  // Asynchronous; stream-ordered before any later receive_many.
  u64 enqueue_from_ptrs(uintptr_t recs_ptr, uintptr_t pay_ptr, int n) {
    if (n <= 0)
      return count_;
    const u64 base = count_;
    {
      py::gil_scoped_release nogil;
      HIP_CHECK(hipMemsetAsync(d_bcast_count_, 0, sizeof(u32), stream_));
      launch_enqueue(reinterpret_cast<const Rec *>(recs_ptr),
                     reinterpret_cast<const u8 *>(pay_ptr), n, base);
    }
    count_ = base + (u64)n;
    if (count_ > g_.num_slots)
      evict_base_ = count_ - g_.num_slots;
    return base;
  }

  // Device-resident send: n REC_DTYPE records in a caller tensor
  // (`headers_ptr`, 48 B each) whose record i owns row i of the
  // [n, stride] payload tensor at `payload_ptr`. k_stage_device copies
  // the records into the engine's own buffer with every value a read
  // depends on forced or bounded (see the kernel), then the ordinary
  // enqueue kernels run on that copy. At most staging_batch records per
  // call (d_bcast_ and the record buffer hold that many); the caller
  // chunks. Every check runs before anything is launched. Synchronizes,
  // so the caller may overwrite its tensors afterwards.
  u64 enqueue_from_device(uintptr_t headers_ptr, uintptr_t payload_ptr, int n,
                          u32 stride) {
    if (n < 0 || (u32)n > staging_batch_)
      throw std::invalid_argument("batch exceeds staging_batch");
    check_row_stride(stride);
    if (n == 0)
      return count_;
    if (!headers_ptr || !payload_ptr)
      throw std::invalid_argument("send buffer pointer is null");
    if (headers_ptr % 16 || payload_ptr % 16)
      throw std::invalid_argument("send buffer is misaligned");
    const u64 base = count_;
    {
      py::gil_scoped_release nogil;
      hipLaunchKernelGGL(k_stage_device, dim3((n + 255) / 256), dim3(256), 0,
                         stream_, reinterpret_cast<const uint4 *>(headers_ptr),
                         n, stride, g_.num_bitmaps, d_dev_recs_);
      HIP_CHECK(hipMemsetAsync(d_bcast_count_, 0, sizeof(u32), stream_));
      launch_enqueue(d_dev_recs_, reinterpret_cast<const u8 *>(payload_ptr), n,
                     base);
      HIP_CHECK(hipStreamSynchronize(stream_));
    }
    count_ = base + (u64)n;
    if (count_ > g_.num_slots)
      evict_base_ = count_ - g_.num_slots;
    return base;
  }

  // Reply to the first `total` rows of a device-resident delivery from
  // device tensors: row r is answered iff lengths[r] >= 0, with row r of
  // the [>= total, rstride] reply tensor as payload (k_build_replies has
  // the field rules). Replies are numbered in row order; returns
  // (base seq, m). Only the polled agents (na words) go to the device
  // and only m (4 B) comes back. `total` is bounded by staging_batch,
  // like any batch; the caller splits a larger delivery by rows.
  // `priority` < 0 inherits the delivered message's. Every check runs
  // before anything is launched; synchronizes.
  py::tuple reply_from_device(uintptr_t headers_ptr, uintptr_t agent_row_ptr,
                              uintptr_t lengths_ptr, uintptr_t payload_ptr,
                              int total, u32 rstride, py::array_t<u32> agents,
                              u32 type_code, int priority, u32 flags,
                              double timestamp) {
    const int na = (int)agents.size();
    if (total < 0 || (u32)total > staging_batch_)
      throw std::invalid_argument("batch exceeds staging_batch");
    check_row_stride(rstride);
    if ((u32)na > g_.max_agents)
      throw std::invalid_argument("more polled agents than max_agents");
    if (priority > 255 || type_code > 255u || flags > 255u)
      throw std::invalid_argument("type, priority and flags are one byte");
    if (total == 0)
      return py::make_tuple(count_, 0u);
    if (!headers_ptr || !agent_row_ptr || !lengths_ptr || !payload_ptr)
      throw std::invalid_argument("reply buffer pointer is null");
    if (headers_ptr % 16 || payload_ptr % 16 || agent_row_ptr % 4 ||
        lengths_ptr % 4)
      throw std::invalid_argument("reply buffer is misaligned");
    const u64 base = count_;
    const int nblk = (total + 255) / 256;
    u32 m = 0;
    {
      py::gil_scoped_release nogil;
      const int *d_len = reinterpret_cast<const int *>(lengths_ptr);
      if (na)
        HIP_CHECK(hipMemcpyAsync(d_agents_, agents.data(), na * sizeof(u32),
                                 hipMemcpyHostToDevice, stream_));
      hipLaunchKernelGGL(k_reply_count, dim3(nblk), dim3(256), 0, stream_,
                         d_len, total, d_reply_blk_);
      hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(256), 4 * sizeof(u32),
                         stream_, d_reply_blk_, nblk, d_reply_off_);
      hipLaunchKernelGGL(k_build_replies, dim3(nblk), dim3(256), 0, stream_,
                         reinterpret_cast<const uint4 *>(headers_ptr),
                         reinterpret_cast<const int *>(agent_row_ptr), d_len,
                         total, d_agents_, na, d_reply_off_, rstride,
                         type_code, priority, flags, timestamp, d_dev_recs_);
      HIP_CHECK(hipMemcpyAsync(h_reply_m_, d_reply_off_ + nblk, sizeof(u32),
                               hipMemcpyDeviceToHost, stream_));
      HIP_CHECK(hipStreamSynchronize(stream_));
      m = *h_reply_m_;
      if (m > (u32)total) // cannot happen: at most one reply per row
        throw std::runtime_error("reply compaction overran its rows");
      if (m) {
        HIP_CHECK(hipMemsetAsync(d_bcast_count_, 0, sizeof(u32), stream_));
        launch_enqueue(d_dev_recs_, reinterpret_cast<const u8 *>(payload_ptr),
                       (int)m, base);
        HIP_CHECK(hipStreamSynchronize(stream_));
      }
    }
    count_ = base + (u64)m;
    if (count_ > g_.num_slots)
      evict_base_ = count_ - g_.num_slots;
    return py::make_tuple(base, m);
  }

  // Returns the allocation HANDLE (monotonic counter). The pool slot is
  // handle % num_bitmaps and the slot's epoch word is set to the handle,
  // so dequeue-time readers can detect recycling exactly (a message
  // whose slot was reused is hidden, never filtered against the wrong
  // bits). Callers put the handle in Rec.bitmap; the engine splits it
  // into (slot, epoch) before staging.
  u64 alloc_bitmap(py::buffer words) {
    py::buffer_info wi = words.request();
    if ((size_t)wi.size * wi.itemsize != g_.bitmap_words * sizeof(u64))
      throw std::invalid_argument("bitmap must be max_agents/64 u64 words");
    const u32 handle = bitmap_next_++;
    const u32 idx = handle % g_.num_bitmaps;
    // invalidate -> write bits -> publish epoch: an in-flight dequeue
    // never pairs the NEW bits with the OLD epoch (it sees EPOCH_NONE
    // and hides the message instead)
    const u32 none = EPOCH_NONE;
    HIP_CHECK(hipMemcpy(d_bitmap_epochs_ + idx, &none, sizeof(u32),
                        hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_bitmaps_ + (size_t)idx * g_.bitmap_words, wi.ptr,
                        g_.bitmap_words * sizeof(u64), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_bitmap_epochs_ + idx, &handle, sizeof(u32),
                        hipMemcpyHostToDevice));
    return handle;
  }

  // Read back one visibility-bitmap pool slot: (epoch, words bytes).
  // Checkpoint save uses this to persist the live bitmaps its records
  // reference (epoch mismatch => the caller's record is already hidden).
  py::tuple get_bitmap(u32 idx) {
    if (idx >= g_.num_bitmaps)
      throw std::out_of_range("bitmap index out of range");
    u32 epoch = 0;
    std::vector<u64> words(g_.bitmap_words);
    HIP_CHECK(hipMemcpy(&epoch, d_bitmap_epochs_ + idx, sizeof(u32),
                        hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(words.data(), d_bitmaps_ + (size_t)idx * g_.bitmap_words,
                        g_.bitmap_words * sizeof(u64), hipMemcpyDeviceToHost));
    return py::make_tuple(
        epoch, py::bytes(reinterpret_cast<const char *>(words.data()),
                         g_.bitmap_words * sizeof(u64)));
  }

  // ---- receive plane ----

  // Returns (counts[n_agents], seqs[n_agents * max_per_agent]) — one
  // dequeue-kernel launch for the whole poll tick.
  py::tuple receive_many(py::array_t<u32> agents, int max_per_agent,
                         bool priority, bool return_seqs = true) {
    const int na = (int)agents.size();
    if (na == 0)
      return py::make_tuple(py::array_t<u32>(0), py::array_t<u64>(0));
    if ((size_t)na * max_per_agent > out_pool_)
      throw std::invalid_argument("receive batch exceeds output pool");
    py::array_t<u32> counts(na);
    py::array_t<u64> seqs(return_seqs ? (size_t)na * max_per_agent : 0);
    {
      py::gil_scoped_release nogil;
      HIP_CHECK(hipMemcpyAsync(d_agents_, agents.data(), na * sizeof(u32),
                               hipMemcpyHostToDevice, stream_));
      hipLaunchKernelGGL(k_receive, dim3(na), dim3(256),
                         (g_.recv_window + 2) * sizeof(u64), stream_,
                         d_agents_,
                         na, max_per_agent, priority ? 1 : 0, evict_base_,
                         (const u64 *)nullptr,
                         d_hdr_, d_status_, d_inbox_, d_wpos_, d_rpos_,
                         d_carry_, d_carry_n_, d_bitmaps_, d_bitmap_epochs_,
                         d_out_seqs_, d_out_counts_, d_by_status_,
                         d_received_, g_);
      HIP_CHECK(hipMemcpyAsync(h_out_counts_, d_out_counts_, na * sizeof(u32),
                               hipMemcpyDeviceToHost, stream_));
      if (return_seqs)
        HIP_CHECK(hipMemcpyAsync(h_out_seqs_, d_out_seqs_,
                                 (size_t)na * max_per_agent * sizeof(u64),
                                 hipMemcpyDeviceToHost, stream_));
      HIP_CHECK(hipStreamSynchronize(stream_));
    }
    std::memcpy(counts.mutable_data(), h_out_counts_, na * sizeof(u32));
    if (return_seqs)
      std::memcpy(seqs.mutable_data(), h_out_seqs_,
                  (size_t)na * max_per_agent * sizeof(u64));
    last_recv_na_ = na;
    last_recv_K_ = max_per_agent;
    return py::make_tuple(counts, seqs);
  }

  // Deliver the payloads of the LAST receive_many/run_tick straight from
  // the device-resident output buffer. The host already holds the
  // counts, so it supplies the prefix offsets and the max per-agent
  // count (a device-side serial scan measured 0.5 ms at 8 k agents;
  // numpy does it in microseconds).
  u64 deliver_outbuf(py::array_t<u32> offsets, u32 total, u32 max_count,
                     u32 stride, bool synchronize) {
    if (total == 0 || last_recv_na_ == 0)
      return 0;
    if ((int)offsets.size() != last_recv_na_)
      throw std::invalid_argument("offsets must match the last receive");
    if (max_count == 0 || (int)max_count > last_recv_K_)
      max_count = last_recv_K_;
    if (stride == 0 || stride > g_.slot_bytes)
      stride = g_.slot_bytes;
    stride = (stride + 15u) & ~15u;
    if ((size_t)total * stride > (size_t)staging_batch_ * g_.slot_bytes)
      throw std::invalid_argument("delivery exceeds the pinned buffer");
    {
      py::gil_scoped_release nogil;
      HIP_CHECK(hipEventRecord(ev_, stream_));
      HIP_CHECK(hipStreamWaitEvent(copy_stream_, ev_, 0));
      HIP_CHECK(hipMemcpyAsync(d_unread_, offsets.data(),
                               last_recv_na_ * sizeof(u32),
                               hipMemcpyHostToDevice, copy_stream_));
      const int waves = last_recv_na_ * (int)max_count;
      hipLaunchKernelGGL(k_gather_outbuf, dim3((waves + 3) / 4), dim3(256), 0,
                         copy_stream_, d_out_seqs_, d_out_counts_, d_unread_,
                         last_recv_na_, last_recv_K_, (int)max_count, d_hdr_,
                         d_payload_, d_fetch_pay_, stride, g_);
      HIP_CHECK(hipMemcpyAsync(h_fetch_pay_, d_fetch_pay_,
                               (size_t)total * stride, hipMemcpyDeviceToHost,
                               copy_stream_));
      if (synchronize) {
        HIP_CHECK(hipStreamSynchronize(copy_stream_));
      } else {
        HIP_CHECK(hipEventRecord(d2h_ev_[d2h_cur_], copy_stream_));
        d2h_cur_ ^= 1;
        HIP_CHECK(hipEventSynchronize(d2h_ev_[d2h_cur_]));
        drain_spree();
      }
    }
    return (u64)total * stride;
  }

  // Device-resident delivery: dequeue + device scan + packed delivery
  // into CALLER-provided device buffers (torch tensors' data_ptr()), all
  // on stream_. Only the per-agent counts (na * 4 B) come back over
  // PCIe. Row r = offsets[b] + i gets payload[r*stride..), headers[r]
  // (48 B, payload_off rebased to r*stride), seqs[r] (i64), lengths[r]
  // and agent_row[r] (i32); offsets is u32[na + 1]. Every check runs
  // BEFORE the dequeue kernel, which advances cursors: a refused call
  // leaves the queue untouched. Synchronizes, so the buffers are safe on
  // any stream after return.
  py::array_t<u32> receive_to_device(py::array_t<u32> agents,
                                     int max_per_agent, bool priority,
                                     u32 stride, uintptr_t payload_ptr,
                                     uintptr_t headers_ptr, uintptr_t seqs_ptr,
                                     uintptr_t lengths_ptr,
                                     uintptr_t agent_row_ptr,
                                     uintptr_t offsets_ptr,
                                     size_t capacity_rows) {
    const int na = (int)agents.size();
    if (max_per_agent < 0)
      throw std::invalid_argument("max_per_agent must be >= 0");
    if ((u32)na > g_.max_agents)
      throw std::invalid_argument("more polled agents than max_agents");
    const size_t rows = (size_t)na * (size_t)max_per_agent;
    if (rows > out_pool_)
      throw std::invalid_argument("receive batch exceeds output pool");
    if (capacity_rows < rows)
      throw std::invalid_argument(
          "delivery buffers hold fewer than agents * max_per_agent rows");
    if (stride < 16 || stride > g_.slot_bytes || stride % 16 != 0)
      throw std::invalid_argument(
          "stride must be a multiple of 16 in 16..slot_bytes");
    if (!offsets_ptr || offsets_ptr % 4)
      throw std::invalid_argument("offsets buffer missing or misaligned");
    if (rows && (!payload_ptr || !headers_ptr || !seqs_ptr || !lengths_ptr ||
                 !agent_row_ptr))
      throw std::invalid_argument("delivery buffer pointer is null");
    if (payload_ptr % 16 || headers_ptr % 16 || seqs_ptr % 8 ||
        lengths_ptr % 4 || agent_row_ptr % 4)
      throw std::invalid_argument("delivery buffer is misaligned");
    const u32 *ap = agents.data();
    for (int i = 0; i < na; ++i)
      if (ap[i] >= g_.max_agents)
        throw std::invalid_argument("agent index out of range");
    py::array_t<u32> counts(na);
    if (na == 0)
      return counts;
    {
      py::gil_scoped_release nogil;
      HIP_CHECK(hipMemcpyAsync(d_agents_, ap, na * sizeof(u32),
                               hipMemcpyHostToDevice, stream_));
      hipLaunchKernelGGL(k_receive, dim3(na), dim3(256),
                         (g_.recv_window + 2) * sizeof(u64), stream_,
                         d_agents_, na, max_per_agent, priority ? 1 : 0,
                         evict_base_, (const u64 *)nullptr, d_hdr_, d_status_,
                         d_inbox_, d_wpos_, d_rpos_, d_carry_, d_carry_n_,
                         d_bitmaps_, d_bitmap_epochs_, d_out_seqs_,
                         d_out_counts_, d_by_status_, d_received_, g_);
      u32 *d_offsets = reinterpret_cast<u32 *>(offsets_ptr);
      hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(256), 4 * sizeof(u32),
                         stream_, d_out_counts_, na, d_offsets);
      // workgroups per agent: enough to give every wave one message,
      // capped where the whole grid already covers the machine
      const unsigned want = ((unsigned)max_per_agent + 3u) / 4u;
      const unsigned fill =
          (kDeliverBlocks + (unsigned)na - 1u) / (unsigned)na;
      const unsigned split = std::max(1u, std::min(want, fill));
      hipLaunchKernelGGL(k_deliver_device, dim3(na, split), dim3(256), 0,
                         stream_,
                         d_out_seqs_, d_out_counts_, d_offsets, na,
                         max_per_agent, d_hdr_, d_payload_,
                         reinterpret_cast<u8 *>(payload_ptr),
                         reinterpret_cast<uint4 *>(headers_ptr),
                         reinterpret_cast<long long *>(seqs_ptr),
                         reinterpret_cast<int *>(lengths_ptr),
                         reinterpret_cast<int *>(agent_row_ptr), stride, g_);
      HIP_CHECK(hipMemcpyAsync(h_out_counts_, d_out_counts_, na * sizeof(u32),
                               hipMemcpyDeviceToHost, stream_));
      HIP_CHECK(hipStreamSynchronize(stream_));
    }
    std::memcpy(counts.mutable_data(), h_out_counts_, na * sizeof(u32));
    last_recv_na_ = na;
    last_recv_K_ = max_per_agent;
    return counts;
  }

  // Mark `n` messages, named by an int64 device array, with `status`
  // without the seqs ever visiting the host (see k_ack_device for the
  // skip rules). Stream-ordered after the delivery; synchronizes.
  void ack_device(uintptr_t seqs_ptr, long long n, u32 status) {
    if (n < 0 || n > (long long)INT32_MAX)
      throw std::invalid_argument("ack count out of range");
    if (status >= (u32)N_STATUS)
      throw std::invalid_argument("unknown status code");
    if (n == 0)
      return;
    if (!seqs_ptr || seqs_ptr % 8)
      throw std::invalid_argument("seqs buffer missing or misaligned");
    py::gil_scoped_release nogil;
    hipLaunchKernelGGL(k_ack_device, dim3((unsigned)((n + 255) / 256)),
                       dim3(256), 0, stream_,
                       reinterpret_cast<const long long *>(seqs_ptr), (int)n,
                       status, evict_base_, count_, d_status_, d_by_status_,
                       g_);
    HIP_CHECK(hipStreamSynchronize(stream_));
  }

  // Conversation context of the first `total` rows of a device-resident
  // delivery (k_context_find has the rules), left in the caller's device
  // buffers: counts int32 [>= total], seqs int64 / lengths int32
  // [>= total, depth], headers [>= total, depth, 48] and payload
  // [>= total, depth, stride]. The polled agents are the only H2D and
  // nothing comes back. `type_code` < 0 means no filter; `group` picks
  // the rows per workgroup (0: CONTEXT_GROUP). The window bounds are the
  // host-tracked count_ / evict_base_ every kernel of stream_ is launched
  // with. Reads queue state only; every check runs before anything is
  // launched; synchronizes.
  void context_to_device(uintptr_t seqs_ptr, uintptr_t agent_row_ptr,
                         uintptr_t headers_ptr, long long total,
                         py::array_t<u32> agents, int depth,
                         long long lookback, int type_code, u32 stride,
                         uintptr_t counts_ptr, uintptr_t ctx_seqs_ptr,
                         uintptr_t ctx_lengths_ptr, uintptr_t ctx_headers_ptr,
                         uintptr_t ctx_payload_ptr, int group) {
    const int na = (int)agents.size();
    if (total < 0 || total > (1ll << 30) / CONTEXT_MAX_DEPTH)
      throw std::invalid_argument("context rows out of range");
    if (depth < 1 || depth > CONTEXT_MAX_DEPTH)
      throw std::invalid_argument("depth must be within 1..64");
    if (lookback < 1 || lookback > (long long)INT32_MAX)
      throw std::invalid_argument("lookback must be within 1..2^31-1");
    if (type_code > 255)
      throw std::invalid_argument("type is one byte");
    if ((u32)na > g_.max_agents)
      throw std::invalid_argument("more polled agents than max_agents");
    if (stride < 16 || stride > g_.slot_bytes || stride % 16 != 0)
      throw std::invalid_argument(
          "stride must be a multiple of 16 in 16..slot_bytes");
    if (group == 0)
      group = CONTEXT_GROUP;
    if (group != CONTEXT_GROUP && group != CONTEXT_GROUP_WIDE)
      throw std::invalid_argument("group must be 0, 4 or 16");
    if (total == 0)
      return;
    if (!seqs_ptr || !agent_row_ptr || !headers_ptr || !counts_ptr ||
        !ctx_seqs_ptr || !ctx_lengths_ptr || !ctx_headers_ptr ||
        !ctx_payload_ptr)
      throw std::invalid_argument("context buffer pointer is null");
    if (seqs_ptr % 8 || agent_row_ptr % 4 || headers_ptr % 16 ||
        counts_ptr % 4 || ctx_seqs_ptr % 8 || ctx_lengths_ptr % 4 ||
        ctx_headers_ptr % 16 || ctx_payload_ptr % 16)
      throw std::invalid_argument("context buffer is misaligned");
    py::gil_scoped_release nogil;
    if (na)
      HIP_CHECK(hipMemcpyAsync(d_agents_, agents.data(), na * sizeof(u32),
                               hipMemcpyHostToDevice, stream_));
    const long long n_slots = total * depth;
#define SWARMQ_CONTEXT_FIND(G)                                                 \
  hipLaunchKernelGGL(k_context_find<G>,                                        \
                     dim3((unsigned)((total + (G) - 1) / (G))), dim3(256), 0,  \
                     stream_, reinterpret_cast<const long long *>(seqs_ptr),   \
                     reinterpret_cast<const int *>(agent_row_ptr),             \
                     reinterpret_cast<const u32 *>(headers_ptr), (int)total,   \
                     d_agents_, na, depth, lookback, type_code, evict_base_,   \
                     count_, d_hdr_, d_status_,                                \
                     reinterpret_cast<int *>(counts_ptr),                      \
                     reinterpret_cast<long long *>(ctx_seqs_ptr),              \
                     reinterpret_cast<int *>(ctx_lengths_ptr), g_)
    if (group == CONTEXT_GROUP_WIDE)
      SWARMQ_CONTEXT_FIND(CONTEXT_GROUP_WIDE);
    else
      SWARMQ_CONTEXT_FIND(CONTEXT_GROUP);
#undef SWARMQ_CONTEXT_FIND
    hipLaunchKernelGGL(k_context_gather, dim3((unsigned)((n_slots + 3) / 4)),
                       dim3(256), 0, stream_,
                       reinterpret_cast<const long long *>(ctx_seqs_ptr),
                       n_slots, d_hdr_, d_payload_,
                       reinterpret_cast<u8 *>(ctx_payload_ptr),
                       reinterpret_cast<uint4 *>(ctx_headers_ptr),
                       reinterpret_cast<int *>(ctx_lengths_ptr), stride, g_);
    HIP_CHECK(hipStreamSynchronize(stream_));
  }

  // ---- message store ----

  // Returns (hdr bytes [n*48], status[n], payload bytes [n*slot_bytes]).
  py::tuple fetch(py::array_t<u64> seqs) {
    const int n = (int)seqs.size();
    if (n == 0)
      return py::make_tuple(py::bytes(""), py::array_t<u32>(0),
                            py::bytes(""));
    if ((u32)n > staging_batch_)
      throw std::invalid_argument("fetch batch exceeds staging_batch");
    {
      py::gil_scoped_release nogil;
      // order the gather after any in-flight enqueue on the main stream
      HIP_CHECK(hipEventRecord(ev_, stream_));
      HIP_CHECK(hipStreamWaitEvent(copy_stream_, ev_, 0));
      HIP_CHECK(hipMemcpyAsync(d_seqs_in_, seqs.data(), n * sizeof(u64),
                               hipMemcpyHostToDevice, copy_stream_));
      hipLaunchKernelGGL(k_gather, dim3((n + 3) / 4), dim3(256), 0,
                         copy_stream_, d_seqs_in_, n, d_hdr_, d_status_,
                         d_payload_, d_fetch_hdr_, d_fetch_status_,
                         d_fetch_pay_, evict_base_, g_.slot_bytes, g_);
      HIP_CHECK(hipMemcpyAsync(h_fetch_hdr_, d_fetch_hdr_, n * sizeof(Rec),
                               hipMemcpyDeviceToHost, copy_stream_));
      HIP_CHECK(hipMemcpyAsync(h_fetch_status_, d_fetch_status_,
                               n * sizeof(u32), hipMemcpyDeviceToHost,
                               copy_stream_));
      HIP_CHECK(hipMemcpyAsync(h_fetch_pay_, d_fetch_pay_,
                               (size_t)n * g_.slot_bytes,
                               hipMemcpyDeviceToHost, copy_stream_));
      HIP_CHECK(hipStreamSynchronize(copy_stream_));
    }
    py::array_t<u32> status(n);
    std::memcpy(status.mutable_data(), h_fetch_status_, n * sizeof(u32));
    return py::make_tuple(
        py::bytes(reinterpret_cast<const char *>(h_fetch_hdr_),
                  (size_t)n * sizeof(Rec)),
        status,
        py::bytes(reinterpret_cast<const char *>(h_fetch_pay_),
                  (size_t)n * g_.slot_bytes));
  }

  // Gather + D2H into pinned host memory WITHOUT building Python
  // objects — the hot-path delivery step (payload bytes land in host
  // RAM; zero per-message host work). Returns payload bytes landed.
  u64 fetch_raw(py::array_t<u64> seqs, u32 stride, bool synchronize) {
    const int n = (int)seqs.size();
    if (n == 0)
      return 0;
    if ((u32)n > staging_batch_)
      throw std::invalid_argument("fetch batch exceeds staging_batch");
    if (stride == 0 || stride > g_.slot_bytes)
      stride = g_.slot_bytes;
    stride = (stride + 15u) & ~15u;
    u64 bytes = 0;
    {
      py::gil_scoped_release nogil;
      HIP_CHECK(hipEventRecord(ev_, stream_));
      HIP_CHECK(hipStreamWaitEvent(copy_stream_, ev_, 0));
      HIP_CHECK(hipMemcpyAsync(d_seqs_in_, seqs.data(), n * sizeof(u64),
                               hipMemcpyHostToDevice, copy_stream_));
      hipLaunchKernelGGL(k_gather, dim3((n + 3) / 4), dim3(256), 0,
                         copy_stream_, d_seqs_in_, n, d_hdr_, d_status_,
                         d_payload_, d_fetch_hdr_, d_fetch_status_,
                         d_fetch_pay_, evict_base_, stride, g_);
      HIP_CHECK(hipMemcpyAsync(h_fetch_hdr_, d_fetch_hdr_, n * sizeof(Rec),
                               hipMemcpyDeviceToHost, copy_stream_));
      HIP_CHECK(hipMemcpyAsync(h_fetch_pay_, d_fetch_pay_,
                               (size_t)n * stride,
                               hipMemcpyDeviceToHost, copy_stream_));
      if (synchronize) {
        HIP_CHECK(hipStreamSynchronize(copy_stream_));
        for (int i = 0; i < n; ++i)
          bytes += h_fetch_hdr_[i].payload_len;
      } else {
        // bounded async pipeline: wait for the delivery issued two
        // calls ago before letting this one fly (an unbounded copy
        // stream backlog eventually hard-blocks the runtime for the
        // whole accumulated drain)
        HIP_CHECK(hipEventRecord(d2h_ev_[d2h_cur_], copy_stream_));
        d2h_cur_ ^= 1;
        HIP_CHECK(hipEventSynchronize(d2h_ev_[d2h_cur_]));
        drain_spree();
        bytes = (u64)n * stride; // upper bound; D2H still in flight
      }
    }
    return bytes;
  }

  void delivery_sync() {
    py::gil_scoped_release nogil;
    HIP_CHECK(hipStreamSynchronize(copy_stream_));
  }

  py::array_t<u32> get_statuses(py::array_t<u64> seqs) {
    const int n = (int)seqs.size();
    py::array_t<u32> out(n);
    if (n == 0)
      return out;
    if ((u32)n > staging_batch_)
      throw std::invalid_argument("status batch exceeds staging_batch");
    {
      py::gil_scoped_release nogil;
      HIP_CHECK(hipEventRecord(ev_, stream_));
      HIP_CHECK(hipStreamWaitEvent(copy_stream_, ev_, 0));
      HIP_CHECK(hipMemcpyAsync(d_seqs_in_, seqs.data(), n * sizeof(u64),
                               hipMemcpyHostToDevice, copy_stream_));
      hipLaunchKernelGGL(k_statuses, dim3((n + 255) / 256), dim3(256), 0,
                         copy_stream_, d_seqs_in_, n, evict_base_, d_status_,
                         d_fetch_status_, g_);
      HIP_CHECK(hipMemcpyAsync(h_fetch_status_, d_fetch_status_,
                               n * sizeof(u32), hipMemcpyDeviceToHost,
                               copy_stream_));
      HIP_CHECK(hipStreamSynchronize(copy_stream_));
    }
    std::memcpy(out.mutable_data(), h_fetch_status_, n * sizeof(u32));
    return out;
  }

  void set_statuses(py::array_t<u64> seqs, py::array_t<u32> sts) {
    const int n = (int)seqs.size();
    if (n == 0)
      return;
    if ((u32)n > staging_batch_)
      throw std::invalid_argument("status batch exceeds staging_batch");
    py::gil_scoped_release nogil;
    HIP_CHECK(hipMemcpyAsync(d_seqs_in_, seqs.data(), n * sizeof(u64),
                             hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipMemcpyAsync(d_choices_, sts.data(), n * sizeof(u32),
                             hipMemcpyHostToDevice, stream_));
    hipLaunchKernelGGL(k_set_statuses, dim3((n + 255) / 256), dim3(256), 0,
                       stream_, d_seqs_in_, d_choices_, n, d_status_,
                       d_by_status_, g_);
    HIP_CHECK(hipStreamSynchronize(stream_));
  }

  void set_status(u64 seq, u32 st) {
    hipLaunchKernelGGL(k_set_status, dim3(1), dim3(64), 0, stream_, seq, st,
                       d_status_, d_by_status_, g_);
    HIP_CHECK(hipStreamSynchronize(stream_));
  }

  u32 get_status(u64 seq) {
    if (seq < evict_base_ || seq >= count_)
      return ST_DELETED;
    u32 st;
    HIP_CHECK(hipMemcpy(&st, d_status_ + (seq % g_.num_slots), sizeof(u32),
                        hipMemcpyDeviceToHost));
    return st;
  }

  // Filter scan over [lo, hi); returns matched seqs (unordered).
  py::array_t<u64> query_range(u64 lo, u64 hi, int f_sender, int f_receiver,
                               int f_type, int f_status, double after,
                               double before, u32 pred_mask, u32 cap) {
    if (lo < evict_base_)
      lo = evict_base_;
    if (hi > count_)
      hi = count_;
    if (cap > staging_batch_)
      cap = staging_batch_;
    if (lo >= hi)
      return py::array_t<u64>(0);
    u32 nmatch = 0;
    {
      py::gil_scoped_release nogil;
      HIP_CHECK(hipMemsetAsync(d_match_count_, 0, sizeof(u32), stream_));
      const u64 span = hi - lo;
      const int blocks = (int)std::min<u64>((span + 255) / 256, 2048); // grid-stride
      hipLaunchKernelGGL(k_filter, dim3(blocks), dim3(256), 0, stream_, lo, hi,
                         f_sender, f_receiver, f_type, f_status, after, before,
                         pred_mask, d_hdr_, d_status_, d_match_,
                         d_match_count_, cap, g_);
      HIP_CHECK(hipMemcpyAsync(&nmatch, d_match_count_, sizeof(u32),
                               hipMemcpyDeviceToHost, stream_));
      HIP_CHECK(hipStreamSynchronize(stream_));
    }
    const u32 take = nmatch < cap ? nmatch : cap;
    py::array_t<u64> out(take);
    if (take)
      HIP_CHECK(hipMemcpy(out.mutable_data(), d_match_, take * sizeof(u64),
                          hipMemcpyDeviceToHost));
    return out;
  }

  py::array_t<u64> search_range(u64 lo, u64 hi, py::bytes needle, bool fold,
                                u32 cap) {
    std::string nd = needle;
    if (nd.empty() || nd.size() > 256)
      throw std::invalid_argument("needle must be 1..256 bytes");
    if (lo < evict_base_)
      lo = evict_base_;
    if (hi > count_)
      hi = count_;
    if (cap > staging_batch_)
      cap = staging_batch_;
    if (lo >= hi)
      return py::array_t<u64>(0);
    u32 nmatch = 0;
    {
      py::gil_scoped_release nogil;
      HIP_CHECK(hipMemcpyAsync(d_needle_, nd.data(), nd.size(),
                               hipMemcpyHostToDevice, stream_));
      HIP_CHECK(hipMemsetAsync(d_match_count_, 0, sizeof(u32), stream_));
      // the slot region of [lo, hi) is at most two contiguous byte
      // ranges (ring wraps once): launch a pure linear-scan kernel per
      // segment. Grid size A/B'd on hardware (see profiles/ and
      // csrc/bench_membw.hip).
      static const int sblocks = [] {
        const char *e = getenv("SWARMQ_SEARCH_BLOCKS");
        return e ? atoi(e) : 16384;
      }();
      const u32 cps = g_.slot_bytes >> 4;
      const u64 span = hi - lo;
      const u32 slot_lo = (u32)(lo % g_.num_slots);
      const u64 first = std::min<u64>(span, g_.num_slots - slot_lo);
      struct Seg {
        u64 off_slots, nslots, seq0;
        u32 slot0;
      } segs[2] = {{slot_lo, first, lo, slot_lo},
                   {0, span - first, lo + first, 0}};
      for (const Seg &s : segs) {
        if (s.nslots == 0)
          continue;
        const u64 chunks = s.nslots * cps;
        const int blocks =
            (int)std::min<u64>((chunks + 255) / 256, sblocks);
        static const int sP = [] {
          const char *e = getenv("SWARMQ_SEARCH_P");
          return e ? atoi(e) : 2; // hardware A/B winner (profiles/)
        }();
        auto kfn = k_search<2>;
        if (sP == 4)
          kfn = k_search<4>;
        else if (sP == 8)
          kfn = k_search<8>;
        hipLaunchKernelGGL(kfn, dim3(blocks), dim3(256), 0, stream_,
                           d_payload_ + s.off_slots * g_.slot_bytes, chunks,
                           s.seq0, s.slot0, d_needle_, (int)nd.size(),
                           fold ? 1 : 0, d_hdr_, d_status_, d_payload_,
                           d_match_, d_match_count_, cap, g_);
      }
      HIP_CHECK(hipMemcpyAsync(&nmatch, d_match_count_, sizeof(u32),
                               hipMemcpyDeviceToHost, stream_));
      HIP_CHECK(hipStreamSynchronize(stream_));
    }
    const u32 take = nmatch < cap ? nmatch : cap;
    py::array_t<u64> out(take);
    if (take)
      HIP_CHECK(hipMemcpy(out.mutable_data(), d_match_, take * sizeof(u64),
                          hipMemcpyDeviceToHost));
    return out;
  }

  // Inbox window for history listing (peek): returns (wpos, entries).
  py::tuple inbox_window(u32 agent) {
    check_agent(agent);
    ull w;
    HIP_CHECK(hipMemcpy(&w, d_wpos_ + agent, sizeof(ull),
                        hipMemcpyDeviceToHost));
    const ull start = w > g_.inbox_capacity ? w - g_.inbox_capacity : 0;
    const size_t nn = (size_t)(w - start);
    py::array_t<u64> out(nn);
    if (nn) {
      // the ring window may wrap; copy in up to two pieces
      std::vector<u64> tmp(nn);
      const u64 *base = d_inbox_ + (u64)agent * g_.inbox_capacity;
      const ull s_mod = start % g_.inbox_capacity;
      const size_t first = std::min<size_t>(nn, g_.inbox_capacity - s_mod);
      HIP_CHECK(hipMemcpy(tmp.data(), base + s_mod, first * sizeof(u64),
                          hipMemcpyDeviceToHost));
      if (first < nn)
        HIP_CHECK(hipMemcpy(tmp.data() + first, base, (nn - first) * sizeof(u64),
                            hipMemcpyDeviceToHost));
      std::memcpy(out.mutable_data(), tmp.data(), nn * sizeof(u64));
    }
    return py::make_tuple((u64)w, out);
  }

  py::array_t<u32> unread_counts(py::array_t<u32> agents) {
    const int na = (int)agents.size();
    py::array_t<u32> out(na);
    if (na == 0)
      return out;
    {
      py::gil_scoped_release nogil;
      HIP_CHECK(hipMemcpyAsync(d_agents_, agents.data(), na * sizeof(u32),
                               hipMemcpyHostToDevice, stream_));
      hipLaunchKernelGGL(k_unread, dim3(na), dim3(256), 0, stream_, d_agents_,
                         na, evict_base_, d_status_, d_inbox_, d_wpos_,
                         d_unread_, g_);
      HIP_CHECK(hipMemcpyAsync(h_out_counts_, d_unread_, na * sizeof(u32),
                               hipMemcpyDeviceToHost, stream_));
      HIP_CHECK(hipStreamSynchronize(stream_));
    }
    std::memcpy(out.mutable_data(), h_out_counts_, na * sizeof(u32));
    return out;
  }

  // ---- counters / stats ----

  py::dict counters() {
    py::array_t<u64> by_type(N_TYPES), by_status(N_STATUS);
    py::array_t<u64> sent(g_.max_agents), received(g_.max_agents);
    HIP_CHECK(hipMemcpy(by_type.mutable_data(), d_by_type_,
                        N_TYPES * sizeof(ull), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(by_status.mutable_data(), d_by_status_,
                        N_STATUS * sizeof(ull), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(sent.mutable_data(), d_sent_,
                        g_.max_agents * sizeof(ull), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(received.mutable_data(), d_received_,
                        g_.max_agents * sizeof(ull), hipMemcpyDeviceToHost));
    ull dropped = 0;
    HIP_CHECK(hipMemcpy(&dropped, d_dropped_, sizeof(ull),
                        hipMemcpyDeviceToHost));
    py::dict d;
    d["by_type"] = by_type;
    d["by_status"] = by_status;
    d["sent"] = sent;
    d["received"] = received;
    d["dropped"] = (u64)dropped; // inbox-ring overwrites of unread entries
    return d;
  }

  // ---- load balancer ----

  void backend_add_load(int idx, long long delta) {
    // balancer state is only touched by lb kernels — running them on
    // their own stream keeps dispatch from serializing against the
    // delivery tick under combined load
    hipLaunchKernelGGL(k_add_load, dim3(1), dim3(64), 0, lb_stream_, idx,
                       delta, d_backend_loads_);
    HIP_CHECK(hipStreamSynchronize(lb_stream_));
  }

  py::array_t<i64> backend_loads() {
    py::array_t<i64> out(g_.num_backends);
    HIP_CHECK(hipMemcpy(out.mutable_data(), d_backend_loads_,
                        g_.num_backends * sizeof(ull), hipMemcpyDeviceToHost));
    return out;
  }

  // Exact sequential least-loaded dispatch of `requests` requests;
  // returns the chosen backend per request.
  py::array_t<u32> lb_dispatch(int requests, int n_backends) {
    if (n_backends <= 0 || n_backends > 64)
      throw std::invalid_argument("1..64 backends supported");
    if ((u32)requests > staging_batch_)
      throw std::invalid_argument("too many requests per dispatch batch");
    py::array_t<u32> out(requests);
    {
      py::gil_scoped_release nogil;
      hipLaunchKernelGGL(k_lb_batch, dim3(1), dim3(64), 0, lb_stream_,
                         requests, n_backends, d_backend_loads_, d_lb_out_);
      HIP_CHECK(hipMemcpyAsync(h_choices_, d_lb_out_,
                               requests * sizeof(u32), hipMemcpyDeviceToHost,
                               lb_stream_));
      HIP_CHECK(hipStreamSynchronize(lb_stream_));
    }
    std::memcpy(out.mutable_data(), h_choices_, requests * sizeof(u32));
    return out;
  }

  // Dispatch the first `total` rows of a device-resident delivery to
  // `n_backends` backends (k_dispatch_rows has the rules), leaving
  // backend / rank / order ([>= total] int32), offsets ([n_backends + 1]
  // int32) and added ([n_backends] int64) in the caller's device buffers.
  // `pinned` is one word per polled agent (-1 or a backend) when
  // `has_pinned`; it is the only H2D, and the per-backend row counts
  // (4 * n_backends bytes) are the only D2H. `type_code` < 0 means no
  // filter. Runs on lb_stream_, ordered with every other user of the
  // load counters. Every check runs before anything is launched;
  // synchronizes.
  py::array_t<i64> dispatch_from_device(
      uintptr_t headers_ptr, uintptr_t agent_row_ptr, int total,
      py::array_t<int> pinned, bool has_pinned, int n_backends, int type_code,
      bool by_tokens, uintptr_t backend_ptr, uintptr_t rank_ptr,
      uintptr_t order_ptr, uintptr_t offsets_ptr, uintptr_t added_ptr) {
    check_dispatch_backends(n_backends);
    if (total < 0 || total > (1 << 30))
      throw std::invalid_argument("dispatch rows out of range");
    if (type_code > 255)
      throw std::invalid_argument("type is one byte");
    const int na = has_pinned ? (int)pinned.size() : 0;
    if ((u32)na > g_.max_agents)
      throw std::invalid_argument("more polled agents than max_agents");
    for (int i = 0; i < na; ++i)
      if (pinned.data()[i] < -1 || pinned.data()[i] >= n_backends)
        throw std::invalid_argument("pinned backend out of range");
    if (!offsets_ptr || !added_ptr)
      throw std::invalid_argument("dispatch buffer pointer is null");
    if (total > 0 && (!headers_ptr || !agent_row_ptr || !backend_ptr ||
                      !rank_ptr || !order_ptr))
      throw std::invalid_argument("dispatch buffer pointer is null");
    if (headers_ptr % 16 || agent_row_ptr % 4 || backend_ptr % 4 ||
        rank_ptr % 4 || order_ptr % 4 || offsets_ptr % 4 || added_ptr % 8)
      throw std::invalid_argument("dispatch buffer is misaligned");
    py::array_t<i64> out(n_backends);
    {
      py::gil_scoped_release nogil;
      if (na)
        HIP_CHECK(hipMemcpyAsync(d_disp_pinned_, pinned.data(),
                                 na * sizeof(int), hipMemcpyHostToDevice,
                                 lb_stream_));
      launch_dispatch_rows(
          reinterpret_cast<const uint4 *>(headers_ptr),
          reinterpret_cast<const int *>(agent_row_ptr), total,
          na ? d_disp_pinned_ : nullptr, na, n_backends, type_code,
          by_tokens ? 1 : 0, reinterpret_cast<int *>(backend_ptr),
          reinterpret_cast<int *>(rank_ptr),
          reinterpret_cast<ull *>(added_ptr),
          reinterpret_cast<int *>(offsets_ptr));
      if (total > 0)
        hipLaunchKernelGGL(k_dispatch_scatter, dim3((total + 255) / 256),
                           dim3(256), 0, lb_stream_,
                           reinterpret_cast<const int *>(backend_ptr),
                           reinterpret_cast<const int *>(rank_ptr),
                           reinterpret_cast<const int *>(offsets_ptr), total,
                           n_backends, reinterpret_cast<int *>(order_ptr));
      HIP_CHECK(hipMemcpyAsync(h_disp_counts_, d_disp_counts_,
                               n_backends * sizeof(u32), hipMemcpyDeviceToHost,
                               lb_stream_));
      HIP_CHECK(hipStreamSynchronize(lb_stream_));
    }
    i64 *o = out.mutable_data();
    for (int k = 0; k < n_backends; ++k)
      o[k] = (i64)h_disp_counts_[k];
    return out;
  }

  // loads[k] -= added[k] for the `added` tensor of an earlier dispatch.
  void release_dispatch(uintptr_t added_ptr, int n_backends) {
    check_dispatch_backends(n_backends);
    if (!added_ptr || added_ptr % 8)
      throw std::invalid_argument("added must be a non-null, 8-byte aligned "
                                  "device pointer");
    py::gil_scoped_release nogil;
    hipLaunchKernelGGL(k_release_loads, dim3(1), dim3(64), 0, lb_stream_,
                       d_backend_loads_,
                       reinterpret_cast<const ull *>(added_ptr), n_backends);
    HIP_CHECK(hipStreamSynchronize(lb_stream_));
  }

  // ---- accessors ----
  u64 total_messages() const { return count_; }
  u64 evict_base() const { return evict_base_; }
  u32 staging_batch() const { return staging_batch_; }
  u32 slot_bytes() const { return g_.slot_bytes; }
  u32 recv_window() const { return g_.recv_window; }
  size_t out_pool() const { return out_pool_; }

private:
  void check_dispatch_backends(int n_backends) const {
    if (n_backends < 1 || n_backends > 64 ||
        (u32)n_backends > g_.num_backends)
      throw std::invalid_argument(
          "n_backends must be within 1..min(64, num_backends)");
  }

  // k_dispatch_rows with the reduction depth n_backends needs: the
  // argmin's butterfly covers 2^levels >= n_backends lanes.
  void launch_dispatch_rows(const uint4 *headers, const int *agent_row,
                            int total, const int *pinned, int na,
                            int n_backends, int type_code, int by_tokens,
                            int *backend, int *rank, ull *added,
                            int *offsets) {
    int levels = 0;
    while ((1 << levels) < n_backends)
      ++levels;
#define SWARMQ_DISPATCH_ROWS(L)                                                \
  hipLaunchKernelGGL(k_dispatch_rows<L>, dim3(1), dim3(64), 0, lb_stream_,     \
                     headers, agent_row, total, pinned, na, n_backends,        \
                     type_code, by_tokens, d_backend_loads_, backend, rank,    \
                     added, d_disp_counts_, offsets)
    switch (levels) {
    case 0: SWARMQ_DISPATCH_ROWS(0); break;
    case 1: SWARMQ_DISPATCH_ROWS(1); break;
    case 2: SWARMQ_DISPATCH_ROWS(2); break;
    case 3: SWARMQ_DISPATCH_ROWS(3); break;
    case 4: SWARMQ_DISPATCH_ROWS(4); break;
    case 5: SWARMQ_DISPATCH_ROWS(5); break;
    default: SWARMQ_DISPATCH_ROWS(6); break;
    }
#undef SWARMQ_DISPATCH_ROWS
  }

  // Launch the enqueue kernel pair (+ fan-out) for n records at
  // `recs`/`pay` (device pointers) with host-known base seq; async on
  // stream_. Callers already reset d_bcast_count_.
  void launch_enqueue(const Rec *recs, const u8 *pay, int n, u64 base) {
    hipLaunchKernelGGL(k_enqueue_meta, dim3((n + 255) / 256), dim3(256), 0,
                       stream_, recs, n, base, (const u64 *)nullptr, d_hdr_,
                       d_status_, d_inbox_, d_wpos_, d_rpos_, d_by_type_,
                       d_by_status_, d_sent_, d_bcast_, d_bcast_count_,
                       d_dropped_, g_);
    hipLaunchKernelGGL(k_enqueue_payload, dim3((n + 3) / 4), dim3(256), 0,
                       stream_, recs, pay, n, base, (const u64 *)nullptr,
                       d_payload_, g_);
    hipLaunchKernelGGL(k_fanout, dim3((g_.max_agents + 255) / 256), dim3(256),
                       0, stream_, d_bcast_, d_bcast_count_, d_active_,
                       d_hdr_, d_bitmaps_, d_bitmap_epochs_, d_inbox_,
                       d_wpos_, d_rpos_, d_dropped_, g_);
  }

  void check_agent(u32 idx) const {
    if (idx >= g_.max_agents)
      throw std::out_of_range("agent index out of range");
  }

  // row stride of a device-side payload tensor: the bounds of a
  // delivery's stride
  void check_row_stride(u32 stride) const {
    if (stride < 16 || stride > g_.slot_bytes || stride % 16 != 0)
      throw std::invalid_argument(
          "stride must be a multiple of 16 in 16..slot_bytes");
  }

  // Streams driven only by event waits accumulate retired-command
  // bookkeeping inside the HIP runtime; the FIRST full
  // hipStreamSynchronize then pays one giant deferred cleanup
  // (measured: a 368 ms stall after 200k async ticks, ~2 s after 1M).
  // A full sync every kSpree async calls amortizes it to noise.
  void drain_spree() {
    if (++async_spree_ < kSpree)
      return;
    async_spree_ = 0;
    HIP_CHECK(hipStreamSynchronize(copy_stream_));
    HIP_CHECK(hipStreamSynchronize(h2d_stream_));
  }

  void ensure_stage_pay(size_t bytes) {
    if (bytes <= stage_pay_bytes_)
      return;
    size_t nb = stage_pay_bytes_;
    while (nb < bytes)
      nb *= 2;
    // all three streams may hold work against the staging buffers
    HIP_CHECK(hipStreamSynchronize(stream_));
    HIP_CHECK(hipStreamSynchronize(h2d_stream_));
    HIP_CHECK(hipStreamSynchronize(copy_stream_));
    for (int s = 0; s < 2; ++s) {
      HIP_CHECK(hipFree(d_stage_pay_[s]));
      (void)hipHostFree(h_pay_[s]);
      HIP_CHECK(hipMalloc(&d_stage_pay_[s], nb));
      HIP_CHECK(hipHostMalloc(&h_pay_[s], nb));
    }
    stage_pay_bytes_ = nb;
  }

  QueueGeom g_;
  int device_;
  u32 staging_batch_;
  u64 count_ = 0;
  u64 evict_base_ = 0;
  int last_recv_na_ = 0;
  int last_recv_K_ = 0;
  u32 bitmap_next_ = 0;
  bool released_ = false;
  size_t out_pool_ = 0;
  size_t stage_pay_bytes_ = 0;

  hipStream_t stream_{}, copy_stream_{}, h2d_stream_{}, lb_stream_{};
  hipEvent_t ev_{};
  hipEvent_t up_ev_[2] = {};
  hipEvent_t d2h_ev_[2] = {};
  int d2h_cur_ = 0;
  static constexpr int kSpree = 512;
  // k_deliver_device grid target: 256 CUs x 8 resident workgroups
  static constexpr unsigned kDeliverBlocks = 2048;
  int async_spree_ = 0;
  bool uploaded_[2] = {false, false};
  // captured steady-state tick (one exec per staging slot)
  hipGraphExec_t tick_exec_[2] = {};
  int tick_n_ = 0, tick_na_ = 0, tick_K_ = 0;
  u64 *d_dyn_{};   // [0]=tick base seq, [1]=evict base
  ull *d_tail_{};  // device-side total-messages counter

  Rec *d_hdr_{};
  u32 *d_status_{};
  u8 *d_payload_{};
  u64 *d_inbox_{};
  ull *d_wpos_{};
  ull *d_rpos_{};
  u64 *d_carry_{};
  u32 *d_carry_n_{};
  u32 *d_active_{};
  u64 *d_bitmaps_{};
  u32 *d_bitmap_epochs_{};
  ull *d_dropped_{};
  ull *d_by_type_{};
  ull *d_by_status_{};
  ull *d_sent_{};
  ull *d_received_{};
  u64 *d_bcast_{};
  u32 *d_bcast_count_{};
  ull *d_backend_loads_{};
  u32 *d_choices_{};
  u32 *d_lb_out_{};
  u64 *d_match_{};
  u32 *d_match_count_{};
  u8 *d_needle_{};
  u32 *d_agents_{};
  u32 *d_unread_{};
  u64 *d_out_seqs_{};
  u32 *d_out_counts_{};
  Rec *d_stage_recs_[2] = {};
  u8 *d_stage_pay_[2] = {};
  int staged_n_[2] = {0, 0};
  size_t staged_pay_[2] = {0, 0};
  hipEvent_t stage_ev_[2] = {};
  u64 *d_seqs_in_{};
  Rec *d_fetch_hdr_{};
  u32 *d_fetch_status_{};
  u8 *d_fetch_pay_{};
  Rec *d_dev_recs_{};   // sanitised records of the device-resident send
  u32 *d_reply_blk_{};  // kept rows per 256-row workgroup
  u32 *d_reply_off_{};  // their exclusive scan, [blocks] = m
  u32 *h_reply_m_{};
  int *d_disp_pinned_{};  // device-resident dispatch: pins per polled agent
  u32 *d_disp_counts_{};  // rows per backend
  u32 *h_disp_counts_{};

  Rec *h_recs_[2] = {};
  u8 *h_pay_[2] = {};
  u64 *h_out_seqs_{};
  u32 *h_out_counts_{};
  Rec *h_fetch_hdr_{};
  u32 *h_fetch_status_{};
  u8 *h_fetch_pay_{};
  u32 *h_choices_{};
};

// ---------------------------------------------------------------------------
// DoorbellQueue — persistent-kernel express lane for single-message
// latency (VERDICT round-1 item 5; the batched tick above is the
// throughput plane). A resident one-wavefront kernel polls a doorbell in
// pinned host memory; the host writes a message + rings, the kernel
// copies it into the receiver's pinned delivery ring and bumps a
// completion word the host spins on. No stream round-trips, no kernel
// launches on the message path: send->receive is two PCIe hops + one
// LDS-free wavefront copy.
//
// Replaces the reference's latency floor of linger.ms=10 + 1 s consumer
// polls ("swarmdb/ main.py":197, 557-558) for the p2p single-message
// regime (BASELINE config 2).
// ---------------------------------------------------------------------------

namespace {

// control block indices (u64 words in pinned host memory)
constexpr int DB_HEAD = 0;     // host writes: total submitted
constexpr int DB_STOP = 1;     // host writes 1 to stop the kernel
constexpr int DB_CONSUMED = 2; // device writes: total consumed
constexpr int DB_EXITED = 3;   // device writes 1 on exit
constexpr int DB_NWORDS = 8;

struct DoorGeom {
  u32 sub_cap;    // submit ring entries
  u32 n_agents;   // express agent slots
  u32 ring_cap;   // delivery ring entries per agent
  u32 slot_bytes; // payload bytes per entry (16-B multiple)
};

} // namespace

// One wavefront; lane 0 does the control-word traffic, all 64 lanes
// cooperate on payload copies. Self-terminates after max_cycles of
// 100 MHz s_memrealtime ticks so a wedged host can never leave the GPU
// spinning forever.
__global__ void k_doorbell(volatile ull *ctrl, const Rec *__restrict__ sub_recs,
                           const u8 *__restrict__ sub_pay,
                           Rec *__restrict__ del_recs, u8 *__restrict__ del_pay,
                           volatile ull *del_count,
                           volatile const ull *del_rpos,
                           ull *__restrict__ del_next,
                           ull *__restrict__ rpos_cache,
                           DoorGeom dg, unsigned long long max_cycles) {
  const int lane = threadIdx.x & 63;
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  u64 consumed = ctrl[DB_CONSUMED];
  for (;;) {
    u64 head, stop;
    if (lane == 0) {
      head = ctrl[DB_HEAD];
      stop = ctrl[DB_STOP];
    }
    head = __shfl(head, 0, 64);
    stop = __shfl(stop, 0, 64);
    if (stop)
      break;
    if (head == consumed) {
      if (__builtin_amdgcn_s_memrealtime() - t0 > max_cycles)
        break;
      __builtin_amdgcn_s_sleep(32);
      continue;
    }
    while (consumed < head) {
      const u32 i = (u32)(consumed % dg.sub_cap);
      // header: lane 0 reads + broadcasts the routing fields
      u64 recv_len;
      if (lane == 0) {
        const Rec &r = sub_recs[i];
        recv_len = ((u64)r.receiver << 32) | r.payload_len;
      }
      recv_len = __shfl(recv_len, 0, 64);
      const u32 recv = (u32)(recv_len >> 32);
      const u32 plen = (u32)recv_len;
      if (recv < dg.n_agents) {
        const u64 pos = del_next[recv];
        // delivery-ring back-pressure: never overwrite an entry the
        // host hasn't consumed. The host's read cursor lives in pinned
        // memory (PCIe-latency read), so a device-side cache
        // (rpos_cache) keeps the hot path free of host reads: refresh
        // only when the ring LOOKS full against the cache. A slow
        // consumer stalls the lane (the express plane assumes prompt
        // consumers); the wall-clock budget still bounds the kernel.
        u32 ok = 1;
        if (lane == 0 && pos - rpos_cache[recv] >= (u64)dg.ring_cap) {
          for (;;) {
            const u64 rp = del_rpos[recv];
            rpos_cache[recv] = rp;
            if (pos - rp < (u64)dg.ring_cap)
              break;
            if (ctrl[DB_STOP] ||
                __builtin_amdgcn_s_memrealtime() - t0 > max_cycles) {
              ok = 0;
              break;
            }
            __builtin_amdgcn_s_sleep(32);
          }
        }
        ok = __shfl(ok, 0, 64);
        if (!ok)
          break; // stop/timeout while full: exit without overwriting
        const u64 slot = (u64)recv * dg.ring_cap + (pos % dg.ring_cap);
        // payload copy: 64 lanes x 16 B per round
        const uint4 *src = reinterpret_cast<const uint4 *>(
            sub_pay + (u64)i * dg.slot_bytes);
        uint4 *dst =
            reinterpret_cast<uint4 *>(del_pay + slot * dg.slot_bytes);
        const u32 nchunk = (plen + 15u) >> 4;
        for (u32 c = lane; c < nchunk; c += 64)
          dst[c] = src[c];
        if (lane == 0) {
          del_recs[slot] = sub_recs[i];
          del_next[recv] = pos + 1;
        }
        // payload+header visible on the host BEFORE the counter bump
        __threadfence_system();
        if (lane == 0)
          del_count[recv] = pos + 1;
      }
      ++consumed;
    }
    if (lane == 0) {
      ctrl[DB_CONSUMED] = consumed;
      __threadfence_system();
    }
  }
  if (lane == 0) {
    ctrl[DB_CONSUMED] = consumed;
    __threadfence_system();
    ctrl[DB_EXITED] = 1;
  }
}

class DoorbellQueue {
public:
  DoorbellQueue(u32 slot_bytes, u32 sub_cap, u32 n_agents, u32 ring_cap,
                int device)
      : device_(device) {
    if (slot_bytes % 16 != 0)
      throw std::invalid_argument("slot_bytes must be a multiple of 16");
    dg_.slot_bytes = slot_bytes;
    dg_.sub_cap = sub_cap;
    dg_.n_agents = n_agents;
    dg_.ring_cap = ring_cap;
    HIP_CHECK(hipSetDevice(device_));
    HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    const unsigned flags = hipHostMallocCoherent | hipHostMallocMapped;
    HIP_CHECK(hipHostMalloc((void **)&h_ctrl_, DB_NWORDS * sizeof(ull), flags));
    HIP_CHECK(hipHostMalloc((void **)&h_sub_recs_,
                            (size_t)sub_cap * sizeof(Rec), flags));
    HIP_CHECK(hipHostMalloc((void **)&h_sub_pay_,
                            (size_t)sub_cap * slot_bytes, flags));
    HIP_CHECK(hipHostMalloc((void **)&h_del_recs_,
                            (size_t)n_agents * ring_cap * sizeof(Rec), flags));
    HIP_CHECK(hipHostMalloc((void **)&h_del_pay_,
                            (size_t)n_agents * ring_cap * slot_bytes, flags));
    HIP_CHECK(hipHostMalloc((void **)&h_del_count_,
                            (size_t)n_agents * sizeof(ull), flags));
    HIP_CHECK(hipHostMalloc((void **)&h_del_rpos_,
                            (size_t)n_agents * sizeof(ull), flags));
    std::memset((void *)h_ctrl_, 0, DB_NWORDS * sizeof(ull));
    std::memset((void *)h_del_count_, 0, (size_t)n_agents * sizeof(ull));
    std::memset((void *)h_del_rpos_, 0, (size_t)n_agents * sizeof(ull));
    // device-private per-agent delivery cursor + host-read-pos cache
    // (only the kernel touches these)
    HIP_CHECK(hipMalloc(&d_del_next_, (size_t)n_agents * sizeof(ull)));
    HIP_CHECK(hipMemset(d_del_next_, 0, (size_t)n_agents * sizeof(ull)));
    HIP_CHECK(hipMalloc(&d_del_rcache_, (size_t)n_agents * sizeof(ull)));
    HIP_CHECK(hipMemset(d_del_rcache_, 0, (size_t)n_agents * sizeof(ull)));
    read_pos_.assign(n_agents, 0);
    HIP_CHECK(hipHostGetDevicePointer((void **)&m_ctrl_, (void *)h_ctrl_, 0));
    HIP_CHECK(hipHostGetDevicePointer((void **)&m_sub_recs_, h_sub_recs_, 0));
    HIP_CHECK(hipHostGetDevicePointer((void **)&m_sub_pay_, h_sub_pay_, 0));
    HIP_CHECK(hipHostGetDevicePointer((void **)&m_del_recs_, h_del_recs_, 0));
    HIP_CHECK(hipHostGetDevicePointer((void **)&m_del_pay_, h_del_pay_, 0));
    HIP_CHECK(
        hipHostGetDevicePointer((void **)&m_del_count_, (void *)h_del_count_, 0));
    HIP_CHECK(
        hipHostGetDevicePointer((void **)&m_del_rpos_, (void *)h_del_rpos_, 0));
  }

  ~DoorbellQueue() { release(); }

  void release() {
    if (released_)
      return;
    released_ = true;
    if (running_)
      stop();
    (void)hipStreamDestroy(stream_);
    (void)hipFree(d_del_next_);
    (void)hipFree(d_del_rcache_);
    (void)hipHostFree((void *)h_del_rpos_);
    (void)hipHostFree((void *)h_ctrl_);
    (void)hipHostFree(h_sub_recs_);
    (void)hipHostFree(h_sub_pay_);
    (void)hipHostFree(h_del_recs_);
    (void)hipHostFree(h_del_pay_);
    (void)hipHostFree((void *)h_del_count_);
  }

  void start(double max_seconds = 60.0) {
    if (running_)
      return;
    h_ctrl_[DB_STOP] = 0;
    h_ctrl_[DB_EXITED] = 0;
    std::atomic_thread_fence(std::memory_order_seq_cst);
    // s_memrealtime ticks at 100 MHz on CDNA
    const unsigned long long max_cycles =
        (unsigned long long)(max_seconds * 100.0e6);
    hipLaunchKernelGGL(k_doorbell, dim3(1), dim3(64), 0, stream_, m_ctrl_,
                       m_sub_recs_, m_sub_pay_, m_del_recs_, m_del_pay_,
                       m_del_count_, m_del_rpos_, d_del_next_,
                       d_del_rcache_, dg_, max_cycles);
    HIP_CHECK(hipGetLastError());
    running_ = true;
  }

  void stop() {
    if (!running_)
      return;
    h_ctrl_[DB_STOP] = 1;
    std::atomic_thread_fence(std::memory_order_seq_cst);
    {
      py::gil_scoped_release nogil;
      HIP_CHECK(hipStreamSynchronize(stream_));
    }
    running_ = false;
  }

  bool running() const { return running_; }
  bool exited() const { return h_ctrl_[DB_EXITED] != 0; }
  u64 consumed() const { return h_ctrl_[DB_CONSUMED]; }
  u64 head() const { return sub_head_; }
  u64 delivered_count(u32 agent) const {
    return ((volatile ull *)h_del_count_)[agent];
  }
  u64 read_pos(u32 agent) const { return read_pos_[agent]; }

  // Submit one message to the express lane. Spins (bounded) if the ring
  // is full. Returns the express sequence number.
  u64 send(u32 receiver, u32 sender, py::buffer payload) {
    py::buffer_info pi = payload.request();
    const size_t n = (size_t)pi.size * pi.itemsize;
    if (n > dg_.slot_bytes)
      throw std::invalid_argument("payload exceeds the doorbell slot");
    if (receiver >= dg_.n_agents)
      throw std::out_of_range("receiver outside the express agent set");
    const u64 h = sub_head_;
    // bounded wait for ring space (the kernel is normally far ahead).
    // GIL released while spinning: the kernel may be stalled on a FULL
    // delivery ring, which only a consumer thread can drain — holding
    // the GIL here would deadlock multithreaded producers/consumers.
    if (h - h_ctrl_[DB_CONSUMED] >= dg_.sub_cap) {
      py::gil_scoped_release nogil;
      const auto t0 = std::chrono::steady_clock::now();
      while (h - h_ctrl_[DB_CONSUMED] >= dg_.sub_cap) {
        std::this_thread::yield();
        if (std::chrono::steady_clock::now() - t0 >
            std::chrono::seconds(5))
          throw std::runtime_error(
              "doorbell submit ring stalled for 5 s — kernel dead, or "
              "every consumer stopped draining (the delivery-ring "
              "back-pressure holds the kernel until try_recv runs)");
      }
    }
    const u32 i = (u32)(h % dg_.sub_cap);
    Rec r{};
    r.sender = sender;
    r.receiver = receiver;
    r.payload_len = (u32)n;
    r.content_len = (u32)n;
    std::memcpy(h_sub_pay_ + (size_t)i * dg_.slot_bytes, pi.ptr, n);
    h_sub_recs_[i] = r;
    std::atomic_thread_fence(std::memory_order_seq_cst);
    h_ctrl_[DB_HEAD] = h + 1; // the doorbell
    std::atomic_thread_fence(std::memory_order_seq_cst);
    sub_head_ = h + 1;
    return h;
  }

  // Non-blocking poll of an agent's delivery ring. Returns
  // (sender, payload bytes) or None. The read position is published
  // back to the kernel (delivery-ring back-pressure): entries are
  // never overwritten before the host consumed them.
  py::object try_recv(u32 agent) {
    if (agent >= dg_.n_agents)
      throw std::out_of_range("agent outside the express agent set");
    const u64 have = h_ctrl_exited_safe_count(agent);
    u64 &rp = read_pos_[agent];
    if (have == rp)
      return py::none();
    std::atomic_thread_fence(std::memory_order_seq_cst);
    const u64 slot = (u64)agent * dg_.ring_cap + (rp % dg_.ring_cap);
    const Rec r = h_del_recs_[slot];
    py::bytes pay(
        reinterpret_cast<const char *>(h_del_pay_ + slot * dg_.slot_bytes),
        r.payload_len);
    ++rp;
    std::atomic_thread_fence(std::memory_order_seq_cst);
    h_del_rpos_[agent] = rp; // release the slot to the kernel
    return py::make_tuple(r.sender, pay);
  }

  // Blocking receive with a spin deadline in microseconds. GIL released
  // while spinning so other threads can send.
  py::object recv_spin(u32 agent, double timeout_us) {
    if (agent >= dg_.n_agents)
      throw std::out_of_range("agent outside the express agent set");
    u64 &rp = read_pos_[agent];
    bool got = false;
    {
      py::gil_scoped_release nogil;
      const auto t0 = std::chrono::steady_clock::now();
      for (;;) {
        if (h_ctrl_exited_safe_count(agent) != rp) {
          got = true;
          break;
        }
        const auto el = std::chrono::duration_cast<std::chrono::microseconds>(
                            std::chrono::steady_clock::now() - t0)
                            .count();
        if ((double)el > timeout_us)
          break;
      }
    }
    if (!got)
      return py::none();
    return try_recv(agent);
  }

private:
  u64 h_ctrl_exited_safe_count(u32 agent) const {
    return ((volatile ull *)h_del_count_)[agent];
  }

  DoorGeom dg_;
  int device_;
  bool running_ = false;
  bool released_ = false;
  u64 sub_head_ = 0;
  hipStream_t stream_{};
  volatile ull *h_ctrl_{};
  Rec *h_sub_recs_{};
  u8 *h_sub_pay_{};
  Rec *h_del_recs_{};
  u8 *h_del_pay_{};
  volatile ull *h_del_count_{};
  volatile ull *h_del_rpos_{};
  ull *d_del_next_{};
  ull *d_del_rcache_{};
  std::vector<u64> read_pos_;
  // device-visible mappings of the pinned blocks
  volatile ull *m_ctrl_{};
  Rec *m_sub_recs_{};
  u8 *m_sub_pay_{};
  Rec *m_del_recs_{};
  u8 *m_del_pay_{};
  volatile ull *m_del_count_{};
  volatile ull *m_del_rpos_{};
};

// ---------------------------------------------------------------------------
// python module
// ---------------------------------------------------------------------------

PYBIND11_MODULE(_swarmq, m) {
  m.doc() = "MI355X-native GPU message-queue engine (CDNA4 HIP kernels)";
  m.attr("RECV_WINDOW") = RECV_WINDOW;
  m.attr("CONTEXT_GROUP") = CONTEXT_GROUP;
  m.attr("CONTEXT_GROUP_WIDE") = CONTEXT_GROUP_WIDE;

  m.def("device_count", []() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
      return 0;
    return n;
  });

  py::class_<DeviceQueue>(m, "DeviceQueue")
      .def(py::init<u32, u32, u32, u32, u32, u32, u32, int, u32>(),
           py::arg("num_slots"), py::arg("slot_bytes"), py::arg("max_agents"),
           py::arg("inbox_capacity"), py::arg("num_bitmaps"),
           py::arg("num_backends"), py::arg("staging_batch"),
           py::arg("device") = 0, py::arg("recv_window") = RECV_WINDOW)
      .def("register_agent", &DeviceQueue::register_agent)
      .def("deregister_agent", &DeviceQueue::deregister_agent)
      .def("active_agents", &DeviceQueue::active_agents)
      .def("enqueue_batch", &DeviceQueue::enqueue_batch)
      .def("enqueue_batch_async", &DeviceQueue::enqueue_batch_async)
      .def("sync", &DeviceQueue::sync)
      .def("stage_fill", &DeviceQueue::stage_fill)
      .def("enqueue_staged", &DeviceQueue::enqueue_staged)
      .def("prefetch_staged", &DeviceQueue::prefetch_staged)
      .def("prefetch_from", &DeviceQueue::prefetch_from)
      .def("build_tick", &DeviceQueue::build_tick)
      .def("run_tick", &DeviceQueue::run_tick)
      .def_static("alloc_pinned", &DeviceQueue::alloc_pinned)
      .def("alloc_bitmap", &DeviceQueue::alloc_bitmap)
      .def("get_bitmap", &DeviceQueue::get_bitmap)
      .def("pack_exchange", &DeviceQueue::pack_exchange)
      .def("enqueue_from_ptrs", &DeviceQueue::enqueue_from_ptrs)
      .def("enqueue_from_device", &DeviceQueue::enqueue_from_device,
           py::arg("headers_ptr"), py::arg("payload_ptr"), py::arg("n"),
           py::arg("stride"))
      .def("reply_from_device", &DeviceQueue::reply_from_device,
           py::arg("headers_ptr"), py::arg("agent_row_ptr"),
           py::arg("lengths_ptr"), py::arg("payload_ptr"), py::arg("total"),
           py::arg("rstride"), py::arg("agents"), py::arg("type_code"),
           py::arg("priority"), py::arg("flags"), py::arg("timestamp"))
      .def("receive_many", &DeviceQueue::receive_many, py::arg("agents"),
           py::arg("max_per_agent"), py::arg("priority"),
           py::arg("return_seqs") = true)
      .def("deliver_outbuf", &DeviceQueue::deliver_outbuf)
      .def("receive_to_device", &DeviceQueue::receive_to_device,
           py::arg("agents"), py::arg("max_per_agent"), py::arg("priority"),
           py::arg("stride"), py::arg("payload_ptr"), py::arg("headers_ptr"),
           py::arg("seqs_ptr"), py::arg("lengths_ptr"),
           py::arg("agent_row_ptr"), py::arg("offsets_ptr"),
           py::arg("capacity_rows"))
      .def("ack_device", &DeviceQueue::ack_device, py::arg("seqs_ptr"),
           py::arg("n"), py::arg("status"))
      .def("context_to_device", &DeviceQueue::context_to_device,
           py::arg("seqs_ptr"), py::arg("agent_row_ptr"),
           py::arg("headers_ptr"), py::arg("total"), py::arg("agents"),
           py::arg("depth"), py::arg("lookback"), py::arg("type_code"),
           py::arg("stride"), py::arg("counts_ptr"), py::arg("ctx_seqs_ptr"),
           py::arg("ctx_lengths_ptr"), py::arg("ctx_headers_ptr"),
           py::arg("ctx_payload_ptr"), py::arg("group") = 0)
      .def("fetch", &DeviceQueue::fetch)
      .def("fetch_raw", &DeviceQueue::fetch_raw, py::arg("seqs"),
           py::arg("stride") = 0, py::arg("synchronize") = true)
      .def("delivery_sync", &DeviceQueue::delivery_sync)
      .def("set_status", &DeviceQueue::set_status)
      .def("set_statuses", &DeviceQueue::set_statuses)
      .def("get_status", &DeviceQueue::get_status)
      .def("get_statuses", &DeviceQueue::get_statuses)
      .def("query_range", &DeviceQueue::query_range)
      .def("search_range", &DeviceQueue::search_range)
      .def("inbox_window", &DeviceQueue::inbox_window)
      .def("unread_counts", &DeviceQueue::unread_counts)
      .def("counters", &DeviceQueue::counters)
      .def("backend_add_load", &DeviceQueue::backend_add_load)
      .def("backend_loads", &DeviceQueue::backend_loads)
      .def("lb_dispatch", &DeviceQueue::lb_dispatch)
      .def("dispatch_from_device", &DeviceQueue::dispatch_from_device,
           py::arg("headers_ptr"), py::arg("agent_row_ptr"), py::arg("total"),
           py::arg("pinned"), py::arg("has_pinned"), py::arg("n_backends"),
           py::arg("type_code"), py::arg("by_tokens"), py::arg("backend_ptr"),
           py::arg("rank_ptr"), py::arg("order_ptr"), py::arg("offsets_ptr"),
           py::arg("added_ptr"))
      .def("release_dispatch", &DeviceQueue::release_dispatch,
           py::arg("added_ptr"), py::arg("n_backends"))
      .def("total_messages", &DeviceQueue::total_messages)
      .def("evict_base", &DeviceQueue::evict_base)
      .def("staging_batch", &DeviceQueue::staging_batch)
      .def("slot_bytes", &DeviceQueue::slot_bytes)
      .def("recv_window", &DeviceQueue::recv_window)
      .def("out_pool", &DeviceQueue::out_pool)
      .def("release", &DeviceQueue::release);

  py::class_<DoorbellQueue>(m, "DoorbellQueue")
      .def(py::init<u32, u32, u32, u32, int>(), py::arg("slot_bytes") = 1024,
           py::arg("sub_cap") = 1024, py::arg("n_agents") = 64,
           py::arg("ring_cap") = 256, py::arg("device") = 0)
      .def("start", &DoorbellQueue::start, py::arg("max_seconds") = 60.0)
      .def("stop", &DoorbellQueue::stop)
      .def("running", &DoorbellQueue::running)
      .def("exited", &DoorbellQueue::exited)
      .def("consumed", &DoorbellQueue::consumed)
      .def("head", &DoorbellQueue::head)
      .def("delivered_count", &DoorbellQueue::delivered_count)
      .def("read_pos", &DoorbellQueue::read_pos)
      .def("send", &DoorbellQueue::send, py::arg("receiver"),
           py::arg("sender"), py::arg("payload"))
      .def("try_recv", &DoorbellQueue::try_recv)
      .def("recv_spin", &DoorbellQueue::recv_spin, py::arg("agent"),
           py::arg("timeout_us") = 1e6)
      .def("release", &DoorbellQueue::release);
}
