#pragma once

#include "swarmq_util.h"

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
//
// SHARED (context_to_device(..., shared=True)) widens the pair rule to
// what one party wrote and the other was allowed to see: broadcasts
// count, and a VIS_BITMAP / VIS_GROUP record is judged as k_receive
// judges it for the OTHER party (never the author): no bitmap -> visible,
// except a VIS_GROUP broadcast, which k_fanout hands to nobody; a pool
// slot whose epoch moved on -> hidden; else that party's bit. Only log
// records are consulted, never the delivered row's own bitmap fields.

// Rows of a delivery one workgroup of k_context_find takes (CONTEXT_GROUP
// / 4 per wavefront). 4 — one row per wavefront — measured best on a
// 4096-row tick, where the call is bound by the serial chain of tiles a
// workgroup walks and not by the log reads the wider group saves; 16 is
// built too, for the comparison in profiles/device_context.md.
constexpr int CONTEXT_GROUP = 4;
constexpr int CONTEXT_GROUP_WIDE = 16;
constexpr int CONTEXT_TILE = 256;     // seqs per tile: one per thread
constexpr int CONTEXT_MAX_DEPTH = 64; // one lane per slot

// SHARED only: 1 loads the record's last 16 B (byte 32: payload_len,
// bitmap, content_len, bitmap_epoch) with the first, for every entry, so
// that it flies with the next tile's loads; 0 loads it at decode time,
// for a restricted candidate only. 0 measured 3 us faster on a 4096-row call
// over a log with 1/16 restricted broadcasts (139 against 142 us) and the
// same with none (profiles/device_context_shared.md), so it is the
// default.
#ifndef SWARMQ_CONTEXT_EAGER_VIS
#define SWARMQ_CONTEXT_EAGER_VIS 0
#endif

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
//
// SHARED: the thread that stages an entry also settles what does not
// depend on the row: it leaves in t_vis NO_BITMAP ("visible to all") or
// the live pool slot, and clears the candidate bit of an entry nobody can
// see. A lane that matches a restricted entry then loads the one bitmap
// word that holds the other party's bit, before the ballot. With SHARED
// false none of this is compiled and the bitmap pointers are not read.
template <int G, bool SHARED>
__global__ void __launch_bounds__(256)
    k_context_find(const long long *__restrict__ d_seqs,
                   const int *__restrict__ d_agent_row,
                   const u32 *__restrict__ d_headers, // 12 words per row
                   int total, const u32 *__restrict__ agents, int na,
                   int depth, long long lookback, int type_code,
                   u64 evict_base, u64 count, const Rec *__restrict__ hdr,
                   const u32 *__restrict__ status, int *__restrict__ out_counts,
                   long long *__restrict__ out_seqs,
                   int *__restrict__ out_lengths, QueueGeom g,
                   const u64 *__restrict__ bitmaps,
                   const u32 *__restrict__ bitmap_epochs) {
  static_assert(G % 4 == 0 && G >= 4, "G/4 rows per wavefront");
  constexpr int RPW = G / 4;
  __shared__ u32 t_sender[CONTEXT_TILE];
  __shared__ u32 t_receiver[CONTEXT_TILE];
  __shared__ u32 t_ok_type[CONTEXT_TILE]; // bit 8: candidate; bits 0..7: type
  __shared__ u32 t_vis[SHARED ? CONTEXT_TILE : 1]; // NO_BITMAP or pool slot
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
  // SHARED: `at` is the entry's record, `w` its last 16 B when loaded
  // here.
  auto load_tile = [&](long long t_top, uint4 &v, u32 &st, const Rec *&at,
                       uint4 &w) {
    v = make_uint4(0u, 0u, 0u, 0u);
    st = ST_DELETED;
    if constexpr (SHARED) {
      at = hdr;
      w = make_uint4(0u, 0u, 0u, 0u);
    }
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
    if constexpr (SHARED) {
      at = hdr + slot;
      if (SWARMQ_CONTEXT_EAGER_VIS)
        w = reinterpret_cast<const uint4 *>(at)[2];
    }
  };

  long long top = whi; // exclusive end of the next tile; whi == 0: no window
  uint4 v, w;
  u32 st;
  const Rec *at;
  load_tile(top, v, st, at, w);
  while (top > wlo) {
    const long long tlo = top - CONTEXT_TILE > wlo ? top - CONTEXT_TILE : wlo;
    const u32 type = v.z & 0xFFu;
    const u32 vis = (v.z >> 16) & 0xFFu;
    bool ok = st != ST_DELETED && st != ST_FAILED &&
              (SHARED || vis == VIS_ALL) &&
              (type_code < 0 || type == (u32)type_code);
    if constexpr (SHARED) {
      u32 pool = NO_BITMAP;
      if (ok && (vis == VIS_BITMAP || vis == VIS_GROUP)) {
        if (!SWARMQ_CONTEXT_EAGER_VIS)
          w = reinterpret_cast<const uint4 *>(at)[2];
        const u32 bm = w.y, epoch = w.w;
        if (bm == NO_BITMAP)
          ok = !(vis == VIS_GROUP && v.y == BROADCAST);
        else if (bm >= g.num_bitmaps || bitmap_epochs[bm] != epoch)
          ok = false; // recycled: hidden for good
        else
          pool = bm;
      }
      t_vis[tid] = pool;
    }
    t_sender[tid] = v.x;
    t_receiver[tid] = v.y;
    t_ok_type[tid] = (ok ? 0x100u : 0u) | type;
    __syncthreads();
    // the next (older) tile's loads fly while this one is tested
    load_tile(tlo, v, st, at, w);

    int open = 0; // a row of this wavefront may still take older seqs
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      if (rc[i] < depth && rlo[i] < rhi[i] && rhi[i] > tlo && rlo[i] < top) {
        for (int c = CONTEXT_TILE / 64 - 1; c >= 0 && rc[i] < depth; --c) {
          const int e = c * 64 + lane;
          const long long qe = tlo + e;
          const u32 es = t_sender[e], er = t_receiver[e];
          bool m = (t_ok_type[e] & 0x100u) && qe >= rlo[i] && qe < rhi[i] &&
                   qe < top;
          if constexpr (SHARED) {
            // written by s for a to see, or by a for s to see
            const bool to_a =
                es == rs[i] && (er == ra[i] || er == BROADCAST);
            const bool to_s =
                es == ra[i] && (er == rs[i] || er == BROADCAST);
            m = m && (to_a || to_s);
            const u32 pool = t_vis[e];
            if (m && pool != NO_BITMAP) {
              const u32 other = to_a ? ra[i] : rs[i];
              m = other < g.max_agents &&
                  ((bitmaps[(u64)pool * g.bitmap_words + (other >> 6)] >>
                    (other & 63)) &
                   1ull);
            }
          } else {
            m = m && ((es == rs[i] && er == ra[i]) ||
                      (es == ra[i] && er == rs[i]));
          }
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
  copy_row_masked(payload + h.payload_off, out_pay + (u64)o * stride, plen,
                  stride >> 4, lane);
  if (lane == 0) {
    store_rec_rebased(reinterpret_cast<Rec *>(out_hdr) + o, h,
                      (u64)o * stride);
  } else if (lane == 1) {
    out_len[o] = (int)plen;
  }
}
