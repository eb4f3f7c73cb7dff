// Device-resident delivery: count scan, packed row delivery, device ack.
#pragma once

#include "swarmq_util.h"

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
    copy_row_masked(payload + h.payload_off, out_pay + r * stride, plen,
                    row_chunks, lane);
    if (lane == 0) {
      store_rec_rebased(reinterpret_cast<Rec *>(out_hdr) + r, h, r * stride);
    } else if (lane == 1) {
      out_seq[r] = (long long)seq;
    } else if (lane == 2) {
      out_len[r] = (int)plen;
    } else if (lane == 3) {
      out_row[r] = b;
    }
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
  swap_status(status, by_status, slot, new_status);
}
