#pragma once

#include "swarmq_util.h"

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
  Rec r;
  load_rec(r, src + (u64)i * 3);
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
