#pragma once

#include "swarmq_util.h"

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
