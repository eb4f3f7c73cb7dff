// swarmq_util.h — what every header of the extension leans on: the
// includes, HIP_CHECK, par_memcpy and the device helpers kernels share.
#pragma once

#include <hip/hip_runtime.h>

#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <thread>
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

// The device and pinned buffers of one queue object. A buffer is recorded
// where it is allocated and free_all() frees what was recorded, so a
// buffer cannot be made without an owner; a constructor that throws
// part-way frees what it had made through the same walk. A buffer that
// is regrown goes through dev_free / host_free and back through
// dev_alloc / host_alloc: the freed pointer leaves the record (and the
// member is nulled), the new one enters it.
struct HipBuffers {
  std::vector<void *> dev, host;

  // `count` elements of T; every byte set to `fill` unless it is negative
  template <class T> void dev_alloc(T *&p, size_t count, int fill = -1) {
    dev.emplace_back(); // the record exists before the buffer does
    HIP_CHECK(hipMalloc(&dev.back(), count * sizeof(T)));
    p = (T *)dev.back();
    if (fill >= 0)
      HIP_CHECK(hipMemset(dev.back(), fill, count * sizeof(T)));
  }

  template <class T>
  void host_alloc(T *&p, size_t count, unsigned flags = hipHostMallocDefault) {
    host.emplace_back();
    HIP_CHECK(hipHostMalloc(&host.back(), count * sizeof(T), flags));
    p = (T *)host.back();
  }

  template <class T> void dev_free(T *&p) {
    dev.erase(std::remove(dev.begin(), dev.end(), (void *)p), dev.end());
    (void)hipFree((void *)p);
    p = nullptr;
  }

  template <class T> void host_free(T *&p) {
    host.erase(std::remove(host.begin(), host.end(), (void *)p), host.end());
    (void)hipHostFree((void *)p);
    p = nullptr;
  }

  void free_all() {
    for (void *p : dev)
      (void)hipFree(p);
    for (void *p : host)
      (void)hipHostFree(p);
    dev.clear();
    host.clear();
  }
};

// ---- device helpers ---- The row copies are one wavefront per row, 64
// lanes x 16 B per round. No helper decides what to trust: the calling
// kernel clamps lengths and tests seqs first.

// Byte mask of the 32-bit word that starts at byte `first` of a 16-B
// chunk whose first `rem` bytes are live (little-endian).
__device__ __forceinline__ u32 tail_mask(u32 rem, u32 first) {
  if (rem >= first + 4)
    return ~0u;
  if (rem <= first)
    return 0u;
  return (1u << (8 * (rem - first))) - 1u;
}

// Plain copy of the 16-B chunks that hold `nbytes` bytes: the last chunk
// is copied whole, so up to 15 bytes past nbytes travel with it.
__device__ __forceinline__ void copy_chunks(const u8 *src, u8 *dst, u32 nbytes,
                                            u32 lane) {
  const uint4 *s = reinterpret_cast<const uint4 *>(src);
  uint4 *d = reinterpret_cast<uint4 *>(dst);
  const u32 nchunk = (nbytes + 15u) >> 4;
  for (u32 c = lane; c < nchunk; c += 64)
    d[c] = s[c];
}

// Fully defined row of `row_chunks` 16-B chunks: the first `plen` bytes
// (<= 16 * row_chunks), the chunk they end in masked there (a reused slot
// still holds its previous occupant's bytes), zeros to the end of the row.
__device__ __forceinline__ void copy_row_masked(const u8 *src, u8 *dst,
                                                u32 plen, u32 row_chunks,
                                                u32 lane) {
  const uint4 *s = reinterpret_cast<const uint4 *>(src);
  uint4 *d = reinterpret_cast<uint4 *>(dst);
  const u32 full = plen >> 4; // whole 16-B chunks
  const u32 rem = plen & 15u; // live bytes of the chunk after them
  for (u32 c = lane; c < row_chunks; c += 64) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (c < full) {
      v = s[c];
    } else if (c == full && rem) {
      v = s[c];
      // keep bytes [0, rem) of the chunk: word w holds bytes 4w..4w+3
      v.x &= tail_mask(rem, 0);
      v.y &= tail_mask(rem, 4);
      v.z &= tail_mask(rem, 8);
      v.w &= tail_mask(rem, 12);
    }
    d[c] = v;
  }
}

// A 48-B record as three 16-B stores / loads.
__device__ __forceinline__ void store_rec(Rec *dst, const Rec &r) {
  uint4 v[3];
  __builtin_memcpy(v, &r, sizeof(Rec));
  uint4 *o = reinterpret_cast<uint4 *>(dst);
  o[0] = v[0];
  o[1] = v[1];
  o[2] = v[2];
}

__device__ __forceinline__ void load_rec(Rec &r, const uint4 *src) {
  uint4 v[3];
  v[0] = src[0];
  v[1] = src[1];
  v[2] = src[2];
  __builtin_memcpy(&r, v, sizeof(Rec));
}

// Record `h` of a packed row: payload_off names the row's own payload.
__device__ __forceinline__ void store_rec_rebased(Rec *dst, const Rec &h,
                                                  u64 payload_off) {
  Rec r = h;
  r.payload_off = payload_off;
  store_rec(dst, r);
}

// Status word of `slot` := new_status, with the by_status counters moved
// exactly once however many threads swap the same slot.
__device__ __forceinline__ void swap_status(u32 *status, ull *by_status,
                                            u32 slot, u32 new_status) {
  const u32 old = atomicExch(&status[slot], new_status);
  if (old != new_status) {
    if (old < N_STATUS)
      atomicAdd(&by_status[old], (ull)(-1ll));
    if (new_status < N_STATUS)
      atomicAdd(&by_status[new_status], 1ull);
  }
}
