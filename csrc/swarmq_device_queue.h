#pragma once

#include "swarmq_context.h"
#include "swarmq_delivery.h"
#include "swarmq_dispatch.h"
#include "swarmq_kernels.h"
#include "swarmq_send.h"

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

    try {
      init(num_slots, slot_bytes, max_agents, inbox_capacity, num_bitmaps,
           num_backends, staging_batch);
    } catch (...) {
      release(); // the destructor of a half-built object never runs
      throw;
    }
  }

  ~DeviceQueue() { release(); }

  // Idempotent, and tolerant of members that were never created (a
  // constructor that threw part-way). Every stream may hold work against
  // a buffer, so all four drain before anything is freed.
  void release() {
    if (released_)
      return;
    released_ = true;
    for (hipStream_t *s : streams())
      if (*s)
        (void)hipStreamSynchronize(*s);
    buf_.free_all();
    for (hipGraphExec_t &g : tick_exec_)
      if (g)
        (void)hipGraphExecDestroy(g);
    for (hipEvent_t *e : {&stage_ev_[0], &stage_ev_[1], &ev_, &up_ev_[0],
                          &up_ev_[1], &d2h_ev_[0], &d2h_ev_[1]})
      if (*e)
        (void)hipEventDestroy(*e);
    for (hipStream_t *s : streams())
      if (*s)
        (void)hipStreamDestroy(*s);
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
  // Fills and enqueues staging slot 0. Returns base seq. The stream sync
  // at the end is the DELIVERED ack.
  u64 enqueue_batch(py::buffer recs, py::buffer pay, int n) {
    py::buffer_info ri = recs.request(), pi = pay.request();
    if ((size_t)ri.size * ri.itemsize < (size_t)n * sizeof(Rec))
      throw std::invalid_argument("recs buffer too small");
    if (n <= 0)
      return count_;
    check_batch(n);
    fill_slot(0, ri, pi, n);
    const u64 base = enqueue_staged(0);
    sync();
    return base;
  }

  void sync() {
    py::gil_scoped_release nogil;
    HIP_CHECK(hipStreamSynchronize(stream_));
  }

  // ---- pipelined staging: fill one pinned set while the other's
  // H2D/kernels are in flight ----

  void stage_fill(int slot, py::buffer recs, py::buffer pay, int n) {
    check_slot(slot);
    check_batch(n);
    fill_slot(slot, recs.request(), pay.request(), n);
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
    check_slot(slot);
    check_batch(n);
    ensure_stage_pay(pay_bytes + 16);
    staged_n_[slot] = n;
    staged_pay_[slot] = pay_bytes;
    py::gil_scoped_release nogil;
    prefetch_slot(slot, reinterpret_cast<void *>(recs_ptr),
                  reinterpret_cast<void *>(pay_ptr));
  }

  // Upload a filled slot's staging buffers on the dedicated H2D stream
  // (overlaps the main stream's kernels and the copy stream's delivery
  // D2H — PCIe is full duplex). enqueue_staged picks the upload up.
  void prefetch_staged(int slot) {
    check_slot(slot);
    if (staged_n_[slot] <= 0)
      return;
    py::gil_scoped_release nogil;
    prefetch_slot(slot, h_recs_[slot], h_pay_[slot]);
  }

  // Launch H2D + enqueue kernels for a previously filled slot; returns
  // the base seq. NO sync — receive_many on the same stream is ordered
  // after it.
  u64 enqueue_staged(int slot) {
    check_slot(slot);
    const int n = staged_n_[slot];
    if (n <= 0)
      return count_;
    const u64 base = count_;
    {
      py::gil_scoped_release nogil;
      // already uploaded by a prefetch: order the kernels after it
      if (!wait_prefetch(slot))
        upload_slot(slot, h_recs_[slot], h_pay_[slot], stream_);
      launch_enqueue(d_stage_recs_[slot], d_stage_pay_[slot], n, base);
    }
    advance_count(base, (u64)n);
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
    check_polled(agents, K, true);
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
      // the reset goes ahead of k_tick_begin, where it always was
      HIP_CHECK(hipMemsetAsync(d_bcast_count_, 0, sizeof(u32), stream_));
      hipLaunchKernelGGL(k_tick_begin, dim3(1), dim3(64), 0, stream_, d_dyn_,
                         d_tail_, n, (u64)g_.num_slots);
      launch_enqueue(d_stage_recs_[s], d_stage_pay_[s], n, 0, d_dyn_, false);
      launch_receive(na, K, priority, 0, d_dyn_);
      counts_to_host(d_out_counts_, na);
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
    if (bad_slot(slot) || !tick_exec_[slot])
      throw std::invalid_argument("tick graph not built for this slot");
    py::array_t<u32> counts(tick_na_);
    py::array_t<u64> seqs((size_t)tick_na_ * tick_K_);
    {
      py::gil_scoped_release nogil;
      wait_prefetch(slot);
      HIP_CHECK(hipGraphLaunch(tick_exec_[slot], stream_));
      HIP_CHECK(hipStreamSynchronize(stream_));
    }
    advance_count(count_, (u64)tick_n_);
    return received(counts, seqs, tick_na_, tick_K_);
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
      launch_enqueue(reinterpret_cast<const Rec *>(recs_ptr),
                     reinterpret_cast<const u8 *>(pay_ptr), n, base);
    }
    advance_count(base, (u64)n);
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
    check_dev_ptrs({{headers_ptr, 16}, {payload_ptr, 16}}, true,
                   "send buffer pointer is null", "send buffer is misaligned");
    const u64 base = count_;
    {
      py::gil_scoped_release nogil;
      hipLaunchKernelGGL(k_stage_device, dim3((n + 255) / 256), dim3(256), 0,
                         stream_, reinterpret_cast<const uint4 *>(headers_ptr),
                         n, stride, g_.num_bitmaps, d_dev_recs_);
      launch_enqueue(d_dev_recs_, reinterpret_cast<const u8 *>(payload_ptr), n,
                     base);
      HIP_CHECK(hipStreamSynchronize(stream_));
    }
    advance_count(base, (u64)n);
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
    check_polled(agents, 0, false);
    if (priority > 255 || type_code > 255u || flags > 255u)
      throw std::invalid_argument("type, priority and flags are one byte");
    if (total == 0)
      return py::make_tuple(count_, 0u);
    check_dev_ptrs({{headers_ptr, 16}, {payload_ptr, 16}, {agent_row_ptr, 4},
                    {lengths_ptr, 4}},
                   true, "reply buffer pointer is null",
                   "reply buffer is misaligned");
    const u64 base = count_;
    const int nblk = (total + 255) / 256;
    u32 m = 0;
    {
      py::gil_scoped_release nogil;
      const int *d_len = reinterpret_cast<const int *>(lengths_ptr);
      upload_agents(agents.data(), na);
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
        launch_enqueue(d_dev_recs_, reinterpret_cast<const u8 *>(payload_ptr),
                       (int)m, base);
        HIP_CHECK(hipStreamSynchronize(stream_));
      }
    }
    advance_count(base, (u64)m);
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
    check_polled(agents, max_per_agent, true);
    if (na == 0)
      return py::make_tuple(py::array_t<u32>(0), py::array_t<u64>(0));
    if ((size_t)na * max_per_agent > out_pool_)
      throw std::invalid_argument("receive batch exceeds output pool");
    py::array_t<u32> counts(na);
    py::array_t<u64> seqs(return_seqs ? (size_t)na * max_per_agent : 0);
    {
      py::gil_scoped_release nogil;
      upload_agents(agents.data(), na);
      launch_receive(na, max_per_agent, priority, evict_base_, nullptr);
      counts_to_host(d_out_counts_, na);
      if (return_seqs)
        HIP_CHECK(hipMemcpyAsync(h_out_seqs_, d_out_seqs_,
                                 (size_t)na * max_per_agent * sizeof(u64),
                                 hipMemcpyDeviceToHost, stream_));
      HIP_CHECK(hipStreamSynchronize(stream_));
    }
    return received(counts, seqs, na, max_per_agent);
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
    stride = clamp_stride(stride);
    if ((size_t)total * stride > (size_t)staging_batch_ * g_.slot_bytes)
      throw std::invalid_argument("delivery exceeds the pinned buffer");
    {
      py::gil_scoped_release nogil;
      copy_after_main();
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
      finish_delivery(synchronize);
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
    check_polled(agents, max_per_agent, true);
    const size_t rows = (size_t)na * (size_t)max_per_agent;
    if (rows > out_pool_)
      throw std::invalid_argument("receive batch exceeds output pool");
    if (capacity_rows < rows)
      throw std::invalid_argument(
          "delivery buffers hold fewer than agents * max_per_agent rows");
    check_row_stride(stride);
    check_dev_ptrs({{offsets_ptr, 4}}, true,
                   "offsets buffer missing or misaligned");
    check_dev_ptrs({{payload_ptr, 16}, {headers_ptr, 16}, {seqs_ptr, 8},
                    {lengths_ptr, 4}, {agent_row_ptr, 4}},
                   rows != 0, "delivery buffer pointer is null",
                   "delivery buffer is misaligned");
    const u32 *ap = agents.data();
    py::array_t<u32> counts(na);
    if (na == 0)
      return counts;
    {
      py::gil_scoped_release nogil;
      upload_agents(ap, na);
      launch_receive(na, max_per_agent, priority, evict_base_, nullptr);
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
      counts_to_host(d_out_counts_, na);
      HIP_CHECK(hipStreamSynchronize(stream_));
    }
    last_recv_na_ = na;
    last_recv_K_ = max_per_agent;
    return host_counts(counts);
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
    check_dev_ptrs({{seqs_ptr, 8}}, true, "seqs buffer missing or misaligned");
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
  // the rows per workgroup (0: CONTEXT_GROUP); `shared` the instantiation
  // that checks visibility against the bitmap pool. The window bounds are the
  // host-tracked count_ / evict_base_ every kernel of stream_ is launched
  // with. Reads queue state only; every check runs before anything is
  // launched; synchronizes.
  void context_to_device(uintptr_t seqs_ptr, uintptr_t agent_row_ptr,
                         uintptr_t headers_ptr, long long total,
                         py::array_t<u32> agents, int depth,
                         long long lookback, int type_code, u32 stride,
                         uintptr_t counts_ptr, uintptr_t ctx_seqs_ptr,
                         uintptr_t ctx_lengths_ptr, uintptr_t ctx_headers_ptr,
                         uintptr_t ctx_payload_ptr, int group, bool shared) {
    const int na = (int)agents.size();
    if (total < 0 || total > (1ll << 30) / CONTEXT_MAX_DEPTH)
      throw std::invalid_argument("context rows out of range");
    if (depth < 1 || depth > CONTEXT_MAX_DEPTH)
      throw std::invalid_argument("depth must be within 1..64");
    if (lookback < 1 || lookback > (long long)INT32_MAX)
      throw std::invalid_argument("lookback must be within 1..2^31-1");
    if (type_code > 255)
      throw std::invalid_argument("type is one byte");
    check_polled(agents, 0, false);
    check_row_stride(stride);
    if (group == 0)
      group = CONTEXT_GROUP;
    if (group != CONTEXT_GROUP && group != CONTEXT_GROUP_WIDE)
      throw std::invalid_argument("group must be 0, 4 or 16");
    if (total == 0)
      return;
    check_dev_ptrs({{seqs_ptr, 8}, {agent_row_ptr, 4}, {headers_ptr, 16},
                    {counts_ptr, 4}, {ctx_seqs_ptr, 8}, {ctx_lengths_ptr, 4},
                    {ctx_headers_ptr, 16}, {ctx_payload_ptr, 16}},
                   true, "context buffer pointer is null",
                   "context buffer is misaligned");
    py::gil_scoped_release nogil;
    upload_agents(agents.data(), na);
    const long long n_slots = total * depth;
#define SWARMQ_CONTEXT_FIND(G, SHARED)                                         \
  hipLaunchKernelGGL((k_context_find<G, SHARED>),                              \
                     dim3((unsigned)((total + (G) - 1) / (G))), dim3(256), 0,  \
                     stream_, reinterpret_cast<const long long *>(seqs_ptr),   \
                     reinterpret_cast<const int *>(agent_row_ptr),             \
                     reinterpret_cast<const u32 *>(headers_ptr), (int)total,   \
                     d_agents_, na, depth, lookback, type_code, evict_base_,   \
                     count_, d_hdr_, d_status_,                                \
                     reinterpret_cast<int *>(counts_ptr),                      \
                     reinterpret_cast<long long *>(ctx_seqs_ptr),              \
                     reinterpret_cast<int *>(ctx_lengths_ptr), g_, d_bitmaps_, \
                     d_bitmap_epochs_)
    if (group == CONTEXT_GROUP_WIDE && shared)
      SWARMQ_CONTEXT_FIND(CONTEXT_GROUP_WIDE, true);
    else if (group == CONTEXT_GROUP_WIDE)
      SWARMQ_CONTEXT_FIND(CONTEXT_GROUP_WIDE, false);
    else if (shared)
      SWARMQ_CONTEXT_FIND(CONTEXT_GROUP, true);
    else
      SWARMQ_CONTEXT_FIND(CONTEXT_GROUP, false);
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
      gather_to_host(seqs.data(), n, g_.slot_bytes, true);
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
    stride = clamp_stride(stride);
    py::gil_scoped_release nogil;
    gather_to_host(seqs.data(), n, stride, false);
    finish_delivery(synchronize);
    if (!synchronize)
      return (u64)n * stride; // upper bound; D2H still in flight
    u64 bytes = 0;
    for (int i = 0; i < n; ++i)
      bytes += h_fetch_hdr_[i].payload_len;
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
      copy_after_main();
      HIP_CHECK(hipMemcpyAsync(d_seqs_in_, seqs.data(), n * sizeof(u64),
                               hipMemcpyHostToDevice, copy_stream_));
      hipLaunchKernelGGL(k_statuses, dim3((n + 255) / 256), dim3(256), 0,
                         copy_stream_, d_seqs_in_, n, evict_base_, count_,
                         d_status_, d_fetch_status_, g_);
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
                       stream_, d_seqs_in_, d_choices_, n, evict_base_, count_,
                       d_status_, d_by_status_, g_);
    HIP_CHECK(hipStreamSynchronize(stream_));
  }

  void set_status(u64 seq, u32 st) {
    hipLaunchKernelGGL(k_set_status, dim3(1), dim3(64), 0, stream_, seq, st,
                       evict_base_, count_, d_status_, d_by_status_, g_);
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
  // `max_blocks` > 0 caps the grid (a test's way into the grid-stride
  // loop at a small size); 0 is the production cap.
  py::array_t<u64> query_range(u64 lo, u64 hi, int f_sender, int f_receiver,
                               int f_type, int f_status, double after,
                               double before, u32 pred_mask, u32 cap,
                               int max_blocks) {
    if (max_blocks < 0)
      throw std::invalid_argument("blocks must be >= 0");
    if (!clamp_scan(lo, hi, cap))
      return py::array_t<u64>(0);
    {
      py::gil_scoped_release nogil;
      HIP_CHECK(hipMemsetAsync(d_match_count_, 0, sizeof(u32), stream_));
      const u64 span = hi - lo;
      const int blocks = (int)std::min<u64>(
          (span + 255) / 256, max_blocks ? max_blocks : 2048); // grid-stride
      hipLaunchKernelGGL(k_filter, dim3(blocks), dim3(256), 0, stream_, lo, hi,
                         f_sender, f_receiver, f_type, f_status, after, before,
                         pred_mask, d_hdr_, d_status_, d_match_,
                         d_match_count_, cap, g_);
    }
    return read_matches(cap);
  }

  // Substring scan over [lo, hi); returns matched seqs (unordered, a seq
  // possibly once per matching chunk). `max_blocks` > 0 caps each
  // segment's grid and `loads` in {2,4,8} picks k_search<loads> (a test's
  // way into the pipelined loop and the other instantiations at a small
  // size); 0 is the production choice: SWARMQ_SEARCH_BLOCKS /
  // SWARMQ_SEARCH_P where they hold a usable value, else the measured
  // defaults.
  py::array_t<u64> search_range(u64 lo, u64 hi, py::bytes needle, bool fold,
                                u32 cap, int max_blocks, int loads) {
    std::string nd = needle;
    if (nd.empty() || nd.size() > 256)
      throw std::invalid_argument("needle must be 1..256 bytes");
    if (max_blocks < 0)
      throw std::invalid_argument("blocks must be >= 0");
    if (loads != 0 && loads != 2 && loads != 4 && loads != 8)
      throw std::invalid_argument("loads must be 0, 2, 4 or 8");
    if (!clamp_scan(lo, hi, cap))
      return py::array_t<u64>(0);
    {
      py::gil_scoped_release nogil;
      HIP_CHECK(hipMemcpyAsync(d_needle_, nd.data(), nd.size(),
                               hipMemcpyHostToDevice, stream_));
      HIP_CHECK(hipMemsetAsync(d_match_count_, 0, sizeof(u32), stream_));
      // the slot region of [lo, hi) is at most two contiguous byte
      // ranges (ring wraps once): launch a pure linear-scan kernel per
      // segment. Grid size A/B'd on hardware (see profiles/ and
      // csrc/bench_membw.hip).
      // an env value that is no positive block count (or no load count
      // of a compiled kernel) never reaches the launch: a zero-block
      // grid is a launch error
      static const int env_blocks = [] {
        const long v = env_long("SWARMQ_SEARCH_BLOCKS");
        return v > 0 && v <= INT_MAX ? (int)v : 16384;
      }();
      static const int env_loads = [] {
        const long v = env_long("SWARMQ_SEARCH_P");
        return v == 4 || v == 8 ? (int)v : 2; // hardware A/B winner (profiles/)
      }();
      const int sblocks = max_blocks ? max_blocks : env_blocks;
      const int sP = loads ? loads : env_loads;
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
    }
    return read_matches(cap);
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
    check_polled(agents, 0, false);
    py::array_t<u32> out(na);
    if (na == 0)
      return out;
    {
      py::gil_scoped_release nogil;
      upload_agents(agents.data(), na);
      hipLaunchKernelGGL(k_unread, dim3(na), dim3(256), 0, stream_, d_agents_,
                         na, evict_base_, d_status_, d_inbox_, d_wpos_,
                         d_unread_, g_);
      counts_to_host(d_unread_, na);
      HIP_CHECK(hipStreamSynchronize(stream_));
    }
    return host_counts(out);
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
    check_dev_ptrs({{headers_ptr, 16}, {agent_row_ptr, 4}, {backend_ptr, 4},
                    {rank_ptr, 4}, {order_ptr, 4}, {offsets_ptr, 4},
                    {added_ptr, 8}},
                   total > 0, "dispatch buffer pointer is null",
                   "dispatch buffer is misaligned");
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
    check_dev_ptrs({{added_ptr, 8}}, true,
                   "added must be a non-null, 8-byte aligned device pointer");
    py::gil_scoped_release nogil;
    hipLaunchKernelGGL(k_release_loads, dim3(1), dim3(64), 0, lb_stream_,
                       d_backend_loads_,
                       reinterpret_cast<const ull *>(added_ptr), n_backends);
    HIP_CHECK(hipStreamSynchronize(lb_stream_));
  }

  // ---- accessors ----
  u64 total_messages() const { return count_; }
  u64 evict_base() const { return evict_base_; }
  size_t out_pool() const { return out_pool_; }

private:
  std::array<hipStream_t *, 4> streams() {
    return {&stream_, &copy_stream_, &h2d_stream_, &lb_stream_};
  }

  static void new_event(hipEvent_t &e) {
    HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }

  // Everything the queue owns, made in one fixed order: the position of
  // each buffer matters to the measured paths (profiles/device_send.md),
  // so new buffers go at the end. Buffers made without a fill value are
  // written before they are read.
  void init(u32 num_slots, u32 slot_bytes, u32 max_agents, u32 inbox_capacity,
            u32 num_bitmaps, u32 num_backends, u32 staging_batch) {
    HIP_CHECK(hipSetDevice(device_));
    for (hipStream_t *s : streams())
      HIP_CHECK(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
    for (hipEvent_t *e :
         {&ev_, &up_ev_[0], &up_ev_[1], &d2h_ev_[0], &d2h_ev_[1]})
      new_event(*e);

    // device state
    buf_.dev_alloc(d_hdr_, num_slots);
    buf_.dev_alloc(d_status_, num_slots, 0);
    buf_.dev_alloc(d_payload_, (size_t)num_slots * slot_bytes);
    buf_.dev_alloc(d_inbox_, (size_t)max_agents * inbox_capacity);
    buf_.dev_alloc(d_wpos_, max_agents, 0);
    buf_.dev_alloc(d_rpos_, max_agents, 0);
    buf_.dev_alloc(d_carry_, (size_t)max_agents * g_.recv_window);
    buf_.dev_alloc(d_carry_n_, max_agents, 0);
    buf_.dev_alloc(d_active_, max_agents, 0);
    buf_.dev_alloc(d_bitmaps_, (size_t)num_bitmaps * g_.bitmap_words);
    buf_.dev_alloc(d_bitmap_epochs_, num_bitmaps, 0xFF); // all EPOCH_NONE
    buf_.dev_alloc(d_dropped_, 1, 0);
    buf_.dev_alloc(d_by_type_, N_TYPES, 0);
    buf_.dev_alloc(d_by_status_, N_STATUS, 0);
    buf_.dev_alloc(d_sent_, max_agents, 0);
    buf_.dev_alloc(d_received_, max_agents, 0);
    buf_.dev_alloc(d_bcast_, staging_batch);
    buf_.dev_alloc(d_bcast_count_, 1);
    buf_.dev_alloc(d_backend_loads_, num_backends, 0);
    buf_.dev_alloc(d_choices_, staging_batch);
    buf_.dev_alloc(d_lb_out_, staging_batch);
    buf_.dev_alloc(d_match_, staging_batch);
    buf_.dev_alloc(d_match_count_, 1);
    buf_.dev_alloc(d_needle_, 256);
    buf_.dev_alloc(d_agents_, max_agents);
    buf_.dev_alloc(d_unread_, max_agents);

    buf_.dev_alloc(d_dyn_, 2);
    buf_.dev_alloc(d_tail_, 1, 0);
    out_pool_ = (size_t)4 << 20; // receive output pool: 4M entries, 32 MB
    buf_.dev_alloc(d_out_seqs_, out_pool_);
    buf_.dev_alloc(d_out_counts_, max_agents);

    // staging (device side of the H2D batch), double-buffered so the
    // host can fill batch i+1 while batch i's H2D/kernels run
    stage_pay_bytes_ = (size_t)staging_batch * 1024; // grows on demand
    for (int s = 0; s < 2; ++s) {
      buf_.dev_alloc(d_stage_recs_[s], staging_batch);
      buf_.dev_alloc(d_stage_pay_[s], stage_pay_bytes_);
      new_event(stage_ev_[s]);
    }
    buf_.dev_alloc(d_seqs_in_, staging_batch);
    buf_.dev_alloc(d_fetch_hdr_, staging_batch);
    buf_.dev_alloc(d_fetch_status_, staging_batch);
    buf_.dev_alloc(d_fetch_pay_, (size_t)staging_batch * slot_bytes);

    // pinned host staging
    for (int s = 0; s < 2; ++s) {
      buf_.host_alloc(h_recs_[s], staging_batch);
      buf_.host_alloc(h_pay_[s], stage_pay_bytes_);
    }
    buf_.host_alloc(h_out_seqs_, out_pool_);
    buf_.host_alloc(h_out_counts_, max_agents);
    buf_.host_alloc(h_fetch_hdr_, staging_batch);
    buf_.host_alloc(h_fetch_status_, staging_batch);
    buf_.host_alloc(h_fetch_pay_, (size_t)staging_batch * slot_bytes);
    buf_.host_alloc(h_choices_, staging_batch);

    // device-resident send: sanitised records, and the per-workgroup
    // reply counts / offsets of the compaction (256 rows per workgroup).
    // Allocated last, so that every buffer above sits where it did
    // before these existed (profiles/device_send.md)
    const size_t reply_blocks = ((size_t)staging_batch + 255) / 256;
    buf_.dev_alloc(d_dev_recs_, staging_batch);
    buf_.dev_alloc(d_reply_blk_, reply_blocks);
    buf_.dev_alloc(d_reply_off_, reply_blocks + 1);
    buf_.host_alloc(h_reply_m_, 1);

    // device-resident dispatch: the device copy of the pins (one word per
    // polled agent) and the per-backend row counts with their pinned
    // landing buffer. Last again, for the same reason
    buf_.dev_alloc(d_disp_pinned_, max_agents);
    buf_.dev_alloc(d_disp_counts_, 64);
    buf_.host_alloc(h_disp_counts_, 64);
  }

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
  // `recs`/`pay` (device pointers); async on stream_. `dyn` (the captured
  // tick) overrides the host-known base seq. The broadcast count is reset
  // first unless the caller has done so (`reset_bcast`).
  void launch_enqueue(const Rec *recs, const u8 *pay, int n, u64 base,
                      const u64 *dyn = nullptr, bool reset_bcast = true) {
    if (reset_bcast)
      HIP_CHECK(hipMemsetAsync(d_bcast_count_, 0, sizeof(u32), stream_));
    hipLaunchKernelGGL(k_enqueue_meta, dim3((n + 255) / 256), dim3(256), 0,
                       stream_, recs, n, base, dyn, d_hdr_, d_status_,
                       d_inbox_, d_wpos_, d_rpos_, d_by_type_, d_by_status_,
                       d_sent_, d_bcast_, d_bcast_count_, d_dropped_, g_);
    hipLaunchKernelGGL(k_enqueue_payload, dim3((n + 3) / 4), dim3(256), 0,
                       stream_, recs, pay, n, base, dyn, d_payload_, g_);
    hipLaunchKernelGGL(k_fanout, dim3((g_.max_agents + 255) / 256), dim3(256),
                       0, stream_, d_bcast_, d_bcast_count_, d_active_,
                       d_hdr_, d_bitmaps_, d_bitmap_epochs_, d_inbox_,
                       d_wpos_, d_rpos_, d_dropped_, g_);
  }

  // The dequeue kernel for the `na` agents in d_agents_, async on stream_.
  // `dyn` (the captured tick) overrides the host-known evict_base.
  void launch_receive(int na, int K, bool priority, u64 evict_base,
                      const u64 *dyn) {
    hipLaunchKernelGGL(k_receive, dim3(na), dim3(256),
                       (g_.recv_window + 2) * sizeof(u64), stream_, d_agents_,
                       na, K, priority ? 1 : 0, evict_base, dyn, d_hdr_,
                       d_status_, d_inbox_, d_wpos_, d_rpos_, d_carry_,
                       d_carry_n_, d_bitmaps_, d_bitmap_epochs_, d_out_seqs_,
                       d_out_counts_, d_by_status_, d_received_, g_);
  }

  void check_agent(u32 idx) const {
    if (idx >= g_.max_agents)
      throw std::out_of_range("agent index out of range");
  }

  // The polled-agent list of a call, checked before it goes to d_agents_
  // (max_agents words) and before anything is launched: no longer than
  // max_agents, every index below it, max_per_agent >= 0 and, for a
  // dequeue (`unique`), no agent twice: two workgroups of k_receive on one
  // agent would race on its cursor, carry buffer and counter. Calls that
  // only read through the list pass unique = false.
  void check_polled(const py::array_t<u32> &agents, int max_per_agent,
                    bool unique) {
    if (max_per_agent < 0)
      throw std::invalid_argument("max_per_agent must be >= 0");
    const size_t na = (size_t)agents.size();
    if (na > g_.max_agents)
      throw std::invalid_argument("more polled agents than max_agents");
    const u32 *ap = agents.data();
    for (size_t i = 0; i < na; ++i)
      if (ap[i] >= g_.max_agents)
        throw std::invalid_argument("agent index out of range");
    if (!unique)
      return;
    polled_seen_.assign(g_.bitmap_words, 0);
    for (size_t i = 0; i < na; ++i) {
      u64 &w = polled_seen_[ap[i] >> 6];
      const u64 bit = 1ull << (ap[i] & 63);
      if (w & bit)
        throw std::invalid_argument("agent polled twice in one call");
      w |= bit;
    }
  }

  static bool bad_slot(int slot) { return slot < 0 || slot > 1; }

  static void check_slot(int slot) {
    if (bad_slot(slot))
      throw std::invalid_argument("slot must be 0 or 1");
  }

  void check_batch(int n) const {
    if ((u32)n > staging_batch_)
      throw std::invalid_argument("batch exceeds staging_batch");
  }

  // ---- staging slots ----

  // Copy a batch into a slot's pinned buffers. The one place that writes
  // them: it waits for the H2D that may still read them, and it forgets
  // an earlier prefetch, so a refilled slot is uploaded again.
  void fill_slot(int slot, const py::buffer_info &ri,
                 const py::buffer_info &pi, int n) {
    const size_t pay_bytes = (size_t)pi.size * pi.itemsize;
    ensure_stage_pay(pay_bytes + 16);
    {
      py::gil_scoped_release nogil;
      HIP_CHECK(hipEventSynchronize(stage_ev_[slot]));
      std::memcpy(h_recs_[slot], ri.ptr, (size_t)n * sizeof(Rec));
      if (pay_bytes)
        par_memcpy(h_pay_[slot], pi.ptr, pay_bytes);
    }
    staged_n_[slot] = n;
    staged_pay_[slot] = pay_bytes;
    uploaded_[slot] = false;
  }

  // H2D of a slot's staged_n_ records and staged_pay_ bytes from pinned
  // `recs` / `pay` on `s`; stage_ev_ marks the pinned side free again.
  void upload_slot(int slot, const void *recs, const void *pay,
                   hipStream_t s) {
    HIP_CHECK(hipMemcpyAsync(d_stage_recs_[slot], recs,
                             (size_t)staged_n_[slot] * sizeof(Rec),
                             hipMemcpyHostToDevice, s));
    if (staged_pay_[slot])
      HIP_CHECK(hipMemcpyAsync(d_stage_pay_[slot], pay, staged_pay_[slot],
                               hipMemcpyHostToDevice, s));
    HIP_CHECK(hipEventRecord(stage_ev_[slot], s));
  }

  // The same on the H2D stream, left for wait_prefetch to pick up.
  void prefetch_slot(int slot, const void *recs, const void *pay) {
    upload_slot(slot, recs, pay, h2d_stream_);
    HIP_CHECK(hipEventRecord(up_ev_[slot], h2d_stream_));
    uploaded_[slot] = true;
  }

  // Order stream_ after a slot's prefetch, if there was one.
  bool wait_prefetch(int slot) {
    if (!uploaded_[slot])
      return false;
    HIP_CHECK(hipStreamWaitEvent(stream_, up_ev_[slot], 0));
    uploaded_[slot] = false;
    return true;
  }

  // ---- receive / delivery sequences ----

  // Per-agent counts at `d_src` into the pinned landing buffer, async on
  // stream_; host_counts copies them out after the sync.
  void counts_to_host(const u32 *d_src, int na) {
    HIP_CHECK(hipMemcpyAsync(h_out_counts_, d_src, na * sizeof(u32),
                             hipMemcpyDeviceToHost, stream_));
  }

  // The arrays are made by the caller before it launches, while the GPU
  // still has earlier work to do, not here on the critical path.
  py::array_t<u32> host_counts(py::array_t<u32> counts) const {
    std::memcpy(counts.mutable_data(), h_out_counts_,
                counts.size() * sizeof(u32));
    return counts;
  }

  // (counts, seqs) of the na x K receive that just landed in the pinned
  // buffers (`seqs` is empty when they were not asked for); it becomes
  // the one deliver_outbuf serves.
  py::tuple received(py::array_t<u32> counts, py::array_t<u64> seqs, int na,
                     int K) {
    std::memcpy(seqs.mutable_data(), h_out_seqs_, seqs.size() * sizeof(u64));
    last_recv_na_ = na;
    last_recv_K_ = K;
    return py::make_tuple(host_counts(counts), seqs);
  }

  // Order copy_stream_ after whatever stream_ holds (an in-flight enqueue
  // or receive).
  void copy_after_main() {
    HIP_CHECK(hipEventRecord(ev_, stream_));
    HIP_CHECK(hipStreamWaitEvent(copy_stream_, ev_, 0));
  }

  // D2H row stride of a host delivery: 0 or too large means slot_bytes,
  // rounded up to the 16-B chunk the gather kernels copy.
  u32 clamp_stride(u32 stride) const {
    if (stride == 0 || stride > g_.slot_bytes)
      stride = g_.slot_bytes;
    return (stride + 15u) & ~15u;
  }

  // k_gather of `n` seqs and the D2H of their headers, statuses (if
  // asked) and `stride`-byte payload rows, on copy_stream_ after stream_.
  void gather_to_host(const u64 *seqs, int n, u32 stride, bool with_status) {
    copy_after_main();
    HIP_CHECK(hipMemcpyAsync(d_seqs_in_, seqs, n * sizeof(u64),
                             hipMemcpyHostToDevice, copy_stream_));
    hipLaunchKernelGGL(k_gather, dim3((n + 3) / 4), dim3(256), 0, copy_stream_,
                       d_seqs_in_, n, d_hdr_, d_status_, d_payload_,
                       d_fetch_hdr_, d_fetch_status_, d_fetch_pay_, evict_base_,
                       stride, g_);
    HIP_CHECK(hipMemcpyAsync(h_fetch_hdr_, d_fetch_hdr_, n * sizeof(Rec),
                             hipMemcpyDeviceToHost, copy_stream_));
    if (with_status)
      HIP_CHECK(hipMemcpyAsync(h_fetch_status_, d_fetch_status_,
                               n * sizeof(u32), hipMemcpyDeviceToHost,
                               copy_stream_));
    HIP_CHECK(hipMemcpyAsync(h_fetch_pay_, d_fetch_pay_, (size_t)n * stride,
                             hipMemcpyDeviceToHost, copy_stream_));
  }

  // End of a delivery on copy_stream_: drain it, or keep a bounded async
  // pipeline: wait for the delivery issued two calls ago before letting
  // this one fly (an unbounded copy stream backlog eventually hard-blocks
  // the runtime for the whole accumulated drain).
  void finish_delivery(bool synchronize) {
    if (synchronize) {
      HIP_CHECK(hipStreamSynchronize(copy_stream_));
      return;
    }
    HIP_CHECK(hipEventRecord(d2h_ev_[d2h_cur_], copy_stream_));
    d2h_cur_ ^= 1;
    HIP_CHECK(hipEventSynchronize(d2h_ev_[d2h_cur_]));
    drain_spree();
  }

  // ---- scans ----

  // [lo, hi) cut to the live window and `cap` to the match buffer; false
  // when nothing is left to scan.
  bool clamp_scan(u64 &lo, u64 &hi, u32 &cap) const {
    lo = std::max(lo, evict_base_);
    hi = std::min(hi, count_);
    cap = std::min(cap, staging_batch_);
    return lo < hi;
  }

  // An environment variable that is one whole decimal integer, else 0.
  static long env_long(const char *name) {
    const char *e = getenv(name);
    if (!e || !*e)
      return 0;
    char *end = nullptr;
    errno = 0;
    const long v = strtol(e, &end, 10);
    return (errno || *end) ? 0 : v;
  }

  // The matches a scan on stream_ left in d_match_ (at most `cap`).
  py::array_t<u64> read_matches(u32 cap) {
    u32 nmatch = 0;
    {
      py::gil_scoped_release nogil;
      HIP_CHECK(hipMemcpyAsync(&nmatch, d_match_count_, sizeof(u32),
                               hipMemcpyDeviceToHost, stream_));
      HIP_CHECK(hipStreamSynchronize(stream_));
    }
    const u32 take = std::min(nmatch, cap);
    py::array_t<u64> out(take);
    if (take)
      HIP_CHECK(hipMemcpy(out.mutable_data(), d_match_, take * sizeof(u64),
                          hipMemcpyDeviceToHost));
    return out;
  }

  // row stride of a device-side payload tensor: the bounds of a
  // delivery's stride
  void check_row_stride(u32 stride) const {
    if (stride < 16 || stride > g_.slot_bytes || stride % 16 != 0)
      throw std::invalid_argument(
          "stride must be a multiple of 16 in 16..slot_bytes");
  }

  // Caller-provided device pointers as (pointer, alignment): every one
  // non-null (when `required`), then every one aligned for the type a
  // kernel reads through it. Without an `align_msg` both read `null_msg`.
  using DevPtr = std::pair<uintptr_t, size_t>;
  static void check_dev_ptrs(std::initializer_list<DevPtr> ptrs, bool required,
                             const char *null_msg,
                             const char *align_msg = nullptr) {
    for (const DevPtr &d : ptrs)
      if (required && !d.first)
        throw std::invalid_argument(null_msg);
    for (const DevPtr &d : ptrs)
      if (d.first % d.second)
        throw std::invalid_argument(align_msg ? align_msg : null_msg);
  }

  // the log grew to base + n messages; the ring keeps the newest num_slots
  void advance_count(u64 base, u64 n) {
    count_ = base + n;
    if (count_ > g_.num_slots)
      evict_base_ = count_ - g_.num_slots;
  }

  // the polled agents of a call, to d_agents_ on stream_
  void upload_agents(const u32 *agents, int na) {
    if (na)
      HIP_CHECK(hipMemcpyAsync(d_agents_, agents, na * sizeof(u32),
                               hipMemcpyHostToDevice, stream_));
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
    // freed and made again through buf_, which forgets the old pointers
    // and records the new ones: release() never sees a freed buffer
    for (int s = 0; s < 2; ++s) {
      buf_.dev_free(d_stage_pay_[s]);
      buf_.host_free(h_pay_[s]);
      buf_.dev_alloc(d_stage_pay_[s], nb);
      buf_.host_alloc(h_pay_[s], nb);
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
  std::vector<u64> polled_seen_; // check_polled's max_agents-bit scratch
  bool released_ = false;
  size_t out_pool_ = 0;
  size_t stage_pay_bytes_ = 0;

  HipBuffers buf_; // owns every d_* / h_* buffer below
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
