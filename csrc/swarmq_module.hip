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
// The code lives in the headers included below (docs/ARCHITECTURE.md has
// the map); this file is the one translation unit and the bindings.
//
// Build: hipcc --offload-arch=gfx950 (see setup.py) — no CUDA paths, no
// hipify, no Triton.

#include "swarmq_device_queue.h"
#include "swarmq_doorbell.h"

// ---------------------------------------------------------------------------
// python module
// ---------------------------------------------------------------------------

PYBIND11_MODULE(_swarmq, m) {
  m.doc() = "MI355X-native GPU message-queue engine (CDNA4 HIP kernels)";
  m.attr("RECV_WINDOW") = RECV_WINDOW;
  m.attr("CONTEXT_GROUP") = CONTEXT_GROUP;
  m.attr("CONTEXT_GROUP_WIDE") = CONTEXT_GROUP_WIDE;
  m.attr("CONTEXT_EAGER_VIS") = SWARMQ_CONTEXT_EAGER_VIS;

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
           py::arg("ctx_payload_ptr"), py::arg("group") = 0,
           py::arg("shared") = false)
      .def("fetch", &DeviceQueue::fetch)
      .def("fetch_raw", &DeviceQueue::fetch_raw, py::arg("seqs"),
           py::arg("stride") = 0, py::arg("synchronize") = true)
      .def("delivery_sync", &DeviceQueue::delivery_sync)
      .def("set_status", &DeviceQueue::set_status)
      .def("set_statuses", &DeviceQueue::set_statuses)
      .def("get_status", &DeviceQueue::get_status)
      .def("get_statuses", &DeviceQueue::get_statuses)
      .def("query_range", &DeviceQueue::query_range, py::arg("lo"),
           py::arg("hi"), py::arg("sender"), py::arg("receiver"),
           py::arg("type_code"), py::arg("status"), py::arg("after"),
           py::arg("before"), py::arg("pred_mask"), py::arg("cap"),
           py::arg("blocks") = 0)
      .def("search_range", &DeviceQueue::search_range, py::arg("lo"),
           py::arg("hi"), py::arg("needle"), py::arg("fold"), py::arg("cap"),
           py::arg("blocks") = 0, py::arg("loads") = 0)
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
