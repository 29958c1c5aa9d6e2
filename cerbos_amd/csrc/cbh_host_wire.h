// Host side of libcerbos_hip.so, part 4 of 5 (included by cbh_engine.hip, host pass only): the wire road.
#pragma once

// ---- device-side ingest: serialized CheckInputs -> a resident batch, flattened by the GPU (cbh_wire.h) ------------------
// H2D of the raw bytes + offsets, count + scan launches, one small D2H (totals, shape), the fill launch, one small D2H
// (what it needed, what it could not take).  The batch is then an ordinary resident batch: cbh_check_resident,
// cbh_result_download - results in INPUT order (no routing sort on this path: nothing to undo).
// bytes of dynamic LDS for a wave that wants `want` bytes: a power of two between 4 and 48 KB, 0 = the kernel works in place.
// CBH_WIRE_LDS (measurement aid): 0 nothing staged, 1 the assembler's outputs only, 2 the flattener's messages too.
static u32 wire_lds_cap(size_t want, int needs_mode) {
  if (wire_lds_mode(CBH_WIRE_LDS_DEFAULT) < needs_mode) return 0;
  u32 c = 4096; while (c < want && c < 49152u) c <<= 1;
  return c > 49152u ? 49152u : c;
}
// The fill kernel's block of messages: staged in LDS - where the dependent loads of the parse are several times shorter than in L2 -
// when the call's LARGEST block (WireStats.max_block) leaves a CU several waves (up to CBH_WIRE_FILL_LDS_MAX bytes, in 1 KB steps);
// a call of larger messages parses them in place (the same code on a global pointer: cbh_wire_fill_kernel).
// CBH_WIRE_LDS=0/1: never; CBH_WIRE_FILL_LDS_MAX=bytes: the bound.
static u32 wire_fill_lds_cap(u32 max_block) {
  static const u32 most = (u32)env_int("CBH_WIRE_FILL_LDS_MAX", 32768);
  if (wire_lds_mode(2) < 2 || max_block == 0 || max_block > most) return 0;
  const u32 c = (max_block + 16u + CBH_WIRE_SLACK + 1023u) & ~1023u;
  return c > most ? 0u : c;
}
static bool is_pinned(const void* p);
// the replica's link streams (made on first use; CBH_WIRE_LINK_STREAMS=0: every batch copies on its own stream, as before)
static bool wire_link_streams(Replica* rep) {
  static const bool on = !env_is("CBH_WIRE_LINK_STREAMS", '0');
  if (!on) return false;
  std::lock_guard<std::mutex> lk(rep->wstream_mu);
  if (!rep->link_streams_tried) {
    rep->link_streams_tried = true;
    if (hipStreamCreateWithFlags(&rep->up_stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); rep->up_stream = nullptr; }
    if (rep->up_stream && hipStreamCreateWithFlags(&rep->down_stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); rep->down_stream = nullptr; }
    if (!rep->down_stream && rep->up_stream) { (void)hipStreamDestroy(rep->up_stream); rep->up_stream = nullptr; }
  }
  return rep->up_stream != nullptr;
}
static hipEvent_t wire_event(cbh_device_batch* b, int which) {
  hipEvent_t& ev = b->w.ev[which];
  if (!ev) {
    std::lock_guard<std::mutex> lk(b->rep->wstream_mu);
    if (!b->rep->wevents_idle.empty()) { ev = b->rep->wevents_idle.back(); b->rep->wevents_idle.pop_back(); }
    else if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); ev = nullptr; }
  }
  return ev;
}
// a place of the batch's page-locked block as a KERNEL addresses it: what hipHostGetDevicePointer says of the block, not the host pointer
// taken on trust
template <class T> static T* pin_dev(const cbh_device_batch* b, T* host_ptr) {
  return reinterpret_cast<T*>(reinterpret_cast<char*>(host_ptr) + b->w.pinned_delta);
}
// ... and as the host addresses it: `off` is one of the layout's answers (WirePin)
template <class T> static T* pin_at(const cbh_device_batch* b, size_t off) { return reinterpret_cast<T*>(static_cast<u8*>(b->w.pinned) + off); }
// The batch's page-locked block: an idle one of the replica that is large enough, or a new one (the call's offsets, defaults and
// statistics cross PCIe from / to it; kernels write it: wire_publish).  Its layout is fixed here, for the call's tail and messages.
static int wire_pin_lease(cbh_device_batch* b, size_t tail_bytes, size_t n, bool offsets_go_up) {
  Replica* rep = b->rep; WireBatch& w = b->w;
  const size_t want = WirePin::wanted(tail_bytes, n);
  {
    std::lock_guard<std::mutex> lk(rep->wstream_mu);
    for (size_t k = 0; k < rep->wpinned_idle.size(); ++k)
      if (rep->wpinned_idle[k].second >= want) { w.pinned = rep->wpinned_idle[k].first; w.pin.cap = rep->wpinned_idle[k].second; rep->wpinned_idle[k] = rep->wpinned_idle.back(); rep->wpinned_idle.pop_back(); break; }
    if (!w.pinned) {
      size_t cap = 1 << 16; while (cap < want) cap <<= 1;
      if (hipHostMalloc(&w.pinned, cap, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); w.pinned = nullptr; }
      w.pin.cap = cap;
    }
  }
  if (!w.pinned) return fail("cbh_wire_flatten: hipHostMalloc failed");
  w.pin.tail_bytes = tail_bytes; w.pin.n = n;
  w.pin.check(offsets_go_up ? n : 0);
  void* dev = nullptr;
  if (hipHostGetDevicePointer(&dev, w.pinned, 0) != hipSuccess || !dev) { (void)hipGetLastError(); dev = w.pinned; }
  w.pinned_delta = static_cast<char*>(dev) - static_cast<char*>(w.pinned);
  return 0;
}
// n_words of device memory -> the batch's page-locked block (cbh_wire_publish_kernel: no copy engine); read after a synchronise
static int wire_publish(cbh_device_batch* b, const void* d_src, void* pinned_dst, u32 n_words) {
  WirePublishArgs pa; pa.src = static_cast<const u32*>(d_src); pa.dst = pin_dev(b, static_cast<u32*>(pinned_dst)); pa.n_words = n_words; pa.pad = 0;
  hipLaunchKernelGGL(cbh_wire_publish_kernel, dim3(1), dim3(64), 0, b->stream, pa);
  HIPCHK(hipGetLastError());
  return 0;
}
static WireStats* wire_stats_land(cbh_device_batch* b) { return pin_at<WireStats>(b, b->w.pin.slot(1)); }
static int wire_stats_read(cbh_device_batch* b, const WireStats* d_stats, WireStats& st) {
  WireStats* land = wire_stats_land(b);
  if (wire_publish(b, d_stats, land, (u32)(sizeof(st) / 4)) != 0) return -1;
  HIPCHK(hipStreamSynchronize(b->stream));
  st = *land;
  return 0;
}
static int wire_stats_write(cbh_device_batch* b, WireStats* d_stats, const WireStats& st) {
  WireStats* from = pin_at<WireStats>(b, b->w.pin.slot(0));
  *from = st;
  HIPCHK(hipMemcpyAsync(d_stats, from, sizeof(st), hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

// (cbh_wire_check_pb) the uploads of a call's slices go over the link ONE AFTER THE OTHER, in slice order, so that slice k is being
// decided while slice k + 1 is still on its way: a slice's upload waits for the event its predecessor recorded behind its own
struct WireChain {
  hipEvent_t wait = nullptr, record = nullptr;
  std::atomic<int>* prev_recorded = nullptr; std::atomic<int>* recorded = nullptr;
  void done() { if (recorded) recorded->store(1, std::memory_order_release); }   // (also on every early return: the successor must not wait for ever)
};
// (cbh_wire_flatten_requests) `bytes` / `offsets` / `n` are CheckResourcesRequests: the messages the flattener works on are made on
// the device (cbh_wire_req.h)
struct WireRequests {
  const uint8_t* aux = nullptr; const uint64_t* aux_offsets = nullptr;   // serialized engine AuxData per request, or null
  uint32_t* first_input = nullptr;   // out [n + 1]: the inputs of request r are first_input[r] .. first_input[r + 1]
  uint8_t* flags = nullptr;          // out [n] (may be null): bit 0 = include_meta
};

// One cbh_wire_flatten call: what its stages (wf_*, below, in the order they run) share.  The call owns the batch until wf_finish
// hands it to the caller: every other way out releases it - and tells the chain's successor, whatever happened, that it need
// not wait any longer.
struct WireFlatten {
  cbh_table* t = nullptr; Replica* rep = nullptr; cbh_device_batch* b = nullptr; hipStream_t s = nullptr;
  const uint8_t* bytes = nullptr; const uint64_t* offsets = nullptr; u32 n_in = 0;   // what the caller gave: CheckInputs, or (reqs) requests
  const WireRequests* reqs = nullptr; WireChain* chain = nullptr; cbh_wire_info* info = nullptr;
  u32 n = 0; u64 total = 0;   // the CheckInputs and their bytes (requests: what wf_split_requests made of them)
  std::string tail; u32 dv_len = 0, ds_len = 0; size_t globals_len = 0, tail_room = 0;   // default version + default scope + "claims" + globals, behind the messages
  u8* d_msg = nullptr; u64* d_moff = nullptr; WireStats* d_stats = nullptr;
  WireArgs a; WireRouteArgs ra; WireStats st; bool try_group = false, have_outputs = false;
  u32 ncol = 0, nw = 0, slots = 0, heap_cap = 0, n_host_count = 0, runs = 0;
  WireFlatten() { std::memset(&a, 0, sizeof(a)); std::memset(&ra, 0, sizeof(ra)); cbh_wire_stats_init(st); }
  WireFlatten(const WireFlatten&) = delete;   // (an owner; and a launch takes the members it needs as locals, never the whole call by value)
  ~WireFlatten() { if (b) cbh_batch_release(b); if (chain) chain->done(); }
};
// (a sliced call, WireChain) the big upload of this slice goes behind its predecessor's
static bool wf_chain_wait(WireFlatten& f, bool enqueue_order_only) {
  WireChain* chain = f.chain;
  if (chain && chain->prev_recorded) {   // (the predecessor's thread has enqueued the record by now, or is about to)
    while (!chain->prev_recorded->load(std::memory_order_acquire)) std::this_thread::yield();
    if (enqueue_order_only) return true;   // (one upload stream: its order is the order of the calls)
    // The successor's upload is handed to the copy engines only when the predecessor's has LANDED (a wait on the host, not a
    // dependency on the device): uploads queued ahead of time are spread over the engines, and a slice's answers - a copy the
    // other way, asked for later - then wait behind them all (measured: downloads began when the last upload had ended, although
    // the link carries both directions at once: tools/pcie_duplex.hip).  CBH_WIRE_CHAIN_DEVICE=1: the dependency on the device.
    static const bool on_device = env_set("CBH_WIRE_CHAIN_DEVICE");
    if (chain->wait && (on_device ? hipStreamWaitEvent(f.s, chain->wait, 0) : hipEventSynchronize(chain->wait)) != hipSuccess) { fail("cbh_wire_flatten: waiting for the previous slice's upload failed"); return false; }
  }
  return true;
}
static void wf_chain_record(WireFlatten& f) { if (f.chain && f.chain->record) { (void)hipEventRecord(f.chain->record, f.s); f.chain->done(); } }
// the bulk upload on the replica's upload stream has been enqueued: the event behind it, the successor may enqueue its own, the
// batch's stream takes over behind the event
static bool wf_upload_landed_behind(WireFlatten& f, hipEvent_t ev) {
  const bool ok = hipEventRecord(ev, f.rep->up_stream) == hipSuccess;
  if (f.chain) f.chain->done();
  return ok && hipStreamWaitEvent(f.s, ev, 0) == hipSuccess;
}
// a malformed message: by index of the CheckInput, or - requests - of the request its resource entry belongs to
static void wf_bad_input(WireFlatten& f, u32 i) {
  if (!f.reqs) { f.info->first_bad = i; fail("malformed CheckInput at index " + std::to_string(i)); return; }
  u32 r = 0;
  while (r + 1u < f.n_in && f.reqs->first_input[r + 1u] <= i) ++r;
  f.info->first_bad = r;
  fail("malformed CheckResourcesRequest at index " + std::to_string(r) + " (resource entry " + std::to_string(i - f.reqs->first_input[r]) + ")");
}

// ---- stage: the batch, its stream, its page-locked block.  1 = the table has no device flattener (the host's call)
static int wf_open(WireFlatten& f, uint32_t device_index, const char* default_version, const char* default_scope, const uint8_t* globals_pb) {
  cbh_table* t = f.t;
  if (device_index >= t->reps.size()) return fail("device index out of range");
  if (t->wire.why_not) { f.info->n_host = f.n_in; g_err = t->wire.why_not; return 1; }
  f.total = f.n_in ? f.offsets[f.n_in] : 0;   // (requests: of the CheckInputs made of them, wf_split_requests)
  std::string dv = default_version ? default_version : "default", ds = default_scope ? default_scope : "";
  if (!ds.empty() && ds[0] == '.') ds.erase(0, 1);   // scope_value (namer.go:276-278)
  if (f.total + dv.size() + ds.size() + f.globals_len + 64 > 0xFFFFFFFFull) return fail("cbh_wire_flatten: more than 4 GB of messages in one call");
  f.dv_len = (u32)dv.size(); f.ds_len = (u32)ds.size(); f.tail_room = dv.size() + ds.size() + f.globals_len + 64;
  f.tail = dv + ds + "claims";
  if (f.globals_len) f.tail.append(reinterpret_cast<const char*>(globals_pb), f.globals_len);
  f.rep = t->reps[device_index];
  HIPCHK(hipSetDevice(f.rep->device));
  f.b = batch_new(t, f.rep, true);
  if (!f.b) return -1;
  f.b->wire = true; f.s = f.b->stream;
  return wire_pin_lease(f.b, f.tail.size(), f.n_in, !f.reqs);
}

// ---- stage (requests only): CheckResourcesRequests -> the CheckInputs of their resource entries, on the device (cbh_wire_req.h):
// counts, two prefix sums on the host, the split.  `n` / `total` come back as the inputs' and their bytes'.
static int wf_split_requests(WireFlatten& f, u32& n, u64& total) {
  cbh_device_batch* b = f.b; Replica* rep = f.rep; hipStream_t s = f.s; const WireRequests* reqs = f.reqs;
  const u32 nr = f.n_in;
  const u64 rtotal = f.total, atotal = (reqs->aux_offsets && nr) ? reqs->aux_offsets[nr] : 0;
  if (atotal > 0xFFFFFFFFull) return fail("cbh_wire_flatten_requests: more than 4 GB of auxiliary data in one call");
  WireReqArgs q; std::memset(&q, 0, sizeof(q));
  u8* d_req = nullptr; u64* d_roff = nullptr; u8* d_aux = nullptr; u64* d_aoff = nullptr; u32* d_first = nullptr; u64* d_fbyte = nullptr;
  int rq = 0;
  rq |= dalloc(b, d_req, (size_t)rtotal + 8); rq |= dalloc(b, d_roff, (size_t)nr + 1);
  rq |= dalloc(b, q.n_inputs, (size_t)nr + 1); rq |= dalloc(b, q.n_bytes, (size_t)nr + 1); rq |= dalloc(b, q.flags, (size_t)nr + 1);
  rq |= dalloc(b, d_first, (size_t)nr + 1); rq |= dalloc(b, d_fbyte, (size_t)nr + 1);
  if (reqs->aux_offsets) { rq |= dalloc(b, d_aux, (size_t)atotal + 8); rq |= dalloc(b, d_aoff, (size_t)nr + 1); }
  if (rq != 0) return -1;
  hipEvent_t ev_rq = wire_link_streams(rep) ? wire_event(b, 0) : nullptr;   // (the replica's upload stream, as for CheckInputs in wf_upload)
  hipStream_t rs = ev_rq ? rep->up_stream : s;
  if (!wf_chain_wait(f, ev_rq != nullptr)) return -1;
  if ((rtotal && hipMemcpyAsync(d_req, f.bytes, rtotal, hipMemcpyHostToDevice, rs) != hipSuccess) ||
      (nr && hipMemcpyAsync(d_roff, f.offsets, ((size_t)nr + 1) * 8, hipMemcpyHostToDevice, rs) != hipSuccess) ||
      (atotal && hipMemcpyAsync(d_aux, reqs->aux, atotal, hipMemcpyHostToDevice, rs) != hipSuccess) ||
      (reqs->aux_offsets && nr && hipMemcpyAsync(d_aoff, reqs->aux_offsets, ((size_t)nr + 1) * 8, hipMemcpyHostToDevice, rs) != hipSuccess))
    return fail("cbh_wire_flatten_requests: upload failed");
  if (ev_rq) { if (!wf_upload_landed_behind(f, ev_rq)) return fail("cbh_wire_flatten_requests: upload failed"); }
  else wf_chain_record(f);
  q.req = d_req; q.roff = d_roff; q.n = nr; q.end = (u32)rtotal; q.aux = d_aux; q.aoff = reqs->aux_offsets ? d_aoff : nullptr; q.aux_end = atotal;
  if (nr) hipLaunchKernelGGL(cbh_wire_req_count_kernel, dim3((nr + CBH_BLOCK - 1) / CBH_BLOCK), dim3(CBH_BLOCK), 0, s, q);
  std::vector<u32> h_inputs((size_t)nr + 1, 0), h_first((size_t)nr + 1, 0); std::vector<u64> h_bytes((size_t)nr + 1, 0), h_fbyte((size_t)nr + 1, 0);
  if (nr && (hipMemcpyAsync(h_inputs.data(), q.n_inputs, (size_t)nr * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
             hipMemcpyAsync(h_bytes.data(), q.n_bytes, (size_t)nr * 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
             (reqs->flags && hipMemcpyAsync(reqs->flags, q.flags, (size_t)nr, hipMemcpyDeviceToHost, s) != hipSuccess)))
    return fail("cbh_wire_flatten_requests: download failed");
  if (hipStreamSynchronize(s) != hipSuccess) return fail("cbh_wire_flatten_requests failed");
  u64 n_inputs = 0, n_bytes = 0;
  for (u32 r = 0; r < nr; ++r) {
    if (h_inputs[r] == CBH_WREQ_BAD) { f.info->first_bad = r; return fail("malformed CheckResourcesRequest at index " + std::to_string(r)); }
    h_first[r] = (u32)n_inputs; h_fbyte[r] = n_bytes;
    n_inputs += h_inputs[r]; n_bytes += h_bytes[r];
    if (n_inputs > 0x7FFFFFFFull) return fail("cbh_wire_flatten_requests: too many resource entries in one call");
  }
  h_first[nr] = (u32)n_inputs; h_fbyte[nr] = n_bytes;
  if (n_bytes + f.tail_room > 0xFFFFFFFFull) return fail("cbh_wire_flatten_requests: more than 4 GB of CheckInputs in one call");
  std::memcpy(reqs->first_input, h_first.data(), ((size_t)nr + 1) * 4);
  n = (u32)n_inputs; total = n_bytes;
  f.info->n_requests = n;
  if (dalloc(b, f.d_msg, (size_t)total + f.tail_room) != 0 || dalloc(b, f.d_moff, (size_t)n + 1) != 0) return -1;
  q.first_input = d_first; q.first_byte = d_fbyte; q.msg = f.d_msg; q.moff = f.d_moff;
  // (pageable sources: the copies are staged before the call returns to this thread, the vectors outlive them)
  if (hipMemcpyAsync(d_first, h_first.data(), ((size_t)nr + 1) * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(d_fbyte, h_fbyte.data(), ((size_t)nr + 1) * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemsetAsync(f.d_moff, 0, 8, s) != hipSuccess)
    return fail("cbh_wire_flatten_requests: upload failed");
  if (nr) hipLaunchKernelGGL(cbh_wire_req_split_kernel, dim3((nr + (CBH_BLOCK / 64u) - 1) / (CBH_BLOCK / 64u)), dim3(CBH_BLOCK), 0, s, q);
  if (hipStreamSynchronize(s) != hipSuccess) return fail("cbh_wire_flatten_requests failed");   // (h_first / h_fbyte go out of scope)
  return 0;
}

// ---- stage: the flattener's arguments, its first arrays, and everything that goes up
static int wf_upload(WireFlatten& f) {
  cbh_table* t = f.t; cbh_device_batch* b = f.b; Replica* rep = f.rep; hipStream_t s = f.s; WireArgs& a = f.a;
  const u32 n = f.n; const u64 total = f.total;
  f.nw = (n + 63u) / 64u; f.ncol = t->meta[CBH_M_NCOLUMNS];
  const TableDev& td = rep->dev;
  a.t_str_off = td.str_off; a.t_str_bytes = td.str_bytes; a.K = td.K; a.t_flags = td.flags;
  a.tix = rep->w_tix; a.tix_mask = t->wire.tix_mask; a.scope_of_sid = rep->w_scope_of_sid;
  a.cols = rep->w_cols; a.col_keys = rep->w_col_keys; a.n_cols = f.ncol; a.sens_cols = t->meta[CBH_M_SENS_COLS];
  a.n = n;
  a.dver_off = (u32)total; a.dver_len = f.dv_len; a.dscope_off = (u32)(total + f.dv_len); a.dscope_len = f.ds_len;
  a.claims_off = (u32)(total + f.dv_len + f.ds_len);
  a.globals_off = a.claims_off + 6u; a.globals_len = (u32)f.globals_len;
  int rc = 0;
  if (!f.reqs) { rc |= dalloc(b, f.d_msg, (size_t)total + f.tail_room); rc |= dalloc(b, f.d_moff, (size_t)n + 1); }
  rc |= dalloc(b, a.cnt, (size_t)n + 1); rc |= dalloc(b, a.status, (size_t)n + 1);
  rc |= dalloc(b, a.wavesum, 4 * (size_t)f.nw + 4); rc |= dalloc(b, a.waveoff, 2 * (size_t)f.nw + 4);
  rc |= dalloc(b, f.d_stats, 1);
  if (rc != 0) return -1;
  a.msg = f.d_msg; a.moff = f.d_moff; a.stats = f.d_stats;
  // everything small goes through the batch's page-locked block: statistics (slots 0 / 1), the tail, the offsets
  const WirePin& pin = b->w.pin;
  WireStats* pin_st = pin_at<WireStats>(b, pin.slot(0));
  u8* pin_tail = pin_at<u8>(b, pin.tail());
  u64* pin_off = pin_at<u64>(b, pin.offsets());
  *pin_st = f.st;
  std::memcpy(pin_tail, f.tail.data(), f.tail.size());
  if (!f.reqs) { if (n) std::memcpy(pin_off, f.offsets, ((size_t)n + 1) * 8); else pin_off[0] = 0; }
  // the uploads: on the replica's upload stream (one copy engine for this direction, the slices of a call in their order - the
  // chain only orders the ENQUEUEING then), the batch's own stream takes over behind an event; else on the batch's stream
  hipEvent_t ev_up = (!f.reqs && wire_link_streams(rep)) ? wire_event(b, 0) : nullptr;
  hipStream_t us = ev_up ? rep->up_stream : s;
  if (!f.reqs) {
    if (!wf_chain_wait(f, ev_up != nullptr)) return -1;
    if (total && hipMemcpyAsync(f.d_msg, f.bytes, total, hipMemcpyHostToDevice, us) != hipSuccess) return fail("cbh_wire_flatten: upload failed");
    if (!ev_up) wf_chain_record(f);
  }
  // (the small ones on the batch's own stream: on the upload stream every one of them would be a gap between two slices' messages)
  if (hipMemcpyAsync(f.d_msg + total, pin_tail, f.tail.size(), hipMemcpyHostToDevice, s) != hipSuccess ||
      (!f.reqs && hipMemcpyAsync(f.d_moff, pin_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s) != hipSuccess) ||
      hipMemcpyAsync(f.d_stats, pin_st, sizeof(f.st), hipMemcpyHostToDevice, s) != hipSuccess) return fail("cbh_wire_flatten: upload failed");
  if (ev_up && !wf_upload_landed_behind(f, ev_up)) return fail("cbh_wire_flatten: upload failed");   // (the successor may enqueue its uploads now)
  return 0;
}

// ---- stage: the count launch (the scan that follows it opens every round of the regrowth loop: wf_scan)
static void wf_count(WireFlatten& f) {
  // the count kernel's staging block: the call's average block and a half (the fill is sized by the largest, which the count finds)
  WireArgs& a = f.a; hipStream_t s = f.s; const u32 nw = f.nw;
  const u64 avg_block = f.n ? f.total / f.n * 64u : 0u;
  a.lds_cap = wire_fill_lds_cap((u32)std::min<u64>(avg_block + avg_block / 2u + 256u, 0xFFFFFFFFull));
  if (nw) hipLaunchKernelGGL(cbh_wire_count_kernel, dim3(nw), dim3(CBH_BLOCK), a.lds_cap, s, a);
  wmark("uploads+count enqueued");
  // Group the requests by route (cbh_wire.h cbh_wire_route_kernel ...): what the host flattener's routing sort does for the
  // decision kernels' merged walk - launched behind every fill (wf_launch_routes).  CBH_WIRE_GROUP=0: leave the batch in input order
  // (measurement aid).
  static const bool group_on = !env_is("CBH_WIRE_GROUP", '0');
  f.try_group = group_on && f.n >= 2u * CBH_BLOCK;
  f.slots = cbh_wire_dict_slots(f.n); f.heap_cap = cbh_wire_heap_guess(f.total);
}
// the dictionary's words and, behind them, its flag bytes; the route table's keys and, behind them, its counters: each one block
// and one memset - these give the size to both
static size_t dict_words(u32 slots) { return (size_t)slots + ((size_t)slots / 4 + 1 + 1) / 2; }
static size_t route_words() { return (size_t)CBH_WIRE_ROUTE_SLOTS + ((size_t)CBH_WIRE_ROUTE_SLOTS + 2 + 1) / 2; }
static int wf_launch_routes(WireFlatten& f) {
  if (!f.try_group) return 0;
  cbh_device_batch* b = f.b; WireRouteArgs& ra = f.ra; const WireArgs& a = f.a; hipStream_t s = f.s; const u32 n = f.n, nw = f.nw;
  if (!ra.rt_key) {
    ra.n = n; ra.n_cols = f.ncol; ra.req_u32 = a.req_u32; ra.roles = a.roles; ra.col_tag = a.col_tag; ra.col_val = a.col_val;
    ra.multi = &f.d_stats->multi_route;
    int rr = 0;
    rr |= dalloc(b, ra.rt_key, route_words());
    ra.rt_cnt = reinterpret_cast<u32*>(ra.rt_key + CBH_WIRE_ROUTE_SLOTS);
    ra.host_routes = pin_dev(b, pin_at<u32>(b, b->w.pin.routes())); ra.stats = f.d_stats; ra.host_stats = pin_dev(b, wire_stats_land(b));
    rr |= dalloc(b, ra.slot, (size_t)n); rr |= dalloc(b, ra.rank, (size_t)n); rr |= dalloc(b, ra.inv, (size_t)n);
    rr |= dalloc(b, ra.req_out, (size_t)CBH_RQ_NFIELDS * n); rr |= dalloc(b, ra.col_tag_out, (size_t)f.ncol * n); rr |= dalloc(b, ra.col_val_out, (size_t)f.ncol * n);
    if (rr != 0) return -1;
  }
  if (hipMemsetAsync(ra.rt_key, 0, route_words() * 8, s) != hipSuccess) return fail("cbh_wire_flatten: memset failed");
  hipLaunchKernelGGL(cbh_wire_route_kernel, dim3(nw), dim3(CBH_BLOCK), 0, s, ra);
  hipLaunchKernelGGL(cbh_wire_route_scan_kernel, dim3(1), dim3(CBH_BLOCK), 0, s, ra);   // (leaves the route words AND the fill's statistics with the host)
  hipLaunchKernelGGL(cbh_wire_gather_kernel, dim3(nw), dim3(CBH_BLOCK), 0, s, ra);
  HIPCHK(hipGetLastError());
  return 0;
}
// what the device's statistics go back to before the fill runs again (either retry loop): what the count found stays, what a fill
// adds starts over
static WireStats wire_stats_reset(const WireStats& st, u32 n_host_count) {
  WireStats reset = st; reset.heap_used = 0; reset.n_host = n_host_count; reset.flags = 0; reset.route_lo = reset.route_hi = reset.multi_route = 0;
  return reset;
}

// ---- stage: (re)start from the scan: the dictionary (f.slots) is empty, the scan interns the call's default strings first.  The
// first time the counts also give the batch's arrays their sizes.  1 = the count found messages for the host flattener
static int wf_scan(WireFlatten& f) {
  cbh_device_batch* b = f.b; hipStream_t s = f.s; WireArgs& a = f.a; WireStats& st = f.st; const u32 n = f.n;
  u64* dict = nullptr;
  if (dalloc(b, dict, dict_words(f.slots)) != 0) return -1;
  a.lix = dict; a.lflags = reinterpret_cast<u32*>(dict + f.slots);
  a.lix_mask = f.slots - 1;
  if (hipMemsetAsync(dict, 0, dict_words(f.slots) * 8, s) != hipSuccess) return fail("cbh_wire_flatten: memset failed");
  a.host_stats = pin_dev(b, wire_stats_land(b));   // (the scan kernel leaves the statistics there itself)
  hipLaunchKernelGGL(cbh_wire_scan_kernel, dim3(1), dim3(CBH_BLOCK), 0, s, a);
  if (hipStreamSynchronize(s) != hipSuccess) return fail("cbh_wire_flatten failed");
  st = *wire_stats_land(b);
  wmark("counts known");
  if (f.have_outputs) return 0;
  f.n_host_count = st.n_host;
  if (st.first_bad != CBH_NONE) { wf_bad_input(f, st.first_bad); return -1; }
  if (st.n_host) {   // the count already found messages for the host flattener (more than 64 actions / 255 roles): no point in filling
    f.info->n_tuples = st.n_tuples; f.info->n_host = st.n_host;
    g_err = "cbh_wire_flatten: " + std::to_string(st.n_host) + " message(s) are the host flattener's (more than 64 actions or 255 roles)";
    return 1;
  }
  int rc = 0;
  rc |= dalloc(b, a.req_u32, (size_t)CBH_RQ_NFIELDS * n); rc |= dalloc(b, a.roles, (size_t)st.n_roles); rc |= dalloc(b, a.tuple_action, (size_t)st.n_tuples);
  rc |= dalloc(b, a.col_tag, (size_t)f.ncol * n); rc |= dalloc(b, a.col_val, (size_t)f.ncol * n);
  rc |= dalloc(b, a.in_span, (size_t)n * 2 * CBH_WSPAN_N); rc |= dalloc(b, a.act_span, (size_t)st.n_tuples * 2);
  if (rc != 0) return -1;
  f.have_outputs = true;
  return 0;
}

// ---- stage: the fill, once more with the heap it asked for if the guess was short.  Leaves the fill's statistics in f.st:
// CBH_WF_DICT_FULL there = the dictionary has to grow and the road start again from the scan (wire_flatten_stages)
static int wf_fill(WireFlatten& f) {
  cbh_device_batch* b = f.b; hipStream_t s = f.s; WireArgs& a = f.a; WireStats& st = f.st; const u32 nw = f.nw, ncol = f.ncol;
  for (;;) {
    if (dalloc(b, a.heap_tag, (size_t)f.heap_cap) != 0 || dalloc(b, a.heap_val, (size_t)f.heap_cap) != 0) return -1;
    a.heap_cap = f.heap_cap;
    // dynamic LDS: room for a wave's 64 messages (a quarter above the call's average; a wave whose block is larger parses in place)
    a.lds_cap = wire_fill_lds_cap(st.max_block);
    if (nw && a.lds_cap) hipLaunchKernelGGL(cbh_wire_fill_lds_kernel, dim3(nw), dim3(CBH_BLOCK), cbh_wire_fill_cur_bytes(ncol) + a.lds_cap, s, a);
    else if (nw) hipLaunchKernelGGL(cbh_wire_fill_kernel, dim3(nw), dim3(CBH_BLOCK), cbh_wire_fill_cur_bytes(ncol), s, a);
    ++f.runs;
    // what the fill wanted and the routing of what it wrote (for nothing, the rare time the fill is run again) - ONE wait for both
    if (!f.try_group && wire_publish(b, f.d_stats, wire_stats_land(b), (u32)(sizeof(st) / 4)) != 0) return -1;
    if (wf_launch_routes(f) != 0) return -1;
    wmark("fill+routes enqueued");
    if (hipStreamSynchronize(s) != hipSuccess) return fail("cbh_wire_flatten failed");
    wmark("filled");
    st = *wire_stats_land(b);
    if ((st.flags & CBH_WF_DICT_FULL) || st.heap_used <= f.heap_cap) return 0;
    f.heap_cap = st.heap_used;
    if (wire_stats_write(b, f.d_stats, wire_stats_reset(st, f.n_host_count)) != 0) return -1;
  }
}

// ---- stage: the flattened arrays become an ordinary resident batch; the grouped view where the routes were worth it.
// 1 = some message is the host flattener's
static int wf_finish(WireFlatten& f, cbh_device_batch** out) {
  cbh_device_batch* b = f.b; Replica* rep = f.rep; const WireArgs& a = f.a; const WireStats& st = f.st; cbh_wire_info* info = f.info; const u32 n = f.n;
  { const hipError_t le = hipGetLastError(); if (le != hipSuccess) return fail(std::string("cbh_wire_flatten: ") + hipGetErrorString(le)); }
  if (st.heap_used >= (1u << 30)) return fail("cbh_wire_flatten: batch too large: nested attribute values exceed the heap's 30-bit offsets");   // (as cbi_flatten_pb)
  info->n_tuples = st.n_tuples; info->n_host = st.n_host; info->dict_slots = f.slots; info->heap_len = st.heap_used; info->fill_runs = f.runs;
  if (st.first_bad != CBH_NONE) { wf_bad_input(f, st.first_bad); return -1; }
  if (st.n_host) { g_err = "cbh_wire_flatten: " + std::to_string(st.n_host) + " message(s) are the host flattener's (more than 64 actions, a resource kind to rewrite that no policy names, containers nested too deep, a map that repeats a key or has more than 256 entries)"; return 1; }
  BatchDev& d = b->dev;
  batch_set_counts(b, n, st.n_tuples, st.n_roles, f.ncol, f.slots, st.heap_used);
  d.req_u32 = a.req_u32; d.roles = a.roles; d.tuple_req = nullptr; d.tuple_action = a.tuple_action; d.col_tag = a.col_tag; d.col_val = a.col_val;
  b->w.req_input = a.req_u32;
  d.heap_tag = a.heap_tag; d.heap_val = a.heap_val; d.str_off = nullptr; d.str_bytes = f.d_msg; d.str_flags = (const u8*)a.lflags; d.str_keys = a.lix;
  b->w.in_span = a.in_span; b->w.act_span = a.act_span; b->w.moff = f.d_moff; b->w.dver_off = a.dver_off; b->w.dver_len = a.dver_len;
  const bool plain = !flat_any_forced() && !(st.flags & CBH_WF_CONTAINER_IN_SENS);
  b->shape = PlanShape{st.max_actions, st.max_roles, st.wide_hi ? st.wide_lo : 0, st.wide_hi, plain};
  const bool globs = nfa_maxw(rep->dev) != 0;   // (no automata: nobody reads the glob bits, one word stands for them)
  if (batch_device_buffers(b, globs ? (size_t)3 * f.slots : (size_t)1) != 0) return -1;
  if (globs && hipMemsetAsync(d.gbits, 0, (size_t)3 * f.slots * sizeof(u64), f.s) != hipSuccess) return fail("cbh_wire_flatten: memset failed");
  { const hipError_t le = hipGetLastError(); if (le != hipSuccess) return fail(std::string("cbh_wire_flatten: ") + hipGetErrorString(le)); }
  const u32* pin_routes = pin_at<u32>(b, b->w.pin.routes());
  if (f.try_group && pin_routes[1] == 0u && pin_routes[0] > 1u) {   // grouped (not: a full route table, or one route - nothing to group)
    d.req_u32 = f.ra.req_out; d.col_tag = f.ra.col_tag_out; d.col_val = f.ra.col_val_out;
    b->w.inv = f.ra.inv;
    if (b->shape.wide_hi) { b->shape.wide_lo = 0; b->shape.wide_hi = n; }   // the wider requests lie anywhere now: their launch skips the others lane by lane
    info->n_routes = pin_routes[0];
  }
  *out = b; f.b = nullptr;
  return 0;
}

// the stages in order; the dictionary's regrowth around the fill
static int wire_flatten_stages(cbh_table* t, uint32_t device_index, const uint8_t* bytes, const uint64_t* offsets, uint32_t n,
                               const char* default_version, const char* default_scope, const uint8_t* globals_pb, size_t globals_len,
                               cbh_device_batch** out, cbh_wire_info* info, WireChain* chain, const WireRequests* reqs) {
  WireFlatten f;
  f.chain = chain;
  if (!t || !out || !info || (n && (!bytes || !offsets)) || (globals_len && !globals_pb)) return fail("null argument");
  std::memset(info, 0, sizeof(*info));
  info->first_bad = CBH_NONE; info->n_requests = n;
  f.t = t; f.bytes = bytes; f.offsets = offsets; f.n_in = n; f.reqs = reqs; f.info = info; f.globals_len = globals_len;
  int rc = wf_open(f, device_index, default_version, default_scope, globals_pb);
  if (rc != 0) return rc;
  f.n = f.n_in;
  if (reqs) {   // (the block was asked for the requests; whether the outputs of their inputs fit it is the layout's answer)
    if ((rc = wf_split_requests(f, f.n, f.total)) != 0) return rc;
    f.b->w.pin.n = f.n; f.b->w.pin.check(0);
  }
  if ((rc = wf_upload(f)) != 0) return rc;
  wf_count(f);
  for (;;) {
    if ((rc = wf_scan(f)) != 0 || (rc = wf_fill(f)) != 0) return rc;
    if (!(f.st.flags & CBH_WF_DICT_FULL)) break;
    if (f.slots >= (1u << 30)) return fail("cbh_wire_flatten: the batch-local dictionary cannot grow further");
    f.slots *= 4;
    if (wire_stats_write(f.b, f.d_stats, wire_stats_reset(f.st, f.n_host_count)) != 0) return -1;
  }
  return wf_finish(f, out);
}
// (no exception leaves the library: the stages allocate strings and vectors; the slices' threads come through here too)
static int wire_flatten_impl(cbh_table* t, uint32_t device_index, const uint8_t* bytes, const uint64_t* offsets, uint32_t n,
                             const char* default_version, const char* default_scope, const uint8_t* globals_pb, size_t globals_len,
                             cbh_device_batch** out, cbh_wire_info* info, WireChain* chain, const WireRequests* reqs = nullptr) {
  try { return wire_flatten_stages(t, device_index, bytes, offsets, n, default_version, default_scope, globals_pb, globals_len, out, info, chain, reqs); }
  catch (...) { return fail("out of memory"); }
}
extern "C" int cbh_wire_flatten_requests(cbh_table* t, uint32_t device_index, const uint8_t* bytes, const uint64_t* offsets, uint32_t n_requests,
                                         const uint8_t* aux_bytes, const uint64_t* aux_offsets, const char* default_version, const char* default_scope,
                                         const uint8_t* globals_pb, size_t globals_len, uint32_t* first_input, uint8_t* request_flags,
                                         cbh_device_batch** out, cbh_wire_info* info) {
  if (!first_input) return fail("null argument");
  if ((aux_bytes == nullptr) != (aux_offsets == nullptr)) return fail("cbh_wire_flatten_requests: aux_bytes and aux_offsets go together");
  WireRequests rq; rq.aux = aux_bytes; rq.aux_offsets = aux_offsets; rq.first_input = first_input; rq.flags = request_flags;
  return wire_flatten_impl(t, device_index, bytes, offsets, n_requests, default_version, default_scope, globals_pb, globals_len, out, info, nullptr, &rq);
}
extern "C" int cbh_wire_flatten(cbh_table* t, uint32_t device_index, const uint8_t* bytes, const uint64_t* offsets, uint32_t n,
                                const char* default_version, const char* default_scope, const uint8_t* globals_pb, size_t globals_len,
                                cbh_device_batch** out, cbh_wire_info* info) {
  return wire_flatten_impl(t, device_index, bytes, offsets, n, default_version, default_scope, globals_pb, globals_len, out, info, nullptr);
}

// Where the strings a CheckOutput repeats sit in each message (what cbi_assemble_wire_pb reads instead of walking the messages
// again): in_span [n][6] (offset, length) pairs relative to the message - request id, principal id / version, resource kind /
// version / id; act_span [n_tuples] (offset, length) of each action; act_off [n + 1] first tuple of each input.
extern "C" int cbh_wire_spans_download(cbh_table* t, cbh_device_batch* b, uint32_t* in_span, uint32_t* act_span, uint32_t* act_off) {
  if (!t || !b || !in_span || !act_span || !act_off) return fail("null argument");
  if (!b->wire) return fail("cbh_wire_spans_download: not a batch of cbh_wire_flatten");
  Replica* rep = b->rep;
  HIPCHK(hipSetDevice(rep->device));
  const BatchDev& d = b->dev;
  const size_t n = d.n_requests;
  if (n) HIPCHK(hipMemcpyAsync(in_span, b->w.in_span, n * 2 * CBH_WSPAN_N * 4, hipMemcpyDeviceToHost, b->stream));
  if (d.n_tuples) HIPCHK(hipMemcpyAsync(act_span, b->w.act_span, (size_t)d.n_tuples * 2 * 4, hipMemcpyDeviceToHost, b->stream));
  if (n) HIPCHK(hipMemcpyAsync(act_off, b->w.req_input + (size_t)CBH_RQ_ACT_OFF * n, n * 4, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  act_off[n] = d.n_tuples;
  return 0;
}

// The serialized CheckOutputs of a batch the device flattened, written by the device (cbh_wire.h cbh_wire_out_*): after
// cbh_check_resident on `b`, three launches on its stream - sizes, scan, bytes - and one copy back.
static int wire_out_args(cbh_table* t, cbh_device_batch* b, WireOutArgs& a) {
  Replica* rep = b->rep; const BatchDev& d = b->dev; WireBatch& w = b->w;
  const u32 n = d.n_requests, nw = (n + 63u) / 64u;
  if (!w.sizes) {
    int rc = 0;
    rc |= dalloc(b, w.sizes, (size_t)n + 1); rc |= dalloc(b, w.wavesum, (size_t)nw + 1); rc |= dalloc(b, w.waveoff, (size_t)nw + 1);
    rc |= dalloc(b, w.ostats, 1); rc |= dalloc(b, w.out_off, (size_t)n + 1); rc |= dalloc(b, w.out_flags, (size_t)n + 1);
    if (rc != 0) return -1;
  }
  std::memset(&a, 0, sizeof(a));
  const TableDev& td = rep->dev;
  a.t_str_off = td.str_off; a.t_str_bytes = td.str_bytes;
  a.scope_sid = reinterpret_cast<const u32*>(static_cast<const uint8_t*>(rep->image) + t->wire.scope_sid_offset); a.n_scopes = t->wire.n_scopes;
  a.n_policies = t->wire.n_policies; a.name_off = rep->w_name_off; a.name_bytes = rep->w_name_bytes; a.n_dr = t->wire.n_dr; a.n = n;
  a.msg = d.str_bytes; a.moff = w.moff; a.dver_off = w.dver_off; a.dver_len = w.dver_len;
  a.req_u32 = w.req_input; a.tuple_action = d.tuple_action; a.in_span = w.in_span; a.act_span = w.act_span; a.inv = w.inv;
  a.effect = b->out.effect; a.policy = b->out.policy; a.scope = b->out.scope; a.status = b->out.status; a.edr = b->out.edr;
  a.sizes = w.sizes; a.wavesum = w.wavesum; a.waveoff = w.waveoff; a.stats = w.ostats; a.out_off = w.out_off; a.out_flags = w.out_flags;
  return 0;
}
// the sizes and offsets of the batch's current results: the size / scan launches, or - they ran for these results already - what they found
static int wire_out_sizes(cbh_device_batch* b, WireOutArgs& a, bool fresh_ostats, WireOutStats& st) {
  WireBatch& w = b->w; hipStream_t s = b->stream;
  std::memset(&st, 0, sizeof(st));
  if (w.total_known) { st.total = w.total; st.errors = w.out_errors; return 0; }
  WireOutStats* pin_st = pin_at<WireOutStats>(b, w.pin.slot(0));   // (the scan kernel writes it and clears the error bits behind itself)
  if (fresh_ostats) HIPCHK(hipMemsetAsync(w.ostats, 0, sizeof(st), s));
  a.host_stats = pin_dev(b, pin_st);
  if (a.n) hipLaunchKernelGGL(cbh_wire_out_size_kernel, dim3((a.n + 63u) / 64u), dim3(CBH_BLOCK), 0, s, a);
  hipLaunchKernelGGL(cbh_wire_out_scan_kernel, dim3(1), dim3(CBH_BLOCK), 0, s, a);
  HIPCHK(hipStreamSynchronize(s));
  st = *pin_st;
  w.total_known = true; w.total = st.total; w.out_errors = st.errors;
  return 0;
}
static int wire_outputs(cbh_table* t, cbh_device_batch* b, uint8_t* bytes, size_t cap, uint64_t* offsets, uint8_t* flags, size_t* need) {
  if (!t || !b || !offsets || !need || (cap && !bytes)) return fail("null argument");
  if (!b->wire) return fail("cbh_wire_outputs: not a batch of cbh_wire_flatten");
  Replica* rep = b->rep;
  HIPCHK(hipSetDevice(rep->device));
  hipStream_t s = b->stream;
  const u32 n = b->dev.n_requests, nw = (n + 63u) / 64u;
  *need = 0;
  const bool fresh_ostats = !b->w.sizes;
  WireOutArgs a;
  if (wire_out_args(t, b, a) != 0) return -1;
  // The outputs' offsets and flags are written by the kernels straight into the batch's page-locked block (where the messages'
  // offsets went up from: long since on the device) when it has the room - two copies less on the link per call, and none that
  // waits behind another slice's bulk copy; the caller's arrays are filled from there.
  const WirePin& pin = b->w.pin;
  const bool direct = b->w.pinned && pin.outputs_fit();
  u64* pin_off = direct ? pin_at<u64>(b, pin.out_offsets()) : nullptr;
  u8* pin_flags = direct ? pin_at<u8>(b, pin.out_flags()) : nullptr;
  if (direct) { a.out_off = pin_dev(b, pin_off); a.out_flags = pin_dev(b, pin_flags); }
  WireOutStats st;
  if (wire_out_sizes(b, a, fresh_ostats, st) != 0) return -1;
  if (st.errors & 1u) return fail("cbh_wire_outputs: a policy or scope id of the results is out of the table's range");
  if (st.errors & 2u) return fail("cbh_wire_outputs: a CheckOutput exceeds 16 MB");
  *need = (size_t)st.total;
  if (st.total > cap) { g_err = "cbh_wire_outputs: the output buffer is too small"; return 2; }
  // Where the bytes are written: into device memory and one copy back - or, with CBH_WIRE_OUT_DIRECT=1, into the CALLER's buffer when
  // that is page-locked memory the device can reach (the kernel's 16-byte stores cross the link themselves).  Measured on the sliced
  // road (C2, 250 000 messages per call): the direct stores run at 43 GB/s and slow the copy engine's uploads and the other slices'
  // kernels beside them - 2.17 ms a call against 1.94 ms with the copy (tools/pcie_duplex.hip: engine upload + kernel download
  // 1.16 ms, both by the engines 0.92 ms) - so the copy is the default.
  static const bool direct_on = env_is("CBH_WIRE_OUT_DIRECT", '1');
  u8* d_out = nullptr; u8* host_out = nullptr;
  if (direct_on && st.total && is_pinned(bytes) && hipHostGetDevicePointer((void**)&host_out, bytes, 0) != hipSuccess) { (void)hipGetLastError(); host_out = nullptr; }
  if (host_out) {
    a.out_bias = (u32)(reinterpret_cast<uintptr_t>(host_out) & 15u);
    a.out = host_out - a.out_bias;
  } else {
    if (dalloc(b, d_out, (size_t)st.total + 1) != 0) return -1;
    a.out = d_out; a.out_bias = 0;
  }
  a.lds_cap = wire_lds_cap(n ? (size_t)(st.total / n) * 80u + 256u : 0u, 1);
  if (nw) hipLaunchKernelGGL(cbh_wire_out_write_kernel, dim3(nw), dim3(CBH_BLOCK), a.lds_cap, s, a);
  // the bytes' way back: on the replica's download stream (the copy engine of that direction), behind an event of the kernel
  hipEvent_t ev_w = (st.total && d_out && wire_link_streams(rep)) ? wire_event(b, 0) : nullptr, ev_d = ev_w ? wire_event(b, 1) : nullptr;
  if (ev_w && ev_d && hipEventRecord(ev_w, s) == hipSuccess && hipStreamWaitEvent(rep->down_stream, ev_w, 0) == hipSuccess) {
    HIPCHK(hipMemcpyAsync(bytes, d_out, (size_t)st.total, hipMemcpyDeviceToHost, rep->down_stream));
    if (hipEventRecord(ev_d, rep->down_stream) != hipSuccess) {   // the copy flies with nothing to wait on but its stream
      (void)hipGetLastError(); (void)hipStreamSynchronize(rep->down_stream);
      return fail("cbh_wire_outputs: hipEventRecord failed behind the download");
    }
  } else {
    ev_d = nullptr;
    if (st.total && d_out) HIPCHK(hipMemcpyAsync(bytes, d_out, (size_t)st.total, hipMemcpyDeviceToHost, s));
  }
  if (!direct) {
    HIPCHK(hipMemcpyAsync(offsets, b->w.out_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, s));
    if (flags && n) HIPCHK(hipMemcpyAsync(flags, b->w.out_flags, (size_t)n, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  if (ev_d) HIPCHK(hipEventSynchronize(ev_d));
  HIPCHK(hipGetLastError());
  if (direct) {
    std::memcpy(offsets, pin_off, ((size_t)n + 1) * 8);
    if (flags && n) std::memcpy(flags, pin_flags, (size_t)n);
  }
  if (d_out) {   // the output block goes back to the pool now: a batch that is asked again allocates again
    std::lock_guard<std::mutex> lk(rep->pool_mu);
    for (size_t i = b->allocs.size(); i-- > 0;) if (b->allocs[i].first == d_out) { rep->pool_free.push_back(b->allocs[i]); b->allocs.erase(b->allocs.begin() + (long)i); break; }
  }
  return 0;
}
extern "C" int cbh_wire_outputs(cbh_table* t, cbh_device_batch* b, uint8_t* bytes, size_t cap, uint64_t* offsets, uint8_t* flags, size_t* need) {
  try { return wire_outputs(t, b, bytes, cap, offsets, flags, need); } catch (...) { return fail("out of memory"); }
}

// Bytes in, bytes out in ONE call: serialized CheckInputs -> serialized CheckOutputs by the device road (cbh_wire_flatten,
// cbh_check_resident, cbh_wire_outputs), the call cut into up to four slices of contiguous messages that go down the road side
// by side, each on a thread and a stream of its own - one slice's copies run under another's kernels, which a single caller
// thread making the three calls in a row never gets (its H2D, kernels and D2H queue behind each other).  The slices' outputs
// land back to back in `out_bytes`: every slice first learns its size (the size / scan launches), the bases follow, then each
// writes and copies into its own range.  Returns 0; 1 = some message is the host flattener's (info->n_host; nothing was
// written); 2 = `out_cap` is too small, *need holds the size; < 0 error.
//
// The same for what the SERVER receives (`rm`): the units are serialized CheckResourcesRequests, a slice is a range of requests, its
// CheckInputs are made on the device (cbh_wire_req.h); the outputs of request r are out_offsets[first_input[r]] ..
// out_offsets[first_input[r + 1]]; with `rm->effective_policies` every request also gets its audit trail (one group per request:
// the one decision-log entry svc.CheckResources writes for the call).  2 also when out_offsets / out_flags hold fewer inputs than the
// requests have (info->n_requests = the inputs).
struct WireReqMode {
  const uint8_t* aux = nullptr; const uint64_t* aux_offsets = nullptr;
  uint32_t* first_input = nullptr; uint8_t* request_flags = nullptr; size_t out_inputs_cap = 0;
  uint32_t* effective_policies = nullptr;
};
struct WireSlice {
  u32 lo = 0, hi = 0; cbh_device_batch* b = nullptr; cbh_wire_info wi{}; size_t total = 0, base = 0; int rc = 0; std::string err;
  std::vector<uint64_t> off, ooff, aoff; std::vector<uint32_t> first; u32 n_in = 0, in_base = 0;
};
// One sliced call: its arguments and what the slices' threads share.
struct WireSliced {
  cbh_table* t; uint32_t device_index; const uint8_t* bytes; const uint64_t* offsets; u32 n;
  const char* default_version; const char* default_scope; const uint8_t* globals_pb; size_t globals_len;
  const cbh_params* p; uint8_t* out_bytes; size_t out_cap; uint64_t* out_offsets; uint8_t* out_flags; const WireReqMode* rm;
  u32 S = 1, words = 0; size_t inputs_cap = 0;
  std::vector<WireSlice> sl;
  std::vector<hipEvent_t> evs; std::vector<std::atomic<int>> recorded; std::vector<WireChain> chains;   // the slices' uploads in slice order (WireChain)
  std::vector<std::atomic<int>> sized;   // 0 not yet, 1 size known, 2 failed
  std::atomic<int> overflow{0};
  std::chrono::steady_clock::time_point call_t0; std::vector<WireMarks> marks;
  std::vector<std::thread> th;
  ~WireSliced() {
    for (auto& q : th) if (q.joinable()) q.join();
    for (auto& x : sl) if (x.b) cbh_batch_release(x.b);
    for (auto e : evs) if (e) (void)hipEventDestroy(e);
  }
};
// how many slices, and which messages (requests) each takes
static void ws_cut(WireSliced& c, int calls_in_flight) {
  const u32 n = c.n;
  static const u32 max_slices = (u32)std::min<long>(std::max<long>(env_long("CBH_WIRE_SLICES", 4), 1), 8);
  // (requests: by their bytes - a request holds any number of resource entries -, about 4 MB to a slice.  CBH_WIRE_SLICE_MIN /
  // CBH_WIRE_SLICE_MIN_BYTES: the smallest slice, for tests and measurements)
  static const u32 slice_min = (u32)std::max<long>(env_long("CBH_WIRE_SLICE_MIN", 16384), 1);
  static const u64 slice_min_bytes = (u64)std::max<long>(env_long("CBH_WIRE_SLICE_MIN_BYTES", 1l << 22), 1);
  const u32 share = std::max<u32>(1u, max_slices / (u32)std::max(1, calls_in_flight));
  c.S = std::max<u32>(1u, std::min<u32>(share, c.rm ? (u32)std::min<u64>(n, (n ? c.offsets[n] : 0) / slice_min_bytes) : n / slice_min));
  const u32 S = c.S;
  c.sl.resize(S);
  // Even slices.  (A smaller LAST slice - what the call waits for at the end is that slice's road after the last message has gone up -
  // was measured and lost: 1.98 ms a call against 1.79 ms, the larger slices in front delay everything behind them.
  // CBH_WIRE_LAST_SLICE=percent of an even share for the last one.)
  static const double last_share = [] { const double v = env_double("CBH_WIRE_LAST_SLICE", 100.0) / 100.0; return v < 0.1 ? 0.1 : v > 1.0 ? 1.0 : v; }();
  const double unit = (double)n / ((double)(S - 1) + (S > 1 ? last_share : 1.0));
  u32 at = 0;
  for (u32 k = 0; k < S; ++k) {
    c.sl[k].lo = at;
    at = (k + 1 == S) ? n : std::min<u32>(n, (u32)(unit * (double)(k + 1) + 0.5));
    if (at < c.sl[k].lo) at = c.sl[k].lo;
    c.sl[k].hi = at;
  }
}
// the slices' uploads in slice order: an event and a flag per slice, each slice waits for its predecessor's
static int ws_chain(WireSliced& c) {
  const u32 S = c.S;
  c.evs.assign(S, nullptr);
  c.recorded = std::vector<std::atomic<int>>(S);
  c.chains.resize(S);
  for (u32 k = 0; k < S; ++k) {
    c.recorded[k].store(0);
    if (S > 1 && hipEventCreateWithFlags(&c.evs[k], hipEventDisableTiming) != hipSuccess) return fail("cbh_wire_check_pb: hipEventCreate failed");
    c.chains[k].record = c.evs[k]; c.chains[k].recorded = &c.recorded[k];
    if (k) { c.chains[k].wait = c.evs[k - 1]; c.chains[k].prev_recorded = &c.recorded[k - 1]; }
  }
  return 0;
}
// the trail of a slice of requests (cbh_check_batch_trail with one group per REQUEST): the inputs' groups follow from the split's
// first_input; a batch the flattener grouped by route keeps its results by position, so the groups move with the inputs
static int ws_trail_on(const WireSliced& c, WireSlice& x, u32*& d_ep) {
  cbh_device_batch* b = x.b;
  hipStream_t s = b->stream;
  const u32 cnt = x.hi - x.lo, words = c.words;
  const size_t ep_n = (size_t)(cnt ? cnt : 1u) * (words ? words : 1u);
  if (dalloc(b, d_ep, ep_n) != 0) return -1;
  HIPCHK(hipMemsetAsync(d_ep, 0, ep_n * 4, s));
  u32* d_grp = nullptr;
  if (x.n_in) {
    std::vector<u32> grp(x.n_in);
    for (u32 r = 0; r < cnt; ++r) for (u32 i = x.first[r]; i < x.first[r + 1]; ++i) grp[i] = r;
    u32* d_by_input = nullptr;
    if (dalloc(b, d_by_input, (size_t)x.n_in) != 0) return -1;
    HIPCHK(hipMemcpyAsync(d_by_input, grp.data(), (size_t)x.n_in * 4, hipMemcpyHostToDevice, s));
    d_grp = d_by_input;
    if (b->w.inv) {
      if (dalloc(b, d_grp, (size_t)x.n_in) != 0) return -1;
      WireScatterArgs sa; sa.by_input = d_by_input; sa.inv = b->w.inv; sa.by_position = d_grp; sa.n = x.n_in; sa.pad = 0;
      const u32 n_in = x.n_in;
      hipLaunchKernelGGL(cbh_wire_scatter_u32_kernel, dim3((n_in + 255u) / 256u), dim3(256), 0, s, sa);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(s));   // (grp is a pageable source going out of scope)
  }
  b->out.eff_pol = d_ep; b->out.ep_words = words; b->dev.ep_group = d_grp;
  return 0;
}
// stage 1 (per slice): flatten, decide, sizes of the outputs
static void ws_stage1(WireSliced& c, u32 k) {
  WireSlice& x = c.sl[k];
  const u32 n = c.n, cnt = x.hi - x.lo; const WireReqMode* rm = c.rm;
  x.off.resize((size_t)cnt + 1);
  const uint64_t o0 = n ? c.offsets[x.lo] : 0;
  for (u32 i = 0; i <= cnt; ++i) x.off[i] = (n ? c.offsets[x.lo + i] : 0) - o0;
  WireRequests rq;
  if (rm) {
    x.first.assign((size_t)cnt + 1, 0u);
    rq.first_input = x.first.data(); rq.flags = rm->request_flags ? rm->request_flags + x.lo : nullptr;
    if (rm->aux_offsets) {
      const uint64_t a0 = n ? rm->aux_offsets[x.lo] : 0;
      x.aoff.resize((size_t)cnt + 1);
      for (u32 i = 0; i <= cnt; ++i) x.aoff[i] = (n ? rm->aux_offsets[x.lo + i] : 0) - a0;   // (out of order: the device refuses the request)
      rq.aux = rm->aux ? rm->aux + a0 : nullptr; rq.aux_offsets = x.aoff.data();
    }
  }
  x.rc = wire_flatten_impl(c.t, c.device_index, c.bytes ? c.bytes + o0 : nullptr, x.off.data(), cnt, c.default_version, c.default_scope, c.globals_pb, c.globals_len,
                           &x.b, &x.wi, c.S > 1 ? &c.chains[k] : nullptr, rm ? &rq : nullptr);
  if (x.rc != 0) { x.err = g_err; x.b = nullptr; return; }
  x.n_in = x.wi.n_requests;   // the slice's messages (requests: the inputs made of them)
  cbh_params q = *c.p;
  q.flags &= ~(u32)CBH_F_WANT_EFFECTIVE_POLICIES;
  u32* d_ep = nullptr;
  if (rm && rm->effective_policies) {
    if (ws_trail_on(c, x, d_ep) != 0) { x.rc = -1; x.err = g_err; return; }
    q.flags |= CBH_F_WANT_EFFECTIVE_POLICIES;
  }
  wmark("flattened");
  x.rc = cbh_check_resident(c.t, x.b, &q);
  if (x.rc != 0) { x.err = g_err; return; }
  wmark("decision enqueued");
  if (d_ep && c.words && cnt) {
    if (hipMemcpyAsync(rm->effective_policies + (size_t)x.lo * c.words, d_ep, (size_t)cnt * c.words * 4, hipMemcpyDeviceToHost, x.b->stream) != hipSuccess ||
        hipStreamSynchronize(x.b->stream) != hipSuccess) { x.rc = fail("cbh_wire_check_requests_trail_pb: download failed"); x.err = g_err; return; }
  }
  x.ooff.resize((size_t)x.n_in + 1);
  size_t nd = 0;
  const int r = wire_outputs(c.t, x.b, nullptr, 0, x.ooff.data(), nullptr, &nd);   // cap 0: sizes only (2 = "too small" unless the slice has no output bytes)
  if (r != 0 && r != 2) { x.rc = r; x.err = g_err; return; }
  x.total = nd;
  wmark("sizes known");
}
// stage 2 (per slice): the bytes, into the slice's own range of the caller's buffer
static void ws_stage2(WireSliced& c, u32 k) {
  WireSlice& x = c.sl[k];
  size_t nd = 0;
  x.rc = wire_outputs(c.t, x.b, c.out_bytes + x.base, x.total, x.ooff.data(), c.out_flags ? c.out_flags + x.in_base : nullptr, &nd);
  if (x.rc != 0) { x.err = g_err; return; }
  for (u32 i = 0; i <= x.n_in; ++i) c.out_offsets[x.in_base + i] = x.ooff[i] + x.base;
  wmark("written + copied back");
}
// A slice writes as soon as the slices before it know their sizes (its base is their sum): no barrier between the stages, so
// the first slice's answers are on their way back while the last slice's messages are still going up.  A slice that failed,
// or met a message for the host flattener, publishes "no size": nobody writes after that.
static void ws_work_body(WireSliced& c, u32 k) {
  ws_stage1(c, k);
  WireSlice& x = c.sl[k];
  c.sized[k].store(x.rc == 0 ? 1 : 2, std::memory_order_release);
  if (x.rc != 0) return;
  size_t base = 0; u32 in_base = 0;
  for (u32 j = 0; j < k; ++j) {
    int st;
    while ((st = c.sized[j].load(std::memory_order_acquire)) == 0) std::this_thread::yield();
    if (st == 2) return;
    base += c.sl[j].total; in_base += c.sl[j].n_in;
  }
  x.base = base; x.in_base = in_base;
  wmark("predecessors sized");
  if (base + x.total > c.out_cap || (size_t)in_base + x.n_in > c.inputs_cap) { c.overflow.store(1); return; }
  ws_stage2(c, k);
}
// a slice's thread (slice 0: the caller's).  No exception leaves it: the slice fails, and says so to the slices that wait for its size
static void ws_work(WireSliced& c, u32 k) {
  if (!c.marks.empty()) { c.marks[k].t0 = c.call_t0; tl_marks = &c.marks[k]; }
  struct Untrace { ~Untrace() { tl_marks = nullptr; } } untrace;
  wmark("thread runs");
  try { ws_work_body(c, k); }
  catch (...) {
    WireSlice& x = c.sl[k];
    x.rc = -1; x.err = "out of memory";
    if (c.recorded[k].load() == 0) c.recorded[k].store(1, std::memory_order_release);
    if (c.sized[k].load() == 0) c.sized[k].store(2, std::memory_order_release);
  }
}
// CBH_TRACE=1: a line per slice, its marks in microseconds since the call began (tools read these lines)
static void ws_print_marks(const WireSliced& c) {
  const double end = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - c.call_t0).count();
  for (u32 k = 0; k < c.S; ++k) {
    std::string line = "[cbh] wire slice " + std::to_string(k) + ":";
    for (auto& m : c.marks[k].v) { char buf[96]; std::snprintf(buf, sizeof(buf), "  %s %.0f", m.first, m.second); line += buf; }
    std::fprintf(stderr, "%s  | joined %.0f us\n", line.c_str(), end);
  }
}
// the slices' results as the call's: counts summed, the first failure's message, the requests' first inputs in call order
static int ws_gather(WireSliced& c, size_t* need, cbh_wire_info* info) {
  const WireReqMode* rm = c.rm;
  int rc = 0; std::string err;
  size_t total = 0; u64 inputs = 0;
  for (auto& x : c.sl) {
    info->n_tuples += x.wi.n_tuples; info->n_host += x.wi.n_host; info->heap_len += x.wi.heap_len; info->dict_slots += x.wi.dict_slots;
    info->fill_runs = std::max(info->fill_runs, x.wi.fill_runs); info->n_routes = std::max(info->n_routes, x.wi.n_routes);
    if (x.wi.first_bad != CBH_NONE && info->first_bad == CBH_NONE) info->first_bad = x.lo + x.wi.first_bad;
    if (x.rc < 0 && rc >= 0) { rc = x.rc; err = x.err; }
    else if (x.rc == 1 && rc == 0) { rc = 1; err = x.err; }
    total += x.total;
    if (rm && x.rc == 0) { for (u32 r = 0; r <= x.hi - x.lo; ++r) rm->first_input[x.lo + r] = (u32)inputs + x.first[r]; }
    inputs += x.n_in;
  }
  for (auto& x : c.sl) if (x.b) { cbh_batch_release(x.b); x.b = nullptr; }
  if (rm) info->n_requests = (u32)inputs;
  if (rc != 0) { g_err = err; return rc; }
  *need = total;
  if (c.overflow.load() || total > c.out_cap || inputs > c.inputs_cap) {
    g_err = rm ? "cbh_wire_check_requests_pb: the output buffer (or out_offsets / out_flags) is too small" : "cbh_wire_check_pb: the output buffer is too small";
    return 2;
  }
  if (inputs == 0 && c.out_offsets) c.out_offsets[0] = 0;
  return 0;
}
static int wire_check_sliced_stages(cbh_table* t, uint32_t device_index, const uint8_t* bytes, const uint64_t* offsets, uint32_t n,
                                    const char* default_version, const char* default_scope, const uint8_t* globals_pb, size_t globals_len,
                                    const cbh_params* p, uint8_t* out_bytes, size_t out_cap, uint64_t* out_offsets, uint8_t* out_flags,
                                    size_t* need, cbh_wire_info* info, const WireReqMode* rm) {
  TableRef ref(t);
  std::memset(info, 0, sizeof(*info));
  info->first_bad = CBH_NONE; info->n_requests = rm ? 0u : n;
  *need = 0;
  // Calls of the road that are in flight at once (several caller threads, or one with cbh_wire_check_pb_submit) share the link and
  // the copy engines: more than about four slices side by side lose (a lone call cut into eight: 392 M against 489 M decisions/s,
  // profiles/r04_wire_onecall.txt; two calls of four: 420 M against 545 M one at a time, round 6) - so a call takes its share of four.
  static std::atomic<int> in_flight{0};
  struct InFlight { std::atomic<int>& c; int k; explicit InFlight(std::atomic<int>& c_) : c(c_), k(c_.fetch_add(1) + 1) {} ~InFlight() { c.fetch_sub(1); } } mine(in_flight);
  WireSliced c{t, device_index, bytes, offsets, n, default_version, default_scope, globals_pb, globals_len, p, out_bytes, out_cap, out_offsets, out_flags, rm};
  ws_cut(c, mine.k);
  c.words = (t->wire.n_policies + 31u) / 32u;
  if (device_index >= t->reps.size()) return fail("device index out of range");
  HIPCHK(hipSetDevice(t->reps[device_index]->device));
  if (ws_chain(c) != 0) return -1;
  c.sized = std::vector<std::atomic<int>>(c.S);
  for (auto& q : c.sized) q.store(0);
  c.inputs_cap = rm ? (out_offsets ? rm->out_inputs_cap : 0) : (size_t)n;
  c.call_t0 = std::chrono::steady_clock::now();
  c.marks.resize(trace_on() ? c.S : 0);
  u32 started = 1;   // (slice 0 runs on this thread)
  try { for (; started < c.S; ++started) c.th.emplace_back([&c, started] { ws_work(c, started); }); }
  catch (...) {   // a thread could not be made: its slice and those behind it fail at once, so that nobody waits for their uploads or sizes
    for (u32 k = started; k < c.S; ++k) {
      c.sl[k].rc = fail("cbh_wire_check_pb: cannot start a slice's thread"); c.sl[k].err = g_err;
      c.recorded[k].store(1, std::memory_order_release); c.sized[k].store(2, std::memory_order_release);
    }
  }
  ws_work(c, 0);
  for (auto& q : c.th) q.join();
  if (!c.marks.empty()) ws_print_marks(c);
  return ws_gather(c, need, info);
}
// (no exception leaves the library: the call allocates vectors and strings and starts threads)
static int wire_check_sliced(cbh_table* t, uint32_t device_index, const uint8_t* bytes, const uint64_t* offsets, uint32_t n,
                             const char* default_version, const char* default_scope, const uint8_t* globals_pb, size_t globals_len,
                             const cbh_params* p, uint8_t* out_bytes, size_t out_cap, uint64_t* out_offsets, uint8_t* out_flags,
                             size_t* need, cbh_wire_info* info, const WireReqMode* rm) {
  try { return wire_check_sliced_stages(t, device_index, bytes, offsets, n, default_version, default_scope, globals_pb, globals_len, p, out_bytes, out_cap, out_offsets, out_flags, need, info, rm); }
  catch (...) { return fail("out of memory"); }
}
extern "C" int cbh_wire_check_pb(cbh_table* t, uint32_t device_index, const uint8_t* bytes, const uint64_t* offsets, uint32_t n,
                                 const char* default_version, const char* default_scope, const uint8_t* globals_pb, size_t globals_len,
                                 const cbh_params* p, uint8_t* out_bytes, size_t out_cap, uint64_t* out_offsets, uint8_t* out_flags,
                                 size_t* need, cbh_wire_info* info) {
  if (!t || !p || !out_offsets || !need || !info || (n && (!bytes || !offsets)) || (out_cap && !out_bytes)) return fail("null argument");
  return wire_check_sliced(t, device_index, bytes, offsets, n, default_version, default_scope, globals_pb, globals_len, p, out_bytes, out_cap, out_offsets, out_flags,
                           need, info, nullptr);
}
// ---- the same call without blocking the caller (include/cerbos_hip.h cbh_wire_check_pb_submit / _collect).  The ticket owns a
// worker thread that makes the synchronous call; the strings are copied, the buffers are the caller's and stay untouched until
// collect.  A caller that keeps two tickets in flight has the second call's uploads under the first's downloads - the fill and
// drain of one call's slices are what a lone synchronous caller pays on top of the link's own time.
struct cbh_wire_ticket {
  cbh_table* table = nullptr;   // (the reference submit took: released by collect, whatever table the caller names there)
  std::thread worker;
  std::string ver, scope, err;
  int rc = -1;
  size_t need = 0;
  cbh_wire_info info{};
};
extern "C" int cbh_wire_check_pb_submit(cbh_table* t, uint32_t device_index, const uint8_t* bytes, const uint64_t* offsets, uint32_t n,
                                        const char* default_version, const char* default_scope, const uint8_t* globals_pb, size_t globals_len,
                                        const cbh_params* p, uint8_t* out_bytes, size_t out_cap, uint64_t* out_offsets, uint8_t* out_flags,
                                        cbh_wire_ticket** ticket) {
  if (!ticket) return fail("null argument");
  *ticket = nullptr;
  if (!t || !p || !out_offsets || (n && (!bytes || !offsets)) || (out_cap && !out_bytes)) return fail("null argument");
  cbh_wire_ticket* k = new (std::nothrow) cbh_wire_ticket();
  if (!k) return fail("out of memory");
  k->ver = default_version ? default_version : ""; k->scope = default_scope ? default_scope : "";
  const bool has_ver = default_version != nullptr, has_scope = default_scope != nullptr;
  const cbh_params params = *p;
  cbh_table_retain(t);   // the table outlives the call whatever the caller does with its own reference meanwhile
  k->table = t;
  try {
    k->worker = std::thread([=]() {
      // (wire_check_sliced lets no exception out; the copy of the message below may still run out of memory - the process must not end for it)
      try {
        k->rc = wire_check_sliced(t, device_index, bytes, offsets, n, has_ver ? k->ver.c_str() : nullptr, has_scope ? k->scope.c_str() : nullptr, globals_pb, globals_len,
                                  &params, out_bytes, out_cap, out_offsets, out_flags, &k->need, &k->info, nullptr);
        if (k->rc != 0) k->err = g_err;   // (the worker's own thread-local message: handed to the collecting thread)
      } catch (...) { k->rc = -1; try { k->err = "out of memory"; } catch (...) {} }
    });
  } catch (...) { cbh_table_release(t); delete k; return fail("cbh_wire_check_pb_submit: cannot start a worker thread"); }
  *ticket = k;
  return 0;
}
extern "C" int cbh_wire_check_pb_collect(cbh_table* t, cbh_wire_ticket* ticket, size_t* need, cbh_wire_info* info) {
  if (!ticket) return fail("null argument");
  if (t && t != ticket->table) return fail("cbh_wire_check_pb_collect: the ticket was issued for another table");   // (the ticket stays valid)
  if (ticket->worker.joinable()) ticket->worker.join();
  const int rc = ticket->rc;
  if (need) *need = ticket->need;
  if (info) *info = ticket->info;
  if (rc != 0) g_err = ticket->err;
  cbh_table* held = ticket->table;
  delete ticket;
  cbh_table_release(held);   // submit's reference
  return rc;
}
static int wire_check_requests_impl(cbh_table* t, uint32_t device_index, const uint8_t* bytes, const uint64_t* offsets, uint32_t n_requests,
                                    const uint8_t* aux_bytes, const uint64_t* aux_offsets, const char* default_version, const char* default_scope,
                                    const uint8_t* globals_pb, size_t globals_len, const cbh_params* p, uint32_t* first_input, uint8_t* request_flags,
                                    uint8_t* out_bytes, size_t out_cap, uint64_t* out_offsets, uint8_t* out_flags, size_t out_inputs_cap, size_t* need,
                                    cbh_wire_info* info, uint32_t* effective_policies) {
  if (!t || !p || !need || !info || !first_input || (n_requests && (!bytes || !offsets)) || (out_cap && !out_bytes)) return fail("null argument");
  if ((aux_bytes == nullptr) != (aux_offsets == nullptr)) return fail("cbh_wire_check_requests_pb: aux_bytes and aux_offsets go together");
  WireReqMode rm;
  rm.aux = aux_bytes; rm.aux_offsets = aux_offsets; rm.first_input = first_input; rm.request_flags = request_flags; rm.out_inputs_cap = out_inputs_cap;
  rm.effective_policies = effective_policies;
  return wire_check_sliced(t, device_index, bytes, offsets, n_requests, default_version, default_scope, globals_pb, globals_len, p, out_bytes, out_cap,
                           out_offsets, out_flags, need, info, &rm);
}
extern "C" int cbh_wire_check_requests_pb(cbh_table* t, uint32_t device_index, const uint8_t* bytes, const uint64_t* offsets, uint32_t n_requests,
                                          const uint8_t* aux_bytes, const uint64_t* aux_offsets, const char* default_version, const char* default_scope,
                                          const uint8_t* globals_pb, size_t globals_len, const cbh_params* p, uint32_t* first_input, uint8_t* request_flags,
                                          uint8_t* out_bytes, size_t out_cap, uint64_t* out_offsets, uint8_t* out_flags, size_t out_inputs_cap, size_t* need,
                                          cbh_wire_info* info) {
  return wire_check_requests_impl(t, device_index, bytes, offsets, n_requests, aux_bytes, aux_offsets, default_version, default_scope, globals_pb, globals_len, p,
                                  first_input, request_flags, out_bytes, out_cap, out_offsets, out_flags, out_inputs_cap, need, info, nullptr);
}
// ... and with the audit trail of every request: effective_policies[r * words + w] (words = (cbh_table_num_policies + 31) / 32) has bit
// k set when policy k was among those the engine went through for ANY resource entry of request r - AuditTrail.EffectivePolicies of
// the one decision-log entry the server writes for the call (check.go:302-304, svc CheckResources: one entry per request).
extern "C" int cbh_wire_check_requests_trail_pb(cbh_table* t, uint32_t device_index, const uint8_t* bytes, const uint64_t* offsets, uint32_t n_requests,
                                                const uint8_t* aux_bytes, const uint64_t* aux_offsets, const char* default_version, const char* default_scope,
                                                const uint8_t* globals_pb, size_t globals_len, const cbh_params* p, uint32_t* first_input, uint8_t* request_flags,
                                                uint8_t* out_bytes, size_t out_cap, uint64_t* out_offsets, uint8_t* out_flags, size_t out_inputs_cap, size_t* need,
                                                cbh_wire_info* info, uint32_t* effective_policies) {
  if (!effective_policies) return fail("null argument");
  return wire_check_requests_impl(t, device_index, bytes, offsets, n_requests, aux_bytes, aux_offsets, default_version, default_scope, globals_pb, globals_len, p,
                                  first_input, request_flags, out_bytes, out_cap, out_offsets, out_flags, out_inputs_cap, need, info, effective_policies);
}
