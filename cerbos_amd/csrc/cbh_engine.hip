// libcerbos_hip.so - MI355X (gfx950 / CDNA4) batched decision engine for the Cerbos
// CheckResources hot path.  Hand-written HIP; no MFMA (branchy integer / string-id work,
// HBM- and VALU-issue bound).
//
// Kernels
//   cbh_resolve_globs_kernel : one lane per batch-local string; bit-parallel glob NFA
//                              (LDS-staged transition tables) -> match bits per dimension.
//                              Replaces gobwas glob.Match per query
//                              (internal/ruletable/index/glob_dimension.go:62-95).
//   cbh_check_kernel*        : one lane per CheckInput (its actions as a bit mask), wave-uniform
//                              table walk (cbh_check_wave.h); restates
//                              ruletable.(*RuleTable).check (internal/ruletable/check.go:97-460),
//                              Index.Query + appendRolePolicyDenies
//                              (internal/ruletable/index/index.go:214-530), GetAllScopes
//                              (internal/ruletable/ruletable.go:848-882) over the flat table image.
//
// Host side: the C ABI of include/cerbos_hip.h.
//   * a table = one replica of the image per device of the engine (broadcast once: RCCL, or peer copies);
//   * cbh_check_batch = the reference's fan-out (engine.go:309-338) as contiguous request ranges over the
//     devices, each range pipelined in chunks over three streams (upload / kernels / download overlap);
//   * tables are reference counted, so a released table drains its in-flight batches (manager.go:86-124).
// This file is the core - errors, the engine, a table and its replicas, a resident batch and the pool its buffers come from -
// and includes the roads, host-only headers, at its end: cbh_host_resident.h, cbh_host_cross.h, cbh_host_wire.h, cbh_host_oneshot.h
// (and cbh_host_env.h, how the CBH_* variables are read, in front of everything).  One translation unit, as before.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <dlfcn.h>
#include <map>
#include <tuple>

#include <algorithm>
#include <atomic>
#include <cassert>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "cbh_kernels.h"
#include "cbh_image.h"
#include "cbh_wire_host.h"

// ======================================================================== host code
// (skipped in the device compilation pass, where the device structs carry address-space qualifiers)
#if !defined(__HIP_DEVICE_COMPILE__)

#include "cbh_host_env.h"        // how a CBH_* variable is read

static thread_local std::string g_err;
static int fail(const std::string& m) { g_err = m; return -1; }
#define HIPCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) return fail(std::string(#x) + ": " + hipGetErrorString(_e)); } while (0)

// ---- engine-wide state -------------------------------------------------------------------------------------
struct Rccl {   // the few RCCL entry points the image broadcast needs, bound at first use (no link-time dependency:
                // a single-GPU deployment never loads the collective library)
  void* lib = nullptr;
  int (*CommInitAll)(void**, int, const int*) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  std::vector<void*> comms;
  bool tried = false, ok = false;
};
static struct Engine {
  std::mutex mu;
  bool inited = false;
  std::vector<int> devices;
  Rccl rccl;
} g_eng;

// CBH_TRACE=1: one line per one-shot call on stderr (path taken, phase times) - measurement aid
static bool trace_on() { static const bool on = env_set("CBH_TRACE"); return on; }
// ... and, for the sliced road (cbh_wire_check_pb), the phases of every slice's thread: marks of (label, microseconds since the call began)
struct WireMarks { std::chrono::steady_clock::time_point t0; std::vector<std::pair<const char*, double>> v; };
static thread_local WireMarks* tl_marks = nullptr;
static inline void wmark(const char* label) {
  if (tl_marks) tl_marks->v.push_back({label, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tl_marks->t0).count()});
}
static double now_us() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3; }
// CBH_SPIN=1: wait for a stream by polling hipStreamQuery instead of hipStreamSynchronize
static hipError_t stream_wait(hipStream_t s) {
  static const bool spin = env_is("CBH_SPIN", '1');
  if (!spin) return hipStreamSynchronize(s);
  for (;;) { const hipError_t e = hipStreamQuery(s); if (e != hipErrorNotReady) return e; }
}
static const size_t SMALL_BATCH_BYTES = (size_t)1 << 20;   // inputs under this: one staged copy each way
static const u32 SHARD_MIN_REQUESTS = 8192;                 // a device is given at least this many requests
static const int N_STREAMS = 3;

extern "C" const char* cbh_last_error(void) { return g_err.c_str(); }
extern "C" uint32_t cbh_abi_version(void) { return CBH_ABI_VERSION; }

extern "C" int cbh_init(const cbh_config* cfg) {
  if (cfg && cfg->abi_version != CBH_ABI_VERSION) return fail("ABI version mismatch");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0) return fail("no HIP device available: the decision engine requires an MI355X (no CPU fallback)");
  std::vector<int> devs;
  if (cfg && cfg->n_devices) {
    if (cfg->n_devices > CBH_MAX_DEVICES) return fail("too many devices");
    for (u32 i = 0; i < cfg->n_devices; ++i) {
      if (cfg->devices[i] < 0 || cfg->devices[i] >= n) return fail("invalid device ordinal");
      devs.push_back(cfg->devices[i]);
    }
  } else {
    for (int i = 0; i < n && i < (int)CBH_MAX_DEVICES; ++i) devs.push_back(i);
    if (!cfg) devs.resize(1);   // no configuration: the first device only
  }
  for (int d : devs) { HIPCHK(hipSetDevice(d)); HIPCHK(hipFree(nullptr)); }   // create the contexts now, not under a request
  // peer access between the engine's devices (image broadcast by peer copy, should RCCL be unavailable)
  for (int a : devs) for (int b : devs) if (a != b) {
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, a, b) == hipSuccess && can) { (void)hipSetDevice(a); (void)hipDeviceEnablePeerAccess(b, 0); (void)hipGetLastError(); }
  }
  HIPCHK(hipSetDevice(devs[0]));
  std::lock_guard<std::mutex> lk(g_eng.mu);
  g_eng.devices = devs;
  g_eng.inited = true;
  return 0;
}

extern "C" void cbh_shutdown(void) {
  std::lock_guard<std::mutex> lk(g_eng.mu);
  Rccl& r = g_eng.rccl;
  if (r.ok) for (void* c : r.comms) if (c) (void)r.CommDestroy(c);
  r.comms.clear(); r.ok = false; r.tried = false;
  if (r.lib) { dlclose(r.lib); r.lib = nullptr; }
  g_eng.inited = false;
  g_eng.devices.clear();
}
extern "C" uint32_t cbh_num_devices(void) { std::lock_guard<std::mutex> lk(g_eng.mu); return (uint32_t)g_eng.devices.size(); }
extern "C" int32_t cbh_device_ordinal(uint32_t i) { std::lock_guard<std::mutex> lk(g_eng.mu); return i < g_eng.devices.size() ? g_eng.devices[i] : -1; }

extern "C" void* cbh_alloc_pinned(size_t bytes) {
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); g_err = "hipHostMalloc failed"; return nullptr; }
  return p;
}
extern "C" void cbh_free_pinned(void* p) { if (p) (void)hipHostFree(p); }

// ---- tables -----------------------------------------------------------------------------------------------
struct OneShot {   // what one cbh_check_batch call owns on one device while it runs
  hipStream_t s[N_STREAMS] = {nullptr, nullptr, nullptr};
  hipEvent_t ev_setup = nullptr;
  hipEvent_t ev_piece[N_STREAMS] = {nullptr, nullptr, nullptr};   // the pieces of a slab upload (run_range)
  uint8_t* h = nullptr; size_t h_cap = 0;   // pinned staging block (small batches)
  uint8_t* d = nullptr; size_t d_cap = 0;   // device block
};

struct Replica {   // the table on one device
  int device = 0;
  void* image = nullptr; bool owns_image = true;
  TableDev dev{};
  hipStream_t stream = nullptr;   // resident path (and the image broadcast)
  // Resident batches are dealt round-robin to a few streams - a batch keeps the one it was uploaded on, so everything that
  // touches it stays ordered - and launches of consecutive batches overlap: the dispatch ramp of one fills the CUs the
  // drain of the one before leaves idle (~40 % of a 15 us launch is ramp + drain, profiles/r02_cycles_flat_C2.txt).
  static constexpr int MAX_RESIDENT_STREAMS = 8;
  hipStream_t rstreams[MAX_RESIDENT_STREAMS] = {};
  std::atomic<int> n_rstreams{1};
  std::atomic<uint32_t> next_rstream{0};
  // Kernel timing: a ring of event sets so that launches queue back to back; the host only waits
  // when it laps the ring.  ev[0..1] bracket the glob-resolve kernel, ev[2..3] the decision kernel.
  static constexpr int RING = 32;
  struct Slot { hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}; bool pending = false; bool resolved = false; };
  Slot ring[RING];
  uint64_t next_slot = 0, launches = 0;
  double check_ms_sum = 0, resolve_ms_sum = 0; uint64_t timed = 0;
  std::mutex mu;
  std::mutex pool_mu;
  std::vector<std::pair<void*, size_t>> pool_free;   // idle device blocks of released batches
  // One-shot calls run on their own small set of contexts so that calls from different threads overlap.
  static constexpr int MAX_ONESHOT = 8;
  std::mutex ctx_mu;
  std::condition_variable ctx_cv;
  std::vector<OneShot*> ctx_idle;
  int ctx_count = 0;
  // the device flattener's per-table data (cbh_wire_host.h WireIndexHost), uploaded at load
  u64* w_tix = nullptr; u32* w_scope_of_sid = nullptr; WireCol* w_cols = nullptr; u8* w_col_keys = nullptr;
  u32* w_name_off = nullptr; u8* w_name_bytes = nullptr;
  // A batch of cbh_wire_flatten has a stream to itself while it lives (the call synchronises it several times: on a shared
  // stream every caller would wait for every other caller's work); idle ones are kept, at most MAX_WIRE_STREAMS are made.
  static constexpr int MAX_WIRE_STREAMS = 64;
  std::mutex wstream_mu; std::vector<hipStream_t> wstreams_idle, wstreams_all; int wstreams_made = 0;
  // ... and a page-locked staging block (the call's offsets, defaults and statistics cross PCIe from / to it: a pageable source makes
  // hipMemcpyAsync a blocking, staged copy)
  std::vector<std::pair<void*, size_t>> wpinned_idle;
  // The link's two directions, a stream each.  A stream's copies go to ONE copy engine, whatever their direction: with every slice
  // of a call uploading and downloading on its own stream the link carried one copy at a time (tools/pcie_duplex2.hip: 4 x (12 MB up,
  // 10 MB down) 1.55 ms a stream per slice, 0.94 ms with one upload stream and one download stream - the link is full duplex, the
  // engines are per stream).  The bulk copies of the wire road go here; a batch's own stream waits for / is waited for by events.
  hipStream_t up_stream = nullptr, down_stream = nullptr; bool link_streams_tried = false;
  std::vector<hipEvent_t> wevents_idle;
};

struct cbh_table {
  std::vector<Replica*> reps;
  size_t image_len = 0;
  std::vector<uint32_t> meta;
  std::atomic<int> refs{1};
  const char* bcast = "none";
  WireIndexHost wire;   // cbh_wire_flatten
};

// The layout of a wire batch's page-locked block - the ONE definition: kernels write through these addresses, so two places that
// disagreed about them would be a silent overwrite.  From the front: WireStats slot 0 (statistics going up; the output scan's
// landing place), slot 1 (statistics coming back), the call's tail strings, then at the next multiple of 64 the messages' offsets
// (up) and later, in the same place, the outputs' offsets (back), at the next multiple of 64 behind those the outputs' flags; the
// block's last 64 bytes start with the two route words (routes in use, overflow flag).
struct WirePin {
  size_t tail_bytes = 0, n = 0, cap = 0;   // the call's tail strings, its CheckInputs, the block's capacity
  // what a call asks of a block: the regions above with their alignment slack (`n`: the caller's messages - a call of requests
  // learns the number of its CheckInputs only later, outputs_fit() says whether the block took them too)
  static size_t wanted(size_t tail_bytes, size_t n) { return 2 * sizeof(WireStats) + tail_bytes + 64 + (n + 1) * 8 + n + 64 + 64; }
  size_t slot(int k) const { return (size_t)k * sizeof(WireStats); }
  size_t tail() const { return 2 * sizeof(WireStats); }
  size_t offsets() const { return (tail() + tail_bytes + 63) & ~(size_t)63; }
  size_t out_offsets() const { return offsets(); }
  size_t out_flags() const { return out_offsets() + (((n + 1) * 8 + 63) & ~(size_t)63); }
  size_t routes() const { return cap - 64; }
  bool outputs_fit() const { return out_flags() + n + 64 + 64 <= cap; }
  // The regions do not overlap and the route words are inside the block; `n_up`: the messages whose offsets go up through the
  // block (a call of requests: none).  Asked whenever the layout is fixed or its `n` becomes known.  The asserts are meant to be
  // live in the product build as well (it does not define NDEBUG): a few comparisons per call, against a silent overwrite.
  void check(size_t n_up) const {
    static_assert(sizeof(WireOutStats) <= sizeof(WireStats), "the output scan's statistics land in WireStats slot 0");
    assert(cap >= 128 && slot(1) + sizeof(WireStats) <= tail() && tail() + tail_bytes <= offsets());
    assert(offsets() + (n_up + 1) * 8 <= routes() && routes() + 2 * sizeof(u32) <= cap);
    assert(!outputs_fit() || (out_offsets() + (n + 1) * 8 <= out_flags() && out_flags() + n <= routes()));
  }
};
// what only the wire road's batches (cbh_wire_flatten) carry
struct WireBatch {
  bool own_stream = false;            // the batch's stream is leased from the replica's wire streams, not one of the resident ones
  u32* in_span = nullptr; u32* act_span = nullptr;   // where the response's strings sit in the messages
  void* pinned = nullptr; WirePin pin;               // the page-locked block and its layout
  ptrdiff_t pinned_delta = 0;   // device address of the page-locked block minus its host address (hipHostGetDevicePointer; 0 where both agree)
  hipEvent_t ev[2] = {nullptr, nullptr};   // (the link streams) upload landed / the outputs are written; download landed
  const u32* req_input = nullptr;   // the request words in INPUT order (dev.req_u32 may be the grouped copy)
  const u32* inv = nullptr;         // grouped by route: input -> position of its per-request results; else null
  u64* edr_input = nullptr;         // scratch of cbh_result_download: the derived-role masks back in input order
  const u64* moff = nullptr; u32 dver_off = 0, dver_len = 0;   // (the device assembler reads the messages again)
  bool total_known = false; uint64_t total = 0; uint32_t out_errors = 0;   // cbh_wire_outputs ran its size / scan launches for this batch's current results
  u32* sizes = nullptr; u64* wavesum = nullptr; u64* waveoff = nullptr; WireOutStats* ostats = nullptr; u64* out_off = nullptr; u8* out_flags = nullptr;
};

// What of a batch's requests selects its kernels (plan_for) and places their launches (launch_plan).  Every maker of a resident batch
// works it out for its own source - BatchShape::shape (host arrays), cross_validate (halves), cross_pairs_upload (pairs of a set),
// wf_finish (the flattener's statistics) - and assigns it once.
struct PlanShape {
  u32 max_actions = 0, max_roles = 0;   // largest CBH_RQ_ACT_CNT / ROLE_CNT of the batch
  u32 wide_lo = 0, wide_hi = 0;         // the requests with more than CBH_W2_NA actions or CBH_W2_NR roles lie in [wide_lo, wide_hi)
  bool plain_tags = false;              // BatchShape::plain_tags
};

struct cbh_device_batch {
  cbh_table* table = nullptr;
  Replica* rep = nullptr;
  BatchDev dev{};
  OutDev out{};
  hipStream_t stream = nullptr;   // the replica's resident stream this batch lives on
  KernelArgs* d_args = nullptr;   // device copy of the launch arguments
  KernelArgs last_args;           // what d_args currently holds
  bool have_args = false;
  PlanShape shape;
  std::vector<std::pair<void*, size_t>> allocs;   // (block, capacity) taken from the replica's pool
  bool wire = false;   // a batch the device flattened (cbh_wire_flatten): `w` is in use
  WireBatch w;
  u32 trail_groups = 0; u32* trail_grp = nullptr;   // cbh_batch_set_trail: groups of out.eff_pol, the requests' groups
  // Which form the last cbh_check_resident wrote: packed - out.policy holds the results as packed words (cbh_vm.h cbh_pk_word), the
  // other three arrays are stale until cbh_result_download unpacks them; edr_zero - no derived-role mask was written, every one is 0.
  bool res_packed = false; bool edr_zero = false;
  // The batch has its compact form (cbh_vm.h BatchDev.creq / cval; batch_compact below): the flat kernels' compact instantiations read it.
  bool compact = false;
  u64* allow_bits = nullptr;   // cbh_result_download_allow_bits: the bitmap's device words, allocated at the first call
  u8* dflag = nullptr;         // action-group launches on a table with derived roles (FlatGroupDev.dflag): [n_requests], allocated at the first such check
};

static void replica_destroy(Replica* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  for (int i = 1; i < Replica::MAX_RESIDENT_STREAMS; ++i) if (r->rstreams[i]) { (void)hipStreamSynchronize(r->rstreams[i]); (void)hipStreamDestroy(r->rstreams[i]); }
  if (r->stream) { (void)hipStreamSynchronize(r->stream); (void)hipStreamDestroy(r->stream); }
  for (auto& sl : r->ring) for (auto& e : sl.ev) if (e) (void)hipEventDestroy(e);
  for (hipStream_t ws : r->wstreams_all) { (void)hipStreamSynchronize(ws); (void)hipStreamDestroy(ws); }
  for (auto& pb : r->wpinned_idle) (void)hipHostFree(pb.first);
  for (hipStream_t ls : {r->up_stream, r->down_stream}) if (ls) { (void)hipStreamSynchronize(ls); (void)hipStreamDestroy(ls); }
  for (hipEvent_t e : r->wevents_idle) (void)hipEventDestroy(e);
  if (r->image && r->owns_image) (void)hipFree(r->image);
  for (void* p : {(void*)r->w_tix, (void*)r->w_scope_of_sid, (void*)r->w_cols, (void*)r->w_col_keys, (void*)r->w_name_off, (void*)r->w_name_bytes}) if (p) (void)hipFree(p);
  for (auto& a : r->pool_free) (void)hipFree(a.first);
  for (auto* c : r->ctx_idle) {
    for (auto& s : c->s) if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
    if (c->ev_setup) (void)hipEventDestroy(c->ev_setup);
    for (auto& e : c->ev_piece) if (e) (void)hipEventDestroy(e);
    if (c->h) (void)hipHostFree(c->h);
    if (c->d) (void)hipFree(c->d);
    delete c;
  }
  delete r;
}
static void table_destroy(cbh_table* t) {
  for (Replica* r : t->reps) replica_destroy(r);
  delete t;
}
// every entry point that works on a table holds a reference while it runs: the table outlives a
// concurrent cbh_table_release (the last reference frees it)
struct TableRef {
  cbh_table* t;
  explicit TableRef(cbh_table* t_) : t(t_) { t->refs.fetch_add(1, std::memory_order_relaxed); }
  ~TableRef() { if (t->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) table_destroy(t); }
};
extern "C" void cbh_table_retain(cbh_table* t) { if (t) t->refs.fetch_add(1, std::memory_order_relaxed); }
extern "C" void cbh_table_release(cbh_table* t) {
  if (t && t->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) table_destroy(t);
}

static int replica_finish(Replica* r) {
  HIPCHK(hipSetDevice(r->device));
  HIPCHK(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
  static const int n_streams = std::min(std::max(env_int("CBH_RESIDENT_STREAMS", 4), 1), (int)Replica::MAX_RESIDENT_STREAMS);
  r->n_rstreams = n_streams;   // (default; cbh_table_set_resident_streams changes it for the batches uploaded afterwards)
  r->rstreams[0] = r->stream;
  for (int i = 1; i < Replica::MAX_RESIDENT_STREAMS; ++i) HIPCHK(hipStreamCreateWithFlags(&r->rstreams[i], hipStreamNonBlocking));
  for (auto& sl : r->ring) for (auto& e : sl.ev) HIPCHK(hipEventCreate(&e));
  return 0;
}

// the device flattener's view of the table (cbh_wire.h): built once from the image, a copy on every replica
static int wire_index_install(cbh_table* t, const uint8_t* host_image, size_t len) {
  if (const char* e = cbh_wire_index_build(t->wire, host_image, len, t->meta)) return fail(e);
  const WireIndexHost& w = t->wire;
  for (Replica* r : t->reps) {
    HIPCHK(hipSetDevice(r->device));
    HIPCHK(hipMalloc((void**)&r->w_tix, w.tix.size() * 8)); HIPCHK(hipMemcpy(r->w_tix, w.tix.data(), w.tix.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void**)&r->w_scope_of_sid, w.scope_of_sid.size() * 4)); HIPCHK(hipMemcpy(r->w_scope_of_sid, w.scope_of_sid.data(), w.scope_of_sid.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void**)&r->w_cols, w.cols.size() * sizeof(WireCol))); HIPCHK(hipMemcpy(r->w_cols, w.cols.data(), w.cols.size() * sizeof(WireCol), hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void**)&r->w_col_keys, w.col_keys.size())); HIPCHK(hipMemcpy(r->w_col_keys, w.col_keys.data(), w.col_keys.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void**)&r->w_name_off, w.name_off.size() * 4)); HIPCHK(hipMemcpy(r->w_name_off, w.name_off.data(), w.name_off.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void**)&r->w_name_bytes, w.name_bytes.size())); HIPCHK(hipMemcpy(r->w_name_bytes, w.name_bytes.data(), w.name_bytes.size(), hipMemcpyHostToDevice));
  }
  return 0;
}

static bool rccl_bind(Rccl& r, const std::vector<int>& devs) {   // under g_eng.mu
  if (r.tried) return r.ok;
  r.tried = true;
  if (env_eq("CBH_BCAST", "peer")) return false;
  for (size_t i = 0; i < devs.size(); ++i) for (size_t j = i + 1; j < devs.size(); ++j) if (devs[i] == devs[j]) return false;   // one rank per GPU
  r.lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!r.lib) r.lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
  if (!r.lib) return false;
  r.CommInitAll = (decltype(r.CommInitAll))dlsym(r.lib, "ncclCommInitAll");
  r.CommDestroy = (decltype(r.CommDestroy))dlsym(r.lib, "ncclCommDestroy");
  r.GroupStart = (decltype(r.GroupStart))dlsym(r.lib, "ncclGroupStart");
  r.GroupEnd = (decltype(r.GroupEnd))dlsym(r.lib, "ncclGroupEnd");
  r.Broadcast = (decltype(r.Broadcast))dlsym(r.lib, "ncclBroadcast");
  if (!r.CommInitAll || !r.CommDestroy || !r.GroupStart || !r.GroupEnd || !r.Broadcast) return false;
  r.comms.assign(devs.size(), nullptr);
  if (r.CommInitAll(r.comms.data(), (int)devs.size(), devs.data()) != 0) { r.comms.clear(); return false; }
  r.ok = true;
  return true;
}

// the image sits on reps[0]; put a copy on every other replica
static int broadcast_image(cbh_table* t) {
  const size_t len = t->image_len;
  for (size_t i = 1; i < t->reps.size(); ++i) {
    HIPCHK(hipSetDevice(t->reps[i]->device));
    HIPCHK(hipMalloc(&t->reps[i]->image, len));
  }
  bool done = false;
  {
    std::lock_guard<std::mutex> lk(g_eng.mu);
    Rccl& r = g_eng.rccl;
    if (rccl_bind(r, g_eng.devices) && r.comms.size() == t->reps.size()) {
      // one-time RCCL broadcast over xGMI from the first device (ncclUint8 = 1)
      bool ok = r.GroupStart() == 0;
      for (size_t i = 0; ok && i < t->reps.size(); ++i) {
        ok = hipSetDevice(t->reps[i]->device) == hipSuccess &&
             r.Broadcast(t->reps[0]->image, t->reps[i]->image, len, 1, 0, r.comms[i], t->reps[i]->stream) == 0;
      }
      ok = (r.GroupEnd() == 0) && ok;
      for (size_t i = 0; i < t->reps.size(); ++i) { (void)hipSetDevice(t->reps[i]->device); ok = (hipStreamSynchronize(t->reps[i]->stream) == hipSuccess) && ok; }
      if (ok) { done = true; t->bcast = "rccl"; } else (void)hipGetLastError();
    }
  }
  if (!done) {
    for (size_t i = 1; i < t->reps.size(); ++i)
      HIPCHK(hipMemcpyPeer(t->reps[i]->image, t->reps[i]->device, t->reps[0]->image, t->reps[0]->device, len));
    t->bcast = "peer-copy";
  }
  return 0;
}

extern "C" int cbh_table_load(const void* blob, size_t len, cbh_table** out) {
  std::vector<int> devs;
  { std::lock_guard<std::mutex> lk(g_eng.mu); if (!g_eng.inited) return fail("cbh_init has not been called"); devs = g_eng.devices; }
  if (!blob || !out) return fail("null argument");
  cbh_table* t = new (std::nothrow) cbh_table();
  if (!t) return fail("out of memory");
  t->image_len = len;
  auto bail = [&]() { table_destroy(t); return -1; };
  for (int d : devs) { Replica* r = new (std::nothrow) Replica(); if (!r) { fail("out of memory"); return bail(); } r->device = d; t->reps.push_back(r); }
  for (Replica* r : t->reps) if (replica_finish(r) != 0) return bail();
  Replica* r0 = t->reps[0];
  if (hipSetDevice(r0->device) != hipSuccess || hipMalloc(&r0->image, len) != hipSuccess) { fail("hipMalloc(table image) failed"); return bail(); }
  if (hipMemcpy(r0->image, blob, len, hipMemcpyHostToDevice) != hipSuccess) { fail("hipMemcpy(table image) failed"); return bail(); }
  if (t->reps.size() > 1 && broadcast_image(t) != 0) return bail();
  for (Replica* r : t->reps) {
    const char* e = cbh_parse_image(r->dev, t->meta, static_cast<const uint8_t*>(r->image), static_cast<const uint8_t*>(blob), len);
    if (e) { fail(e); return bail(); }
  }
  if (wire_index_install(t, static_cast<const uint8_t*>(blob), len) != 0) return bail();
  *out = t;
  return 0;
}

extern "C" int cbh_table_adopt_device_image(void* device_image, size_t len, cbh_table** out) {
  int dev0;
  { std::lock_guard<std::mutex> lk(g_eng.mu); if (!g_eng.inited) return fail("cbh_init has not been called"); dev0 = g_eng.devices[0]; }
  if (!device_image || !out) return fail("null argument");
  HIPCHK(hipSetDevice(dev0));
  std::vector<uint8_t> host(len);
  HIPCHK(hipMemcpy(host.data(), device_image, len, hipMemcpyDeviceToHost));
  cbh_table* t = new (std::nothrow) cbh_table();
  if (!t) return fail("out of memory");
  Replica* r = new (std::nothrow) Replica();
  if (!r) { delete t; return fail("out of memory"); }
  r->device = dev0; r->image = device_image; r->owns_image = false;
  t->reps.push_back(r); t->image_len = len;
  const char* e = cbh_parse_image(r->dev, t->meta, static_cast<const uint8_t*>(r->image), host.data(), len);
  if (e) { table_destroy(t); return fail(e); }
  if (replica_finish(r) != 0) { table_destroy(t); return -1; }
  if (wire_index_install(t, host.data(), len) != 0) { table_destroy(t); return -1; }
  *out = t;
  return 0;
}

extern "C" const char* cbh_table_broadcast_kind(const cbh_table* t) { return t ? t->bcast : "none"; }
extern "C" uint32_t cbh_table_num_strings(const cbh_table* t) { return t ? t->meta[CBH_M_NSTRINGS] : 0; }
extern "C" uint32_t cbh_table_num_columns(const cbh_table* t) { return t ? t->meta[CBH_M_NCOLUMNS] : 0; }
extern "C" uint64_t cbh_table_device_bytes(const cbh_table* t) { return t ? t->image_len : 0; }
extern "C" void* cbh_table_device_ptr(const cbh_table* t) { return t ? t->reps[0]->image : nullptr; }


// ---- resident path ----------------------------------------------------------------------------------------
// Device buffers of batches come from a per-replica pool of power-of-two blocks: a small synchronous
// CheckResources round trip must not pay ~17 hipMalloc / hipFree pairs (each hipFree also
// synchronises the device).  Blocks go back to the pool on cbh_batch_release and to the driver when the
// table goes.
static int pool_alloc(cbh_device_batch* b, size_t bytes, void** out) {
  size_t cap = 256;
  while (cap < bytes) cap <<= 1;
  Replica* r = b->rep;
  {
    std::lock_guard<std::mutex> lk(r->pool_mu);
    for (size_t i = 0; i < r->pool_free.size(); ++i)
      if (r->pool_free[i].second == cap) {
        *out = r->pool_free[i].first;
        r->pool_free[i] = r->pool_free.back(); r->pool_free.pop_back();
        b->allocs.push_back({*out, cap});
        return 0;
      }
  }
  HIPCHK(hipMalloc(out, cap));
  b->allocs.push_back({*out, cap});
  return 0;
}

extern "C" void cbh_batch_release(cbh_device_batch* b) {
  if (!b) return;
  cbh_table* t = b->table;
  (void)hipSetDevice(b->rep->device); (void)hipStreamSynchronize(b->stream ? b->stream : b->rep->stream);
  // a copy of this batch's outputs may still run on the replica's SHARED download stream (cbh_wire_outputs left early on an
  // error between the copy's enqueue and its wait): its block must not go back to the pool - and its event not to another
  // batch - before the copy has landed.  The event was recorded behind the copy; an event never recorded is complete.
  if (b->w.ev[1]) { if (hipEventSynchronize(b->w.ev[1]) != hipSuccess) (void)hipGetLastError(); }
  {
    std::lock_guard<std::mutex> lk(b->rep->pool_mu);
    for (auto& a : b->allocs) b->rep->pool_free.push_back(a);
  }
  if (b->w.own_stream || b->w.pinned || b->w.ev[0] || b->w.ev[1]) {
    std::lock_guard<std::mutex> lk(b->rep->wstream_mu);
    if (b->w.own_stream) b->rep->wstreams_idle.push_back(b->stream);
    if (b->w.pinned) b->rep->wpinned_idle.push_back({b->w.pinned, b->w.pin.cap});
    for (hipEvent_t e : b->w.ev) if (e) b->rep->wevents_idle.push_back(e);
  }
  delete b;
  cbh_table_release(t);   // the reference the batch held
}

template <typename T>
static int up(cbh_device_batch* b, const T*& dst, const T* src, size_t n, hipStream_t s) {
  dst = nullptr;
  size_t bytes = (n ? n : 1) * sizeof(T);
  void* p = nullptr;
  if (pool_alloc(b, bytes, &p) != 0) return -1;
  if (n) HIPCHK(hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, s));
  dst = static_cast<const T*>(p);
  return 0;
}
template <typename T>
static int dalloc(cbh_device_batch* b, T*& dst, size_t n) {
  void* p = nullptr;
  if (pool_alloc(b, (n ? n : 1) * sizeof(T), &p) != 0) return -1;
  dst = static_cast<T*>(p);
  return 0;
}

#include "cbh_host_resident.h"   // batches that stay on the device: upload, plan, launch, download, trail
#include "cbh_host_cross.h"      // N x M x A from N + M halves: the materialised product, the direct set, its pairs
#include "cbh_host_wire.h"       // serialized messages in, serialized answers out: the device flattener and assembler
#include "cbh_host_oneshot.h"    // cbh_check_batch / cbh_trace_batch: a host batch, one round trip
#endif  // !__HIP_DEVICE_COMPILE__
