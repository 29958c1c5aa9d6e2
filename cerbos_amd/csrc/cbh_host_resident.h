// Host side of libcerbos_hip.so, part 2 of 5 (included by cbh_engine.hip, host pass only): resident batches - validation, the
// maker from host arrays and what every maker shares (the cross road's are in cbh_host_cross.h, the wire road's in cbh_host_wire.h),
// the choice of kernels and their launches, the downloads, the audit trail.
#pragma once

// Would cbh_plan decide a batch of this shape in action groups (flags permitting)?  Then the tags select its kernel, as for four actions.
static bool flat_groups_shape(const cbh_table* t, u32 max_actions, u32 max_roles) {
  return flat_action_groups_on() && !t->reps.empty() && cbh_flat_action_groups(t->reps[0]->dev.n_dr, max_actions, max_roles) != 0;
}
// ---- plain tags: do the attribute columns hold plain scalars only - no int / uint (cross-type numerics) and no list / map (deep
// equality)?  Then no classified leaf can need the shared evaluator and the flat kernel without that call decides the batch
// (cbh_check_flat.h).  The answer costs a pass over tag bytes, so it is asked only where it can select a kernel, for the counts the
// plan is made for - a batch's largest ones; for a direct set (cbh_host_cross.h) min(A, 4) and, with role groups, min(max_roles, 4):
//   CBH_MF_FLAT   max_roles <= 4 and (max_actions <= 4 or flat_groups_shape)   yes: a flat kernel decides the batch, at once or in action groups
//   CBH_MF_WALK2  GSLOTS_ALL > GSLOTS_GENERIC, whatever the shape              yes: the answer sizes the walk's evaluation sites
//   neither line holds (a flat table's other shapes among them)                no: the walk's or the general kernels, no site that depends on it
static bool plain_tags_select(const cbh_table* t, u32 max_actions, u32 max_roles) {
  const u32 mf = t->meta[CBH_M_FLAGS];
  return ((mf & CBH_MF_FLAT) && max_roles <= 4 && (max_actions <= 4 || flat_groups_shape(t, max_actions, max_roles))) ||
         ((mf & CBH_MF_WALK2) && t->meta[CBH_M_GSLOTS_ALL] > t->meta[CBH_M_GSLOTS_GENERIC]);
}
// tags 2, 3 (int, uint) and 6, 7 (list, map) are exactly the bytes x with (x & 0xFA) == 0x02: eight at a time
static bool has_int_or_container_tag(const uint8_t* p, size_t n) {
  size_t i = 0; uint64_t hit = 0;
  for (; i + 8 <= n; i += 8) {
    uint64_t w; std::memcpy(&w, p + i, 8);
    const uint64_t z = (w & 0xFAFAFAFAFAFAFAFAull) ^ 0x0202020202020202ull;              // a zero byte where a tag matched
    hit |= (z - 0x0101010101010101ull) & ~z & 0x8080808080808080ull;
  }
  for (; i < n; ++i) hit |= (uint64_t)((p[i] & 0xFAu) == 0x02u);
  return hit != 0;
}
// The scan: does a column that can send a classified leaf to the evaluator (CBH_M_SENS_COLS, bit c) hold such a tag in a row that
// counts?  `tags`: [n_columns][n_rows]; `rows(c)`: which rows of column c some request of the batch reads -
//   a host batch: the whole column;
//   halves, N principals then M resources: rows [0, N) of a principal-side column, rows [N, N + M) of a resource-side one - what a column's other rows hold is in no request of the product.
struct TagRows { size_t first, count; };
template <typename Rows>
static bool sens_tag_hit(const cbh_table* t, const uint8_t* tags, u32 n_columns, size_t n_rows, Rows rows) {
  for (u32 c = 0; c < 32 && c < n_columns; ++c) if ((t->meta[CBH_M_SENS_COLS] >> c) & 1u) {
    const TagRows r = rows(c);
    if (has_int_or_container_tag(tags + (size_t)c * n_rows + r.first, r.count)) return true;
  }
  return false;
}

// ---- batch validation (O(n_requests), both entry points) ---------------------------------------------------
// Offsets and counts the kernels index device memory with must lie inside the arrays they index.  String ids
// need no host pass: the kernels only compare them, or bound them before using one as an index.
struct BatchShape {
  u32 max_actions = 0, max_roles = 0; bool ascending = true;
  u32 wide_lo = 0, wide_hi = 0;   // the requests with more than CBH_W2_NA actions or CBH_W2_NR roles lie in [wide_lo, wide_hi)
  // plain tags (above): one pass over the tag bytes, made only where the answer selects a kernel and only when the first
  // launch is being prepared - by then the uploads are enqueued and the pass runs beside them.
  const uint8_t* tags = nullptr;             // [n_columns][n_req]; nullptr: the answer cannot matter (plain_tags_select)
  const cbh_table* table = nullptr; uint32_t n_columns = 0; size_t n_req = 0;
  mutable std::atomic<int> plain{-1};        // -1 not looked at yet (racing threads compute the same answer)
  bool plain_tags() const {
    int v = plain.load(std::memory_order_relaxed);
    if (v < 0) {
      const bool hit = tags && sens_tag_hit(table, tags, n_columns, n_req, [&](u32) { return TagRows{0, n_req}; });
      v = (!flat_any_forced() && !hit) ? 1 : 0;
      plain.store(v, std::memory_order_relaxed);
    }
    return v == 1;
  }
  PlanShape shape() const { return PlanShape{max_actions, max_roles, wide_lo, wide_hi, plain_tags()}; }   // (the late part: beside the uploads)
};
// the O(1) part of validate_batch: the arrays a batch of these counts needs are there
static int validate_header(const cbh_table* t, const cbh_batch* in) {
  if (in->n_columns != t->meta[CBH_M_NCOLUMNS]) return fail("cbh_batch.n_columns does not match the table's column schema");
  const size_t NR = in->n_requests;
  if (NR && !in->req_u32) return fail("cbh_batch: a required array is NULL");
  if (in->n_tuples && !in->tuple_action) return fail("cbh_batch: a required array is NULL");
  if (in->n_roles && !in->roles) return fail("cbh_batch: a required array is NULL");
  if (NR && in->n_columns && (!in->col_tag || !in->col_val)) return fail("cbh_batch: a required array is NULL");
  if (in->heap_len && (!in->heap_tag || !in->heap_val)) return fail("cbh_batch: a required array is NULL");
  if (in->n_strings && (!in->str_off || !in->str_flags)) return fail("cbh_batch: a required array is NULL");
  if (in->str_bytes_len && !in->str_bytes) return fail("cbh_batch: a required array is NULL");
  return 0;
}
static int validate_batch(const cbh_table* t, const cbh_batch* in, BatchShape& sh) {
  if (validate_header(t, in) != 0) return -1;
  const size_t NR = in->n_requests;
  const u32* role_off = in->req_u32 + (size_t)CBH_RQ_ROLE_OFF * NR; const u32* role_cnt = in->req_u32 + (size_t)CBH_RQ_ROLE_CNT * NR;
  const u32* act_off = in->req_u32 + (size_t)CBH_RQ_ACT_OFF * NR; const u32* act_cnt = in->req_u32 + (size_t)CBH_RQ_ACT_CNT * NR;
  // (three passes without loop-carried dependences other than max / or reductions: the compiler vectorises them - this scan
  // sits on the path of every one-shot call, 250 000 requests at the headline size)
  u32 maxa = 0, maxr = 0; u32 bad = 0;
  const u64 n_roles = in->n_roles, n_tuples = in->n_tuples;
  for (size_t r = 0; r < NR; ++r) {
    maxa = act_cnt[r] > maxa ? act_cnt[r] : maxa;
    maxr = role_cnt[r] > maxr ? role_cnt[r] : maxr;
    bad |= (u32)((u64)role_off[r] + role_cnt[r] > n_roles) | (u32)((u64)act_off[r] + act_cnt[r] > n_tuples);
  }
  u32 unordered = 0;
  for (size_t r = 1; r < NR; ++r) unordered |= (u32)((u64)act_off[r] < (u64)act_off[r - 1] + act_cnt[r - 1]);
  u32 wlo = 0xFFFFFFFFu, whi = 0;
  if (maxa > CBH_W2_NA || maxr > CBH_W2_NR)   // where the requests wider than the walk's base shape lie (rare: found in a pass of its own)
    for (size_t r = 0; r < NR; ++r)
      if (act_cnt[r] > CBH_W2_NA || role_cnt[r] > CBH_W2_NR) { if (wlo == 0xFFFFFFFFu) wlo = (u32)r; whi = (u32)r + 1; }
  if (maxa > CBH_MAX_ACTIONS_PER_REQUEST) return fail("cbh_batch: a request carries more than CBH_MAX_ACTIONS_PER_REQUEST actions");
  if (bad) return fail("cbh_batch: a request's role or action slice lies outside the batch");
  if (in->n_strings && in->str_off[in->n_strings] > in->str_bytes_len) return fail("cbh_batch: string offsets exceed str_bytes_len");
  sh.max_actions = maxa; sh.max_roles = maxr; sh.ascending = !unordered;
  sh.wide_lo = whi ? wlo : 0; sh.wide_hi = whi;
  sh.table = t; sh.tags = plain_tags_select(t, maxa, maxr) ? in->col_tag : nullptr; sh.n_columns = in->n_columns; sh.n_req = NR;
  sh.plain.store(-1, std::memory_order_relaxed);
  return 0;
}

// The compact form of a batch the flat kernels can decide (cbh_vm.h BatchDev.creq / cval), derived on the batch's stream from the wide
// arrays already enqueued: the scan's verdict crosses to the host (one word), then the records, the 32-bit planes and the tag planes are written.  A
// batch with a field that does not fit the record keeps the wide form; so does every batch under CBH_COMPACT_INPUTS=0 (measurement aid).
static bool compact_inputs_on() { static const bool on = env_int("CBH_COMPACT_INPUTS", 1) != 0; return on; }
static int batch_compact(cbh_device_batch* b, hipStream_t s) {
  const TableDev& dev = b->rep->dev;
  BatchDev& d = b->dev;
  if (!compact_inputs_on() || !(dev.flags & CBH_MF_FLAT) || b->shape.max_actions > 4 || b->shape.max_roles > 4 || !d.n_requests) return 0;
  CompactArgs ca{};
  ca.req_u32 = d.req_u32; ca.roles = d.roles; ca.tuple_action = d.tuple_action; ca.col_val = d.col_val; ca.col_tag = d.col_tag;
  ca.action_class = dev.action_class; ca.role_class = dev.role_class; ca.K = dev.K;
  ca.scope_parent = dev.scope_parent; ca.scope_flags = dev.scope_flags; ca.n_scopes = dev.n_scopes;
  ca.n_requests = d.n_requests; ca.n_cached = d.n_columns < CBH_CACHE_COLS ? d.n_columns : CBH_CACHE_COLS;
  if (dalloc(b, ca.info, 1) != 0) return -1;
  const dim3 grid((d.n_requests + 255u) / 256u);
  u32 info = 0;
  HIPCHK(hipMemsetAsync(ca.info, 0, 4, s));
  hipLaunchKernelGGL(cbh_compact_scan_kernel, grid, dim3(256), 0, s, ca);
  HIPCHK(hipMemcpyAsync(&info, ca.info, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (info & CBH_CI_MISFIT) return 0;
  ca.narrow = ~info & ((1u << ca.n_cached) - 1u) & CBH_CI_NARROW_MASK;
  if (dalloc(b, ca.creq, (size_t)4 * d.n_requests) != 0 || dalloc(b, ca.cval, (size_t)__builtin_popcount(ca.narrow) * d.n_requests) != 0 ||
      dalloc(b, ca.ctag, (size_t)((ca.n_cached + 3u) / 4u) * d.n_requests) != 0) return -1;
  hipLaunchKernelGGL(cbh_compact_pack_kernel, grid, dim3(256), 0, s, ca);
  HIPCHK(hipGetLastError());
  d.creq = ca.creq; d.cval = ca.cval; d.ctag = ca.ctag; d.compact_info = ca.narrow | ((info & CBH_CI_ACT4) ? 0u : CBH_CI_ACT4);
  b->compact = true;
  return 0;
}

// what a resident batch owns beside its inputs: glob bits, evaluation-site results, the result arrays, the launch arguments
// (b->dev's counts and b->shape are set).  gbits_words: three per batch-local string - or, for a wire batch of a table without
// automata, whose dictionary has many slots and nobody to read their bits, one
static int batch_device_buffers(cbh_device_batch* b, size_t gbits_words) {
  BatchDev& d = b->dev; const Replica* rep = b->rep;
  int rc = dalloc(b, d.gbits, gbits_words);
  d.n_gwords = (rep->dev.flags & CBH_MF_WALK2) ? w2_gwords(rep->dev.gslots_generic, rep->dev.gslots_all, b->shape.plain_tags) : 0;
  d.n_gslots = 0;   // per launch (launch_plan)
  if (d.n_gwords) rc |= dalloc(b, d.gres, (size_t)d.n_gwords * d.n_requests); else d.gres = nullptr;
  rc |= dalloc(b, b->out.effect, d.n_tuples);
  rc |= dalloc(b, b->out.policy, d.n_tuples);
  rc |= dalloc(b, b->out.scope, d.n_tuples);
  rc |= dalloc(b, b->out.status, d.n_tuples);
  rc |= dalloc(b, b->out.edr, d.n_requests);
  rc |= dalloc(b, b->d_args, 1);
  return rc;
}

// A new resident batch of table `t` on `rep` (the caller has made the replica's device current): it holds a reference to the table
// and has its stream - one of the replica's resident streams, dealt round-robin; the wire road asks for an idle wire stream of
// its own first.  nullptr: out of memory.
static cbh_device_batch* batch_new(cbh_table* t, Replica* rep, bool own_wire_stream_wanted) {
  cbh_device_batch* b = new (std::nothrow) cbh_device_batch();
  if (!b) { fail("out of memory"); return nullptr; }
  cbh_table_retain(t);
  b->table = t; b->rep = rep;
  if (own_wire_stream_wanted) {
    std::lock_guard<std::mutex> lk(rep->wstream_mu);
    if (!rep->wstreams_idle.empty()) { b->stream = rep->wstreams_idle.back(); rep->wstreams_idle.pop_back(); b->w.own_stream = true; }
    else if (rep->wstreams_made < Replica::MAX_WIRE_STREAMS && hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) == hipSuccess) { ++rep->wstreams_made; rep->wstreams_all.push_back(b->stream); b->w.own_stream = true; }
  }
  if (!b->w.own_stream) b->stream = rep->rstreams[rep->next_rstream.fetch_add(1, std::memory_order_relaxed) % (uint32_t)rep->n_rstreams.load(std::memory_order_relaxed)];
  return b;
}
static void batch_set_counts(cbh_device_batch* b, u32 n_requests, u32 n_tuples, u32 n_roles, u32 n_columns, u32 n_strings, u32 heap_len) {
  BatchDev& d = b->dev;
  d.n_requests = n_requests; d.n_tuples = n_tuples; d.n_roles = n_roles; d.n_columns = n_columns; d.n_strings = n_strings; d.heap_len = heap_len;
  d.req_lo = 0; d.req_hi = n_requests;
}

// ---- what the makers of a resident batch share (batch_upload below; cross_upload, cross_pairs_upload: cbh_host_cross.h) ----
// A batch that is still being made, made with cbh_batch_release as its deleter: released on every way out but the last, where batch_finish hands it out.
typedef std::unique_ptr<cbh_device_batch, void (*)(cbh_device_batch*)> BatchOwner;
// The six arrays a batch takes from its source as they are (`from`: a cbh_batch, or the BatchDev of a set's halves - `str_bytes_len`
// is a count only the former keeps).  `copy(dst, src, n)`: up - from host memory - or dcopy, device to device.
template <typename Source, typename Copy>
static int batch_shared_arrays(BatchDev& d, const Source& from, size_t str_bytes_len, Copy copy) {
  int rc = 0;
  rc |= copy(d.roles, from.roles, from.n_roles);
  rc |= copy(d.heap_tag, from.heap_tag, from.heap_len);
  rc |= copy(d.heap_val, from.heap_val, from.heap_len);
  rc |= copy(d.str_off, from.str_off, from.n_strings ? (size_t)from.n_strings + 1 : 0);
  rc |= copy(d.str_bytes, from.str_bytes, str_bytes_len);
  rc |= copy(d.str_flags, from.str_flags, from.n_strings);
  d.tuple_req = nullptr;   // informational on the host side; no kernel reads it
  return rc;
}
// The end of a maker.  `rc`: what its uploads and allocations returned so far (each has left its text); `launches`: what the maker
// enqueues behind the cleared glob bits - its own kernels, then batch_compact where the batch may take the compact form.  The wait
// is the last step: pageable host memory a maker copied from (the caller's arrays, a vector of the maker's frame) may go after it.
template <typename Launches>
static int batch_finish(BatchOwner& b, int rc, cbh_device_batch** out, Launches launches) {
  BatchDev& d = b->dev; hipStream_t s = b->stream;
  rc |= batch_device_buffers(b.get(), (size_t)3 * d.n_strings);
  if (rc != 0) return -1;
  // glob bits of the batch-local strings: all zero unless the table has automata to run (then
  // cbh_check_resident overwrites every word on each launch)
  if (d.n_strings && hipMemsetAsync(d.gbits, 0, (size_t)3 * d.n_strings * sizeof(u64), s) != hipSuccess) return fail("upload failed");
  if (launches() != 0) return -1;
  if (hipStreamSynchronize(s) != hipSuccess) return fail("upload failed");
  *out = b.release();
  return 0;
}

static int batch_upload(cbh_table* t, uint32_t device_index, const cbh_batch* in, cbh_device_batch** out, bool compact) {
  if (!t || !in || !out) return fail("null argument");
  if (device_index >= t->reps.size()) return fail("device index out of range");
  BatchShape sh;
  if (validate_batch(t, in, sh) != 0) return -1;
  Replica* rep = t->reps[device_index];
  HIPCHK(hipSetDevice(rep->device));
  BatchOwner b(batch_new(t, rep, false), cbh_batch_release);
  if (!b) return -1;
  b->shape = sh.shape();
  BatchDev& d = b->dev;
  batch_set_counts(b.get(), in->n_requests, in->n_tuples, in->n_roles, in->n_columns, in->n_strings, in->heap_len);
  hipStream_t s = b->stream;
  const size_t NR = in->n_requests;
  int rc = up(b.get(), d.req_u32, in->req_u32, (size_t)CBH_RQ_NFIELDS * NR, s);
  rc |= up(b.get(), d.tuple_action, in->tuple_action, in->n_tuples, s);
  rc |= up(b.get(), d.col_tag, in->col_tag, (size_t)in->n_columns * NR, s);
  rc |= up(b.get(), d.col_val, in->col_val, (size_t)in->n_columns * NR, s);
  rc |= batch_shared_arrays(d, *in, in->str_bytes_len, [&](auto& dst, auto* src, size_t n) { return up(b.get(), dst, src, n, s); });
  return batch_finish(b, rc, out, [&] { return compact ? batch_compact(b.get(), s) : 0; });
}
extern "C" int cbh_batch_upload_on(cbh_table* t, uint32_t device_index, const cbh_batch* in, cbh_device_batch** out) { return batch_upload(t, device_index, in, out, true); }
extern "C" int cbh_batch_upload(cbh_table* t, const cbh_batch* in, cbh_device_batch** out) { return cbh_batch_upload_on(t, 0, in, out); }

static void collect_slot(Replica* r, Replica::Slot& sl) {   // the slot's last event has completed
  if (!sl.pending) return;
  float a = 0, c = 0;
  if (sl.resolved && hipEventElapsedTime(&a, sl.ev[0], sl.ev[1]) != hipSuccess) a = 0;
  if (hipEventElapsedTime(&c, sl.ev[2], sl.ev[3]) == hipSuccess) {
    r->resolve_ms_sum += a; r->check_ms_sum += c; r->timed += 1;
  }
  sl.pending = false;
}
static void collect_times(Replica* r) {   // after the stream has been synchronised
  for (auto& sl : r->ring) collect_slot(r, sl);
}

// CBH_NO_FLAT=1 / CBH_NO_WALK2=1 / CBH_NO_WALK2_WIDE=1 (measurement aids): leave the flat kernels / cbh_walk2_kernel out of the choice
// `action_groups` = false: the plan as it is without the flat kernels' action groups (what CBH_FLAT_ACTION_GROUPS=0 gives everywhere)
static CbhPlan plan_for(const TableDev& dev, u32 max_actions, u32 max_roles, bool plain_tags, u32 eval_flags, bool action_groups = true) {
  static const bool no_flat = env_set("CBH_NO_FLAT"), no_walk2 = env_set("CBH_NO_WALK2");
  static const bool no_walk2_wide = env_set("CBH_NO_WALK2_WIDE");   // (measurement aid: requests with five to eight roles on the general walk, as before the wider shape)
  const bool has_globs = (dev.nfa_words[0] | dev.nfa_words[1] | dev.nfa_words[2]) != 0 || (dev.flags & CBH_MF_HAS_ANY_PATTERN);
  static const bool force_staged = env_set("CBH_FORCE_STAGED");   // (tests: the staged record walk on tables of any size)
  return cbh_plan(dev.flags, dev.n_dr, has_globs, dev.gslots_generic, dev.gslots_all, max_actions, max_roles, plain_tags, eval_flags, no_flat, no_walk2,
                  force_staged ? 0xFFFFFFFFu : dev.max_bucket, no_walk2_wide, cbh_flat_use_masks(dev.segs, dev.max_bucket), action_groups && flat_action_groups_on());
}
static CbhPlan plan_for(const TableDev& dev, const PlanShape& sh, u32 eval_flags) { return plan_for(dev, sh.max_actions, sh.max_roles, sh.plain_tags, eval_flags); }   // (a batch's own plan)
// (on by default since round 5: C5 11.8 -> 12.4 G decisions/s, C5W 7.61 -> 7.67, profiles/r05_presplit_ab.txt; CBH_PRE_SPLIT=0: the fused pre-pass)
static bool pre_split_on() { static const bool on = env_int("CBH_PRE_SPLIT", 1) != 0; return on; }
// Does the packed form of the column cache's tags (cbh_vm.h CBH_CC_DWORDS) let a CU hold more workgroups of `fn` than the wide one?
// The runtime's occupancy figure for the kernel at either LDS size, kept per (kernel, size).  CBH_PACKED_TAGS=0/1 (tests,
// measurement): never / always.
static bool packed_tags_pay(cbh_check_kernel_fn fn, u32 threads, size_t lds_wide, size_t lds_packed) {
  static const int forced = env_int("CBH_PACKED_TAGS", -1);
  if (forced >= 0) return forced != 0;
  if (lds_packed >= lds_wide) return false;
  static std::mutex mu;
  static std::map<std::tuple<const void*, u32, size_t>, int> memo;
  auto blocks = [&](size_t lds) {
    const auto key = std::make_tuple((const void*)fn, threads, lds);
    std::lock_guard<std::mutex> g(mu);
    auto it = memo.find(key);
    if (it != memo.end()) return it->second;
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)fn, (int)threads, lds) != hipSuccess) { (void)hipGetLastError(); n = 0; }
    memo.emplace(key, n);
    return n;
  };
  return blocks(lds_packed) > blocks(lds_wide);
}
// the launches that decide the requests [lo, hi) of `ka.b`; [wide_lo, wide_hi) = where the batch's requests wider than
// cbh_walk2_kernel's shape lie (empty: none)
static void launch_plan(const CbhPlan& pl, const TableDev& dev, KernelArgs ka, const KernelArgs* d_args, u32 lo, u32 hi, u32 wide_lo, u32 wide_hi,
                        size_t pad, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr, u8* dflag = nullptr) {
  if (hi <= lo) return;
  ka.b.req_lo = lo; ka.b.req_hi = hi;
  ka.flags &= ~(u32)(CBH_FI_MASK & ~(CBH_FI_PACKED_RES | CBH_FI_COMPACT));   // (the result form and the input form are the caller's choice: cbh_check_resident)
  const u32 n = hi - lo;
  // (timed launches: the start event rides on the first kernel of the plan, the stop event on the last - the figure is the
  // whole plan's, gaps between its kernels included)
  // `lds_of(packed)`: the launch's dynamic LDS with the column cache's tags in either form (cbh_vm.h CBH_CC_DWORDS); the packed form
  // where it lets a CU hold more workgroups of this kernel
  auto go = [&](cbh_check_kernel_fn fn, u32 grid, u32 threads, auto lds_of, const KernelArgs& a0, bool last) {
    const size_t wide = lds_of(false), packed = lds_of(true);
    const bool use_packed = cbh_is_flat_compact_kernel(fn) || packed_tags_pay(fn, threads, wide, packed);   // (a compact instantiation has no other form)
    const size_t lds = use_packed ? packed : wide;
    KernelArgs a = a0;
    if (use_packed) a.flags |= CBH_FI_PACKED_TAGS;
    if (ev0 || (ev1 && last)) { hipExtLaunchKernelGGL(fn, dim3(grid), dim3(threads), lds, s, ev0, last ? ev1 : nullptr, 0, a, d_args); ev0 = nullptr; }
    else hipLaunchKernelGGL(fn, dim3(grid), dim3(threads), lds, s, a, d_args);
  };
  auto plan_lds = [&](bool pre, u32 na, size_t extra) {
    return [=, &pl, &dev, &ka](bool packed) { return cbh_plan_lds(pl, dev.flags, dev.max_depth, dev.n_scopes, dev.K, ka.b.n_columns, dev.inline_cols, dev.n_dr, pre, na, packed) + extra; };
  };
  if (pl.kind == 2) {
    const u32 wlo = std::max(lo, wide_lo), whi = std::min(hi, wide_hi);   // where the requests wider than the base shape lie
    if (pl.wide_kernel) {   // the few requests wider than the walk's shapes: the general walk, on the lanes the walks below leave alone
      KernelArgs kw = ka;
      kw.b.req_lo = wlo; kw.b.req_hi = whi;
      kw.flags |= (pl.walk_wide || pl.walk_awide) ? CBH_FI_ONLY_WIDER : CBH_FI_ONLY_WIDE;
      if (whi > wlo) go(pl.wide_kernel, (whi - wlo + CBH_BLOCK - 1) / CBH_BLOCK, CBH_BLOCK, [&](bool packed) { return cbh_general_lds(dev.flags, ka.b.n_columns, packed); }, kw, false);
    }
    if (pl.wide_kernel || pl.walk_wide || pl.walk_awide) ka.flags |= CBH_FI_SKIP_WIDE;
    ka.b.n_gwords = ka.b.gres ? pl.n_gwords : 0; ka.b.n_gslots = ka.b.gres ? pl.n_gslots : 0;
    // the requests with five to eight roles / nine to sixteen actions: the walk's wider forms (and their pre-passes), over their part of the batch
    for (int shape = 1; shape <= 2 && whi > wlo; ++shape) {
      if (!(shape == 1 ? pl.walk_wide : pl.walk_awide)) continue;
      KernelArgs kv = ka;
      kv.b.req_lo = wlo; kv.b.req_hi = whi;
      const u32 na = shape == 1 ? CBH_W2_NA : CBH_W2_AWIDE_NA;
      if (kv.b.n_gwords)
        go(shape == 1 ? cbh_walk2_pre_wide_kernel : cbh_walk2_pre_awide_kernel, (whi - wlo + CBH_BLOCK - 1) / CBH_BLOCK, CBH_BLOCK,
           plan_lds(true, na, 0), kv, false);
      go(shape == 1 ? (pl.trail ? cbh_walk2_wide_trail_kernel : cbh_walk2_wide_kernel) : (pl.trail ? cbh_walk2_awide_trail_kernel : cbh_walk2_awide_kernel),
         (whi - wlo + pl.threads - 1) / pl.threads, pl.threads, plan_lds(false, na, 0), kv, false);
    }
    if (ka.b.n_gwords && ka.b.site_cnt && ka.b.site_cap >= n && pre_split_on()) {
      // the evaluation sites in two kernels: who reaches which site (the walk's registers), then the sites' lists (the interpreter's)
      (void)hipMemsetAsync(ka.b.site_cnt, 0, (size_t)ka.b.n_gslots * 4, s);
      go(cbh_walk2_collect_kernel, (n + CBH_BLOCK - 1) / CBH_BLOCK, CBH_BLOCK,
         [&](bool packed) { return w2_lds_bytes(w2_layout(dev.inline_cols, false, dev.max_depth, dev.n_scopes, true, pl.n_gwords, dev.K, dev.n_dr, CBH_W2_NA, packed), 1u); }, ka, false);
      go(cbh_walk2_interp_kernel, ka.b.n_gslots * ((n + CBH_BLOCK - 1) / CBH_BLOCK), CBH_BLOCK, plan_lds(true, CBH_W2_NA, 0), ka, false);
    } else if (ka.b.n_gwords)   // the evaluation sites first: their results are what the walk reads
      go(cbh_walk2_pre_kernel, (n + CBH_BLOCK - 1) / CBH_BLOCK, CBH_BLOCK, plan_lds(true, CBH_W2_NA, 0), ka, false);
  }
  static const bool pre_only = env_set("CBH_PRE_ONLY");   // measurement aid (profiling build): the pre-pass alone
  if (pre_only && pl.kind == 2) return;
  if (pl.kind == 1 && pl.groups > 1) {
    // ---- action groups (cbh_check_flat.h flat_body AGROUP): the plan's kernel once per four actions, in order, same grid, range and LDS.
    // `dflag` ([n_requests] bytes of the batch, a table with derived roles whose call wants them): cleared for the range, ORed into
    // by the groups, read by the status kernel behind the last one.
    const cbh_group_kernel_fn gfn = cbh_flat_group_variant(pl.kernel);
    const auto lds_of = plan_lds(false, CBH_W2_NA, pad);
    const size_t wide = lds_of(false), packed = lds_of(true);
    const bool use_packed = packed_tags_pay(reinterpret_cast<cbh_check_kernel_fn>(gfn), pl.threads, wide, packed);
    KernelArgs a = ka;
    if (use_packed) a.flags |= CBH_FI_PACKED_TAGS;
    FlatGroupDev ag{};
    ag.dflag = (dev.n_dr && (ka.flags & CBH_F_WANT_DERIVED_ROLES) && ((ka.flags & CBH_FI_PACKED_RES) || ka.o.status)) ? dflag : nullptr;
    ag.each_from = pl.each_from;
    if (ag.dflag) (void)hipMemsetAsync(ag.dflag + lo, 0, n, s);
    const dim3 grid((n + pl.threads - 1) / pl.threads), block(pl.threads);
    if (trace_on()) std::fprintf(stderr, "[cbh] action groups=%u requests [%u,%u) status kernel=%d\n", pl.groups, lo, hi, ag.dflag ? 1 : 0);
    for (u32 g = 0; g < pl.groups; ++g) {
      ag.group = g;
      const bool last = g + 1 == pl.groups && !ag.dflag;
      if (ev0 || (ev1 && last)) { hipExtLaunchKernelGGL(gfn, grid, block, use_packed ? packed : wide, s, ev0, last ? ev1 : nullptr, 0, a, d_args, ag); ev0 = nullptr; }
      else hipLaunchKernelGGL(gfn, grid, block, use_packed ? packed : wide, s, a, d_args, ag);
    }
    if (ag.dflag) {
      FlatGroupStatusArgs sa{};
      sa.req_u32 = ka.b.req_u32; sa.dflag = ag.dflag; sa.n_requests = ka.b.n_requests; sa.lo = lo; sa.hi = hi;
      if (ka.flags & CBH_FI_PACKED_RES) sa.packed = ka.o.policy; else sa.status = ka.o.status;
      if (ev1) hipExtLaunchKernelGGL(cbh_flat_group_status_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, nullptr, ev1, 0, sa);
      else hipLaunchKernelGGL(cbh_flat_group_status_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, sa);
    }
    return;
  }
  go((ka.flags & CBH_FI_COMPACT) ? cbh_flat_compact_variant(pl.kernel) : pl.kernel, (n + pl.threads - 1) / pl.threads, pl.threads, plan_lds(false, CBH_W2_NA, pad), ka, true);
}
// CBH_LDS_PAD=<bytes> (measurement aid): extra dynamic LDS per workgroup of the resident launches, to hold the occupancy down
static size_t lds_pad() { static const size_t pad = (size_t)env_long("CBH_LDS_PAD", 0); return pad; }
static u32 nfa_maxw(const TableDev& d) { return std::max(std::max(d.nfa_words[0], d.nfa_words[1]), d.nfa_words[2]); }
static size_t check_lds_bytes(const BatchDev& d, u32 table_flags) {   // the column cache (tags in the wide form)
  const u32 ncc = d.n_columns < CBH_CACHE_COLS ? d.n_columns : CBH_CACHE_COLS;
  // ... and, for a table whose programs build lists, the lanes' arenas behind it (cbh_vm.h arena_vals)
  return (size_t)CBH_CC_DWORDS(ncc, false) * 4 + ((table_flags & CBH_MF_NEEDS_ARENA) ? (size_t)CBH_ARENA_ENTRIES * CBH_BLOCK * 9 : 0);
}

// Can the flat kernels' results of this table take the packed form (cbh_vm.h cbh_pk_word)?  Its ids and scope indices must fit the
// word's fields.  CBH_PACKED_RESULTS=0 (measurement aid): never.
static bool pk_fits(const TableDev& dev) {
  static const bool on = env_int("CBH_PACKED_RESULTS", 1) != 0;
  return on && cbh_pk_bits(dev.n_scopes) <= CBH_PK_MAX_BITS;
}

// Does this launch read the batch's compact form?  A flat kernel that has a compact instantiation (not: the variants with the
// evaluator call, the trail's kernels), and not a cycle-count launch - except in the profiling build, whose cycle counts are wanted
// of the kernel the product launches (tools/gpu_cycles_flat.py).
static bool launch_is_compact(const cbh_device_batch* b, const CbhPlan& pl, u32 eval_flags) {
#ifdef CBH_PROFILE_CYCLES
  eval_flags &= ~(u32)CBH_F_DEBUG_CYCLES;
#endif
  return b->compact && pl.kind == 1 && pl.groups <= 1 && !(eval_flags & CBH_F_DEBUG_CYCLES) && cbh_flat_compact_variant(pl.kernel) != nullptr;
}

extern "C" int cbh_check_resident(cbh_table* t, cbh_device_batch* b, const cbh_params* p) {
  if (!t || !b || !p) return fail("null argument");
  if (b->table != t) return fail("batch was uploaded for a different table");
  Replica* rep = b->rep;
  std::lock_guard<std::mutex> lk(rep->mu);
  HIPCHK(hipSetDevice(rep->device));
  hipStream_t s = b->stream;
  b->w.total_known = false;   // (the sizes cbh_wire_outputs computed belong to the results this launch replaces)
  // The walk's pre-pass as a collector and an interpreter over per-site lists - the lists
  // live with the batch (slots x requests items).  Tables whose programs read runtime.effectiveDerivedRoles keep the fused pre-pass.
  if (pre_split_on() && !b->dev.site_cnt && b->dev.n_requests && (rep->dev.flags & CBH_MF_WALK2) && rep->dev.gslots_all &&
      !(rep->dev.flags & CBH_MF_USES_RUNTIME_EDR) && b->dev.gres) {
    u32* cnt = nullptr; u64* list = nullptr;
    if (dalloc(b, cnt, (size_t)rep->dev.gslots_all) != 0 || dalloc(b, list, (size_t)rep->dev.gslots_all * b->dev.n_requests) != 0) return -1;
    b->dev.site_cnt = cnt; b->dev.site_list = list; b->dev.site_cap = b->dev.n_requests;
  }
  // Kernel durations come from the dispatches' own begin / end timestamps (hipExtLaunchKernelGGL
  // with start / stop events: what rocprofv3's kernel trace reads too), not from event-record
  // packets placed around them, which would sit between back-to-back launches and add their own
  // latency to the figure.
  // Every fourth launch is timed (and the first few, so that a short run has a figure): a
  // timestamped dispatch costs the queue a little more than a plain one.
  const uint64_t launch_no = rep->launches++;
  const bool timed = launch_no < 4 || (launch_no & 3) == 0;
  Replica::Slot scratch_slot;
  Replica::Slot& sl = timed ? rep->ring[rep->next_slot++ % Replica::RING] : scratch_slot;
  if (timed && sl.pending) { HIPCHK(hipEventSynchronize(sl.ev[3])); collect_slot(rep, sl); }
  const BatchDev& d = b->dev;
  const CbhPlan pl = d.n_requests ? plan_for(rep->dev, b->shape, p->flags) : CbhPlan{};
  // A flat launch writes its results packed, a word per tuple, where the table's ids fit (not: the trail's kernels, the wire road's
  // batches - cbh_wire_outputs reads the wide arrays -, cycle-count launches); and for a table without derived roles no mask at all.
  // (action groups on a table with derived roles: a byte per request for the error of a definition, flat_body AGROUP)
  if (pl.kind == 1 && pl.groups > 1 && rep->dev.n_dr && !b->dflag && dalloc(b, b->dflag, (size_t)d.n_requests) != 0) { b->dflag = nullptr; return -1; }
  b->res_packed = pl.kind == 1 && !cbh_is_flat_trail_kernel(pl.kernel) && !b->wire && !(p->flags & CBH_F_DEBUG_CYCLES) && pk_fits(rep->dev);
  b->edr_zero = b->res_packed && rep->dev.n_dr == 0;
  {
    // launch arguments live in device memory; re-sent only when they change (the kernel itself
    // writes every output word of every request, so nothing needs clearing between launches)
    KernelArgs ka;
    std::memset(&ka, 0, sizeof(ka));
    ka.t = rep->dev; ka.b = d; ka.o = b->out; ka.now_ns = p->now_ns; ka.flags = p->flags & ~(u32)CBH_FI_MASK;
    if (b->res_packed) ka.flags |= CBH_FI_PACKED_RES;
    if (launch_is_compact(b, pl, p->flags)) ka.flags |= CBH_FI_COMPACT;
    if (b->edr_zero) ka.o.edr = nullptr;
    if (!b->have_args || std::memcmp(&ka, &b->last_args, sizeof(ka)) != 0) {
      b->last_args = ka; b->have_args = true;
      HIPCHK(hipMemcpyAsync(b->d_args, &b->last_args, sizeof(ka), hipMemcpyHostToDevice, s));
    }
  }
  // batch-local strings against the table's glob automata; a table without globs has nothing to
  // resolve (the bits were zeroed once at upload)
  const u32 maxw = nfa_maxw(rep->dev);
  sl.resolved = d.n_strings && maxw;
  if (sl.resolved) {
    const u32 grid = (d.n_strings + CBH_BLOCK - 1) / CBH_BLOCK;
    const size_t lds = (size_t)(2 + 512) * maxw * sizeof(u64);
    if (timed) hipExtLaunchKernelGGL(cbh_resolve_globs_kernel, dim3(grid), dim3(CBH_BLOCK), lds, s, sl.ev[0], sl.ev[1], 0, rep->dev, d);
    else hipLaunchKernelGGL(cbh_resolve_globs_kernel, dim3(grid), dim3(CBH_BLOCK), lds, s, rep->dev, d);
  }
  sl.pending = false;
  if (d.n_requests) {
    launch_plan(pl, rep->dev, b->last_args, (const KernelArgs*)b->d_args, 0, d.n_requests, b->shape.wide_lo, b->shape.wide_hi, lds_pad(), s, timed ? sl.ev[2] : nullptr, timed ? sl.ev[3] : nullptr, b->dflag);
    sl.pending = timed;
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// A sweep: cbh_check_resident for each of `n` resident batches of the table, in order, in one call (what a server's dispatch loop
// does between two polls of its queue; saves the caller n - 1 crossings of the boundary).
extern "C" int cbh_check_resident_many(cbh_table* t, cbh_device_batch* const* bs, uint32_t n, const cbh_params* p) {
  if (!t || (!bs && n) || !p) return fail("null argument");
  for (uint32_t i = 0; i < n; ++i) if (cbh_check_resident(t, bs[i], p) != 0) return -1;
  return 0;
}

// How many of the replica's resident streams batches uploaded FROM NOW ON are dealt to (1 .. Replica::MAX_RESIDENT_STREAMS; a batch keeps its stream).
// 1 = every launch queues behind the one before it: the setting for timing one kernel by itself.
extern "C" int cbh_table_set_resident_streams(cbh_table* t, uint32_t n) {
  if (!t) return fail("null argument");
  if (n < 1 || n > (uint32_t)Replica::MAX_RESIDENT_STREAMS) return fail("resident streams: 1 .. " + std::to_string(Replica::MAX_RESIDENT_STREAMS));
  for (Replica* rep : t->reps) { rep->n_rstreams.store((int)n); rep->next_rstream.store(0); }
  return 0;
}
extern "C" uint32_t cbh_table_resident_streams(const cbh_table* t) { return t && !t->reps.empty() ? (uint32_t)t->reps[0]->n_rstreams.load() : 0u; }

// Which kernels cbh_check_resident launches for this batch (measurement aid: bench.py names them in its line).
extern "C" const char* cbh_plan_describe(cbh_table* t, cbh_device_batch* b, const cbh_params* p) {
  static thread_local std::string s;
  if (!t || !b || !p) return "";
  const CbhPlan pl = plan_for(b->rep->dev, b->shape, p->flags & ~(u32)CBH_FI_MASK);
  // (the pre-pass's form: cbh_check_resident's own condition for giving the batch its site lists)
  const Replica* rep = b->rep;
  const bool pre_split = pre_split_on() && b->dev.n_requests && (rep->dev.flags & CBH_MF_WALK2) && rep->dev.gslots_all && !(rep->dev.flags & CBH_MF_USES_RUNTIME_EDR) && b->dev.gres;
  if (pl.kind == 2) s = std::string(pl.wide_kernel ? "cbh_check_kernel*(wide requests)+" : "") + (pl.walk_wide ? (pl.trail ? "cbh_walk2_wide_trail_kernel(5-8 roles)+" : "cbh_walk2_wide_kernel(5-8 roles)+") : "") + (pl.walk_awide ? (pl.trail ? "cbh_walk2_awide_trail_kernel(9-16 actions)+" : "cbh_walk2_awide_kernel(9-16 actions)+") : "") + (pl.n_gwords && b->dev.gres ? (pre_split ? "cbh_walk2_collect_kernel+cbh_walk2_interp_kernel+" : "cbh_walk2_pre_kernel+") : "") + (pl.trail ? "cbh_walk2_trail_kernel" : "cbh_walk2_kernel");
  else if (pl.kind == 1 && cbh_is_flat_trail_kernel(pl.kernel)) s = cbh_is_mask_kernel(pl.kernel) ? "cbh_check_flat_trail_kernel*_masks" : "cbh_check_flat_trail_kernel*";
  else if (pl.kind == 0 && pl.kernel == cbh_check_trail_kernel) s = "cbh_check_trail_kernel";
  else if (pl.kind == 1) s = pl.kernel == cbh_check_flat_kernel ? "cbh_check_flat_kernel" : pl.kernel == cbh_check_flat_kernel_dr ? "cbh_check_flat_kernel_dr" : pl.kernel == cbh_check_flat_kernel_any ? "cbh_check_flat_kernel_any"
                           : pl.kernel == cbh_check_flat_kernel_staged ? "cbh_check_flat_kernel_staged" : pl.kernel == cbh_check_flat_kernel_masks ? "cbh_check_flat_kernel_masks"
                           : pl.kernel == cbh_check_flat_kernel_any_masks ? "cbh_check_flat_kernel_any_masks" : "cbh_check_flat_kernel_any_staged";
  else s = "cbh_check_kernel*";
  if (pl.kind == 1 && pl.groups > 1) { char m[32]; snprintf(m, sizeof m, ", %u action groups", pl.groups); s += m; }
  if (launch_is_compact(b, pl, p->flags)) { char m[64]; snprintf(m, sizeof m, "[compact inputs, narrow columns 0x%x]", b->dev.compact_info & CBH_CI_NARROW_MASK); s += m; }
  return s.c_str();
}

extern "C" int cbh_synchronize(cbh_table* t) {
  if (!t) return fail("null argument");
  for (Replica* rep : t->reps) {
    std::lock_guard<std::mutex> lk(rep->mu);
    HIPCHK(hipSetDevice(rep->device));
    for (int i = 0; i < Replica::MAX_RESIDENT_STREAMS; ++i) if (rep->rstreams[i]) HIPCHK(hipStreamSynchronize(rep->rstreams[i]));
    { std::vector<hipStream_t> ws; { std::lock_guard<std::mutex> lw(rep->wstream_mu); ws = rep->wstreams_all; } for (hipStream_t x : ws) HIPCHK(hipStreamSynchronize(x)); }
    collect_times(rep);
  }
  return 0;
}

extern "C" int cbh_kernel_time_ms(cbh_table* t, float* check_ms, float* resolve_ms) {
  if (!t) return fail("null argument");
  double c = 0, r = 0; uint64_t n = 0;
  for (Replica* rep : t->reps) {
    std::lock_guard<std::mutex> lk(rep->mu);
    c += rep->check_ms_sum; r += rep->resolve_ms_sum; n += rep->timed;
    rep->check_ms_sum = rep->resolve_ms_sum = 0; rep->timed = 0;
  }
  if (n == 0) return fail("no timed launches yet");
  if (check_ms) *check_ms = (float)(c / (double)n);
  if (resolve_ms) *resolve_ms = (float)(r / (double)n);
  return 0;
}

extern "C" int cbh_result_download(cbh_table* t, cbh_device_batch* b, cbh_result* out) {
  if (!t || !b || !out) return fail("null argument");
  if (b->dev.n_tuples && !out->effect) return fail("cbh_result.effect is required");
  Replica* rep = b->rep;
  std::lock_guard<std::mutex> lk(rep->mu);
  HIPCHK(hipSetDevice(rep->device));
  hipStream_t s = b->stream;
  const BatchDev& d = b->dev;
  if (b->res_packed && d.n_tuples) {   // the last launch wrote the packed form: unpacked into the wide arrays, which then cross as before
    PkUnpackArgs ua; ua.effect = b->out.effect; ua.status = b->out.status; ua.policy = b->out.policy; ua.scope = b->out.scope;
    ua.n = d.n_tuples; ua.bits = cbh_pk_bits(rep->dev.n_scopes);
    hipLaunchKernelGGL(cbh_unpack_results_kernel, dim3((d.n_tuples + 255u) / 256u), dim3(256), 0, s, ua);
    HIPCHK(hipGetLastError());
    b->res_packed = false;   // (in place: the wide form is the live one now)
  }
  if (d.n_tuples) HIPCHK(hipMemcpyAsync(out->effect, b->out.effect, d.n_tuples, hipMemcpyDeviceToHost, s));
  if (out->policy && d.n_tuples) HIPCHK(hipMemcpyAsync(out->policy, b->out.policy, (size_t)d.n_tuples * 4, hipMemcpyDeviceToHost, s));
  if (out->scope && d.n_tuples) HIPCHK(hipMemcpyAsync(out->scope, b->out.scope, (size_t)d.n_tuples * 4, hipMemcpyDeviceToHost, s));
  if (out->status && d.n_tuples) HIPCHK(hipMemcpyAsync(out->status, b->out.status, d.n_tuples, hipMemcpyDeviceToHost, s));
  if (out->edr_mask && d.n_requests && b->edr_zero) std::memset(out->edr_mask, 0, (size_t)d.n_requests * 8);
  else if (out->edr_mask && d.n_requests) {
    const u64* src = b->out.edr;
    if (b->w.inv) {   // a batch grouped by route: the masks follow their requests back to input order
      if (!b->w.edr_input && dalloc(b, b->w.edr_input, (size_t)d.n_requests) != 0) return -1;
      WireUnsortArgs ua; ua.edr_grouped = b->out.edr; ua.inv = b->w.inv; ua.edr_input = b->w.edr_input; ua.n = d.n_requests; ua.pad = 0;
      hipLaunchKernelGGL(cbh_wire_unsort_edr_kernel, dim3((d.n_requests + 255u) / 256u), dim3(256), 0, s, ua);
      src = b->w.edr_input;
    }
    HIPCHK(hipMemcpyAsync(out->edr_mask, src, (size_t)d.n_requests * 8, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  collect_times(rep);
  return 0;
}

// One bit per tuple instead of at least one byte: the bitmap is made on the device from whichever form the last launch wrote (the
// packed words are NOT unpacked: the batch's results stay as they are for a later cbh_result_download) and crosses by itself.
extern "C" int cbh_result_download_allow_bits(cbh_table* t, cbh_device_batch* b, uint64_t* bits, size_t n_words) {
  if (!t || !b || !bits) return fail("null argument");
  if (b->table != t) return fail("batch was uploaded for a different table");
  const size_t need = ((size_t)b->dev.n_tuples + 63) / 64;
  if (n_words < need) return fail("cbh_result_download_allow_bits: the buffer is shorter than (n_tuples + 63) / 64 words");
  if (!need) return 0;
  Replica* rep = b->rep;
  std::lock_guard<std::mutex> lk(rep->mu);
  HIPCHK(hipSetDevice(rep->device));
  hipStream_t s = b->stream;
  if (!b->allow_bits && dalloc(b, b->allow_bits, need) != 0) { b->allow_bits = nullptr; return -1; }
  AllowBitsArgs a{};
  a.packed = b->res_packed ? b->out.policy : nullptr; a.effect = b->out.effect; a.bits = b->allow_bits; a.n_tuples = b->dev.n_tuples;
  hipLaunchKernelGGL(cbh_allow_bits_kernel, dim3((u32)(((size_t)b->dev.n_tuples + 255u) / 256u)), dim3(256), 0, s, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(bits, b->allow_bits, need * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  collect_times(rep);
  return 0;
}


// ---- engine.Check's second return value: the policies a call touched (AuditTrail.EffectivePolicies) ---------------------------
extern "C" uint32_t cbh_table_num_policies(const cbh_table* t) { return t ? t->wire.n_policies : 0; }
extern "C" int cbh_table_policy_key(const cbh_table* t, uint32_t i, const char** key, uint32_t* len) {
  if (!t || !key || !len) return fail("null argument");
  if (i >= t->wire.n_policies) return fail("policy index out of range");
  *key = reinterpret_cast<const char*>(t->wire.name_bytes.data()) + t->wire.name_off[i];
  *len = t->wire.name_off[i + 1] - t->wire.name_off[i];
  return 0;
}
// cbh_check_batch with the trail: the batch goes through the resident path of device 0 (upload, the general walk with
// CBH_F_WANT_EFFECTIVE_POLICIES, download) - the walk that iterates a request's roles one after the other as check.go:208-442
// does, so that "touched" means what it means there.
// The trail of a RESIDENT batch: cbh_batch_set_trail says which group (engine.Check call) every request of the batch belongs to and
// gives the batch its masks; from then on a cbh_check_resident with CBH_F_WANT_EFFECTIVE_POLICIES ORs into them, cbh_trail_download
// reads them (and cbh_batch_set_trail again clears them).  group_of_request: host memory, DEVICE order of the batch, NULL = one group.
extern "C" int cbh_batch_set_trail(cbh_table* t, cbh_device_batch* b, const uint32_t* group_of_request, uint32_t n_groups) {
  if (!t || !b) return fail("null argument");
  if (b->table != t) return fail("batch was uploaded for a different table");
  if (n_groups == 0) n_groups = 1;
  const u32 n = b->dev.n_requests;
  if (group_of_request) for (u32 r = 0; r < n; ++r) if (group_of_request[r] >= n_groups) return fail("cbh_batch_set_trail: group index out of range");
  Replica* rep = b->rep;
  HIPCHK(hipSetDevice(rep->device));
  hipStream_t s = b->stream;
  const u32 words = (t->wire.n_policies + 31u) / 32u;
  const size_t ep_n = (size_t)n_groups * (words ? words : 1u);
  if (!b->out.eff_pol || b->trail_groups != n_groups) {
    u32* d_ep = nullptr;
    if (dalloc(b, d_ep, ep_n) != 0) return -1;
    b->out.eff_pol = d_ep; b->out.ep_words = words; b->trail_groups = n_groups;
  }
  HIPCHK(hipMemsetAsync(b->out.eff_pol, 0, ep_n * 4, s));
  if (group_of_request && n) {
    if (!b->trail_grp && dalloc(b, b->trail_grp, (size_t)n) != 0) return -1;   // (kept: a batch is asked again and again)
    HIPCHK(hipMemcpyAsync(b->trail_grp, group_of_request, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));   // (a pageable source)
  }
  b->dev.ep_group = (group_of_request && n) ? b->trail_grp : nullptr;
  return 0;
}
extern "C" int cbh_trail_download(cbh_table* t, cbh_device_batch* b, uint32_t* effective_policies) {
  if (!t || !b || !effective_policies) return fail("null argument");
  if (!b->out.eff_pol) return fail("cbh_trail_download: the batch has no trail (cbh_batch_set_trail)");
  HIPCHK(hipSetDevice(b->rep->device));
  if (b->out.ep_words) HIPCHK(hipMemcpyAsync(effective_policies, b->out.eff_pol, (size_t)b->trail_groups * b->out.ep_words * 4, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

extern "C" int cbh_check_batch_trail(cbh_table* t, const cbh_batch* in, const cbh_params* p, cbh_result* out, const uint32_t* group_of_request,
                                     uint32_t n_groups, uint32_t* effective_policies) {
  if (!t || !in || !p || !out || !effective_policies) return fail("null argument");
  cbh_device_batch* b = nullptr;
  if (batch_upload(t, 0, in, &b, false) != 0) return -1;   // (a trail launch reads the wide arrays)
  struct Release { cbh_device_batch* b; ~Release() { cbh_batch_release(b); } } release{b};
  if (cbh_batch_set_trail(t, b, group_of_request, n_groups) != 0) return -1;
  cbh_params q = *p;
  q.flags |= CBH_F_WANT_EFFECTIVE_POLICIES;
  if (cbh_check_resident(t, b, &q) != 0) return -1;
  if (cbh_result_download(t, b, out) != 0) return -1;
  return cbh_trail_download(t, b, effective_policies);
}
