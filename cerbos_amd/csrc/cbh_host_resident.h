// Host side of libcerbos_hip.so, part 2 of 4 (included by cbh_engine.hip, host pass only): resident batches - validation, the
// three makers (host arrays, cross product; the wire road's is in cbh_host_wire.h), the choice of kernels and their launches,
// the downloads, the audit trail.
#pragma once

// Would cbh_plan decide a batch of this shape in action groups (flags permitting)?  Then the tags select its kernel, as for four actions.
static bool flat_groups_shape(const cbh_table* t, u32 max_actions, u32 max_roles) {
  return flat_action_groups_on() && !t->reps.empty() && cbh_flat_action_groups(t->reps[0]->dev.n_dr, max_actions, max_roles) != 0;
}
// ---- batch validation (O(n_requests), both entry points) ---------------------------------------------------
// Offsets and counts the kernels index device memory with must lie inside the arrays they index.  String ids
// need no host pass: the kernels only compare them, or bound them before using one as an index.
struct BatchShape {
  u32 max_actions = 0, max_roles = 0; bool ascending = true;
  u32 wide_lo = 0, wide_hi = 0;   // the requests with more than CBH_W2_NA actions or CBH_W2_NR roles lie in [wide_lo, wide_hi)
  // Do the attribute columns hold plain scalars only - no int / uint (cross-type numerics) and no list / map (deep
  // equality)?  Then no classified leaf can need the shared evaluator and the flat kernel without that call decides
  // the batch (cbh_check_flat.h).  One pass over the tag bytes, made only where the answer selects a kernel and only
  // when the first launch is being prepared - by then the uploads are enqueued and the pass runs beside them.
  const uint8_t* tags = nullptr; size_t n_tags = 0;   // nullptr: the answer cannot matter (no flat kernel for this table / shape)
  uint32_t sens_cols = 0; size_t n_req = 0;           // only these columns [bit c: tags + c * n_req] can send a classified leaf to the evaluator (CBH_M_SENS_COLS)
  mutable std::atomic<int> plain{-1};                 // -1 not looked at yet (racing threads compute the same answer)
  bool plain_tags() const {
    int v = plain.load(std::memory_order_relaxed);
    if (v < 0) {
      bool hit = false;
      if (tags) for (uint32_t c = 0; c < 32 && !hit; ++c) if ((sens_cols >> c) & 1u) hit = has_int_or_container_tag(tags + (size_t)c * n_req, n_req);
      v = (!flat_any_forced() && !hit) ? 1 : 0;
      plain.store(v, std::memory_order_relaxed);
    }
    return v == 1;
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
  sh.tags = nullptr; sh.n_tags = 0; sh.plain.store(-1, std::memory_order_relaxed);
  // (a flat kernel decides the batch: four actions or, in the action groups cbh_plan takes, up to CBH_MAX_ACTIONS_PER_REQUEST)
  if (((t->meta[CBH_M_FLAGS] & CBH_MF_FLAT) && maxr <= 4 && (maxa <= 4 || flat_groups_shape(t, maxa, maxr))) ||
      ((t->meta[CBH_M_FLAGS] & CBH_MF_WALK2) && t->meta[CBH_M_GSLOTS_ALL] > t->meta[CBH_M_GSLOTS_GENERIC])) { sh.tags = in->col_tag; sh.n_tags = (size_t)in->n_columns * NR; }
  sh.sens_cols = t->meta[CBH_M_SENS_COLS]; sh.n_req = NR;
  if (in->n_columns < 32) sh.sens_cols &= (1u << in->n_columns) - 1u;
  return 0;
}

// The compact form of a batch the flat kernels can decide (cbh_vm.h BatchDev.creq / cval), derived on the batch's stream from the wide
// arrays already enqueued: the scan's verdict crosses to the host (one word), then the records, the 32-bit planes and the tag planes are written.  A
// batch with a field that does not fit the record keeps the wide form; so does every batch under CBH_COMPACT_INPUTS=0 (measurement aid).
static bool compact_inputs_on() { static const bool on = env_int("CBH_COMPACT_INPUTS", 1) != 0; return on; }
static int batch_compact(cbh_device_batch* b, hipStream_t s) {
  const TableDev& dev = b->rep->dev;
  BatchDev& d = b->dev;
  if (!compact_inputs_on() || !(dev.flags & CBH_MF_FLAT) || b->max_actions > 4 || b->max_roles > 4 || !d.n_requests) return 0;
  CompactArgs ca{};
  ca.req_u32 = d.req_u32; ca.roles = d.roles; ca.tuple_action = d.tuple_action; ca.col_val = d.col_val; ca.col_tag = d.col_tag;
  ca.action_class = dev.action_class; ca.role_class = dev.role_class; ca.K = dev.K;
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
// (b->dev's counts and b->plain_tags are set).  gbits_words: three per batch-local string - or, for a wire batch of a table without
// automata, whose dictionary has many slots and nobody to read their bits, one
static int batch_device_buffers(cbh_device_batch* b, size_t gbits_words) {
  BatchDev& d = b->dev; const Replica* rep = b->rep;
  int rc = dalloc(b, d.gbits, gbits_words);
  d.n_gwords = (rep->dev.flags & CBH_MF_WALK2) ? w2_gwords(rep->dev.gslots_generic, rep->dev.gslots_all, b->plain_tags) : 0;
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

static int batch_upload(cbh_table* t, uint32_t device_index, const cbh_batch* in, cbh_device_batch** out, bool compact) {
  if (!t || !in || !out) return fail("null argument");
  if (device_index >= t->reps.size()) return fail("device index out of range");
  BatchShape sh;
  if (validate_batch(t, in, sh) != 0) return -1;
  Replica* rep = t->reps[device_index];
  HIPCHK(hipSetDevice(rep->device));
  cbh_device_batch* b = batch_new(t, rep, false);
  if (!b) return -1;
  b->max_actions = sh.max_actions; b->max_roles = sh.max_roles; b->plain_tags = sh.plain_tags();
  b->wide_lo = sh.wide_lo; b->wide_hi = sh.wide_hi;
  BatchDev& d = b->dev;
  batch_set_counts(b, in->n_requests, in->n_tuples, in->n_roles, in->n_columns, in->n_strings, in->heap_len);
  hipStream_t s = b->stream;
  const size_t NR = in->n_requests;
  int rc = 0;
  rc |= up(b, d.req_u32, in->req_u32, (size_t)CBH_RQ_NFIELDS * NR, s);
  rc |= up(b, d.roles, in->roles, in->n_roles, s);
  d.tuple_req = nullptr;   // informational on the host side; no kernel reads it
  rc |= up(b, d.tuple_action, in->tuple_action, in->n_tuples, s);
  rc |= up(b, d.col_tag, in->col_tag, (size_t)in->n_columns * NR, s);
  rc |= up(b, d.col_val, in->col_val, (size_t)in->n_columns * NR, s);
  rc |= up(b, d.heap_tag, in->heap_tag, in->heap_len, s);
  rc |= up(b, d.heap_val, in->heap_val, in->heap_len, s);
  rc |= up(b, d.str_off, in->str_off, in->n_strings ? (size_t)in->n_strings + 1 : 0, s);
  rc |= up(b, d.str_bytes, in->str_bytes, in->str_bytes_len, s);
  rc |= up(b, d.str_flags, in->str_flags, in->n_strings, s);
  rc |= batch_device_buffers(b, (size_t)3 * d.n_strings);
  if (rc != 0) { cbh_batch_release(b); return -1; }
  // glob bits of the batch-local strings: all zero unless the table has automata to run (then
  // cbh_check_resident overwrites every word on each launch)
  if (in->n_strings && hipMemsetAsync(d.gbits, 0, (size_t)3 * in->n_strings * sizeof(u64), s) != hipSuccess) {
    cbh_batch_release(b); return fail("upload failed");
  }
  if (compact && batch_compact(b, s) != 0) { cbh_batch_release(b); return -1; }
  if (hipStreamSynchronize(s) != hipSuccess) { cbh_batch_release(b); return fail("upload failed"); }
  *out = b;
  return 0;
}
extern "C" int cbh_batch_upload_on(cbh_table* t, uint32_t device_index, const cbh_batch* in, cbh_device_batch** out) { return batch_upload(t, device_index, in, out, true); }
extern "C" int cbh_batch_upload(cbh_table* t, const cbh_batch* in, cbh_device_batch** out) { return cbh_batch_upload_on(t, 0, in, out); }

// ---- cross-product batches: N + M halves up, the N x M product built in device memory (cbh_cross.h) ------------------------
// The batch's shape comes from the halves, looking only at the rows the product uses, so that the product gets the plan a
// host-built batch of the same requests gets (validate_batch's answers for that batch, without the batch).
// (`bounded`: the product is materialised, so N * M and N * M * A must stay below 2^32 - the direct road, cbh_cross_upload, has no such bound)
// (`plan_a`, set by the caller: the action count the plan is made for where it is not A - the direct road decides A > 4 four at a time)
// (`group_roles`, set by the caller: the plan is made for at most four roles - the direct road decides more four at a time)
struct CrossShape { std::vector<u8> side; u32 maxr = 0, wide_lo = 0, wide_hi = 0; bool plain = true; u32 plan_a = 0; bool group_roles = false; };
static int cross_validate(cbh_table* t, uint32_t device_index, const cbh_batch* h, const cbh_cross* x, bool bounded, CrossShape& cs) {
  if (device_index >= t->reps.size()) return fail("device index out of range");
  const u64 N = x->n_principals, M = x->n_resources, A = x->n_actions;
  if (!N || !M || !A) return fail("cbh_cross: n_principals, n_resources and n_actions must be at least 1");
  if (A > CBH_MAX_ACTIONS_PER_REQUEST) return fail("cbh_cross: more than CBH_MAX_ACTIONS_PER_REQUEST actions");
  if (!x->action_ids) return fail("null argument");
  if ((u64)h->n_requests != N + M) return fail("cbh_cross: the halves batch must hold n_principals + n_resources requests");
  if (bounded && (N * M >= (1ull << 32) || N * M * A >= (1ull << 32))) return fail("cbh_cross: the product has 2^32 requests or tuples, or more: split the resources");
  const u32 ncol = h->n_columns;
  if (ncol != t->meta[CBH_M_NCOLUMNS]) return fail("cbh_batch.n_columns does not match the table's column schema");
  if (t->wire.cols.size() < ncol) return fail("the image names no column paths (CBH_SEC_COLUMN_PATHS): which half a column comes from is unknown");
  if (!h->req_u32 || (h->n_roles && !h->roles) || (ncol && (!h->col_tag || !h->col_val)) || (h->heap_len && (!h->heap_tag || !h->heap_val)) ||
      (h->n_strings && (!h->str_off || !h->str_flags)) || (h->str_bytes_len && !h->str_bytes)) return fail("cbh_batch: a required array is NULL");
  if (h->n_strings && h->str_off[h->n_strings] > h->str_bytes_len) return fail("cbh_batch: string offsets exceed str_bytes_len");
  const size_t NH = (size_t)(N + M), NM = (size_t)(N * M);
  std::vector<u8>& side = cs.side; std::vector<u8> seen;
  try { side.assign(ncol ? ncol : 1, 0); seen.assign(std::max(N, M), 0); } catch (...) { return fail("out of memory"); }
  for (u32 c = 0; c < ncol; ++c) side[c] = t->wire.cols[c].root == 1 ? 1 : 0;
  for (int which = 0; which < 2; ++which) {   // the orders are permutations
    const uint32_t* ord = which ? x->r_order : x->p_order; const u64 cnt = which ? M : N;
    if (!ord) continue;
    std::fill(seen.begin(), seen.begin() + cnt, (u8)0);
    for (u64 i = 0; i < cnt; ++i) {
      if (ord[i] >= cnt || seen[ord[i]]) return fail(which ? "cbh_cross: r_order is not a permutation of 0 .. n_resources - 1" : "cbh_cross: p_order is not a permutation of 0 .. n_principals - 1");
      seen[ord[i]] = 1;
    }
  }
  // roles of the principals; where the requests wider than the walk's base shape lie in the product (validate_batch's wide_lo / wide_hi)
  const u32* role_off = h->req_u32 + (size_t)CBH_RQ_ROLE_OFF * NH; const u32* role_cnt = h->req_u32 + (size_t)CBH_RQ_ROLE_CNT * NH;
  u32 maxr = 0, bad = 0; u64 ilo = N, ihi = 0;   // device positions i' of the principals with more than CBH_W2_NR roles
  for (u64 ip = 0; ip < N; ++ip) {
    const size_t i = x->p_order ? x->p_order[ip] : ip;
    maxr = role_cnt[i] > maxr ? role_cnt[i] : maxr;
    bad |= (u32)((u64)role_off[i] + role_cnt[i] > (u64)h->n_roles);
    if (role_cnt[i] > CBH_W2_NR) { if (ilo == N) ilo = ip; ihi = ip + 1; }
  }
  if (bad) return fail("cbh_batch: a request's role or action slice lies outside the batch");
  u32 wide_lo = 0, wide_hi = 0;
  if (A > CBH_W2_NA) wide_hi = (u32)NM;
  else if (ihi) { wide_lo = (u32)ilo; wide_hi = (u32)((M - 1) * N + ihi); }
  // plain tags: BatchShape::plain_tags over the rows the product uses
  bool plain = true;
  {
    const u32 mf = t->meta[CBH_M_FLAGS];
    const bool matters = ((mf & CBH_MF_FLAT) && ((cs.plan_a ? cs.plan_a : A) <= 4 || flat_groups_shape(t, (u32)A, maxr)) && (maxr <= 4 || cs.group_roles)) || ((mf & CBH_MF_WALK2) && t->meta[CBH_M_GSLOTS_ALL] > t->meta[CBH_M_GSLOTS_GENERIC]);
    u32 sens = t->meta[CBH_M_SENS_COLS];
    if (ncol < 32) sens &= (1u << ncol) - 1u;
    bool hit = false;
    if (matters) for (u32 c = 0; c < 32 && c < ncol && !hit; ++c) if ((sens >> c) & 1u)
      hit = side[c] ? BatchShape::has_int_or_container_tag(h->col_tag + (size_t)c * NH + N, M) : BatchShape::has_int_or_container_tag(h->col_tag + (size_t)c * NH, N);
    plain = !flat_any_forced() && !hit;
  }
  cs.maxr = maxr; cs.wide_lo = wide_lo; cs.wide_hi = wide_hi; cs.plain = plain;
  return 0;
}
static int cross_upload(cbh_table* t, uint32_t device_index, const cbh_batch* h, const cbh_cross* x, cbh_device_batch** out) {
  if (!t || !h || !x || !out) return fail("null argument");
  *out = nullptr;
  CrossShape cs;
  if (cross_validate(t, device_index, h, x, true, cs) != 0) return -1;
  const u64 N = x->n_principals, M = x->n_resources, A = x->n_actions;
  const u32 ncol = h->n_columns;
  const size_t NH = (size_t)(N + M), NM = (size_t)(N * M), NT = (size_t)(N * M * A);
  const std::vector<u8>& side = cs.side;
  const u32 maxr = cs.maxr, wide_lo = cs.wide_lo, wide_hi = cs.wide_hi; const bool plain = cs.plain;
  Replica* rep = t->reps[device_index];
  HIPCHK(hipSetDevice(rep->device));
  cbh_device_batch* b = batch_new(t, rep, false);
  if (!b) return -1;
  b->max_actions = (u32)A; b->max_roles = maxr; b->plain_tags = plain; b->wide_lo = wide_lo; b->wide_hi = wide_hi;
  BatchDev& d = b->dev;
  batch_set_counts(b, (u32)NM, (u32)NT, h->n_roles, ncol, h->n_strings, h->heap_len);
  hipStream_t s = b->stream;
  CrossArgs ca{};
  ca.n = (u32)N; ca.m = (u32)M; ca.a = (u32)A; ca.n_columns = ncol;
  int rc = 0;
  // the halves, the orders, the sides and the action ids (they stay with the batch until it is released: N + M rows)
  rc |= up(b, ca.h_req, h->req_u32, (size_t)CBH_RQ_NFIELDS * NH, s);
  rc |= up(b, ca.h_tag, h->col_tag, (size_t)ncol * NH, s);
  rc |= up(b, ca.h_val, h->col_val, (size_t)ncol * NH, s);
  if (x->p_order) rc |= up(b, ca.p_order, x->p_order, (size_t)N, s);
  if (x->r_order) rc |= up(b, ca.r_order, x->r_order, (size_t)M, s);
  rc |= up(b, ca.col_side, (const u8*)side.data(), (size_t)ncol, s);
  rc |= up(b, ca.action_ids, x->action_ids, (size_t)A, s);
  // shared as they are
  rc |= up(b, d.roles, h->roles, h->n_roles, s);
  rc |= up(b, d.heap_tag, h->heap_tag, h->heap_len, s);
  rc |= up(b, d.heap_val, h->heap_val, h->heap_len, s);
  rc |= up(b, d.str_off, h->str_off, h->n_strings ? (size_t)h->n_strings + 1 : 0, s);
  rc |= up(b, d.str_bytes, h->str_bytes, h->str_bytes_len, s);
  rc |= up(b, d.str_flags, h->str_flags, h->n_strings, s);
  // the product
  d.tuple_req = nullptr;
  rc |= dalloc(b, ca.req, (size_t)CBH_RQ_NFIELDS * NM);
  rc |= dalloc(b, ca.tag, (size_t)ncol * NM);
  rc |= dalloc(b, ca.val, (size_t)ncol * NM);
  rc |= dalloc(b, ca.tuple_action, NT);
  rc |= batch_device_buffers(b, (size_t)3 * d.n_strings);
  if (rc != 0) { cbh_batch_release(b); return -1; }
  d.req_u32 = ca.req; d.col_tag = ca.tag; d.col_val = ca.val; d.tuple_action = ca.tuple_action;
  if (h->n_strings && hipMemsetAsync(d.gbits, 0, (size_t)3 * h->n_strings * sizeof(u64), s) != hipSuccess) { cbh_batch_release(b); return fail("upload failed"); }
  hipLaunchKernelGGL(cbh_cross_expand_kernel, dim3((u32)((NM + 255u) / 256u)), dim3(256), 0, s, ca);
  hipLaunchKernelGGL(cbh_cross_actions_kernel, dim3((u32)(((NT + 3u) / 4u + 255u) / 256u)), dim3(256), 0, s, ca);
  if (hipGetLastError() != hipSuccess) { cbh_batch_release(b); return fail("cross-product expansion failed to launch"); }
  // (`side` is pageable memory of this frame: its copy must have left before the frame goes - batch_compact synchronises, or the wait below)
  if (batch_compact(b, s) != 0) { cbh_batch_release(b); return -1; }
  if (hipStreamSynchronize(s) != hipSuccess) { cbh_batch_release(b); return fail("upload failed"); }
  *out = b;
  return 0;
}
extern "C" int cbh_batch_upload_cross(cbh_table* t, uint32_t device_index, const cbh_batch* halves, const cbh_cross* x, cbh_device_batch** out) {
  try { return cross_upload(t, device_index, halves, x, out); } catch (...) { return fail("out of memory"); }
}

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
  const CbhPlan pl = d.n_requests ? plan_for(rep->dev, b->max_actions, b->max_roles, b->plain_tags, p->flags) : CbhPlan{};
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
    launch_plan(pl, rep->dev, b->last_args, (const KernelArgs*)b->d_args, 0, d.n_requests, b->wide_lo, b->wide_hi, lds_pad(), s, timed ? sl.ev[2] : nullptr, timed ? sl.ev[3] : nullptr, b->dflag);
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

// How many of the replica's resident streams batches uploaded FROM NOW ON are dealt to (1 .. 4; a batch keeps its stream).
// 1 = every launch queues behind the one before it: the setting for timing one kernel by itself.
extern "C" int cbh_table_set_resident_streams(cbh_table* t, uint32_t n) {
  if (!t) return fail("null argument");
  if (n < 1 || n > (uint32_t)Replica::MAX_RESIDENT_STREAMS) return fail("resident streams: 1 .. 8");
  for (Replica* rep : t->reps) { rep->n_rstreams.store((int)n); rep->next_rstream.store(0); }
  return 0;
}
extern "C" uint32_t cbh_table_resident_streams(const cbh_table* t) { return t && !t->reps.empty() ? (uint32_t)t->reps[0]->n_rstreams.load() : 0u; }

// Which kernels cbh_check_resident launches for this batch (measurement aid: bench.py names them in its line).
extern "C" const char* cbh_plan_describe(cbh_table* t, cbh_device_batch* b, const cbh_params* p) {
  static thread_local std::string s;
  if (!t || !b || !p) return "";
  const CbhPlan pl = plan_for(b->rep->dev, b->max_actions, b->max_roles, b->plain_tags, p->flags & ~(u32)CBH_FI_MASK);
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


// ---- the direct cross road: N x M decided straight from the N + M halves (cerbos_hip.h cbh_cross_upload_ex / cbh_cross_check) ----
// The set is the HALVES as a resident batch in its compact form (batch_upload + batch_compact, unchanged: the device holds N + M
// rows, the wide arrays included - cbh_cross_pairs_upload gathers from them), the two orders, the columns' sides and the actions'
// classes as one word per group of four.  A check launches the `_x` sibling of the kernel plan_for picks for (min(A, 4) actions,
// the principals' roles, plain tags) with the compact launch's LDS, over the tile's N * (r_end - r_begin) pairs - once per group
// of four actions, on the set's stream, each launch writing its own planes; what comes back is one ballot word per 64 pairs and
// action.  The planes' device words belong to the set's batch (the replica's pool) and serve every tile that fits them.
// A set whose principals have five to CBH_CX_MAX_ROLES roles (CBH_CX_ROLE_GROUPS) is uploaded with the principals' role counts
// clamped to four - the compact record then holds a principal's first four roles, group 0 - and keeps one role word per principal
// and further group of four roles (cbh_cross_role_word_kernel); a check launches, per group of actions, role group 0, then 1, 2, ...
// of the same kernel, each ORing into the planes what the groups before it left open (flat_body CROSS).
struct cbh_cross_set {
  cbh_device_batch* b = nullptr;
  u32 n = 0, m = 0, a = 0, maxr = 0; bool plain = true;
  const u32* p_order = nullptr; const u32* r_order = nullptr;   // device, or null = identity
  u32 side = 0;                                                   // the cached columns' sides as a mask (CrossDev.side)
  std::vector<u32> act_words;                                     // one per group of four actions (cbh_cross_act_word_kernel)
  u64* planes = nullptr; size_t plane_cap = 0;   // [allow | flagged][a][words]
  // what cbh_cross_pairs_upload needs beside the halves' own arrays: every column's side and the action ids on the device, the
  // principals' role counts by device position (the shape of a batch of chosen pairs), the length of the strings' bytes
  const u8* d_side = nullptr; const u32* d_act = nullptr;
  std::vector<u8> p_roles; u32 str_bytes_len = 0;
  // a set with role groups (maxr > 4): [(groups - 1)][n] role words and [n] class masks of all roles, by halves row (CrossRoleGroup), and the
  // principals' true role counts by halves row for the gather (the halves' request words on the device hold them clamped)
  const u32* role_words = nullptr; const u32* rc_all = nullptr; const u32* d_role_cnt = nullptr;
  const CrossRoleGroup* d_rg = nullptr;   // ... and the launches' records, one per role group (CrossDev.rg)
};
static u32 cross_groups(const cbh_cross_set* cs) { return (cs->a + 3u) / 4u; }
static u32 cross_role_groups(const cbh_cross_set* cs) { return cs->maxr > 4u ? (cs->maxr + 3u) / 4u : 1u; }
// The flagged planes are the status of the materialised product, and the kernels that decide a product of wide requests do not agree
// on where an error of a derived-role definition is marked (cbh_check_flat.h flat_body): from how many roles on a principal's
// requests would be decided by the general walk, by the product's own plan (launch_plan: CBH_FI_ONLY_WIDE / CBH_FI_ONLY_WIDER).
// (The flags that change a product's plan - strict evaluation, the trail - have no direct form: the plan under flags 0 is the one.)
static u32 cross_open_from(const TableDev& dev, const cbh_cross_set* cs) {
  const CbhPlan pp = plan_for(dev, cs->a, cs->maxr, cs->plain, 0, false);   // (the marks' places are those of the plan without action groups, which the groups reproduce)
  if (pp.kind == 0) return 0u;
  if (pp.kind != 2 || !pp.wide_kernel) return 0xFFFFFFFFu;
  if (pp.walk_wide || pp.walk_awide) return cs->a > CBH_W2_AWIDE_NA ? 0u : cs->a > CBH_W2_NA ? CBH_W2_NR + 1u : CBH_W2_WIDE_NR + 1u;   // cbh_is_wider
  return cs->a > CBH_W2_NA ? 0u : CBH_W2_NR + 1u;                                                                                          // cbh_is_wide
}
static cbh_cross_kernel_fn cross_kernel_for(const cbh_cross_set* cs, u32 eval_flags, CbhPlan& pl) {
  // (for at most four roles: with more, plan_for picks a walk kernel, which has no `_x` variant)
  pl = plan_for(cs->b->rep->dev, std::min(cs->a, 4u), std::min(cs->maxr, 4u), cs->plain, eval_flags & ~(u32)CBH_FI_MASK);
  if (pl.kind != 1 || (eval_flags & CBH_F_DEBUG_CYCLES)) return nullptr;
  return cbh_flat_cross_variant(pl.kernel);
}
static int cross_set_upload(cbh_table* t, uint32_t device_index, const cbh_batch* h, const cbh_cross* x, uint32_t accept, cbh_cross_set** out) {
  if (out) *out = nullptr;
  if (!t || !h || !x || !out) return fail("null argument");
  if (accept & ~(uint32_t)(CBH_CX_DERIVED_ROLES | CBH_CX_ACTION_GROUPS | CBH_CX_ROLE_GROUPS)) return fail("cbh_cross_upload_ex: `accept` has a bit this library does not know");
  CrossShape shape;
  shape.plan_a = std::min(x->n_actions, 4u);
  shape.group_roles = (accept & CBH_CX_ROLE_GROUPS) != 0;
  if (cross_validate(t, device_index, h, x, false, shape) != 0) return -1;
  Replica* rep = t->reps[device_index];
  const u32 N = x->n_principals, M = x->n_resources, A = x->n_actions;
  // no direct form: the caller takes cbh_batch_upload_cross, which gives the same answers
  if (!(rep->dev.flags & CBH_MF_FLAT)) { g_err = "cbh_cross_upload: no direct form - the table is not flat"; return 1; }
  if (rep->dev.n_dr && !(accept & CBH_CX_DERIVED_ROLES)) { g_err = "cbh_cross_upload: no direct form - the table has derived roles"; return 1; }
  if (A > 4 && !(accept & CBH_CX_ACTION_GROUPS)) { g_err = "cbh_cross_upload: no direct form - more than four actions"; return 1; }
  if (shape.maxr > 4 && !(accept & CBH_CX_ROLE_GROUPS)) { g_err = "cbh_cross_upload: no direct form - a principal has more than four roles"; return 1; }
  if (shape.maxr > CBH_CX_MAX_ROLES) { g_err = "cbh_cross_upload: no direct form - a principal has more than CBH_CX_MAX_ROLES (16) roles"; return 1; }
  if (!shape.plain) { g_err = "cbh_cross_upload: no direct form - an attribute value needs the evaluator (int / uint / list / map in a sensitive column)"; return 1; }
  if (!compact_inputs_on()) { g_err = "cbh_cross_upload: no direct form - compact inputs are switched off"; return 1; }
  {   // the kernel the product would be planned (mask walk of a table that is not closed over the classified leaves: cbh_flat_cross_mode)
    const CbhPlan pl = plan_for(rep->dev, shape.plan_a, std::min(shape.maxr, 4u), shape.plain, 0);
    if (pl.kind != 1 || !cbh_flat_cross_variant(pl.kernel)) { g_err = "cbh_cross_upload: no direct form - the kernel planned for this table has no direct instantiation"; return 1; }
  }
  cbh_cross_set* cs = new (std::nothrow) cbh_cross_set();
  if (!cs) return fail("out of memory");
  cs->n = N; cs->m = M; cs->a = A; cs->maxr = shape.maxr; cs->plain = shape.plain; cs->str_bytes_len = h->str_bytes_len;
  for (u32 c = 0; c < h->n_columns && c < CBH_CACHE_COLS; ++c) if (shape.side[c]) cs->side |= 1u << c;
  const size_t NH = (size_t)N + M;
  cs->p_roles.resize(N);
  for (u32 ip = 0; ip < N; ++ip) cs->p_roles[ip] = (u8)h->req_u32[(size_t)CBH_RQ_ROLE_CNT * NH + (x->p_order ? x->p_order[ip] : ip)];   // (<= CBH_CX_MAX_ROLES: checked above)
  // The halves' OWN actions are not read by any road of a set, but a row that carries more than four of them has no compact
  // record (cbh_compact_scan_kernel) - and the flattener hands the set's A actions to the first row.  A set of action groups
  // therefore uploads the request words with such rows' action counts cleared; a set of up to four actions is uploaded as it is.
  // Likewise a principal's row with more than four roles: a set of role groups uploads it with the count clamped to four, so that
  // its record holds the first four roles (the slices were checked by cross_validate; the resources' rows stay as they are).
  cbh_batch hh = *h;
  std::vector<u32> req_copy;
  if (A > 4 || shape.maxr > 4) req_copy.assign(h->req_u32, h->req_u32 + (size_t)CBH_RQ_NFIELDS * NH);
  if (shape.maxr > 4) {
    u32* cnt = req_copy.data() + (size_t)CBH_RQ_ROLE_CNT * NH;
    for (size_t r = 0; r < N; ++r) cnt[r] = std::min(cnt[r], 4u);
    hh.req_u32 = req_copy.data();
  }
  if (A > 4) {
    u32* cnt = req_copy.data() + (size_t)CBH_RQ_ACT_CNT * NH;
    for (size_t r = 0; r < NH; ++r) if (cnt[r] > 4u && (u64)req_copy[(size_t)CBH_RQ_ACT_OFF * NH + r] + cnt[r] <= (u64)h->n_tuples) cnt[r] = 0;   // (a slice outside the batch stays, to be refused)
    hh.req_u32 = req_copy.data();
  }
  // the halves: an ordinary resident batch of N + M requests (validated as one: the scan and the pack read every row's role and
  // action slices) with its compact form
  if (batch_upload(t, device_index, &hh, &cs->b, true) != 0) { delete cs; return -1; }
  cbh_device_batch* b = cs->b;
  auto drop = [&](int rc) { cbh_batch_release(b); delete cs; return rc; };
  b->max_actions = A; b->max_roles = shape.maxr; b->plain_tags = shape.plain;   // (the PRODUCT's shape; the plan is made for min(A, 4) actions: cross_kernel_for)
  if (!b->compact) { g_err = "cbh_cross_upload: no direct form - a field of the halves does not fit the compact record (CBH_CI_MISFIT)"; return drop(1); }
  hipStream_t s = b->stream;
  u32* d_word = nullptr;
  const u32 G = cross_groups(cs);
  cs->act_words.assign(G, 0u);
  int rc = 0;
  if (x->p_order) rc |= up(b, cs->p_order, x->p_order, (size_t)N, s);
  if (x->r_order) rc |= up(b, cs->r_order, x->r_order, (size_t)M, s);
  rc |= up(b, cs->d_act, x->action_ids, (size_t)A, s);
  rc |= up(b, cs->d_side, (const u8*)shape.side.data(), (size_t)h->n_columns, s);   // (pageable memory of this frame: the wait below)
  rc |= dalloc(b, d_word, G);
  const u32 R = cross_role_groups(cs);
  u32* d_rw = nullptr; u32* d_all = nullptr;
  if (R > 1) {
    rc |= up(b, cs->d_role_cnt, h->req_u32 + (size_t)CBH_RQ_ROLE_CNT * NH, (size_t)N, s);   // (the caller's words: the true counts)
    rc |= dalloc(b, d_rw, (size_t)(R - 1) * N);
    rc |= dalloc(b, d_all, (size_t)N);
  }
  if (rc != 0) return drop(-1);
  if (R > 1) {
    CrossRoleWordArgs ra{}; ra.role_off = b->dev.req_u32 + (size_t)CBH_RQ_ROLE_OFF * NH; ra.role_cnt = cs->d_role_cnt; ra.roles = b->dev.roles;
    ra.role_class = rep->dev.role_class; ra.words = d_rw; ra.all = d_all; ra.n = N; ra.groups = R; ra.K = rep->dev.K;
    hipLaunchKernelGGL(cbh_cross_role_word_kernel, dim3((N + 255u) / 256u), dim3(256), 0, s, ra);
    cs->role_words = d_rw; cs->rc_all = d_all;
    std::vector<CrossRoleGroup> recs(R);   // (pageable memory of this frame: the wait below)
    const u32 open_from = cross_open_from(rep->dev, cs);
    for (u32 g = 0; g < R; ++g) recs[g] = CrossRoleGroup{g ? d_rw + (size_t)(g - 1u) * N : nullptr, d_all, cs->d_role_cnt, g, open_from};
    if (up(b, cs->d_rg, recs.data(), (size_t)R, s) != 0 || hipStreamSynchronize(s) != hipSuccess) { (void)hipGetLastError(); fail("cbh_cross_upload: upload failed"); return drop(-1); }
  }
  CrossActWordArgs wa{}; wa.action_ids = cs->d_act; wa.action_class = rep->dev.action_class; wa.out = d_word; wa.a = A; wa.K = rep->dev.K;
  hipLaunchKernelGGL(cbh_cross_act_word_kernel, dim3(1), dim3(64), 0, s, wa);
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(cs->act_words.data(), d_word, (size_t)G * 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
    (void)hipGetLastError(); fail("cbh_cross_upload: upload failed"); return drop(-1);
  }
  *out = cs;
  return 0;
}
extern "C" int cbh_cross_upload_ex(cbh_table* t, uint32_t device_index, const cbh_batch* halves, const cbh_cross* x, uint32_t accept, cbh_cross_set** out) {
  try { return cross_set_upload(t, device_index, halves, x, accept, out); } catch (...) { return fail("out of memory"); }
}
extern "C" int cbh_cross_upload(cbh_table* t, uint32_t device_index, const cbh_batch* halves, const cbh_cross* x, cbh_cross_set** out) {
  return cbh_cross_upload_ex(t, device_index, halves, x, 0, out);
}
static int cross_set_check(cbh_table* t, cbh_cross_set* cs, const cbh_params* p, uint32_t r_begin, uint32_t r_end, uint64_t* allow, uint64_t* flagged, size_t words_per_plane) {
  if (!t || !cs || !p || !allow) return fail("null argument");
  cbh_device_batch* b = cs->b;
  if (b->table != t) return fail("the set was uploaded for a different table");
  if (r_begin >= r_end || r_end > cs->m) return fail("cbh_cross_check: [r_begin, r_end) must be a non-empty range of the set's resources");
  const u64 nt = (u64)cs->n * (r_end - r_begin);
  if (nt >= (1ull << 32)) return fail("cbh_cross_check: the tile has 2^32 requests or more: take fewer resources");
  const size_t W = (size_t)((nt + 63) / 64);
  if (words_per_plane < W) return fail("cbh_cross_check: words_per_plane is less than (n_principals * (r_end - r_begin) + 63) / 64");
  CbhPlan pl;
  const cbh_cross_kernel_fn fn = cross_kernel_for(cs, p->flags, pl);
  if (!fn) { g_err = "cbh_cross_check: these flags choose a plan without a direct form"; return 1; }
  Replica* rep = b->rep;
  std::lock_guard<std::mutex> lk(rep->mu);
  HIPCHK(hipSetDevice(rep->device));
  hipStream_t s = b->stream;
  const size_t per = (size_t)cs->a * W, need = per * (flagged ? 2 : 1);
  if (need > cs->plane_cap) {
    // a larger tile than any before: a new block, and the old one back to the replica's pool (every check ends with a wait for its
    // copies, so nothing of the stream still reads it)
    u64* np = nullptr;
    if (dalloc(b, np, need) != 0) return -1;
    if (cs->planes) {
      for (size_t i = 0; i < b->allocs.size(); ++i) if (b->allocs[i].first == (void*)cs->planes) {
        { std::lock_guard<std::mutex> pl(rep->pool_mu); rep->pool_free.push_back(b->allocs[i]); }
        b->allocs[i] = b->allocs.back(); b->allocs.pop_back();
        break;
      }
    }
    cs->planes = np; cs->plane_cap = need;
  }
  KernelArgs ka;
  std::memset(&ka, 0, sizeof(ka));
  ka.t = rep->dev; ka.b = b->dev; ka.now_ns = p->now_ns;
  ka.flags = (p->flags & ~(u32)CBH_FI_MASK) | CBH_FI_COMPACT | CBH_FI_PACKED_TAGS;   // (a compact launch: the cache's tags in the packed form)
  CrossDev x{};
  x.p_order = cs->p_order; x.r_order = cs->r_order;
  x.n = cs->n; x.r_begin = r_begin; x.n_tile = (u32)nt; x.words = (u32)W; x.side = cs->side;
  const TableDev& dev = rep->dev;
  const size_t lds = cbh_plan_lds(pl, dev.flags, dev.max_depth, dev.n_scopes, dev.K, ka.b.n_columns, dev.inline_cols, dev.n_dr, false, CBH_W2_NA, true) + lds_pad();
  // one launch per group of four actions, each with the group's word and its own planes [4 g, 4 g + 4) of the block - and within it
  // one per group of four roles, in order: group 0 stores its ballots, every later one ORs into them what the earlier ones left open
  const u32 R = cross_role_groups(cs);
  for (u32 g = 0; g < cross_groups(cs); ++g) {
    x.act_word = cs->act_words[g];
    x.allow = cs->planes + (size_t)4 * g * W; x.flagged = flagged ? cs->planes + per + (size_t)4 * g * W : nullptr;
    for (u32 rg = 0; rg < R; ++rg) {
      x.rg = cs->d_rg ? cs->d_rg + rg : nullptr;   // (null in a set without role groups: exactly the launch such a set always had)
      hipLaunchKernelGGL(fn, dim3((u32)((nt + pl.threads - 1) / pl.threads)), dim3(pl.threads), lds, s, ka, (const KernelArgs*)nullptr, x);   // (the arguments in memory are the evaluator call's: no _x kernel has one)
    }
  }
  HIPCHK(hipGetLastError());
  for (int which = 0; which < (flagged ? 2 : 1); ++which) {
    uint64_t* dst = which ? flagged : allow; const u64* src = cs->planes + (size_t)which * per;
    if (words_per_plane == W) HIPCHK(hipMemcpyAsync(dst, src, per * 8, hipMemcpyDeviceToHost, s));
    else for (u32 k = 0; k < cs->a; ++k) HIPCHK(hipMemcpyAsync(dst + (size_t)k * words_per_plane, src + (size_t)k * W, W * 8, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}
extern "C" int cbh_cross_check(cbh_table* t, cbh_cross_set* cs, const cbh_params* p, uint32_t r_begin, uint32_t r_end, uint64_t* allow, uint64_t* flagged, size_t words_per_plane) {
  try { return cross_set_check(t, cs, p, r_begin, r_end, allow, flagged, words_per_plane); } catch (...) { return fail("out of memory"); }
}
extern "C" const char* cbh_cross_describe(cbh_table* t, cbh_cross_set* cs, const cbh_params* p) {
  static thread_local std::string s;
  if (!t || !cs || !p) return "";
  try {
    CbhPlan pl;
    if (cs->b->table != t) s = "none: the set was uploaded for a different table";
    else if (!cross_kernel_for(cs, p->flags, pl)) s = "none: these flags choose a plan without a direct form";
    else {
      char m[160], g[40] = "", r[40] = "";
      if (cross_groups(cs) > 1) snprintf(g, sizeof g, ", %u action groups", cross_groups(cs));
      if (cross_role_groups(cs) > 1) snprintf(r, sizeof r, ", %u role groups", cross_role_groups(cs));
      snprintf(m, sizeof m, "[direct cross, %u + %u rows, narrow columns 0x%x%s%s]", cs->n, cs->m, cs->b->dev.compact_info & CBH_CI_NARROW_MASK, g, r);
      s = std::string(cbh_flat_cross_name(pl.kernel)) + m;
    }
  } catch (...) { return ""; }
  return s.c_str();
}
extern "C" void cbh_cross_release(cbh_cross_set* cs) {
  if (!cs) return;
  cbh_batch_release(cs->b);
  delete cs;
}

// Chosen pairs of a set - the flagged ones, as a rule - as an ordinary resident batch built on the device from the set's own rows
// (cbh_cross_gather_kernel), by cross_upload's steps: the same constructor, counts, buffers and compact form, and the shape a
// host-built batch of those requests would get.  Roles, heap and strings are copied device to device: the batch outlives the set.
template <typename T>
static int dcopy(cbh_device_batch* b, const T*& dst, const T* src, size_t n, hipStream_t s) {
  T* p = nullptr; dst = nullptr;
  if (dalloc(b, p, n) != 0) return -1;
  if (n) HIPCHK(hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyDeviceToDevice, s));
  dst = p;
  return 0;
}
static int cross_pairs_upload(cbh_table* t, cbh_cross_set* cs, const uint32_t* pair_p, const uint32_t* pair_r, uint32_t n_pairs, cbh_device_batch** out) {
  if (out) *out = nullptr;
  if (!t || !cs || !pair_p || !pair_r || !out) return fail("null argument");
  cbh_device_batch* hb = cs->b;
  if (hb->table != t) return fail("the set was uploaded for a different table");
  if (!n_pairs) return fail("cbh_cross_pairs_upload: n_pairs must be at least 1");
  const u64 NP = n_pairs, A = cs->a;
  if (NP * A >= (1ull << 32)) return fail("cbh_cross_pairs_upload: the batch has 2^32 tuples or more: take fewer pairs");
  u32 maxr = 0;
  for (u32 q = 0; q < n_pairs; ++q) {   // before anything is launched: the kernel indexes the set's rows with these
    if (pair_p[q] >= cs->n || pair_r[q] >= cs->m) return fail("cbh_cross_pairs_upload: a pair's index is outside the set (pair_p < n_principals, pair_r < n_resources, device order)");
    maxr = std::max(maxr, (u32)cs->p_roles[pair_p[q]]);
  }
  Replica* rep = hb->rep;
  HIPCHK(hipSetDevice(rep->device));
  cbh_device_batch* b = batch_new(t, rep, false);
  if (!b) return -1;
  const BatchDev& hd = hb->dev;
  const u32 ncol = hd.n_columns;
  b->max_actions = (u32)A; b->max_roles = maxr; b->plain_tags = cs->plain;   // (every row of a set holds plain values)
  // where the requests wider than the walk's base shape lie (validate_batch's wide_lo / wide_hi): every pair of a set of more than
  // CBH_W2_NA actions, else the pairs whose principal has more than CBH_W2_NR roles (a set with role groups)
  b->wide_lo = 0; b->wide_hi = A > CBH_W2_NA ? n_pairs : 0;
  if (A <= CBH_W2_NA && maxr > CBH_W2_NR) {
    u32 wlo = n_pairs, whi = 0;
    for (u32 q = 0; q < n_pairs; ++q) if (cs->p_roles[pair_p[q]] > CBH_W2_NR) { if (wlo == n_pairs) wlo = q; whi = q + 1; }
    b->wide_lo = wlo; b->wide_hi = whi;
  }
  BatchDev& d = b->dev;
  batch_set_counts(b, n_pairs, (u32)(NP * A), hd.n_roles, ncol, hd.n_strings, hd.heap_len);
  hipStream_t s = b->stream;
  CrossGatherArgs ga{};
  ga.h_req = hd.req_u32; ga.h_tag = hd.col_tag; ga.h_val = hd.col_val; ga.p_order = cs->p_order; ga.r_order = cs->r_order; ga.col_side = cs->d_side;
  ga.p_role_cnt = cs->d_role_cnt;   // (a set with role groups: the true counts; else null - the request words')
  ga.n = cs->n; ga.nh = cs->n + cs->m; ga.n_pairs = n_pairs; ga.a = (u32)A; ga.n_columns = ncol;
  CrossArgs ca{};   // (for cbh_cross_actions_kernel: a product of n_pairs x 1)
  ca.n = n_pairs; ca.m = 1; ca.a = (u32)A; ca.action_ids = cs->d_act;
  int rc = 0;
  rc |= up(b, ga.pair_p, pair_p, (size_t)n_pairs, s);
  rc |= up(b, ga.pair_r, pair_r, (size_t)n_pairs, s);
  rc |= dcopy(b, d.roles, hd.roles, hd.n_roles, s);
  rc |= dcopy(b, d.heap_tag, hd.heap_tag, hd.heap_len, s);
  rc |= dcopy(b, d.heap_val, hd.heap_val, hd.heap_len, s);
  rc |= dcopy(b, d.str_off, hd.str_off, hd.n_strings ? (size_t)hd.n_strings + 1 : 0, s);
  rc |= dcopy(b, d.str_bytes, hd.str_bytes, cs->str_bytes_len, s);
  rc |= dcopy(b, d.str_flags, hd.str_flags, hd.n_strings, s);
  d.tuple_req = nullptr;
  rc |= dalloc(b, ga.req, (size_t)CBH_RQ_NFIELDS * NP);
  rc |= dalloc(b, ga.tag, (size_t)ncol * NP);
  rc |= dalloc(b, ga.val, (size_t)ncol * NP);
  rc |= dalloc(b, ca.tuple_action, (size_t)(NP * A));
  rc |= batch_device_buffers(b, (size_t)3 * d.n_strings);
  if (rc != 0) { cbh_batch_release(b); return -1; }
  d.req_u32 = ga.req; d.col_tag = ga.tag; d.col_val = ga.val; d.tuple_action = ca.tuple_action;
  if (d.n_strings && hipMemsetAsync(d.gbits, 0, (size_t)3 * d.n_strings * sizeof(u64), s) != hipSuccess) { cbh_batch_release(b); return fail("upload failed"); }
  hipLaunchKernelGGL(cbh_cross_gather_kernel, dim3((n_pairs + 255u) / 256u), dim3(256), 0, s, ga);
  hipLaunchKernelGGL(cbh_cross_actions_kernel, dim3((u32)(((NP * A + 3u) / 4u + 255u) / 256u)), dim3(256), 0, s, ca);
  if (hipGetLastError() != hipSuccess) { cbh_batch_release(b); return fail("cbh_cross_pairs_upload: the gather failed to launch"); }
  // (the pair lists are the caller's pageable memory: their copies must have left before the call returns - batch_compact synchronises, or the wait below)
  if (batch_compact(b, s) != 0) { cbh_batch_release(b); return -1; }
  if (hipStreamSynchronize(s) != hipSuccess) { cbh_batch_release(b); return fail("upload failed"); }
  *out = b;
  return 0;
}
extern "C" int cbh_cross_pairs_upload(cbh_table* t, cbh_cross_set* set, const uint32_t* pair_p, const uint32_t* pair_r, uint32_t n_pairs, cbh_device_batch** out) {
  try { return cross_pairs_upload(t, set, pair_p, pair_r, n_pairs, out); } catch (...) { return fail("out of memory"); }
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
