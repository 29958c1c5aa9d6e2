// Host side of libcerbos_hip.so, part 3 of 5 (included by cbh_engine.hip, host pass only, behind cbh_host_resident.h, whose plan_for, batch constructor and
// makers' tail it uses): the cross road - N x M x A from N + M halves, as a materialised product, as a direct set - checked tile by tile or reviewed range by range -, as a batch of chosen pairs of a set.
#pragma once

// ---- cross-product batches: N + M halves up, the N x M product built in device memory (cbh_cross.h) ------------------------
// The batch's shape comes from the halves, looking only at the rows the product uses, so that the product gets the plan a
// host-built batch of the same requests gets (validate_batch's answers for that batch, without the batch).
// (`bounded`: the product is materialised, so N * M and N * M * A must stay below 2^32 - the direct road, cbh_cross_upload, has no such bound)
// (`plan_a`, set by the caller: the action count the plan is made for where it is not A - the direct road decides A > 4 four at a time)
// (`group_roles`, set by the caller: the plan is made for at most four roles - the direct road decides more four at a time)
struct CrossShape { std::vector<u8> side; PlanShape shape; u32 plan_a = 0; bool group_roles = false; };   // `shape`: the PRODUCT's
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
  // plain tags: BatchShape::plain_tags over the rows the product uses, for the shape the plan is made for
  const bool hit = plain_tags_select(t, cs.plan_a ? cs.plan_a : (u32)A, cs.group_roles ? std::min(maxr, 4u) : maxr) &&
                   sens_tag_hit(t, h->col_tag, ncol, NH, [&](u32 c) { return side[c] ? TagRows{(size_t)N, (size_t)M} : TagRows{0, (size_t)N}; });
  cs.shape = PlanShape{(u32)A, maxr, wide_lo, wide_hi, !flat_any_forced() && !hit};
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
  Replica* rep = t->reps[device_index];
  HIPCHK(hipSetDevice(rep->device));
  BatchOwner b(batch_new(t, rep, false), cbh_batch_release);
  if (!b) return -1;
  b->shape = cs.shape;
  BatchDev& d = b->dev;
  batch_set_counts(b.get(), (u32)NM, (u32)NT, h->n_roles, ncol, h->n_strings, h->heap_len);
  hipStream_t s = b->stream;
  CrossArgs ca{};
  ca.n = (u32)N; ca.m = (u32)M; ca.a = (u32)A; ca.n_columns = ncol;
  int rc = 0;
  // the halves, the orders, the sides and the action ids (they stay with the batch until it is released: N + M rows)
  rc |= up(b.get(), ca.h_req, h->req_u32, (size_t)CBH_RQ_NFIELDS * NH, s);
  rc |= up(b.get(), ca.h_tag, h->col_tag, (size_t)ncol * NH, s);
  rc |= up(b.get(), ca.h_val, h->col_val, (size_t)ncol * NH, s);
  if (x->p_order) rc |= up(b.get(), ca.p_order, x->p_order, (size_t)N, s);
  if (x->r_order) rc |= up(b.get(), ca.r_order, x->r_order, (size_t)M, s);
  rc |= up(b.get(), ca.col_side, (const u8*)cs.side.data(), (size_t)ncol, s);
  rc |= up(b.get(), ca.action_ids, x->action_ids, (size_t)A, s);
  rc |= batch_shared_arrays(d, *h, h->str_bytes_len, [&](auto& dst, auto* src, size_t n) { return up(b.get(), dst, src, n, s); });
  // the product
  rc |= dalloc(b.get(), ca.req, (size_t)CBH_RQ_NFIELDS * NM);
  rc |= dalloc(b.get(), ca.tag, (size_t)ncol * NM);
  rc |= dalloc(b.get(), ca.val, (size_t)ncol * NM);
  rc |= dalloc(b.get(), ca.tuple_action, NT);
  d.req_u32 = ca.req; d.col_tag = ca.tag; d.col_val = ca.val; d.tuple_action = ca.tuple_action;
  // (`cs.side` is pageable memory of this frame: its copy must have left before the frame goes - batch_compact synchronises, or batch_finish's wait)
  return batch_finish(b, rc, out, [&] {
    hipLaunchKernelGGL(cbh_cross_expand_kernel, dim3((u32)((NM + 255u) / 256u)), dim3(256), 0, s, ca);
    hipLaunchKernelGGL(cbh_cross_actions_kernel, dim3((u32)(((NT + 3u) / 4u + 255u) / 256u)), dim3(256), 0, s, ca);
    if (hipGetLastError() != hipSuccess) return fail("cross-product expansion failed to launch");
    return batch_compact(b.get(), s);
  });
}
extern "C" int cbh_batch_upload_cross(cbh_table* t, uint32_t device_index, const cbh_batch* halves, const cbh_cross* x, cbh_device_batch** out) {
  try { return cross_upload(t, device_index, halves, x, out); } catch (...) { return fail("out of memory"); }
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
  CrossShape cx;
  cx.plan_a = std::min(x->n_actions, 4u);
  cx.group_roles = (accept & CBH_CX_ROLE_GROUPS) != 0;
  if (cross_validate(t, device_index, h, x, false, cx) != 0) return -1;
  const PlanShape& shape = cx.shape;
  Replica* rep = t->reps[device_index];
  const u32 N = x->n_principals, M = x->n_resources, A = x->n_actions;
  // no direct form: the caller takes cbh_batch_upload_cross, which gives the same answers
  if (!(rep->dev.flags & CBH_MF_FLAT)) { g_err = "cbh_cross_upload: no direct form - the table is not flat"; return 1; }
  if (rep->dev.n_dr && !(accept & CBH_CX_DERIVED_ROLES)) { g_err = "cbh_cross_upload: no direct form - the table has derived roles"; return 1; }
  if (A > 4 && !(accept & CBH_CX_ACTION_GROUPS)) { g_err = "cbh_cross_upload: no direct form - more than four actions"; return 1; }
  if (shape.max_roles > 4 && !(accept & CBH_CX_ROLE_GROUPS)) { g_err = "cbh_cross_upload: no direct form - a principal has more than four roles"; return 1; }
  if (shape.max_roles > CBH_CX_MAX_ROLES) { g_err = "cbh_cross_upload: no direct form - a principal has more than CBH_CX_MAX_ROLES (16) roles"; return 1; }
  if (!shape.plain_tags) { g_err = "cbh_cross_upload: no direct form - an attribute value needs the evaluator (int / uint / list / map in a sensitive column)"; return 1; }
  if (!compact_inputs_on()) { g_err = "cbh_cross_upload: no direct form - compact inputs are switched off"; return 1; }
  {   // the kernel the product would be planned (mask walk of a table that is not closed over the classified leaves: cbh_flat_cross_mode)
    const CbhPlan pl = plan_for(rep->dev, cx.plan_a, std::min(shape.max_roles, 4u), shape.plain_tags, 0);
    if (pl.kind != 1 || !cbh_flat_cross_variant(pl.kernel)) { g_err = "cbh_cross_upload: no direct form - the kernel planned for this table has no direct instantiation"; return 1; }
  }
  std::unique_ptr<cbh_cross_set, void (*)(cbh_cross_set*)> cs(new (std::nothrow) cbh_cross_set(), cbh_cross_release);   // (the set's batch goes with it)
  if (!cs) return fail("out of memory");
  cs->n = N; cs->m = M; cs->a = A; cs->maxr = shape.max_roles; cs->plain = shape.plain_tags; cs->str_bytes_len = h->str_bytes_len;
  for (u32 c = 0; c < h->n_columns && c < CBH_CACHE_COLS; ++c) if (cx.side[c]) cs->side |= 1u << c;
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
  if (A > 4 || shape.max_roles > 4) { req_copy.assign(h->req_u32, h->req_u32 + (size_t)CBH_RQ_NFIELDS * NH); hh.req_u32 = req_copy.data(); }
  if (shape.max_roles > 4) {
    u32* cnt = req_copy.data() + (size_t)CBH_RQ_ROLE_CNT * NH;
    for (size_t r = 0; r < N; ++r) cnt[r] = std::min(cnt[r], 4u);
  }
  if (A > 4) {
    u32* cnt = req_copy.data() + (size_t)CBH_RQ_ACT_CNT * NH;
    for (size_t r = 0; r < NH; ++r) if (cnt[r] > 4u && (u64)req_copy[(size_t)CBH_RQ_ACT_OFF * NH + r] + cnt[r] <= (u64)h->n_tuples) cnt[r] = 0;   // (a slice outside the batch stays, to be refused)
  }
  // the halves: an ordinary resident batch of N + M requests (validated as one: the scan and the pack read every row's role and
  // action slices) with its compact form
  if (batch_upload(t, device_index, &hh, &cs->b, true) != 0) return -1;
  cbh_device_batch* b = cs->b;
  b->shape = shape;   // the set's batch carries the PRODUCT's shape, not the halves' (the plan is made for min(A, 4) actions: cross_kernel_for)
  if (!b->compact) { g_err = "cbh_cross_upload: no direct form - a field of the halves does not fit the compact record (CBH_CI_MISFIT)"; return 1; }
  hipStream_t s = b->stream;
  u32* d_word = nullptr;
  const u32 G = cross_groups(cs.get());
  cs->act_words.assign(G, 0u);
  int rc = 0;
  if (x->p_order) rc |= up(b, cs->p_order, x->p_order, (size_t)N, s);
  if (x->r_order) rc |= up(b, cs->r_order, x->r_order, (size_t)M, s);
  rc |= up(b, cs->d_act, x->action_ids, (size_t)A, s);
  rc |= up(b, cs->d_side, (const u8*)cx.side.data(), (size_t)h->n_columns, s);   // (pageable memory of this frame: the wait below)
  rc |= dalloc(b, d_word, G);
  const u32 R = cross_role_groups(cs.get());
  u32* d_rw = nullptr; u32* d_all = nullptr;
  if (R > 1) {
    rc |= up(b, cs->d_role_cnt, h->req_u32 + (size_t)CBH_RQ_ROLE_CNT * NH, (size_t)N, s);   // (the caller's words: the true counts)
    rc |= dalloc(b, d_rw, (size_t)(R - 1) * N);
    rc |= dalloc(b, d_all, (size_t)N);
  }
  if (rc != 0) return -1;
  if (R > 1) {
    CrossRoleWordArgs ra{}; ra.role_off = b->dev.req_u32 + (size_t)CBH_RQ_ROLE_OFF * NH; ra.role_cnt = cs->d_role_cnt; ra.roles = b->dev.roles;
    ra.role_class = rep->dev.role_class; ra.words = d_rw; ra.all = d_all; ra.n = N; ra.groups = R; ra.K = rep->dev.K;
    hipLaunchKernelGGL(cbh_cross_role_word_kernel, dim3((N + 255u) / 256u), dim3(256), 0, s, ra);
    cs->role_words = d_rw; cs->rc_all = d_all;
    std::vector<CrossRoleGroup> recs(R);   // (pageable memory of this frame: the wait below)
    const u32 open_from = cross_open_from(rep->dev, cs.get());
    for (u32 g = 0; g < R; ++g) recs[g] = CrossRoleGroup{g ? d_rw + (size_t)(g - 1u) * N : nullptr, d_all, cs->d_role_cnt, g, open_from};
    if (up(b, cs->d_rg, recs.data(), (size_t)R, s) != 0 || hipStreamSynchronize(s) != hipSuccess) { (void)hipGetLastError(); return fail("cbh_cross_upload: upload failed"); }
  }
  CrossActWordArgs wa{}; wa.action_ids = cs->d_act; wa.action_class = rep->dev.action_class; wa.out = d_word; wa.a = A; wa.K = rep->dev.K;
  hipLaunchKernelGGL(cbh_cross_act_word_kernel, dim3(1), dim3(64), 0, s, wa);
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(cs->act_words.data(), d_word, (size_t)G * 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
    (void)hipGetLastError(); return fail("cbh_cross_upload: upload failed");
  }
  *out = cs.release();
  return 0;
}
extern "C" int cbh_cross_upload_ex(cbh_table* t, uint32_t device_index, const cbh_batch* halves, const cbh_cross* x, uint32_t accept, cbh_cross_set** out) {
  try { return cross_set_upload(t, device_index, halves, x, accept, out); } catch (...) { return fail("out of memory"); }
}
extern "C" int cbh_cross_upload(cbh_table* t, uint32_t device_index, const cbh_batch* halves, const cbh_cross* x, cbh_cross_set** out) {
  return cbh_cross_upload_ex(t, device_index, halves, x, 0, out);
}
// What cbh_cross_check and cbh_cross_review refuse alike, under the caller's name: null handles, a set of another table, a range
// that is empty or ends behind the set's resources.
static int cross_call_args(cbh_table* t, cbh_cross_set* cs, const cbh_params* p, uint32_t r_begin, uint32_t r_end, const char* who) {
  if (!t || !cs || !p) return fail("null argument");
  if (cs->b->table != t) return fail("the set was uploaded for a different table");
  if (r_begin >= r_end || r_end > cs->m) return fail(std::string(who) + ": [r_begin, r_end) must be a non-empty range of the set's resources");
  return 0;
}
// The set's plane block holds `need` words (called with the replica's lock held): a larger tile than any before gets a new block,
// and the old one goes back to the replica's pool (every check and review ends with a wait for its copies, so nothing of the stream
// still reads it).
static int cross_planes_reserve(cbh_cross_set* cs, size_t need) {
  if (need <= cs->plane_cap) return 0;
  cbh_device_batch* b = cs->b;
  Replica* rep = b->rep;
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
  return 0;
}
// The launches that decide the tile [r_begin, r_end) into the set's plane block, [allow | flagged][a][W], on the set's stream: the
// one loop of cbh_cross_check and cbh_cross_review (the block holds the tile: cross_planes_reserve).
static int cross_launch_tile(cbh_cross_set* cs, const cbh_params* p, cbh_cross_kernel_fn fn, const CbhPlan& pl, uint32_t r_begin, uint32_t r_end, bool flagged) {
  cbh_device_batch* b = cs->b;
  Replica* rep = b->rep;
  hipStream_t s = b->stream;
  const u64 nt = (u64)cs->n * (r_end - r_begin);
  const size_t W = (size_t)((nt + 63) / 64), per = (size_t)cs->a * W;
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
  return 0;
}
static int cross_set_check(cbh_table* t, cbh_cross_set* cs, const cbh_params* p, uint32_t r_begin, uint32_t r_end, uint64_t* allow, uint64_t* flagged, size_t words_per_plane) {
  if (!allow) return fail("null argument");
  if (cross_call_args(t, cs, p, r_begin, r_end, "cbh_cross_check") != 0) return -1;
  cbh_device_batch* b = cs->b;
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
  const size_t per = (size_t)cs->a * W;
  if (cross_planes_reserve(cs, per * (flagged ? 2 : 1)) != 0) return -1;
  if (cross_launch_tile(cs, p, fn, pl, r_begin, r_end, flagged != nullptr) != 0) return -1;
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

// ---- the review of a set: a range of resources decided tile by tile, every tile's planes reduced on the device (cbh_cross.h) ----
// The launches per tile are cbh_cross_check's (cross_launch_tile) into the set's own plane block, which is reused from tile to tile;
// behind them the review kernels read the planes and add to counters that live for the call.  No plane is copied to the host.
// Tile rule: the caller's tile_resources, else the largest count of resources whose planes - [kinds][A][words], kinds = 2 where
// anything flagged is asked for - fit CBH_CROSS_REVIEW_PLANE_BYTES; in either case fewer than 2^32 requests, and at least one resource.
static const size_t CBH_CROSS_REVIEW_PLANE_BYTES = (size_t)256 << 20;
static const u32 CBH_CROSS_REVIEW_MAX_GRID = 8192;   // workgroups of a rows / columns launch: the kernels stride over the rest
// The device blocks a review takes from the replica's pool, behind `mark` in the set's batch: back to the pool when the call ends,
// however it ends - after a wait for whatever of the stream may still use them.
struct CrossScratch {
  cbh_device_batch* b; size_t mark; bool idle;
  ~CrossScratch() {
    if (!idle && hipStreamSynchronize(b->stream) != hipSuccess) (void)hipGetLastError();
    std::lock_guard<std::mutex> pl(b->rep->pool_mu);
    while (b->allocs.size() > mark) { b->rep->pool_free.push_back(b->allocs.back()); b->allocs.pop_back(); }
  }
};
static u32 bit_length(u64 v) { u32 n = 0; while (v) { ++n; v >>= 1; } return n; }
static int cross_set_review(cbh_table* t, cbh_cross_set* cs, const cbh_params* p, uint32_t r_begin, uint32_t r_end, struct cbh_cross_review* rv) {
  if (!rv) return fail("null argument");
  if (cross_call_args(t, cs, p, r_begin, r_end, "cbh_cross_review") != 0) return -1;
  const u32 N = cs->n, A = cs->a, mr = r_end - r_begin;
  if (rv->pairs != 0 && rv->pairs != CBH_RV_PAIRS_FLAGGED && rv->pairs != CBH_RV_PAIRS_ALLOWED) return fail("cbh_cross_review: `pairs` must be 0, CBH_RV_PAIRS_FLAGGED or CBH_RV_PAIRS_ALLOWED");
  if (A < 64u && (rv->pair_actions >> A) != 0) return fail("cbh_cross_review: `pair_actions` has a bit of an action the set does not have");
  if (rv->pairs && rv->pair_cap && (!rv->pair_p || !rv->pair_r || !rv->pair_mask)) return fail("cbh_cross_review: pair_cap entries are asked for, and pair_p, pair_r or pair_mask is NULL");
  CbhPlan pl;
  const cbh_cross_kernel_fn fn = cross_kernel_for(cs, p->flags, pl);
  if (!fn) { g_err = "cbh_cross_review: these flags choose a plan without a direct form"; return 1; }
  const bool want_p = rv->allow_by_principal || rv->flagged_by_principal;
  const bool want_r = rv->allow_by_resource || rv->flagged_by_resource || rv->totals;   // (the totals are the sums of the per-resource counts)
  const bool want_f = rv->flagged_by_principal || rv->flagged_by_resource || rv->totals || rv->pairs == CBH_RV_PAIRS_FLAGGED;
  const u32 kinds = want_f ? 2u : 1u;
  const size_t n_planes = (size_t)kinds * A;
  // the tile
  u64 mt = rv->tile_resources;
  if (!mt) mt = (u64)(CBH_CROSS_REVIEW_PLANE_BYTES / 8 / n_planes) * 64u / N;   // (N * mt bits in that many words)
  mt = std::min(std::max<u64>(mt, 1), std::min<u64>(((1ull << 32) - 1u) / N, mr));
  const size_t W_max = (size_t)(((u64)N * mt + 63) / 64);
  const u64 sel = rv->pair_actions ? rv->pair_actions : (A < 64u ? (1ull << A) - 1ull : ~0ull);
  cbh_device_batch* b = cs->b;
  Replica* rep = b->rep;
  std::lock_guard<std::mutex> lk(rep->mu);
  HIPCHK(hipSetDevice(rep->device));
  hipStream_t s = b->stream;
  if (cross_planes_reserve(cs, n_planes * W_max) != 0) return -1;
  CrossScratch scratch{b, b->allocs.size(), false};
  u32* d_by_p = nullptr; u32* d_by_r = nullptr; u64* d_tot = nullptr;
  u32* d_wavesum = nullptr; u64* d_state = nullptr; u32* d_pp = nullptr; u32* d_pr = nullptr; u64* d_pm = nullptr;
  const u64 cap = rv->pairs ? std::min<u64>(rv->pair_cap, (u64)N * mr) : 0;
  if (want_p) {   // accumulated over the tiles: zeroed on the stream
    if (dalloc(b, d_by_p, n_planes * N) != 0) return -1;
    HIPCHK(hipMemsetAsync(d_by_p, 0, n_planes * N * 4, s));
  }
  if (want_r && dalloc(b, d_by_r, n_planes * mr) != 0) return -1;   // (every count is written once, by its tile)
  if (rv->totals && dalloc(b, d_tot, (size_t)2 * A) != 0) return -1;
  if (rv->pairs) {
    if (dalloc(b, d_wavesum, (W_max + 63) / 64) != 0 || dalloc(b, d_state, 2) != 0) return -1;
    HIPCHK(hipMemsetAsync(d_state, 0, 16, s));
    if (cap && (dalloc(b, d_pp, (size_t)cap) != 0 || dalloc(b, d_pr, (size_t)cap) != 0 || dalloc(b, d_pm, (size_t)cap) != 0)) return -1;
  }
  for (u64 lo = r_begin; lo < r_end; lo += mt) {
    const u32 hi = (u32)std::min<u64>(lo + mt, r_end), m = hi - (u32)lo;
    if (cross_launch_tile(cs, p, fn, pl, (u32)lo, hi, want_f) != 0) return -1;
    const u32 W = (u32)(((u64)N * m + 63) / 64);
    CrossReviewArgs ra{};
    ra.planes = cs->planes; ra.by_r = d_by_r; ra.by_p = d_by_p;
    ra.n = N; ra.mt = m; ra.a = A; ra.kinds = kinds; ra.words = W; ra.mr = mr; ra.j0 = (u32)lo - r_begin;
    if (want_r) {
      // as many lanes to a resource as it has words, up to a wave; a lane counts at most the bits of its share of the words, and of the resource
      const u32 wpr = (N + 63u) / 64u;
      ra.g = 1; while (ra.g * 2u <= std::min(wpr, 64u)) ra.g *= 2u;
      ra.bits = bit_length(std::min<u64>(N, 64ull * ((wpr + 1u + ra.g - 1u) / ra.g)));
      const u64 blocks = ((u64)n_planes * m + 256u / ra.g - 1u) / (256u / ra.g);
      ra.grid = (u32)std::min<u64>(blocks, CBH_CROSS_REVIEW_MAX_GRID);
      hipLaunchKernelGGL(cbh_cross_review_rows_kernel, dim3(ra.grid), dim3(256), 0, s, ra);
    }
    if (want_p) {
      // strips long enough that a destination gets few atomics, short enough that the launch has some 32 K waves; 16 .. 256 resources
      const u64 per_strip = (u64)n_planes * ((N + 63u) / 64u);
      const u32 strips_wanted = (u32)std::max<u64>(1, 32768u / per_strip);
      ra.strip = std::min(std::max((m + strips_wanted - 1u) / strips_wanted, 16u), 256u);
      const u64 blocks = (per_strip * ((m + ra.strip - 1u) / ra.strip) + 3u) / 4u;
      ra.grid = (u32)std::min<u64>(blocks, CBH_CROSS_REVIEW_MAX_GRID);
      hipLaunchKernelGGL(cbh_cross_review_cols_kernel, dim3(ra.grid), dim3(256), 0, s, ra);
    }
    if (rv->pairs) {
      CrossPairArgs pa{};
      pa.planes = cs->planes + (rv->pairs == CBH_RV_PAIRS_FLAGGED ? (size_t)A * W : 0);
      pa.wavesum = d_wavesum; pa.state = d_state; pa.pair_p = d_pp; pa.pair_r = d_pr; pa.pair_mask = d_pm;
      pa.sel = sel; pa.cap = cap; pa.n = N; pa.a = A; pa.words = W; pa.r0 = (u32)lo;
      hipLaunchKernelGGL(cbh_cross_review_pair_count_kernel, dim3((W + 255u) / 256u), dim3(256), 0, s, pa);
      hipLaunchKernelGGL(cbh_cross_review_pair_scan_kernel, dim3(1), dim3(64), 0, s, pa);
      if (cap) hipLaunchKernelGGL(cbh_cross_review_pair_scatter_kernel, dim3((W + 255u) / 256u), dim3(256), 0, s, pa);
    }
    HIPCHK(hipGetLastError());
  }
  if (rv->totals) {
    CrossTotalsArgs ta{d_by_r, d_tot, mr, bit_length((u64)((mr + 63u) / 64u) * N)};
    hipLaunchKernelGGL(cbh_cross_review_totals_kernel, dim3(2u * A), dim3(64), 0, s, ta);
    HIPCHK(hipGetLastError());
  }
  // one copy per wanted output, one wait (and, where a list is wanted, its entries - as many as there are - and a second wait)
  const size_t by_p = (size_t)A * N * 4, by_r = (size_t)A * mr * 4;
  if (rv->allow_by_principal) HIPCHK(hipMemcpyAsync(rv->allow_by_principal, d_by_p, by_p, hipMemcpyDeviceToHost, s));
  if (rv->flagged_by_principal) HIPCHK(hipMemcpyAsync(rv->flagged_by_principal, d_by_p + (size_t)A * N, by_p, hipMemcpyDeviceToHost, s));
  if (rv->allow_by_resource) HIPCHK(hipMemcpyAsync(rv->allow_by_resource, d_by_r, by_r, hipMemcpyDeviceToHost, s));
  if (rv->flagged_by_resource) HIPCHK(hipMemcpyAsync(rv->flagged_by_resource, d_by_r + (size_t)A * mr, by_r, hipMemcpyDeviceToHost, s));
  if (rv->totals) HIPCHK(hipMemcpyAsync(rv->totals, d_tot, (size_t)2 * A * 8, hipMemcpyDeviceToHost, s));
  u64 n_pairs = 0;
  if (rv->pairs) HIPCHK(hipMemcpyAsync(&n_pairs, d_state, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const size_t n_out = (size_t)std::min(n_pairs, cap);
  if (n_out) {
    HIPCHK(hipMemcpyAsync(rv->pair_p, d_pp, n_out * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(rv->pair_r, d_pr, n_out * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(rv->pair_mask, d_pm, n_out * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  scratch.idle = true;
  rv->n_pairs = n_pairs;
  if (n_pairs > rv->pair_cap) { g_err = "cbh_cross_review: pair_cap is smaller than the number of pairs (n_pairs says how many)"; return 2; }
  return 0;
}
extern "C" int cbh_cross_review(cbh_table* t, cbh_cross_set* cs, const cbh_params* p, uint32_t r_begin, uint32_t r_end, struct cbh_cross_review* rv) {
  try { return cross_set_review(t, cs, p, r_begin, r_end, rv); } catch (...) { return fail("out of memory"); }
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
  // where the requests wider than the walk's base shape lie (validate_batch's wide_lo / wide_hi): every pair of a set of more than
  // CBH_W2_NA actions, else the pairs whose principal has more than CBH_W2_NR roles (a set with role groups)
  u32 maxr = 0, wide_lo = 0, wide_hi = A > CBH_W2_NA ? n_pairs : 0;
  for (u32 q = 0; q < n_pairs; ++q) {   // before anything is launched: the kernel indexes the set's rows with these
    if (pair_p[q] >= cs->n || pair_r[q] >= cs->m) return fail("cbh_cross_pairs_upload: a pair's index is outside the set (pair_p < n_principals, pair_r < n_resources, device order)");
    maxr = std::max(maxr, (u32)cs->p_roles[pair_p[q]]);
    if (A <= CBH_W2_NA && cs->p_roles[pair_p[q]] > CBH_W2_NR) { if (!wide_hi) wide_lo = q; wide_hi = q + 1; }
  }
  Replica* rep = hb->rep;
  HIPCHK(hipSetDevice(rep->device));
  BatchOwner b(batch_new(t, rep, false), cbh_batch_release);
  if (!b) return -1;
  const BatchDev& hd = hb->dev;
  const u32 ncol = hd.n_columns;
  b->shape = PlanShape{(u32)A, maxr, wide_lo, wide_hi, cs->plain};   // (every row of a set holds plain values)
  BatchDev& d = b->dev;
  batch_set_counts(b.get(), n_pairs, (u32)(NP * A), hd.n_roles, ncol, hd.n_strings, hd.heap_len);
  hipStream_t s = b->stream;
  CrossGatherArgs ga{};
  ga.h_req = hd.req_u32; ga.h_tag = hd.col_tag; ga.h_val = hd.col_val; ga.p_order = cs->p_order; ga.r_order = cs->r_order; ga.col_side = cs->d_side;
  ga.p_role_cnt = cs->d_role_cnt;   // (a set with role groups: the true counts; else null - the request words')
  ga.n = cs->n; ga.nh = cs->n + cs->m; ga.n_pairs = n_pairs; ga.a = (u32)A; ga.n_columns = ncol;
  CrossArgs ca{};   // (for cbh_cross_actions_kernel: a product of n_pairs x 1)
  ca.n = n_pairs; ca.m = 1; ca.a = (u32)A; ca.action_ids = cs->d_act;
  int rc = up(b.get(), ga.pair_p, pair_p, (size_t)n_pairs, s);
  rc |= up(b.get(), ga.pair_r, pair_r, (size_t)n_pairs, s);
  rc |= batch_shared_arrays(d, hd, cs->str_bytes_len, [&](auto& dst, auto* src, size_t n) { return dcopy(b.get(), dst, src, n, s); });
  rc |= dalloc(b.get(), ga.req, (size_t)CBH_RQ_NFIELDS * NP);
  rc |= dalloc(b.get(), ga.tag, (size_t)ncol * NP);
  rc |= dalloc(b.get(), ga.val, (size_t)ncol * NP);
  rc |= dalloc(b.get(), ca.tuple_action, (size_t)(NP * A));
  d.req_u32 = ga.req; d.col_tag = ga.tag; d.col_val = ga.val; d.tuple_action = ca.tuple_action;
  // (the pair lists are the caller's pageable memory: their copies must have left before the call returns - batch_compact synchronises, or batch_finish's wait)
  return batch_finish(b, rc, out, [&] {
    hipLaunchKernelGGL(cbh_cross_gather_kernel, dim3((n_pairs + 255u) / 256u), dim3(256), 0, s, ga);
    hipLaunchKernelGGL(cbh_cross_actions_kernel, dim3((u32)(((NP * A + 3u) / 4u + 255u) / 256u)), dim3(256), 0, s, ca);
    if (hipGetLastError() != hipSuccess) return fail("cbh_cross_pairs_upload: the gather failed to launch");
    return batch_compact(b.get(), s);
  });
}
extern "C" int cbh_cross_pairs_upload(cbh_table* t, cbh_cross_set* set, const uint32_t* pair_p, const uint32_t* pair_r, uint32_t n_pairs, cbh_device_batch** out) {
  try { return cross_pairs_upload(t, set, pair_p, pair_r, n_pairs, out); } catch (...) { return fail("out of memory"); }
}
