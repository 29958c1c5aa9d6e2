// Host side of libcerbos_hip.so, part 5 of 5 (included by cbh_engine.hip, host pass only): the one-shot path.
#pragma once

// ---- one-shot path: CheckResources round trip for a host batch ------------------------------------------
// All arrays of the batch go into ONE device block per device used, laid out for the whole batch; a device
// that decides the request range [lo, hi) receives only the slices of that range (the kernels address the
// whole-batch layout through BatchDev.req_lo / req_hi).
static OneShot* ctx_acquire(Replica* r) {
  std::unique_lock<std::mutex> lk(r->ctx_mu);
  for (;;) {
    if (!r->ctx_idle.empty()) { auto* c = r->ctx_idle.back(); r->ctx_idle.pop_back(); return c; }
    if (r->ctx_count < Replica::MAX_ONESHOT) {
      ++r->ctx_count;
      lk.unlock();
      auto* c = new (std::nothrow) OneShot();
      bool ok = c != nullptr;
      for (int i = 0; ok && i < N_STREAMS; ++i) ok = hipStreamCreateWithFlags(&c->s[i], hipStreamNonBlocking) == hipSuccess;
      ok = ok && hipEventCreateWithFlags(&c->ev_setup, hipEventDisableTiming) == hipSuccess;
      if (c) for (auto& e : c->ev_piece) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
      if (!ok) {
        if (c) { for (auto& s : c->s) if (s) (void)hipStreamDestroy(s); if (c->ev_setup) (void)hipEventDestroy(c->ev_setup); for (auto& e : c->ev_piece) if (e) (void)hipEventDestroy(e); delete c; c = nullptr; }
        lk.lock(); --r->ctx_count; r->ctx_cv.notify_one();
      }
      return c;
    }
    r->ctx_cv.wait(lk);
  }
}
struct CtxLease {
  Replica* r; OneShot* c;
  int used = N_STREAMS;   // streams the call has touched
  ~CtxLease() {
    if (!c) return;
    (void)hipSetDevice(r->device);
    for (int i = 0; i < used; ++i) (void)hipStreamSynchronize(c->s[i]);   // an error return must not leave copies from caller memory in flight
    { std::lock_guard<std::mutex> lk(r->ctx_mu); r->ctx_idle.push_back(c); }
    r->ctx_cv.notify_one();
  }
};
static int ctx_reserve(OneShot* c, size_t hbytes, size_t dbytes) {
  if (hbytes > c->h_cap) {
    if (c->h) { (void)hipHostFree(c->h); c->h = nullptr; c->h_cap = 0; }
    size_t cap = 1 << 16; while (cap < hbytes) cap <<= 1;
    HIPCHK(hipHostMalloc((void**)&c->h, cap, hipHostMallocDefault));
    c->h_cap = cap;
  }
  if (dbytes && dbytes > c->d_cap) {
    if (c->d) { (void)hipFree(c->d); c->d = nullptr; c->d_cap = 0; }
    size_t cap = 1 << 16; while (cap < dbytes) cap <<= 1;
    HIPCHK(hipMalloc((void**)&c->d, cap));
    c->d_cap = cap;
  }
  return 0;
}

static bool is_pinned(const void* p) {
  if (!p) return true;   // an absent array does not decide
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.type == hipMemoryTypeHost;
}

struct Seg { size_t off, bytes; const void* src; };
// The canonical order of a batch's arrays.  It is the order of the device block AND of a caller's "slab" (one
// page-locked block holding all arrays, cbh_batch_bind_slab): a slab crosses PCIe in ONE copy because the device
// block mirrors it byte for byte.  What a table may not need comes last - the raw request strings (req_u32 rows
// CBH_RQ_NCORE..), then the batch-local string pool - so that the one copy simply stops earlier.
struct InOffsets { size_t roles, act, ctag, cval, htag, hval, req, soff, sbytes, sflags, end; };
static InOffsets in_offsets(const cbh_batch* in) {
  InOffsets o; size_t cur = 0;
  const size_t NR = in->n_requests, NT = in->n_tuples, NS = in->n_strings;
  auto seg = [&](size_t bytes) { const size_t at = cur; cur += (bytes + 255) & ~(size_t)255; return at; };
  o.roles = seg((size_t)in->n_roles * 4); o.act = seg(NT * 4);
  o.ctag = seg((size_t)in->n_columns * NR + 4);   // + 4: a lane reads the aligned dword around its tag byte
  o.cval = seg((size_t)in->n_columns * NR * 8);
  o.htag = seg(in->heap_len); o.hval = seg((size_t)in->heap_len * 8);
  o.req = seg((size_t)CBH_RQ_NFIELDS * NR * 4);
  o.soff = seg(NS ? (NS + 1) * 4 : 0); o.sbytes = seg(in->str_bytes_len); o.sflags = seg(NS);
  o.end = cur;
  return o;
}
struct OutOffsets { size_t eff, status, pol, scope, edr, end; };
static OutOffsets out_offsets(size_t NT, size_t NR) {
  OutOffsets o; size_t cur = 0;
  auto seg = [&](size_t bytes) { const size_t at = cur; cur += (bytes + 255) & ~(size_t)255; return at; };
  o.eff = seg(NT); o.status = seg(NT); o.pol = seg(NT * 4); o.scope = seg(NT * 4); o.edr = seg(NR * 8);
  o.end = cur;
  return o;
}
extern "C" size_t cbh_batch_slab_bytes(const cbh_batch* counts) { return counts ? in_offsets(counts).end : 0; }
extern "C" void cbh_batch_bind_slab(cbh_batch* b, void* slab) {
  if (!b || !slab) return;
  const InOffsets o = in_offsets(b);
  uint8_t* p = static_cast<uint8_t*>(slab);
  b->roles = (const uint32_t*)(p + o.roles); b->tuple_req = nullptr; b->tuple_action = (const uint32_t*)(p + o.act);
  b->col_tag = p + o.ctag; b->col_val = (const uint64_t*)(p + o.cval); b->heap_tag = p + o.htag; b->heap_val = (const uint64_t*)(p + o.hval);
  b->req_u32 = (const uint32_t*)(p + o.req); b->str_off = (const uint32_t*)(p + o.soff); b->str_bytes = p + o.sbytes; b->str_flags = p + o.sflags;
}
extern "C" size_t cbh_result_slab_bytes(uint32_t n_tuples, uint32_t n_requests) { return out_offsets(n_tuples, n_requests).end; }
extern "C" void cbh_result_bind_slab(cbh_result* r, void* slab, uint32_t n_tuples, uint32_t n_requests) {
  if (!r || !slab) return;
  const OutOffsets o = out_offsets(n_tuples, n_requests);
  uint8_t* p = static_cast<uint8_t*>(slab);
  r->effect = p + o.eff; r->status = p + o.status; r->policy = (uint32_t*)(p + o.pol); r->scope = (uint32_t*)(p + o.scope); r->edr_mask = (uint64_t*)(p + o.edr);
}

struct Layout {
  Seg args, req, roles, act, ctag, cval, htag, hval, soff, sbytes, sflags, gbits, gres, dflag, eff, pol, scope, status, edr;
  size_t in_begin, in_end, out_begin, total;
};
static Layout make_layout(const cbh_batch* in, const cbh_table* t) {
  Layout L;
  const size_t NR = in->n_requests, NT = in->n_tuples, NS = in->n_strings;
  const InOffsets io = in_offsets(in);
  const size_t A = (sizeof(KernelArgs) + 255) & ~(size_t)255;
  L.args = Seg{0, sizeof(KernelArgs), nullptr};
  L.in_begin = A;
  L.roles = Seg{A + io.roles, (size_t)in->n_roles * 4, in->roles}; L.act = Seg{A + io.act, NT * 4, in->tuple_action};
  L.ctag = Seg{A + io.ctag, (size_t)in->n_columns * NR, in->col_tag}; L.cval = Seg{A + io.cval, (size_t)in->n_columns * NR * 8, in->col_val};
  L.htag = Seg{A + io.htag, in->heap_len, in->heap_tag}; L.hval = Seg{A + io.hval, (size_t)in->heap_len * 8, in->heap_val};
  L.req = Seg{A + io.req, (size_t)CBH_RQ_NFIELDS * NR * 4, in->req_u32};
  L.soff = Seg{A + io.soff, NS ? (NS + 1) * 4 : 0, in->str_off}; L.sbytes = Seg{A + io.sbytes, in->str_bytes_len, in->str_bytes};
  L.sflags = Seg{A + io.sflags, NS, in->str_flags};
  L.in_end = A + io.end;
  size_t cur = L.in_end;
  L.gbits = Seg{cur, 3 * NS * 8, nullptr}; cur += (L.gbits.bytes + 255) & ~(size_t)255;
  // results of the evaluation sites (cbh_walk2_pre_kernel -> cbh_walk2_kernel), sized for a batch that needs all of them
  const size_t gw = (t->meta[CBH_M_FLAGS] & CBH_MF_WALK2) ? w2_gwords(t->meta[CBH_M_GSLOTS_GENERIC], t->meta[CBH_M_GSLOTS_ALL], false) : 0;
  L.gres = Seg{cur, gw * NR * 8, nullptr}; cur += (L.gres.bytes + 255) & ~(size_t)255;
  // a byte per request for the flat kernels' action groups on a table with derived roles (FlatGroupDev.dflag).  Whatever the
  // batch's action counts: the layout is fixed before the O(n_requests) scan that finds them (cbh_check_batch starts a slab's upload first).
  const bool groups = (t->meta[CBH_M_FLAGS] & CBH_MF_FLAT) && !t->reps.empty() && t->reps[0]->dev.n_dr && flat_action_groups_on();
  L.dflag = Seg{cur, groups ? NR : 0, nullptr}; cur += (L.dflag.bytes + 255) & ~(size_t)255;
  L.out_begin = cur;
  const OutOffsets oo = out_offsets(NT, NR);
  L.eff = Seg{cur + oo.eff, NT, nullptr}; L.status = Seg{cur + oo.status, NT, nullptr}; L.pol = Seg{cur + oo.pol, NT * 4, nullptr};
  L.scope = Seg{cur + oo.scope, NT * 4, nullptr}; L.edr = Seg{cur + oo.edr, NR * 8, nullptr};
  L.total = cur + oo.end;
  return L;
}
// are the batch's arrays one slab in canonical order?  -> its base address, else nullptr
static const uint8_t* slab_base(const Layout& L) {
  const uint8_t* base = nullptr;
  for (const Seg* g : {&L.roles, &L.act, &L.ctag, &L.cval, &L.htag, &L.hval, &L.req, &L.soff, &L.sbytes, &L.sflags}) {
    if (!g->bytes) continue;
    const uint8_t* b = static_cast<const uint8_t*>(g->src) - (g->off - L.in_begin);
    if (!base) base = b; else if (b != base) return nullptr;
  }
  return base;
}
static void bind_args(KernelArgs& ka, const TableDev& tdev, const cbh_batch* in, const cbh_params* p, const Layout& L, uint8_t* base) {
  std::memset(&ka, 0, sizeof(ka));
  ka.t = tdev; ka.now_ns = p->now_ns; ka.flags = p->flags & ~(u32)CBH_FI_MASK;
  BatchDev& d = ka.b;
  d.n_requests = in->n_requests; d.n_tuples = in->n_tuples; d.n_roles = in->n_roles;
  d.n_columns = in->n_columns; d.n_strings = in->n_strings; d.heap_len = in->heap_len;
  d.req_lo = 0; d.req_hi = in->n_requests;
  d.req_u32 = (const u32*)(base + L.req.off); d.roles = (const u32*)(base + L.roles.off); d.tuple_req = nullptr;
  d.tuple_action = (const u32*)(base + L.act.off); d.col_tag = base + L.ctag.off; d.col_val = (const u64*)(base + L.cval.off);
  d.heap_tag = base + L.htag.off; d.heap_val = (const u64*)(base + L.hval.off); d.str_off = (const u32*)(base + L.soff.off);
  d.str_bytes = base + L.sbytes.off; d.str_flags = base + L.sflags.off; d.gbits = (u64*)(base + L.gbits.off);
  d.gres = L.gres.bytes ? (u64*)(base + L.gres.off) : nullptr; d.n_gwords = 0; d.n_gslots = 0;   // n_gwords: per launch (launch_plan)
  ka.o.effect = base + L.eff.off; ka.o.policy = (u32*)(base + L.pol.off); ka.o.scope = (u32*)(base + L.scope.off);
  ka.o.status = base + L.status.off; ka.o.edr = (u64*)(base + L.edr.off);
}
static void launch_resolve(const Replica* rep, const KernelArgs& ka, const Layout& L, hipStream_t s, int& rc) {
  const u32 maxw = nfa_maxw(rep->dev);
  if (!ka.b.n_strings) return;
  if (maxw) {
    const u32 grid = (ka.b.n_strings + CBH_BLOCK - 1) / CBH_BLOCK;
    hipLaunchKernelGGL(cbh_resolve_globs_kernel, dim3(grid), dim3(CBH_BLOCK), (size_t)(2 + 512) * maxw * sizeof(u64), s, rep->dev, ka.b);
  } else if (hipMemsetAsync(ka.b.gbits, 0, L.gbits.bytes, s) != hipSuccess) rc = -1;   // no automata: no string matches a glob
}
static void launch_check(const Replica* rep, KernelArgs ka, const KernelArgs* d_args, u32 lo, u32 hi, const BatchShape& sh, hipStream_t s, u8* dflag) {
  if (hi <= lo) return;
  launch_plan(plan_for(rep->dev, sh.max_actions, sh.max_roles, sh.plain_tags(), ka.flags), rep->dev, ka, d_args, lo, hi, sh.wide_lo, sh.wide_hi, 0, s, nullptr, nullptr, dflag);
}

// a small batch on one device: everything packed into the pinned staging block.  Two ways across PCIe:
//   copy      one H2D of the inputs, kernels on device memory, one D2H of the results (three queue operations);
//   zero-copy the kernels read the inputs from, and write the results to, the page-locked block itself (it is
//             mapped into the device's address space): a few KB per request wave over PCIe, ONE queue operation.
// Zero-copy wins while a batch is a handful of waves (the latency case); the choice is by input size.
static int run_small(cbh_table* t, Replica* rep, const cbh_batch* in, const cbh_params* p, cbh_result* out, const BatchShape& sh, const Layout& L) {
  HIPCHK(hipSetDevice(rep->device));
  CtxLease lease{rep, ctx_acquire(rep)};
  OneShot* c = lease.c;
  if (!c) return fail("could not create a launch context");
  static const size_t zc_limit = (size_t)env_long("CBH_ZEROCOPY_BYTES", 64 << 10);
  const bool zero_copy = L.in_end <= zc_limit;
  if (ctx_reserve(c, L.total, zero_copy ? 0 : L.total) != 0) return -1;
  hipStream_t s = c->s[0];
  lease.used = 1;
  const double t_0 = trace_on() ? now_us() : 0;
  uint8_t* base = c->d;
  if (zero_copy) HIPCHK(hipHostGetDevicePointer((void**)&base, c->h, 0));
  KernelArgs ka;
  bind_args(ka, rep->dev, in, p, L, base);
  std::memcpy(c->h + L.args.off, &ka, sizeof(ka));
  for (const Seg* g : {&L.req, &L.roles, &L.act, &L.ctag, &L.cval, &L.htag, &L.hval, &L.soff, &L.sbytes, &L.sflags})
    if (g->bytes) std::memcpy(c->h + g->off, g->src, g->bytes);
  int rc = 0;
  if (zero_copy) {
    if (in->n_strings && !nfa_maxw(rep->dev)) std::memset(c->h + L.gbits.off, 0, L.gbits.bytes);   // no automata: no string matches a glob
    else launch_resolve(rep, ka, L, s, rc);
  } else {
    HIPCHK(hipMemcpyAsync(c->d, c->h, L.in_end, hipMemcpyHostToDevice, s));
    launch_resolve(rep, ka, L, s, rc);
  }
  launch_check(rep, ka, (const KernelArgs*)(base + L.args.off), 0, in->n_requests, sh, s, L.dflag.bytes ? base + L.dflag.off : nullptr);
  HIPCHK(hipGetLastError());
  if (rc != 0) return fail("hipMemsetAsync failed");
  if (!zero_copy && L.total > L.out_begin) HIPCHK(hipMemcpyAsync(c->h + L.out_begin, c->d + L.out_begin, L.total - L.out_begin, hipMemcpyDeviceToHost, s));
  const double t_1 = trace_on() ? now_us() : 0;
  HIPCHK(stream_wait(s));
  if (trace_on()) std::fprintf(stderr, "[cbh] small zero_copy=%d in=%zu B enqueue=%.1f us wait=%.1f us\n", (int)zero_copy, L.in_end, t_1 - t_0, now_us() - t_1);
  struct Dst { const Seg* g; void* dst; };
  const Dst outs[5] = {{&L.eff, out->effect}, {&L.pol, out->policy}, {&L.scope, out->scope}, {&L.status, out->status}, {&L.edr, out->edr_mask}};
  for (const Dst& o : outs) if (o.dst && o.g->bytes) std::memcpy(o.dst, c->h + o.g->off, o.g->bytes);
  (void)t;
  return 0;
}

// the request range [lo, hi) of a large batch on one device
// the bytes of a slab that go up: it stops before the raw request strings / the string pool when the table reads neither
static size_t slab_upload_end(const Replica* rep, const Layout& L, size_t NR) {
  const bool reads_strings = (rep->dev.flags & CBH_MF_READS_REQUEST_STRINGS) != 0, need_bytes = (rep->dev.flags & CBH_MF_NEEDS_STRING_BYTES) != 0;
  return need_bytes ? L.in_end : L.req.off + (size_t)(reads_strings ? CBH_RQ_NFIELDS : CBH_RQ_NCORE) * NR * 4;
}
// One DMA engine does not fill the host link (a 29 MB slab went up at ~39 GB/s where the link gives 56): a large slab goes up
// in pieces on the context's streams - each stream's copies run on an engine of their own - and stream 0 waits for all.
static int slab_upload(OneShot* c, const Replica* rep, const Layout& L, const uint8_t* slab, size_t NR) {
  static const u32 slab_split = (u32)std::min<long>(std::max<long>(env_long("CBH_SLAB_SPLIT", 2), 1), N_STREAMS);
  uint8_t* base = c->d;
  const size_t up = slab_upload_end(rep, L, NR) - L.in_begin;
  const u32 pieces = up >= ((size_t)8 << 20) ? slab_split : 1u;
  if (pieces <= 1) { HIPCHK(hipMemcpyAsync(base + L.in_begin, slab, up, hipMemcpyHostToDevice, c->s[0])); return 0; }
  const size_t step = ((up / pieces) + 4095) & ~(size_t)4095;
  for (u32 i = 0; i < pieces; ++i) {
    const size_t o = (size_t)i * step, n = o >= up ? 0 : std::min(step, up - o);
    if (!n) break;
    HIPCHK(hipMemcpyAsync(base + L.in_begin + o, slab + o, n, hipMemcpyHostToDevice, c->s[i]));
    if (i) { HIPCHK(hipEventRecord(c->ev_piece[i], c->s[i])); HIPCHK(hipStreamWaitEvent(c->s[0], c->ev_piece[i], 0)); }
  }
  return 0;
}
// `pre`: a context the caller holds whose slab upload is already in flight (cbh_check_batch starts it before it validates)
static int run_range(cbh_table* t, Replica* rep, const cbh_batch* in, const cbh_params* p, cbh_result* out, const BatchShape& sh,
                     const Layout& L, u32 lo, u32 hi, bool pinned, u32 chunk_requests, OneShot* pre = nullptr) {
  HIPCHK(hipSetDevice(rep->device));
  CtxLease lease{rep, pre ? nullptr : ctx_acquire(rep)};
  OneShot* c = pre ? pre : lease.c;
  if (!c) return fail("could not create a launch context");
  const double t_0 = trace_on() ? now_us() : 0;
  if (!pre && ctx_reserve(c, 4096, L.total) != 0) return -1;
  const size_t NR = in->n_requests;
  const bool whole = lo == 0 && hi == NR;
  KernelArgs ka;
  uint8_t* base = c->d;
  bind_args(ka, rep->dev, in, p, L, base);
  std::memcpy(c->h, &ka, sizeof(ka));
  const KernelArgs* d_args = (const KernelArgs*)(base + L.args.off);
  const u32* act_off = in->req_u32 + (size_t)CBH_RQ_ACT_OFF * NR; const u32* act_cnt = in->req_u32 + (size_t)CBH_RQ_ACT_CNT * NR;
  // tuples of the requests [a, b), a < b (ACT_OFF ascends whenever a batch is split; a batch in any other
  // order is only ever handled whole)
  auto tuples_of = [&](u32 a, u32 b, size_t& tb, size_t& te) {
    if (!sh.ascending) { tb = 0; te = in->n_tuples; return; }
    tb = act_off[a]; te = (size_t)act_off[b - 1] + act_cnt[b - 1];
  };
  const bool reads_strings = (rep->dev.flags & CBH_MF_READS_REQUEST_STRINGS) != 0;

  const bool need_bytes = (rep->dev.flags & CBH_MF_NEEDS_STRING_BYTES) != 0;
  hipStream_t s0 = c->s[0];
  int rc = 0;

  // ---- a slab (cbh_batch_bind_slab) in page-locked memory, decided whole on this device: ONE copy up - it stops
  // before the raw request strings / the string pool when the table reads neither -, the kernels, and the
  // results down in as few copies as the caller's result arrays are contiguous (one for a result slab)
  const uint8_t* slab = (whole && pinned) ? slab_base(L) : nullptr;
  if (slab) {
    const size_t end = slab_upload_end(rep, L, NR);
    HIPCHK(hipMemcpyAsync(base, c->h, sizeof(ka), hipMemcpyHostToDevice, s0));
    if (!pre && slab_upload(c, rep, L, slab, NR) != 0) return -1;
    launch_resolve(rep, ka, L, s0, rc);
    if (rc != 0) return fail("hipMemsetAsync failed");
    launch_check(rep, ka, d_args, 0, (u32)NR, sh, s0, L.dflag.bytes ? base + L.dflag.off : nullptr);
    HIPCHK(hipGetLastError());
    struct Run { size_t off, bytes; uint8_t* dst; };
    Run run{0, 0, nullptr};
    const Seg* segs[5] = {&L.eff, &L.status, &L.pol, &L.scope, &L.edr};
    void* dsts[5] = {out->effect, out->status, out->policy, out->scope, out->edr_mask};
    for (int i = 0; i < 5; ++i) {
      if (!dsts[i] || !segs[i]->bytes) continue;
      uint8_t* d = static_cast<uint8_t*>(dsts[i]);
      if (run.dst && d == run.dst + (segs[i]->off - run.off)) { run.bytes = segs[i]->off + segs[i]->bytes - run.off; continue; }   // contiguous with the run: extend it
      if (run.dst) HIPCHK(hipMemcpyAsync(run.dst, base + run.off, run.bytes, hipMemcpyDeviceToHost, s0));
      run = Run{segs[i]->off, segs[i]->bytes, d};
    }
    if (run.dst) HIPCHK(hipMemcpyAsync(run.dst, base + run.off, run.bytes, hipMemcpyDeviceToHost, s0));
    const double t_1 = trace_on() ? now_us() : 0;
    HIPCHK(stream_wait(s0));
    if (trace_on()) std::fprintf(stderr, "[cbh] slab dev=%d up=%zu B enqueue=%.1f us wait=%.1f us\n", rep->device, end - L.in_begin, t_1 - t_0, now_us() - t_1);
    return 0;
  }

  // ---- setup on stream 0: launch arguments + the arrays that are not per request (roles, heap, strings)
  HIPCHK(hipMemcpyAsync(base, c->h, sizeof(ka), hipMemcpyHostToDevice, s0));
  for (const Seg* g : {&L.roles, &L.htag, &L.hval, &L.soff, &L.sbytes, &L.sflags}) {
    if (!need_bytes && (g == &L.soff || g == &L.sbytes || g == &L.sflags)) continue;   // no program looks inside a string
    if (g->bytes) HIPCHK(hipMemcpyAsync(base + g->off, g->src, g->bytes, hipMemcpyHostToDevice, s0));
  }
  launch_resolve(rep, ka, L, s0, rc);
  if (rc != 0) return fail("hipMemsetAsync failed");
  HIPCHK(hipEventRecord(c->ev_setup, s0));

  // rows [r0, r1) of a field-major [rows][NR] array of `esz`-byte elements, requests [a, b): one 2-D copy
  static const int copy_mode = env_int("CBH_COPY_MODE", 0);   // 1: a row at a time instead of 2-D copies
  auto up2d = [&](const Seg& g, size_t esz, u32 r0, u32 r1, u32 a, u32 b, hipStream_t s) -> hipError_t {
    if (r1 <= r0 || b <= a) return hipSuccess;
    const size_t pitch = NR * esz, o = (size_t)r0 * pitch + (size_t)a * esz;
    if (a == 0 && b == NR) return hipMemcpyAsync(base + g.off + o, (const uint8_t*)g.src + o, (size_t)(r1 - r0) * pitch, hipMemcpyHostToDevice, s);
    if (copy_mode == 1) {
      for (u32 r = r0; r < r1; ++r) {
        const size_t oo = (size_t)r * pitch + (size_t)a * esz;
        const hipError_t e = hipMemcpyAsync(base + g.off + oo, (const uint8_t*)g.src + oo, (size_t)(b - a) * esz, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return e;
      }
      return hipSuccess;
    }
    return hipMemcpy2DAsync(base + g.off + o, pitch, (const uint8_t*)g.src + o, pitch, (size_t)(b - a) * esz, r1 - r0, hipMemcpyHostToDevice, s);
  };
  if (!pinned) {
    // pageable arrays: the driver stages every copy itself and the calling thread waits for it - chunking buys
    // nothing, so the range goes up array by array, is decided by one launch and comes down array by array
    hipStream_t s = s0;
    HIPCHK(up2d(L.req, 4, 0, reads_strings ? CBH_RQ_NFIELDS : CBH_RQ_NCORE, lo, hi, s));
    HIPCHK(up2d(L.ctag, 1, 0, in->n_columns, lo, hi, s));
    HIPCHK(up2d(L.cval, 8, 0, in->n_columns, lo, hi, s));
    size_t tb = 0, te = 0;
    if (hi > lo) tuples_of(lo, hi, tb, te);
    if (te > tb) HIPCHK(hipMemcpyAsync(base + L.act.off + tb * 4, in->tuple_action + tb, (te - tb) * 4, hipMemcpyHostToDevice, s));
    launch_check(rep, ka, d_args, lo, hi, sh, s, L.dflag.bytes ? base + L.dflag.off : nullptr);
    HIPCHK(hipGetLastError());
    if (te > tb) {
      HIPCHK(hipMemcpyAsync(out->effect + tb, base + L.eff.off + tb, te - tb, hipMemcpyDeviceToHost, s));
      if (out->policy) HIPCHK(hipMemcpyAsync(out->policy + tb, base + L.pol.off + tb * 4, (te - tb) * 4, hipMemcpyDeviceToHost, s));
      if (out->scope) HIPCHK(hipMemcpyAsync(out->scope + tb, base + L.scope.off + tb * 4, (te - tb) * 4, hipMemcpyDeviceToHost, s));
      if (out->status) HIPCHK(hipMemcpyAsync(out->status + tb, base + L.status.off + tb, te - tb, hipMemcpyDeviceToHost, s));
    }
    if (out->edr_mask && hi > lo) HIPCHK(hipMemcpyAsync(out->edr_mask + lo, base + L.edr.off + (size_t)lo * 8, (size_t)(hi - lo) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (trace_on()) std::fprintf(stderr, "[cbh] range [%u,%u) dev=%d pageable total=%.1f us\n", lo, hi, rep->device, now_us() - t_0);
    (void)t;
    return 0;
  }
  // ---- page-locked arrays: chunks of the range round-robin over the streams; on each stream a chunk is
  // uploaded, decided and downloaded in order, and the three streams overlap each other's phases
  u32 k = 0;
  for (u32 a = lo; a < hi; a += chunk_requests, ++k) {
    const u32 b = std::min<u64>((u64)a + chunk_requests, hi);
    hipStream_t s = c->s[k % N_STREAMS];
    if (k < (u32)N_STREAMS && s != s0) HIPCHK(hipStreamWaitEvent(s, c->ev_setup, 0));
    if (reads_strings) HIPCHK(up2d(L.req, 4, 0, CBH_RQ_NFIELDS, a, b, s));
    else HIPCHK(up2d(L.req, 4, 0, CBH_RQ_NCORE, a, b, s));
    HIPCHK(up2d(L.ctag, 1, 0, in->n_columns, a, b, s));
    HIPCHK(up2d(L.cval, 8, 0, in->n_columns, a, b, s));
    size_t tb = 0, te = 0;
    tuples_of(a, b, tb, te);
    if (te > tb) HIPCHK(hipMemcpyAsync(base + L.act.off + tb * 4, in->tuple_action + tb, (te - tb) * 4, hipMemcpyHostToDevice, s));
    launch_check(rep, ka, d_args, a, b, sh, s, L.dflag.bytes ? base + L.dflag.off : nullptr);
    if (te > tb) {
      HIPCHK(hipMemcpyAsync(out->effect + tb, base + L.eff.off + tb, te - tb, hipMemcpyDeviceToHost, s));
      if (out->policy) HIPCHK(hipMemcpyAsync(out->policy + tb, base + L.pol.off + tb * 4, (te - tb) * 4, hipMemcpyDeviceToHost, s));
      if (out->scope) HIPCHK(hipMemcpyAsync(out->scope + tb, base + L.scope.off + tb * 4, (te - tb) * 4, hipMemcpyDeviceToHost, s));
      if (out->status) HIPCHK(hipMemcpyAsync(out->status + tb, base + L.status.off + tb, te - tb, hipMemcpyDeviceToHost, s));
    }
    if (out->edr_mask) HIPCHK(hipMemcpyAsync(out->edr_mask + a, base + L.edr.off + (size_t)a * 8, (size_t)(b - a) * 8, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipGetLastError());
  const double t_1 = trace_on() ? now_us() : 0;
  for (auto& s : c->s) HIPCHK(stream_wait(s));
  if (trace_on()) std::fprintf(stderr, "[cbh] range [%u,%u) dev=%d pinned chunks=%u enqueue=%.1f us wait=%.1f us\n", lo, hi, rep->device, k, t_1 - t_0, now_us() - t_1);
  return 0;
}

extern "C" int cbh_check_batch(cbh_table* t, const cbh_batch* in, const cbh_params* p, cbh_result* out) {
  if (!t || !in || !p || !out) return fail("null argument");
  if (in->n_tuples && !out->effect) return fail("cbh_result.effect is required");
  TableRef ref(t);
  BatchShape sh;
  if (validate_header(t, in) != 0) return -1;
  const Layout L = make_layout(in, t);
  const u32 NR = in->n_requests;
  if (L.in_end <= SMALL_BATCH_BYTES || NR == 0) {
    if (validate_batch(t, in, sh) != 0) return -1;
    return run_small(t, t->reps[0], in, p, out, sh, L);
  }

  // chunks of the three-stream pipeline carry at least ~32 MB of input each: a copy costs a fixed ~20 us on top of
  // its bytes, so smaller chunks lose more to that than the overlap wins (measured, profiles/r02_oneshot_probe.txt)
  const u32 chunk_env = [&] {
    const long v = env_long("CBH_CHUNK_REQUESTS", 0);   // (read at every call: tests change it between calls)
    if (v > 0) return (u32)((v + 63) & ~63l);
    const size_t per_request = NR ? std::max<size_t>(1, (L.in_end - L.in_begin) / NR) : 1;
    return (u32)std::min<size_t>(0xFFFFFFC0u, ((((size_t)32 << 20) / per_request) + 63) & ~(size_t)63);
  }();
  bool pinned = true;
  for (const void* q : {(const void*)in->req_u32, (const void*)in->tuple_action, (const void*)in->col_tag, (const void*)in->col_val,
                        (const void*)out->effect, (const void*)out->policy, (const void*)out->scope, (const void*)out->status, (const void*)out->edr_mask})
    pinned = pinned && is_pinned(q);
  // One device and a page-locked slab: the upload starts NOW and the O(n_requests) validation below runs while the DMA does
  // (a batch that fails it never reaches a kernel: the lease waits for the copies and hands the context back).
  CtxLease early{t->reps[0], nullptr};
  if (pinned && t->reps.size() == 1) {
    if (const uint8_t* slab = slab_base(L)) {
      HIPCHK(hipSetDevice(t->reps[0]->device));
      early.c = ctx_acquire(t->reps[0]);
      if (!early.c) return fail("could not create a launch context");
      if (ctx_reserve(early.c, 4096, L.total) != 0 || slab_upload(early.c, t->reps[0], L, slab, NR) != 0) return -1;
    }
  }
  if (validate_batch(t, in, sh) != 0) return -1;
  // contiguous request ranges over the devices (engine.go:309-338 deals inputs to workers; here a worker is a GPU)
  u32 n_dev = 1;
  if (t->reps.size() > 1 && sh.ascending) n_dev = (u32)std::min<size_t>(t->reps.size(), std::max<u32>(1, NR / SHARD_MIN_REQUESTS));
  if (n_dev == 1) return run_range(t, t->reps[0], in, p, out, sh, L, 0, NR, pinned, sh.ascending ? chunk_env : NR, early.c);
  std::vector<int> rcs(n_dev, 0);
  std::vector<std::string> errs(n_dev);
  auto work = [&](u32 i) {
    const u32 lo = (u32)(((u64)NR * i / n_dev) & ~63ull), hi = i + 1 == n_dev ? NR : (u32)(((u64)NR * (i + 1) / n_dev) & ~63ull);
    rcs[i] = run_range(t, t->reps[i], in, p, out, sh, L, lo, hi, pinned, chunk_env);
    if (rcs[i] != 0) errs[i] = g_err;
  };
  std::vector<std::thread> th;
  for (u32 i = 1; i < n_dev; ++i) th.emplace_back(work, i);
  work(0);
  for (auto& x : th) x.join();
  for (u32 i = 0; i < n_dev; ++i) if (rcs[i] != 0) return fail("device " + std::to_string(t->reps[i]->device) + ": " + errs[i]);
  return 0;
}
// The trace pass (cerbos_hip.h): the batch packed into the staging block, one copy up, the tracing kernel, the
// results and the log down.  Not a fast path - it serves the (few) inputs whose evaluation errors / outputs are wanted.
extern "C" int cbh_trace_batch(cbh_table* t, const cbh_batch* in, const cbh_params* p, cbh_result* out, cbh_trace* trace) {
  if (!t || !in || !p || !out || !trace) return fail("null argument");
  if (in->n_tuples && !out->effect) return fail("cbh_result.effect is required");
  if (trace->capacity && !trace->records) return fail("cbh_trace.records is required");
  TableRef ref(t);
  Replica* rep = t->reps[0];
  if (!rep->dev.trace_pool) return fail("the table was lowered without the trace sections");
  BatchShape sh;
  if (validate_batch(t, in, sh) != 0) return -1;
  trace->count = 0;
  if (in->n_requests == 0) return 0;
  const Layout L = make_layout(in, t);
  const size_t log_off = (L.total + 255) & ~(size_t)255;                       // {count, pad ...} then the records
  const size_t rec_off = log_off + 256, rec_bytes = (size_t)trace->capacity * CBH_TRACE_RECORD_WORDS * 4;
  const size_t total = rec_off + rec_bytes;
  HIPCHK(hipSetDevice(rep->device));
  CtxLease lease{rep, ctx_acquire(rep)};
  OneShot* c = lease.c;
  if (!c) return fail("could not create a launch context");
  if (ctx_reserve(c, total, total) != 0) return -1;
  hipStream_t s = c->s[0];
  lease.used = 1;
  uint8_t* base = c->d;
  KernelArgs ka;
  bind_args(ka, rep->dev, in, p, L, base);
  ka.o.trace_rec = (u32*)(base + rec_off); ka.o.trace_cnt = (u32*)(base + log_off); ka.o.trace_cap = trace->capacity;
  std::memcpy(c->h + L.args.off, &ka, sizeof(ka));
  for (const Seg* g : {&L.req, &L.roles, &L.act, &L.ctag, &L.cval, &L.htag, &L.hval, &L.soff, &L.sbytes, &L.sflags})
    if (g->bytes) std::memcpy(c->h + g->off, g->src, g->bytes);
  int rc = 0;
  HIPCHK(hipMemcpyAsync(c->d, c->h, L.in_end, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(base + log_off, 0, 256, s));
  launch_resolve(rep, ka, L, s, rc);
  if (rc != 0) return fail("hipMemsetAsync failed");
  const u32 grid = (in->n_requests + CBH_BLOCK - 1) / CBH_BLOCK;
  hipLaunchKernelGGL(cbh_trace_kernel, dim3(grid), dim3(CBH_BLOCK), check_lds_bytes(ka.b, rep->dev.flags), s, ka, (const KernelArgs*)(base + L.args.off));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(c->h + L.out_begin, c->d + L.out_begin, log_off + 256 - L.out_begin, hipMemcpyDeviceToHost, s));
  HIPCHK(stream_wait(s));
  struct Dst { const Seg* g; void* dst; };
  const Dst outs[5] = {{&L.eff, out->effect}, {&L.pol, out->policy}, {&L.scope, out->scope}, {&L.status, out->status}, {&L.edr, out->edr_mask}};
  for (const Dst& o : outs) if (o.dst && o.g->bytes) std::memcpy(o.dst, c->h + o.g->off, o.g->bytes);
  std::memcpy(&trace->count, c->h + log_off, 4);
  const size_t kept = std::min<size_t>(trace->count, trace->capacity);
  if (kept) HIPCHK(hipMemcpy(trace->records, base + rec_off, kept * CBH_TRACE_RECORD_WORDS * 4, hipMemcpyDeviceToHost));
  return 0;
}
