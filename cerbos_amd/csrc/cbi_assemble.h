// cbi_assemble.h - device results -> serialized CheckOutputs / one CheckResourcesResponse (part of cbh_ingest.cpp).
#pragma once

struct cbi_outputs { std::vector<u8> bytes, flags; std::vector<u64> offsets; };   // output i = bytes[offsets[i] .. offsets[i + 1])

namespace {
// How the tuples of `res` (device order) answer the inputs a batch was flattened from.  inv: input-order tuple k -> the device tuple
// that answers it; first[i]: input-order index of input i's first tuple (first[n] = all of them); edr: the effective derived
// roles of input i, OR-ed over its device requests.
struct TupleIndex {
  std::vector<u32> inv;
  std::vector<u64> first, edr;
  // -> an error text, or nullptr.  `foreign`: what to say of a batch that was not made from these n inputs.
  const char* build(const cbi_batch* b, u32 n, const u64* edr_mask, const char* foreign, bool with_inv = true) {
    const u32 T = b->view.n_tuples, R = b->view.n_requests;
    if (with_inv) inv.resize(T);
    for (u32 j = 0; with_inv && j < T; ++j) { if (b->tuple_perm[j] >= T) return "corrupt tuple permutation"; inv[b->tuple_perm[j]] = j; }
    edr.assign(n, 0); first.assign((size_t)n + 1, 0);
    for (u32 q = 0; q < R; ++q) {
      const u32 i = b->req_input[q];
      if (i >= n) return foreign;
      if (edr_mask) edr[i] |= edr_mask[q];
      first[i + 1] += b->req[(size_t)RQ_ACT_CNT * R + q];
    }
    for (u32 i = 0; i < n; ++i) first[i + 1] += first[i];
    return first[n] != T ? foreign : nullptr;
  }
};

// The actions of one output, each name once, with the tuple that decides it.
struct Act { std::string_view name; u32 j; };
// Action `name` of an input is answered by tuple j.  setEffect (check.go:513-530): a later duplicate replaces an earlier one
// unless that one is a DENY and it is not.  The tuple's status goes into the output's flags whether it is kept or not.
inline void fold_action(std::vector<Act>& acts, std::string_view name, u32 j, const cbh_result* res, u8& flags) {
  auto a = std::find_if(acts.begin(), acts.end(), [&](const Act& x) { return x.name == name; });
  if (a == acts.end()) acts.push_back(Act{name, j});
  else if (res->effect[j] == CBH_EFFECT_DENY || res->effect[a->j] != CBH_EFFECT_DENY) a->j = j;
  const u8 st = res->status ? res->status[j] : (u8)CBH_ST_OK;
  flags |= st == CBH_ST_UNSUPPORTED ? CBI_OUT_UNSUPPORTED : st == CBH_ST_CEL_ERROR ? CBI_OUT_CEL_ERROR : st == CBH_ST_WANTS_TRACE ? CBI_OUT_WANTS_TRACE : 0u;
}

// Policy key and scope of the tuple that decides an action (the CheckOutput's ActionEffect, the response's meta), or an error text.
// `pol` holds the key of `pol_word`: the actions of one input mostly share it.
struct Matched {
  const cbi_table* t; const cbh_result* res; std::string_view dver;
  std::string pol, kbuf, vbuf;
  u32 pol_word = 0xFFFFFFFFu;
  std::string_view key, scope;   // of the last tuple asked for
  Matched(const cbi_table* t, const cbh_result* res, std::string_view dver) : t(t), res(res), dver(dver) {}
  const char* of(u32 j, const PrincipalView& P, const ResourceView& Rs) {
    if (res->policy && res->policy[j] != pol_word) {
      pol_word = res->policy[j];
      if (const char* e = policy_key(t, pol_word, P, Rs, dver, pol, kbuf, vbuf)) return e;
    }
    scope = std::string_view();
    if (res->scope && res->scope[j] != 0xFFFFFFFFu) {
      if (res->scope[j] >= t->scopes.size()) return "scope index out of range";
      scope = t->scopes[res->scope[j]];
    }
    key = res->policy ? std::string_view(pol) : std::string_view();
    return nullptr;
  }
};

// The CheckOutputs of inputs 0 .. n - 1.  inv: input-order tuple k -> the tuple of `res` that answers it (null: k itself);
// edr: effective derived roles per input; first[i]: input-order index of input i's first tuple; in_span / act_span: where the
// strings sit in the messages (null: every message is walked again).
int assemble_outputs(const cbi_table* t, const cbh_result* res, const uint8_t* bytes, const uint64_t* offsets, uint32_t n,
                     std::string_view dver, int n_threads, const u32* inv, const u64* edr, const u64* first,
                     const u32* in_span, const u32* act_span, cbi_outputs** out) {
  const bool spans = in_span != nullptr && act_span != nullptr;
  // inputs [lo, hi) -> o (offsets relative to the part)
  auto assemble_range = [&](u32 lo, u32 hi, cbi_outputs* o, std::string& err) -> int {
    auto bail = [&](const std::string& m) { err = m; return -1; };
    o->offsets.reserve(hi - lo + 1); o->offsets.push_back(0); o->flags.assign(hi - lo, 0);
    o->bytes.reserve((size_t)(hi - lo) * 96);
    std::vector<std::string_view> names;
    std::vector<Act> acts;
    Matched matched(t, res, dver);
    u64 k = first[lo]; const u64 k_hi = first[hi];
    for (u32 i = lo; i < hi; ++i) {
      const Span m{bytes + offsets[i], bytes + offsets[i + 1]};
      std::string_view request_id;
      PrincipalView P; ResourceView Rs;
      acts.clear();
      bool ours = true;
      auto take = [&](std::string_view name) { fold_action(acts, name, inv ? inv[k] : (u32)k, res, o->flags[i - lo]); ++k; };
      // request id, principal, resource, action names of input i: from where the flattener noted them (cbi_batch::in_span), or by a second walk
      if (spans) {
        const size_t mlen = (size_t)(m.e - m.p);
        const u32* sp = in_span + (size_t)i * 2 * IN_SPAN_N;
        auto at = [&](const u32* s) { if ((size_t)s[0] + s[1] > mlen) { ours = false; return std::string_view(); } return std::string_view((const char*)m.p + s[0], s[1]); };
        request_id = at(sp + 2 * SPAN_REQUEST_ID);
        P = PrincipalView{at(sp + 2 * SPAN_P_ID), at(sp + 2 * SPAN_P_VERSION), {}};
        Rs = ResourceView{at(sp + 2 * SPAN_R_KIND), at(sp + 2 * SPAN_R_VERSION), at(sp + 2 * SPAN_R_ID), {}};
        for (const u64 k_end = first[i + 1]; k < k_end && ours;) take(at(act_span + 2 * k));
      } else {
        CheckInputView v; bool bad = false;
        names.clear();
        read_check_input(m, v, names, bad);
        read_principal(v.principal, P, bad);
        read_resource(v.resource, Rs, bad);
        request_id = v.request_id;
        ours = names.size() <= k_hi - k;
        if (ours && bad) return bail("malformed CheckInput at index " + std::to_string(i));
        if (ours) for (std::string_view name : names) take(name);
      }
      if (!ours) return bail("batch does not belong to these inputs");
      // One reservation for everything but the derived-role names, then plain pointer writes (action_entry_bound)
      std::vector<u8>& ob = o->bytes;
      size_t bound = 2 * LD_OVERHEAD + request_id.size() + Rs.id.size();
      for (const Act& a : acts) bound += action_entry_bound(a.name.size());
      const size_t at0 = ob.size();
      ob.resize(at0 + bound);
      RawWriter w{ob.data() + at0, ob.data() + ob.size()};
      w.str(1, request_id); w.str(2, Rs.id);
      matched.pol_word = 0xFFFFFFFFu;   // another principal and resource: so are the keys made of them
      for (const Act& a : acts) {
        if (const char* e = matched.of(a.j, P, Rs)) return bail(e);
        const std::string_view pol_s = matched.key, scope_s = matched.scope;
        const size_t need = action_entry_bound(a.name.size(), pol_s.size() + scope_s.size());
        if ((size_t)(w.end - w.w) < need) {   // a key longer than the allowance (unusual): grow
          const size_t used = (size_t)(w.w - ob.data());
          ob.resize(ob.size() + need);
          w = RawWriter{ob.data() + used, ob.data() + ob.size()};
        }
        // sizes first, then one pass of writes: entry {1: action, 2: ActionEffect {1: effect, 2: policy, 3: scope}}
        const u8 effect = res->effect[a.j];
        const size_t eff_len = (effect ? 1 + varint_size(effect) : 0) + (pol_s.empty() ? 0 : ld_size(pol_s.size())) +
                               (scope_s.empty() ? 0 : ld_size(scope_s.size()));
        w.varint(3u << 3 | 2); w.varint(ld_size(a.name.size()) + ld_size(eff_len));
        w.ld(1, a.name);
        w.varint(2u << 3 | 2); w.varint(eff_len);
        if (effect) { w.varint(1 << 3 | 0); w.varint(effect); }
        w.str(2, pol_s); w.str(3, scope_s);
        assert(w.w <= w.end);
      }
      ob.resize((size_t)(w.w - ob.data()));
      for (u32 d = 0; d < 64 && d < t->dr_names.size(); ++d) if ((edr[i] >> d) & 1) put_ld(ob, 4, t->dr_names[d]);
      o->offsets.push_back(ob.size());
    }
    if (k != k_hi) return bail("batch does not belong to these inputs");
    return 0;
  };

  const std::vector<u32> base = split_parts(n, n_threads); const u32 P = (u32)base.size() - 1;
  auto o = std::make_unique<cbi_outputs>();
  std::vector<cbi_outputs> parts(P > 1 ? P : 0);   // a single part is assembled straight into o
  std::string err;
  if (run_parts(P, [&](u32 k, std::string& e) { return assemble_range(base[k], base[k + 1], P > 1 ? &parts[k] : o.get(), e); }, err) >= 0) return fail(err);
  if (P > 1) {
    size_t total = 0;
    for (const cbi_outputs& p : parts) total += p.bytes.size();
    o->bytes.resize(total); o->flags.resize(n); o->offsets.resize((size_t)n + 1);
    size_t at = 0;
    for (u32 k = 0; k < P; ++k) {
      const cbi_outputs& p = parts[k];
      if (!p.bytes.empty()) std::memcpy(o->bytes.data() + at, p.bytes.data(), p.bytes.size());
      if (!p.flags.empty()) std::memcpy(o->flags.data() + base[k], p.flags.data(), p.flags.size());
      for (u32 i = base[k]; i <= base[k + 1]; ++i) o->offsets[i] = at + p.offsets[i - base[k]];
      at += p.bytes.size();
    }
  }
  o->bytes.reserve(1);
  *out = o.release();
  return 0;
}
}  // namespace

extern "C" {
int cbi_assemble_pb_mt(const cbi_table* t, const cbi_batch* b, const cbh_result* res, const uint8_t* bytes, const uint64_t* offsets,
                       uint32_t n, const char* default_version, int n_threads, cbi_outputs** out) {
  if (!t || !b || !res || (!res->effect && b->view.n_tuples) || !out || (n && (!bytes || !offsets))) return fail("cbi_assemble_pb: null argument");   // (inputs without an action: no tuple, no array)
  std::string_view dver = default_version ? default_version : "default";
  TupleIndex ix;
  if (const char* e = ix.build(b, n, res->edr_mask, "batch does not belong to these inputs")) return fail(e);
  const u32 T = b->view.n_tuples;
  return assemble_outputs(t, res, bytes, offsets, n, dver, n_threads, ix.inv.data(), ix.edr.data(), ix.first.data(),
                          b->in_span.size() == (size_t)n * 2 * IN_SPAN_N && b->act_span.size() == (size_t)T * 2 ? b->in_span.data() : nullptr,
                          b->act_span.data(), out);
}

// Results of a batch the DEVICE flattened (cerbos_hip.h cbh_wire_flatten: tuples in input order, one request per input) ->
// serialized CheckOutputs; in_span / act_span / act_off as cbh_wire_spans_download returns them.
int cbi_assemble_wire_pb(const cbi_table* t, const cbh_result* res, const uint8_t* bytes, const uint64_t* offsets, uint32_t n,
                         uint32_t n_tuples, const uint32_t* in_span, const uint32_t* act_span, const uint32_t* act_off,
                         const char* default_version, int n_threads, cbi_outputs** out) {
  if (!t || !res || (!res->effect && n_tuples) || !out || (n && (!bytes || !offsets || !in_span || !act_off)) || (n_tuples && !act_span)) return fail("cbi_assemble_wire_pb: null argument");
  std::string_view dver = default_version ? default_version : "default";
  TupleIndex ix;   // from the device's own offsets: tuples in input order (no inv), derived roles per input already
  std::vector<u64>& first = ix.first;
  first.assign((size_t)n + 1, 0); ix.edr.assign(res->edr_mask ? 0 : n, 0);
  for (u32 i = 0; i <= n; ++i) {
    first[i] = n ? act_off[i] : 0;
    if (first[i] > n_tuples || (i && first[i] < first[i - 1])) return fail("cbi_assemble_wire_pb: action offsets are not a partition of the tuples");
  }
  if (first[n] != n_tuples) return fail("cbi_assemble_wire_pb: action offsets are not a partition of the tuples");
  return assemble_outputs(t, res, bytes, offsets, n, dver, n_threads, nullptr, res->edr_mask ? res->edr_mask : ix.edr.data(), first.data(), in_span, act_span, out);
}

int cbi_assemble_pb(const cbi_table* t, const cbi_batch* b, const cbh_result* res, const uint8_t* bytes, const uint64_t* offsets,
                    uint32_t n, const char* default_version, cbi_outputs** out) {
  return cbi_assemble_pb_mt(t, b, res, bytes, offsets, n, default_version, 1, out);
}

int cbi_assemble_response_pb(const cbi_table* t, const cbi_batch* b, const cbh_result* res, const uint8_t* request, uint64_t request_len,
                             const char* default_version, cbi_outputs** out) {
  return cbi_assemble_response_traced_pb(t, b, res, request, request_len, default_version, nullptr, out);
}

int cbi_assemble_response_traced_pb(const cbi_table* t, const cbi_batch* b, const cbh_result* res, const uint8_t* request, uint64_t request_len,
                                    const char* default_version, const cbi_outputs* traced, cbi_outputs** out) {
  if (!t || !b || !res || (!res->effect && b->view.n_tuples) || !out || !request) return fail("cbi_assemble_response_pb: null argument");
  const std::string_view dver = default_version ? default_version : "default";
  RequestParts rp;
  if (!split_request(request, request_len, rp)) return fail("malformed CheckResourcesRequest");
  const u32 n = (u32)rp.entries.size(), T = b->view.n_tuples;
  TupleIndex ix;
  if (const char* e = ix.build(b, n, res->edr_mask, "batch does not belong to this request")) return fail(e);
  auto o = std::make_unique<cbi_outputs>();
  o->flags.assign(n, 0);
  std::vector<u8>& ob = o->bytes;
  ob.reserve((size_t)n * 96 + 64);
  // CheckResourcesResponse (response.proto:187-300): request_id = 1, results = 2 {resource = 1 {id, kind, policy_version,
  // scope}, actions = 2 map<string, Effect>, meta = 4 {actions = 1 map<string, {matched_policy = 1, matched_scope = 2}>,
  // effective_derived_roles = 2}} - what CheckResources assembles from the outputs (cerbos_svc.go:297-343)
  put_str(ob, 1, rp.request_id);
  PrincipalView P;
  { bool bad = false; read_principal(rp.principal, P, bad); if (bad) return fail("malformed principal"); }
  std::vector<std::string_view> names;
  std::vector<Act> acts;
  std::vector<u8> entry_buf, meta_buf, tmp;
  Matched matched(t, res, dver);
  u64 k = 0;
  for (u32 i = 0; i < n; ++i) {
    Span resource{nullptr, nullptr}; bool bad = false;
    names.clear();
    read_entry(rp.entries[i], resource, names, bad);
    if (names.size() > T - k) return fail("batch does not belong to this request");
    ResourceView Rs;
    read_resource(resource, Rs, bad);
    if (bad) return fail("malformed resource entry " + std::to_string(i));
    acts.clear();
    for (std::string_view name : names) fold_action(acts, name, ix.inv[k++], res, o->flags[i]);
    entry_buf.clear(); meta_buf.clear(); tmp.clear();
    put_str(tmp, 1, Rs.id); put_str(tmp, 2, Rs.kind); put_str(tmp, 3, Rs.version); put_str(tmp, 4, Rs.scope);
    put_msg(entry_buf, 1, tmp);
    matched.pol_word = 0xFFFFFFFFu;   // another resource: so are the keys made of it
    for (const Act& a : acts) {
      const u8 effect = res->effect[a.j];
      // actions map entry {1: name, 2: effect (enum varint, left out when 0)}
      put_head(entry_buf, 2, ld_size(a.name.size()) + (effect ? 1 + varint_size(effect) : 0));
      put_ld(entry_buf, 1, a.name);
      if (effect) { entry_buf.push_back(2 << 3 | 0); put_varint(entry_buf, effect); }
      if (rp.include_meta) {
        if (const char* e = matched.of(a.j, P, Rs)) return fail(e);
        const std::string_view pol_s = matched.key, scope_s = matched.scope;
        const size_t em_len = (pol_s.empty() ? 0 : ld_size(pol_s.size())) + (scope_s.empty() ? 0 : ld_size(scope_s.size()));
        put_head(meta_buf, 1, ld_size(a.name.size()) + ld_size(em_len));
        put_ld(meta_buf, 1, a.name);
        put_head(meta_buf, 2, em_len);
        put_str(meta_buf, 1, pol_s); put_str(meta_buf, 2, scope_s);
      }
    }
    if (rp.include_meta) {
      for (u32 d = 0; d < 64 && d < t->dr_names.size(); ++d) if ((ix.edr[i] >> d) & 1) put_ld(meta_buf, 2, t->dr_names[d]);
      put_msg(entry_buf, 4, meta_buf);   // present (possibly empty) when asked for
    }
    if (traced) {   // ResultEntry.outputs = 5 <- CheckOutput.outputs = 6 of the trace consumer's bytes for this entry (cerbos_svc.go:325-327)
      if (traced->offsets.size() != (size_t)n + 1) return fail("traced outputs do not belong to this request");
      Span ts{traced->bytes.data() + traced->offsets[i], traced->bytes.data() + traced->offsets[i + 1]}; Field tf; bool tbad = false;
      while (next(ts, tf, tbad)) if (tf.num == 6 && tf.wt == 2) put_ld(entry_buf, 5, sv(tf.s));
      o->flags[i] |= traced->flags[i] & (CBI_TRACE_ERRORS_INCOMPLETE | CBI_TRACE_OUTPUTS_INCOMPLETE);
    }
    put_msg(ob, 2, entry_buf);
  }
  if (k != T) return fail("batch does not belong to this request");
  o->offsets.assign({0, (u64)ob.size()});
  ob.reserve(1);
  *out = o.release();
  return 0;
}
}  // extern "C"
