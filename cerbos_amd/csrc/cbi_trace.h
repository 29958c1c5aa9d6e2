// cbi_trace.h - the trace pass's consumer: cbh_trace records -> the evaluation_errors / outputs fields of a CheckOutput (part of
// cbh_ingest.cpp).  cerbos_amd/trace.py is the same consumer in Python; nothing here evaluates CEL.
#pragma once

namespace {
struct TraceIncomplete {};

// %s of a value (cel-go strings.go formatString and the per-type formatters)
void format_value(const TVal& v, bool nested, std::string& out) {
  switch (v.k) {
    case TVal::Null: out += "null"; return;
    case TVal::Bool: out += v.b ? "true" : "false"; return;
    case TVal::String: if (nested) { out += '"'; out += v.s; out += '"'; } else out += v.s; return;
    case TVal::Int: out += std::to_string(v.i); return;
    case TVal::Double: {
      if (std::isnan(v.d) || std::isinf(v.d)) throw TraceIncomplete{};
      if (v.d == std::floor(v.d) && std::fabs(v.d) < 1e21) {
        if (std::fabs(v.d) < 9e18) { out += std::to_string((long long)v.d); return; }
        char buf[64]; std::snprintf(buf, sizeof buf, "%.0f", v.d); out += buf; return;
      }
      char buf[64]; auto r = std::to_chars(buf, buf + sizeof buf, v.d); out.append(buf, r.ptr); return;   // shortest round-trip, as Python's repr
    }
    case TVal::List: {
      out += '[';
      for (size_t i = 0; i < v.items.size(); ++i) { if (i) out += ", "; format_value(v.items[i], true, out); }
      out += ']'; return;
    }
    case TVal::Map: {
      std::vector<std::pair<std::string, size_t>> order;   // by the keys' text
      for (size_t i = 0; i + 1 < v.items.size(); i += 2) { std::string k; format_value(v.items[i], false, k); order.emplace_back(std::move(k), i); }
      std::stable_sort(order.begin(), order.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
      out += '{';
      for (size_t n = 0; n < order.size(); ++n) {
        if (n) out += ", ";
        format_value(v.items[order[n].second], true, out); out += ": "; format_value(v.items[order[n].second + 1], true, out);
      }
      out += '}'; return;
    }
  }
}
// cel-go ext.Strings format: %s, %d, %% (anything else is left to the caller's engine)
TVal format_call(const std::string& fmt, const std::vector<TVal>& args) {
  TVal r; r.k = TVal::String;
  size_t ai = 0;
  for (size_t i = 0; i < fmt.size();) {
    const char c = fmt[i++];
    if (c != '%') { r.s += c; continue; }
    if (i >= fmt.size()) throw TraceIncomplete{};
    const char spec = fmt[i++];
    if (spec == '%') { r.s += '%'; continue; }
    if (ai >= args.size() || (spec != 's' && spec != 'd')) throw TraceIncomplete{};
    const TVal& a = args[ai++];
    if (spec == 'd') {
      if (a.k == TVal::Int) r.s += std::to_string(a.i);
      else if (a.k == TVal::Double && a.d == std::floor(a.d) && std::fabs(a.d) < 9e18) r.s += std::to_string((long long)a.d);
      else throw TraceIncomplete{};
    } else format_value(a, false, r.s);
  }
  return r;
}
bool tval_key_equal(const TVal& a, const TVal& b) {
  if (a.k != b.k) return false;
  switch (a.k) { case TVal::Bool: return a.b == b.b; case TVal::Int: return a.i == b.i; case TVal::Double: return a.d == b.d; case TVal::String: return a.s == b.s; default: return false; }
}
TVal assemble_template(const TNode& t, const std::vector<TVal>& holes) {
  switch (t.kind) {
    case 0: if (t.hole >= holes.size()) throw TraceIncomplete{}; return holes[t.hole];
    case 1: return t.cst;
    case 2: { TVal r; r.k = TVal::List; for (const TNode& k : t.kids) r.items.push_back(assemble_template(k, holes)); return r; }
    case 3: {
      TVal r; r.k = TVal::Map;
      for (size_t i = 0; i + 1 < t.kids.size(); i += 2) {
        TVal key = assemble_template(t.kids[i], holes);
        if (key.k == TVal::Null || key.k == TVal::List || key.k == TVal::Map) throw TraceIncomplete{};   // "unsupported key type"
        for (size_t j = 0; j < r.items.size(); j += 2) if (tval_key_equal(r.items[j], key)) throw TraceIncomplete{};   // a repeated key
        r.items.push_back(std::move(key)); r.items.push_back(assemble_template(t.kids[i + 1], holes));
      }
      return r;
    }
    default: { std::vector<TVal> args; for (const TNode& k : t.kids) args.push_back(assemble_template(k, holes)); return format_call(t.fmt, args); }
  }
}
// the derived roles of the low `bits` bits of `mask`, by name
std::vector<std::string> sorted_dr_names(const cbi_table* t, u64 mask, u32 bits) {
  std::vector<std::string> names;
  for (u32 d = 0; d < bits && d < t->dr_names.size(); ++d) if ((mask >> d) & 1) names.push_back(t->dr_names[d]);
  std::sort(names.begin(), names.end());
  return names;
}
// google.protobuf.Value (struct.proto): null 1, number 2, string 3, bool 4, struct 5 {fields 1: map<string, Value>}, list 6 {values 1}
void put_value(std::vector<u8>& o, const TVal& v) {
  switch (v.k) {
    case TVal::Null: o.push_back(1 << 3 | 0); o.push_back(0); return;
    case TVal::Bool: o.push_back(4 << 3 | 0); o.push_back(v.b ? 1 : 0); return;
    case TVal::Int: case TVal::Double: { const double d = v.k == TVal::Int ? (double)v.i : v.d; o.push_back(2 << 3 | 1); u8 b[8]; memcpy(b, &d, 8); o.insert(o.end(), b, b + 8); return; }
    case TVal::String: put_ld(o, 3, v.s); return;
    case TVal::List: {
      std::vector<u8> lst;
      for (const TVal& e : v.items) { std::vector<u8> eb; put_value(eb, e); put_msg(lst, 1, eb); }
      put_msg(o, 6, lst); return;
    }
    case TVal::Map: {
      std::vector<u8> st;
      for (size_t i = 0; i + 1 < v.items.size(); i += 2) {
        std::string key; format_value(v.items[i], false, key);
        std::vector<u8> vb, ent; put_value(vb, v.items[i + 1]);
        put_ld(ent, 1, key); put_msg(ent, 2, vb);
        put_msg(st, 1, ent);
      }
      put_msg(o, 5, st); return;
    }
  }
}
// what the consumer reads of input i: the messages its attribute paths resolve in, and its action names in order
struct InputView : CheckInputView { std::vector<std::string_view> actions; };
// view_of(i, InputView&) reads input i, when a record first refers to it
template <class ViewOf>
int trace_decode(const cbi_table* t, const cbi_batch* b, const cbh_result* res, const uint32_t* records, uint32_t count, uint32_t n,
                 const ViewOf& view_of, cbi_outputs** out) {
  if (!t->has_trace) return fail("the table was lowered without the trace sections");
  const u32 R = b->view.n_requests;
  auto RQ = [&](u32 f, u32 q) { return b->req[(size_t)f * R + q]; };
  TupleIndex ix;
  if (const char* e = ix.build(b, n, nullptr, "batch does not belong to these inputs", false)) return fail(e);
  const std::vector<u64>& first = ix.first;
  const u32 K = t->K;
  auto str = [&](u64 id) -> std::string_view {
    if (id < K) return t->at((u32)id);
    const u64 l = id - K;
    if (l >= b->str_flags.size()) throw TraceIncomplete{};
    return b->local((u32)l);
  };
  std::function<TVal(u32, u64, int)> to_tval = [&](u32 tag, u64 v, int depth) -> TVal {
    TVal r;
    if (depth > 64) throw TraceIncomplete{};
    switch (tag) {
      case 0: return r;
      case 1: r.k = TVal::Bool; r.b = v != 0; return r;
      case 2: r.k = TVal::Int; r.i = (long long)v; return r;
      case 3: if (v >> 63) { r.k = TVal::Double; r.d = (double)v; } else { r.k = TVal::Int; r.i = (long long)v; } return r;
      case 4: r.k = TVal::Double; memcpy(&r.d, &v, 8); return r;
      case 5: r.k = TVal::String; r.s = std::string(str(v & 0xFFFFFFFFu)); return r;
      case 6: case 7: {
        const u32 sel = (u32)(v >> 62), off = (u32)((v >> 32) & 0x3FFFFFFFu), len = (u32)v;
        r.k = tag == 6 ? TVal::List : TVal::Map;
        if (sel == CBH_HEAP_ROLES) { if ((u64)off + len > b->roles.size()) throw TraceIncomplete{}; for (u32 i = 0; i < len; ++i) { TVal e; e.k = TVal::String; e.s = std::string(str(b->roles[off + i])); r.items.push_back(std::move(e)); } return r; }
        if (sel == CBH_HEAP_LOCAL && tag == 6 && depth == 0) { r.local = true; r.i = len; return r; }
        const u8* tags; const u64* vals; u64 cap;
        if (sel == CBH_HEAP_BATCH) { tags = b->heap_tag.data(); vals = b->heap_val.data(); cap = b->heap_tag.size(); }
        else if (sel == CBH_HEAP_TABLE) { tags = t->theap_tag; vals = t->theap_val; cap = t->theap_len; }
        else throw TraceIncomplete{};
        const u64 cnt = tag == 6 ? (u64)len : 2ull * len;
        if ((u64)off + cnt > cap) throw TraceIncomplete{};
        for (u64 i = 0; i < cnt; ++i) r.items.push_back(to_tval(tags[off + i], vals[off + i], depth + 1));
        return r;
      }
      case 11: {   // CBH_T_EDRSET: runtime.effectiveDerivedRoles as a value - the names of the mask's bits, sorted (check.go:593-610)
        r.k = TVal::List;
        for (auto& nm : sorted_dr_names(t, v, 64)) { TVal e; e.k = TVal::String; e.s = std::move(nm); r.items.push_back(std::move(e)); }
        return r;
      }
      default: throw TraceIncomplete{};   // timestamps / durations as output values
    }
  };
  // the text of an error (include/cerbos_hip.h CBH_ERR_*) for input `iv`
  auto message = [&](u64 payload, const InputView& iv) -> std::string {
    const u32 code = (u32)(payload & 0xFF); const u64 detail = payload >> 8;
    switch (code) {
      case CBH_ERR_NO_SUCH_OVERLOAD: return "no such overload";
      case CBH_ERR_DIV_BY_ZERO: return "division by zero";
      case CBH_ERR_MOD_BY_ZERO: return "modulus by zero";
      case CBH_ERR_INT_OVERFLOW: return "integer overflow";
      case CBH_ERR_UINT_OVERFLOW: return "unsigned integer overflow";
      case CBH_ERR_NEG_SHIFT:   // cel-go ext/math.go: detail bit 0 = bitShiftRight, the rest the offset's magnitude
        return std::string("math.bitShift") + ((detail & 1) ? "Right" : "Left") + "() negative offset: -" + std::to_string(detail >> 1);
      case CBH_ERR_OPT_NONE: return "optional.none() dereference";
      case CBH_ERR_NO_SUCH_KEY: return "no such key: " + std::string(str(detail & 0xFFFFFFFFu));
      case CBH_ERR_UNDEFINED_FIELD: if (detail >= t->trace_strings.size()) throw TraceIncomplete{}; return "undefined field '" + t->trace_strings[detail] + "'";
      case CBH_ERR_EDR_FAILED: {
        const std::vector<std::string> names = sorted_dr_names(t, detail, 56);
        std::string m = "failed to compute effective derived roles [";
        for (size_t i = 0; i < names.size(); ++i) { if (i) m += ", "; m += names[i]; }
        return m + "]";
      }
      case CBH_ERR_ATTR_MISSING: {
        // the column's path did not resolve in this input: the step that failed decides the text
        if (detail >= t->columns.size()) throw TraceIncomplete{};
        const Column& col = t->columns[detail];
        bool bad = false;
        Span holder = col.root == 0 ? iv.principal : col.root == 1 ? iv.resource : iv.aux;   // the message whose map field is the root
        u32 fnum = col.root == 2 ? 1u : col.root == 3 ? 2u : 4u;
        size_t k = 0;
        Span cur{nullptr, nullptr};
        if (col.keys.empty()) throw TraceIncomplete{};
        if (!map_get(holder, fnum, col.keys[0], cur, bad)) return "no such key: " + col.keys[0];
        k = 1;
        if (col.root == 3) {   // name -> {"claims": {...}}
          if (k >= col.keys.size()) throw TraceIncomplete{};
          if (col.keys[k] != "claims") return "no such key: " + col.keys[k];
          ++k;
          if (k >= col.keys.size()) throw TraceIncomplete{};
          Span inner{nullptr, nullptr};
          if (!map_get(cur, 1, col.keys[k], inner, bad)) return "no such key: " + col.keys[k];
          cur = inner; ++k;
        }
        for (; k < col.keys.size(); ++k) {
          Val v;
          if (!value(cur, v, bad) || v.kind != 5) return "no such overload";
          Span nxt{nullptr, nullptr};
          if (!map_get(v.s, 1, col.keys[k], nxt, bad)) return "no such key: " + col.keys[k];
          cur = nxt;
        }
        throw TraceIncomplete{};
      }
      default: throw TraceIncomplete{};
    }
  };

  struct Visit { u32 src = 0; u64 mask = 0; bool drfail = false; std::map<u32, std::pair<bool, TVal>> ok_parts; std::map<u32, std::string> err_parts;
                 std::map<u32, std::map<u32, TVal>> elems; };
  struct Key { u32 q, pass, ri, site, rule; bool operator<(const Key& o) const { return std::tie(q, pass, ri, site, rule) < std::tie(o.q, o.pass, o.ri, o.site, o.rule); } };
  std::vector<std::set<std::pair<std::string, std::string>>> errs(n);
  std::vector<std::map<Key, Visit>> visits(n);
  std::vector<u8> flags(n, 0), have_view(n, 0);
  std::vector<InputView> views(n);
  if (res->status) for (u32 q = 0; q < R; ++q) { const u32 o0 = RQ(RQ_ACT_OFF, q), c = RQ(RQ_ACT_CNT, q); for (u32 k = 0; k < c; ++k) if (res->status[o0 + k] == CBH_ST_UNSUPPORTED) flags[b->req_input[q]] |= CBI_TRACE_ERRORS_INCOMPLETE | CBI_TRACE_OUTPUTS_INCOMPLETE; }
  for (u32 x = 0; x < count; ++x) {
    const uint32_t* rec = records + (size_t)x * CBH_TRACE_RECORD_WORDS;
    const u32 q = rec[0], w1 = rec[1], w2 = rec[2], w3 = rec[3], kind = w1 & 0xF;
    if (q >= R) return fail("trace record refers to a request outside the batch");
    const u32 i = b->req_input[q];
    if (!have_view[i]) { view_of(i, views[i]); have_view[i] = 1; }
    const InputView& msg = views[i];
    try {
      if (kind == CBH_TR_INCOMPLETE) flags[i] |= CBI_TRACE_OUTPUTS_INCOMPLETE;
      else if (kind == CBH_TR_ERROR) {
        if (w2 >= t->trace_strings.size()) return fail("trace record refers to an unknown string");
        errs[i].emplace(t->trace_strings[w2], message((u64)rec[4] | ((u64)rec[5] << 32), msg));
      } else if (kind == CBH_TR_OUTPUT || kind == CBH_TR_OUTPUT_ERROR || kind == CBH_TR_OUTPUT_ELEMENT) {
        const u32 rule = kind != CBH_TR_OUTPUT_ERROR ? (w3 >> 8) : rec[4];
        Visit& v = visits[i][Key{q, (w1 >> 4) & 1, (w1 >> 12) & 0xFF, w1 >> 20, rule}];
        const u32 part = (w1 >> 6) & 63;
        v.src = w2; v.drfail = (w1 & 32u) != 0;
        if (kind == CBH_TR_OUTPUT_ELEMENT) { v.elems[part][rec[6]] = to_tval(w3 & 0xFF, (u64)rec[4] | ((u64)rec[5] << 32), 1); continue; }
        v.mask = (u64)rec[6] | ((u64)rec[7] << 32);
        if (kind == CBH_TR_OUTPUT) v.ok_parts[part] = {true, to_tval(w3 & 0xFF, (u64)rec[4] | ((u64)rec[5] << 32), 0)};
        else v.err_parts[part] = message((u64)w3 | ((u64)rec[5] << 32), msg);
      }
    } catch (const TraceIncomplete&) { flags[i] |= kind == CBH_TR_ERROR ? CBI_TRACE_ERRORS_INCOMPLETE : CBI_TRACE_OUTPUTS_INCOMPLETE; }
  }

  auto o = std::make_unique<cbi_outputs>();
  o->offsets.reserve((size_t)n + 1); o->offsets.push_back(0); o->flags = flags;
  std::vector<u8>& ob = o->bytes;
  struct Entry { u64 a; u32 pass, ri, site; bool drfail; u32 rule; std::vector<u8> body; std::string_view action; };
  for (u32 i = 0; i < n; ++i) {
    // outputs (field 6), in the order check.go's loops reach them: action, policy kind, role, rule
    if (!visits[i].empty() && !have_view[i]) { view_of(i, views[i]); have_view[i] = 1; }
    const std::vector<std::string_view>& actions = views[i].actions;
    std::vector<Entry> entries;
    for (auto& kv : visits[i]) {
      const Key& key = kv.first; Visit& v = kv.second;
      auto tm = t->trace_templates.find(key.rule);
      if (tm == t->trace_templates.end() || v.src >= t->trace_strings.size()) return fail("trace record refers to an unknown output");
      std::vector<u8> body;
      put_ld(body, 1, t->trace_strings[v.src]);
      bool lost = false;
      try {
        if (v.ok_parts.size() + v.err_parts.size() != tm->second.second) throw TraceIncomplete{};
        if (!v.err_parts.empty()) put_ld(body, 4, v.err_parts.begin()->second);   // the first part to fail in evaluation order
        else {
          std::vector<TVal> holes;
          for (auto& pk : v.ok_parts) {
            if (pk.first != holes.size()) throw TraceIncomplete{};
            TVal hv = pk.second.second;
            if (hv.local) {   // its elements were logged one by one
              const auto& el = v.elems[pk.first];
              if (el.size() != (size_t)hv.i) throw TraceIncomplete{};
              hv.local = false;
              u32 want = 0;
              for (const auto& ek : el) { if (ek.first != want++ || ek.second.local) throw TraceIncomplete{}; hv.items.push_back(ek.second); }
            }
            holes.push_back(std::move(hv));
          }
          std::vector<u8> vb; put_value(vb, assemble_template(tm->second.first, holes));
          put_msg(body, 2, vb);
        }
      } catch (const TraceIncomplete&) { lost = true; }
      if (lost) { o->flags[i] |= CBI_TRACE_OUTPUTS_INCOMPLETE; continue; }
      const u32 o0 = RQ(RQ_ACT_OFF, key.q), cnt = RQ(RQ_ACT_CNT, key.q);
      for (u32 k = 0; k < cnt && k < 64; ++k) if ((v.mask >> k) & 1) {
        const u64 tp = b->tuple_perm[o0 + k];
        if (tp < first[i] || tp >= first[i + 1] || tp - first[i] >= actions.size()) return fail("batch does not belong to these inputs");
        entries.push_back(Entry{tp - first[i], key.pass, key.ri, key.site, v.drfail, key.rule & 0x7FFFFFu, body, actions[tp - first[i]]});
      }
    }
    std::stable_sort(entries.begin(), entries.end(), [](const Entry& x, const Entry& y) { return std::tie(x.a, x.pass, x.ri, x.site) < std::tie(y.a, y.pass, y.ri, y.site); });
    std::set<u32> seen_drfail;
    for (Entry& e : entries) {
      // the first visit of a rule whose derived-role condition fails emits nothing (check.go:343-347 caches "false" under the
      // evaluation key and moves on); later visits find the cached outcome and emit conditionNotMet
      if (e.drfail && seen_drfail.insert(e.rule).second) continue;
      put_ld(e.body, 3, e.action);
      put_msg(ob, 6, e.body);
    }
    // evaluation_errors (field 7), sorted and deduplicated as CELErrors.All() (cel_errors.go:98-118)
    for (const auto& em : errs[i]) {
      std::vector<u8> ce; put_str(ce, 1, em.first); put_str(ce, 2, em.second);
      std::vector<u8> ee; put_msg(ee, 1, ce);
      put_msg(ob, 7, ee);
    }
    o->offsets.push_back(ob.size());
  }
  ob.reserve(1);
  *out = o.release();
  return 0;
}
}  // namespace

extern "C" {
int cbi_trace_pb(const cbi_table* t, const cbi_batch* b, const cbh_result* res, const uint32_t* records, uint32_t count,
                 const uint8_t* bytes, const uint64_t* offsets, uint32_t n, cbi_outputs** out) {
  if (!t || !b || !res || !out || (count && !records) || (n && (!bytes || !offsets))) return fail("cbi_trace_pb: null argument");
  return trace_decode(t, b, res, records, count, n, [&](u32 i, InputView& v) {
    bool bad = false;
    read_check_input(Span{bytes + offsets[i], bytes + offsets[i + 1]}, v, v.actions, bad);
  }, out);
}

// The same for the batch cbi_flatten_request_pb made of ONE CheckResourcesRequest: input i = its i-th resource entry, the principal
// is the request's, the auxiliary data what the caller passed to the flattener.
int cbi_trace_request_pb(const cbi_table* t, const cbi_batch* b, const cbh_result* res, const uint32_t* records, uint32_t count,
                         const uint8_t* request, uint64_t request_len, const uint8_t* aux_data, uint64_t aux_len, cbi_outputs** out) {
  if (!t || !b || !res || !out || (count && !records) || !request) return fail("cbi_trace_request_pb: null argument");
  RequestParts rp;
  if (!split_request(request, request_len, rp)) return fail("malformed CheckResourcesRequest");
  const Span aux = aux_data ? Span{aux_data, aux_data + aux_len} : Span{nullptr, nullptr};
  return trace_decode(t, b, res, records, count, (u32)rp.entries.size(), [&](u32 i, InputView& v) {
    bool bad = false;
    v.principal = rp.principal; v.aux = aux;
    read_entry(rp.entries[i], v.resource, v.actions, bad);
  }, out);
}
}  // extern "C"
