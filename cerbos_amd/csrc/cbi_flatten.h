// cbi_flatten.h - serialized CheckInputs, or the resource entries of one CheckResourcesRequest, -> cbi_batch: interning, attribute
// columns, slices on threads and their merge, the routing sort (part of cbh_ingest.cpp).
#pragma once

struct cbi_batch {
  cbh_batch view{};
  std::vector<u32> req, roles, tuple_req, tuple_action, str_off, req_input;
  std::vector<u8> col_tag, heap_tag, str_bytes, str_flags;
  std::vector<u64> col_val, heap_val, tuple_perm;
  std::vector<u64> str_hash;   // hash_bytes of each batch-local string (merge of slices)
  // Where the strings the response needs sit in each CheckInput (offset, length relative to the message; CheckInput source only):
  // per input IN_SPAN_N pairs - request id, principal id / version, resource kind / version / id - and per input-order tuple
  // its action.  cbi_assemble_pb then reads them instead of walking every message a second time.
  std::vector<u32> in_span, act_span;
  std::string_view local(u32 j) const { return std::string_view((const char*)str_bytes.data() + str_off[j], str_off[j + 1] - str_off[j]); }   // batch-local string j
};

namespace {
enum { SPAN_REQUEST_ID, SPAN_P_ID, SPAN_P_VERSION, SPAN_R_KIND, SPAN_R_VERSION, SPAN_R_ID, IN_SPAN_N };
enum { T_NULL = 0, T_BOOL = 1, T_DOUBLE = 4, T_STRING = 5, T_LIST = 6, T_MAP = 7, T_ABSENT = 0xF0, T_ERR = 0xFF };
enum { RQ_PRINCIPAL_ID, RQ_P_SCOPE, RQ_P_VERSION, RQ_KIND, RQ_R_SCOPE, RQ_R_VERSION, RQ_ROLE_OFF, RQ_ROLE_CNT, RQ_ACT_OFF, RQ_ACT_CNT,
       RQ_S_RESOURCE_ID, RQ_S_KIND, RQ_S_P_SCOPE, RQ_S_R_SCOPE, RQ_S_P_VERSION, RQ_S_R_VERSION, RQ_N };
static_assert(RQ_ACT_OFF == CBH_RQ_ACT_OFF && RQ_S_R_VERSION == CBH_RQ_S_R_VERSION && RQ_N == CBH_RQ_NFIELDS, "field order of include/cerbos_hip.h");
constexpr u32 MAX_ACTIONS = 64;
constexpr u32 SF_ACTION = 1, SF_ROLE = 2, SF_KIND = 4;

// ---- parts of a call with n_threads > 1.  base[k] .. base[k + 1] = the inputs of part k: at most 64 parts and none below 1024
// inputs (not worth a thread), else a single one. ----
std::vector<u32> split_parts(u32 n, int n_threads) {
  u32 P = n_threads > 1 ? std::min(64u, (u32)n_threads) : 1u;
  if (n < 1024u * P) P = n / 1024u ? n / 1024u : 1u;
  std::vector<u32> base(P + 1);
  for (u32 k = 0; k <= P; ++k) base[k] = (u32)((u64)n * k / P);
  return base;
}
// fn(0) .. fn(P - 1), one thread each; a single one runs on the caller's.
template <class F> void fan_out(u32 P, F&& fn) {
  if (P == 1) { fn(0u); return; }
  std::vector<std::thread> th;
  for (u32 k = 0; k < P; ++k) th.emplace_back([&fn, k]() { fn(k); });
  for (auto& x : th) x.join();
}
// The same for parts that can fail: part(k, err) returns 0 or leaves its text in err.  -> the first failing part (its text in `err`), or -1.
template <class F> int run_parts(u32 P, F&& part, std::string& err) {
  std::vector<std::string> errs(P); std::vector<int> rcs(P, 0);
  fan_out(P, [&](u32 k) { rcs[k] = part(k, errs[k]); });
  for (u32 k = 0; k < P; ++k) if (rcs[k] != 0) { err = std::move(errs[k]); return (int)k; }
  return -1;
}

struct Interner {
  const cbi_table* t;
  cbi_batch* b;
  StrIndex local;
  // A small direct-mapped cache in front of the two dictionaries: the vocabularies that repeat from message to message - actions,
  // roles, enum-like attribute values - are answered by one probe and one short compare.  Entries point into the caller's message
  // bytes (valid for the whole call); `flags` = the CBH_SF_* bits already recorded for the string.
  struct CacheEnt { const char* p = nullptr; u32 len = 0, id = 0, flags = 0; u64 key = 0; };
  CacheEnt cache[256];
  u32 sid(std::string_view s, u32 flag = 0) {
    u64 w = 0;
    if (!s.empty()) memcpy(&w, s.data(), s.size() < 8 ? s.size() : 8);
    const u64 key = (w ^ ((u64)s.size() << 56)) * 0x9E3779B97F4A7C15ull;
    CacheEnt& e = cache[key >> 56];
    if (e.key == key && e.len == s.size() && e.p && (e.flags & flag) == flag && (s.size() <= 8 || memcmp(e.p, s.data(), s.size()) == 0)) return e.id;
    const u32 id = sid_slow(s, flag);
    if (e.key == key && e.len == s.size() && e.id == id) e.flags |= flag; else e = CacheEnt{s.data(), (u32)s.size(), id, flag, key};
    return id;
  }
  u32 sid_slow(std::string_view s, u32 flag) {
    const u64 h = hash_bytes(s);
    u32 id;
    if (t->ids.find(s, h, [this](u32 i) { return t->at(i); }, id)) return id;
    if (local.find(s, h, [this](u32 i) { return b->local(i); }, id)) {
      if (flag) b->str_flags[id] |= (u8)flag;
    } else {
      id = (u32)b->str_flags.size();
      b->str_bytes.insert(b->str_bytes.end(), s.begin(), s.end());
      b->str_off.push_back((u32)b->str_bytes.size());
      b->str_flags.push_back((u8)flag);
      b->str_hash.push_back(h);
      local.insert(h, id);
    }
    return t->K + id;
  }
  // Same, through a one-entry memo: request fields that rarely change from one message to the next
  // (versions, scopes, kind) skip the hash.  The views stay valid for the whole call.
  struct Memo { std::string_view s; u32 id = 0; bool set = false; };
  Memo memo[8];
  u32 sid_memo(u32 slot, std::string_view s, u32 flag = 0) {
    Memo& m = memo[slot];
    if (m.set && m.s == s) return m.id;
    m.s = s; m.id = sid(s, flag); m.set = true;
    return m.id;
  }
};

struct TV { u8 tag; u64 val; };

struct Encoder {
  Interner& in;
  cbi_batch* b;
  bool bad = false;
  int depth = 0;

  u64 container(u32 off, size_t n) { return ((u64)1 << 62) | ((u64)off << 32) | (u64)n; }
  // `items` appended to the batch heap as one tape: a list of items.size() values, or a map of half as many (key, value) pairs
  TV tape(u8 tag, const std::vector<TV>& items) {
    const u32 off = (u32)b->heap_tag.size();
    for (const TV& x : items) { b->heap_tag.push_back(x.tag); b->heap_val.push_back(x.val); }
    return TV{tag, container(off, tag == T_MAP ? items.size() / 2 : items.size())};
  }

  // (key, value) pairs as a map with ONE entry per key: of a key the wire repeats, the last entry is the map's, as protobuf maps decode
  // (the constant paths read it so: map_get, cbi_pb.h).  The earlier entries leave only what their values put on the heap before, which
  // nothing points at.
  TV map_tape(std::vector<TV>& ents) {
    const size_t n = ents.size() / 2;
    bool repeated = false;
    if (n <= 16) {   // the common map: a few compares, no allocation
      for (size_t i = 1; i < n && !repeated; ++i) for (size_t j = 0; j < i; ++j) if (ents[2 * j].val == ents[2 * i].val) { repeated = true; break; }
    } else {
      std::vector<u64> keys(n);
      for (size_t i = 0; i < n; ++i) keys[i] = ents[2 * i].val;
      std::sort(keys.begin(), keys.end());
      repeated = std::adjacent_find(keys.begin(), keys.end()) != keys.end();
    }
    if (repeated) {
      std::unordered_map<u64, size_t> last;
      for (size_t i = 0; i < n; ++i) last[ents[2 * i].val] = i;
      size_t w = 0;
      for (size_t i = 0; i < n; ++i) if (last[ents[2 * i].val] == i) { ents[2 * w] = ents[2 * i]; ents[2 * w + 1] = ents[2 * i + 1]; ++w; }
      ents.resize(2 * w);
    }
    return tape((u8)T_MAP, ents);
  }

  // entries of a map<string, Value> field `fnum` of `msg`, children first, then the (key, value) pairs
  TV enc_map(Span msg, u32 fnum) {
    std::vector<TV> ents;
    Field f;
    while (next(msg, f, bad)) {
      if (f.num != fnum || f.wt != 2) continue;
      Entry en;
      if (!entry(f.s, en, bad)) break;
      ents.push_back(TV{(u8)T_STRING, in.sid(sv(en.key))});
      ents.push_back(enc(en.val));
    }
    return map_tape(ents);
  }

  TV enc(Span m) {
    Val v;
    if (!value(m, v, bad)) return TV{(u8)T_NULL, 0};
    switch (v.kind) {
      case 1: return TV{(u8)T_NULL, 0};
      case 2: return TV{(u8)T_DOUBLE, v.v};                 // structpb: every number is a double
      case 3: return TV{(u8)T_STRING, in.sid(sv(v.s))};
      case 4: return TV{(u8)T_BOOL, v.v ? 1u : 0u};
      case 5: {
        if (++depth > 100) { bad = true; return TV{(u8)T_NULL, 0}; }
        TV r = enc_map(v.s, 1);
        --depth;
        return r;
      }
      default: {  // 6: ListValue.values = 1
        if (++depth > 100) { bad = true; return TV{(u8)T_NULL, 0}; }
        std::vector<TV> vals;
        Span l = v.s; Field f;
        while (next(l, f, bad)) if (f.num == 1 && f.wt == 2) vals.push_back(enc(f.s));
        --depth;
        return tape((u8)T_LIST, vals);
      }
    }
  }
};
// Where the inputs come from: serialized CheckInputs (bytes + offsets), or the resource entries of ONE serialized
// CheckResourcesRequest, which share its principal and the caller's (verified) auxiliary data - the CheckInputs
// svc.CheckResources would build from it (cerbos_svc.go:274-287), without building them.
struct Source {
  const uint8_t* bytes = nullptr; const uint64_t* offsets = nullptr;
  bool request = false; Span principal{nullptr, nullptr}, aux{nullptr, nullptr};
  Span globals{nullptr, nullptr};   // the call's globals as a serialized google.protobuf.Struct (columns of root 4), or empty
  const Span* entries = nullptr;   // CheckResourcesRequest.ResourceEntry messages: actions = 1, resource = 2
};

// Flattens inputs [first, first + n) of `src` into `b` in input order: no routing sort, no view; req_input holds
// slice-local indices.
int flatten_slice(const cbi_table* t, const Source& src, uint32_t first, uint32_t n, std::string_view dver,
                         std::string_view dscope, cbi_batch* b, std::string& err) {
  const uint8_t* bytes = src.bytes;
  const uint64_t* offsets = src.request ? nullptr : src.offsets + first;
  auto bail = [&](const std::string& m) { err = m; return -1; };
  const u32 ncol = (u32)t->columns.size();

  // pass 1: count device requests (a CheckInput with > 64 actions becomes several) and tuples
  u64 nreq = 0, ntup = 0;
  const u32 action_field = src.request ? 1u : 4u;
  for (u32 i = 0; i < n; ++i) {
    if (!src.request && offsets[i + 1] < offsets[i]) return bail("offsets must not decrease");
    Span m = src.request ? src.entries[first + i] : Span{bytes + offsets[i], bytes + offsets[i + 1]};
    Field f; bool bad = false; size_t na = 0;
    while (next(m, f, bad)) na += (f.num == action_field && f.wt == 2);
    if (bad) return bail("malformed CheckInput at index " + std::to_string(i));
    nreq += na ? (na + MAX_ACTIONS - 1) / MAX_ACTIONS : 1;
    ntup += na;
  }
  if (nreq > 0xFFFFFFFFull || ntup > 0xFFFFFFFFull) return bail("batch too large");
  const u32 R = (u32)nreq;
  b->req.assign((size_t)RQ_N * R, 0);
  b->col_tag.assign((size_t)ncol * R, (u8)T_ABSENT);
  b->col_val.assign((size_t)ncol * R, 0);
  b->req_input.reserve(R);
  b->tuple_req.reserve(ntup); b->tuple_action.reserve(ntup);
  b->str_off.reserve((size_t)n * 2 + 64); b->str_flags.reserve((size_t)n * 2 + 64); b->str_hash.reserve((size_t)n * 2 + 64);
  b->roles.reserve((size_t)n * 3);
  if (!src.request) { b->in_span.resize((size_t)n * 2 * IN_SPAN_N); b->act_span.resize((size_t)ntup * 2); }
  size_t act_at = 0;   // next slot of act_span
  b->str_off.push_back(0);
  b->str_bytes.reserve((size_t)n * 24 + (1 << 12));
  Interner in{t, b, {}, {}};
  in.local.reserve(n);
  Encoder encd{in, b};
  ScopeCache scopes;
  Interner::Memo scope_memos[2];
  auto RQ = [&](u32 f, u32 r) -> u32& { return b->req[(size_t)f * R + r]; };

  // per message scratch, reused
  std::vector<std::string_view> actions, roles;
  std::vector<std::pair<std::string_view, u32>> prev_roles, prev_actions;
  std::vector<Entry> attrs[5];   // entries of Principal.attr / Resource.attr / AuxData.jwt, wire order; [4]: the call's globals (once)
  std::string kind_buf;
  bool need_root[5] = {false, false, false, false, false};
  for (const Column& c : t->columns) need_root[c.root] = true;
  if (need_root[4]) {   // EvalParams.Globals (evaluator.go:52-57): Struct.fields = 1
    bool bad = false;
    read_map(src.globals, 1, attrs[4], bad);
    if (bad) return bail("malformed globals");
  }

  u32 r = 0;
  for (u32 i = 0; i < n; ++i) {
    CheckInputView m;
    actions.clear(); roles.clear();
    for (int a = 0; a < 3; ++a) attrs[a].clear();
    bool bad = false;
    if (src.request) { m.principal = src.principal; m.aux = src.aux; read_entry(src.entries[first + i], m.resource, actions, bad); }
    else read_check_input(Span{bytes + offsets[i], bytes + offsets[i + 1]}, m, actions, bad);
    PrincipalView P; ResourceView Rs;
    read_principal(m.principal, P, bad, &roles, need_root[0] ? &attrs[0] : nullptr);
    read_resource(m.resource, Rs, bad, need_root[1] ? &attrs[1] : nullptr);
    if (need_root[2]) read_map(m.aux, 1, attrs[2], bad);   // AuxData.jwt
    if (bad) return bail("malformed CheckInput at index " + std::to_string(i));
    if (!src.request) {
      const char* base0 = (const char*)(bytes + offsets[i]);
      u32* sp = b->in_span.data() + (size_t)i * 2 * IN_SPAN_N;
      auto span = [&](u32 which, std::string_view v) { sp[2 * which] = v.empty() ? 0u : (u32)(v.data() - base0); sp[2 * which + 1] = (u32)v.size(); };
      span(SPAN_REQUEST_ID, m.request_id); span(SPAN_P_ID, P.id); span(SPAN_P_VERSION, P.version); span(SPAN_R_KIND, Rs.kind);
      span(SPAN_R_VERSION, Rs.version); span(SPAN_R_ID, Rs.id);
      u32* ap = b->act_span.data() + act_at;
      for (std::string_view a : actions) { *ap++ = a.empty() ? 0u : (u32)(a.data() - base0); *ap++ = (u32)a.size(); }
      act_at += 2 * actions.size();
    }
    const size_t na = actions.size();
    const size_t nchunks = na ? (na + MAX_ACTIONS - 1) / MAX_ACTIONS : 1;
    for (size_t ch = 0; ch < nchunks; ++ch, ++r) {
      b->req_input.push_back(i);
      std::string_view p_scope = scope_value(P.scope.empty() ? dscope : P.scope);
      std::string_view r_scope = scope_value(Rs.scope.empty() ? dscope : Rs.scope);
      std::string_view p_ver = P.version.empty() ? dver : P.version;
      std::string_view r_ver = Rs.version.empty() ? dver : Rs.version;
      RQ(RQ_PRINCIPAL_ID, r) = in.sid(P.id);
      auto scope_memo = [&](u32 slot, std::string_view sc) {   // scopes rarely change from one message to the next
        Interner::Memo& mk = scope_memos[slot];
        if (!(mk.set && mk.s == sc)) { mk.s = sc; mk.id = scope_word(t, scopes, sc); mk.set = true; }
        return mk.id;
      };
      RQ(RQ_P_SCOPE, r) = scope_memo(0, p_scope);
      RQ(RQ_P_VERSION, r) = in.sid_memo(0, p_ver);
      { Interner::Memo& mk = in.memo[1];   // keyed by the raw kind, holds the id of the sanitised one
        if (!(mk.set && mk.s == Rs.kind)) { mk.s = Rs.kind; const std::string_view sk = sanitize(Rs.kind, kind_buf);
          // a rewritten kind lives in the reused scratch string, not in the message bytes: it must never enter the cache
          // in front of the dictionaries (whose entries point at what they were made from)
          mk.id = sk.data() == Rs.kind.data() ? in.sid(sk, SF_KIND) : in.sid_slow(sk, SF_KIND); mk.set = true; }
        RQ(RQ_KIND, r) = mk.id; }
      RQ(RQ_R_SCOPE, r) = scope_memo(1, r_scope);
      RQ(RQ_R_VERSION, r) = in.sid_memo(2, r_ver);
      RQ(RQ_ROLE_OFF, r) = (u32)b->roles.size();
      RQ(RQ_ROLE_CNT, r) = (u32)roles.size();
      // role and action lists repeat from one message to the next: try the previous message's string at the same
      // position before hashing (the id already carries the role / action flag from when it was interned that way)
      auto sid_at = [&](std::vector<std::pair<std::string_view, u32>>& prev, size_t x, std::string_view s, u32 flag) {
        if (x >= prev.size()) prev.emplace_back(std::string_view(), 0u);
        auto& pr = prev[x];
        if (!(pr.first.data() && pr.first == s)) { pr.first = s; pr.second = in.sid(s, flag); }
        return pr.second;
      };
      for (size_t x = 0; x < roles.size(); ++x) b->roles.push_back(sid_at(prev_roles, x, roles[x], SF_ROLE));
      RQ(RQ_S_RESOURCE_ID, r) = in.sid(Rs.id);
      RQ(RQ_S_KIND, r) = in.sid_memo(3, Rs.kind);
      RQ(RQ_S_P_SCOPE, r) = in.sid_memo(4, scope_value(P.scope));
      RQ(RQ_S_R_SCOPE, r) = in.sid_memo(5, scope_value(Rs.scope));
      RQ(RQ_S_P_VERSION, r) = in.sid_memo(6, P.version);
      RQ(RQ_S_R_VERSION, r) = in.sid_memo(7, Rs.version);
      for (u32 c = 0; c < ncol; ++c) {
        const Column& col = t->columns[c];
        u8 tag = 0; u64 val = 0; bool done = false;
        const size_t nk = col.keys.size();
        Span cur{nullptr, nullptr};
        size_t k = 0;   // keys consumed so far; `cur` is a google.protobuf.Value once k > 0
        if (col.root == 3) {
          // AuxData.jwts (field 2): map<string, JWT>, JWT.claims (field 1): map<string, Value>.  The request view
          // is name -> {"claims": {...}} (check.go:536-554), so the 2nd key of a path must be "claims".
          auto jwt_as_map = [&](Span jwt) {   // {"claims": {...}}: the key is interned before the claims, children first
            const u64 key = in.sid("claims");
            const TV inner = encd.enc_map(jwt, 1);
            return encd.tape((u8)T_MAP, {TV{(u8)T_STRING, key}, inner});
          };
          Span jwt{nullptr, nullptr};
          if (nk == 0) {
            std::vector<TV> ents;
            Span s = m.aux; Field f;
            while (next(s, f, encd.bad)) {
              if (f.num != 2 || f.wt != 2) continue;
              Entry en;
              if (!entry(f.s, en, encd.bad)) break;
              ents.push_back(TV{(u8)T_STRING, in.sid(sv(en.key))});
              ents.push_back(jwt_as_map(en.val));
            }
            const TV tv = encd.map_tape(ents);
            tag = tv.tag; val = tv.val; done = true;
          } else if (!map_get(m.aux, 2, col.keys[0], jwt, encd.bad)) { tag = nk == 1 ? (u8)T_ABSENT : (u8)T_ERR; done = true; }
          else if (nk == 1) { TV tv = jwt_as_map(jwt); tag = tv.tag; val = tv.val; done = true; }
          else if (col.keys[1] != "claims") { tag = nk == 2 ? (u8)T_ABSENT : (u8)T_ERR; done = true; }
          else if (nk == 2) { TV tv = encd.enc_map(jwt, 1); tag = tv.tag; val = tv.val; done = true; }
          else if (!map_get(jwt, 1, col.keys[2], cur, encd.bad)) { tag = nk == 3 ? (u8)T_ABSENT : (u8)T_ERR; done = true; }
          else k = 3;
        } else if (nk == 0) {
          // the whole root map: Principal.attr (4) / Resource.attr (4) / AuxData.jwt (1)
          TV tv = encd.enc_map(col.root == 0 ? m.principal : col.root == 1 ? m.resource : col.root == 4 ? src.globals : m.aux, (col.root == 2 || col.root == 4) ? 1 : 4);
          tag = tv.tag; val = tv.val; done = true;
        } else {
          bool found = false;
          for (const Entry& en : attrs[col.root]) if (sv(en.key) == col.keys[0]) { cur = en.val; found = true; }   // last entry wins
          if (!found) { tag = nk == 1 ? (u8)T_ABSENT : (u8)T_ERR; done = true; }
          k = 1;
        }
        for (; k < nk && !done; ++k) {
          Val v;
          if (!value(cur, v, encd.bad) || v.kind != 5) { tag = (u8)T_ERR; done = true; break; }
          if (!map_get(v.s, 1, col.keys[k], cur, encd.bad)) { tag = (k == nk - 1) ? (u8)T_ABSENT : (u8)T_ERR; done = true; }
        }
        if (!done) { TV tv = encd.enc(cur); tag = tv.tag; val = tv.val; }
        b->col_tag[(size_t)c * R + r] = tag;
        b->col_val[(size_t)c * R + r] = val;
      }
      if (encd.bad) return bail("malformed attribute value at index " + std::to_string(i));
      RQ(RQ_ACT_OFF, r) = (u32)b->tuple_action.size();
      size_t a0 = ch * MAX_ACTIONS, a1 = std::min(na, a0 + MAX_ACTIONS);
      RQ(RQ_ACT_CNT, r) = (u32)(a1 - a0);
      for (size_t a = a0; a < a1; ++a) { b->tuple_req.push_back(r); b->tuple_action.push_back(sid_at(prev_actions, a, actions[a], SF_ACTION)); }
    }
  }
  return 0;
}

// Routing sort (flatten.py sort_batch_by_route): kind, resource version, resource scope, role count,
// order-sensitive signature of the role list; stable.  Fills tuple_perm.
void sort_batch(cbi_batch* b, u32 ncol, bool sort, int n_threads) {
  const u32 R = (u32)b->req_input.size();
  auto RQ = [&](u32 f, u32 r) -> u32& { return b->req[(size_t)f * R + r]; };
  const u32 T = (u32)b->tuple_action.size();
  b->tuple_perm.resize(T);
  std::iota(b->tuple_perm.begin(), b->tuple_perm.end(), (u64)0);
  if (!sort || R < 2) return;
  // Requests fall into few routing groups (distinct kind / version / scope / role list): find the groups with a
  // hash table, order the groups, then place the requests with one stable counting pass - O(R + G log G)
  // instead of a comparison sort of all requests.
  struct Key { u32 kind, ver, scope, cnt; u64 sig; };
  auto key_eq = [](const Key& x, const Key& y) { return x.kind == y.kind && x.ver == y.ver && x.scope == y.scope && x.cnt == y.cnt && x.sig == y.sig; };
  auto key_less = [](const Key& x, const Key& y) { return std::tie(x.kind, x.ver, x.scope, x.cnt, x.sig) < std::tie(y.kind, y.ver, y.scope, y.cnt, y.sig); };
  std::vector<Key> groups;
  std::vector<u32> group_of(R);
  {
    size_t cap = 256;
    std::vector<u32> slots(cap, 0);   // group index + 1
    auto hash = [](const Key& k) {
      u64 h = (u64)k.kind * 0x9E3779B97F4A7C15ull ^ (u64)k.ver * 0xC2B2AE3D27D4EB4Full ^ (u64)k.scope * 0x165667B19E3779F9ull ^ k.sig ^ ((u64)k.cnt << 40);
      h ^= h >> 29; h *= 0xff51afd7ed558ccdull; h ^= h >> 32;
      return (size_t)h;
    };
    for (u32 q = 0; q < R; ++q) {
      const u32 off = RQ(RQ_ROLE_OFF, q), cnt = RQ(RQ_ROLE_CNT, q);
      u64 sg = 0;
      for (u32 k = 0; k < cnt; ++k) sg += ((u64)b->roles[off + k] + 1) * ((u64)k * 0x9E3779B97F4A7C15ull + 0xC2B2AE3D27D4EB4Full);
      const Key key{RQ(RQ_KIND, q), RQ(RQ_R_VERSION, q), RQ(RQ_R_SCOPE, q), cnt, sg};
      if ((groups.size() + 1) * 2 > cap) {   // grow and re-place
        cap *= 4;
        slots.assign(cap, 0);
        for (u32 g = 0; g < groups.size(); ++g) { size_t i = hash(groups[g]) & (cap - 1); while (slots[i]) i = (i + 1) & (cap - 1); slots[i] = g + 1; }
      }
      size_t i = hash(key) & (cap - 1);
      while (slots[i] && !key_eq(groups[slots[i] - 1], key)) i = (i + 1) & (cap - 1);
      if (!slots[i]) { groups.push_back(key); slots[i] = (u32)groups.size(); }
      group_of[q] = slots[i] - 1;
    }
  }
  const u32 G = (u32)groups.size();
  std::vector<u32> by_rank(G);
  std::iota(by_rank.begin(), by_rank.end(), 0u);
  std::sort(by_rank.begin(), by_rank.end(), [&](u32 x, u32 y) { return key_less(groups[x], groups[y]); });
  std::vector<u32> rank(G), start(G + 1, 0);
  for (u32 r = 0; r < G; ++r) rank[by_rank[r]] = r;
  for (u32 q = 0; q < R; ++q) ++start[rank[group_of[q]] + 1];
  for (u32 r = 0; r < G; ++r) start[r + 1] += start[r];
  std::vector<u32> order(R);
  bool identity = true;
  for (u32 q = 0; q < R; ++q) { const u32 pos = start[rank[group_of[q]]]++; order[pos] = q; identity = identity && pos == q; }
  if (identity) return;
  // gather array by array (sequential writes, reads confined to one array at a time); the arrays are independent
  // jobs and go round-robin to the threads of a parallel call
  std::vector<u32> req2((size_t)RQ_N * R), ta(T), tr(T), ri(R), new_off(R + 1, 0);
  std::vector<u8> ct((size_t)ncol * R);
  std::vector<u64> cv((size_t)ncol * R), tp(T);
  const u32* ord = order.data();
  for (u32 q = 0; q < R; ++q) new_off[q + 1] = new_off[q] + RQ(RQ_ACT_CNT, ord[q]);
  const u32 n_jobs = RQ_N + ncol + 1;
  auto job = [&](u32 j) {
    if (j < RQ_N) {
      const u32* src = &b->req[(size_t)j * R]; u32* dst = &req2[(size_t)j * R];
      if (j == RQ_ACT_OFF) { for (u32 q = 0; q < R; ++q) dst[q] = new_off[q]; }
      else for (u32 q = 0; q < R; ++q) dst[q] = src[ord[q]];
    } else if (j < RQ_N + ncol) {
      const u32 c = j - RQ_N;
      const u8* st = &b->col_tag[(size_t)c * R]; u8* dt = &ct[(size_t)c * R];
      const u64* sv_ = &b->col_val[(size_t)c * R]; u64* dv = &cv[(size_t)c * R];
      for (u32 q = 0; q < R; ++q) { dt[q] = st[ord[q]]; dv[q] = sv_[ord[q]]; }
    } else {
      for (u32 q = 0; q < R; ++q) {
        const u32 o = ord[q], s0 = RQ(RQ_ACT_OFF, o), cn = RQ(RQ_ACT_CNT, o);
        u32 pos = new_off[q];
        for (u32 k = 0; k < cn; ++k, ++pos) { ta[pos] = b->tuple_action[s0 + k]; tr[pos] = q; tp[pos] = s0 + k; }
        ri[q] = b->req_input[o];
      }
    }
  };
  const u32 W = n_threads > 1 ? std::min<u32>((u32)n_threads, n_jobs) : 1u;
  fan_out(W, [&](u32 w) { for (u32 j = w; j < n_jobs; j += W) job(j); });
  b->req.swap(req2); b->col_tag.swap(ct); b->col_val.swap(cv);
  b->tuple_action.swap(ta); b->tuple_req.swap(tr); b->tuple_perm.swap(tp); b->req_input.swap(ri);
}

void finish_view(cbi_batch* b, u32 ncol) {
  // never hand out null pointers for empty arrays
  auto nz32 = [](std::vector<u32>& v) { if (v.empty()) v.reserve(1); return v.data(); };
  cbh_batch& v = b->view;
  v.n_requests = (u32)b->req_input.size(); v.n_tuples = (u32)b->tuple_action.size(); v.n_roles = (u32)b->roles.size(); v.n_columns = ncol;
  v.n_strings = (u32)b->str_flags.size(); v.heap_len = (u32)b->heap_tag.size(); v.str_bytes_len = b->str_bytes.size();
  b->heap_tag.reserve(1); b->heap_val.reserve(1); b->str_bytes.reserve(1); b->str_flags.reserve(1);
  b->col_tag.reserve(1); b->col_val.reserve(1); b->tuple_perm.reserve(1); b->req_input.reserve(1);
  v.req_u32 = nz32(b->req); v.roles = nz32(b->roles); v.tuple_req = nz32(b->tuple_req); v.tuple_action = nz32(b->tuple_action);
  v.col_tag = b->col_tag.data(); v.col_val = b->col_val.data(); v.heap_tag = b->heap_tag.data(); v.heap_val = b->heap_val.data();
  v.str_off = b->str_off.data(); v.str_bytes = b->str_bytes.data(); v.str_flags = b->str_flags.data();
}

// Concatenates slice batches (slice k = inputs [base[k], base[k+1])) into one.  A batch-local string keeps
// the id it would have had in a single pass: the merged dictionary takes slice 0's strings, then the
// strings slice 1 saw first, ... - which is first-appearance order over the whole input.  Heap tapes
// and role lists concatenate; only offsets and batch-local ids are rebased.
void merge_slices(const cbi_table* t, const std::vector<std::unique_ptr<cbi_batch>>& parts, const std::vector<u32>& base, cbi_batch* out, int n_threads) {
  const u32 ncol = (u32)t->columns.size(), K = t->K, P = (u32)parts.size();
  std::vector<u32> rb(P + 1, 0), tb(P + 1, 0), hb(P + 1, 0), lb(P + 1, 0);   // request / tuple / heap / role bases
  for (u32 k = 0; k < P; ++k) {
    rb[k + 1] = rb[k] + (u32)parts[k]->req_input.size(); tb[k + 1] = tb[k] + (u32)parts[k]->tuple_action.size();
    hb[k + 1] = hb[k] + (u32)parts[k]->heap_tag.size(); lb[k + 1] = lb[k] + (u32)parts[k]->roles.size();
  }
  const u32 R = rb[P], T = tb[P];
  // Merged dictionary.  The id of a string is its rank in first-appearance order over (slice, position).
  // Finding each string's first appearance is the expensive part (hashing, comparing) and splits by hash:
  // partition p looks only at strings with hash % B == p, so partitions never share a string.  What is left
  // for the serial pass is handing out ids in order and copying the bytes.
  std::vector<std::vector<u32>> remap(P);
  std::vector<std::vector<u64>> owner(P);           // (slice << 32 | position) of the first appearance
  std::vector<std::vector<u8>> oflags(P);           // flags OR-ed over all appearances, kept at the owner
  for (u32 k = 0; k < P; ++k) { const size_t ns = parts[k]->str_flags.size(); remap[k].resize(ns); owner[k].resize(ns); oflags[k] = parts[k]->str_flags; }
  auto str_of = [&](u64 ref) { return parts[ref >> 32]->local((u32)ref); };
  const u32 B = n_threads > 1 ? (u32)n_threads : 1u;
  auto dedupe = [&](u32 part) {
    size_t mine = 0;
    for (u32 k = 0; k < P; ++k) for (u64 h : parts[k]->str_hash) mine += ((h >> 32) % B) == part;
    size_t cap = 64; while (cap < 2 * mine) cap <<= 1;
    struct Slot { u32 h; u32 used; u64 ref; };
    std::vector<Slot> slots(cap, Slot{0, 0, 0});
    for (u32 k = 0; k < P; ++k) {
      const std::vector<u64>& hs = parts[k]->str_hash;
      for (u32 j = 0; j < hs.size(); ++j) {
        const u64 h = hs[j];
        if (((h >> 32) % B) != part) continue;
        const u64 ref = ((u64)k << 32) | j;
        size_t i = (size_t)h & (cap - 1);
        for (;; i = (i + 1) & (cap - 1)) {
          Slot& sl = slots[i];
          if (!sl.used) { sl = Slot{(u32)h, 1, ref}; owner[k][j] = ref; break; }
          if (sl.h == (u32)h && str_of(sl.ref) == str_of(ref)) {
            owner[k][j] = sl.ref;
            oflags[sl.ref >> 32][(u32)sl.ref] |= parts[k]->str_flags[j];
            break;
          }
        }
      }
    }
  };
  fan_out(B, dedupe);
  out->str_off.assign(1, 0);
  { size_t bytes = 0, cnt = 0; for (const auto& p : parts) { bytes += p->str_bytes.size(); cnt += p->str_flags.size(); }
    out->str_bytes.reserve(bytes); out->str_off.reserve(cnt + 1); out->str_flags.reserve(cnt); out->str_hash.reserve(cnt); }
  for (u32 k = 0; k < P; ++k) {
    const cbi_batch* p = parts[k].get();
    for (u32 j = 0; j < p->str_flags.size(); ++j) {
      const u64 ow = owner[k][j];
      if (ow == (((u64)k << 32) | j)) {
        remap[k][j] = (u32)out->str_flags.size();
        out->str_bytes.insert(out->str_bytes.end(), p->str_bytes.begin() + p->str_off[j], p->str_bytes.begin() + p->str_off[j + 1]);
        out->str_off.push_back((u32)out->str_bytes.size());
        out->str_flags.push_back(oflags[k][j]);
        out->str_hash.push_back(p->str_hash[j]);
      } else {
        remap[k][j] = remap[ow >> 32][(u32)ow];   // the owner comes earlier in (slice, position) order
      }
    }
  }
  for (u32 k = 0; k < P; ++k) {   // slices hold consecutive inputs: their spans follow each other
    out->in_span.insert(out->in_span.end(), parts[k]->in_span.begin(), parts[k]->in_span.end());
    out->act_span.insert(out->act_span.end(), parts[k]->act_span.begin(), parts[k]->act_span.end());
  }
  out->req.assign((size_t)RQ_N * R, 0);
  out->col_tag.assign((size_t)ncol * R, 0); out->col_val.assign((size_t)ncol * R, 0);
  out->roles.resize(lb[P]); out->tuple_req.resize(T); out->tuple_action.resize(T);
  out->heap_tag.resize(hb[P]); out->heap_val.resize(hb[P]); out->req_input.resize(R);
  static const u32 STRING_FIELDS[] = {RQ_PRINCIPAL_ID, RQ_P_VERSION, RQ_KIND, RQ_R_VERSION, RQ_S_RESOURCE_ID, RQ_S_KIND,
                                      RQ_S_P_SCOPE, RQ_S_R_SCOPE, RQ_S_P_VERSION, RQ_S_R_VERSION};
  auto place = [&](u32 k) {   // slices write disjoint ranges: one thread each
    const cbi_batch* p = parts[k].get();
    const std::vector<u32>& mp = remap[k];
    const u32 r0 = rb[k], nr = rb[k + 1] - rb[k], h0 = hb[k];
    auto sid = [&](u32 id) { return id >= K ? K + mp[id - K] : id; };
    auto val = [&](u8 tag, u64 v) -> u64 {
      if (tag == T_STRING) return sid((u32)v);
      if (tag == T_LIST || tag == T_MAP) return v + ((u64)h0 << 32);   // (HEAP_BATCH << 62) | off << 32 | len
      return v;
    };
    for (u32 f = 0; f < RQ_N; ++f) std::memcpy(&out->req[(size_t)f * R + r0], &p->req[(size_t)f * nr], (size_t)nr * 4);
    for (u32 f : STRING_FIELDS) for (u32 r = 0; r < nr; ++r) { u32& x = out->req[(size_t)f * R + r0 + r]; x = sid(x); }
    for (u32 r = 0; r < nr; ++r) {
      out->req[(size_t)RQ_ROLE_OFF * R + r0 + r] += lb[k]; out->req[(size_t)RQ_ACT_OFF * R + r0 + r] += tb[k];
      out->req_input[r0 + r] = p->req_input[r] + base[k];
    }
    for (size_t i = 0; i < p->roles.size(); ++i) out->roles[lb[k] + i] = sid(p->roles[i]);
    for (size_t i = 0; i < p->tuple_action.size(); ++i) { out->tuple_action[tb[k] + i] = sid(p->tuple_action[i]); out->tuple_req[tb[k] + i] = p->tuple_req[i] + r0; }
    for (u32 c = 0; c < ncol; ++c)
      for (u32 r = 0; r < nr; ++r) {
        const u8 tag = p->col_tag[(size_t)c * nr + r];
        out->col_tag[(size_t)c * R + r0 + r] = tag;
        out->col_val[(size_t)c * R + r0 + r] = val(tag, p->col_val[(size_t)c * nr + r]);
      }
    for (size_t i = 0; i < p->heap_tag.size(); ++i) { out->heap_tag[h0 + i] = p->heap_tag[i]; out->heap_val[h0 + i] = val(p->heap_tag[i], p->heap_val[i]); }
  };
  fan_out(P, place);
}

int flatten_source(const cbi_table* t, const Source& src, uint32_t n, const char* default_version, const char* default_scope,
                          int sort, int n_threads, cbi_batch** out) {
  const std::string_view dver = default_version ? default_version : "default";
  const std::string_view dscope = default_scope ? default_scope : "";
  const u32 ncol = (u32)t->columns.size();
  const std::vector<u32> base = split_parts(n, n_threads); const u32 P = (u32)base.size() - 1;
  auto b = std::make_unique<cbi_batch>();
  std::vector<std::unique_ptr<cbi_batch>> parts(P);   // the slices of a call cut into parts; a single part is flattened straight into b
  if (P > 1) for (auto& p : parts) p = std::make_unique<cbi_batch>();
  std::string err;
  const int bad = run_parts(P, [&](u32 k, std::string& e) {
    return flatten_slice(t, src, base[k], base[k + 1] - base[k], dver, dscope, P > 1 ? parts[k].get() : b.get(), e); }, err);
  if (bad >= 0) return fail(P > 1 ? err + " (slice starting at message " + std::to_string(base[bad]) + ")" : err);
  if (P > 1) { merge_slices(t, parts, base, b.get(), (int)P); parts.clear(); }
  if (b->heap_tag.size() >= ((size_t)1 << 30)) return fail("batch too large: nested attribute values exceed the heap's 30-bit offsets");
  sort_batch(b.get(), ncol, sort != 0, (int)P);
  finish_view(b.get(), ncol);
  *out = b.release();
  return 0;
}

// The resource entries (field 4) of a CheckResourcesRequest, its principal (3), request id (1), include_meta (2).
// Scalars: the last occurrence wins.  The principal and an entry's resource are MESSAGE fields: protobuf merges their occurrences
// (what proto.Unmarshal did to the request the server validated and logged), and parsing the concatenation of their bytes is that
// merge - so a request that is not canonical in this way is read through a canonical copy (`owned`: the occurrences back to back),
// as the device road's split does (cbh_wire_req.h).
struct RequestParts {
  std::vector<Span> entries; Span principal{nullptr, nullptr}; std::string_view request_id; bool include_meta = false;
  std::vector<std::vector<u8>> owned;   // (an inner vector's bytes stay where they are when the outer one grows)
};
bool split_request(const uint8_t* request, uint64_t len, RequestParts& rp) {
  Span s{request, request + len}; Field f; bool bad = false;
  u32 n_principal = 0;
  while (next(s, f, bad)) {
    if (f.num == 2 && f.wt == 0) rp.include_meta = f.v != 0;
    if (f.wt != 2) continue;
    if (f.num == 1) rp.request_id = sv(f.s); else if (f.num == 3) { rp.principal = f.s; ++n_principal; } else if (f.num == 4) rp.entries.push_back(f.s);
  }
  if (bad) return false;
  if (n_principal > 1) {
    std::vector<u8> all;
    s = Span{request, request + len};
    while (next(s, f, bad)) if (f.wt == 2 && f.num == 3) all.insert(all.end(), f.s.p, f.s.e);
    rp.owned.push_back(std::move(all));
    rp.principal = Span{rp.owned.back().data(), rp.owned.back().data() + rp.owned.back().size()};
  }
  for (Span& e : rp.entries) {
    u32 n_res = 0;
    { Span t = e; while (next(t, f, bad)) n_res += (f.wt == 2 && f.num == 2); }
    if (bad) return false;
    if (n_res <= 1) continue;
    std::vector<u8> canon, res;   // the entry's other fields as they are, then ONE resource made of all its occurrences
    Span t = e;
    for (;;) {
      const u8* start = t.p;
      if (!next(t, f, bad)) break;
      if (f.wt == 2 && f.num == 2) res.insert(res.end(), f.s.p, f.s.e); else canon.insert(canon.end(), start, t.p);
    }
    put_msg(canon, 2, res);
    rp.owned.push_back(std::move(canon));
    e = Span{rp.owned.back().data(), rp.owned.back().data() + rp.owned.back().size()};
  }
  return !bad;
}
}  // namespace

extern "C" {
int cbi_flatten_pb_g(const cbi_table* t, const uint8_t* bytes, const uint64_t* offsets, uint32_t n, const char* default_version,
                     const char* default_scope, const uint8_t* globals_pb, uint64_t globals_len, int sort, int n_threads, cbi_batch** out) {
  if (!t || !out || (n && (!bytes || !offsets)) || (globals_len && !globals_pb)) return fail("cbi_flatten_pb: null argument");
  Source src; src.bytes = bytes; src.offsets = offsets;
  if (globals_len) src.globals = Span{globals_pb, globals_pb + globals_len};
  return flatten_source(t, src, n, default_version, default_scope, sort, n_threads, out);
}

int cbi_flatten_pb_mt(const cbi_table* t, const uint8_t* bytes, const uint64_t* offsets, uint32_t n, const char* default_version,
                      const char* default_scope, int sort, int n_threads, cbi_batch** out) {
  return cbi_flatten_pb_g(t, bytes, offsets, n, default_version, default_scope, nullptr, 0, sort, n_threads, out);
}

int cbi_flatten_request_pb(const cbi_table* t, const uint8_t* request, uint64_t request_len, const uint8_t* aux_data, uint64_t aux_len,
                           const char* default_version, const char* default_scope, int sort, int n_threads, cbi_batch** out) {
  if (!t || !out || !request) return fail("cbi_flatten_request_pb: null argument");
  RequestParts rp;
  if (!split_request(request, request_len, rp)) return fail("malformed CheckResourcesRequest");
  if (rp.entries.size() > 0xFFFFFFFFull) return fail("batch too large");
  Source src; src.request = true; src.principal = rp.principal; src.entries = rp.entries.data();
  if (aux_data) src.aux = Span{aux_data, aux_data + aux_len};
  return flatten_source(t, src, (u32)rp.entries.size(), default_version, default_scope, sort, n_threads, out);
}

int cbi_flatten_pb(const cbi_table* t, const uint8_t* bytes, const uint64_t* offsets, uint32_t n, const char* default_version,
                   const char* default_scope, int sort, cbi_batch** out) {
  return cbi_flatten_pb_mt(t, bytes, offsets, n, default_version, default_scope, sort, 1, out);
}
}  // extern "C"
