// cbi_pb.h - the protobuf wire format as libcerbos_ingest handles it (part of cbh_ingest.cpp): walking a message in place, one reader
// per message the stages look into, and the writers of the assemblers.
#pragma once

namespace {
// ---- protobuf wire walking -------------------------------------------------------------------------
struct Span { const u8* p = nullptr; const u8* e = nullptr; bool empty() const { return p >= e; } };
struct Field { u32 num = 0; u32 wt = 0; u64 v = 0; Span s{}; };   // v: varint / fixed value, s: length-delimited payload

inline bool varint(Span& s, u64& out) {
  if (s.p < s.e && !(*s.p & 0x80)) { out = *s.p++; return true; }   // one byte: every tag and almost every length
  u64 r = 0;
  for (int sh = 0; sh < 64 && s.p < s.e; sh += 7) {
    u8 b = *s.p++;
    r |= (u64)(b & 0x7F) << sh;
    if (!(b & 0x80)) { out = r; return true; }
  }
  return false;
}

// Next field of a message; false at the end or on malformed input (`bad` set).
inline bool next(Span& s, Field& f, bool& bad) {
  if (s.empty()) return false;
  u64 key;
  if (!varint(s, key)) { bad = true; return false; }
  f.num = (u32)(key >> 3); f.wt = (u32)(key & 7);
  if (f.wt == 2) {   // length-delimited first: strings and sub-messages are most of a CheckInput
    u64 n;
    if (!varint(s, n) || n > (u64)(s.e - s.p)) { bad = true; return false; }
    f.s = Span{s.p, s.p + n}; s.p += n; return true;
  }
  switch (f.wt) {
    case 0: if (!varint(s, f.v)) { bad = true; return false; } return true;
    case 1: if (s.e - s.p < 8) { bad = true; return false; } memcpy(&f.v, s.p, 8); s.p += 8; return true;
    case 5: if (s.e - s.p < 4) { bad = true; return false; } { u32 w; memcpy(&w, s.p, 4); f.v = w; } s.p += 4; return true;
    default: bad = true; return false;
  }
}

std::string_view sv(Span s) { return std::string_view((const char*)s.p, (size_t)(s.e - s.p)); }

// map<string, google.protobuf.Value> entry: key = 1, value = 2
struct Entry { Span key{nullptr, nullptr}; Span val{nullptr, nullptr}; };
inline bool entry(Span e, Entry& out, bool& bad) {
  // the shape every encoder writes - key (field 1) then value (field 2), both with one-byte lengths, nothing else - is read
  // without the field loop; anything else takes the general walk below
  {
    const u8* p = e.p; const size_t n = (size_t)(e.e - e.p);
    if (n >= 4 && p[0] == 0x0A && !(p[1] & 0x80)) {
      const size_t kl = p[1];
      if (2 + kl + 2 <= n && p[2 + kl] == 0x12 && !(p[3 + kl] & 0x80) && 4 + kl + (size_t)p[3 + kl] == n) {
        out.key = Span{p + 2, p + 2 + kl};
        out.val = Span{p + 4 + kl, e.e};
        return true;
      }
    }
  }
  Field f;
  while (next(e, f, bad)) {
    if (f.num == 1 && f.wt == 2) out.key = f.s;
    else if (f.num == 2 && f.wt == 2) out.val = f.s;
  }
  return !bad;
}

// The entries of the map field `fnum` of message `msg`, in wire order.
inline void read_map(Span msg, u32 fnum, std::vector<Entry>& out, bool& bad) {
  Field f;
  while (next(msg, f, bad)) if (f.num == fnum && f.wt == 2) { Entry en; if (entry(f.s, en, bad)) out.push_back(en); }
}

// Looks `key` up in the map field `fnum` of message `msg` (last entry wins, as protobuf maps decode).
bool map_get(Span msg, u32 fnum, std::string_view key, Span& val, bool& bad) {
  Field f; bool found = false;
  while (next(msg, f, bad)) {
    if (f.num != fnum || f.wt != 2) continue;
    Entry en;
    if (!entry(f.s, en, bad)) return false;
    if (sv(en.key) == key) { val = en.val; found = true; }
  }
  return found;
}

// google.protobuf.Value oneof: null 1, number 2 (double), string 3, bool 4, struct 5, list 6.  The last
// field present wins; an empty message is null.
struct Val { u32 kind = 1; u64 v = 0; Span s{nullptr, nullptr}; };
inline bool value(Span m, Val& out, bool& bad) {
  // a field counts only with the wire type its declaration has (null / bool: varint, number: fixed64,
  // string / struct / list: length-delimited); anything else is an unknown field, skipped as protobuf does
  static const u8 want_wt[7] = {0xFF, 0, 1, 2, 0, 2, 2};
  // one field filling the whole message - what an encoder writes for a scalar - without the field loop
  {
    const u8* p = m.p; const size_t n = (size_t)(m.e - m.p);
    if (n == 9 && p[0] == 0x11) { out.kind = 2; memcpy(&out.v, p + 1, 8); out.s = Span{}; return true; }                      // number_value
    if (n >= 2 && p[0] == 0x1A && !(p[1] & 0x80) && 2 + (size_t)p[1] == n) { out.kind = 3; out.v = 0; out.s = Span{p + 2, m.e}; return true; }   // string_value
    if (n == 2 && p[0] == 0x20 && !(p[1] & 0x80)) { out.kind = 4; out.v = p[1]; out.s = Span{}; return true; }              // bool_value
  }
  Field f;
  while (next(m, f, bad)) {
    if (f.num >= 1 && f.num <= 6 && f.wt == want_wt[f.num]) {
      out.kind = f.num; out.v = f.wt == 2 ? 0 : f.v; out.s = f.wt == 2 ? f.s : Span{};
    }
  }
  return !bad;
}

// ---- one reader per message: a single walk fills a small record.  Only length-delimited fields count, a repeated scalar field
// keeps its last occurrence, and roles / attribute entries are collected only for a caller that passes where to. ----
struct PrincipalView { std::string_view id, version, scope; };          // Principal: id 1, policy_version 2, roles 3, attr 4, scope 5
struct ResourceView { std::string_view kind, version, id, scope; };     // Resource: kind 1, policy_version 2, id 3, attr 4, scope 5
struct CheckInputView { std::string_view request_id; Span resource{nullptr, nullptr}, principal{nullptr, nullptr}, aux{nullptr, nullptr}; };

inline void read_principal(Span s, PrincipalView& P, bool& bad, std::vector<std::string_view>* roles = nullptr, std::vector<Entry>* attr = nullptr) {
  Field f;
  while (next(s, f, bad)) { if (f.wt != 2) continue;
    if (f.num == 1) P.id = sv(f.s); else if (f.num == 2) P.version = sv(f.s); else if (f.num == 5) P.scope = sv(f.s);
    else if (f.num == 3 && roles) roles->push_back(sv(f.s));
    else if (f.num == 4 && attr) { Entry en; if (entry(f.s, en, bad)) attr->push_back(en); } }
}
inline void read_resource(Span s, ResourceView& Rs, bool& bad, std::vector<Entry>* attr = nullptr) {
  Field f;
  while (next(s, f, bad)) { if (f.wt != 2) continue;
    if (f.num == 1) Rs.kind = sv(f.s); else if (f.num == 2) Rs.version = sv(f.s); else if (f.num == 3) Rs.id = sv(f.s);
    else if (f.num == 5) Rs.scope = sv(f.s);
    else if (f.num == 4 && attr) { Entry en; if (entry(f.s, en, bad)) attr->push_back(en); } }
}
// CheckInput: request_id 1, resource 2, principal 3, actions 4 (appended to `actions`), aux_data 5
inline void read_check_input(Span s, CheckInputView& m, std::vector<std::string_view>& actions, bool& bad) {
  Field f;
  while (next(s, f, bad)) { if (f.wt != 2) continue;
    if (f.num == 2) m.resource = f.s; else if (f.num == 3) m.principal = f.s; else if (f.num == 4) actions.push_back(sv(f.s));
    else if (f.num == 5) m.aux = f.s; else if (f.num == 1) m.request_id = sv(f.s); }
}
// CheckResourcesRequest.ResourceEntry: actions 1 (appended to `actions`), resource 2
inline void read_entry(Span s, Span& resource, std::vector<std::string_view>& actions, bool& bad) {
  Field f;
  while (next(s, f, bad)) { if (f.wt != 2) continue; if (f.num == 1) actions.push_back(sv(f.s)); else if (f.num == 2) resource = f.s; }
}

// ---- writing ---------------------------------------------------------------------------------------
inline void put_varint(std::vector<u8>& o, u64 v) { while (v >= 0x80) { o.push_back((u8)(v | 0x80)); v >>= 7; } o.push_back((u8)v); }
inline size_t varint_size(u64 v) { size_t n = 1; while (v >= 0x80) { v >>= 7; ++n; } return n; }
inline size_t ld_size(size_t n) { return 1 + varint_size(n) + n; }   // a length-delimited field (number below 16) of n bytes
inline void put_head(std::vector<u8>& o, u32 field, size_t len) { put_varint(o, (u64)field << 3 | 2); put_varint(o, len); }
inline void put_ld(std::vector<u8>& o, u32 field, std::string_view s) { put_head(o, field, s.size()); o.insert(o.end(), s.begin(), s.end()); }
inline void put_str(std::vector<u8>& o, u32 field, std::string_view s) { if (!s.empty()) put_ld(o, field, s); }   // proto3 default: omitted
inline void put_msg(std::vector<u8>& o, u32 field, const std::vector<u8>& body) { put_ld(o, field, std::string_view((const char*)body.data(), body.size())); }

// The same three operations over reserved memory, for cbi_assemble_pb's pass over every action of a batch (tools/ingest_microbench.cpp
// measures it).  The caller reserves by action_entry_bound and asserts after an entry that `w` kept to it (tests/asan/ingest_fuzz.cpp).
struct RawWriter {
  u8* w; const u8* end;
  void varint(u64 v) { while (v >= 0x80) { *w++ = (u8)(v | 0x80); v >>= 7; } *w++ = (u8)v; }
  void ld(u32 field, std::string_view v) { varint((u64)field << 3 | 2); varint(v.size()); if (!v.empty()) { memcpy(w, v.data(), v.size()); w += v.size(); } }
  void str(u32 field, std::string_view v) { if (!v.empty()) ld(field, v); }
};
constexpr size_t LD_OVERHEAD = 6;   // the most a length-delimited field takes besides its payload: a byte of tag, five of a 32-bit length
// The most bytes one actions entry of a CheckOutput takes - {1: name, 2: ActionEffect {1: effect, 2: policy key, 3: scope}}: five such
// fields, the effect's tag and two bytes of value, the strings.  Key and scope are known only once policy_key has run: a reservation
// made before that allows them 224 bytes together, and a writer about to pass it asks again with the real lengths.
inline size_t action_entry_bound(size_t name, size_t key_and_scope = 224) { return 5 * LD_OVERHEAD + 3 + name + key_and_scope; }
}  // namespace
