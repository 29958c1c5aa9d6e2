// cbi_table.h - the host dictionaries of one lowered table image (cbi_table) and the naming rules that read them: scope words,
// sanitised kinds, policy keys (part of cbh_ingest.cpp).
#pragma once

namespace {
// ---- string dictionaries ---------------------------------------------------------------------------------
inline u64 hash_bytes(std::string_view s) {
  const char* p = s.data(); size_t n = s.size();
  u64 h = 0x9E3779B97F4A7C15ull ^ (n * 0xff51afd7ed558ccdull);
  while (n >= 8) { u64 w; memcpy(&w, p, 8); h = (h ^ w) * 0xff51afd7ed558ccdull; h ^= h >> 29; p += 8; n -= 8; }
  if (n) { u64 w = 0; memcpy(&w, p, n); h = (h ^ w) * 0xff51afd7ed558ccdull; h ^= h >> 29; }
  return h ^ (h >> 32);
}

// Open-addressing set of string ids; the strings themselves live wherever `at(id)` finds them.
struct StrIndex {
  struct Slot { u32 h; u32 id1; };   // id1 = id + 1, 0 = empty
  std::vector<Slot> slots;
  u32 used = 0;
  StrIndex() : slots(64, Slot{0, 0}) {}
  template <class At> bool find(std::string_view s, u64 h, At at, u32& id) const {
    const u32 mask = (u32)slots.size() - 1, h32 = (u32)h;
    for (u32 i = h32 & mask;; i = (i + 1) & mask) {
      const Slot& sl = slots[i];
      if (!sl.id1) return false;
      if (sl.h == h32) {
        const std::string_view c = at(sl.id1 - 1);
        if (c.size() == s.size() && (s.empty() || std::memcmp(c.data(), s.data(), s.size()) == 0)) { id = sl.id1 - 1; return true; }
      }
    }
  }
  void insert(u64 h, u32 id) {   // the caller knows the string is absent
    if ((used + 1) * 2 > slots.size()) {
      std::vector<Slot> old(slots.size() * 2, Slot{0, 0});
      old.swap(slots);
      for (const Slot& sl : old) if (sl.id1) place(sl);
    }
    place(Slot{(u32)h, id + 1});
    ++used;
  }
  void reserve(size_t n) {
    size_t want = 64;
    while (want < 4 * n) want *= 2;
    if (want > slots.size() && !used) slots.assign(want, Slot{0, 0});
  }
  void place(Slot s) {
    const u32 mask = (u32)slots.size() - 1;
    u32 i = s.h & mask;
    while (slots[i].id1) i = (i + 1) & mask;
    slots[i] = s;
  }
};
struct Column { u32 root; std::vector<std::string> keys; };

// A CEL value as the trace pass's consumer handles it (cbi_trace_pb): it keeps its CEL type for format().
struct TVal {
  enum Kind { Null, Bool, Int, Double, String, List, Map } k = Null;
  bool b = false; long long i = 0; double d = 0; std::string s;
  std::vector<TVal> items;   // List: the elements; Map: key, value, key, value ...
  bool local = false;        // a list the program built in its lane's arena: i elements, logged as CBH_TR_OUTPUT_ELEMENT records
};
// Template of an output expression (celc.py _output_template; cbh_blob.h CBH_SEC_TRACE_HOST)
struct TNode { u8 kind = 0; u32 hole = 0; TVal cst; std::string fmt; std::vector<TNode> kids; };
}  // namespace

// (a handle of the C interface: a global name, between the types it holds and the functions over it; the library is one translation
// unit, so holding types of the anonymous namespace is sound)
#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC diagnostic ignored "-Wsubobject-linkage"
#endif
struct cbi_table {
  std::vector<u8> blob;
  u32 K = 0;
  const u32* str_off = nullptr;      // table string pool (views into blob)
  const char* str_bytes = nullptr;
  StrIndex ids;                      // table string -> id
  std::unordered_map<std::string, u32> scope_index;    // scope -> index
  std::vector<Column> columns;
  std::vector<std::string> policy_keys, dr_names, scopes;   // response assembly
  // the trace pass (cbi_trace_pb): strings its records refer to, output templates by rule word, the table's constant heap
  std::vector<std::string> trace_strings;
  std::unordered_map<u32, std::pair<TNode, u32>> trace_templates;
  const u8* theap_tag = nullptr; const u64* theap_val = nullptr; u32 theap_len = 0;
  bool has_trace = false, trace_all = false;
  std::string_view at(u32 i) const { return std::string_view(str_bytes + str_off[i], str_off[i + 1] - str_off[i]); }
};

namespace {
constexpr u32 SCOPE_EXACT = 0x80000000u;
// namer.go:276-278
std::string_view scope_value(std::string_view s) { return (!s.empty() && s[0] == '.') ? s.substr(1) : s; }

bool name_char(char c) {
  return (c >= '0' && c <= '9') || (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || c == '_' || c == '@' || c == '.' || c == '-' || c == '/';
}
bool alpha(char c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); }

// namer.go:213-218: a name of the pre-0.30 form (segments "[A-Za-z][0-9A-Za-z_@.\-/]*" joined by ':') has
// every run of characters outside [0-9A-Za-z_.] replaced by one '_'; any other name is kept as it is.
std::string_view sanitize(std::string_view v, std::string& out) {
  bool plain = true;
  for (char c : v) if (!((c >= '0' && c <= '9') || alpha(c) || c == '_' || c == '.')) { plain = false; break; }
  if (plain) return v;   // nothing to rewrite whichever form it is
  bool old_form = !v.empty();
  bool seg_start = true;
  for (char c : v) {
    if (seg_start) { if (!alpha(c)) { old_form = false; break; } seg_start = false; }
    else if (c == ':') seg_start = true;
    else if (!name_char(c)) { old_form = false; break; }
  }
  if (seg_start) old_form = false;
  if (!old_form) return v;
  out.clear(); bool in_run = false;
  for (char c : v) {
    bool ok = (c >= '0' && c <= '9') || alpha(c) || c == '_' || c == '.';
    if (ok) { out.push_back(c); in_run = false; }
    else if (!in_run) { out.push_back('_'); in_run = true; }
  }
  return out;
}
struct ScopeCache {   // scope -> scope word, per call (the table stays immutable and shareable between threads)
  StrIndex index;
  std::vector<std::string> keys;
  std::vector<u32> words;
};

u32 scope_word(const cbi_table* t, ScopeCache& sc, std::string_view scope) {
  const u64 h = hash_bytes(scope);
  u32 slot;
  if (sc.index.find(scope, h, [&sc](u32 i) { return std::string_view(sc.keys[i]); }, slot)) return sc.words[slot];
  std::string key(scope);
  u32 w = 0;
  auto it = t->scope_index.find(key);
  if (it != t->scope_index.end()) w = it->second | SCOPE_EXACT;
  else {
    // namer.go:77-87: "a.b.c" -> "a.b", "a", ""
    for (size_t i = scope.size(); i-- > 0;) {
      if (scope[i] == '.' || i == 0) {
        auto p = t->scope_index.find(std::string(scope.substr(0, i)));
        if (p != t->scope_index.end()) { w = p->second; break; }
      }
    }
  }
  sc.index.insert(h, (u32)sc.keys.size());
  sc.keys.push_back(std::move(key));
  sc.words.push_back(w);
  return w;
}

// Policy key of a device policy word (enum cbh_policy_kind), as namer.PolicyKeyFromFQN gives it (namer.go:95-134).
// Returns an error text, or nullptr.
const char* policy_key(const cbi_table* t, u32 word, const PrincipalView& P, const ResourceView& Rs, std::string_view dver,
                       std::string& pol, std::string& kbuf, std::string& vbuf) {
  const u32 kind = word >> 28, ident = word & 0x0FFFFFFFu;
  pol.clear();
  switch (kind) {
    case CBH_P_EMPTY: return nullptr;
    case CBH_P_NO_MATCH: pol = "NO_MATCH"; return nullptr;
    case CBH_P_NO_MATCH_SCOPE_PERMISSIONS: pol = "NO_MATCH_FOR_SCOPE_PERMISSIONS"; return nullptr;
    case CBH_P_TABLE:
      if (ident >= t->policy_keys.size()) return "policy id out of range";
      pol = t->policy_keys[ident];
      return nullptr;
    case CBH_P_RESOURCE: case CBH_P_PRINCIPAL: {
      if (ident >= t->scopes.size()) return "scope index out of range";
      const bool rp = kind == CBH_P_RESOURCE;
      std::string_view ver = rp ? Rs.version : P.version;
      pol = rp ? "resource." : "principal.";
      pol += sanitize(rp ? Rs.kind : P.id, kbuf); pol += ".v"; pol += sanitize(ver.empty() ? dver : ver, vbuf);
      if (!t->scopes[ident].empty()) { pol += '/'; pol += t->scopes[ident]; }
      return nullptr;
    }
    default: return "unknown policy word";
  }
}
}  // namespace

extern "C" {
int cbi_table_open(const void* blob, size_t len, cbi_table** out) {
  if (!blob || !out) return fail("cbi_table_open: null argument");
  if (len < sizeof(CbhBlobHeader)) return fail("blob too small");
  auto t = std::make_unique<cbi_table>();
  t->blob.assign((const u8*)blob, (const u8*)blob + len);
  const u8* base = t->blob.data();
  auto* h = (const CbhBlobHeader*)base;
  if (h->magic != CBH_BLOB_MAGIC) return fail("bad blob magic");
  if (h->version != CBH_BLOB_VERSION) return fail("blob version mismatch: re-lower the rule table");
  if (h->total_len != len || sizeof(CbhBlobHeader) + (u64)h->n_sections * sizeof(CbhBlobSection) > len) return fail("blob length mismatch");
  auto* secs = (const CbhBlobSection*)(base + sizeof(CbhBlobHeader));
  auto find = [&](u32 id) -> const CbhBlobSection* {
    for (u32 i = 0; i < h->n_sections; ++i)
      if (secs[i].id == id)   // sections are 64-byte aligned and lie inside the image (no wrap-around)
        return (secs[i].offset % 8 == 0 && secs[i].offset <= len && secs[i].nbytes <= len - secs[i].offset) ? &secs[i] : nullptr;
    return nullptr;
  };
  auto names16 = [](const u8*& q, const u8* qe, u32 cnt, std::vector<std::string>& dst) {   // cnt strings, each after its 16-bit length
    for (u32 k = 0; k < cnt; ++k) {
      if (qe - q < 2) return false;
      const u32 l = q[0] | (q[1] << 8); q += 2;
      if ((u32)(qe - q) < l) return false;
      dst.emplace_back((const char*)q, l); q += l;
    }
    return true;
  };
  const CbhBlobSection *so = find(CBH_SEC_STR_OFF), *sb = find(CBH_SEC_STR_BYTES), *ss = find(CBH_SEC_SCOPE_SID), *sc = find(CBH_SEC_COLUMN_PATHS),
                       *sm = find(CBH_SEC_META);
  if (!so || !sb || !ss || !sc || !sm) return fail("blob is missing a section the ingest needs");
  if (sm->nbytes < (u64)CBH_META_N * 4) return fail("META section too short");
  const u32* meta = (const u32*)(base + sm->offset);
  t->K = meta[CBH_M_NSTRINGS];
  if (((u64)t->K + 1) * 4 > so->nbytes) return fail("string offset section too short");
  const u32* off = (const u32*)(base + so->offset);
  const char* bytes = (const char*)(base + sb->offset);
  if (off[t->K] > sb->nbytes) return fail("string byte section too short");
  t->str_off = off; t->str_bytes = bytes;
  for (u32 i = 0; i < t->K; ++i) {
    if (off[i + 1] < off[i] || off[i + 1] > off[t->K]) return fail("string offsets are not monotonic");
    t->ids.insert(hash_bytes(t->at(i)), i);
  }
  u32 ns = meta[CBH_M_NSCOPES];
  if ((u64)ns * 4 > ss->nbytes) return fail("scope section too short");
  const u32* ssid = (const u32*)(base + ss->offset);
  for (u32 i = 0; i < ns; ++i) {
    if (ssid[i] >= t->K) return fail("scope string id out of range");
    t->scope_index.emplace(std::string(bytes + off[ssid[i]], off[ssid[i] + 1] - off[ssid[i]]), i);
  }
  t->scopes.resize(ns);
  for (u32 i = 0; i < ns; ++i) t->scopes[i] = std::string(t->at(ssid[i]));
  if (const CbhBlobSection* sn = find(CBH_SEC_HOST_NAMES)) {
    const u8* q = base + sn->offset; const u8* qe = q + sn->nbytes;
    for (std::vector<std::string>* dst : {&t->policy_keys, &t->dr_names}) {
      if (qe - q < 4) return fail("host name section truncated");
      u32 cnt; memcpy(&cnt, q, 4); q += 4;
      if (!names16(q, qe, cnt, *dst)) return fail("host name section truncated");
    }
  } else return fail("blob is missing the host name section");
  if (const CbhBlobSection* st = find(CBH_SEC_TRACE_HOST)) {
    const u8* q = base + st->offset; const u8* qe = q + st->nbytes;
    bool ok = true;
    auto rd32 = [&](u32& v) { if (qe - q < 4) { ok = false; v = 0; return; } memcpy(&v, q, 4); q += 4; };
    auto rdstr = [&](std::string& out) { u32 l; rd32(l); if (!ok || (u32)(qe - q) < l) { ok = false; return; } out.assign((const char*)q, l); q += l; };
    u32 ns2; rd32(ns2);
    for (u32 k = 0; ok && k < ns2; ++k) { std::string x; rdstr(x); t->trace_strings.push_back(std::move(x)); }
    std::function<void(TNode&, int)> rdnode = [&](TNode& nd, int depth) {
      if (!ok || depth > 64 || qe - q < 1) { ok = false; return; }
      nd.kind = *q++;
      if (nd.kind == 0) rd32(nd.hole);
      else if (nd.kind == 1) {
        if (qe - q < 1) { ok = false; return; }
        const u8 ct = *q++;
        if (ct == 0) nd.cst.k = TVal::Null;
        else if (ct == 1) { if (qe - q < 1) { ok = false; return; } nd.cst.k = TVal::Bool; nd.cst.b = *q++ != 0; }
        else if (ct == 2) { if (qe - q < 8) { ok = false; return; } nd.cst.k = TVal::Int; memcpy(&nd.cst.i, q, 8); q += 8; }
        else if (ct == 3) { if (qe - q < 8) { ok = false; return; } nd.cst.k = TVal::Double; memcpy(&nd.cst.d, q, 8); q += 8; }
        else if (ct == 4) { nd.cst.k = TVal::String; rdstr(nd.cst.s); }
        else ok = false;
      } else if (nd.kind == 2 || nd.kind == 3 || nd.kind == 4) {
        if (nd.kind == 4) rdstr(nd.fmt);
        u32 cnt; rd32(cnt);
        if (nd.kind == 3) cnt *= 2;
        if (!ok || cnt > (u32)(qe - q)) { ok = false; return; }
        nd.kids.resize(cnt);
        for (u32 k = 0; ok && k < cnt; ++k) rdnode(nd.kids[k], depth + 1);
      } else ok = false;
    };
    u32 nt; rd32(nt);
    for (u32 k = 0; ok && k < nt; ++k) {
      u32 word, holes; rd32(word); rd32(holes);
      TNode nd; rdnode(nd, 0);
      if (ok) t->trace_templates.emplace(word, std::make_pair(std::move(nd), holes));
    }
    if (!ok) return fail("trace host section truncated");
    const CbhBlobSection *ht = find(CBH_SEC_THEAP_TAG), *hv = find(CBH_SEC_THEAP_VAL);
    if (ht && hv && hv->nbytes / 8 >= ht->nbytes) { t->theap_tag = base + ht->offset; t->theap_val = (const u64*)(base + hv->offset); t->theap_len = (u32)ht->nbytes; }
    t->has_trace = true;
    // variables are evaluated whether a condition reads them or not, outputs on every visit of their rule: such a table's
    // inputs are all traced, any other table's only where a decision kernel marked CBH_ST_CEL_ERROR
    const CbhBlobSection* tp = find(CBH_SEC_TRACE_POOL);
    t->trace_all = (tp && tp->count > 0) || !t->trace_templates.empty();
  }
  const u8* p = base + sc->offset; const u8* e = p + sc->nbytes;
  u32 ncol = meta[CBH_M_NCOLUMNS];
  for (u32 c = 0; c < ncol; ++c) {
    if (e - p < 2) return fail("column path section truncated");
    Column col; col.root = p[0]; u32 nk = p[1]; p += 2;
    if (col.root > 4) return fail("bad column root");
    if (!names16(p, e, nk, col.keys)) return fail("column path section truncated");
    t->columns.push_back(std::move(col));
  }
  *out = t.release();
  return 0;
}
}  // extern "C"
