// cbh_ingest.cpp - libcerbos_ingest.so: serialized enginev1.CheckInput -> cbh_batch (include/cerbos_ingest.h).
//
// The one file handed to the compiler: a header per stage, included in dependency order (the file table and what
// has one definition each); here are the error slot and the accessors / frees of the handles.
//
// Host-only C++ (no HIP, no protobuf runtime): the wire format is walked in place, attribute columns are
// looked up directly in the serialized google.protobuf.Struct maps, and only the values a column selects
// are materialised (scalars inline, lists / maps as tapes in the batch heap).  The interning order, heap
// order and routing sort are those of cerbos_amd/flatten.py - tests/test_ingest.py compares every array.
//
// Reference behaviour restated (never copied):
//   internal/ruletable/check.go:536-554     checkInputToRequest (which fields a condition can see)
//   internal/ruletable/check.go:101-117     effective scope / policy version of principal and resource
//   internal/evaluator/evaluator.go:108-122 defaults (EvalParams.DefaultScope / DefaultPolicyVersion)
//   internal/namer/namer.go:213-218         SanitizedResource; :77-87 ScopeParents; :276-278 ScopeValue
//   api/public/cerbos/engine/v1/engine.proto:130-200 field numbers of CheckInput / Resource / Principal / AuxData
#include <algorithm>
#include <charconv>
#include <cmath>
#include <functional>
#include <cassert>
#include <map>
#include <memory>
#include <set>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <string>
#include <string_view>
#include <thread>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/cerbos_ingest.h"
#include "cbh_blob.h"

namespace {
thread_local std::string g_err;
int fail(const std::string& m) { g_err = m; return -1; }

using u8 = uint8_t; using u32 = uint32_t; using u64 = uint64_t;
}  // namespace

#include "cbi_pb.h"
#include "cbi_table.h"
#include "cbi_flatten.h"
#include "cbi_assemble.h"
#include "cbi_trace.h"

extern "C" {
const char* cbi_last_error(void) { return g_err.c_str(); }
void cbi_table_close(cbi_table* t) { delete t; }
uint32_t cbi_table_trace_scope(const cbi_table* t) { return !t || !t->has_trace ? 0u : t->trace_all ? 2u : 1u; }
void cbi_outputs_free(cbi_outputs* o) { delete o; }
const uint8_t* cbi_outputs_bytes(const cbi_outputs* o) { return o ? o->bytes.data() : nullptr; }
const uint64_t* cbi_outputs_offsets(const cbi_outputs* o) { return o ? o->offsets.data() : nullptr; }
const uint8_t* cbi_outputs_flags(const cbi_outputs* o) { return o ? o->flags.data() : nullptr; }
void cbi_batch_free(cbi_batch* b) { delete b; }
const cbh_batch* cbi_batch_view(const cbi_batch* b) { return b ? &b->view : nullptr; }
const uint64_t* cbi_batch_tuple_perm(const cbi_batch* b) { return b ? b->tuple_perm.data() : nullptr; }
const uint32_t* cbi_batch_request_input(const cbi_batch* b) { return b ? b->req_input.data() : nullptr; }
}  // extern "C"
