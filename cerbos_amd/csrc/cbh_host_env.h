// Host side of libcerbos_hip.so, part 1 of 5 (cbh_engine.hip includes them in order): how the library reads a CBH_* variable.
// A few helpers, no cache of their own: a call site that wants the value read once keeps it in a `static const`, as every site
// but CBH_CHUNK_REQUESTS and CBH_BCAST does.  The conventions differ from knob to knob and are kept as they grew (the table in
// DESIGN.md lists every variable with its own): "set at all" (env_set), "first character is c" (env_is), "is exactly this word" (env_eq), atoi / atol with a
// default (env_int / env_long), atof (env_double).
#pragma once
#include <cstdlib>
#include <cstring>

static inline bool env_set(const char* name) { return getenv(name) != nullptr; }
static inline bool env_is(const char* name, char c) { const char* e = getenv(name); return e && *e == c; }
static inline bool env_eq(const char* name, const char* value) { const char* e = getenv(name); return e && !strcmp(e, value); }
static inline int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
static inline long env_long(const char* name, long dflt) { const char* e = getenv(name); return e ? atol(e) : dflt; }
static inline double env_double(const char* name, double dflt) { const char* e = getenv(name); return e ? atof(e) : dflt; }

// CBH_WIRE_LDS (measurement aid) selects what the wire road stages in LDS: 0 nothing, 1 the assembler's outputs only, 2 the
// flattener's messages too.  Parsed once; unset, its two consumers have different defaults, and both are kept:
//   wire_lds_cap      (the output assembler's staging)  CBH_WIRE_LDS_DEFAULT, 1 unless the build says otherwise;
//   wire_fill_lds_cap (the flattener's messages)        2.
#ifndef CBH_WIRE_LDS_DEFAULT
#define CBH_WIRE_LDS_DEFAULT 1
#endif
static inline int wire_lds_mode(int dflt_when_unset) {
  static const bool set = env_set("CBH_WIRE_LDS");
  static const int m = env_int("CBH_WIRE_LDS", 0);
  return set ? m : dflt_when_unset;
}
// CBH_FLAT_ANY (measurement / test aid): every batch counts as one with int or container tags - always the flat variant with
// the evaluator call.  Read here for the three places that call a batch "plain" (host batches, cross products, wire batches).
static inline bool flat_any_forced() { static const bool on = env_set("CBH_FLAT_ANY"); return on; }
// CBH_FLAT_ACTION_GROUPS=0 (measurement aid, like CBH_NO_FLAT): a flat table's batches of requests with more than four actions keep the
// plan they had before the flat kernels' action groups (cbh_check_walk2.h cbh_plan) - the walk's kernels and the general walk.
static inline bool flat_action_groups_on() { static const bool on = env_int("CBH_FLAT_ACTION_GROUPS", 1) != 0; return on; }
