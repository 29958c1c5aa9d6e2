"""Every numeric comparison leaf of the device on the edge values a request can bring: signed zeros, subnormals, the neighbours of
1, 2^53, 2^63 and 2^64, the largest doubles, the infinities, NaNs of either sign and several payloads (as raw 64-bit patterns), the
same slots tagged CBH_T_INT / CBH_T_UINT, and next to them an absent attribute, a string, a bool, null and a list - against every
operator and the constants of CONSTS, and column against column.  Compared per action: the effect; per request: whether a CEL error
was recorded; nothing may be flagged CBH_ST_UNSUPPORTED.  Everything is exact.

Two references, which must agree before the device is looked at: `_leaf` below (Python's own operators: its int / float comparison
is mathematically exact) and oracle.check.RuleTableOracle.  The oracle has no door for typed request attributes (every number of a
request dict is a double there, as in structpb), so the rows whose slots are tagged int / uint are compared with the plain reference
only.  Nothing in the reference's fixtures or tests decides whether cel-go compares int64 / uint64 with double exactly or after a
conversion (DESIGN.md names the open question); this module pins the exact rule the oracle, the folder and the device implement.

Where each copy of the comparison is reached (every run asserts the kernel it meant to reach: VARIANTS):
  cbh_check_flat.h flat_leaf case 2 / 3          test_on_emulator[record_walk | staged_walk | derived_role_variant], test_resident_compact_*,
                                                 test_derived_role_variant_*, test_forced_variant_*[staged_walk]
  cbh_check_flat.h leaf_block_codes cls 2 / 3    test_on_emulator[mask_walk | typed_slots_mask_walk], test_forced_variant_*[mask_walk]
  cbh_check_wave.h leaf_fast                     test_on_emulator[walk2 | general_walk], test_forced_variant_*[walk2 | general_walk]
  cbh_vm.h num_cmp / cmp_i64_f64 / cmp_u64_f64   test_on_emulator[typed_slots | doubles_generic_leaves | ...], test_typed_slots_* (int / uint
                                                 slots and the int / uint literals beyond 2^53: the variants with the evaluator call)
  cc_fill_compact, the scan / pack kernels       test_resident_compact_*, test_resident_wide_* (CBH_COMPACT_INPUTS=0), test_narrow_planes_*,
                                                 test_narrow_without_numbers_*, test_seventeen_columns_*
The roads in: the dict road's bits are asserted where the batches are flattened (Matrix._flatten); test_wire_roads_* send the same
values as number_value in serialized CheckInputs through libcerbos_ingest.so and the device parser (tests/test_wire_device.py's
comparison of the two: bit for bit), decisions the references'; test_trace_outputs_refuse_nan_and_inf_* is the response side.
Tiers: test_on_emulator[*] runs every variant on the emulator (CPU tier); *_on_simulator is the library's host side on the simulator
(CPU tier: test_forced_variant_on_simulator runs every forced variant), *_on_gpu the library on the device.
Mutation check (on a scratch copy, tests/mutation_probe.py's way; CPU tier of this module next to the whole of test_flat_kernel.py,
test_compact_inputs.py and test_uint_and_mixed_numeric.py - those three stay green, 104 passed, under every mutant but (e)):
  (a) leaf_block_codes `a_un = false`            test_on_emulator[mask_walk | typed_slots_mask_walk], test_forced_variant_on_simulator[mask_walk]
  (b) flat_leaf `p <= q` -> `!(p > q)`           test_on_emulator[record_walk | staged_walk | typed_slots | doubles_with_the_call | doubles_generic_leaves |
                                                 derived_role_variant | walk2], the *_on_simulator runs of the same, test_wire_roads_*
  (c) cmp_i64_f64 `d >= 2^63` -> `>`             test_on_emulator[typed_slots | typed_slots_mask_walk | doubles_generic_leaves | walk2 | general_walk],
                                                 test_typed_slots_on_simulator, test_forced_variant_on_simulator[typed_slots_mask_walk | walk2 | general_walk]
  (d) case 3 / cls 3 `dbl_eq` -> `bits_eq`       every test_on_emulator variant but general_walk, the *_on_simulator runs of the same, test_wire_roads_*
  (e) the scan testing the low word              test_narrow_planes_on_simulator, test_narrow_without_numbers_on_simulator, test_seventeen_columns_on_simulator;
                                                 caught before too: test_compact_inputs.py test_workloads / test_random_flat_stores /
                                                 test_column_width_changes / test_strict_and_default_alternate _on_simulator
  (f) cc_fill_compact without the zero fill      test_narrow_planes_on_simulator, test_seventeen_columns_on_simulator
CPU tier: the kernel source on the host wave emulator (tests/hostsim_api.py) and the library's host side on the simulator
(tests/sim_engine.py).  GPU tier: libcerbos_hip.so on the device; the variants an environment variable forces run in one fresh
child process each (the library reads those once per process)."""
import operator
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from cerbos_amd.flatten import Flattener
from cerbos_amd.lower.blob import lower_rule_table
from cerbos_amd.policy.loader import policies_from_docs
from cerbos_amd.ruletable.build import rule_table_from_policies
from oracle.check import EvalParams, RuleTableOracle

API = "api.cerbos.dev/v1"
NOW = 1_700_000_000_000_000_000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_NULL, T_BOOL, T_INT, T_UINT, T_DOUBLE, T_STRING, T_LIST = 0, 1, 2, 3, 4, 5, 6   # cerbos_hip.h cbh_tag
T_ABSENT = 0xF0
COMPACT = "[compact inputs"
EFFECT_ALLOW, ST_CEL_ERROR, ST_UNSUPPORTED, F_WANT_DERIVED_ROLES = 1, 1, 2, 4   # cerbos_amd/capi.py


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def dbl(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


# ---- the values, as bit patterns
DOUBLE_BITS = [
    0x0000000000000000, 0x8000000000000000,                       # +0.0, -0.0
    0x0000000000000001, 0x8000000000000001,                       # +-5e-324
    0x000FFFFFFFFFFFFF,                                           # the largest subnormal
    0x00000000FFFFFFFF,                                           # a subnormal with a zero high word and a full low word
    bits_of(2.2250738585072014e-308), bits_of(1.0), bits_of(-1.0),
    0x3FEFFFFFFFFFFFFF, 0x3FF0000000000001,                       # 1 - 2^-53, 1 + 2^-52
    bits_of(2.0 ** 53 - 1), bits_of(2.0 ** 53), bits_of(2.0 ** 53 + 2),
    bits_of(2.0 ** 63), bits_of(-2.0 ** 63), bits_of(-2.0 ** 63) + 1,   # ... and the double just below -2^63
    bits_of(2.0 ** 64), bits_of(2.0 ** 64) - 1,                   # ... and the double just below 2^64
    bits_of(1.7976931348623157e308), bits_of(-1.7976931348623157e308),
    0x7FF0000000000000, 0xFFF0000000000000,                       # +-inf
    0x7FF8000000000000, 0xFFF8000000000000,                       # quiet NaN, negative NaN
    0x7FF4000000000000,                                           # a signalling pattern with a zero low word
    0x7FF0000000000001,                                           # ... with a zero mantissa-high part
    0x7FFABCDE12345678,                                           # a payload in both words
]
assert dbl(bits_of(-2.0 ** 63) + 1) < -2.0 ** 63 and dbl(bits_of(2.0 ** 64) - 1) < 2.0 ** 64 and dbl(0x3FEFFFFFFFFFFFFF) == 1 - 2.0 ** -53
INT_VALUES = [0, 1, -1, 2 ** 53, 2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 63 - 1, -2 ** 63]
UINT_VALUES = [0, 1, 2 ** 53 + 1, 2 ** 63, 2 ** 64 - 1]
ABSENT = ("absent",)
OTHERS = [ABSENT, ("s", "seven"), ("b", True), ("n",)]
DOUBLES = [("d", b) for b in DOUBLE_BITS]
TYPED = [("i", v) for v in INT_VALUES] + [("u", v) for v in UINT_VALUES] + [("l",)]   # (a list tag, as an int / uint tag, selects the variant with the evaluator call)


def py_value(v):
    """what the plain reference compares"""
    k = v[0]
    return dbl(v[1]) if k == "d" else v[1] if k in ("i", "u", "s", "b") else None if k == "n" else [1.0]


def json_value(v):
    """what the request dict holds (an int / uint slot: a placeholder the flattened batch overwrites)"""
    return 0.0 if v[0] in ("i", "u") else py_value(v)


# ---- the conditions.  A leaf is (lhs, op, rhs): a side is one of "x" (R.attr.x), "y" (R.attr.y), "px" (P.attr.x), "g" (R.attr.g)
# or a constant ("k", CEL text, Python value); a tree is ("all" | "any" | "none", [conditions]).
OPS = {"==": operator.eq, "!=": operator.ne, "<": operator.lt, "<=": operator.le, ">": operator.gt, ">=": operator.ge}
NAMES = {"x": "R.attr.x", "y": "R.attr.y", "px": "P.attr.x", "g": "R.attr.g"}
CONSTS = [("0.0", 0.0), ("-0.0", -0.0), ("1.0", 1.0), ("5e-324", 5e-324), ("9007199254740992.0", 2.0 ** 53), ("9223372036854775808.0", 2.0 ** 63),
          ("1.7976931348623157e308", 1.7976931348623157e308),
          ("0", 0), ("100", 100), ("9007199254740993", 2 ** 53 + 1), ("9223372036854775807", 2 ** 63 - 1), ("-9223372036854775808", -2 ** 63),
          ("0u", 0), ("18446744073709551615u", 2 ** 64 - 1)]
CONST_CONDS = [("x", op, ("k", text, val)) for text, val in CONSTS for op in OPS]
PAIR_CONDS = [("x", "==", "y"), ("x", "!=", "y"), ("x", "<", "y"), ("x", "==", "px")]
# The classified leaves (celc.py _leaf_class 2 and 3: a column against a double constant - an int / uint literal a double holds exactly is
# lowered as one -, a column ==/!= a column): a table of these alone is closed over the inline leaves, the flat kernels without the
# evaluator call decide it.  An int / uint literal beyond 2^53 must NOT become a double constant (it would be rounded): those and
# the ordering of two columns are generic leaves, which the variants with the call hand to the evaluator.
CLOSED_CONDS = [c for c in CONST_CONDS if isinstance(c[2][2], float) or abs(c[2][2]) <= 2 ** 53]
CLOSED_PAIRS = [c for c in PAIR_CONDS if c[1] in ("==", "!=")]
assert len(CONST_CONDS) - len(CLOSED_CONDS) == 4 * 6
TRUE, K1, K0, K63 = ("k", "true", True), ("k", "1.0", 1.0), ("k", "0.0", 0.0), ("k", "9223372036854775808.0", 2.0 ** 63)
# leaves behind a deciding one (g is true in every other request): their error must not be reported
TREE_CONDS = [("any", [("g", "==", TRUE), ("x", "<", K1)]),
              ("all", [("g", "==", TRUE), ("x", ">=", K0)]),
              ("none", [("g", "==", TRUE), ("x", "==", "y")]),
              ("any", [("x", "!=", K0), ("all", [("g", "==", TRUE), ("x", "<=", K63)])])]


def _is_num(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _leaf(op, a, b):
    """THE PLAIN REFERENCE -> (satisfied, evaluation error).  Numbers compare mathematically, whatever their types (Python's int /
    float comparison is exact); a NaN is unequal to everything and unordered; a non-number is plainly unequal to a number, and
    ordering the two (or two values of different, or of unordered, types) is "no such overload"; an absent attribute is an error."""
    if a is ABSENT or b is ABSENT:
        return False, True
    if _is_num(a) and _is_num(b):
        if a != a or b != b:
            return op == "!=", False
        return OPS[op](a, b), False
    if op in ("==", "!="):
        return ((type(a) is type(b) and a == b) == (op == "=="), False)
    if type(a) is type(b) and isinstance(a, (str, bool)):
        return OPS[op](a, b), False
    return False, True


def reference(cond, env):
    """-> (satisfied, evaluation error).  A level ends at its first deciding operand (what lies behind it is not evaluated: no
    error of its is recorded); a leaf that errs counts as not satisfied, its error is recorded, and the level goes on."""
    if cond[0] in ("all", "any", "none"):
        err = False
        for c in cond[1]:
            sat, e = reference(c, env)
            err = err or e
            if sat != (cond[0] == "all"):
                return cond[0] == "any", err
        return cond[0] != "any", err
    lhs, op, rhs = cond
    side = lambda s: s[2] if isinstance(s, tuple) else env[s]   # noqa: E731
    return _leaf(op, side(lhs), side(rhs))


def match_of(cond):
    if cond[0] in ("all", "any", "none"):
        return {cond[0]: {"of": [match_of(c) for c in cond[1]]}}
    lhs, op, rhs = cond
    side = lambda s: s[1] if isinstance(s, tuple) else NAMES[s]   # noqa: E731
    return {"expr": "%s %s %s" % (side(lhs), op, side(rhs))}


class Matrix:
    """Policies: one resource kind per four conditions, each condition its own ALLOW rule on its own action (requests of four
    actions: the flat kernels' shape).  Requests: for a kind of constant conditions every value of `values` in x; for the kind of
    the column-against-column conditions every pair; filler up to a size that is no multiple of 64, with a NaN at lane 0, -0.0 at
    lane 63, the smallest subnormal in the last lane of the partial last wave."""

    def __init__(self, conds, values, pair_conds=(), derived=False):
        self.kinds = [conds[i:i + 4] for i in range(0, len(conds), 4)]
        self.pair_kind = len(self.kinds) if pair_conds else None
        if pair_conds:
            self.kinds.append(list(pair_conds))
        docs, n = [], 0
        for k, cs in enumerate(self.kinds):
            rules, defs = [], []
            for j, c in enumerate(cs):
                cond = {"match": match_of(c)}
                if derived:
                    defs.append({"name": "dr%d" % n, "parentRoles": ["*"], "condition": cond})
                    rules.append({"actions": ["a%d" % j], "derivedRoles": ["dr%d" % n], "effect": "EFFECT_ALLOW"})
                else:
                    rules.append({"actions": ["a%d" % j], "roles": ["*"], "effect": "EFFECT_ALLOW", "condition": cond})
                n += 1
            pol = {"resource": "k%d" % k, "version": "default", "rules": rules}
            if derived:
                docs.append({"apiVersion": API, "derivedRoles": {"name": "defs%d" % k, "definitions": defs}})
                pol["importDerivedRoles"] = ["defs%d" % k]
            docs.append({"apiVersion": API, "resourcePolicy": pol})
        self.rt = rule_table_from_policies(policies_from_docs(docs))
        self.lt = lower_rule_table(self.rt)
        one = ("d", bits_of(1.0))
        rows = []
        for k in range(len(self.kinds)):
            if k == self.pair_kind:
                rows += [(k, x, y) for x in values for y in values]
            else:
                rows += [(k, x, values[(i + k) % len(values)]) for i, x in enumerate(values)]
        while len(rows) < 300 or len(rows) % 64 != 37:
            rows.append((len(rows) % len(self.kinds), ("d", bits_of(float(len(rows) % 200))), one))
        # by index: the edge values at the ends of the first wave and in the last lane of the partial last one
        for at, want in ((0, 0x7FF8000000000000), (63, 0x8000000000000000), (len(rows) - 1, 0x0000000000000001)):
            src = next(i for i, r in enumerate(rows) if r[1] == ("d", want) and i not in (0, 63))
            rows[at], rows[src] = rows[src], rows[at]
        self.rows = rows
        self.inputs = []
        for i, (k, x, y) in enumerate(rows):
            rattr = {"g": i % 2 == 0}
            pattr = {}
            if x is not ABSENT:
                rattr["x"] = json_value(x)
            if y is not ABSENT:
                rattr["y"] = json_value(y)
                pattr["x"] = json_value(y)
            self.inputs.append({"requestId": "q%d" % i, "actions": ["a%d" % j for j in range(len(self.kinds[k]))],
                                "principal": {"id": "p", "roles": ["user"], "attr": pattr},
                                "resource": {"kind": "k%d" % k, "id": "r", "attr": rattr}})
        self.typed = any(v[0] in ("i", "u") for r in rows for v in r[1:])
        self.batch = self._flatten()
        self.want = self._expected()

    def column(self, root, name):
        return next(i for i, (r, keys) in enumerate(self.lt.columns) if r == root and tuple(keys) == (name,))

    def _flatten(self):
        """The dict road: the bits of a double are the IEEE bits of the input, NaN payloads and signs included (the requests keep
        their order: lane = index).  Then the int / uint slots, written into the flattened batch."""
        b = Flattener(self.lt).flatten(self.inputs, sort=False)
        assert b.n_requests == len(self.rows) and b.n_requests % 64 and b.n_requests > 256
        assert int(b.req_u32[9].max()) <= 4 and int(b.req_u32[7].max()) <= 4   # the flat kernels' batch shape
        cols = {"x": [self.column("R", "x")], "y": [c for c in (self._col("R", "y"), self._col("P", "x")) if c is not None]}
        for i, (_, x, y) in enumerate(self.rows):
            for v, cs in ((x, cols["x"]), (y, cols["y"])):
                for c in cs:
                    if v[0] == "d":
                        assert b.col_tag[c, i] == T_DOUBLE and int(b.col_val[c, i]) == v[1], (i, v)
                    elif v[0] in ("i", "u"):
                        b.col_tag[c, i] = T_INT if v[0] == "i" else T_UINT
                        b.col_val[c, i] = np.uint64(v[1] & 0xFFFFFFFFFFFFFFFF)
                    elif v is ABSENT:
                        assert b.col_tag[c, i] == T_ABSENT
        return b

    def _col(self, root, name):
        try:
            return self.column(root, name)
        except StopIteration:
            return None

    def _expected(self):
        """[(allow per action, evaluation error)] by the plain reference - and by the oracle, wherever it can be asked"""
        orc = RuleTableOracle(self.rt)
        out = []
        for inp, (k, x, y) in zip(self.inputs, self.rows):
            env = {"x": ABSENT if x is ABSENT else py_value(x), "y": ABSENT if y is ABSENT else py_value(y), "g": inp["resource"]["attr"]["g"]}
            env["px"] = env["y"]
            got = [reference(c, env) for c in self.kinds[k]]
            allow, err = [s for s, _ in got], any(e for _, e in got)
            if x[0] not in ("i", "u") and y[0] not in ("i", "u"):
                o = orc.check(inp, EvalParams(now_ns=NOW))
                assert [o["actions"][a]["effect"] == "EFFECT_ALLOW" for a in inp["actions"]] == allow, ("the references disagree", self.kinds[k], x, y)
                assert bool(o.get("evaluationErrors")) == err, ("the references disagree on the error", self.kinds[k], x, y)
            out.append((allow, err))
        return out

    def compare(self, res, what):
        """`res` in input order"""
        assert not (res.status == ST_UNSUPPORTED).any(), (what, "flagged for the CPU path", int((res.status == ST_UNSUPPORTED).sum()))
        t = 0
        for i, ((k, x, y), (allow, err)) in enumerate(zip(self.rows, self.want)):
            na = len(allow)
            have = [int(e) == EFFECT_ALLOW for e in res.effect[t:t + na]]
            assert have == allow, (what, "lane %d" % (i % 64), [match_of(c) for c in self.kinds[k]], x, y, have, allow)
            assert bool((res.status[t:t + na] == ST_CEL_ERROR).any()) == err, (what, "error", i, [match_of(c) for c in self.kinds[k]], x, y)
            t += na
        assert t == res.effect.size


_MATRICES = {}


def matrix(which):
    """doubles: the classified leaves, no int / uint / list tag in the batch; doubles_all: every condition; typed: every condition,
    those tags too; derived: the doubles' conditions as derived-role conditions (a table names at most 64 derived roles: two tables)"""
    if which not in _MATRICES:
        if which == "doubles":
            m = [Matrix(CLOSED_CONDS + TREE_CONDS, DOUBLES + OTHERS, CLOSED_PAIRS)]
        elif which == "doubles_all":
            m = [Matrix(CONST_CONDS + TREE_CONDS, DOUBLES + OTHERS, PAIR_CONDS)]
        elif which == "typed":
            m = [Matrix(CONST_CONDS + TREE_CONDS, DOUBLES + OTHERS + TYPED, PAIR_CONDS)]
        else:
            half = len(CLOSED_CONDS) // 2
            m = [Matrix(CLOSED_CONDS[:half], DOUBLES + OTHERS, CLOSED_PAIRS, derived=True), Matrix(CLOSED_CONDS[half:] + TREE_CONDS, DOUBLES + OTHERS, derived=True)]
        for x in m:
            assert x.lt.stats["flat"] and x.lt.stats["flat_closed"] == (which in ("doubles", "derived")), (which, x.lt.stats)
        _MATRICES[which] = m
    return _MATRICES[which]


# ---- the runs.  VARIANTS: name -> (matrix, environment, what the plan must say, the emulator's last_kind / last_masks)
def _flat(plan, *suffixes, no=()):
    name = plan.split("[")[0]
    return name.startswith("cbh_check_flat_kernel") and all(s in name for s in suffixes) and not any(s in name for s in no)


VARIANTS = {
    "record_walk": ("doubles", {}, lambda p: _flat(p, no=("_any", "_staged", "_masks", "_dr")), (1, 0)),
    "staged_walk": ("doubles", {"CBH_FORCE_STAGED": "1"}, lambda p: _flat(p, "_staged", no=("_any",)), (1, 0)),
    "mask_walk": ("doubles", {"CBH_FLAT_MASKS": "1"}, lambda p: _flat(p, "_masks", no=("_any",)), (1, 1)),
    "typed_slots": ("typed", {}, lambda p: _flat(p, "_any"), (1, 0)),
    "typed_slots_mask_walk": ("typed", {"CBH_FLAT_MASKS": "1"}, lambda p: _flat(p, "_any_masks"), (1, 1)),
    "doubles_with_the_call": ("doubles", {"CBH_FLAT_ANY": "1"}, lambda p: _flat(p, "_any"), (1, 0)),
    "doubles_generic_leaves": ("doubles_all", {}, lambda p: _flat(p, "_any"), (1, 0)),
    "derived_role_variant": ("derived", {}, lambda p: _flat(p, "_dr"), (1, 0)),
    "walk2": ("typed", {"CBH_NO_FLAT": "1"}, lambda p: p.endswith("cbh_walk2_kernel"), (2, None)),
    "general_walk": ("typed", {"CBH_NO_FLAT": "1", "CBH_NO_WALK2": "1"}, lambda p: p.startswith("cbh_check_kernel*"), (0, None)),
}


def check_on_emulator(variant, monkeypatch):
    import hostsim_api
    which, env, _, (kind, masks) = VARIANTS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for m in matrix(which):
        res = hostsim_api.check(m.lt, m.batch, NOW, F_WANT_DERIVED_ROLES)
        assert hostsim_api.last_kind() == kind, (variant, hostsim_api.last_kind())
        if masks is not None:
            assert hostsim_api.lib().hostsim_last_masks() == masks, variant
        m.compare(res, variant)


def check_on_library(capi, variant, compact=None):
    """cbh_check_batch and the resident path (upload / launch / download: packed results, and the compact inputs where the kernel
    has a compact instantiation), each against the references; the plan names the kernel"""
    which, _, plan_ok, _ = VARIANTS[variant]
    for m in matrix(which):
        table = capi.Table(m.lt.blob)
        m.compare(table.check(m.batch, now_ns=NOW, flags=F_WANT_DERIVED_ROLES), variant + ", cbh_check_batch")
        db = table.upload(m.batch)
        try:
            for flags in (F_WANT_DERIVED_ROLES, 0):
                table.launch(db, now_ns=NOW, flags=flags)
                m.compare(table.download(db), variant + ", resident")
            plan = table.plan(db, flags=F_WANT_DERIVED_ROLES)
            assert plan_ok(plan), (variant, plan)   # a test that passes because everything fell back proves nothing
            if compact is not None:
                assert (COMPACT in plan) == compact, (variant, plan)
        finally:
            db.close()
        table.close()


CHILD = """
import sys
sys.path.insert(0, %(tests)r)
import test_numeric_edges as tn
if %(sim)r:
    from sim_engine import sim_engine
    with sim_engine() as capi:
        tn.check_on_library(capi, %(variant)r, %(compact)r)
else:
    from cerbos_amd import capi
    tn.check_on_library(capi, %(variant)r, %(compact)r)
print("numeric edges: ok")
"""


def check_in_child(sim, variant, compact=None, extra_env=None):
    """One fresh process per forced variant (the library reads its switches once).  A child that a signal ended fails the test."""
    env = dict(os.environ, **VARIANTS[variant][1], **(extra_env or {}))
    r = subprocess.run([sys.executable, "-c", CHILD % {"tests": os.path.join(ROOT, "tests"), "sim": sim, "variant": variant, "compact": compact}],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode >= 0, "the child was ended by signal %d\n%s" % (-r.returncode, r.stderr[-4000:])
    assert r.returncode == 0 and "numeric edges: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]


# ---- the compact planes by bit pattern
def _narrow(plan):
    return int(plan.split("narrow columns 0x")[1].split("]")[0], 16)


def _small_table(conds_by_column):
    """{column name: [(op, CEL constant, Python value)]} -> one kind, four actions at most per kind ... one policy per column"""
    docs = []
    for name, conds in conds_by_column.items():
        assert len(conds) <= 4
        docs.append({"apiVersion": API, "resourcePolicy": {"resource": "k_" + name, "version": "default", "rules": [
            {"actions": ["a%d" % j], "roles": ["*"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": "R.attr.%s %s %s" % (name, op, text)}}}
            for j, (op, text, _) in enumerate(conds)]}})
    rt = rule_table_from_policies(policies_from_docs(docs))
    return rt, lower_rule_table(rt)


def _decide(capi, lt, conds_by_column, rows, expect_narrow, compact=True):
    """rows: [(column name, {column: value spec})] - a request of kind k_<column> carrying those attributes.  Both paths of the
    library against the plain reference; -> ({column: its bit of the resident plan's narrow mask}, {column: index}, the plan)."""
    inputs = [{"requestId": "q%d" % i, "actions": ["a%d" % j for j in range(len(conds_by_column[name]))], "principal": {"id": "p", "roles": ["user"], "attr": {}},
               "resource": {"kind": "k_" + name, "id": "r", "attr": {k: json_value(v) for k, v in attrs.items() if v is not ABSENT}}}
              for i, (name, attrs) in enumerate(rows)]
    batch = Flattener(lt).flatten(inputs, sort=False)
    col = {name: next(i for i, (r, keys) in enumerate(lt.columns) if r == "R" and tuple(keys) == (name,)) for name in conds_by_column}
    for i, (_, attrs) in enumerate(rows):
        for k, v in attrs.items():
            if v[0] == "d":
                assert int(batch.col_val[col[k], i]) == v[1] and batch.col_tag[col[k], i] == T_DOUBLE
    want_allow, want_err = [], []
    for name, attrs in rows:
        x = attrs.get(name, ABSENT)
        got = [_leaf(op, ABSENT if x is ABSENT else py_value(x), val) for op, _, val in conds_by_column[name]]
        want_allow += [s for s, _ in got]
        want_err.append(any(e for _, e in got))
    table = capi.Table(lt.blob)
    db = table.upload(batch)
    try:
        table.launch(db, now_ns=NOW, flags=0)
        plan = table.plan(db, flags=0)
        for res, what in ((table.download(db), "resident"), (table.check(batch, now_ns=NOW, flags=0), "cbh_check_batch")):
            assert not (res.status == ST_UNSUPPORTED).any(), what
            assert [int(e) == EFFECT_ALLOW for e in res.effect] == want_allow, (what, plan)
            t = 0
            for (name, _), err in zip(rows, want_err):
                na = len(conds_by_column[name])
                assert bool((res.status[t:t + na] == ST_CEL_ERROR).any()) == err, (what, name)
                t += na
    finally:
        db.close()
        table.close()
    assert plan.startswith("cbh_check_flat_kernel") and (COMPACT in plan) == compact, plan
    mask = _narrow(plan) if compact else 0
    return {name: (mask >> col[name]) & 1 for name in expect_narrow}, col, plan


TINY = [("d", b) for b in (0x1, 0x2, 0x7E7, 0xFFFFFFFF, 0x0, 0x80000000, 0x12345678)]   # below 2^-1042: a zero high word, low words that are not
TINY_CONDS = {"x": [(">", "0.0", 0.0), ("==", "5e-324", 5e-324), ("<", "1e-320", 1e-320), ("!=", "0.0", 0.0)]}


def check_narrow_planes(capi):
    """a double column of subnormals below 2^-1042 and +0.0 has a 32-bit plane (on the GPU: and is not flushed to zero); one -0.0 in
    the last lane of the partial last wave takes the plane away and changes no answer"""
    _, lt = _small_table(TINY_CONDS)
    rows = [("x", {"x": TINY[i % len(TINY)]}) for i in range(300 + 37)]
    bit, _, _ = _decide(capi, lt, TINY_CONDS, rows, ["x"])
    assert bit["x"] == 1
    rows[-1] = ("x", {"x": ("d", 0x8000000000000000)})
    bit, _, _ = _decide(capi, lt, TINY_CONDS, rows, ["x"])
    assert bit["x"] == 0
    zero = {"x": [("==", "0.0", 0.0), ("<", "0.0", 0.0), (">=", "-0.0", -0.0), ("!=", "5e-324", 5e-324)]}
    _, lt0 = _small_table(zero)
    bit, _, _ = _decide(capi, lt0, zero, rows, ["x"])   # -0.0 == 0.0, not -0.0 < 0.0
    assert bit["x"] == 0 and _leaf("==", -0.0, 0.0) == (True, False) and _leaf("<", -0.0, 0.0) == (False, False)


def check_narrow_without_numbers(capi):
    """a column that is narrow only because no request brings a number: absent, a bool, a string id - against double constants"""
    conds = {"x": [("==", "1.0", 1.0), ("!=", "1.0", 1.0), ("<", "1.0", 1.0), (">=", "0.0", 0.0)]}
    _, lt = _small_table(conds)
    vals = [ABSENT, ("b", True), ("s", "seven"), ("b", False), ("s", "")]
    bit, _, _ = _decide(capi, lt, conds, [("x", {"x": vals[i % len(vals)]}) for i in range(300 + 21)], ["x"])
    assert bit["x"] == 1


def check_seventeen_columns(capi):
    """as many attribute columns as the cache holds (CBH_CACHE_COLS = 16 = the bits of CBH_CI_NARROW_MASK): all sixteen narrow at once
    (mask 0xFFFF, right below CBH_CI_ACT4), then edge values in column 15.  One column more: column 16 is read the other way (no
    cached column: its leaves are generic ones, the variant with the evaluator call decides the table from the wide form), edge
    values in columns 15 and 16."""
    edge = [("d", b) for b in (0x7FF8000000000000, 0x8000000000000000, 0x1, 0xFFF0000000000000, 0x7FF0000000000001, bits_of(2.0 ** 53))]
    for ncol in (16, 17):
        names = ["c%02d" % i for i in range(ncol)]
        conds = {n: [(">", "0.0", 0.0), ("==", "5e-324", 5e-324), ("!=", "0.0", 0.0), ("<=", "-0.0", -0.0)] for n in names}
        _, lt = _small_table(conds)
        assert len(lt.columns) == ncol, lt.columns
        rows = [(names[i % ncol], {m: TINY[(i + j) % len(TINY)] for j, m in enumerate(names)}) for i in range(ncol * 19 + 5)]
        if ncol == 16:
            bit, col, _ = _decide(capi, lt, conds, rows, names)
            assert all(bit[n] for n in names), bit          # 0xFFFF
        else:
            col = {n: next(i for i, (r, keys) in enumerate(lt.columns) if tuple(keys) == (n,)) for n in names}
        for i, (_, attrs) in enumerate(rows):   # wide values in the last cached column (and in the first beyond the cache)
            for n in names:
                if col[n] >= 15:
                    attrs[n] = edge[(i + col[n]) % len(edge)]
        got, _, plan = _decide(capi, lt, conds, rows, names, compact=ncol == 16)
        if ncol == 16:
            assert [got[n] for n in names if col[n] < 15] == [1] * 15 and not any(got[n] for n in names if col[n] == 15), got
        else:
            assert plan == "cbh_check_flat_kernel_any", plan


# ---- the roads in: the same values as number_value in serialized CheckInputs
def _number_bits_arrived(m, b, what):
    """every number of the flattened batch `b` (input order) has the bits the dict road gave it"""
    assert np.array_equal(b.col_tag, m.batch.col_tag), what
    num = m.batch.col_tag == T_DOUBLE
    assert num.sum() > 1000 and np.array_equal(np.asarray(b.col_val)[num], m.batch.col_val[num]), what


def check_wire_roads_on_emulator():
    """C++ ingest (cbi_flatten_pb) and the device parser's kernels on the emulator: tests/test_wire_device.py's comparison of the two,
    value by value; every NaN payload and sign, -0.0 and the subnormals arrive bit for bit (= the dict road's bits); the decisions
    from either batch are the references'"""
    import hostsim_api
    import wire_device_util as wu
    from test_wire_device import _compare
    m = matrix("doubles")[0]
    hb, wb = _compare(m.lt, m.inputs)
    _number_bits_arrived(m, hb, "libcerbos_ingest.so")
    _number_bits_arrived(m, wb, "the device parser")
    m.compare(hostsim_api.check(m.lt, hb, NOW, F_WANT_DERIVED_ROLES), "wire road, host flattener")
    m.compare(hostsim_api.check(m.lt, wu.to_batch(m.lt, wb), NOW, F_WANT_DERIVED_ROLES), "wire road, device flattener")
    assert hostsim_api.last_kind() == 1


def check_wire_roads_on_library(capi):
    """through the library: cbi_flatten_pb -> cbh_check_batch, cbh_wire_flatten -> cbh_check_resident, and cbh_wire_check_pb (the
    device road in one call: the answers as serialized CheckOutputs) - every decision the references'"""
    from cerbos_amd import wire
    from cerbos_amd.ingest import IngestTable
    m = matrix("doubles")[0]
    data, off = wire.pack_messages([wire.encode_check_input(i) for i in m.inputs])
    table, it = capi.Table(m.lt.blob), IngestTable(m.lt.blob)
    try:
        hb = it.flatten_pb(data, off, sort=False)
        _number_bits_arrived(m, hb, "libcerbos_ingest.so")
        m.compare(table.check(hb, now_ns=NOW, flags=F_WANT_DERIVED_ROLES), "wire road, host flattener")
        db = table.wire_flatten(data, off)
        try:
            assert db.wire_info["n_host"] == 0, db.wire_info
            table.launch(db, now_ns=NOW, flags=F_WANT_DERIVED_ROLES)
            m.compare(table.download(db), "wire road, cbh_wire_flatten")
            assert table.plan(db, flags=F_WANT_DERIVED_ROLES).startswith("cbh_check_flat_kernel")
        finally:
            db.close()
        raw, flags = table.wire_check_pb(data, off, now_ns=NOW, flags=F_WANT_DERIVED_ROLES)
        for i, (r, inp, (allow, err)) in enumerate(zip(raw, m.inputs, m.want)):
            out = wire.decode_check_output(r)
            assert [out["actions"][a]["effect"] == "EFFECT_ALLOW" for a in inp["actions"]] == allow, ("cbh_wire_check_pb", i, m.rows[i])
            assert int(flags[i]) == (2 if err else 0), ("cbh_wire_check_pb", i, m.rows[i], int(flags[i]))   # cerbos_ingest.h CBI_OUT_CEL_ERROR, nothing else
    finally:
        table.close()
        it.close()


def check_trace_outputs_refuse_nan_and_inf(make_evaluator, close):
    """The response side: an output expression that formats a request's NaN / infinity is not assembled (cel-go's text for those is
    not reproduced) - the Python assembler (cerbos_amd/trace.py) names the input in `incomplete`, the C++ one (cbh_ingest.cpp
    format_value: TraceIncomplete) sets the outputs-incomplete flag; the decision stands, and an ordinary number is formatted."""
    from cerbos_amd import wire
    docs = [{"apiVersion": API, "resourcePolicy": {"resource": "k", "version": "default", "rules": [
        {"actions": ["a"], "roles": ["*"], "effect": "EFFECT_ALLOW", "name": "r", "condition": {"match": {"expr": "R.attr.x != 0.0"}},
         "output": {"when": {"ruleActivated": '"x=%s".format([R.attr.x])'}}}]}}]
    lt = lower_rule_table(rule_table_from_policies(policies_from_docs(docs)))
    bits = [bits_of(1.5), 0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000000, 0xFFF0000000000000, bits_of(-0.0)]
    inputs = [{"requestId": "q%d" % i, "actions": ["a"], "principal": {"id": "p", "roles": ["user"], "attr": {}},
               "resource": {"kind": "k", "id": "r", "attr": {"x": dbl(b)}}} for i, b in enumerate(bits)]
    refused = {1, 2, 3, 4}
    ev = make_evaluator(lt)
    try:
        outs, bad, incomplete = ev.check(inputs, now_ns=NOW, allow_unsupported=True, trace=True)
        assert not bad and {i for i, what in incomplete.items() if "outputs" in what} == refused, incomplete
        data, off = wire.pack_messages([wire.encode_check_input(i) for i in inputs])
        raw, flags = ev.check_pb(data, off, now_ns=NOW, trace=True)
        assert {i for i in range(len(inputs)) if flags[i] & 8} == refused and not (np.asarray(flags) & 1).any(), flags
        for have in (outs, [wire.decode_check_output(r) for r in raw]):
            assert [o["actions"]["a"]["effect"] == "EFFECT_ALLOW" for o in have] == [True] * 5 + [False]   # (-0.0 != 0.0 is false)
            assert [x["val"] for x in have[0].get("outputs") or []] == ["x=1.5"], have[0]
            assert not have[5].get("outputs")
    finally:
        if close:
            ev.close()


# ---- CPU tier: the wave emulator (the kernels' source) ...


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_on_emulator(variant, monkeypatch):
    check_on_emulator(variant, monkeypatch)


# ---- ... and the simulator build of the library


@pytest.fixture()
def engine():
    from sim_engine import sim_engine
    with sim_engine() as capi:
        yield capi


def test_resident_compact_on_simulator(engine):
    check_on_library(engine, "record_walk", compact=True)


def test_typed_slots_on_simulator(engine):
    check_on_library(engine, "typed_slots", compact=False)


def test_derived_role_variant_on_simulator(engine):
    check_on_library(engine, "derived_role_variant", compact=False)


@pytest.mark.parametrize("variant", ["staged_walk", "mask_walk", "typed_slots_mask_walk", "doubles_with_the_call", "walk2", "general_walk"])
def test_forced_variant_on_simulator(variant):
    check_in_child(True, variant)


def test_resident_wide_on_simulator():
    check_in_child(True, "record_walk", compact=False, extra_env={"CBH_COMPACT_INPUTS": "0"})


def test_narrow_planes_on_simulator(engine):
    check_narrow_planes(engine)


def test_narrow_without_numbers_on_simulator(engine):
    check_narrow_without_numbers(engine)


def test_seventeen_columns_on_simulator(engine):
    check_seventeen_columns(engine)


def test_wire_roads_on_emulator():
    check_wire_roads_on_emulator()


def test_wire_roads_on_simulator(engine):
    check_wire_roads_on_library(engine)


def test_trace_outputs_refuse_nan_and_inf_on_emulator():
    from cerbos_amd.engine import Conf
    from test_trace_pass import _HostSimBytes
    check_trace_outputs_refuse_nan_and_inf(lambda lt: _HostSimBytes(lt, Conf()), False)


def test_folder_and_oracle_follow_the_exact_rule():
    """int64 / uint64 against double, exactly - oracle.celeval and the lowering's constant folder (cerbos_amd/cel/fold.py), on the
    rows where a conversion to double first would answer differently"""
    from cerbos_amd.cel import fold
    from oracle import celeval
    for a, b in ((2 ** 53 + 1, 2.0 ** 53), (2 ** 63 - 1, 2.0 ** 63), (-(2 ** 53 + 1), -2.0 ** 53), (celeval.UInt(2 ** 64 - 1), 2.0 ** 64), (celeval.UInt(2 ** 53 + 1), 2.0 ** 53)):
        want = (int(a) > b) - (int(a) < b)
        assert want != 0 and float(a) == b
        assert celeval._num_cmp(a, b) == want and celeval._num_cmp(b, a) == -want
        assert fold._num_cmp(a, b) == want and fold._num_cmp(b, a) == -want


# ---- GPU tier


@pytest.mark.gpu
def test_resident_compact_on_gpu():
    from cerbos_amd import capi
    check_on_library(capi, "record_walk", compact=True)


@pytest.mark.gpu
def test_typed_slots_on_gpu():
    from cerbos_amd import capi
    check_on_library(capi, "typed_slots", compact=False)


@pytest.mark.gpu
def test_derived_role_variant_on_gpu():
    from cerbos_amd import capi
    check_on_library(capi, "derived_role_variant", compact=False)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["staged_walk", "mask_walk", "typed_slots_mask_walk", "doubles_with_the_call", "walk2", "general_walk"])
def test_forced_variant_on_gpu(variant):
    check_in_child(False, variant)


@pytest.mark.gpu
def test_resident_wide_on_gpu():
    check_in_child(False, "record_walk", compact=False, extra_env={"CBH_COMPACT_INPUTS": "0"})


@pytest.mark.gpu
def test_narrow_planes_on_gpu():
    from cerbos_amd import capi
    check_narrow_planes(capi)


@pytest.mark.gpu
def test_narrow_without_numbers_on_gpu():
    from cerbos_amd import capi
    check_narrow_without_numbers(capi)


@pytest.mark.gpu
def test_seventeen_columns_on_gpu():
    from cerbos_amd import capi
    check_seventeen_columns(capi)


@pytest.mark.gpu
def test_wire_roads_on_gpu():
    from cerbos_amd import capi
    check_wire_roads_on_library(capi)


@pytest.mark.gpu
def test_trace_outputs_refuse_nan_and_inf_on_gpu():
    from cerbos_amd.engine import Conf, HipEvaluator
    check_trace_outputs_refuse_nan_and_inf(lambda lt: HipEvaluator(lt, Conf()), True)
