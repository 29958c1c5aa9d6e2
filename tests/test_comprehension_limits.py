"""Comprehensions and the lists a program builds, at the sizes the interpreter has built in.

all / exists / exists_one / filter / map / transformList run as ONE wave-uniform loop of the operand-stack interpreter
(cbh_interp.h OP_ITER_BEGIN / _NEXT / _ACC / _END) in which every lane makes its own progress, and the lists a program builds
(filter, map, `+`, intersect, except, reverse, lists.range) live in a per-lane arena (cbh_vm.h).  The sizes, restated here from
the headers and used to BUILD the inputs - the set of flagged (request, action) pairs follows from these numbers and the rules
below alone, never from what the code answers:
  ITERS = 2             cbh_vm.h CBH_MAX_ITERS, lower/celc.py MAX_ITERS: loops nested in one another
  LOCALS = 4            CBH_MAX_LOCALS / MAX_LOCALS: loop variables and cel.bind variables alive at once (they share the slots)
  ARENA = 48            cbh_blob.h CBH_ARENA_ENTRIES: values per lane
  COUNT_BITS = 14       it_state (per lane and loop): [7:0] the macro, [11:8] ITS_ERRSEEN / _DECIDED / _ENTRY_LIVE / _RUNNING,
                        [29:16] a count, [30] ITS_MAP (the range is a map), [31] ITS_FAIL.  it_idx: [31:26] where the result begins
                        in the arena, [25:20] the arena's fill when the loop began, [19:0] the index
  STEPS = 1 000 000     operations of one call of the interpreter; a wave that spends them is flagged as a whole
A comprehension nested deeper than ITERS, or one that would need a fifth local, is refused at lowering (lt.unsupported): the macro
becomes OP_UNSUPPORTED, and every lane that REACHES it live is flagged (a request whose enclosing range is empty never does, and
is decided).

The arena's rules (cbh_interp.h), `ap` = the lane's fill:
  filter / map / transformList   reserve the RANGE's length at OP_ITER_BEGIN (n > ARENA - ap: flagged), whatever they keep
  all / exists / exists_one / filter   what a turn of the body built is released at the next OP_ITER_NEXT (ap = the fill at the begin)
  map / transformList            what the body built stays (the body's value may be what it built): turn k of a body that
                                 builds b entries needs range + k * b <= ARENA
  a + b                          len(a) + len(b), and each operand at most ARENA
  intersect(a, b)                the length of the SHORTER operand (the operands are swapped so that it is iterated; equal lengths:
                                 a); except(a, b): len(a); for both, each operand at most ARENA
  reverse(l), lists.range(n)     len(l), n
  slice                          nothing (a view)
  hasIntersection / isSubset / in   nothing: operands of any length are answered
  a result is never given back before the program ends: two filters in one expression need the sum of their ranges
Concatenation: `+` becomes a list concatenation (OP_LISTOP) only where one operand is VISIBLY a list - a literal, filter / map /
transformList, intersect / except / slice, reverse of such, split, lists.range, or a `+` of such (lower/celc.py _builds_list).
`R.attr.xs + R.attr.xs` shows neither, stays the arithmetic OP_ADD, and OP_ADD flags a lane that brings it a list:
CBH_ST_UNSUPPORTED for every length, the empty list included.  `R.attr.xs + ["zz"]` and `[] + R.attr.xs + R.attr.xs` run.

What was found.  exists_one counted its hits in the 14 bits without a bound: the 16 384th hit carried into ITS_MAP, after which
the count read 0 and the lane took its list for a map (OP_ITER_NEXT then read heap entry 2 * i, beyond the list's end).  16 385
hits read as one: `[1] * 16385` with `exists_one(x, x > 0)` was ALLOWED, status OK.  The count now stops at 2.  On the parent
test_*[counter_*] fail with exactly that difference (h16385_* and h32769_*: ALLOW where DENY is wanted), nothing else does.

The reference is oracle/check.py per (request, action): effect, policy key and status - CBH_ST_CEL_ERROR exactly where the oracle
reports an evaluation error for that action's expression.  Every layer exists twice, the same requests against two stores: `w`,
which plans to cbh_walk2_kernel with cbh_walk2_interp_kernel as its pre-pass, and `g`, the same store with a resource kind of 17
action globs beside it, which the walk refuses (16 patterns per dimension), so that the general walk cbh_check_kernel* decides:
the two copies of the interpreter's LDS set-up (cbh_check_walk2.h, cbh_check_wave.h).  Tiers and roads as in
tests/test_string_limits.py: *_on_emulator (the kernels on the wave emulator, the family from hostsim_last_kind), *_on_simulator
(the library on tests/sim_engine.py: dict road, device road cbh_wire_flatten -> cbh_check_resident, cbh_wire_check_pb),
*_on_gpu.  Per layer: exactly the pairs built to exceed a limit are flagged, every other pair equals the oracle, and per label the
decided pairs hold an ALLOW and a DENY.  Only the step-budget layer has no exact flagged set: there every pair equals the oracle
or is flagged, and per condition the flagged lengths are upward closed - together: no length comes back unflagged and wrong.
Its requests are decided one batch per length, since spending the budget flags the whole wave; on the library they take the device
road (the emulator and one simulator case take the dict road).

Mutation check (each mutant on a scratch copy, CPU tier, never committed; "older" = the CPU tier of test_list_ops,
test_fuzz_parity, test_math_bind_split, test_hostsim_cel_kats and test_string_limits[arena]).
   1  the parent's count (no bound)        killed: test_on_emulator / test_on_simulator[counter_w | counter_g] (h16385_front, _back, _every_other and
                                           _as_map, h32769_front: ALLOW where DENY is wanted); every other test of the module passes -
                                           this IS the parent with the module added.  older: all pass
   2  the count's mask 0x3FFF -> 0x1FFF    passes, and must, now: the count never exceeds 48 (filter / map) or 2 (exists_one) - an
                                           equivalent mutant since the fix (not run together with mutant 1).  older: all pass
   3  ITS_MAP ignored in OP_ITER_NEXT      killed: test_on_emulator[ragged_* | nesting_*] (the map lanes among lists, map_of_lists).  older: all pass
   4  the per-turn release dropped         killed: test_on_emulator[arena_* | nesting_*] (in_exists: flagged where every turn fits;
                                           range_of_outer).  older: all pass
   5  ... applied to map as well           killed: test_on_emulator[arena_*] (in_map: decided where turn k no longer fits).  older: all pass
   6  n > ARENA - ap -> >= (OP_ITER_BEGIN) killed: test_on_emulator[ragged_* | arena_*] (a range of exactly 48).  older: all pass
      the same in OP_LISTOP                killed: test_on_emulator[arena_* | concatenation_*];  in OP_LISTFN (reverse, lists.range):
                                           test_on_emulator[arena_*].  older: all pass, both
   7  intersect's swap removed             killed: test_on_emulator[arena_*] (`intersect`: 40 entries taken, the shorter operand fits,
                                           the longer does not).  older: test_list_ops fails too - the control
   8  ITS_ENTRY_LIVE ignored, OP_ITER_END  killed: test_on_emulator[ragged_*] (the lanes a condition tree switched off).  older:
                                           test_fuzz_parity::test_fuzz_store[11 | 15 | 22 | 26] and test_math_bind_split[math] fail too
   9  the loop left on the lane's own      passes on the emulator, and must: its lanes are fibers with a program counter each, so a
      `more`, not on wave_ballot(more)     lane that leaves alone is still right there (on the device the counter is the wave's).  The
                                           mutant the emulator can show - the wave leaves as soon as ANY lane is done,
                                           wave_ballot(!more) != 0 - is killed by every test_on_emulator case; older: 14 tests fail too
  10  `i < 0xFFFFF` dropped, OP_ITER_NEXT  passes: the equivalent mutant - the step budget ends a loop long before (see the comment there)
  11  all: ITS_ERRSEEN read before         killed: test_on_emulator[errors_*] (an erring element beside a false one).  older: all pass
      ITS_DECIDED at OP_ITER_END
"""
import numpy as np
import pytest

from cerbos_amd import namer, wire
from cerbos_amd.flatten import Flattener
from cerbos_amd.lower import celc
from cerbos_amd.lower.blob import lower_rule_table
from cerbos_amd.policy.loader import policies_from_docs
from cerbos_amd.ruletable.build import rule_table_from_policies
from oracle.check import EvalParams, RuleTableOracle
from test_string_limits import (API, EFFECT_ALLOW, F_WANT_DR, NOW, ST_CEL_ERROR, ST_UNSUPPORTED, Layer, _constants, cond_store, header_value,
                                judge_outputs, request)

ITERS, LOCALS, ARENA, COUNT_BITS, STEPS = 2, 4, 48, 14, 1_000_000
WRAP = 1 << COUNT_BITS                      # 16 384: the hit that carried into ITS_MAP
KIND = "c"
WALK2_GLOBS = 16                            # lower/blob.py WALK2_MAX_GLOBS
ROADS = ("w", "g")


def test_the_limits_are_the_headers():
    import re
    from cerbos_amd.lower import blob
    assert header_value("CBH_MAX_ITERS", "cbh_vm.h") == ITERS == celc.MAX_ITERS
    assert header_value("CBH_MAX_LOCALS", "cbh_vm.h") == LOCALS == celc.MAX_LOCALS
    assert header_value("CBH_ARENA_ENTRIES", "cbh_blob.h") == ARENA
    assert header_value("ITS_MAP", "cbh_interp.h") == 1 << (16 + COUNT_BITS) and header_value("ITS_FAIL", "cbh_interp.h") == 1 << 31
    assert blob.WALK2_MAX_GLOBS == WALK2_GLOBS
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cerbos_amd", "csrc", "cbh_interp.h")) as fh:
        text = fh.read()
    assert re.search(r"steps < (\d+)u", text).group(1) == str(STEPS)
    assert "(st >> 16) & 0x%Xu" % (WRAP - 1) in text and "(start << 26) | (ap << 20)" in text and "iw & 0xFFFFFu" in text


# ---- a layer: the requests and what must happen to them, once; a store per road; the oracle's answers, once


def policy_key(capi, lt, word, inp):
    """the policy word of a result (cerbos_amd/engine.py _policy_string)"""
    kind, ident = word >> 28, word & 0x0FFFFFFF
    if kind == capi.P_EMPTY:
        return ""
    if kind == capi.P_NO_MATCH:
        return "NO_MATCH"
    if kind == capi.P_TABLE:
        return lt.policy_keys[ident]
    assert kind == capi.P_RESOURCE, kind
    return namer.policy_key_from_fqn(namer.resource_policy_fqn(inp["resource"]["kind"], "default", lt.scopes[ident]))


class Spec:
    """conds: {action: expression}; inputs; over: the pairs built to exceed a limit; groups: {label: pairs};
    refused: how many expressions the lowering refuses"""

    def __init__(self, name, conds, inputs, over=(), groups=None, refused=0):
        self.name, self.conds, self.inputs, self.over, self.groups, self.refused = name, conds, inputs, set(over), groups or {}, refused
        self.layers = {}

    def layer(self, road):
        if road not in self.layers:
            self.layers[road] = CompLayer(self, road)
        return self.layers[road]


def general_walk_doc():
    """a resource kind no request names, with one action glob more than cbh_walk2_kernel keeps bits for"""
    return {"apiVersion": API, "resourcePolicy": {"resource": "globs", "version": "default", "rules": [
        {"actions": ["g%d:*" % i], "roles": ["*"], "effect": "EFFECT_ALLOW"} for i in range(WALK2_GLOBS + 1)]}}


def expressions(match):
    """the expressions of a condition: one, or the leaves of a match tree"""
    if isinstance(match, str):
        return [match]
    if "expr" in match:
        return [match["expr"]]
    return [e for kid in next(iter(match.values()))["of"] for e in expressions(kid)]


class CompLayer(Layer):
    def __init__(self, spec, road):
        self.spec, self.road = spec, road
        self.name, self.inputs, self.over, self.groups, self.loud = "%s_%s" % (spec.name, road), spec.inputs, spec.over, spec.groups, False
        docs = [{"apiVersion": API, "resourcePolicy": {"resource": KIND, "version": "default", "rules": [
            {"actions": [a], "roles": ["*"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": m} if isinstance(m, str) else m}} for a, m in spec.conds.items()]}}]
        docs += [general_walk_doc()] if road == "g" else []
        self.rt = rule_table_from_policies(policies_from_docs(docs))
        self.lt = lower_rule_table(self.rt)
        assert len(self.lt.unsupported) == spec.refused, (self.name, self.lt.unsupported)
        assert bool(self.lt.walk2_refused) == (road == "g"), (self.name, self.lt.walk2_refused)
        self.kinds = (0,) if road == "g" else (2,)
        self.plan_ok = (lambda plan: plan.startswith("cbh_check_kernel")) if road == "g" else (lambda plan: "cbh_walk2_interp_kernel" in plan)
        assert len({i["requestId"] for i in self.inputs}) == len(self.inputs)
        if not hasattr(spec, "want"):    # (the other road's store differs in a kind no request names)
            orc = RuleTableOracle(self.rt)
            want = [orc.check(i, EvalParams(now_ns=NOW)) for i in self.inputs]
            by_expr = {e: a for a, m in spec.conds.items() for e in expressions(m)}
            assert len(by_expr) == sum(len(expressions(m)) for m in spec.conds.values())      # an evaluation error names its expression: one action each
            spec.errors = {(i["requestId"], by_expr[e["celError"]["expression"]]) for i, w in zip(self.inputs, want) for e in w["evaluationErrors"]}
            spec.want = want
        self.want, self.errors = spec.want, spec.errors
        self.batch = Flattener(self.lt).flatten(self.inputs, sort=False)
        assert self.batch.n_requests == len(self.inputs)
        self.data, self.off = wire.pack_messages([wire.encode_check_input(i) for i in self.inputs])

    def check_oracle(self):
        ids = {(i["requestId"], a) for i in self.inputs for a in i["actions"]}
        assert self.over <= ids and self.errors <= ids, (self.name, sorted(self.over - ids)[:3])
        index = {i["requestId"]: k for k, i in enumerate(self.inputs)}
        for label, pairs in self.groups.items():
            seen = {self.want[index[r]]["actions"][a]["effect"] for r, a in pairs if (r, a) not in self.over}
            if seen or not set(pairs) <= self.over:      # (a label whose pairs are ALL built to be flagged has nothing decided)
                assert seen == {"EFFECT_ALLOW", "EFFECT_DENY"}, (self.name, label, "the decided pairs do not discriminate", seen)
        grouped = {p for pairs in self.groups.values() for p in pairs}
        assert ids - self.over <= grouped | self.errors, (self.name, "decided pairs in no group", sorted(ids - self.over - grouped - self.errors)[:4])
        assert len(self.inputs) <= 400, (self.name, len(self.inputs))


def judge(capi, layer, res, what, exact=True):
    """per tuple, in input order: flagged exactly where the layer says; effect, policy key and status equal to the oracle's
    everywhere else.  -> the flagged pairs"""
    flagged, t = set(), 0
    for inp, w in zip(layer.inputs, layer.want):
        for a in inp["actions"]:
            pair = (inp["requestId"], a)
            if int(res.status[t]) & ST_UNSUPPORTED:
                flagged.add(pair)
            else:
                want = w["actions"][a]
                have = "EFFECT_ALLOW" if int(res.effect[t]) == EFFECT_ALLOW else "EFFECT_DENY"
                assert have == want["effect"], (layer.name, what, pair, want["effect"], "is wanted")
                assert bool(int(res.status[t]) & ST_CEL_ERROR) == (pair in layer.errors), (layer.name, what, pair, "evaluation error", pair in layer.errors)
                assert policy_key(capi, layer.lt, int(res.policy[t]), inp) == want["policy"], (layer.name, what, pair, want["policy"])
            t += 1
    assert t == len(res.effect)
    if exact:
        assert flagged == layer.over, (layer.name, what, "flagged but not built to be", sorted(flagged - layer.over)[:4], "built to be flagged but decided", sorted(layer.over - flagged)[:4])
    return flagged


def run_on_emulator(layer, exact=True):
    import hostsim_api
    from cerbos_amd import capi
    res = hostsim_api.check(layer.lt, layer.batch, NOW, F_WANT_DR)
    assert hostsim_api.last_kind() in layer.kinds, (layer.name, hostsim_api.last_kind())
    return [judge(capi, layer, res, "emulator", exact)]


def run_on_library(capi, layer, exact=True, dict_road=True):
    _constants(capi)
    table = capi.Table(layer.lt.blob)
    out = []
    try:
        if dict_road:
            res = table.check(layer.batch, now_ns=NOW, flags=F_WANT_DR)
            out.append(judge(capi, layer, res, "dict road, cbh_check_batch", exact))
        db = table.wire_flatten(layer.data, layer.off)
        try:
            assert db.wire_info["n_host"] == 0, db.wire_info
            table.launch(db, now_ns=NOW, flags=F_WANT_DR)
            out.append(judge(capi, layer, table.download(db), "device road, cbh_check_resident", exact))
            plan = table.plan(db, flags=F_WANT_DR)
            assert layer.plan_ok(plan), (layer.name, plan)    # a test that passes because another kernel decided proves nothing
        finally:
            db.close()
        if exact:
            raw, flags = table.wire_check_pb(layer.data, layer.off, now_ns=NOW, flags=F_WANT_DR)
            judge_outputs(layer, raw, flags, "device road, cbh_wire_check_pb")
    finally:
        table.close()
    return out


def grouped(groups, label, rid, actions):
    for a in actions:
        groups.setdefault("%s %s" % (a, label), []).append((rid, a))


# ---- 1. the width of the count


HITS = (0, 1, 2, WRAP - 1, WRAP, WRAP + 1, WRAP + 2, 2 * WRAP + 1)
assert HITS[3:] == (16_383, 16_384, 16_385, 16_386, 32_769)
END, OTHER = -0.25, -0.75     # every list ends with END, no hit; the controls look for P.attr.z = END (decided by the LAST element) or OTHER (never)
COUNTER_CONDS = {
    "one": "R.attr.xs.exists_one(x, x > 0.0)", "one_camel": "R.attr.xs.existsOne(x, x > 0.0)",
    "one2": "R.attr.xs.exists_one(i, v, v > 0.0 && i >= 0)", "one2_camel": "R.attr.xs.existsOne(i, v, v > 0.0)",
    "all": "R.attr.xs.all(x, x != P.attr.z)", "exists": "R.attr.xs.exists(x, x == P.attr.z)",        # the controls: they do not count
    "all2": "R.attr.xs.all(i, v, v != P.attr.z)", "exists2": "R.attr.xs.exists(i, v, v == P.attr.z)",
}


def counter_lists():
    """(name, list, big): h hits at the front, at the back, every other element; one hit in a long list (the ALLOW of the long
    lists); and, for 16 385 hits, the list of the issue's second symptom: after the 16 384th hit the elements are no hits but for
    ONE at index 2 * 16 384 - a lane that takes its list for a map from turn 16 384 on reads entry 2 * i for the key, finds that
    hit on turn 16 384 and nothing after it"""
    out = []
    for h in HITS:
        big = h >= WRAP - 1
        out.append(("h%d_front" % h, [1.0] * h + [0.0] * 5, big))
        if not big or h in (WRAP, WRAP + 1):      # (the long lists go to a handful of requests)
            out.append(("h%d_back" % h, [0.0] * 5 + [1.0] * h, big))
            out.append(("h%d_every_other" % h, [1.0, 0.0] * h, big))
    out.append(("h1_long_front", [1.0] + [0.0] * (WRAP + 5), True))
    out.append(("h1_long_back", [0.0] * (WRAP + 5) + [1.0], True))
    out.append(("h0_long", [0.0] * (WRAP + 6), True))
    out.append(("h16385_as_map", [1.0] * WRAP + [0.0] * WRAP + [1.0] + [0.0] * 3, True))
    return out


def make_counter():
    inputs, groups = [], {}
    for k, (name, xs, big) in enumerate(counter_lists()):
        inputs.append(request(name, KIND, list(COUNTER_CONDS), pattr={"z": OTHER if k % 2 else END}, rattr={"xs": xs + [END]}))
        grouped(groups, "long" if big else "short", name, COUNTER_CONDS)
    assert sum(len(i["resource"]["attr"]["xs"]) > WRAP for i in inputs) <= 16
    return Spec("counter", COUNTER_CONDS, inputs, groups=groups)


# ---- 2. ragged waves


RAGGED_LENGTHS = (0, 1, 2, 3, ARENA - 1, ARENA, ARENA + 1, 300)
RAGGED_CONDS = {
    "all": "R.attr.xs.all(x, x != P.attr.z)", "exists": "R.attr.xs.exists(x, x == P.attr.z)", "one": "R.attr.xs.exists_one(x, x == P.attr.z)",
    "filter": "R.attr.xs.filter(x, x != P.attr.z).size() == int(P.attr.n)",
    "map": "P.attr.w in R.attr.xs.map(x, x * 2.0)",
    "map3": "R.attr.xs.map(x, x == P.attr.z, x * 2.0).size() == int(P.attr.c)",
    "tl": "P.attr.w in R.attr.xs.transformList(i, v, v * 2.0)",
    "tlp": "R.attr.xs.transformList(i, v, v == P.attr.zv, i).size() == int(P.attr.c)",
    "all2": "R.attr.xs.all(i, v, v != P.attr.zv)", "exists2": "R.attr.xs.exists(k, v, v == P.attr.zv)",
    # `&&`, `||` and `?:` of an expression evaluate BOTH sides on every lane (lower/celc.py: uniform control flow, errors absorbed as CEL
    # absorbs them): the lane is live in a macro CEL would skip, and a limit exceeded there flags the pair whatever `on` is
    "sc_and": "P.attr.on && R.attr.xs.exists(x, x == P.attr.z)",
    "sc_or": "P.attr.on || R.attr.xs.all(x, x != P.attr.z)",
    "sc_tern": "P.attr.on ? R.attr.xs.exists_one(x, x == P.attr.z) : P.attr.alt",
    "sc_filter": "P.attr.on && R.attr.xs.filter(x, x != P.attr.z).size() == int(P.attr.n)",
    "sc_map": "!P.attr.on || P.attr.w in R.attr.xs.map(x, x * 2.0)",
    # a condition TREE stops evaluating a lane once it is decided (all: at the first false, any / none: at the first true): that lane is
    # not live, sits the loop out and keeps its status - no flag, no evaluation error, whatever its range is
    "tree_all": {"all": {"of": [{"expr": "P.attr.on"}, {"expr": "R.attr.xs.filter(e, e != P.attr.z).size() == int(P.attr.n)"}]}},
    "tree_any": {"any": {"of": [{"expr": "P.attr.on == true"}, {"expr": "P.attr.w in R.attr.xs.map(e, e * 2.0)"}]}},
    "tree_none": {"none": {"of": [{"expr": "true == P.attr.on"}, {"expr": "R.attr.xs.transformList(i, e, e == P.attr.zv, i).size() == int(P.attr.c)"}]}},
    "tree_one": {"all": {"of": [{"expr": "P.attr.on != false"}, {"expr": "R.attr.xs.exists_one(e, e == P.attr.z)"}, {"expr": "R.attr.xs.all(j, e, e != -5.0)"}]}},
}
RAGGED_BUILD = ("filter", "map", "map3", "tl", "tlp", "sc_filter", "sc_map", "tree_all", "tree_any", "tree_none")     # reserve the range's length
RAGGED_LIVE = {"tree_all": True, "tree_any": False, "tree_none": False}                        # the value of `on` with which the lane reaches the macro


def ragged_lanes():
    """(name, xs or None, z, zv): lists with the deciding element first, last, absent, twice; no attribute; a string; a number; maps"""
    out = []
    for n in RAGGED_LENGTHS:
        xs = [float(j + 1) for j in range(n)]
        out.append(("l%d_absent" % n, xs, -1.0, -1.0))
        if n >= 1:
            out.append(("l%d_first" % n, xs, xs[0], xs[0]))
        if n >= 2:
            out.append(("l%d_last" % n, xs, xs[-1], xs[-1]))
            out.append(("l%d_twice" % n, xs[:-1] + xs[:1], xs[0], xs[0]))
    out += [("missing", None, 1.0, 1.0), ("string", "abc", 1.0, 1.0), ("number", 7.0, 7.0, 7.0),
            ("map_hit", {"a": 1.0, "b": 2.0, "c": 3.0}, "a", 1.0), ("map_value_twice", {"a": 1.0, "b": 2.0, "c": 1.0}, "c", 1.0),
            ("map_miss", {"a": 1.0, "b": 2.0}, "zz", 9.0), ("map_empty", {}, "a", 1.0)]
    return out


def make_ragged():
    """every lane kind with on = true and false, the counts right and wrong by one; shuffled, so that a wave holds every kind"""
    cases = [(name, xs, z, zv, on, good) for name, xs, z, zv in ragged_lanes() for on in (True, False) for good in (True, False)]
    order = np.random.default_rng(64).permutation(len(cases))
    inputs, over, groups = [], set(), {}
    for k in order:
        name, xs, z, zv, on, good = cases[k]
        rid = "%s_%s_%s" % (name, "on" if on else "off", "good" if good else "bad")
        elements = list(xs) if isinstance(xs, (list, dict)) else []
        hits = elements.count(z)
        w = 2.0 * z if isinstance(z, float) else 2.0
        pattr = {"z": z, "zv": zv, "on": on, "alt": good, "w": w, "n": float(len(elements) - hits + (not good)), "c": float(hits + (not good))}
        inputs.append(request(rid, KIND, list(RAGGED_CONDS), pattr=pattr, rattr={} if xs is None else {"xs": xs}))
        long = isinstance(xs, list) and len(xs) > ARENA
        for a in RAGGED_CONDS:
            live = RAGGED_LIVE.get(a, on) == on
            if a in RAGGED_BUILD and long and live:
                over.add((rid, a))
        label = "beyond the arena" if long else "map" if isinstance(xs, dict) else "a list or no range"      # (no range: one answer)
        arithmetic = ("map", "map3", "tl", "sc_map")      # (x * 2.0 of a map's key: an evaluation error, one answer)
        grouped(groups, label, rid, [a for a in RAGGED_CONDS if not a.startswith("tree_") and not (label == "map" and a in arithmetic)])
        grouped(groups, "a list or no range", rid, [a for a in arithmetic if label == "map"])
        grouped(groups, "", rid, [a for a in RAGGED_CONDS if a.startswith("tree_")])     # (a lane that is not live has one answer)
    assert len(inputs) > 128     # more than two waves
    return Spec("ragged", RAGGED_CONDS, inputs, over=over, groups=groups)


# ---- 3. errors: absorbed, propagated


def error_conds():
    """per kind of error a predicate p(x): true for T, false for F, an error for E"""
    preds = {"type": ("ty", "x > 0.0"), "div": ("dz", "6 / int(x) > 0"), "key": ("mk", "x.k > 0.0")}
    conds = {}
    for kind, (attr, p) in preds.items():
        conds[kind + "_all"] = "R.attr.%s.all(x, %s)" % (attr, p)
        conds[kind + "_exists"] = "R.attr.%s.exists(x, %s)" % (attr, p)
        conds[kind + "_one"] = "R.attr.%s.exists_one(x, %s)" % (attr, p)
        conds[kind + "_filter"] = "R.attr.%s.filter(x, %s).size() == 1" % (attr, p)
    conds["filter_not_bool"] = "R.attr.bs.filter(b, b).size() == 1"
    conds["map"] = "R.attr.dz.map(x, 6 / int(x)).size() == 2"
    conds["map3_rejects"] = "R.attr.dz.map(x, x > 0.5, 6 / int(x)).size() == 1"          # the predicate rejects the erring element (0.0)
    conds["map3_passes"] = "R.attr.dz.map(x, x > -1.0, 6 / int(x)).size() == 1"          # ... lets it through (and rejects F, -2.0)
    conds["tl_rejects"] = "R.attr.dz.transformList(i, x, x > 0.5, 6 / int(x)).size() == 1"
    conds["tl_passes"] = "R.attr.dz.transformList(i, x, x > -1.0, 6 / int(x)).size() == 1"
    return conds


ERROR_VALUES = {"ty": {"T": 1.0, "F": -1.0, "E": "s"}, "dz": {"T": 2.0, "F": -2.0, "E": 0.0},
                "mk": {"T": {"k": 1.0}, "F": {"k": -1.0}, "E": {"j": 1.0}}, "bs": {"T": True, "F": False, "E": 1.0}}


def make_errors():
    """every list of one to four elements over {T, F, E}: the erring element first, last, before and after the deciding one"""
    import itertools
    conds = error_conds()
    inputs, groups, intended = [], {}, set()
    for n in (1, 2, 3, 4):
        for pat in itertools.product("TFE", repeat=n):
            rid = "".join(pat)
            inputs.append(request(rid, KIND, list(conds), rattr={attr: [vals[c] for c in pat] for attr, vals in ERROR_VALUES.items()}))
            grouped(groups, "", rid, conds)
            for a in conds:      # where the macro's value is an error, from the macros' definitions
                err = "E" in pat
                if a.endswith("_all"):
                    err = err and "F" not in pat
                elif a.endswith("_exists"):
                    err = err and "T" not in pat
                elif a.endswith("_rejects"):
                    err = False
                if err:
                    intended.add((rid, a))
    spec = Spec("errors", conds, inputs, groups=groups)
    spec.intended = intended
    return spec


# ---- 4. the arena's accounting


def arena_cases():
    """(lx, ly, lz, k): xs = 1 .. lx, ys = 2, 4 .. 2 * ly, zs = 1 .. lz, k an int the request brings"""
    out = []
    for lx in (0, 1, ARENA - 1, ARENA, ARENA + 1, 300):
        for ly in (0, 5, ARENA):
            out.append((lx, ly, 0, lx))
    for lx, ly in ((24, 24), (24, 25), (25, 24), (1, 47), (1, 48), (47, 1), (40, 8), (40, 9)):     # two results: 48 and 49 together
        out.append((lx, ly, 0, 3))
    for lx, ly in ((5, 8), (6, 8), (6, 7), (7, 6), (4, 11), (4, 12), (10, 48), (10, 49), (3, 15), (2, 23), (2, 24)):   # a filter in a map's body: the turn it no longer fits
        out.append((lx, ly, 0, 2))
    for lx, ly, lz in ((5, 20, 40), (20, 5, 40), (8, 20, 40), (9, 20, 40), (20, 9, 40), (20, 20, 28), (20, 20, 29), (9, 9, 40), (8, 8, 40)):   # intersect's swap
        out.append((lx, ly, lz, 1))
    for k in (0, 1, ARENA - 1, ARENA, ARENA + 1):
        out.append((300, 300, 0, k))
    return out


ARENA_CONDS = {
    "filter": "R.attr.xs.filter(x, x > P.attr.t).size() == int(P.attr.n_filter)",
    "map": "P.attr.w in R.attr.xs.map(x, x + 0.5)",
    "two": "R.attr.xs.filter(x, x > P.attr.t).size() + R.attr.ys.filter(y, y > P.attr.t).size() == int(P.attr.n_two)",
    "cat_literal": "(R.attr.xs + [0.5]).size() == int(P.attr.n_cat)",
    "cat_two": "([] + R.attr.xs + R.attr.ys).size() == int(P.attr.n_cat2)",
    "intersect": "R.attr.zs.filter(z, z > 0.0).size() + intersect(R.attr.xs, R.attr.ys).size() == int(P.attr.n_int)",
    "except": "R.attr.zs.filter(z, z > 0.0).size() + except(R.attr.xs, R.attr.ys).size() == int(P.attr.n_exc)",
    "reverse": "R.attr.xs.slice(0, int(P.attr.k)).reverse()[0] == P.attr.w_rev",
    "range": "lists.range(int(P.attr.k)).exists(i, double(i) == P.attr.w_range)",
    "slice": "R.attr.xs.slice(0, int(P.attr.k)).size() == int(P.attr.n_slice)",
    "in_exists": "R.attr.xs.exists(x, R.attr.ys.filter(y, y > x).size() == int(P.attr.n_inner))",
    "in_map": "R.attr.xs.map(x, R.attr.ys.filter(y, y > x).size()).size() == int(P.attr.n_outer)",
    "has": "hasIntersection(R.attr.xs, R.attr.ys)", "subset": "isSubset(R.attr.ys, R.attr.xs)", "in": "P.attr.w_in in R.attr.xs",
}
CROSS_CONDS = {     # 1 against 1.0 against 1u; empty operands; duplicates
    "has_int": "hasIntersection(R.attr.xs, [1])", "has_uint": "hasIntersection([1u], R.attr.xs)", "has_both": "hasIntersection([7, 7u, 1u], R.attr.xs)",
    "sub_int": "isSubset([1, 1u, 1.0, 1], R.attr.xs)", "sub_of": "isSubset(R.attr.xs, [1, 2u, 2, 3.0])", "sub_dup": "isSubset(R.attr.xs, R.attr.ys)",
}
CROSS_LISTS = ([], [1.0], [2.0], [1.0, 1.0], [2.0, 1.0, 2.0], [1.0, 2.0, 3.0, 3.0], [4.0], [1.5], [3.0, 3.0, 3.0])


def arena_fits(cond, lx, ly, lz, k):
    """the rules of the module's text, for the expression `cond`"""
    if cond in ("filter", "map"):
        return lx <= ARENA
    if cond == "two":
        return lx + ly <= ARENA
    if cond == "cat_literal":
        return lx + 1 <= ARENA
    if cond == "cat_two":          # [] + xs takes lx, (that) + ys takes lx + ly more
        return lx <= ARENA and ly <= ARENA and lx + lx + ly <= ARENA
    if cond == "intersect":
        return lz <= ARENA and max(lx, ly) <= ARENA and lz + min(lx, ly) <= ARENA
    if cond == "except":
        return lz <= ARENA and max(lx, ly) <= ARENA and lz + lx <= ARENA
    if cond in ("reverse", "range"):
        return k <= ARENA
    if cond == "in_exists":        # released every turn
        return lx == 0 or ly <= ARENA
    if cond == "in_map":           # turn j needs lx + j * ly
        return lx <= ARENA and lx + lx * ly <= ARENA
    return True                    # slice, hasIntersection, isSubset, in: no arena


def make_arena():
    inputs, over, groups = [], set(), {}
    conds = dict(ARENA_CONDS, **CROSS_CONDS)
    for j, (lx, ly, lz, k) in enumerate(arena_cases()):
        xs, ys, zs = [float(i + 1) for i in range(lx)], [float(2 * i + 2) for i in range(ly)], [float(i + 1) for i in range(lz)]
        k = min(k, lx)
        t = float(lx // 2)
        good = j % 2 == 0
        bump = 0.0 if good else 1.0
        both = [x for x in xs if x in ys]
        pattr = {
            "t": t, "k": float(k), "w": (xs[-1] if xs else 0.0) + 0.5 + bump, "w_in": (xs[-1] if xs else 1.0) + bump,
            "n_filter": sum(x > t for x in xs) + bump, "n_two": sum(x > t for x in xs) + sum(y > t for y in ys) + bump,
            "n_cat": lx + 1 + bump, "n_cat2": lx + ly + bump,
            "n_int": lz + (len(both) if lx <= ly else len([y for y in ys if y in xs])) + bump, "n_exc": lz + lx - len(both) + bump,
            "w_rev": (xs[k - 1] if k else 0.0) + bump, "w_range": float(k - 1) + bump, "n_slice": k + bump,
            "n_inner": (sum(y > xs[-1] for y in ys) if xs else 0) + bump, "n_outer": lx + bump,
        }
        rid = "x%d_y%d_z%d_k%d_%d" % (lx, ly, lz, k, j)
        inputs.append(request(rid, KIND, list(ARENA_CONDS), pattr=pattr, rattr={"xs": xs, "ys": ys, "zs": zs}))
        for a in ARENA_CONDS:
            if not arena_fits(a, lx, ly, lz, k):
                over.add((rid, a))
        grouped(groups, "", rid, [a for a in ARENA_CONDS if a != "reverse" or k])       # (reverse of an empty list: [0] is an evaluation error)
    for j, xs in enumerate(CROSS_LISTS):
        for i, ys in enumerate(([1.0, 2.0], [])):
            rid = "cross%d_%d" % (j, i)
            inputs.append(request(rid, KIND, list(CROSS_CONDS), rattr={"xs": xs, "ys": ys, "zs": []}))
            grouped(groups, "", rid, CROSS_CONDS)
    spec = Spec("arena", conds, inputs, over=over, groups=groups)
    for a in ("filter", "map", "two", "cat_literal", "cat_two", "intersect", "except", "reverse", "range", "in_exists", "in_map"):   # both sides of every rule
        assert {arena_fits(a, *c[:3], min(c[3], c[0])) for c in arena_cases()} == {True, False}, a
    return spec


# ---- 5. nesting


NEST_CONDS = {
    # depth two, four locals: every inner list holds its own index; some inner list lies above its indices
    "own_index": "R.attr.ll.all(i, v, v.exists(j, w, w == double(i) && j >= 0))",
    "above": "R.attr.ll.exists(i, v, v.all(j, w, w > double(j) + double(i) + P.attr.d))",
    "map_of_lists": "R.attr.ml.all(k, v, v.exists(j, w, w == P.attr.z && k != 'none'))",
    "range_of_outer": "R.attr.ns.all(n, lists.range(int(n)).exists_one(i, double(i) == n - 1.0))",     # the inner range's length IS the outer variable
    "bind_inside": "R.attr.ll.all(v, cel.bind(n, v.size(), v.exists(w, w == double(n) + P.attr.d)))",
    "bind_around": "cel.bind(t, P.attr.z, R.attr.ll.exists(v, v.exists(w, w == t)))",
    "bind_between": "R.attr.ll.exists(i, v, cel.bind(t, P.attr.z + double(i), v.exists(w, w == t)))",
    "five_locals": "cel.bind(t, P.attr.z, R.attr.ll.all(i, v, v.exists(j, w, w == t || w == double(i))))",          # refused: a fifth local
    "depth_three": "R.attr.lll.exists(a, a.exists(b, b.exists(c, c == P.attr.z)))",                                 # refused: a third loop
}
NEST_REFUSED = ("five_locals", "depth_three")


def make_nesting():
    rng = np.random.default_rng(5)
    inputs, over, groups = [], set(), {}
    for k in range(96):
        n_outer = int(rng.integers(1, 7))
        ll = []
        for i in range(n_outer):
            inner = [float(v) for v in rng.integers(0, 9, int(rng.integers(0, 12)))]
            if k % 3 and float(i) not in inner:
                inner.insert(int(rng.integers(0, len(inner) + 1)), float(i))
            ll.append(inner)
        if k % 4 == 0:
            ll.append([float(len(ll) + j + 2 + k % 8) for j in range(int(rng.integers(1, 40)))])    # an inner list above its indices, of another length
        if k % 5 == 0:
            ll = [v + [float(len(v) + 1)] for v in ll]
        ml = {"k%d" % i: v for i, v in enumerate(ll)}
        z = float(rng.integers(0, 4))
        if k % 2:
            ml = {key: v + [z] for key, v in ml.items()}
        ns = [float(v) for v in rng.integers(1, 30, int(rng.integers(0, 6)))] + ([0.0] if k % 6 == 5 else [])
        rid = "n%d" % k
        inputs.append(request(rid, KIND, list(NEST_CONDS), pattr={"z": z, "d": float(k % 2)}, rattr={"ll": ll, "ml": ml, "ns": ns, "lll": [ll, [[z]]]}))
        assert ll and ll[0] is not None     # the refused macros are reached: the enclosing ranges are not empty
        over |= {(rid, a) for a in NEST_REFUSED}
        grouped(groups, "", rid, [a for a in NEST_CONDS if a not in NEST_REFUSED])
    inputs.append(request("empty", KIND, list(NEST_CONDS), pattr={"z": 1.0, "d": 0.0}, rattr={"ll": [], "ml": {}, "ns": [], "lll": []}))   # reaches no refused macro: decided
    grouped(groups, "", "empty", [a for a in NEST_CONDS if a not in NEST_REFUSED])
    groups["refused, not reached"] = [("empty", a) for a in NEST_REFUSED]      # all() of nothing, exists() of nothing
    return Spec("nesting", NEST_CONDS, inputs, over=over, groups=groups, refused=len(NEST_REFUSED))


# ---- concatenation of two lists of the request


CAT_CONDS = {
    "two_request_lists": "(R.attr.xs + R.attr.xs).size() == int(P.attr.n) * 2",      # neither operand is visibly a list: OP_ADD, flagged
    "literal_right": "(R.attr.xs + [9.5]).size() == int(P.attr.n) + 1",
    "literal_left": "([] + R.attr.xs + R.attr.xs).size() == int(P.attr.n) * 2",
    "filter_left": "(R.attr.xs.filter(x, true) + R.attr.xs).size() == int(P.attr.n) * 2",
}


def make_concatenation():
    inputs, over, groups = [], set(), {}
    for k, n in enumerate((0, 1, 2, 5, 16)):
        for good in (True, False):
            rid = "cat%d_%s" % (n, good)
            inputs.append(request(rid, KIND, list(CAT_CONDS), pattr={"n": float(n + (not good))}, rattr={"xs": [float(i) for i in range(n)]}))
            over.add((rid, "two_request_lists"))
            grouped(groups, "", rid, [a for a in CAT_CONDS if a != "two_request_lists"])
    return Spec("concatenation", CAT_CONDS, inputs, over=over, groups=groups)


MAKERS = {"counter": make_counter, "ragged": make_ragged, "errors": make_errors, "arena": make_arena, "nesting": make_nesting,
          "concatenation": make_concatenation}
_SPECS = {}


def layer(name, road):
    if name not in _SPECS:
        _SPECS[name] = MAKERS[name]()
    return _SPECS[name].layer(road)


CASES = [(name, road) for name in MAKERS for road in ROADS]
IDS = ["%s_%s" % c for c in CASES]


# ---- 6. the step budget: one small batch per length


BUDGET_CONDS = {
    # a single loop over a long list, decided by its last element (a body of some thirty operations, so that the budget is spent by a
    # list of tens of thousands of elements and building the lists does not dominate the test)
    "last_decides": "R.attr.xs.all(x, x%s != P.attr.z)" % (" + 1.0" * 12),
    "nested": "R.attr.xs.all(x, R.attr.ys.all(y, y%s != x + P.attr.z))" % (" + 1.0" * 5),      # n * n turns, decided by the last turn of all
}
# two lengths below and two above where the budget is spent - STEPS / (a turn's operations): some 34 000 elements; some 250 * 250 turns.
# (a spent budget is a second of GPU time: no more lengths than the two properties need)
BUDGET_LENGTHS = {"last_decides": (1_000, 30_000, 36_000, 45_000), "nested": (30, 200, 290, 400)}
assert max(BUDGET_LENGTHS["last_decides"]) < 0xFFFFF // 2          # cbh_wire.h CBH_WIRE_MAX_VALUE_ENTRIES, with room


def budget_spec(cond, n):
    """two requests: the same list, decided ALLOW and DENY"""
    if cond == "last_decides":
        xs, ys = [1.0] * (n - 1) + [2.0], []
        zs = (14.0, 15.0)
    else:
        xs, ys = [float(i) for i in range(n)], [float(-i - 1) for i in range(n - 1)] + [float(n + 5)]
        zs = (11.0, 0.5)                # the last y + 5 equals the last x + 11; nothing equals x + 0.5
    inputs = [request("%s_%d_%d" % (cond, n, k), KIND, [cond], pattr={"z": z}, rattr={"xs": xs, "ys": ys}) for k, z in enumerate(zs)]
    return Spec("budget_%s_%d" % (cond, n), {cond: BUDGET_CONDS[cond]}, inputs, groups={cond: [(i["requestId"], cond) for i in inputs]})


def budget_layers(cond, road):
    key = ("budget", cond)
    if key not in _SPECS:
        _SPECS[key] = [budget_spec(cond, n) for n in BUDGET_LENGTHS[cond]]
    return [s.layer(road) for s in _SPECS[key]]


def check_budget(cond, road, run):
    """every pair equals the oracle or is flagged (judge); a batch is flagged as a whole or not at all; once a length is flagged,
    every longer one is; the shortest is decided and the longest flagged, so that both sides of the budget are there"""
    n_roads, flagged = None, []
    for lay in budget_layers(cond, road):
        lay.check_oracle()
        sets = run(lay)
        n_roads = len(sets)
        assert all(s in (set(), {(i["requestId"], cond) for i in lay.inputs}) for s in sets), (lay.name, sets)
        flagged.append([bool(s) for s in sets])
    for r in range(n_roads):
        col = [f[r] for f in flagged]
        print("step budget", cond, road, "road", r, "flagged:", dict(zip(BUDGET_LENGTHS[cond], col)))
        assert col == sorted(col), (cond, road, r, "a length is decided beyond a flagged one", list(zip(BUDGET_LENGTHS[cond], col)))
        assert not col[0] and col[-1], (cond, road, r, list(zip(BUDGET_LENGTHS[cond], col)))


# ---- CPU tier: what the generators must make happen


@pytest.mark.parametrize("name,road", CASES, ids=IDS)
def test_the_oracle_decides_and_the_pairs_discriminate(name, road):
    layer(name, road).check_oracle()


def test_errors_are_where_the_macros_put_them():
    """the oracle's evaluation errors, per action, are the ones the macros' definitions give for the lists built"""
    lay = layer("errors", "w")
    assert lay.errors == lay.spec.intended, (sorted(lay.errors - lay.spec.intended)[:5], sorted(lay.spec.intended - lay.errors)[:5])
    assert {a for _, a in lay.errors} == {a for a in lay.spec.conds if not a.endswith("_rejects")}     # every macro meets its error; the rejecting predicates never
    for name in ("counter", "nesting", "concatenation"):
        assert not layer(name, "w").errors, name


def test_nesting_beyond_the_limits_is_refused_at_lowering():
    lay = layer("nesting", "w")
    texts = {t for t, _ in lay.lt.unsupported}
    assert texts == {NEST_CONDS[a] for a in NEST_REFUSED}, lay.lt.unsupported
    assert all("nesting beyond the device limits" in why for _, why in lay.lt.unsupported)


def test_concatenation_needs_a_visible_list():
    """lower/celc.py _builds_list: which `+` becomes OP_LISTOP"""
    from cerbos_amd.cel.parser import parse      # the lowering's own parser: what _builds_list is given
    for a, e in CAT_CONDS.items():
        ast = parse(e)
        plus = ast[2][2]                   # (<a + b>.size()) == ...: the target of size()
        assert plus[0] == "bin" and plus[1] == "+", plus
        assert (celc._builds_list(plus[2]) or celc._builds_list(plus[3])) == (a != "two_request_lists"), a


# ---- CPU tier: the kernels on the wave emulator


@pytest.mark.parametrize("name,road", CASES, ids=IDS)
def test_on_emulator(name, road):
    run_on_emulator(layer(name, road))


@pytest.mark.parametrize("road", ROADS)
@pytest.mark.parametrize("cond", list(BUDGET_CONDS))
def test_step_budget_on_emulator(cond, road):
    check_budget(cond, road, lambda lay: run_on_emulator(lay, exact=False))


# ---- CPU tier: the library on the simulator


@pytest.fixture()
def engine():
    from sim_engine import sim_engine
    with sim_engine() as capi:
        yield capi


@pytest.mark.parametrize("name,road", CASES, ids=IDS)
def test_on_simulator(engine, name, road):
    run_on_library(engine, layer(name, road))


@pytest.mark.parametrize("cond,road", [("last_decides", "w"), ("nested", "g")])      # (a spent budget is a million steps on the CPU: one road each)
def test_step_budget_on_simulator(engine, cond, road):
    check_budget(cond, road, lambda lay: run_on_library(engine, lay, exact=False, dict_road=road == "g"))


# ---- GPU tier


@pytest.mark.gpu
@pytest.mark.parametrize("name,road", CASES, ids=IDS)
def test_on_gpu(name, road):
    from cerbos_amd import capi       # (CBH_TEST_SIM_ENGINE=1, the developer's aid of tests/conftest.py: the simulator)
    run_on_library(capi, layer(name, road))


@pytest.mark.gpu
@pytest.mark.parametrize("road", ROADS)
@pytest.mark.parametrize("cond", list(BUDGET_CONDS))
def test_step_budget_on_gpu(cond, road):
    from cerbos_amd import capi
    check_budget(cond, road, lambda lay: run_on_library(capi, lay, exact=False, dict_road=False))      # (the device road: the plan's text is asserted there)
