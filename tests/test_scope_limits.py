"""The scope dimension at its limits: chains of 8, 9, 15, 16 and 17 entries, tables of 255, 256, 257, 4095 and 4096 scopes.

What is pinned here (cbh_check_flat.h, cbh_check_walk2.h, cbh_vm.h and the host's launch code):
  the depth planes dp0 .. dp3     the chain position a walk was decided at, accumulated in the walk, read back by the fold and by the
                                  second climb for derived roles (`reach`): chains of more than eight entries use dp3
  the chain table's width         one byte per entry up to 256 scopes (chain_si8), four above; its size on the host
                                  (cbh_flat_chain_bytes, cbh_flat_trail_bytes, w2_layout)
  scope_bits, cbh_pk_bits         lanes merged by scope; packed results up to 4095 scopes (CBH_PK_MAX_BITS), the wide form from 4096
  CBH_FLAT_MAX_DEPTH              16 entries are flat and walk2, 17 go to the general walk

The reference is oracle/check.py (RuleTableOracle) everywhere, exactly and per tuple: effect, policy key, the scope string (the
result's scope index through lt.scopes); per request whether evaluation errors were recorded and effectiveDerivedRoles; for the trail
the effective policies per request.  Nothing may be flagged CBH_ST_UNSUPPORTED.  Every road asserts the kernel it ran (the plan's
text, or the emulator's hostsim_last_kind / hostsim_last_masks): a test that passes because something fell back proves nothing.

The stores.  chain_docs(N): kind `doc` has a policy at every entry of "", s0, s0.s1, ... (N entries), kind `rep` the same with
three entries missing (gaps are legal).  Level p names action a<p>: ALLOW for r0, DENY for r1 - a request at the deepest scope that
asks for a<p> is decided at chain position N - 1 - p.  The exceptions are deliberate: levels 2, 9 and N - 2 carry
REQUIRE_PARENTAL_CONSENT_FOR_ALLOWS and are confirmed two levels up (which moves the deciding position); levels with p % 3 == 1 have
a rule for r2 whose condition reads an attribute a quarter of the requests lack, and the level above a level with p % 3 == 0 has one
for that level's action (an error a role after the one that allowed must not report); derived roles are imported at chain positions
0, 8 and the last of the deepest scope, each behind a condition.  count_docs(n): a chain of four entries and n - 4 sibling scopes of
one literal rule each.  chain_docs(N, rng=...): random rules per level on the same chain (the fuzz layer).

Tiers: *_on_emulator is the kernels' source on the wave emulator (tests/hostsim_api.py), *_on_simulator the library's host side on
the simulator (tests/sim_engine.py; the forced variants in one child process each, the library reads its switches once), *_four_waves
the simulator with four waves to a workgroup (the per-wave quarters of the LDS), *_on_gpu the library on the device.

Mutation check (each mutant on a scratch copy, CPU tier only).  "older": tests/test_flat_kernel.py, test_walk2.py,
test_effective_policies.py, test_packed_results.py, test_compact_inputs.py, test_capacity_limits.py, test_cross_direct.py (373 tests).
   1  flat fold without the dp3 term            killed: test_chains_on_emulator[chain9 | chain15 | chain16 | plain16 - record_walk | staged_walk | mask_walk],
                                                test_list_valued_attribute_on_emulator, test_fuzz_on_emulator[9 | 15 | 16], test_sixteen_entries_inside_257_scopes_on_emulator
                                                [record_walk | mask_walk], test_as_planned_on_simulator[chain9 | chain16 | any16 | plain16, trail], test_forced_variant_on_simulator
                                                [staged_walk | mask_walk], test_four_waves_to_a_workgroup.  older: all pass
   2  walk2 fold without the dp3 term           killed: test_chains_on_emulator[* - walk2] from chain9 on, test_a_glob_action_takes_walk2_on_emulator, test_fuzz_on_emulator[* - 2],
                                                test_as_planned_on_simulator[glob16], test_forced_variant_on_simulator[walk2], ...inside_257_scopes_on_emulator[walk2].  older: all pass
   3  the walk accumulates no dp3               killed by the tests of 1 (the walk2 kernel's line: by the tests of 2).  older: all pass
   4  reach without `tp = cand & dp3`           killed: test_chains_on_emulator[chain9 | chain15 | chain16 - the three flat walks], test_fuzz_on_emulator, ...inside_257_scopes_on_emulator,
                                                test_as_planned_on_simulator[chain9 | chain16, trail], test_four_waves_to_a_workgroup (walk2's line: the walk2 tests of 2).  older: all pass
   5  flat chain8 <= 257                        killed: test_scope_counts_on_emulator[257 - the three flat walks], test_scope_counts_on_simulator[257], ...inside_257_scopes_on_emulator
                                                [record_walk | mask_walk], test_forced_variant_on_simulator[staged_walk | mask_walk], test_four_waves_to_a_workgroup.  older (without the
                                                disassembly audits, which decide nothing): all pass
   6  walk2 chain8 <= 257                       killed: test_scope_counts_on_emulator[257-walk2], ...inside_257_scopes_on_emulator[walk2], test_forced_variant_on_simulator[walk2].  older: all pass
   7  cbh_flat_chain_bytes 256 -> 257           killed, on the one-wave simulator already: its launches check every dynamic LDS access against the size asked for and abort
                                                ("wrote dynamic LDS at byte 1568, beyond the 1568") - test_scope_counts_on_simulator[257], test_forced_variant_on_simulator[staged_walk],
                                                test_four_waves_to_a_workgroup.  older: all pass
   8  cbh_flat_trail_bytes with half the depth  killed the same way: test_as_planned_on_simulator[check_trail-chain16], test_forced_variant_on_simulator[mask_walk],
                                                test_four_waves_to_a_workgroup.  older: test_packed_results.py::test_forms_switch_on_simulator fails too
   9  scope_bits from clz(n_scopes - 2)         the walk never ends on a table of 2^k + 1 scopes (the merged maximum lacks the top bit, no lane stands there):
                                                test_chains_on_emulator[chain9-*] and every other run of chain9, count257 and combo stop at a time limit only.  Killed by a hang,
                                                not by an assertion; chain16 and walk2 at 257 scopes pass
  10  packed word's shift 6 + cbh_pk_bits       killed: test_scope_counts_on_simulator[255 | 256 | 257 | 4095] (4096 keeps the wide form and passes), test_as_planned_on_simulator[chain9 |
                                                chain16 | any16 | plain16], test_forced_variant_on_simulator[staged_walk | mask_walk].  older: test_packed_results.py and
                                                test_compact_inputs.py fail too (12 tests)
  11  reach = d                                 killed: test_chains_on_emulator[chain8 | chain9 | chain15 | chain16 - the three flat walks], test_fuzz_on_emulator[8 | 9 | 15 | 16],
                                                test_as_planned_on_simulator[chain9 | chain16, trail] (walk2's line: test_chains_on_emulator[* - walk2] and the walk2 tests of 2).
                                                older: tests/test_flat_kernel.py fails too (53 tests)
The new file's CPU tier takes 85 s in one process (109 tests)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cerbos_amd.engine import HipEvaluator, effective_policy_keys
from cerbos_amd.flatten import Flattener
from cerbos_amd.lower.blob import lower_rule_table
from cerbos_amd.policy.loader import policies_from_docs
from cerbos_amd.ruletable.build import rule_table_from_policies
from oracle.check import EvalParams, RuleTableOracle

API = "api.cerbos.dev/v1"
NOW = 1_700_000_000_000_000_000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPACT = "[compact inputs"
ROLES = ["r0", "r1", "r2", "r3"]
ACTIONS = ["a%d" % i for i in range(16)]
CONSENT = "SCOPE_PERMISSIONS_REQUIRE_PARENTAL_CONSENT_FOR_ALLOWS"
FLAG_COND = {"match": {"expr": "R.attr.flag == true"}}
ROLE_SETS = [["r0"], ["r1"], ["r2"], ["r3"], ["r0", "r2"], ["r2", "r0"], ["r0", "r3"], ["r3", "r0"], ["r1", "r0"], ["r0", "r1"], ["r2", "r1"],
             ["r2", "r3", "r0"], ["r0", "r1", "r2", "r3"], ["r3", "r2"]]
EFFECT_ALLOW, ST_CEL_ERROR, ST_UNSUPPORTED = 1, 1, 2                                     # cerbos_amd/capi.py
F_LENIENT, F_WANT_DR, F_WANT_EP = 1, 4, 8                                                # ... asserted against capi in _flags()


def _flags(capi):
    assert (capi.F_LENIENT_SCOPE_SEARCH, capi.F_WANT_DERIVED_ROLES, capi.F_WANT_EFFECTIVE_POLICIES, capi.EFFECT_ALLOW, capi.ST_CEL_ERROR,
            capi.ST_UNSUPPORTED) == (F_LENIENT, F_WANT_DR, F_WANT_EP, EFFECT_ALLOW, ST_CEL_ERROR, ST_UNSUPPORTED)


# ---- the stores


def chain_scope(p):
    """the scope of p segments: entry p of the chain "", s0, s0.s1, ..."""
    return ".".join("s%d" % i for i in range(p))


def group(g):
    return ACTIONS[4 * g:4 * g + 4]


def _rule(actions, effect, roles=None, derived=None, cond=None):
    r = {"actions": list(actions), "effect": "EFFECT_" + effect}
    if roles:
        r["roles"] = list(roles)
    if derived:
        r["derivedRoles"] = list(derived)
    if cond:
        r["condition"] = cond
    return r


def _policy(kind, scope, rules, consent=False, imports=None):
    pol = {"resource": kind, "version": "default", "rules": rules}
    if scope:
        pol["scope"] = scope
        if consent:
            pol["scopePermissions"] = CONSENT
    if imports:
        pol["importDerivedRoles"] = list(imports)
    return {"apiVersion": API, "resourcePolicy": pol}


def dr_levels(n):
    """level -> the derived role its policy imports: chain positions 0, 8 and the last of a request at the deepest scope"""
    at = {n - 1: "deep", 0: "root"}
    if n >= 10:
        at[n - 9] = "mid"
    return at


def consent_levels(n):
    return {c for c in (2, 9, n - 2) if 2 <= c < min(n, 16)}


def _sibling_docs(count):
    """`count` scopes beside the chain, one literal rule each"""
    return [_policy("doc", "x%04d" % k, [_rule(["a%d" % (k % 4)], "ALLOW" if k % 3 else "DENY", roles=["r0"])]) for k in range(count)]


def chain_docs(n, derived=True, siblings=0, glob=False, rng=None, owner_rule=False):
    """see the module's text; rng: the levels' rules are random ones instead (the fuzz layer); owner_rule: level 5 orders a
    column against a number (a leaf that hands a list to the evaluator: BatchShape::plain_tags looks at the columns of such leaves only)"""
    docs = []
    drs = dr_levels(n) if derived else {}
    if derived:
        conds = {"deep": "R.attr.owner == P.id", "mid": "R.attr.owner == P.id", "root": "P.attr.lvl >= 2.0"}
        parents = {"deep": ["*"], "mid": ["r0", "r3"], "root": ["*"]}
        for name in sorted(set(drs.values())):
            docs.append({"apiVersion": API, "derivedRoles": {"name": "set_" + name, "definitions": [
                {"name": name, "parentRoles": parents[name], "condition": {"match": {"expr": conds[name]}}}]}})
    consent = consent_levels(n)
    for kind, missing in (("doc", ()), ("rep", (3, 6, n - 3))):
        for p in range(n):
            if p in missing:
                continue
            rules = []
            if rng is not None:
                for _ in range(int(rng.integers(1, 4))):
                    rules.append(_rule([str(a) for a in rng.choice(ACTIONS, size=int(rng.integers(1, 4)), replace=False)],
                                       "ALLOW" if rng.random() < 0.65 else "DENY",
                                       roles=[str(r) for r in rng.choice(ROLES + ["*"], size=int(rng.integers(1, 3)), replace=False)],
                                       cond=[None, None, FLAG_COND, {"match": {"expr": "R.attr.owner == P.id"}}][int(rng.integers(0, 4))]))
                if p in drs and rng.random() < 0.7:
                    rules.append(_rule([str(rng.choice(ACTIONS))], "ALLOW", derived=[drs[p]]))
                docs.append(_policy(kind, chain_scope(p), rules, consent=rng.random() < 0.3, imports=["set_" + drs[p]] if p in drs else None))
                continue
            if p < 16:
                a = "a%d" % p
                rules += [_rule([a], "ALLOW", roles=["r0"]), _rule([a], "DENY", roles=["r1"])]
                if p % 3 == 1:
                    rules.append(_rule([a], "ALLOW", roles=["r2"], cond=FLAG_COND))
                if p in drs:
                    rules.append(_rule([a], "ALLOW", derived=[drs[p]]))
            else:
                rules += [_rule(["a15"], "ALLOW", roles=["r3"]), _rule(["a14"], "DENY", roles=["r3"])]
            if (p + 1) % 3 == 0 and p + 1 < min(n, 16):
                rules.append(_rule(["a%d" % (p + 1)], "DENY", roles=["r2"], cond=FLAG_COND))       # the level ABOVE the one that names the action
            if p + 2 in consent:
                rules.append(_rule(["a%d" % (p + 2)], "ALLOW", roles=["r0", "r3"]))                # the consent of level p + 2
            if glob and p == 0:
                rules.append(_rule(["g:*"], "ALLOW", roles=["r3"]))
            if owner_rule and p == 5:
                rules.append(_rule(["a5"], "ALLOW", roles=["r3"], cond={"match": {"expr": "R.attr.rank >= 2.0"}}))
            docs.append(_policy(kind, chain_scope(p), rules, consent=p in consent, imports=["set_" + drs[p]] if p in drs else None))
    return docs + _sibling_docs(siblings)


def _req(i, scope, roles, acts, kind="doc", flag=True, owner="p0", pid="p0", lvl=3.0):
    rattr = {"owner": owner, "rank": lvl}
    if flag is not None:
        rattr["flag"] = flag
    return {"requestId": "q%d" % i, "actions": list(acts), "principal": {"id": pid, "roles": list(roles), "attr": {"lvl": lvl}},
            "resource": {"kind": kind, "id": "d%d" % i, "attr": rattr, "scope": scope}}


def chain_requests(n, count=301, seed=0, list_attr=False, targets=()):
    """-> (requests, notes).  The first wave is interleaved (lane i stands at level i % (n + 5): the merged climb); then the deepest
    two levels with every action group under r0 and r1 (every chain position decides an ALLOW and a DENY); the reach cases (notes
    ["reach"]: [r0, r3] against [r3, r0] on the deepest level's own action - the first role allows at chain position 0, the later one
    would climb the whole chain); the error cases (notes["errors"]: (suppressed, reported) - [r0, r2] against [r2, r0] without the
    attribute); requests at the scopes of `targets`; random ones.  Levels go five entries below the deepest scope of the table."""
    rng = np.random.default_rng(5_000 + 97 * n + seed)
    reqs, notes = [], {"reach": [], "errors": []}
    flags = (True, False, None, True)

    def add(level, roles, acts, **kw):
        reqs.append(_req(len(reqs), level if isinstance(level, str) else chain_scope(level), roles, acts, **kw))
        return len(reqs) - 1

    for i in range(64):
        add(i % (n + 5), ROLE_SETS[i % len(ROLE_SETS)], group((i // 7) % 4), flag=flags[i % 4], owner="p%d" % (i % 2), lvl=float(1 + i % 3))
    for level in (n - 1, n - 2):
        for g in range(4):
            for r in ("r0", "r1"):
                add(level, [r], group(g))
    deep_act = ["a%d" % min(n - 1, 15)]
    first, later = ("r0", "r3") if n <= 16 else ("r3", "r2")       # (level 16 names a15 for r3; r2 without the flag climbs to the root)
    for owner in ("p0", "p1"):
        for lvl in (3.0, 1.0):
            notes["reach"].append((add(n - 1, [first, later], deep_act, owner=owner, lvl=lvl, flag=False),
                                   add(n - 1, [later, first], deep_act, owner=owner, lvl=lvl, flag=False)))
    for g in range(4):
        notes["errors"].append((add(n - 1, ["r0", "r2"], group(g), flag=None), add(n - 1, ["r2", "r0"], group(g), flag=None)))
    for k, scope in enumerate(targets):
        add(scope, ROLE_SETS[k % 2], group(0))
    while len(reqs) < count:
        level = n - 1 if rng.random() < 0.35 else int(rng.integers(0, n + 5))
        acts = group(int(rng.integers(0, 4)))
        if rng.random() < 0.15:
            acts = acts[:int(rng.integers(0, 4))]
        add(level, ROLE_SETS[int(rng.integers(0, len(ROLE_SETS)))], acts, kind="rep" if rng.random() < 0.2 else "doc",
            flag=flags[int(rng.integers(0, 4))], owner="p%d" % rng.integers(0, 2), lvl=float(rng.integers(1, 4)))
    if list_attr:
        reqs[70]["resource"]["attr"]["rank"] = [1.0, 2.0]  # one list-valued attribute in the batch: the variant with the evaluator call
    assert len(reqs) == count and count % 64
    return reqs, notes


def count_docs(n_scopes):
    return chain_docs(4, derived=False, siblings=n_scopes - 4)


class Case:
    """a store, its lowering, ~300 requests flattened in their own order (lane = index), and the oracle's answers under both scope
    searches - computed once, shared by every road, never changed"""

    def __init__(self, name, docs, n, make_requests, flat=True):
        self.name, self.n = name, n
        self.rt = rule_table_from_policies(policies_from_docs(docs))
        self.lt = lower_rule_table(self.rt)
        assert bool(self.lt.stats["flat"]) == flat, (name, self.lt.stats)
        self.inputs, self.notes = make_requests(self.lt)
        self.batch = Flattener(self.lt).flatten(self.inputs, sort=False)
        assert self.batch.n_requests == len(self.inputs) and self.batch.tuple_perm is None
        assert int(self.batch.req_u32[9].max()) <= 4 and int(self.batch.req_u32[7].max()) <= 4   # the flat kernels' batch shape
        orc = RuleTableOracle(self.rt)
        self.want = {len_: [orc.check(i, EvalParams(now_ns=NOW, lenient_scope_search=len_)) for i in self.inputs] for len_ in (False, True)}
        self.asm = _Assembler(self.lt)

    @property
    def n_scopes(self):
        return len(self.lt.scopes)

    def decided_at(self):
        """{scope index: tuples the oracle decides at that scope by a policy of the table}"""
        ix = {s: i for i, s in enumerate(self.lt.scopes)}
        out = {}
        for want in self.want.values():
            for w in want:
                for e in w["actions"].values():
                    if e["policy"].startswith("resource."):
                        out[ix[e["scope"]]] = out.get(ix[e["scope"]], 0) + 1
        return out


class _Assembler:
    """HipEvaluator.assemble without an engine: the ids of a Result -> CheckOutputs"""
    assemble = HipEvaluator.assemble
    _policy_string = HipEvaluator._policy_string

    def __init__(self, lt):
        self.lt = lt


def compare(case, res, lenient, what):
    """`res` in input order against the oracle: per tuple effect, policy key and scope string; per request the evaluation errors and
    effectiveDerivedRoles; nothing flagged for the CPU path"""
    assert not (res.status == ST_UNSUPPORTED).any(), (case.name, what, "UNSUPPORTED tuples", int((res.status == ST_UNSUPPORTED).sum()))
    outs, bad = case.asm.assemble(case.inputs, case.batch, res, "default", allow_unsupported=True)
    assert not bad
    t = 0
    for i, (inp, have, want) in enumerate(zip(case.inputs, outs, case.want[lenient])):
        for a in inp["actions"]:
            h, w = have["actions"][a], want["actions"][a]
            assert (h["effect"], h["policy"], h["scope"]) == (w["effect"], w["policy"], w["scope"]), (case.name, what, lenient, "lane %d" % (i % 64), inp, a, h, w)
        assert sorted(have["effectiveDerivedRoles"]) == sorted(want["effectiveDerivedRoles"]), (case.name, what, lenient, inp, have["effectiveDerivedRoles"], want["effectiveDerivedRoles"])
        na = len(inp["actions"])
        assert bool((res.status[t:t + na] == ST_CEL_ERROR).any()) == (bool(want["evaluationErrors"]) and na > 0), (case.name, what, lenient, inp, want["evaluationErrors"])
        t += na
    assert t == res.effect.size


def compare_trail(case, masks, lenient, what):
    """one group per request: the effective policies, as tests/test_effective_policies.py compares them"""
    have = [effective_policy_keys(case.lt.policy_keys, row) for row in masks]
    want = [w["effectivePolicies"] for w in case.want[lenient]]
    bad = [k for k in range(len(want)) if have[k] != want[k]]
    assert not bad, (case.name, what, lenient, bad[:3], have[bad[0]], want[bad[0]], case.inputs[bad[0]])
    assert len({tuple(k) for k in have}) > 3


_CASES = {}


def case(name):
    """chain<N>: the directed store with derived roles; plain<N>: without (the compact, packed and cross forms have no derived-role
    variant); any16: plain16 with an ordering leaf and one list-valued attribute in the batch (the derived-role variant
    decides such batches itself); glob16: chain16 with a glob action (walk2 by itself); count<n>: n scopes;
    combo: the 16-entry chain inside 257 scopes; fuzz<N>_<seed>"""
    if name not in _CASES:
        if name.startswith("fuzz"):
            n, seed = (int(x) for x in name[4:].split("_"))
            docs = chain_docs(n, rng=np.random.default_rng(8_000 + 31 * n + seed))
            c = Case(name, docs, n, lambda lt: chain_requests(n, seed=seed + 1), flat=n <= 16)
        elif name.startswith("count"):
            c = Case(name, count_docs(int(name[5:])), 4, lambda lt: chain_requests(4, targets=_targets(lt)))
            assert c.n_scopes == int(name[5:]), c.n_scopes
        elif name == "combo":
            c = Case(name, chain_docs(16, siblings=257 - 16), 16, lambda lt: chain_requests(16, targets=_targets(lt)))
            assert c.n_scopes == 257 and c.lt.stats["derived_roles"]
        else:
            kind, n = name.rstrip("0123456789"), int(name[len(name.rstrip("0123456789")):])
            docs = chain_docs(n, derived=kind not in ("plain", "any"), glob=kind == "glob", owner_rule=kind == "any")
            c = Case(name, docs, n, lambda lt: chain_requests(n, list_attr=kind == "any"), flat=n <= 16 and kind != "glob")
            assert c.n_scopes == n and bool(c.lt.stats["derived_roles"]) == (kind not in ("plain", "any")), c.lt.stats
            if kind == "glob":
                assert c.lt.stats["walk2"] and not c.lt.stats["flat"]
            if n == 17:
                assert not c.lt.stats["walk2"], "17 entries: the general walk"
        _CASES[name] = c
    return _CASES[name]


def _targets(lt):
    """requests concentrate on the highest scope indices and on 254 .. 257: three requests at each"""
    n = len(lt.scopes)
    ix = sorted({i for i in (254, 255, 256, 257, n - 4, n - 3, n - 2, n - 1) if 0 <= i < n})
    return [lt.scopes[i] for i in ix for _ in range(4)] + [lt.scopes[i] for i in range(n - 40, n - 4)]


def check_chain_conditions(c):
    """what the directed store must make happen (read off the oracle's answers, which every road is compared with)"""
    n = c.n
    seen = set()
    res_scopes = set(c.rt["resource_scopes"])
    for want in c.want.values():
        for inp, w in zip(c.inputs, want):
            s = inp["resource"]["scope"]
            chain = [x for x in [s] + [s.rsplit(".", k)[0] for k in range(1, s.count(".") + 1)] + ([""] if s else []) if x in res_scopes]
            if inp["resource"]["kind"] != "doc" or s not in res_scopes:
                continue
            for e in w["actions"].values():
                if e["policy"].startswith("resource.") and e["scope"] in chain and e["policy"] != "":
                    seen.add((chain.index(e["scope"]), e["effect"]))
    if n <= 16:
        for pos in range(n):
            assert (pos, "EFFECT_ALLOW") in seen and (pos, "EFFECT_DENY") in seen, (c.name, "no tuple decided at chain position", pos, sorted(seen))
    want = c.want[False]
    assert any(w["evaluationErrors"] for w in want)
    assert any(not want[a]["evaluationErrors"] and want[b]["evaluationErrors"] for a, b in c.notes["errors"]), "no error suppressed by the role-after-allow rule"
    if c.lt.stats["derived_roles"]:
        assert any(want[a]["effectiveDerivedRoles"] != want[b]["effectiveDerivedRoles"] for a, b in c.notes["reach"]), "requests that differ in reach alone have the same derived roles"
        assert len({tuple(w["effectiveDerivedRoles"]) for w in want}) >= 2


def check_count_conditions(c):
    at = c.decided_at()
    assert at.get(c.n_scopes - 1), (c.name, "no tuple decided at the highest scope index")
    if c.n_scopes >= 257:
        assert any(i >= 256 for i in at), (c.name, "no tuple decided at a scope index of 256 or more")
    assert any(w["evaluationErrors"] for w in c.want[False])


def packs(n_scopes):
    """cbh_vm.h cbh_pk_bits(n_scopes) <= CBH_PK_MAX_BITS: what tests/test_packed_results.py check_scopes_too_wide reads off lt.stats"""
    return (n_scopes | 1).bit_length() <= 12


# ---- the roads.  The emulator: the kernels' source; asserts hostsim_last_kind / hostsim_last_masks


EMULATOR = {   # road -> (environment, hostsim_last_kind, hostsim_last_masks or None)
    "record_walk": ({"CBH_FLAT_MASKS": "0"}, 1, 0),
    "staged_walk": ({"CBH_FORCE_STAGED": "1", "CBH_FLAT_MASKS": "0"}, 1, 0),
    "mask_walk": ({"CBH_FLAT_MASKS": "1"}, 1, 1),
    "walk2": ({"CBH_NO_FLAT": "1"}, 2, None),
    "general_walk": ({"CBH_NO_FLAT": "1", "CBH_NO_WALK2": "1"}, 0, None),
}


def check_on_emulator(name, road, monkeypatch, trail=False, kind=None):
    import hostsim_api
    env, want_kind, masks = EMULATOR[road]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = case(name)
    for lenient in (False, True):
        flags = F_WANT_DR | (F_LENIENT if lenient else 0)
        res = hostsim_api.check(c.lt, c.batch, NOW, flags)
        assert hostsim_api.last_kind() == (want_kind if kind is None else kind), (name, road, hostsim_api.last_kind())
        if masks is not None and kind is None:
            assert hostsim_api.lib().hostsim_last_masks() == masks, (name, road)
        compare(c, res, lenient, road)
        if trail:
            groups = np.arange(c.batch.n_requests, dtype=np.uint32)
            res, m = hostsim_api.check_trail(c.lt, c.batch, groups, c.batch.n_requests, NOW, flags)
            assert hostsim_api.last_kind() == (want_kind if kind is None else kind), (name, road, "trail")
            compare(c, res, lenient, road + ", trail")
            compare_trail(c, m, lenient, road + ", trail")


# ---- the library: cbh_check_batch, the resident path, the trail, the direct cross form; asserts the plan


def _flat(plan, *suffixes, no=()):
    name = plan.split("[")[0]
    return name.startswith("cbh_check_flat_kernel") and all(s in name for s in suffixes) and not any(s in name for s in no)


def check_decisions(capi, name, plan_ok, compact=None):
    """one-shot and resident (upload / launch / download: packed results where the scope count allows, compact inputs where the
    kernel has the instantiation), each against the oracle under both scope searches"""
    _flags(capi)
    c = case(name)
    table = capi.Table(c.lt.blob)
    db = table.upload(c.batch)
    try:
        for lenient in (False, True):
            flags = F_WANT_DR | (F_LENIENT if lenient else 0)
            compare(c, table.check(c.batch, now_ns=NOW, flags=flags), lenient, "cbh_check_batch")
            table.launch(db, now_ns=NOW, flags=flags)
            compare(c, table.download(db), lenient, "resident")
        table.launch(db, now_ns=NOW, flags=0)                       # without the derived roles: no second climb
        have = table.download(db)
        assert np.array_equal(have.effect, table.check(c.batch, now_ns=NOW, flags=0).effect)
        plan = table.plan(db, flags=F_WANT_DR)
        assert plan_ok(plan), (name, plan)
        if compact is not None:
            assert (COMPACT in plan) == compact, (name, plan)
    finally:
        db.close()
        table.close()


def check_trail(capi, name, plan_ok):
    """cbh_check_batch_trail and the resident trail, one group per request"""
    _flags(capi)
    c = case(name)
    table = capi.Table(c.lt.blob)
    db = table.upload(c.batch)
    groups = np.arange(c.batch.n_requests, dtype=np.uint32)
    try:
        plan = table.plan(db, flags=F_WANT_DR | F_WANT_EP)
        assert plan_ok(plan), (name, plan)
        for lenient in (False, True):
            flags = F_WANT_DR | (F_LENIENT if lenient else 0)
            res, masks = table.check_trail(c.batch, groups, c.batch.n_requests, now_ns=NOW, flags=flags)
            compare(c, res, lenient, "cbh_check_batch_trail")
            compare_trail(c, masks, lenient, "cbh_check_batch_trail")
            table.set_trail(db, groups, c.batch.n_requests)
            table.launch(db, now_ns=NOW, flags=flags | F_WANT_EP)
            compare_trail(c, table.trail(db), lenient, "resident trail")
            compare(c, table.download(db), lenient, "resident trail")
    finally:
        db.close()
        table.close()


def check_cross(capi, name, kernel):
    """the direct cross form: 23 principals x 19 resources at every level of the chain, four actions whose levels span it; the allow
    bits per pair and action and the pair's `flagged` (any action) rebuilt from the oracle"""
    from cerbos_amd.cross import allow_cube_planes, cross_direct_upload
    _flags(capi)
    c = case(name)
    n = c.n
    acts = ["a0", "a%d" % (n // 3), "a%d" % (2 * n // 3 + 1), "a%d" % (n - 1)]
    ps = [{"id": "p%d" % (i % 2), "roles": ROLE_SETS[i % len(ROLE_SETS)], "attr": {"lvl": float(1 + i % 3)}} for i in range(23)]
    rs = []
    for j in range(19):
        attr = {"owner": "p%d" % (j % 2)}
        if j % 4:
            attr["flag"] = j % 3 == 0
        rs.append({"kind": "rep" if j % 6 == 5 else "doc", "id": "d%d" % j, "attr": attr, "scope": chain_scope(n - 1 if j % 3 == 0 else (j * 5) % (n + 3))})
    orc = RuleTableOracle(c.rt)
    table = capi.Table(c.lt.blob)
    cs = cross_direct_upload(table, Flattener(c.lt), c.lt.columns, ps, rs, acts)
    try:
        assert cs is not None, "the set has no direct form: " + capi.load().cbh_last_error().decode("utf-8", "replace")
        for lenient in (False, True):
            flags = F_LENIENT if lenient else 0
            desc = cs.describe(flags)
            assert desc.split("[")[0] == kernel and "_x[direct cross" in desc, desc
            allow, flagged = cs.check(0, len(rs), flags=flags, now_ns=NOW, want_flagged=True)
            have_a, have_f = allow_cube_planes(cs, 0, len(rs), allow), allow_cube_planes(cs, 0, len(rs), flagged)
            n_allow = n_err = 0
            for i, p in enumerate(ps):
                for j, r in enumerate(rs):
                    w = orc.check({"principal": p, "resource": r, "actions": acts}, EvalParams(now_ns=NOW, lenient_scope_search=lenient))
                    want_a = [w["actions"][a]["effect"] == "EFFECT_ALLOW" for a in acts]
                    assert list(have_a[i, j]) == want_a, (name, lenient, p, r, list(have_a[i, j]), want_a)
                    assert bool(have_f[i, j].any()) == bool(w["evaluationErrors"]), (name, lenient, p, r, w["evaluationErrors"])
                    n_allow += sum(want_a)
                    n_err += bool(w["evaluationErrors"])
            assert n_allow > 50 and n_err > 5, (n_allow, n_err)
    finally:
        if cs is not None:
            cs.close()
        table.close()


def check_counts(capi, name):
    """a table of `n` scopes on the flat kernel's compact instantiation; 4095 scopes still pack their results, 4096 do not"""
    c = case(name)
    check_count_conditions(c)
    assert packs(c.n_scopes) == (c.n_scopes <= 4095)
    check_decisions(capi, name, lambda p: _flat(p, no=("_any", "_dr")), compact=True)


LIBRARY = {   # road -> (environment, [(body, arguments)])
    "default": ({}, [
        (check_decisions, ("chain9", lambda p: _flat(p, "_dr"), False)),
        (check_decisions, ("chain16", lambda p: _flat(p, "_dr"), False)),
        (check_decisions, ("any16", lambda p: _flat(p, "_any"), False)),
        (check_decisions, ("plain16", lambda p: _flat(p, no=("_any", "_dr", "_staged", "_masks")), True)),
        (check_decisions, ("glob16", lambda p: p.endswith("cbh_walk2_kernel"), None)),
        (check_decisions, ("chain17", lambda p: p.startswith("cbh_check_kernel*"), None)),
        (check_trail, ("chain16", lambda p: p == "cbh_check_flat_trail_kernel*")),
        (check_trail, ("glob16", lambda p: p.endswith("cbh_walk2_trail_kernel"))),
        (check_cross, ("plain16", "cbh_check_flat_kernel_x")),
        (check_cross, ("plain9", "cbh_check_flat_kernel_x")),
    ]),
    "staged_walk": ({"CBH_FORCE_STAGED": "1"}, [
        (check_decisions, ("plain16", lambda p: _flat(p, "_staged", no=("_any",)), True)),
        (check_decisions, ("count257", lambda p: _flat(p, "_staged", no=("_any",)), True)),
        (check_cross, ("plain16", "cbh_check_flat_kernel_staged_x")),
    ]),
    "mask_walk": ({"CBH_FLAT_MASKS": "1"}, [
        (check_decisions, ("plain16", lambda p: _flat(p, "_masks", no=("_any",)), True)),
        (check_decisions, ("count257", lambda p: _flat(p, "_masks", no=("_any",)), True)),
        (check_trail, ("chain16", lambda p: p == "cbh_check_flat_trail_kernel*_masks")),
        (check_trail, ("combo", lambda p: p == "cbh_check_flat_trail_kernel*_masks")),
        (check_cross, ("plain16", "cbh_check_flat_kernel_masks_x")),
    ]),
    "walk2": ({"CBH_NO_FLAT": "1"}, [
        (check_decisions, ("chain16", lambda p: p.endswith("cbh_walk2_kernel"), None)),
        (check_decisions, ("combo", lambda p: p.endswith("cbh_walk2_kernel"), None)),
        (check_trail, ("chain16", lambda p: p.endswith("cbh_walk2_trail_kernel"))),
    ]),
    "general_walk": ({"CBH_NO_FLAT": "1", "CBH_NO_WALK2": "1"}, [
        (check_decisions, ("chain16", lambda p: p.startswith("cbh_check_kernel*"), None)),
    ]),
    "four_waves": ({}, [
        (check_decisions, ("combo", lambda p: _flat(p, "_dr"), False)),
        (check_decisions, ("count257", lambda p: _flat(p, no=("_any", "_dr")), True)),
        (check_trail, ("combo", lambda p: p == "cbh_check_flat_trail_kernel*")),
    ]),
    "four_waves_mask_walk": ({"CBH_FLAT_MASKS": "1"}, [
        (check_trail, ("combo", lambda p: p == "cbh_check_flat_trail_kernel*_masks")),
        (check_decisions, ("count257", lambda p: _flat(p, "_masks", no=("_any",)), True)),
    ]),
}


def run_road(capi, road, only=None):
    for k, (body, args) in enumerate(LIBRARY[road][1]):
        if only is None or k in only:
            body(capi, *args)


CHILD = """
import sys
sys.path.insert(0, %(tests)r)
import %(module)s as ts
if %(sim)r:
    from sim_engine import sim_engine
    with sim_engine() as capi:
        ts.run_road(capi, %(road)r)
else:
    from cerbos_amd import capi
    ts.run_road(capi, %(road)r)
print("%(module)s: ok")
"""
_ABNORMAL = []   # the first child that a signal or its time limit ended: no child is started after it


def check_in_child(sim, road, lib=None, limit=600, module="test_scope_limits", library=None):
    """One fresh process per forced variant (the library reads its switches once), one after another, each under its own time
    limit.  After a child that ended abnormally none is started.  `module`, `library`: another test file's road table (its
    run_road(capi, road) is what the child calls)."""
    assert not _ABNORMAL, "not started: an earlier child ended abnormally (%s)" % _ABNORMAL[0]
    env = dict(os.environ, **(LIBRARY if library is None else library)[road][0])
    if lib:
        env["CBH_TEST_SIM_LIB"] = lib
    try:
        r = subprocess.run([sys.executable, "-c", CHILD % {"tests": os.path.join(ROOT, "tests"), "sim": sim, "road": road, "module": module}],
                           env=env, cwd=ROOT, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        _ABNORMAL.append(road + ": time limit")
        raise
    if r.returncode < 0 or r.returncode in (134, 137, 139):
        _ABNORMAL.append("%s: exit status %d" % (road, r.returncode))
    assert r.returncode >= 0, "the child was ended by signal %d\n%s" % (-r.returncode, r.stderr[-4000:])
    assert r.returncode == 0 and module + ": ok" in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]


# ---- CPU tier: the conditions the generators must meet


@pytest.mark.parametrize("name", ["chain8", "chain9", "chain15", "chain16", "chain17", "plain9", "plain16", "any16", "glob16", "combo"])
def test_the_directed_store_reaches_every_chain_position(name):
    check_chain_conditions(case(name))


@pytest.mark.parametrize("n", [255, 256, 257, 4095, 4096])
def test_the_scope_count_store_decides_at_the_highest_indices(n):
    check_count_conditions(case("count%d" % n))
    assert packs(n) == (n <= 4095)


def test_the_combined_store_decides_at_index_256():
    c = case("combo")
    assert max(c.decided_at()) == 256 and c.lt.stats["flat"]


# ---- CPU tier: the wave emulator


@pytest.mark.parametrize("road", ["record_walk", "staged_walk", "mask_walk", "walk2", "general_walk"])
@pytest.mark.parametrize("name", ["chain8", "chain9", "chain15", "chain16", "plain16"])
def test_chains_on_emulator(name, road, monkeypatch):
    check_on_emulator(name, road, monkeypatch, trail=name in ("chain9", "chain16"))


@pytest.mark.parametrize("road", ["record_walk", "mask_walk"])
def test_list_valued_attribute_on_emulator(road, monkeypatch):
    check_on_emulator("any16", road, monkeypatch)


def test_seventeen_entries_take_the_general_walk_on_emulator(monkeypatch):
    check_on_emulator("chain17", "record_walk", monkeypatch, trail=True, kind=0)


def test_a_glob_action_takes_walk2_on_emulator(monkeypatch):
    check_on_emulator("glob16", "record_walk", monkeypatch, trail=True, kind=2)


@pytest.mark.parametrize("road", ["record_walk", "staged_walk", "mask_walk", "walk2"])
@pytest.mark.parametrize("n", [255, 256, 257, 4095, 4096])
def test_scope_counts_on_emulator(n, road, monkeypatch):
    check_on_emulator("count%d" % n, road, monkeypatch)


@pytest.mark.parametrize("road", ["record_walk", "mask_walk", "walk2"])
def test_sixteen_entries_inside_257_scopes_on_emulator(road, monkeypatch):
    check_on_emulator("combo", road, monkeypatch, trail=True)


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("n", [8, 9, 15, 16, 17])
def test_fuzz_on_emulator(n, seed, monkeypatch):
    roads = ["record_walk", "mask_walk", "walk2"] if n <= 16 else ["general_walk"]
    check_on_emulator("fuzz%d_%d" % (n, seed), roads[seed % len(roads)], monkeypatch, trail=seed == 0)


# ---- CPU tier: the library's host side on the simulator


@pytest.fixture()
def engine():
    from sim_engine import sim_engine
    with sim_engine() as capi:
        yield capi


@pytest.mark.parametrize("k", range(len(LIBRARY["default"][1])), ids=["%s-%s" % (b.__name__, a[0]) for b, a in LIBRARY["default"][1]])
def test_as_planned_on_simulator(engine, k):
    run_road(engine, "default", only=(k,))


@pytest.mark.parametrize("n", [255, 256, 257, 4095, 4096])
def test_scope_counts_on_simulator(engine, n):
    check_counts(engine, "count%d" % n)


@pytest.mark.parametrize("road", ["staged_walk", "mask_walk", "walk2", "general_walk"])
def test_forced_variant_on_simulator(road):
    check_in_child(True, road)


@pytest.mark.parametrize("road", ["four_waves", "four_waves_mask_walk"])
def test_four_waves_to_a_workgroup(road):
    from sim_engine import build_four_waves
    check_in_child(True, road, lib=build_four_waves())


# ---- GPU tier


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(LIBRARY["default"][1])), ids=["%s-%s" % (b.__name__, a[0]) for b, a in LIBRARY["default"][1]])
def test_as_planned_on_gpu(k):
    from cerbos_amd import capi
    run_road(capi, "default", only=(k,))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [255, 256, 257, 4095, 4096])
def test_scope_counts_on_gpu(n):
    from cerbos_amd import capi
    check_counts(capi, "count%d" % n)


@pytest.mark.gpu
def test_sixteen_entries_inside_257_scopes_on_gpu():
    from cerbos_amd import capi
    run_road(capi, "four_waves")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 9, 15, 16, 17])
def test_fuzz_on_gpu(n):
    from cerbos_amd import capi
    for seed in range(4):
        check_decisions(capi, "fuzz%d_%d" % (n, seed), lambda p: (p.startswith("cbh_check_flat_kernel") and n <= 16) or (p.startswith("cbh_check_kernel*") and n == 17))


@pytest.mark.gpu
@pytest.mark.parametrize("road", ["staged_walk", "mask_walk", "walk2", "general_walk"])
def test_forced_variant_on_gpu(road):
    check_in_child(os.environ.get("CBH_TEST_SIM_ENGINE") == "1", road, limit=300)   # (the developer's aid of tests/conftest.py: the simulator)
