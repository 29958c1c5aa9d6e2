"""The flat kernels' action groups (cerbos_hip.h CBH_HAS_FLAT_ACTION_GROUPS): on a flat table a batch whose requests have at most four
roles and 5 .. 64 actions is decided by the four-action kernel once per four actions (cbh_check_walk2.h cbh_plan `action_groups`,
cbh_host_resident.h launch_plan, cbh_check_flat.h flat_body AGROUP) instead of by the walk's kernels and the general walk.

The contract: `effect`, `status`, `policy`, `scope` per tuple and `edr` per request are bit for bit what the same library returns
with CBH_FLAT_ACTION_GROUPS=0.  Three references, none of which runs the new code:
  * the switched-off library in a child process (the switch is read once per process): every case below, once per tier - the
    child writes every case's arrays to one file, the tests of the tier share it;
  * the kernel emulator (hostsim_api.check: cbh_plan without groups, the walk's kernels and the general walk, in this process) on
    the CPU tier;
  * oracle/check.py for the directed store: every tuple's effect, policy and scope, every request's evaluation-error flag.
The one-shot road is run twice: small batches (one packed block) and batches of more than 1 MB of inputs by cbh_check_batch's three
ways - two chunks on two streams, one slab, pageable arrays - where the library's CBH_TRACE lines show the way taken and the
group launches per request range.
Every case asserts what cbh_plan_describe names, so that a fallback to the old road cannot pass.

The plan takes action groups from three groups on for a table without derived roles and from five on for one with
(cbh_check_walk2.h CBH_FLAT_MIN_GROUPS / _DR): below, the launches were not measured faster than the walk's kernels
(profiles/flat_action_groups_ab.txt - C2 at 2 groups 56.0 - 58.4 G decisions/s against 55.5 - 58.6 G, C3 at 2 - 4 groups 18.3 - 22.9 G
against 23.7 - 30.6 G), and such a shape stays on the road it had.  So the plan test's batch has one request of NINE actions on C2
(3 groups: the first count the plan takes) and pins that five actions on C2, and up to sixteen on C3, keep the plan without groups.
CPU tier: the library's host side and the kernels' source on the simulator (tests/sim_engine.py).  GPU tier: the same bodies on the device."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from cerbos_amd import wire, workloads
from cerbos_amd.cross import upload_halves
from cerbos_amd.flatten import Flattener
from sim_engine import sim_engine
from test_cross_device import NOW, _halves_of, _lower
from test_cross_direct import _halves

API = "api.cerbos.dev/v1"
FIELDS = ("effect", "status", "policy", "scope", "edr")
COUNTS = (1, 4, 5, 7, 8, 9, 12, 13, 16, 17, 63, 64)
SIZES = (1, 63, 64, 65, 257)
ALLOW, DENY = 1, 2   # cerbos_hip.h CBH_EFFECT_*
T_INT, T_DOUBLE = 2, 4   # cerbos_hip.h cbh_tag


def _groups(desc):
    """G of ", G action groups" in a describe string (1 = not named)"""
    return int(desc.split(" action groups")[0].rsplit(", ", 1)[1]) if " action groups" in desc else 1


def _is_sim(capi):
    return "sim" in os.path.basename(capi.LIB_PATH)


# ---- the directed store: a chain of three scopes, no derived roles

LEAF, MID, ROOT = ["l%d" % i for i in range(4)], ["m%d" % i for i in range(4)], ["r%d" % i for i in range(4)]
DIRECTED_DOCS = [
    {"apiVersion": API, "resourcePolicy": {"resource": "doc", "version": "default", "rules": [
        {"actions": ROOT + ["view"], "roles": ["user"], "effect": "EFFECT_ALLOW"},
        {"actions": ["last_allow"], "roles": ["user"], "effect": "EFFECT_ALLOW"},
        {"actions": ["last_deny"], "roles": ["user", "manager"], "effect": "EFFECT_DENY"},
        {"actions": ["tagged"], "roles": ["user"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": 'R.attr.tag == "x"'}}},
        {"actions": ["pub"], "roles": ["manager"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": "R.attr.public == true"}}},
        {"actions": ["big"], "roles": ["manager", "user"], "effect": "EFFECT_DENY", "condition": {"match": {"expr": "R.attr.amount > 100.5"}}}]}},
    {"apiVersion": API, "resourcePolicy": {"resource": "doc", "version": "default", "scope": "acme", "rules": [
        {"actions": MID, "roles": ["user"], "effect": "EFFECT_ALLOW"},
        {"actions": ["r1"], "roles": ["user"], "effect": "EFFECT_DENY"}]}},
    {"apiVersion": API, "resourcePolicy": {"resource": "doc", "version": "default", "scope": "acme.hr", "rules": [
        {"actions": LEAF, "roles": ["user"], "effect": "EFFECT_ALLOW"},
        {"actions": ["big"], "roles": ["manager"], "effect": "EFFECT_ALLOW"}]}},
]
NAMED = ["view", "tagged", "pub", "big"] + LEAF + MID + ROOT
FILL = ["f%d" % i for i in range(64)]          # names no rule has
CHAIN = LEAF + MID + ROOT                      # the request of twelve actions whose three groups are decided at three scopes


def _directed_inputs(n):
    """n CheckInputs.  Request i has COUNTS[i % 12] actions - so ACT_OFF + 4 g is a multiple of four for some requests and not for
    others (the counts 1, 5, 7 shift what follows), and the counts 5, 9, 13, 17 leave a last group of one.  A request of more than
    four actions carries `last_allow` and `last_deny` in its last group only; the request of twelve actions is CHAIN at scope
    acme.hr.  n = 257: four-action requests and ONE request of 64 actions in the middle - most waves have no lane in a group >= 1."""
    rng = np.random.default_rng(1000 + n)
    out = []
    for i in range(n):
        cnt = COUNTS[i % len(COUNTS)] if n != 257 else (64 if i == 130 else 4)
        if n == 1:
            cnt = 17       # (five groups, a last group of one)
        if cnt == 12:
            acts, scope = list(CHAIN), "acme.hr"
        else:
            pool = [str(a) for a in rng.permutation(NAMED)] + FILL
            acts = pool[:cnt]
            if cnt > 4:
                last = 4 * ((cnt - 1) // 4)        # the last group's first action
                acts[last] = "last_allow"
                if cnt - last > 1:
                    acts[cnt - 1] = "last_deny"
                elif i % 2:
                    acts[last] = "last_deny"
            scope = str(rng.choice(["", "acme", "acme.hr", "acme.hr.uk", "zzz"]))
        attr = {"amount": 40.5 * (i % 7), "public": bool(i % 3 == 0)}
        if i % 4:
            attr["tag"] = "x" if i % 8 < 4 else "y"
        roles = [["user"], ["manager"], ["user", "manager"], ["stranger", "user", "guest", "manager"], []][i % 5 if cnt != 12 else 0]
        out.append({"requestId": "q%d" % i, "actions": acts, "principal": {"id": "p%d" % (i % 5), "roles": roles, "attr": {"department": "eng"}},
                    "resource": {"kind": "doc" if i % 11 else "other", "id": "d%d" % i, "scope": scope, "attr": attr}})
    if n >= 12:
        out[6]["resource"]["kind"] = "doc"
    return out


def _run(capi, table, lt, batch, flags_seq, kernel, groups, emulator=True):
    """upload, describe, launch and download under every flag set -> {flags: Result}; on the CPU tier each is the emulator's too"""
    out = {}
    db = table.upload(batch)
    try:
        for flags in flags_seq:
            plan = table.plan(db, flags=flags)
            if kernel is None:      # the switched-off library: the walk's kernels and the general walk, as before
                assert "action groups" not in plan and not plan.startswith("cbh_check_flat") and ("walk2" in plan or plan.startswith("cbh_check_kernel")), plan
            else:
                assert plan.split(",")[0].split("[")[0] == kernel and _groups(plan) == groups and "compact" not in plan, (plan, kernel, groups)
            table.launch(db, now_ns=NOW, flags=flags)
            out[flags] = table.download(db)
            if emulator and _is_sim(capi):
                import hostsim_api
                want = hostsim_api.check(lt, batch, now_ns=NOW, flags=flags)
                assert hostsim_api.last_kind() != 1 or groups == 1      # the emulator took the walk's kernels / the general walk
                for f in FIELDS:
                    assert np.array_equal(getattr(out[flags], f), getattr(want, f)), (f, flags, plan)
    finally:
        db.close()
    return out


def _arrays(prefix, results):
    return {"%s/%d/%s" % (prefix, flags, f): getattr(r, f) for flags, r in results.items() for f in FIELDS}


def _max_groups(batch):
    return (int(batch.req_u32[9].max()) + 3) // 4


def case_directed(capi, kernel="cbh_check_flat_kernel", oracle=True, sizes=SIZES, docs=DIRECTED_DOCS, prefix="directed"):
    lt = _lower(docs)
    assert lt.stats["flat"], lt.stats
    table = capi.Table(lt.blob)
    out = {}
    try:
        for n in sizes:
            inputs = _directed_inputs(n)
            batch = Flattener(lt).flatten(inputs, sort=False)
            assert batch.n_requests == n and int(batch.req_u32[7].max()) <= 4
            offs, cnts = batch.req_u32[8], batch.req_u32[9]
            if n >= 63:
                wide = cnts > 4
                assert n == 257 or (offs[wide] % 4 == 0).any() and (offs[wide] % 4 != 0).any()       # both result-store paths
                assert sorted(set(int(c) for c in cnts)) == (list(COUNTS) if n != 257 else [4, 64])
            flags_seq = (0, capi.F_LENIENT_SCOPE_SEARCH)
            res = _run(capi, table, lt, batch, flags_seq, kernel, _max_groups(batch))
            out.update(_arrays("%s%d" % (prefix, n), res))
            if docs is DIRECTED_DOCS:
                _directed_asserts(lt, inputs, batch, res[0])
                if oracle and n in (1, 65, 257):
                    for flags in flags_seq:
                        _against_oracle(lt, inputs, batch, res[flags], lenient=flags == capi.F_LENIENT_SCOPE_SEARCH)
    finally:
        table.close()
    return out


def _directed_asserts(lt, inputs, batch, res):
    t = 0
    seen_chain = seen_last = 0
    for inp in inputs:
        acts = inp["actions"]
        na = len(acts)
        eff, scp = res.effect[t:t + na], res.scope[t:t + na]
        if acts == CHAIN:
            # (r1: allowed at the root, but the walk meets acme's DENY first)
            assert list(eff) == [ALLOW] * 9 + [DENY, ALLOW, ALLOW] and [lt.scopes[int(s)] for s in scp] == ["acme.hr"] * 4 + ["acme"] * 4 + ["", "acme", "", ""], (eff, scp)
            seen_chain += 1
        if "user" in inp["principal"]["roles"] and inp["resource"]["kind"] == "doc" and inp["resource"]["scope"] in ("", "acme", "acme.hr"):
            for k, a in enumerate(acts):
                if a in ("last_allow", "last_deny"):
                    assert k >= 4 * ((na - 1) // 4) and eff[k] == (ALLOW if a == "last_allow" else DENY), (inp["requestId"], k, a)
                    if a == "last_deny" and "f0" in acts:
                        assert scp[k] != 0xFFFFFFFF and scp[acts.index("f0")] == 0xFFFFFFFF    # a rule's DENY at a scope, not "no match"
                    seen_last += 1
        t += na
    assert t == batch.n_tuples and (len(inputs) not in (63, 64, 65) or (seen_chain and seen_last > 2)), (seen_chain, seen_last)


_oracle = []


def _against_oracle(lt, inputs, batch, res, lenient):
    """every tuple's effect, policy and scope (the CheckOutput the library's ids assemble to, check.go:64-94) and every request's
    "an evaluation error was absorbed" against oracle/check.py"""
    from cerbos_amd.engine import HipEvaluator
    from cerbos_amd.policy.loader import policies_from_docs
    from cerbos_amd.ruletable.build import rule_table_from_policies
    from helpers import norm_actions
    from oracle.check import EvalParams, RuleTableOracle
    if not _oracle:
        _oracle.append(RuleTableOracle(rule_table_from_policies(policies_from_docs(DIRECTED_DOCS))))
    ev = object.__new__(HipEvaluator)          # (assemble reads the lowered table only)
    ev.lt = lt
    outs, bad = HipEvaluator.assemble(ev, inputs, batch, res, "default", allow_unsupported=True)
    assert not bad
    t = 0
    for inp, have in zip(inputs, outs):
        want = _oracle[0].check(inp, EvalParams(now_ns=NOW, lenient_scope_search=lenient))
        assert norm_actions(have) == norm_actions(want), (inp["requestId"], lenient)
        na = len(inp["actions"])
        assert bool(want.get("evaluationErrors")) == bool((res.status[t:t + na] == 1).any()), (inp["requestId"], lenient)
        t += na


# ---- each instantiation

ANY_DOCS = [dict(DIRECTED_DOCS[0], resourcePolicy=dict(DIRECTED_DOCS[0]["resourcePolicy"], rules=DIRECTED_DOCS[0]["resourcePolicy"]["rules"] + [
    {"actions": ["m0", "f1"], "roles": ["guest", "user"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": "P.id in R.attr.viewers"}}},
    {"actions": ["f2", "l0"], "roles": ["manager"], "effect": "EFFECT_DENY", "condition": {"match": {"expr": "R.attr.count > 2"}}}]))] + DIRECTED_DOCS[1:]


def _any_inputs(n):
    ins = _directed_inputs(n)
    for i, inp in enumerate(ins):
        inp["resource"]["attr"]["viewers"] = ["p%d" % v for v in range(i % 4)]
        if i % 3:
            inp["resource"]["attr"]["count"] = i % 5                                    # an int: cross-type numerics are the evaluator's
    return ins


def case_any(capi, kernel="cbh_check_flat_kernel_any"):
    lt = _lower(ANY_DOCS)
    assert lt.stats["flat"] and not lt.stats["flat_closed"], lt.stats
    table = capi.Table(lt.blob)
    out = {}
    try:
        for n in (65,):
            batch = Flattener(lt).flatten(_any_inputs(n), sort=False)
            # (numbers cross the flattener as doubles: the int slots are written into the flattened batch, as tests/test_numeric_edges.py does)
            col = next(i for i, (r, keys) in enumerate(lt.columns) if r == "R" and tuple(keys) == ("count",))
            for i in np.flatnonzero(batch.col_tag[col] == T_DOUBLE):
                batch.col_tag[col, i] = T_INT
                batch.col_val[col, i] = np.uint64(int(np.array([batch.col_val[col, i]], dtype=np.uint64).view(np.float64)[0]))
            assert (batch.col_tag[col] == T_INT).sum() > 20
            res = _run(capi, table, lt, batch, (0, capi.F_LENIENT_SCOPE_SEARCH), kernel, _max_groups(batch))
            out.update(_arrays("any%d" % n, res))
    finally:
        table.close()
    return out


def _c3_inputs(n, seed):
    """C3's requests, every one's action list re-dealt to one of COUNTS from C3's eight actions and names no rule has"""
    rng = np.random.default_rng(seed)
    ins = workloads.c3_requests(n, seed=seed).to_inputs()
    names = list(workloads.C3_ACTIONS) + FILL
    for i, inp in enumerate(ins):
        inp["actions"] = [str(a) for a in rng.choice(names, size=COUNTS[i % len(COUNTS)], replace=False)]
    return ins


def case_c3(capi, kernel="cbh_check_flat_kernel_dr"):
    lt = _lower(workloads.c3_policies())
    table = capi.Table(lt.blob)
    try:
        inputs = _c3_inputs(65, 11)
        batch = Flattener(lt).flatten(inputs, sort=False)
        flags_seq = (0, capi.F_WANT_DERIVED_ROLES, capi.F_WANT_DERIVED_ROLES | capi.F_LENIENT_SCOPE_SEARCH)
        res = _run(capi, table, lt, batch, flags_seq, kernel, 16)
        assert res[capi.F_WANT_DERIVED_ROLES].edr.any()
        return _arrays("c3", res)
    finally:
        table.close()


# ---- derived-role definitions that fail: the case the two marking rules differ on

UP_AT = 5          # the one action (of group 1) that no rule of the leaf scope names: it alone walks up to the parent scope
DR_LEAF = ["a%d" % i for i in range(20)]
DRFAIL_DOCS = [
    {"apiVersion": API, "derivedRoles": {"name": "own", "definitions": [
        {"name": "owner", "parentRoles": ["user"], "condition": {"match": {"expr": "R.attr.owner == P.id"}}},
        {"name": "local", "parentRoles": ["user"], "condition": {"match": {"expr": 'R.attr.zone == "z"'}}}]}},
    {"apiVersion": API, "resourcePolicy": {"resource": "doc", "version": "default", "importDerivedRoles": ["own"], "rules": [
        {"actions": ["up"], "derivedRoles": ["owner"], "effect": "EFFECT_ALLOW"},
        {"actions": ["never"], "derivedRoles": ["local"], "effect": "EFFECT_ALLOW"}]}},     # (a policy's definitions are those its rules name; nobody asks for `never`)
    {"apiVersion": API, "resourcePolicy": {"resource": "doc", "version": "default", "scope": "acme", "rules": [
        {"actions": DR_LEAF, "roles": ["user"], "effect": "EFFECT_ALLOW"}]}},
]


def _drfail_inputs(n=66):
    out = []
    for i in range(n):
        cnt = (8, 20, 4, 8, 20, 1)[i % 6]
        acts = DR_LEAF[:cnt]
        if cnt > UP_AT:
            acts[UP_AT] = "up"
        attr = {"owner": "p%d" % (i % 2)}
        if i % 4:
            attr["zone"] = "z"                                                            # every fourth resource lacks `zone`: the definition `local` fails on it
        out.append({"requestId": "q%d" % i, "actions": acts, "principal": {"id": "p0", "roles": ["user"], "attr": {}},
                    "resource": {"kind": "doc", "id": "d%d" % i, "scope": "acme" if i % 7 else "", "attr": attr}})
    return out


def case_drfail(capi, kernel="cbh_check_flat_kernel_dr", groups=5):
    lt = _lower(DRFAIL_DOCS)
    assert lt.stats["flat"] and len(lt.scopes) == 2, lt.stats
    table = capi.Table(lt.blob)
    try:
        inputs = _drfail_inputs()
        batch = Flattener(lt).flatten(inputs, sort=False)
        want = capi.F_WANT_DERIVED_ROLES
        res = _run(capi, table, lt, batch, (0, want, want | capi.F_LENIENT_SCOPE_SEARCH), kernel, groups)
        t = 0
        met = set()
        for inp in inputs:
            na = len(inp["actions"])
            st0, st1 = res[0].status[t:t + na], res[want].status[t:t + na]
            assert not st0.any(), (inp["requestId"], st0)                                # definitions are evaluated for the derived roles' sake only
            fails = "zone" not in inp["resource"]["attr"]
            if inp["resource"]["scope"] == "acme" and na > UP_AT:
                assert (res[want].effect[t:t + na] == ALLOW).sum() == na - 1 + (inp["resource"]["attr"].get("owner") == "p0")
                if not fails:
                    assert not st1.any()
                elif na <= 16:
                    assert (st1 == 1).all(), (inp["requestId"], st1)                     # the walk kernels' marks: every action of the request
                else:
                    assert st1[UP_AT] == 1 and st1.sum() == 1, (inp["requestId"], st1)   # the general walk's: the action that reached the scope
                met.add((na, fails))
            elif inp["resource"]["scope"] == "acme":
                assert not st1.any(), (inp["requestId"], st1)                            # decided at the leaf: the parent's definitions are not reached
            t += na
        assert met == {(8, True), (8, False), (20, True), (20, False)}, met
        return _arrays("drfail", res)
    finally:
        table.close()


# ---- fuzz.  Of tests/test_fuzz_parity.py's stores only seed 33 lowers to a flat table (none of that file's own SEEDS, range(30), does:
# its generator mixes in principal policies), so the coverage here is in the main tests/test_flat_kernel.py's stores, flat by construction.

FUZZ = (("parity", 33), ("flat", 0), ("flat", 1), ("flat", 2), ("flat", 3), ("deep", 0), ("deep", 1), ("deep", 3))


def _fuzz_case(kind, seed):
    if kind == "parity":
        import test_fuzz_parity as tf
        rng = np.random.default_rng(10_000 + seed)
        docs = tf._policies(rng)
        inputs = tf._requests(rng, 130)
        for inp in inputs:
            inp.pop("auxData", None)
        names = tf.ACTIONS + FILL
    else:
        import test_flat_kernel as tfk
        rng = np.random.default_rng(40_000 + seed)
        docs = tfk._store(rng, None, False, kind == "deep")
        inputs = tfk._requests(rng, 130, False, kind == "deep")
        names = tfk.ACTIONS + FILL
    rng = np.random.default_rng(77_000 + seed)
    for inp in inputs:
        inp["actions"] = [str(a) for a in rng.choice(names, size=int(rng.integers(1, 65)), replace=False)]
    return docs, inputs


def case_fuzz(capi, switched_off=False):
    out = {}
    taken = 0
    for kind, seed in FUZZ:
        docs, inputs = _fuzz_case(kind, seed)
        lt = _lower(docs)
        assert lt.stats["flat"], (kind, seed)
        batch = Flattener(lt).flatten(inputs, sort=bool(seed % 2))
        assert int(batch.req_u32[9].max()) > 16 and int(batch.req_u32[7].max()) <= 4
        table = capi.Table(lt.blob)
        try:
            db = table.upload(batch)
            want = capi.F_WANT_DERIVED_ROLES
            for flags in (0, want, want | capi.F_LENIENT_SCOPE_SEARCH):
                plan = table.plan(db, flags=flags)
                if switched_off:
                    assert "action groups" not in plan and not plan.startswith("cbh_check_flat"), plan
                else:
                    assert plan.startswith("cbh_check_flat_kernel") and _groups(plan) == _max_groups(batch), (kind, seed, plan)
                table.launch(db, now_ns=NOW, flags=flags)
                out.update(_arrays("fuzz_%s%d" % (kind, seed), {flags: table.download(db)}))
            db.close()
            taken += 1
        finally:
            table.close()
    print("fuzz seeds taken: %d of %d" % (taken, len(FUZZ)))
    assert taken == len(FUZZ)
    return out


# ---- the other roads into launch_plan

def case_oneshot(capi):
    """cbh_check_batch on SMALL batches (inputs under 1 MB: one packed block, zero-copy or one copy each way - run_small); compared
    with the RESIDENT reference of the same batches.  Only the results are compared here: the large batches below also show, from
    the library's trace lines, that the one-shot call took action groups."""
    out = {}
    for name, docs, inputs in (("directed65", DIRECTED_DOCS, _directed_inputs(65)), ("drfail", DRFAIL_DOCS, _drfail_inputs())):
        lt = _lower(docs)
        table = capi.Table(lt.blob)
        try:
            batch = capi.pin_batch(Flattener(lt).flatten(inputs, sort=False))
            for flags in ((0, capi.F_LENIENT_SCOPE_SEARCH) if name != "drfail" else (0, capi.F_WANT_DERIVED_ROLES, capi.F_WANT_DERIVED_ROLES | capi.F_LENIENT_SCOPE_SEARCH)):
                out.update(_arrays(name, {flags: table.check(batch, now_ns=NOW, flags=flags, pinned=True)}))
                small = table.check(batch, now_ns=NOW, flags=flags)                      # pageable results
                for f in FIELDS:
                    assert np.array_equal(getattr(small, f), out["%s/%d/%s" % (name, flags, f)]), (name, flags, f)
        finally:
            table.close()
    return out


# Large one-shot batches: inputs of more than 1 MB (cbh_engine.hip SMALL_BATCH_BYTES) take run_range.  (name, docs, inputs, requests, groups)
BIG = (("big_directed", DIRECTED_DOCS, _directed_inputs, 6144, 16), ("big_drfail", DRFAIL_DOCS, _drfail_inputs, 11520, 5))


def _big_flags(capi, name):
    return (0,) if name == "big_directed" else (capi.F_WANT_DERIVED_ROLES,)


def case_big_resident(capi, switched_off=False):
    """the large batches through the resident road (the reference child: with the switch off)"""
    out = {}
    for name, docs, make, n, groups in BIG:
        lt = _lower(docs)
        table = capi.Table(lt.blob)
        try:
            batch = Flattener(lt).flatten(make(n), sort=False)
            res = _run(capi, table, lt, batch, _big_flags(capi, name), None if switched_off else table_kernel(name), groups, emulator=False)
            out.update(_arrays(name, res))
        finally:
            table.close()
    return out


def table_kernel(name):
    return "cbh_check_flat_kernel" if name == "big_directed" else "cbh_check_flat_kernel_dr"


def case_oneshot_big(capi):
    """cbh_check_batch on the large batches by its three ways (run in a child under CBH_TRACE=1, which the parent reads):
    "chunks" - page-locked arrays that are no slab, CBH_CHUNK_REQUESTS = half the batch: two chunks on two streams, each with its own
    clearing of the flag bytes, its own group launches over [lo, hi) and its own status kernel; "slab" - one page-locked slab, one
    launch; "pageable" - ordinary arrays, one launch.  -> the chunked call's arrays; the other two must equal them."""
    out = {}
    for name, docs, make, n, groups in BIG:
        lt = _lower(docs)
        table = capi.Table(lt.blob)
        os.environ["CBH_CHUNK_REQUESTS"] = str(n // 2)
        try:
            inputs = make(n)
            pageable = Flattener(lt).flatten(inputs, sort=False)
            chunked = Flattener(lt).flatten(inputs, sort=False)
            for f in ("req_u32", "tuple_action", "col_tag", "col_val"):                  # each array page-locked by itself
                a = getattr(chunked, f)
                v = capi.pinned_empty(a.shape, a.dtype)
                v[...] = a
                setattr(chunked, f, v)
            slab = capi.pin_batch(Flattener(lt).flatten(inputs, sort=False))
            for flags in _big_flags(capi, name):
                print("way chunks %s" % name, file=sys.stderr, flush=True)
                res = table.check(chunked, now_ns=NOW, flags=flags, pinned=True)
                out.update(_arrays(name, {flags: res}))
                for way, batch, pinned in (("slab", slab, True), ("pageable", pageable, False)):
                    print("way %s %s" % (way, name), file=sys.stderr, flush=True)
                    other = table.check(batch, now_ns=NOW, flags=flags, pinned=pinned)
                    for f in FIELDS:
                        assert np.array_equal(getattr(other, f), getattr(res, f)), (name, way, f)
        finally:
            del os.environ["CBH_CHUNK_REQUESTS"]
            table.close()
    return out


BIG_BODY = r'''
import numpy as np
import test_flat_action_groups as tg
np.savez(%r, **tg.case_oneshot_big(capi))
print("big ok")
'''


def check_oneshot_big(sim):
    """the three ways give the reference's arrays, and the trace shows which way each call went and that it went in action groups"""
    path = os.path.join(tempfile.mkdtemp(prefix="flat_action_groups_"), "big.npz")
    err = _spawn(BIG_BODY % path, {"CBH_TRACE": "1"}, "big ok", sim)
    _same_as_reference(dict(np.load(path)), _reference(sim))
    for name, _, _, n, groups in BIG:
        half = n // 2
        status = 1 if name == "big_drfail" else 0
        ways = err.split("way ")
        by = {w.split("\n", 1)[0]: w for w in ways[1:]}
        chunks, slab, pageable = by["chunks " + name], by["slab " + name], by["pageable " + name]
        assert "pinned chunks=2" in chunks, chunks[-600:]
        for lo, hi in ((0, half), (half, n)):
            assert "[cbh] action groups=%d requests [%d,%d) status kernel=%d" % (groups, lo, hi, status) in chunks, chunks[-600:]
        assert "[cbh] slab " in slab and "[cbh] action groups=%d requests [0,%d) status kernel=%d" % (groups, n, status) in slab, slab[-600:]
        assert "pageable" in pageable and "[cbh] action groups=%d requests [0,%d) status kernel=%d" % (groups, n, status) in pageable, pageable[-600:]


def case_wire(capi, switched_off=False):
    """cbh_wire_check_pb: the device flattens the messages, the outputs are assembled from the wide results -> the outputs' bytes"""
    out = {}
    for name, docs, inputs in (("directed", DIRECTED_DOCS, _directed_inputs(65)), ("drfail", DRFAIL_DOCS, _drfail_inputs())):
        lt = _lower(docs)
        table = capi.Table(lt.blob)
        try:
            data, off = wire.pack_messages([wire.encode_check_input(i) for i in inputs])
            db = table.wire_flatten(data, off)
            plan = table.plan(db, flags=capi.F_WANT_DERIVED_ROLES)
            assert switched_off == ("action groups" not in plan), plan
            assert switched_off or (plan.startswith("cbh_check_flat_kernel") and _groups(plan) == (16 if name == "directed" else 5)), plan
            db.close()
            raw, flags = table.wire_check_pb(data, off, now_ns=NOW, flags=capi.F_WANT_DERIVED_ROLES)
            out["wire_%s/bytes" % name] = np.frombuffer(b"".join(raw), dtype=np.uint8)
            out["wire_%s/len" % name] = np.array([len(r) for r in raw], dtype=np.uint64)
            out["wire_%s/flags" % name] = flags
        finally:
            table.close()
    return out


def case_cross(capi, switched_off=False):
    """cbh_batch_upload_cross: the materialised product of C3 with 5 and 9 actions (below the bound for a table with derived roles: the
    plan without groups, still the product the direct planes are held against) and with 20 (five groups)"""
    lt = _lower(workloads.c3_policies())
    table = capi.Table(lt.blob)
    out = {}
    try:
        n, m = 20, 7
        p, r, acts, aux = _halves_of("c3", n, m, seed=31)
        for a in (5, 9, 20):
            names = (list(workloads.C3_ACTIONS) + FILL)[:a]
            h, po, ro, act = _halves(lt, p, r, names, aux)
            db = upload_halves(table, h, n, m, act, po, ro)
            for flags in (0, capi.F_WANT_DERIVED_ROLES):
                plan = table.plan(db, flags=flags)
                if switched_off or a < 17:
                    assert "action groups" not in plan and "flat" not in plan, plan
                else:
                    assert plan == "cbh_check_flat_kernel_dr, 5 action groups", plan
                table.launch(db, now_ns=NOW, flags=flags)
                out.update(_arrays("cross%d" % a, {flags: table.download(db)}))
            db.close()
    finally:
        table.close()
    return out


# ---- 1. the plan

def check_plan(capi):
    lt = _lower(workloads.c2_policies())
    table = capi.Table(lt.blob)
    try:
        inputs = workloads.c2_requests(65, seed=5).to_inputs()
        four = table.upload(Flattener(lt).flatten(inputs))
        assert table.plan(four).startswith("cbh_check_flat_kernel[compact") and "action groups" not in table.plan(four)
        four.close()
        wide = ["archive", "share", "print", "rename", "move"]
        inputs[40]["actions"] = list(inputs[40]["actions"]) + wide                          # one request of nine actions
        db = table.upload(Flattener(lt).flatten(inputs))
        plan = table.plan(db)
        assert plan == "cbh_check_flat_kernel, 3 action groups", plan                     # (before action groups: cbh_walk2_awide_kernel + cbh_walk2_kernel)
        for flags in (capi.F_STRICT_EVALUATION, capi.F_WANT_EFFECTIVE_POLICIES):
            assert "action groups" not in table.plan(db, flags=flags) and not table.plan(db, flags=flags).startswith("cbh_check_flat_kernel,"), table.plan(db, flags=flags)
        db.close()
        inputs[3]["principal"]["roles"] = ["user", "manager", "a", "b", "c"]
        db = table.upload(Flattener(lt).flatten(inputs))
        assert "action groups" not in table.plan(db) and "flat" not in table.plan(db), table.plan(db)
        db.close()
        # below the measured bounds the plan is the one without groups: C2 (no derived roles) at five actions ...
        inputs = workloads.c2_requests(65, seed=5).to_inputs()
        inputs[40]["actions"] = list(inputs[40]["actions"]) + wide[:1]
        db = table.upload(Flattener(lt).flatten(inputs))
        assert table.plan(db).endswith("cbh_walk2_kernel") and "flat" not in table.plan(db), table.plan(db)
        db.close()
    finally:
        table.close()
    # ... and C3 (derived roles) up to sixteen; seventeen is five groups
    lt = _lower(workloads.c3_policies())
    table = capi.Table(lt.blob)
    try:
        for cnt, groups in ((5, 0), (16, 0), (17, 5)):
            inputs = workloads.c3_requests(65, seed=5).to_inputs()
            inputs[40]["actions"] = (list(workloads.C3_ACTIONS) + FILL)[:cnt]
            db = table.upload(Flattener(lt).flatten(inputs))
            plan = table.plan(db, flags=capi.F_WANT_DERIVED_ROLES)
            assert (plan == "cbh_check_flat_kernel_dr, 5 action groups") if groups else (plan.endswith("cbh_walk2_kernel") and "flat" not in plan), (cnt, plan)
            db.close()
    finally:
        table.close()


CASES = {"directed": case_directed, "any": case_any, "c3": case_c3, "drfail": case_drfail, "fuzz": case_fuzz, "wire": case_wire, "cross": case_cross}


# ---- the switched-off library: one child process per tier writes every case's arrays

REFERENCE_BODY = r'''
import numpy as np
import test_flat_action_groups as tg
out = {}
out.update(tg.case_directed(capi, kernel=None))
out.update(tg.case_any(capi, kernel=None))
out.update(tg.case_c3(capi, kernel=None))
out.update(tg.case_drfail(capi, kernel=None, groups=1))
out.update(tg.case_fuzz(capi, switched_off=True))
out.update(tg.case_wire(capi, switched_off=True))
out.update(tg.case_cross(capi, switched_off=True))
out.update(tg.case_big_resident(capi, switched_off=True))
np.savez(%r, **out)
print("reference ok")
'''
_reference_files = {}


def _child(body, env, ok, sim):
    if sim:
        import test_sim_engine as ts
        return ts._in_own_process(body, env)
    from test_cross_direct import _gpu_child
    return _gpu_child(body, env, ok)


def _spawn(body, env, ok, sim):
    """a child process of its own on the simulator build or on the device (the switches are read once per process) -> its stderr"""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    if sim:
        code = ("import sys; sys.path[:0] = [%r, %r]\nfrom sim_engine import sim_engine\nwith sim_engine() as capi:\n" % (here, root)
                + "".join("    " + line + "\n" for line in body.strip().splitlines()))
    else:
        code = "import sys; sys.path[:0] = [%r, %r]\nfrom cerbos_amd import capi\n" % (here, root) + body
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0 and ok in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stderr


def _reference(sim):
    """{key: array} of every case under CBH_FLAT_ACTION_GROUPS=0, computed once per tier"""
    if sim not in _reference_files:
        path = os.path.join(tempfile.mkdtemp(prefix="flat_action_groups_"), "reference.npz")
        _child(REFERENCE_BODY % path, {"CBH_FLAT_ACTION_GROUPS": "0"}, "reference ok", sim)
        _reference_files[sim] = path
    return np.load(_reference_files[sim])


def _same_as_reference(got, ref, renamed=None):
    assert got
    for key, arr in got.items():
        rkey = renamed(key) if renamed else key
        assert rkey in ref.files, rkey
        assert np.array_equal(arr, ref[rkey]), key


def check_case(capi, name):
    _same_as_reference(CASES[name](capi), _reference(_is_sim(capi)))


def check_oneshot(capi):
    _same_as_reference(case_oneshot(capi), _reference(_is_sim(capi)))


# the walks and result forms that are read once per process: a child each, compared with the same reference file
MODE_BODY = r'''
import numpy as np
import test_flat_action_groups as tg
ref = np.load(%r)
tg._same_as_reference(tg.case_directed(capi, kernel=%r, oracle=False, sizes=(65, 257)), ref)
tg._same_as_reference(tg.case_any(capi, kernel=%r), ref)
tg._same_as_reference(tg.case_drfail(capi, kernel=%r), ref)
print("mode ok")
'''
MODES = {"staged": ({"CBH_FORCE_STAGED": "1"}, ("cbh_check_flat_kernel_staged", "cbh_check_flat_kernel_any_staged", "cbh_check_flat_kernel_staged")),
         "masks": ({"CBH_FLAT_MASKS": "1"}, ("cbh_check_flat_kernel_masks", "cbh_check_flat_kernel_any_masks", "cbh_check_flat_kernel_masks")),
         "wide_results": ({"CBH_PACKED_RESULTS": "0"}, ("cbh_check_flat_kernel", "cbh_check_flat_kernel_any", "cbh_check_flat_kernel_dr"))}


def check_mode(mode, sim):
    env, kernels = MODES[mode]
    _child(MODE_BODY % ((_reference(sim) and _reference_files[sim],) + kernels), env, "mode ok", sim)


def check_switch_off(sim):
    """CBH_FLAT_ACTION_GROUPS=0: the plan of before (the reference child asserts it for every case it runs)"""
    assert len(_reference(sim).files) > 50


# ---- CPU tier: the simulator


@pytest.fixture()
def engine():
    with sim_engine() as capi:
        yield capi


def test_plan_on_simulator(engine):
    check_plan(engine)


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_equals_the_switched_off_library_on_simulator(engine, name):
    check_case(engine, name)


def test_one_shot_small_batches_on_simulator(engine):
    check_oneshot(engine)


def test_one_shot_large_batches_on_simulator(engine):
    _same_as_reference(case_big_resident(engine), _reference(True))
    check_oneshot_big(True)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_other_walks_and_result_forms_on_simulator(mode):
    check_mode(mode, True)


def test_switch_off_on_simulator():
    check_switch_off(True)


def test_failing_allocations_are_survived():
    """Fault injection (simulator only): the k-th device allocation from now on fails, for every k until the calls succeed - the upload
    of a wide batch of a table with derived roles and its first check (which allocates the per-request flag bytes) either report an
    error with a text or give the right results, and the batch decides correctly afterwards."""
    import test_sim_engine as ts
    ts._in_own_process('''
import ctypes as C
import numpy as np
import test_flat_action_groups as tg
from cerbos_amd.flatten import Flattener
lib = capi.load()
lib.cbh_sim_set_alloc_budget.argtypes = [C.c_long]
lt = tg._lower(tg.DRFAIL_DOCS)
batch = Flattener(lt).flatten(tg._drfail_inputs(), sort=False)
FL = capi.F_WANT_DERIVED_ROLES
ref = capi.Table(lt.blob)
db = ref.upload(batch)
assert tg._groups(ref.plan(db, flags=FL)) == 5
ref.launch(db, now_ns=tg.NOW, flags=FL)
want = ref.download(db)
assert (want.status == 1).any()
db.close()
ref.close()
for phase in ("upload", "check"):
    failed = 0
    for k in range(200):
        table = capi.Table(lt.blob)          # (a fresh table: empty pools, every buffer a real allocation)
        db = table.upload(batch) if phase == "check" else None
        lib.cbh_sim_set_alloc_budget(k)
        try:
            if phase == "upload":
                db = table.upload(batch)
            else:
                table.launch(db, now_ns=tg.NOW, flags=FL)
        except capi.HipEngineError as e:
            assert str(e), "an error without a message"
            failed += 1
        finally:
            lib.cbh_sim_set_alloc_budget(-1)
        if db is None:
            db = table.upload(batch)
        table.launch(db, now_ns=tg.NOW, flags=FL)      # the batch is usable after a failed call
        got = table.download(db)
        for f in tg.FIELDS:
            assert np.array_equal(getattr(got, f), getattr(want, f)), (phase, k, f)
        db.close()
        table.close()
        if failed == k:                       # the k-th was not reached: the call had enough
            break
    assert failed >= 1 and failed == k, (phase, failed, k)
''', {})


# ---- GPU tier


def _on_gpu_or_simulator(fn, *args):
    """(under CBH_TEST_SIM_ENGINE=1 tests/conftest.py has pointed capi at the simulator build: the children follow, see _is_sim)"""
    from cerbos_amd import capi
    return fn(capi, *args)


@pytest.mark.gpu
def test_plan_on_gpu():
    _on_gpu_or_simulator(check_plan)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_case_equals_the_switched_off_library_on_gpu(name):
    _on_gpu_or_simulator(check_case, name)


@pytest.mark.gpu
def test_one_shot_small_batches_on_gpu():
    _on_gpu_or_simulator(check_oneshot)


@pytest.mark.gpu
def test_one_shot_large_batches_on_gpu():
    sim = os.environ.get("CBH_TEST_SIM_ENGINE") == "1"
    _on_gpu_or_simulator(lambda capi: _same_as_reference(case_big_resident(capi), _reference(sim)))
    check_oneshot_big(sim)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODES))
def test_other_walks_and_result_forms_on_gpu(mode):
    check_mode(mode, os.environ.get("CBH_TEST_SIM_ENGINE") == "1")


@pytest.mark.gpu
def test_switch_off_on_gpu():
    check_switch_off(os.environ.get("CBH_TEST_SIM_ENGINE") == "1")
