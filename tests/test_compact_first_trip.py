"""The compact flat kernels' prologue in ONE trip to memory (cbh_check_flat.h flat_body COMPACT, cbh_check_wave.h cc_fill_compact, cbh_vm.h
cbh_creq_first): the columns' and the tags' copies are issued in front of the record's load, unrolled behind uniform guards, and the
chain's first scope comes with the record - cbh_compact_pack_kernel resolves it when the batch is uploaded, under both scope searches
(the scope field of word 2, bits 30 and 31 of word 3), and neither compact branch of flat_body reads the scope arrays for it.

Nothing a caller sees changes.  Every case compares cbh_check_resident + cbh_result_download on ONE resident batch with cbh_check_batch
(the one-shot road keeps the wide arrays and calls chain_first), every field bit for bit, and asserts that the resident plan reads
the compact inputs - a case that fell back to the wide form would prove nothing.  Where oracle/check.py is named the effects are compared
with it too.
  C2 at 1, 63, 64, 65, 255, 256, 257 and 1000 requests   a workgroup is 256 lanes, a wave 64: partial waves, waves wholly beyond the batch's
                                                          end (they shadow its first request), narrow and wide columns side by side
  every column narrow / no column narrow                  the unrolled guards at their two ends; one value with a high word makes a column wide
  scopes "", a, a.b, a.b.c, a.b without a policy          requests at each of them, at a.b.c.d and at zzz: the strict search fails where the lenient
                                                          one climbs; the flags alternate (0, LENIENT, 0, LENIENT) on the same resident batch
  257 scopes, requests at the highest indices             the field at indices of 255, 256 and beyond (tests/test_scope_limits.py's store)
  the direct cross road, 3 x 5 over the scoped table      the resource's record decides the chain; against the materialised product
CPU tier: the library's host side on the simulator (tests/sim_engine.py).  GPU tier: the library on the device."""
import numpy as np
import pytest

from cerbos_amd import workloads
from cerbos_amd.flatten import Flattener
from cerbos_amd.lower.blob import lower_rule_table
from cerbos_amd.policy.loader import policies_from_docs
from cerbos_amd.ruletable.build import rule_table_from_policies
from sim_engine import sim_engine

API = "api.cerbos.dev/v1"
NOW = 1_700_000_000_000_000_000
FIELDS = ("effect", "status", "policy", "scope", "edr")
COMPACT = "[compact inputs"
SCOPES = ["", "a", "a.b", "a.b.c", "a.b.c.d", "zzz"]


def _lower(docs):
    rt = rule_table_from_policies(policies_from_docs(docs))
    return rt, lower_rule_table(rt)


def _same(capi, lt, batch, flag_seq):
    """cbh_check_batch (wide) against launch + download on ONE resident batch, for every flags word of `flag_seq` in turn, every field
    bit for bit.  -> (the resident plan, the resident results per launch)"""
    table = capi.Table(lt.blob)
    db = table.upload(batch)
    out = []
    try:
        for flags in flag_seq:
            want = table.check(batch, now_ns=NOW, flags=flags)
            table.launch(db, now_ns=NOW, flags=flags)
            have = table.download(db)
            for f in FIELDS:
                assert np.array_equal(getattr(have, f), getattr(want, f)), (flags, f)
            out.append(have)
        plan = table.plan(db, flags=flag_seq[0])
        assert COMPACT in plan, plan
        return plan, out
    finally:
        db.close()
        table.close()


def _narrow(plan):
    return int(plan.split("narrow columns 0x")[1].split("]")[0], 16)


def _effects(rt, inputs, lenient):
    from oracle.check import EvalParams, RuleTableOracle
    orc = RuleTableOracle(rt)
    want = []
    for inp in inputs:
        out = orc.check(inp, EvalParams(now_ns=NOW, lenient_scope_search=lenient))
        want.extend(1 if out["actions"][a]["effect"] == "EFFECT_ALLOW" else 2 for a in inp["actions"])
    return np.array(want, dtype=np.uint8)


# ---- the stores


_C2 = []


def c2_table():
    if not _C2:
        _C2.append(_lower(workloads.c2_policies())[1])
    return _C2[0]


def number_docs():
    """three columns, all numbers: a batch decides by its values whether their planes are narrow"""
    rules = [{"actions": ["view"], "effect": "EFFECT_ALLOW", "roles": ["user"], "condition": {"match": {"expr": "R.attr.x > 1.5"}}},
             {"actions": ["edit"], "effect": "EFFECT_ALLOW", "roles": ["user"], "condition": {"match": {"expr": "R.attr.y < 4.5"}}},
             {"actions": ["edit"], "effect": "EFFECT_DENY", "roles": ["guest"], "condition": {"match": {"expr": "P.attr.z >= 2.5"}}},
             {"actions": ["drop"], "effect": "EFFECT_ALLOW", "roles": ["admin"]}]
    return [{"apiVersion": API, "resourcePolicy": {"resource": "doc", "version": "default", "rules": rules}}]


def number_requests(n, value):
    return [{"requestId": "q%d" % i, "actions": ["view", "edit", "drop", "none"][: 1 + i % 4],
             "principal": {"id": "p%d" % i, "roles": [["user"], ["guest", "user"], ["admin"], ["guest"]][i % 4], "attr": {"z": value(i, 2)}},
             "resource": {"kind": "doc", "id": "d%d" % i, "attr": {"x": value(i, 0), "y": value(i, 1)}}} for i in range(n)]


def scoped_docs():
    """kind doc at "", a and a.b.c - a.b is a scope of the table without a resource policy; each level names its own action and
    overrides one of the level above"""
    def pol(scope, rules):
        p = {"resource": "doc", "version": "default", "rules": rules}
        if scope:
            p["scope"] = scope
        return {"apiVersion": API, "resourcePolicy": p}
    return [pol("", [{"actions": ["view", "root"], "effect": "EFFECT_ALLOW", "roles": ["user"]},
                     {"actions": ["edit"], "effect": "EFFECT_DENY", "roles": ["user"]}]),
            pol("a", [{"actions": ["edit", "at_a"], "effect": "EFFECT_ALLOW", "roles": ["user"]},
                      {"actions": ["view"], "effect": "EFFECT_DENY", "roles": ["guest"]}]),
            pol("a.b.c", [{"actions": ["at_abc"], "effect": "EFFECT_ALLOW", "roles": ["user", "guest"]},
                          {"actions": ["at_a"], "effect": "EFFECT_DENY", "roles": ["user"]}])]


SCOPED_ACTIONS = ["view", "edit", "at_a", "at_abc", "root"]


def scoped_requests(n):
    return [{"requestId": "q%d" % i, "actions": [SCOPED_ACTIONS[(i + k) % 5] for k in range(1 + (i // 6) % 4)],
             "principal": {"id": "p%d" % i, "roles": [["user"], ["guest"], ["guest", "user"]][(i // 6) % 3], "attr": {}},
             "resource": {"kind": "doc", "id": "d%d" % i, "attr": {}, "scope": SCOPES[i % 6]}} for i in range(n)]


_SCOPED = []


def scoped_table():
    if not _SCOPED:
        rt, lt = _lower(scoped_docs())
        assert lt.stats["flat"] and not lt.stats["derived_roles"], lt.stats
        assert "a.b" in lt.scopes and "a.b.c" in lt.scopes, lt.scopes   # a scope of the table that no resource policy has
        _SCOPED.append((rt, lt))
    return _SCOPED[0]


# ---- the bodies: the same on the simulator and on the device


def check_c2(capi, n):
    lt = c2_table()
    batch = workloads.c2_requests(n, seed=40 + n).to_batch(Flattener(lt))
    assert batch.n_requests == n
    plan, _ = _same(capi, lt, batch, (capi.F_WANT_DERIVED_ROLES, capi.F_LENIENT_SCOPE_SEARCH))
    assert plan.startswith("cbh_check_flat_kernel"), plan
    if n >= 255:   # C2's strings and bools have 32-bit planes, its numbers do not: both kinds of copy in one launch
        ncols = min(batch.col_tag.shape[0], 16)
        assert 0 < _narrow(plan) < (1 << ncols) - 1, (plan, ncols)


def check_c2_against_oracle(capi):
    """the smallest sizes once more, against oracle/check.py"""
    rt, lt = _lower(workloads.c2_policies())
    cr = workloads.c2_requests(65, seed=7)
    batch = cr.to_batch(Flattener(lt))
    _, res = _same(capi, lt, batch, (0,))   # (the results come back in input order)
    assert np.array_equal(res[0].effect, _effects(rt, cr.to_inputs(), False))


def check_column_ends(capi):
    _, lt = _lower(number_docs())
    fl = Flattener(lt)
    n = 130
    ncols = 3
    for how, value in (("all narrow", lambda i, c: 0.0),                                         # 0.0: both words zero
                       ("none narrow", lambda i, c: 2.5 if i == 11 * (c + 1) else 0.0),          # ONE value with a high word in each column
                       ("no value narrow", lambda i, c: float((i + c) % 5) + 0.5)):
        batch = fl.flatten(number_requests(n, value))
        assert batch.col_tag.shape[0] == ncols, batch.col_tag.shape
        plan, res = _same(capi, lt, batch, (0, capi.F_LENIENT_SCOPE_SEARCH))
        assert _narrow(plan) == ((1 << ncols) - 1 if how == "all narrow" else 0), (how, plan)
        if how == "no value narrow":
            assert len(set(res[0].effect.tolist())) > 1   # the values decide


def check_scoped(capi):
    rt, lt = scoped_table()
    inputs = scoped_requests(65)
    batch = Flattener(lt).flatten(inputs, sort=False)
    assert batch.n_requests == 65 and batch.tuple_perm is None
    L = capi.F_LENIENT_SCOPE_SEARCH
    plan, res = _same(capi, lt, batch, (0, L, 0, L))
    assert plan.startswith("cbh_check_flat_kernel") and "_dr" not in plan, plan
    want = {False: _effects(rt, inputs, False), True: _effects(rt, inputs, True)}
    assert not np.array_equal(want[False], want[True]), "the two searches decide the same: the store proves nothing"
    for have, lenient in zip(res, (False, True, False, True)):
        assert np.array_equal(have.effect, want[lenient]), lenient
    # the strict search stands nowhere at a.b (no policy), a.b.c.d and zzz (not the table's): NO_MATCH, no scope
    assert np.array_equal(res[0].effect, res[2].effect) and np.array_equal(res[1].effect, res[3].effect)


def check_257_scopes(capi):
    import test_scope_limits as ts
    _, lt = _lower(ts.count_docs(257))
    assert len(lt.scopes) == 257
    inputs, _ = ts.chain_requests(4, targets=ts._targets(lt))
    batch = Flattener(lt).flatten(inputs, sort=False)
    plan, res = _same(capi, lt, batch, (capi.F_WANT_DERIVED_ROLES, capi.F_WANT_DERIVED_ROLES | capi.F_LENIENT_SCOPE_SEARCH))
    assert plan.startswith("cbh_check_flat_kernel"), plan
    for r in res:   # decided AT the highest indices: the scope word of a tuple a policy decided is its scope's index
        assert int(r.scope[r.scope != 0xFFFFFFFF].max()) == 256, r.scope.max()


def check_cross(capi):
    import test_cross_direct as tc
    rt, lt = scoped_table()
    ps = [{"id": "p%d" % i, "roles": [["user"], ["guest"], ["guest", "user"]][i], "attr": {}} for i in range(3)]
    rs = [{"kind": "doc", "id": "d%d" % j, "attr": {}, "scope": SCOPES[1 + j]} for j in range(5)]
    acts = ["view", "edit", "at_a", "at_abc"]
    h, po, ro, act = tc._halves(lt, ps, rs, acts)
    table = capi.Table(lt.blob)
    try:
        names = tc._same(table, h, 3, 5, act, po, ro, flag_seq=(0, capi.F_LENIENT_SCOPE_SEARCH, 0))
        assert names == {"cbh_check_flat_kernel_x"}, names
        db = tc.upload_halves(table, h, 3, 5, act, po, ro)      # the materialised product reads compact inputs too
        try:
            assert COMPACT in table.plan(db, flags=0)
        finally:
            db.close()
    finally:
        table.close()


# ---- CPU tier: the simulator


@pytest.fixture()
def engine():
    with sim_engine() as capi:
        yield capi


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_c2_on_simulator(engine, n):
    check_c2(engine, n)


def test_c2_against_oracle_on_simulator(engine):
    check_c2_against_oracle(engine)


def test_column_ends_on_simulator(engine):
    check_column_ends(engine)


def test_scoped_table_alternating_searches_on_simulator(engine):
    check_scoped(engine)


def test_257_scopes_on_simulator(engine):
    check_257_scopes(engine)


def test_direct_cross_on_simulator(engine):
    check_cross(engine)


# ---- GPU tier


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_c2_on_gpu(n):
    from cerbos_amd import capi
    check_c2(capi, n)


@pytest.mark.gpu
def test_c2_against_oracle_on_gpu():
    from cerbos_amd import capi
    check_c2_against_oracle(capi)


@pytest.mark.gpu
def test_column_ends_on_gpu():
    from cerbos_amd import capi
    check_column_ends(capi)


@pytest.mark.gpu
def test_scoped_table_alternating_searches_on_gpu():
    from cerbos_amd import capi
    check_scoped(capi)


@pytest.mark.gpu
def test_257_scopes_on_gpu():
    from cerbos_amd import capi
    check_257_scopes(capi)


@pytest.mark.gpu
def test_direct_cross_on_gpu():
    from cerbos_amd import capi
    check_cross(capi)
