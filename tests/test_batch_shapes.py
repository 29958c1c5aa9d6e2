"""One batch of requests, made four ways, at the shapes where the batch's shape record selects a kernel.

The same N x M x A requests (N = 9 principals, M = 7 resources) enter as
  (1) a host batch (cross.cross_product_batch + cbh_batch_upload_on),
  (2) a materialised product (cbh_batch_upload_cross),
  (3) a pairs batch over ALL pairs of a direct set (cbh_cross_pairs_upload), where the set exists,
  (4) the direct set itself (cbh_cross_upload_ex / cbh_cross_check), where it exists.
Every maker works out the batch's shape - largest action and role counts, where the wide requests lie, plain tags - by code of its
own; what is asserted here is that they agree: the three batch forms get the same plan string (cbh_plan_describe) under every flags
word and every field of their downloads is equal, and the set's planes are the product's effects and statuses bit for bit.

The shapes: 4 and 5, 8 and 9, 16 and 17 actions x 4 and 5, 8 and 9, and 16 roles, on a flat table without derived roles (C2), a flat
table with them (C3) and a table the walk decides (C5, CBH_MF_WALK2).  Principals keep different role counts and the widest ones sit
in the middle of the order, so that the range of wide requests is a proper part of the batch.
And the rows the plain-tags scan reads: an `int` in a sensitive principal-side column counts only in a principal's row of the halves.
CPU tier: the library's host side and the kernels' source on the simulator (tests/sim_engine.py).  GPU tier: the same bodies on the device."""
import numpy as np
import pytest

from cerbos_amd import workloads
from cerbos_amd.cross import cross_product_batch, direct_upload_halves, upload_halves
from cerbos_amd.flatten import Flattener
from sim_engine import sim_engine
from test_cross_device import ALLOW, FIELDS, NOW, _halves_of, _lower
from test_cross_direct import API, _column_halves, _halves, _named_x, _words, table_error
from test_cross_direct_ex import _action_list

N, M = 9, 7
ACTIONS = (4, 5, 8, 9, 16, 17)
ROLES = (4, 5, 8, 9, 16)
MIN_GROUPS = {"c2": 3, "c3": 5}   # cbh_check_walk2.h CBH_FLAT_MIN_GROUPS / CBH_FLAT_MIN_GROUPS_DR (C3 has derived roles)
T_INT = 2   # flatten.T_INT
# a closed flat table (its plan depends on the tags) with a numeric comparison on either side
LEVEL_DOCS = [{"apiVersion": API, "resourcePolicy": {"resource": "doc", "version": "default", "rules": [
    {"actions": ["view"], "roles": ["user", "guest"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": "P.attr.level >= 3.5"}}},
    {"actions": ["edit"], "roles": ["user", "manager"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": "R.attr.amount > 100.5"}}},
    {"actions": ["delete"], "roles": ["manager", "admin"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": "R.attr.owner == P.id"}}}]}}]


def _role_counts(r):
    """nine principals, the two with `r` roles at positions 2 and 4, one without a role"""
    return [min(r, 2), 0, r, min(r, 4), r, 1, min(r, 3), min(r, 4), 1]


def _principals(ps, known, r):
    out = []
    for p, cnt in zip(ps, _role_counts(r)):
        pool = list(dict.fromkeys(list(p["roles"]) + list(known) + ["zr%d" % i for i in range(16)]))
        out.append(dict(p, roles=pool[:cnt]))
    assert max(len(p["roles"]) for p in out) == r
    return out


def _four_ways(capi, table, lt, ps, rs, names, aux, flag_seq):
    """-> (plans of the host batch per flags word, the set's describe or None)"""
    fl = Flattener(lt)
    a = len(names)
    cb = cross_product_batch(fl, lt.columns, ps, rs, names, aux, sort=False)
    h, po, ro, act = _halves(lt, ps, rs, names, aux, sort=False)
    hb = table.upload(cb)
    db = upload_halves(table, h, N, M, act, po, ro)
    cs = direct_upload_halves(table, h, N, M, act, po, ro, accept=capi.CX_ALL | capi.CX_ROLE_GROUPS)
    pb = cs.pairs_batch(np.tile(np.arange(N), M), np.repeat(np.arange(M), N)) if cs is not None else None
    forms = [x for x in (hb, db, pb) if x is not None]
    plans = []
    try:
        assert all(x.n_requests == N * M and x.n_tuples == N * M * a for x in forms)
        for flags in flag_seq:
            plan = table.plan(hb, flags=flags)
            plans.append(plan)
            for x in forms[1:]:
                assert table.plan(x, flags=flags) == plan, (flags, table.plan(x, flags=flags), plan)
            for x in forms:
                table.launch(x, now_ns=NOW, flags=flags)
            want = table.download(hb)
            for x in forms[1:]:
                have = table.download(x)
                for f in FIELDS:
                    assert np.array_equal(getattr(have, f), getattr(want, f)), (flags, f, x is pb)
            if cs is not None and not cs.describe(flags).startswith("none"):
                _named_x(cs.describe(flags))
                allow, flagged = cs.check(0, M, flags=flags, now_ns=NOW, want_flagged=True)
                for k in range(a):
                    assert np.array_equal(allow[k], _words(want.effect.reshape(M, N, a)[:, :, k] == ALLOW)), (flags, k, "allow")
                    assert np.array_equal(flagged[k], _words(want.status.reshape(M, N, a)[:, :, k] != 0)), (flags, k, "flagged")
        return plans, (cs.describe(0) if cs is not None else None)
    finally:
        for x in forms:
            x.close()
        if cs is not None:
            cs.close()


def check_boundaries(capi, name):
    """every (actions, roles) of ACTIONS x ROLES on one workload's table"""
    lt = _lower(getattr(workloads, name + "_policies")())
    flat = bool(lt.stats["flat"])
    assert flat == (name != "c5")
    ps0, rs, acts, aux = _halves_of(name, N, M, seed=31)
    known = workloads.C3_ROLES if name in ("c3", "c5") else ["user", "manager"]
    flag_seq = (0, capi.F_WANT_DERIVED_ROLES, capi.F_STRICT_EVALUATION, capi.F_WANT_EFFECTIVE_POLICIES)
    table = capi.Table(lt.blob)
    seen = set()
    try:
        for r in ROLES:
            ps = _principals(ps0, known, r)
            for a in ACTIONS:
                plans, desc = _four_ways(capi, table, lt, ps, rs, _action_list(acts, a), aux, flag_seq)
                seen.add(plans[0].split("[")[0])
                if flat:       # every one of these shapes has a direct form; its groups are the shape's
                    assert desc is not None, (a, r, table_error())
                    assert (", %d action groups" % ((a + 3) // 4) in desc) == (a > 4), (a, r, desc)
                    assert (", %d role groups" % ((r + 3) // 4) in desc) == (r > 4), (a, r, desc)
                    # a flat kernel decides the batch of at most four roles: once, or in action groups from MIN_GROUPS groups on
                    groups = (a + 3) // 4
                    grouped = r <= 4 and groups >= MIN_GROUPS[name]
                    assert plans[0].startswith("cbh_check_flat_kernel") == (r <= 4 and (a <= 4 or grouped)), (a, r, plans[0])
                    assert (", %d action groups" % groups in plans[0]) == grouped, (a, r, plans[0])
                else:
                    assert desc is None and "cbh_walk2" in plans[0], (a, r, desc, plans[0])
    finally:
        table.close()
    assert len(seen) > 1, seen     # the shapes did select different kernels


def check_int_tag_rows(capi):
    """LEVEL_DOCS reads P.attr.level against a double: its column is principal-side and sensitive.  An `int` tag there in a
    RESOURCE's row of the halves is in no request of the product: plan, set and results are those of the clean halves.  The same tag
    in a principal's row is in M requests: the plain-tags plan is lost (by the host batch of those requests too), and the set."""
    lt = _lower(LEVEL_DOCS)
    assert lt.stats["flat"] and lt.stats["flat_closed"], lt.stats
    level = [i for i, (root, path) in enumerate(lt.columns) if root == "P" and "level" in str(path)]
    assert len(level) == 1, lt.columns
    c = level[0]
    ps, rs = _column_halves(N, M, np.random.default_rng(3))
    acts = ["view", "edit", "delete", "approve"]
    table = capi.Table(lt.blob)
    try:
        def product(row):
            h, po, ro, act = _halves(lt, ps, rs, acts, sort=False)
            if row is not None:
                h.col_tag[c, row], h.col_val[c, row] = T_INT, 7
            db = upload_halves(table, h, N, M, act, po, ro)
            cs = direct_upload_halves(table, h, N, M, act, po, ro)
            text = table_error()
            try:
                table.launch(db, now_ns=NOW)
                return table.plan(db), table.download(db), cs is not None, text
            finally:
                db.close()
                if cs is not None:
                    cs.close()

        def host(row):
            cb = cross_product_batch(Flattener(lt), lt.columns, ps, rs, acts, None, sort=False)
            if row is not None:
                cb.col_tag[c, row::N], cb.col_val[c, row::N] = T_INT, 7      # principal `row` of every resource
            hb = table.upload(cb)
            try:
                table.launch(hb, now_ns=NOW)
                return table.plan(hb), table.download(hb)
            finally:
                hb.close()

        clean_plan, clean, direct, _ = product(None)
        assert direct and clean_plan.startswith("cbh_check_flat_kernel[compact inputs"), clean_plan
        assert host(None)[0] == clean_plan
        plan, res, direct, _ = product(N + 1)                     # a resource's row
        assert plan == clean_plan and direct
        for f in FIELDS:
            assert np.array_equal(getattr(res, f), getattr(clean, f)), f
        plan, res, direct, text = product(1)                      # a principal's row
        assert plan != clean_plan and plan.startswith("cbh_check_flat_kernel_any"), plan
        assert not direct and "needs the evaluator" in text, text
        host_plan, host_res = host(1)
        assert host_plan == plan
        for f in FIELDS:
            assert np.array_equal(getattr(res, f), getattr(host_res, f)), f
    finally:
        table.close()


# ---- CPU tier: the simulator


@pytest.fixture()
def engine():
    with sim_engine() as capi:
        yield capi


@pytest.mark.parametrize("name", ("c2", "c3", "c5"))
def test_boundaries_on_simulator(engine, name):
    check_boundaries(engine, name)


def test_int_tag_rows_on_simulator(engine):
    check_int_tag_rows(engine)


# ---- GPU tier


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("c2", "c3", "c5"))
def test_boundaries_on_gpu(name):
    from cerbos_amd import capi
    check_boundaries(capi, name)


@pytest.mark.gpu
def test_int_tag_rows_on_gpu():
    from cerbos_amd import capi
    check_int_tag_rows(capi)
