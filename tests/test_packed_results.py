"""The resident path's packed result form (cbh_vm.h cbh_pk_word): a flat launch of cbh_check_resident writes one word per tuple instead
of effect, status, policy and scope, and no derived-role mask for a table without derived roles; cbh_result_download gives the wide
form's bytes.  Compared bit for bit with cbh_check_batch, whose one-shot path keeps the wide form, on the benchmark's flat tables, on
random flat stores (requests of zero to four actions: the unaligned stores), on a table whose scope ids are too wide for the word (the
wide form) and across launches that switch between the forms.
CPU tier: the library's host side on the simulator (tests/sim_engine.py).  GPU tier: the library on the device."""
import numpy as np
import pytest

from cerbos_amd import workloads
from cerbos_amd.flatten import Flattener
from cerbos_amd.lower.blob import lower_rule_table
from cerbos_amd.policy.loader import policies_from_docs
from cerbos_amd.ruletable.build import rule_table_from_policies
from sim_engine import sim_engine

NOW = 1_700_000_000_000_000_000
API = "api.cerbos.dev/v1"
FIELDS = ("effect", "status", "policy", "scope", "edr")
F_DEBUG_CYCLES = 0x100   # cerbos_hip.h CBH_F_DEBUG_CYCLES: a launch that keeps the wide form (the cycle counts need a profiling build)


def _lower(docs):
    return lower_rule_table(rule_table_from_policies(policies_from_docs(docs)))


def _workload(name, n, seed, **kw):
    lt = _lower(getattr(workloads, name + "_policies")())
    return lt, getattr(workloads, name + "_requests")(n, seed=seed, **kw).to_batch(Flattener(lt))


def _same(capi, lt, batch, flags=None):
    """cbh_check_batch (wide) against cbh_check_resident + cbh_result_download, every field bit for bit; returns the resident plan."""
    flags = capi.F_WANT_DERIVED_ROLES if flags is None else flags
    table = capi.Table(lt.blob)
    db = table.upload(batch)
    try:
        want = table.check(batch, now_ns=NOW, flags=flags)
        table.launch(db, now_ns=NOW, flags=flags)
        have = table.download(db)
        for f in FIELDS:
            assert np.array_equal(getattr(have, f), getattr(want, f)), f
        return table.plan(db, flags=flags)
    finally:
        db.close()


def _many_scopes_store(n_scopes):
    """a flat store of `n_scopes` scoped resource policies: scope indices too wide for the packed word (CBH_PK_MAX_BITS)"""
    docs = [{"apiVersion": API, "resourcePolicy": {"resource": "doc", "version": "default", "rules": [
        {"actions": ["view"], "effect": "EFFECT_ALLOW", "roles": ["user"]}]}}]
    for i in range(n_scopes):
        docs.append({"apiVersion": API, "resourcePolicy": {"resource": "doc", "version": "default", "scope": "s%d" % i, "rules": [
            {"actions": ["edit", "view"], "effect": "EFFECT_ALLOW" if i % 3 else "EFFECT_DENY", "roles": ["user"],
             "condition": {"match": {"expr": "R.attr.amount > %d" % (i % 50)}}}]}})
    return docs


def _many_scopes_requests(n, n_scopes, seed):
    rng = np.random.default_rng(seed)
    return [{"requestId": "q%d" % i, "actions": ["view", "edit", "delete"][: 1 + i % 3],
             "principal": {"id": "p%d" % (i % 7), "roles": ["user"], "attr": {}},
             "resource": {"kind": "doc", "id": "r%d" % i, "attr": {"amount": float(rng.integers(0, 100))},
                          "scope": "s%d" % int(rng.integers(n_scopes - 64, n_scopes + 8))}} for i in range(n)]


# ---- the bodies: the same on the simulator and on the device


def check_workloads(capi, n):
    # n is not a multiple of the 256-lane workgroup: a partial last wave; C2 with three actions a request: unaligned stores
    for name, kw in (("c2", {}), ("c2", {"actions_per_request": 3}), ("c3", {}), ("t", {})):
        lt, batch = _workload(name, n, seed=11, **kw)
        assert _same(capi, lt, batch).startswith("cbh_check_flat_kernel"), name
    lt, batch = _workload("c3", n, seed=12)
    assert lt.stats["derived_roles"] and _same(capi, lt, batch, flags=0)


def check_c4(capi, n):
    lt, batch = _workload("c4", n, seed=13)
    assert _same(capi, lt, batch).startswith("cbh_check_flat_kernel")


def check_random_flat_stores(capi, seeds):
    import test_flat_kernel as tf
    for seed in seeds:
        rng = np.random.default_rng(77_000 + seed)
        lt = _lower(tf._store(rng))
        batch = Flattener(lt).flatten(tf._requests(rng, 300))
        for flags in (capi.F_WANT_DERIVED_ROLES, capi.F_WANT_DERIVED_ROLES | capi.F_LENIENT_SCOPE_SEARCH, 0):
            _same(capi, lt, batch, flags)


def check_scopes_too_wide(capi, n_scopes):
    lt = _lower(_many_scopes_store(n_scopes))
    assert lt.stats["flat"] and lt.stats["scopes"] >= 1 << 12   # (CBH_PK_MAX_BITS)
    batch = Flattener(lt).flatten(_many_scopes_requests(500, n_scopes, seed=5))
    assert _same(capi, lt, batch).startswith("cbh_check_flat_kernel")


def check_forms_switch_between_launches(capi, n):
    """a packed launch, a launch of the trail's kernel (wide), a cycle-count launch (wide), a packed one again: each download is
    the last launch's"""
    lt, batch = _workload("c2", n, seed=14)
    table = capi.Table(lt.blob)
    db = table.upload(batch)
    try:
        table.set_trail(db, None, 1)
        seq = (capi.F_WANT_DERIVED_ROLES, capi.F_WANT_DERIVED_ROLES | capi.F_WANT_EFFECTIVE_POLICIES, F_DEBUG_CYCLES,
               capi.F_WANT_DERIVED_ROLES | capi.F_LENIENT_SCOPE_SEARCH)
        for flags in seq + seq[::-1]:
            want = table.check(batch, now_ns=NOW, flags=flags & ~(capi.F_WANT_EFFECTIVE_POLICIES | F_DEBUG_CYCLES))
            table.launch(db, now_ns=NOW, flags=flags)
            for _ in range(2):   # (a second download of the same launch gives the same)
                have = table.download(db)
                for f in FIELDS:
                    assert np.array_equal(getattr(have, f), getattr(want, f)), (flags, f)
    finally:
        db.close()


# ---- CPU tier: the simulator


@pytest.fixture()
def engine():
    with sim_engine() as capi:
        yield capi


def test_workloads_on_simulator(engine):
    check_workloads(engine, 700)


def test_c4_on_simulator(engine):
    check_c4(engine, 300)


def test_random_flat_stores_on_simulator(engine):
    check_random_flat_stores(engine, range(4))


def test_scopes_too_wide_on_simulator(engine):
    check_scopes_too_wide(engine, 4200)


def test_forms_switch_on_simulator(engine):
    check_forms_switch_between_launches(engine, 500)


# ---- GPU tier


@pytest.mark.gpu
def test_workloads_on_gpu():
    from cerbos_amd import capi
    check_workloads(capi, 100_003)


@pytest.mark.gpu
def test_c4_on_gpu():
    from cerbos_amd import capi
    check_c4(capi, 50_001)


@pytest.mark.gpu
def test_random_flat_stores_on_gpu():
    from cerbos_amd import capi
    check_random_flat_stores(capi, range(12))


@pytest.mark.gpu
def test_scopes_too_wide_on_gpu():
    from cerbos_amd import capi
    check_scopes_too_wide(capi, 4200)


@pytest.mark.gpu
def test_forms_switch_on_gpu():
    from cerbos_amd import capi
    check_forms_switch_between_launches(capi, 20_001)
