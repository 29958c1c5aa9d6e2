"""The resident path's compact input form (cbh_vm.h BatchDev.creq / cval): when a batch the flat kernels can decide is uploaded, the
device derives a 16-byte record per request (principal, kind, version, scope, counts and the action / role CLASSES) and a 32-bit
plane for every cached column whose high words are all zero; the flat kernels' compact instantiations read those instead of the
request words, the role and action ids and the 64-bit planes.  Nothing a caller sees changes: every array cbh_result_download gives
is compared bit for bit with cbh_check_batch, whose one-shot path keeps the wide form - on the benchmark's flat tables, random flat
stores (zero to four actions and roles: the record's counts, unaligned action offsets), unknown action / role / kind, a column that
is wide in one batch and narrow in the next, int / uint values (the variant with the evaluator call, which ignores the form), ids
that do not fit the record (the wide form), launches that alternate between strict and default mode, and CBH_COMPACT_INPUTS=0.
CPU tier: the library's host side on the simulator (tests/sim_engine.py).  GPU tier: the library on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cerbos_amd import workloads
from cerbos_amd.flatten import Flattener
from cerbos_amd.lower.blob import lower_rule_table
from cerbos_amd.policy.loader import policies_from_docs
from cerbos_amd.ruletable.build import rule_table_from_policies
from sim_engine import sim_engine

NOW = 1_700_000_000_000_000_000
FIELDS = ("effect", "status", "policy", "scope", "edr")
COMPACT = "[compact inputs"
T_INT, T_UINT, T_DOUBLE = 2, 3, 4   # cerbos_hip.h cbh_tag
RQ_KIND = 3                         # cerbos_hip.h CBH_RQ_KIND
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lower(docs):
    return lower_rule_table(rule_table_from_policies(policies_from_docs(docs)))


def _workload(name, n, seed, **kw):
    lt = _lower(getattr(workloads, name + "_policies")())
    return lt, getattr(workloads, name + "_requests")(n, seed=seed, **kw).to_batch(Flattener(lt))


def _same(capi, lt, batch, flag_seq=None):
    """cbh_check_batch (wide) against cbh_check_resident + cbh_result_download on ONE resident batch, for every flags word of
    `flag_seq` in turn, every field bit for bit; returns the resident plan of the first."""
    flag_seq = (capi.F_WANT_DERIVED_ROLES,) if flag_seq is None else flag_seq
    table = capi.Table(lt.blob)
    db = table.upload(batch)
    try:
        for flags in flag_seq:
            want = table.check(batch, now_ns=NOW, flags=flags)
            table.launch(db, now_ns=NOW, flags=flags)
            have = table.download(db)
            for f in FIELDS:
                assert np.array_equal(getattr(have, f), getattr(want, f)), (flags, f)
        return table.plan(db, flags=flag_seq[0])
    finally:
        db.close()


def _narrow(plan):
    """the mask of 32-bit planes the plan's description names"""
    return int(plan.split("narrow columns 0x")[1].split("]")[0], 16)


def _flat_store(seed, derived_roles=None):
    """a random flat store (tests/test_flat_kernel.py); derived_roles False: one without derived roles - the plain flat kernel, which
    has a compact instantiation (the derived-role variant has none)"""
    import test_flat_kernel as tf
    for attempt in range(64):
        rng = np.random.default_rng(88_000 + seed + 1000 * attempt)
        lt = _lower(tf._store(rng))
        if derived_roles is None or bool(lt.stats["derived_roles"]) == derived_roles:
            return tf, rng, lt
    raise AssertionError("no such store in 64 draws")


# ---- the bodies: the same on the simulator and on the device


def check_workloads(capi, n, expect_compact=True):
    # n is not a multiple of the 256-lane workgroup: a partial last wave
    for name in ("c2", "c3", "c4", "t"):
        lt, batch = _workload(name, n, seed=21)
        plan = _same(capi, lt, batch)
        assert plan.startswith("cbh_check_flat_kernel"), (name, plan)
        # a test that passes because everything fell back proves nothing
        # (C3's kernel, the derived-role variant, has no compact instantiation: it reads the wide arrays of a compact batch)
        assert (COMPACT in plan) == (expect_compact and name != "c3"), (name, plan)
    if expect_compact:
        lt, batch = _workload("c2", n, seed=22)
        plan = _same(capi, lt, batch, (0,))
        assert _narrow(plan) != 0, plan   # C2's string and bool columns have 32-bit planes
    # C2 with three actions a request: counts below four, offsets that are not 4 * request
    lt, batch = _workload("c2", n, seed=23, actions_per_request=3)
    assert (COMPACT in _same(capi, lt, batch)) == expect_compact


def check_random_flat_stores(capi, seeds, expect_compact=True):
    """requests of zero to four actions and zero to four roles, with actions, roles and kinds no rule names"""
    for seed in seeds:
        tf, rng, lt = _flat_store(seed, derived_roles=seed % 4 == 3)   # three in four: the plain flat kernel
        batch = Flattener(lt).flatten(tf._requests(rng, 300))
        plan = _same(capi, lt, batch, (capi.F_WANT_DERIVED_ROLES, capi.F_WANT_DERIVED_ROLES | capi.F_LENIENT_SCOPE_SEARCH, 0))
        assert (COMPACT in plan) == (expect_compact and seed % 4 != 3), plan


def check_unknown_strings(capi):
    """an action, a role and a kind the table does not know (class 31; their ids lie beyond the table's strings), each alone and together"""
    tf, rng, lt = _flat_store(100, derived_roles=False)
    reqs = tf._requests(rng, 64)
    for i, r in enumerate(reqs):
        r["actions"] = ["view", "nothing-%d" % i, "edit", "never"][: 1 + i % 4] if i % 2 else ["nothing-%d" % i]
        r["principal"]["roles"] = ["stranger-%d" % i] + (["user"] if i % 3 == 0 else [])
        if i % 5 == 0:
            r["resource"]["kind"] = "unheard-of-%d" % i
    assert COMPACT in _same(capi, lt, Flattener(lt).flatten(reqs), (capi.F_WANT_DERIVED_ROLES, 0))


def check_column_width_changes(capi):
    """one column across three batches of one table: strings mixed with doubles (a 64-bit plane), doubles that are all 0.0 (a 32-bit
    plane), doubles again"""
    tf, rng, lt = _flat_store(101, derived_roles=False)
    masks = []
    for how in ("mixed", "zero", "doubles"):
        reqs = tf._requests(rng, 200)
        for i, r in enumerate(reqs):
            r["resource"]["attr"]["amount"] = {"mixed": "many" if i % 3 else float(i), "zero": 0.0, "doubles": float(i) + 0.5}[how]
        plan = _same(capi, lt, Flattener(lt).flatten(reqs))
        assert COMPACT in plan, plan
        masks.append(_narrow(plan))
    assert masks[0] == masks[2] and masks[1] != masks[0] and (masks[1] & masks[0]) == masks[0], masks   # all 0.0: one more 32-bit plane


def check_int_uint_values(capi):
    """int and uint attribute values: the variant with the evaluator call decides the batch, from the wide form"""
    tf, rng, lt = _flat_store(102, derived_roles=False)
    batch = Flattener(lt).flatten(tf._requests(rng, 300))
    tag, val = batch.col_tag.reshape(-1), batch.col_val.reshape(-1)
    dbl = np.flatnonzero(tag == T_DOUBLE)
    assert dbl.size > 50
    ints = val[dbl].view(np.float64).astype(np.int64)
    tag[dbl] = np.where(np.arange(dbl.size) % 2 == 0, T_INT, T_UINT).astype(tag.dtype)
    val[dbl] = ints.view(np.uint64)
    plan = _same(capi, lt, batch, (capi.F_WANT_DERIVED_ROLES, 0))
    assert "_any" in plan and COMPACT not in plan, plan


def check_ids_too_wide(capi):
    """a kind id of 2^16 or more does not fit the record: the batch keeps the wide form, and still agrees"""
    tf, rng, lt = _flat_store(103, derived_roles=False)
    batch = Flattener(lt).flatten(tf._requests(rng, 300))
    kinds = batch.req_u32.reshape(-1)[RQ_KIND * batch.n_requests:(RQ_KIND + 1) * batch.n_requests]
    kinds[7] = 70_000      # (no such string anywhere: no policy for that request, on either path)
    kinds[130] = 1 << 16
    plan = _same(capi, lt, batch, (capi.F_WANT_DERIVED_ROLES, 0))
    assert plan.startswith("cbh_check_flat_kernel") and COMPACT not in plan, plan


def check_strict_and_default_alternate(capi, n):
    """strict mode is not a flat launch: it reads the wide arrays of the same resident batch"""
    lt, batch = _workload("c2", n, seed=24)
    d, s = capi.F_WANT_DERIVED_ROLES, capi.F_WANT_DERIVED_ROLES | capi.F_STRICT_EVALUATION
    assert COMPACT in _same(capi, lt, batch, (d, s, d | capi.F_LENIENT_SCOPE_SEARCH, s, d))
    tf, rng, lt = _flat_store(104, derived_roles=False)
    _same(capi, lt, Flattener(lt).flatten(tf._requests(rng, 300)), (s, d, s, 0))


CHILD = """
import sys
sys.path.insert(0, %(tests)r)
import test_compact_inputs as tc
if %(sim)r:
    from sim_engine import sim_engine
    with sim_engine() as capi:
        tc.check_workloads(capi, %(n)d, expect_compact=False)
        tc.check_random_flat_stores(capi, range(2), expect_compact=False)
else:
    from cerbos_amd import capi
    tc.check_workloads(capi, %(n)d, expect_compact=False)
    tc.check_random_flat_stores(capi, range(2), expect_compact=False)
print("wide everywhere: ok")
"""


def check_switched_off(sim, n):
    """CBH_COMPACT_INPUTS=0 is read once per process: a child"""
    env = dict(os.environ, CBH_COMPACT_INPUTS="0")
    r = subprocess.run([sys.executable, "-c", CHILD % {"tests": os.path.join(ROOT, "tests"), "sim": sim, "n": n}], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "wide everywhere: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def check_audit_lists_dr():
    """tools/audit_prologue_waits.py reads the derived-role variant and the compact instantiations by default; no prologue has
    more than three bulk trips"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_prologue_waits.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    for k in ("cbh_check_flat_kernel:", "cbh_check_flat_kernel_dr:", "cbh_check_flat_kernel_c:", "cbh_check_flat_kernel_masks_c:"):
        assert k in r.stdout, r.stdout


# ---- CPU tier: the simulator


@pytest.fixture()
def engine():
    with sim_engine() as capi:
        yield capi


def test_workloads_on_simulator(engine):
    check_workloads(engine, 700)


def test_random_flat_stores_on_simulator(engine):
    check_random_flat_stores(engine, range(4))


def test_unknown_strings_on_simulator(engine):
    check_unknown_strings(engine)


def test_column_width_changes_on_simulator(engine):
    check_column_width_changes(engine)


def test_int_uint_values_on_simulator(engine):
    check_int_uint_values(engine)


def test_ids_too_wide_on_simulator(engine):
    check_ids_too_wide(engine)


def test_strict_and_default_alternate_on_simulator(engine):
    check_strict_and_default_alternate(engine, 500)


def test_switched_off_on_simulator():
    check_switched_off(True, 300)


def test_prologue_audit_lists_the_shared_prologues():
    check_audit_lists_dr()


# ---- GPU tier


@pytest.mark.gpu
def test_workloads_on_gpu():
    from cerbos_amd import capi
    check_workloads(capi, 100_003)


@pytest.mark.gpu
def test_random_flat_stores_on_gpu():
    from cerbos_amd import capi
    check_random_flat_stores(capi, range(12))


@pytest.mark.gpu
def test_unknown_strings_on_gpu():
    from cerbos_amd import capi
    check_unknown_strings(capi)


@pytest.mark.gpu
def test_column_width_changes_on_gpu():
    from cerbos_amd import capi
    check_column_width_changes(capi)


@pytest.mark.gpu
def test_int_uint_values_on_gpu():
    from cerbos_amd import capi
    check_int_uint_values(capi)


@pytest.mark.gpu
def test_ids_too_wide_on_gpu():
    from cerbos_amd import capi
    check_ids_too_wide(capi)


@pytest.mark.gpu
def test_strict_and_default_alternate_on_gpu():
    from cerbos_amd import capi
    check_strict_and_default_alternate(capi, 20_001)


@pytest.mark.gpu
def test_switched_off_on_gpu():
    check_switched_off(False, 20_001)
