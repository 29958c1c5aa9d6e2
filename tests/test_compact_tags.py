"""The tag planes of a resident batch's compact form (cbh_vm.h BatchDev.ctag) and the flat kernels' fold on wave-uniform facts.

A compact batch carries the tags of its cached columns four to a dword per request; a compact launch copies one dword per lane and
group of four columns into the column cache and reads a column's tag at a byte position that depends on the column alone.  The fold
writes the constant status for a wave in which no lane has an evaluation error, and forms the packed result words from the walk's
facts directly.  Nothing a caller sees changes: every array cbh_result_download gives is compared bit for bit with cbh_check_batch,
whose one-shot path keeps the wide arrays and the per-lane byte position of a tag; every case asserts that the resident plan really
says "[compact inputs" - a test that passes because everything fell back proves nothing.
CPU tier: the library's host side on the simulator (tests/sim_engine.py).  GPU tier: the library on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cerbos_amd.flatten import Flattener
from sim_engine import sim_engine
import test_compact_inputs as tc

API = "api.cerbos.dev/v1"
NOW = tc.NOW
COMPACT = tc.COMPACT
T_ABSENT, T_ERR = 0xF0, 0xFF   # cerbos_hip.h cbh_tag
ROOT = tc.ROOT
ROLES = ["user", "manager", "admin", "guest"]
ACTIONS = ["view", "edit", "delete", "approve"]


def _cond_on(j, n):
    """a classified condition on attribute column j of n: the five leaf classes in turn"""
    a = "R.attr.a%d" % j
    return [a + ' == "x"', a + " > 10", a + ' in ["x", "y"]', a + " == P.id", a + " != R.attr.a%d" % ((j + 1) % n)][j % 5]


def _column_store(n_cols, scopes=("",)):
    """a flat store without derived roles whose conditions name exactly the attributes a0 .. a<n_cols - 1>: that many cached columns.
    The first rule of every policy applies to every role and action, so that every request evaluates a condition."""
    docs = []
    for kind in ("doc", "report"):
        for si, scope in enumerate(scopes):
            rules = [{"actions": ["*"], "roles": ["*"], "effect": "EFFECT_ALLOW" if si % 2 == 0 else "EFFECT_DENY",
                      "condition": {"match": {"expr": _cond_on(si % n_cols, n_cols)}}}]
            for j in range(n_cols):
                rules.append({"actions": [ACTIONS[j % 4], ACTIONS[(j + si + 1) % 4]], "roles": [ROLES[(j + si) % 4], ROLES[(j + 2) % 4]],
                              "effect": "EFFECT_DENY" if (j + si) % 3 == 0 else "EFFECT_ALLOW",
                              "condition": {"match": {"expr": _cond_on(j, n_cols)}}})
            pol = {"resource": kind, "version": "default", "rules": rules}
            if scope:
                pol["scope"] = scope
                if si % 2:
                    pol["scopePermissions"] = "SCOPE_PERMISSIONS_REQUIRE_PARENTAL_CONSENT_FOR_ALLOWS"
            docs.append({"apiVersion": API, "resourcePolicy": pol})
    return docs


def _column_requests(rng, n, n_cols, scopes=("",), full=True):
    """requests that bring every attribute (a string, a double or a bool); full: four actions and one to four roles"""
    out = []
    for i in range(n):
        vals = ["x", "y", "p1", 5.0, 50.0, True]   # (the column an ordering reads holds numbers: ordering a string is a CEL error)
        attr = {"a%d" % j: vals[int(rng.integers(3, 5) if j % 5 == 1 else rng.integers(0, len(vals)))] for j in range(n_cols)}
        roles = [str(r) for r in rng.choice(ROLES, size=int(rng.integers(1 if full else 0, 5)), replace=False)]
        acts = list(ACTIONS) if full else [str(a) for a in rng.choice(ACTIONS + ["nothing"], size=int(rng.integers(0, 5)), replace=False)]
        out.append({"requestId": "q%d" % i, "actions": acts, "principal": {"id": "p%d" % rng.integers(0, 3), "roles": roles, "attr": {}},
                    "resource": {"kind": "doc" if i % 3 else "report", "id": "r%d" % i, "attr": attr, "scope": str(rng.choice(list(scopes)))}})
    return out


def _column_batch(n_cols, n, seed, scopes=("",), full=True):
    rng = np.random.default_rng(91_000 + seed)
    lt = tc._lower(_column_store(n_cols, scopes))
    batch = Flattener(lt).flatten(_column_requests(rng, n, n_cols, scopes, full))
    assert batch.col_tag.shape == (n_cols, n), batch.col_tag.shape
    return lt, batch


# ---- the bodies: the same on the simulator and on the device


def check_workloads(capi, sizes, expect_compact=True):
    """C2, C4 and T with a partial last wave and a partial last workgroup; the sizes are odd, so that the wide form's byte position of a
    tag (column * n_requests + request, mod 4) differs from column to column - the side the compact launch is compared with"""
    for n in sizes:
        assert n % 2 == 1 and n % 256 != 0
        for name in ("c2", "c4", "t"):
            lt, batch = tc._workload(name, n, seed=31)
            plan = tc._same(capi, lt, batch)
            assert plan.startswith("cbh_check_flat_kernel") and (COMPACT in plan) == expect_compact, (name, plan)


def check_column_counts(capi, n, expect_compact=True):
    """1, 4, 5, 8 and 9 cached columns: one group that is not full, a full last group, a last group of one byte, three groups.  ABSENT
    and error tags in every column - every byte position of every group - and next to lanes without them"""
    for n_cols in (1, 4, 5, 8, 9):
        lt, batch = _column_batch(n_cols, n, seed=n_cols)
        i = np.arange(n)
        for c in range(n_cols):
            batch.col_tag[c, (i + 3 * c) % 7 == 0] = T_ABSENT
            batch.col_tag[c, (i + 5 * c) % 11 == 0] = T_ERR
            assert (batch.col_tag[c] == T_ABSENT).any() and (batch.col_tag[c] == T_ERR).any() and (batch.col_tag[c] < T_ABSENT).any()
        plan = tc._same(capi, lt, batch, (capi.F_WANT_DERIVED_ROLES, 0))
        assert plan.startswith("cbh_check_flat_kernel") and (COMPACT in plan) == expect_compact, (n_cols, plan)


def check_fold_without_errors(capi, n):
    """no request has an evaluation error: every wave writes the constant status; one scope and several"""
    for scopes in (("",), ("", "acme", "acme.hr", "acme.hr.uk")):
        lt, batch = _column_batch(5, n, seed=40 + len(scopes), scopes=scopes)
        table = capi.Table(lt.blob)
        assert (table.check(batch, now_ns=NOW, flags=0).status == capi.ST_OK).all()
        assert COMPACT in tc._same(capi, lt, batch, (capi.F_WANT_DERIVED_ROLES, capi.F_LENIENT_SCOPE_SEARCH, 0))


def check_fold_one_error_lane(capi, n):
    """exactly one lane of one wave has a dropped attribute (a CEL error); its neighbours do not.  One scope and several"""
    for scopes in (("",), ("", "acme", "acme.hr")):
        lt, batch = _column_batch(5, n, seed=50 + len(scopes), scopes=scopes)
        victim = 64 * (n // 128) + 37   # the middle of a wave, not the first
        batch.col_tag[:, victim] = T_ABSENT
        table = capi.Table(lt.blob)
        want = table.check(batch, now_ns=NOW, flags=0)
        bad = np.flatnonzero(want.status != capi.ST_OK)
        # (every request has four actions: the tuples of ONE request, wherever the batch's order put it)
        assert bad.size and (want.status[bad] == capi.ST_CEL_ERROR).all() and bad.min() % 4 == 0 and bad.max() < bad.min() + 4, bad
        assert COMPACT in tc._same(capi, lt, batch, (capi.F_WANT_DERIVED_ROLES, 0))


def check_counts_and_unknowns(capi, n):
    """requests with 0 to 4 actions and 0 to 4 roles, an action no rule names, on a store of one scope and on one of several; then
    the random flat stores (unknown roles and kinds too) and the unknown strings of tests/test_compact_inputs.py on other seeds"""
    for scopes in (("",), ("", "acme", "acme.hr", "acme.hr.uk")):
        lt, batch = _column_batch(4, n, seed=60 + len(scopes), scopes=scopes, full=False)
        cnt = np.asarray(batch.req_u32).reshape(-1, n)
        assert set(np.unique(cnt[9])) == {0, 1, 2, 3, 4}   # CBH_RQ_ACT_CNT
        assert COMPACT in tc._same(capi, lt, batch, (capi.F_WANT_DERIVED_ROLES, 0))
    tc.check_random_flat_stores(capi, (20, 21, 22))
    tc.check_unknown_strings(capi)


def check_allow_bits(capi, n):
    """cbh_result_download_allow_bits after a launch of the compact kernel = the unpacked effects"""
    lt, batch = _column_batch(5, n, seed=70, scopes=("", "acme"))
    batch.col_tag[2, ::9] = T_ABSENT
    table = capi.Table(lt.blob)
    db = table.upload(batch)
    try:
        assert COMPACT in table.plan(db, flags=0)
        want = table.check(batch, now_ns=NOW, flags=0, device_order=True)
        table.launch(db, now_ns=NOW, flags=0)
        bits = table.download_allow_bits(db)   # BEFORE the download: from the packed words the launch wrote
        by = np.packbits(np.asarray(want.effect) == capi.EFFECT_ALLOW, bitorder="little")
        assert np.array_equal(bits, np.concatenate([by, np.zeros(-by.size % 8, dtype=np.uint8)]).view("<u8"))
        have = table.download(db)
        assert np.array_equal(have.effect, want.to_input_order(batch).effect)
    finally:
        db.close()


CHILD = """
import sys
sys.path.insert(0, %(tests)r)
import test_compact_tags as tt
if %(sim)r:
    from sim_engine import sim_engine
    with sim_engine() as capi:
        tt.check_workloads(capi, (%(n)d,), expect_compact=False)
        tt.check_column_counts(capi, 300, expect_compact=False)
else:
    from cerbos_amd import capi
    tt.check_workloads(capi, (%(n)d,), expect_compact=False)
    tt.check_column_counts(capi, 300, expect_compact=False)
print("wide everywhere: ok")
"""


def check_switched_off(sim, n):
    """CBH_COMPACT_INPUTS=0 is read once per process: a child.  The same bodies on the wide arrays"""
    env = dict(os.environ, CBH_COMPACT_INPUTS="0")
    r = subprocess.run([sys.executable, "-c", CHILD % {"tests": os.path.join(ROOT, "tests"), "sim": sim, "n": n}], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "wide everywhere: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def check_audit():
    """tools/audit_prologue_waits.py lists the derived-role variant and the compact instantiations by default; the compact prologue
    stays at two bulk trips (the record; the columns' and the tags' copies)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_prologue_waits.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    for k in ("cbh_check_flat_kernel_dr:", "cbh_check_flat_kernel_c:", "cbh_check_flat_kernel_masks_c:"):
        assert k in r.stdout, r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_prologue_waits.py"), "--max-bulk-trips", "2", "cbh_check_flat_kernel_c10"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- CPU tier: the simulator


@pytest.fixture()
def engine():
    with sim_engine() as capi:
        yield capi


def test_workloads_on_simulator(engine):
    check_workloads(engine, (293,))


def test_column_counts_on_simulator(engine):
    check_column_counts(engine, 333)


def test_column_width_changes_on_simulator(engine):
    tc.check_column_width_changes(engine)


def test_fold_without_errors_on_simulator(engine):
    check_fold_without_errors(engine, 300)


def test_fold_one_error_lane_on_simulator(engine):
    check_fold_one_error_lane(engine, 300)


def test_counts_and_unknowns_on_simulator(engine):
    check_counts_and_unknowns(engine, 300)


def test_int_values_on_simulator(engine):
    tc.check_int_uint_values(engine)


def test_strict_and_default_alternate_on_simulator(engine):
    tc.check_strict_and_default_alternate(engine, 293)


def test_allow_bits_on_simulator(engine):
    check_allow_bits(engine, 300)


def test_switched_off_on_simulator():
    check_switched_off(True, 293)


def test_compact_prologue_has_two_bulk_trips():
    check_audit()


# ---- GPU tier


@pytest.mark.gpu
def test_workloads_on_gpu():
    from cerbos_amd import capi
    check_workloads(capi, (1037,))


@pytest.mark.gpu
def test_column_counts_on_gpu():
    from cerbos_amd import capi
    check_column_counts(capi, 1037)


@pytest.mark.gpu
def test_column_width_changes_on_gpu():
    from cerbos_amd import capi
    tc.check_column_width_changes(capi)


@pytest.mark.gpu
def test_fold_without_errors_on_gpu():
    from cerbos_amd import capi
    check_fold_without_errors(capi, 1037)


@pytest.mark.gpu
def test_fold_one_error_lane_on_gpu():
    from cerbos_amd import capi
    check_fold_one_error_lane(capi, 1037)


@pytest.mark.gpu
def test_counts_and_unknowns_on_gpu():
    from cerbos_amd import capi
    check_counts_and_unknowns(capi, 1037)


@pytest.mark.gpu
def test_int_values_on_gpu():
    from cerbos_amd import capi
    tc.check_int_uint_values(capi)


@pytest.mark.gpu
def test_strict_and_default_alternate_on_gpu():
    from cerbos_amd import capi
    tc.check_strict_and_default_alternate(capi, 1037)


@pytest.mark.gpu
def test_allow_bits_on_gpu():
    from cerbos_amd import capi
    check_allow_bits(capi, 1037)


@pytest.mark.gpu
def test_switched_off_on_gpu():
    check_switched_off(False, 1037)
