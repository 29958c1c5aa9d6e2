"""Cross-product batches built ON THE DEVICE (cerbos_hip.h cbh_batch_upload_cross, cerbos_amd/csrc/cbh_cross.h) and the allow
bitmap (cbh_result_download_allow_bits).

The N + M halves go up, the device expands them into an ordinary resident batch, the existing kernels decide it.  What is asserted:
every array cbh_result_download gives for the device-built product equals, bit for bit, what it gives for the host-built product
(cerbos_amd.cross.cross_product_batch + cbh_batch_upload) of the same principals, resources, actions and aux data, AND the two
batches get the same plan (cbh_plan_describe) - so the product really runs on the flat / compact / walk kernels the host-built
batch runs on; the results against oracle/ccheck and against explicit CheckInputs; the bitmap against the downloaded effects after
packed and after wide launches; every refusal the header lists; failing allocations and copies (simulator only).
CPU tier: the library's host side on the simulator (tests/sim_engine.py).  GPU tier: the library on the device."""
import os

import numpy as np
import pytest

from cerbos_amd import workloads
from cerbos_amd.cross import allow_cube, cross_halves, cross_product_batch, cross_product_upload, effect_cube, result_cubes, upload_halves
from cerbos_amd.flatten import Flattener
from cerbos_amd.lower.blob import lower_rule_table
from cerbos_amd.lower.celc import LoweringError
from cerbos_amd.policy.loader import policies_from_docs
from cerbos_amd.ruletable.build import rule_table_from_policies
from sim_engine import sim_engine

NOW = 1_700_000_000_000_000_000
FIELDS = ("effect", "status", "policy", "scope", "edr")
COMPACT = "[compact inputs"
ALLOW = 1          # cerbos_hip.h CBH_EFFECT_ALLOW
MAX_ACTIONS = 64   # cerbos_hip.h CBH_MAX_ACTIONS_PER_REQUEST


def _lower(docs, **kw):
    return lower_rule_table(rule_table_from_policies(policies_from_docs(docs)), **kw)


def _mode_flags(capi):
    return (capi.F_WANT_DERIVED_ROLES, capi.F_WANT_DERIVED_ROLES | capi.F_LENIENT_SCOPE_SEARCH, capi.F_STRICT_EVALUATION)


def _halves_of(name, n, m, seed):
    """n principals (with their aux data) and m resources of a workload, and its four actions"""
    ins = getattr(workloads, name + "_requests")(n + m, seed=seed).to_inputs()
    return [i["principal"] for i in ins[:n]], [i["resource"] for i in ins[n:]], list(ins[0]["actions"]), [i.get("auxData") for i in ins[:n]]


def _bits_of(effect):
    """the bitmap the header defines, from downloaded effects"""
    by = np.packbits(np.asarray(effect) == ALLOW, bitorder="little")
    return np.concatenate([by, np.zeros(-by.size % 8, dtype=np.uint8)]).view("<u8")


def _same(capi, lt, principals, resources, actions, aux=None, sort=True, flag_seq=None, flattener=None, orders=None, table=None):
    """The host-built product uploaded against the device-built one, on one table: every field of cbh_result_download bit for bit
    under every flags word of `flag_seq`, the same plan, and the allow bitmap of the device-built batch.  `orders` = (p_order,
    r_order): the device-built product laid out in THOSE orders, compared through the cubes.  Returns the first plan."""
    flag_seq = _mode_flags(capi) if flag_seq is None else flag_seq
    fl = flattener or Flattener(lt)
    own = table is None
    table = table or capi.Table(lt.blob)
    cb = cross_product_batch(fl, lt.columns, principals, resources, actions, aux, sort=sort)
    hb = table.upload(cb)
    if orders is None:
        db = cross_product_upload(table, fl, lt.columns, principals, resources, actions, aux, sort=sort)
    else:
        h, _, _, act = cross_halves(fl, principals, resources, actions, aux, "default", "", False)
        db = upload_halves(table, h, len(principals), len(resources), act, orders[0], orders[1])
    try:
        assert db.n_requests == cb.n_requests and db.n_tuples == cb.n_tuples and db.shape == cb.shape
        plans = []
        for flags in flag_seq:
            assert table.plan(db, flags=flags) == table.plan(hb, flags=flags), flags
            plans.append(table.plan(db, flags=flags))
            table.launch(hb, now_ns=NOW, flags=flags)
            table.launch(db, now_ns=NOW, flags=flags)
            bits = table.download_allow_bits(db)      # BEFORE the download: from whichever form the launch wrote
            want, have = table.download(hb), table.download(db)
            if orders is None:
                for f in FIELDS:
                    assert np.array_equal(getattr(have, f), getattr(want, f)), (flags, f)
            else:
                (cw, ew), (ch, eh) = result_cubes(cb, want), result_cubes(db, have)
                for f in ("effect", "status", "policy", "scope"):
                    assert np.array_equal(ch[f], cw[f]), (flags, f)
                assert np.array_equal(eh, ew), flags
            assert np.array_equal(bits, _bits_of(have.effect)), flags
            assert np.array_equal(allow_cube(db, bits), effect_cube(db, have) == ALLOW)
        return plans[0]
    finally:
        db.close()
        hb.close()
        if own:
            table.close()


# ---- the bodies: the same on the simulator and on the device


def check_workloads(capi, n, m):
    """C2, C3, C4, T (flat tables: the compact records and planes for C2 and T) and C5 (the walk, aux data free)"""
    for name in ("c2", "c3", "c4", "t", "c5"):
        lt = _lower(getattr(workloads, name + "_policies")())
        p, r, a, aux = _halves_of(name, n, m, seed=31)
        plan = _same(capi, lt, p, r, a, aux)
        if name in ("c2", "t"):     # a test that passes because something fell back proves nothing
            assert plan.startswith("cbh_check_flat_kernel") and COMPACT in plan, (name, plan)
        if name == "c5":
            assert "cbh_walk2_kernel" in plan, plan


def check_fuzz_stores(capi, seeds, n, m):
    """the fuzzed stores of tests/test_fuzz_parity.py: scopes, derived roles, principal and role policies, JWT aux data per
    principal - the walk and the general kernels; one to five actions and twelve; a principal without roles, one with six roles
    among four-role ones; sorted and unsorted"""
    import test_fuzz_parity as tf
    done = 0
    for seed in seeds:
        rng = np.random.default_rng(52_000 + seed)
        try:
            lt = _lower(tf._policies(rng))
        except LoweringError:
            continue
        sample = tf._requests(rng, n + m)
        principals, resources = [s["principal"] for s in sample[:n]], [s["resource"] for s in sample[n:]]
        aux = [s.get("auxData") for s in sample[:n]]
        principals[0]["roles"] = []
        for k in range(1, min(n, 6)):
            principals[k]["roles"] = tf.ROLES[:4]
        if n > 2:
            principals[2]["roles"] = tf.ROLES + ["other"]      # six roles
        n_act = (1, 2, 3, 4, 5, 12)[seed % 6]
        actions = (tf.ACTIONS + ["act%d" % k for k in range(8)])[:n_act]
        _same(capi, lt, principals, resources, actions, aux, sort=seed % 2 == 0)
        done += 1
    assert done >= max(1, len(list(seeds)) // 2), done


def check_shapes(capi):
    """N and M that are no multiples of 64, N below 64 (a wave spans several resources), N = 1, M = 1, A = 1 .. 5 and 9,
    unsorted, explicit orders that are not the identity"""
    lt = _lower(workloads.c2_policies())
    table = capi.Table(lt.blob)
    rng = np.random.default_rng(7)
    try:
        for n, m, a, sort in ((1, 50, 4, True), (50, 1, 4, True), (1, 1, 1, True), (5, 70, 2, True), (70, 3, 3, False), (67, 13, 5, True),
                              (13, 9, 9, True), (130, 5, 1, False)):
            p, r, acts, aux = _halves_of("c2", n, m, seed=40 + n)
            acts = (acts + ["extra%d" % k for k in range(8)])[:a]
            plan = _same(capi, lt, p, r, acts, aux, sort=sort, table=table, flag_seq=(0, capi.F_STRICT_EVALUATION))
            assert (COMPACT in plan) == (a <= 4), (n, m, a, plan)
        p, r, acts, aux = _halves_of("c2", 37, 21, seed=77)
        _same(capi, lt, p, r, acts, aux, table=table, orders=(rng.permutation(37), rng.permutation(21)), flag_seq=(0,))
        _same(capi, lt, p, r, acts, aux, table=table, orders=(np.arange(37)[::-1], None), flag_seq=(0,))
    finally:
        table.close()


def check_wide_walk(capi, n, m):
    """C5 with four-role principals and ONE of six roles: the walk's wider shape decides [wide_lo, wide_hi), which the host derives
    from the halves"""
    lt = _lower(workloads.c5_policies())
    ins = workloads.c5_requests(n + m, seed=11, roles_per_request=(4, 4)).to_inputs()
    principals, resources = [i["principal"] for i in ins[:n]], [i["resource"] for i in ins[n:]]
    principals[n // 3]["roles"] = list(principals[n // 3]["roles"]) + ["contractor", "auditor"]
    for sort in (True, False):
        plan = _same(capi, lt, principals, resources, ins[0]["actions"], sort=sort)
        assert "5-8 roles" in plan, plan
    plan = _same(capi, lt, principals, resources, ins[0]["actions"] + ["a%d" % k for k in range(6)], flag_seq=(capi.F_WANT_DERIVED_ROLES,))
    assert "9-16 actions" in plan or "wide requests" in plan, plan


class _WithGlobals:
    """a flattener that brings the CALL's globals (they travel with the principal half)"""

    def __init__(self, lt, g):
        self.fl, self.g = Flattener(lt), g

    def flatten(self, inputs, default_policy_version="default", default_scope="", sort=True):
        return self.fl.flatten(inputs, default_policy_version, default_scope, sort=sort, globals_=self.g)


def check_per_call_globals(capi):
    """a table lowered with per_call_globals=True: the columns of root G come from the principal half"""
    from helpers import load_json, store_rule_table
    lt = lower_rule_table(store_rule_table(), per_call_globals=True)
    assert any(root == "G" for root, _ in lt.columns)
    vectors = load_json("verify_vectors.json")
    with_g = [v for v in vectors if v["globals"]]
    assert with_g
    ins = [v["input"] for v in with_g] + [v["input"] for v in vectors if not v["globals"]][:40]
    principals, resources = [i["principal"] for i in ins[:23]], [i["resource"] for i in ins]
    aux = [i.get("auxData") for i in ins[:23]]
    actions = (list(with_g[0]["input"]["actions"]) + sorted({a for i in ins for a in i["actions"]} - set(with_g[0]["input"]["actions"])))[:5]
    for g in (with_g[0]["globals"], {}):
        _same(capi, lt, principals, resources, actions, aux, flattener=_WithGlobals(lt, g))


def check_against_oracle(capi, fuzz_nm, c3_nm):
    """the device-built product against oracle/ccheck run on the host-built batch, and a corner of the cube against explicit
    CheckInputs through Table.check"""
    import test_fuzz_parity as tf
    from oracle import ccheck
    flags = capi.F_WANT_DERIVED_ROLES
    rng = np.random.default_rng(61_000)
    lt_f = _lower(tf._policies(rng, wide=False))
    sample = tf._requests(rng, sum(fuzz_nm), wide=False)
    fuzz = ([s["principal"] for s in sample[:fuzz_nm[0]]], [s["resource"] for s in sample[fuzz_nm[0]:]], tf.ACTIONS[:4], None)
    for lt, (principals, resources, actions, aux), (n, m) in ((lt_f, fuzz, fuzz_nm), (_lower(workloads.c3_policies()), _halves_of("c3", *c3_nm, seed=9), c3_nm)):
        table = capi.Table(lt.blob)
        cb = cross_product_batch(Flattener(lt), lt.columns, principals, resources, actions, aux)
        db = cross_product_upload(table, Flattener(lt), lt.columns, principals, resources, actions, aux)
        try:
            table.launch(db, now_ns=NOW, flags=flags)
            got = table.download(db)
            want = ccheck.check(lt, cb, NOW, flags, threads=min(16, os.cpu_count() or 1))
            a = len(actions)
            ok = ~(want.status == capi.ST_UNSUPPORTED).reshape(-1, a).any(axis=1)      # requests the C++ restatement covers
            assert ok.mean() > 0.5, ok.mean()
            okt = np.repeat(ok, a)
            for f in ("effect", "policy", "scope"):
                assert np.array_equal(getattr(got, f)[okt], getattr(want, f)[okt]), f
            assert np.array_equal(got.edr[ok], want.edr[ok])
            assert np.array_equal((got.status == capi.ST_CEL_ERROR).reshape(-1, a).any(axis=1)[ok], (want.status == capi.ST_CEL_ERROR).reshape(-1, a).any(axis=1)[ok])
            cn, cm = min(20, n), min(15, m)
            explicit = [{"principal": p, "resource": r, "actions": actions} for p in principals[:cn] for r in resources[:cm]]
            eff = table.check(Flattener(lt).flatten(explicit), now_ns=NOW, flags=flags).effect
            assert np.array_equal(effect_cube(db, got)[:cn, :cm].reshape(-1), eff)
            assert np.array_equal(allow_cube(db, table.download_allow_bits(db))[:cn, :cm].reshape(-1), eff == ALLOW)
        finally:
            db.close()
            table.close()


def check_allow_bits(capi, n):
    """after a flat resident launch (packed results), after a strict launch (wide results), on a walk table, with a tuple count
    that is no multiple of 64, on an ordinary uploaded batch; the full results are still there afterwards; a short buffer is
    refused and left untouched"""
    for name, apr in (("c2", 3), ("c2", 4), ("c5", 4)):
        lt = _lower(getattr(workloads, name + "_policies")())
        kw = {"actions_per_request": apr}
        batch = getattr(workloads, name + "_requests")(n, seed=5, **kw).to_batch(Flattener(lt))
        assert batch.n_tuples == n * apr and (apr != 3 or batch.n_tuples % 64 != 0)
        table = capi.Table(lt.blob)
        db = table.upload(batch)
        try:
            for flags in (0, capi.F_STRICT_EVALUATION, capi.F_WANT_DERIVED_ROLES):
                plan = table.plan(db, flags=flags)
                # the flat kernels write packed result words on the resident path where the table's ids fit (C2's do): the bitmap
                # is read from those; a strict launch and the walk write the wide arrays
                assert plan.startswith("cbh_check_flat_kernel") == (name == "c2" and not flags & capi.F_STRICT_EVALUATION), (name, flags, plan)
                want = table.check(batch, now_ns=NOW, flags=flags, device_order=True)
                want_bits = _bits_of(want.effect)                                   # (the bitmap is in device order)
                want = want.to_input_order(batch)
                table.launch(db, now_ns=NOW, flags=flags)
                words = (batch.n_tuples + 63) // 64
                short = np.full(words - 1, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
                with pytest.raises(capi.HipEngineError) as e:
                    table.download_allow_bits(db, into=short)
                assert str(e.value) and (short == 0x5A5A5A5A5A5A5A5A).all()
                longer = np.full(words + 2, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
                bits = table.download_allow_bits(db, into=longer)
                assert bits.size == words and np.array_equal(bits, want_bits), (name, flags)
                assert (longer[words:] == 0x5A5A5A5A5A5A5A5A).all()
                assert np.array_equal(table.download_allow_bits(db), bits)          # twice: nothing was consumed
                have = table.download(db)                                           # the full results are still there
                for f in ("effect", "status", "policy", "scope"):
                    assert np.array_equal(getattr(have, f), getattr(want, f)), (name, flags, f)
                assert np.array_equal(table.download_allow_bits(db), bits)          # ... and from the wide form now
        finally:
            db.close()
            table.close()


def check_refusals(capi):
    """every case of the header's "Refused" list: < 0 with a text, and a valid call on the same table afterwards succeeds"""
    import ctypes as C
    lt = _lower(workloads.c2_policies())
    table = capi.Table(lt.blob)
    p, r, acts, aux = _halves_of("c2", 6, 5, seed=3)
    h, po, ro, act = cross_halves(Flattener(lt), p, r, acts, aux, "default", "", True)
    lib = capi.load()

    def raw(n=6, m=5, a=None, halves=h, p_order=po, r_order=ro, device=0, null=None):
        a_ids = np.ascontiguousarray(act if a is None else np.resize(act, a), dtype=np.uint32)
        pa = None if p_order is None else np.ascontiguousarray(p_order, dtype=np.uint32)
        ra = None if r_order is None else np.ascontiguousarray(r_order, dtype=np.uint32)
        cb = capi.make_cbatch(halves, table.num_columns)
        x = capi.CCross(n, m, a_ids.size, a_ids.ctypes.data if a_ids.size else None, pa.ctypes.data if pa is not None else None,
                        ra.ctypes.data if ra is not None else None)
        if null == "actions":
            x.action_ids = None
        out = C.c_void_p()
        rc = lib.cbh_batch_upload_cross(None if null == "table" else table.h, device, None if null == "halves" else C.byref(cb),
                                        None if null == "cross" else C.byref(x), None if null == "out" else C.byref(out))
        return rc, out

    def refused(**kw):
        rc, out = raw(**kw)
        assert rc < 0 and not out.value, kw
        assert lib.cbh_last_error(), kw
        rc, out = raw()                         # ... and the table still serves
        assert rc == 0 and out.value
        lib.cbh_batch_release(out)

    for what in ("table", "halves", "cross", "out", "actions"):
        refused(null=what)
    refused(n=5)                                # n_requests != N + M
    refused(n=0, m=11, p_order=None)
    refused(n=11, m=0, r_order=None)
    refused(a=0)
    refused(a=MAX_ACTIONS + 1)
    refused(device=capi.num_devices())
    refused(p_order=[0, 1, 2, 3, 4, 4])         # not a permutation: a repeat, an entry out of range
    refused(p_order=[0, 1, 2, 3, 4, 6])
    refused(r_order=[1, 1, 2, 3, 4])
    # N * M and N * M * A of 2^32 or more: refused from the counts (the halves' arrays are sized for n_requests, which is checked first)
    big = capi.make_cbatch(h, table.num_columns)
    for n, m, a in ((1 << 16, 1 << 16, 1), (1 << 16, (1 << 16) - 1, 2), (1 << 20, 1 << 10, 4)):
        big.n_requests = n + m
        a_ids = np.resize(act, a).astype(np.uint32)
        x = capi.CCross(n, m, a, a_ids.ctypes.data, None, None)
        out = C.c_void_p()
        assert lib.cbh_batch_upload_cross(table.h, 0, C.byref(big), C.byref(x), C.byref(out)) < 0 and not out.value
        assert b"2^32" in lib.cbh_last_error()
    # the bitmap's own refusals
    db = upload_halves(table, h, 6, 5, act, po, ro)
    table.launch(db, now_ns=NOW)
    assert lib.cbh_result_download_allow_bits(table.h, db.h, None, 100) < 0 and lib.cbh_last_error()
    assert lib.cbh_result_download_allow_bits(table.h, None, np.zeros(4, np.uint64).ctypes.data, 4) < 0
    assert table.download_allow_bits(db).size == (6 * 5 * len(act) + 63) // 64
    db.close()
    table.close()


# ---- CPU tier: the simulator


@pytest.fixture()
def engine():
    with sim_engine() as capi:
        yield capi


def test_workloads_on_simulator(engine):
    check_workloads(engine, 37, 23)


def test_fuzz_stores_on_simulator(engine):
    check_fuzz_stores(engine, range(6), 19, 14)


def test_shapes_on_simulator(engine):
    check_shapes(engine)


def test_wide_walk_on_simulator(engine):
    check_wide_walk(engine, 21, 17)


def test_per_call_globals_on_simulator(engine):
    check_per_call_globals(engine)


def test_against_oracle_on_simulator(engine):
    check_against_oracle(engine, (23, 31), (40, 30))


def test_allow_bits_on_simulator(engine):
    check_allow_bits(engine, 333)


def test_refusals_on_simulator(engine):
    check_refusals(engine)


def test_failing_allocations_and_copies_are_survived():
    """Fault injection (simulator only): the k-th device allocation - or asynchronous copy - from now on fails, for every k until the
    call succeeds; upload_cross either reports an error with a text or returns a batch that decides correctly, and the table can
    be released afterwards."""
    import test_sim_engine as ts
    ts._in_own_process('''
import ctypes as C
import numpy as np
from cerbos_amd import workloads
from cerbos_amd.cross import cross_halves, cross_product_batch, upload_halves
from cerbos_amd.flatten import Flattener
import test_cross_device as tc
NOW = tc.NOW
lib = capi.load()
lib.cbh_sim_set_alloc_budget.argtypes = [C.c_long]
lib.cbh_sim_set_copy_budget.argtypes = [C.c_long]
for name in ("c2", "c5"):
    lt = tc._lower(getattr(workloads, name + "_policies")())
    p, r, acts, aux = tc._halves_of(name, 9, 7, seed=4)
    fl = Flattener(lt)
    ref = capi.Table(lt.blob)
    want = ref.check(cross_product_batch(fl, lt.columns, p, r, acts, aux), now_ns=NOW, flags=0, device_order=True)
    h, po, ro, act = cross_halves(fl, p, r, acts, aux, "default", "", True)
    for setter in (lib.cbh_sim_set_alloc_budget, lib.cbh_sim_set_copy_budget):
        failed = 0
        for k in range(200):
            table = capi.Table(lt.blob)          # (a fresh table: empty pools, every buffer a real allocation)
            setter(k)
            db = None
            try:
                db = upload_halves(table, h, 9, 7, act, po, ro)
            except capi.HipEngineError as e:
                assert str(e), "an error without a message"
                failed += 1
            finally:
                setter(-1)
            if db is None:                        # allowed again: as if nothing had happened
                db = upload_halves(table, h, 9, 7, act, po, ro)
            table.launch(db, now_ns=NOW, flags=0)
            got = table.download(db)
            assert np.array_equal(got.effect, want.effect) and np.array_equal(got.policy, want.policy)
            assert np.array_equal(table.download_allow_bits(db), tc._bits_of(want.effect))
            db.close()
            table.close()
            if failed == k:                       # the k-th was not reached: the call had enough
                break
        assert failed >= 10 and failed == k, (name, failed, k)
    ref.close()
''', {})


# ---- GPU tier


@pytest.mark.gpu
def test_workloads_on_gpu():
    from cerbos_amd import capi
    check_workloads(capi, 203, 131)


@pytest.mark.gpu
def test_fuzz_stores_on_gpu():
    from cerbos_amd import capi
    check_fuzz_stores(capi, range(12), 45, 37)


@pytest.mark.gpu
def test_shapes_on_gpu():
    from cerbos_amd import capi
    check_shapes(capi)


@pytest.mark.gpu
def test_wide_walk_on_gpu():
    from cerbos_amd import capi
    check_wide_walk(capi, 150, 70)


@pytest.mark.gpu
def test_per_call_globals_on_gpu():
    from cerbos_amd import capi
    check_per_call_globals(capi)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_against_oracle_on_gpu():
    from cerbos_amd import capi
    check_against_oracle(capi, (60, 90), (400, 300))


@pytest.mark.gpu
def test_allow_bits_on_gpu():
    from cerbos_amd import capi
    check_allow_bits(capi, 50_001)


@pytest.mark.gpu
def test_refusals_on_gpu():
    from cerbos_amd import capi
    check_refusals(capi)


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("name,n,m", [("c2", 2_000, 2_000), ("t", 1_000, 1_000)])
def test_at_size_on_gpu(name, n, m):
    """16 M decisions (C2) and 4 M (T): the device-built product's effects and bitmap against the host-built product, which is
    built and uploaded in blocks of resources (the product is resource-major: a block of resources is a contiguous range of it)"""
    from cerbos_amd import capi
    lt = _lower(getattr(workloads, name + "_policies")())
    p, r, acts, aux = _halves_of(name, n, m, seed=13)
    fl, table = Flattener(lt), capi.Table(lt.blob)
    h, po, ro, act = cross_halves(fl, p, r, acts, aux, "default", "", True)
    db = upload_halves(table, h, n, m, act, po, ro)
    try:
        plan = table.plan(db)
        assert plan.startswith("cbh_check_flat_kernel") and COMPACT in plan, plan
        table.launch(db, now_ns=NOW)
        bits = table.download_allow_bits(db)
        eff = table.download(db, want=()).effect.reshape(m, n * len(acts))
        assert np.array_equal(bits, _bits_of(eff.reshape(-1)))
        assert 0.01 < (eff == ALLOW).mean() < 0.99
        step = 250
        for lo in range(0, m, step):      # resources ro[lo : lo + step] in that order, principals in po's order
            block = [r[j] for j in ro[lo:lo + step]]
            cb = cross_product_batch(fl, lt.columns, [p[i] for i in po], block, acts, [aux[i] for i in po], sort=False)
            hb = table.upload(cb)
            assert table.plan(hb).startswith("cbh_check_flat_kernel")
            table.launch(hb, now_ns=NOW)
            want = table.download(hb, want=()).effect
            hb.close()
            assert np.array_equal(eff[lo:lo + step].reshape(-1), want), lo
    finally:
        db.close()
        table.close()
