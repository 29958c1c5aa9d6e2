"""The direct cross road's second entry point (cerbos_hip.h cbh_cross_upload_ex / cbh_cross_pairs_upload): tables with derived roles
(cbh_check_flat_kernel_dr_x), five to 64 actions decided four at a time, and the flagged pairs of a set as an ordinary resident batch
gathered on the device (cbh_cross_gather_kernel).

The reference everywhere is the MATERIALISED road on the same table and the same halves (cross.upload_halves -> launch -> download),
as in tests/test_cross_direct.py, whose helpers this module uses; for more than four actions that road takes the walk's kernels, an
independent family.  Every case asserts that cbh_cross_describe names an `_x[direct cross` kernel.
CPU tier: the library's host side and the kernels' source on the simulator (tests/sim_engine.py).  GPU tier: the same bodies on the device.

Two things the issue asked for are not here, because the library has no entry point for them: cbh_trace_batch and
cbh_check_batch_trail take HOST batches, so a pairs batch (device memory) goes through the resident trail (cbh_batch_set_trail,
a launch with CBH_F_WANT_EFFECTIVE_POLICIES, cbh_trail_download - what cbh_check_batch_trail is made of) and is compared with the
same calls on the materialised product; no trace pass runs on it.  And a derived-role fuzz seed qualifies by the plan
"cbh_check_flat_kernel_dr" of its materialised product (or "[compact inputs" for the staged / mask plans): cbh_check_flat_kernel_dr
has no compact instantiation, so that plan never says "[compact inputs"."""
import os

import numpy as np
import pytest

from cerbos_amd import workloads
from cerbos_amd.cross import allow_cube_planes, direct_upload_halves, flagged_pairs, upload_halves
from sim_engine import sim_engine
from test_cross_device import NOW, _halves_of, _lower
from test_cross_direct import FILL, _fuzz_case, _gpu_child, _halves, _named_x, _reference, _words, table_error

API = "api.cerbos.dev/v1"
DR_X = "cbh_check_flat_kernel_dr_x"


def _direct(table, h, n, m, act, po, ro, accept):
    cs = direct_upload_halves(table, h, n, m, act, po, ro, accept=accept)
    assert cs is not None, "the set has no direct form: " + table_error()
    return cs


def _same(table, h, n, m, act, po, ro, accept, flag_seq=(0,), tiles=None):
    """test_cross_direct._same with `accept`: the direct set against the materialised product under every flags word - both kinds of
    planes of the whole (or of `tiles`), with and without the second set of planes, and the cube in the caller's orders.  Returns the
    kernels describe named."""
    cs = _direct(table, h, n, m, act, po, ro, accept)
    names = set()
    a = len(act)
    try:
        assert cs.shape == (n, m, a)
        for flags in flag_seq:
            names.add(_named_x(cs.describe(flags)))
            want_a, want_f, dpo, dro = _reference(table, h, n, m, act, po, ro, flags)
            cube = np.empty((n, m, a), dtype=bool)
            cube[np.ix_(dpo, dro)] = want_a.transpose(1, 0, 2)
            for lo, hi in (tiles or ((0, m),)):
                allow, flagged = cs.check(lo, hi, flags=flags, now_ns=NOW, want_flagged=True)
                assert allow.shape == (a, (n * (hi - lo) + 63) // 64) and flagged.shape == allow.shape
                for k in range(a):
                    assert np.array_equal(allow[k], _words(want_a[lo:hi, :, k])), (flags, lo, hi, k, "allow")
                    assert np.array_equal(flagged[k], _words(want_f[lo:hi, :, k])), (flags, lo, hi, k, "flagged")
                only, none = cs.check(lo, hi, flags=flags, now_ns=NOW)
                assert none is None and np.array_equal(only, allow)
                assert np.array_equal(allow_cube_planes(cs, lo, hi, allow), cube[:, np.sort(np.asarray(dro)[lo:hi])]), (flags, lo, hi)
        return names
    finally:
        cs.close()


def _c3(n, m):
    p, r, acts, aux = _halves_of("c3", n, m, seed=31)
    return p, r, acts, aux


# ---- 1. C3: derived roles


def check_c3(capi):
    """C3 at 70 x 9 and 5 x 70 under flags 0, want-derived-roles, lenient; whole and in tiles; the kernel is the memo's instantiation.
    At 70 x 9 under CBH_F_WANT_DERIVED_ROLES both kinds of planes have ones and differ (on the simulator: 684 and 72 of 2 520)."""
    lt = _lower(workloads.c3_policies())
    table = capi.Table(lt.blob)
    flag_seq = (0, capi.F_WANT_DERIVED_ROLES, capi.F_LENIENT_SCOPE_SEARCH)
    try:
        for n, m in ((70, 9), (5, 70)):
            p, r, acts, aux = _c3(n, m)
            h, po, ro, act = _halves(lt, p, r, acts, aux)
            names = _same(table, h, n, m, act, po, ro, capi.CX_DERIVED_ROLES, flag_seq, tiles=((0, m), (0, 4), (4, 9)))
            assert names == {DR_X}, names
            if (n, m) == (70, 9):
                cs = _direct(table, h, n, m, act, po, ro, capi.CX_DERIVED_ROLES)
                allow, flagged = cs.check(0, m, flags=capi.F_WANT_DERIVED_ROLES, now_ns=NOW, want_flagged=True)
                cs.close()
                print("C3 70 x 9, want derived roles: %d allow bits, %d flagged bits of %d" % (_ones(allow), _ones(flagged), n * m * len(act)))
                assert allow.any() and flagged.any() and not np.array_equal(allow, flagged)
    finally:
        table.close()


def _ones(planes):
    return int(np.unpackbits(np.ascontiguousarray(planes).view(np.uint8)).sum())


# ---- 2. the other walks of a derived-role table (child processes: the library reads its switches once)

STAGED_BODY = r'''
from cerbos_amd import workloads
import test_cross_direct as td
import test_cross_direct_ex as tx
lt = td._lower(workloads.c3_policies())
table = capi.Table(lt.blob)
p, r, acts, aux = tx._c3(70, 9)
h, po, ro, act = td._halves(lt, p, r, acts, aux)
names = tx._same(table, h, 70, 9, act, po, ro, capi.CX_DERIVED_ROLES, flag_seq=(0, capi.F_WANT_DERIVED_ROLES, capi.F_LENIENT_SCOPE_SEARCH))
assert names == {"cbh_check_flat_kernel_staged_x"}, names
table.close()
print("staged ok")
'''
MASKS_BODY = r'''
from cerbos_amd import workloads
from cerbos_amd.cross import direct_upload_halves, upload_halves
import test_cross_direct as td
import test_cross_direct_ex as tx
lt = td._lower(workloads.c3_policies())
table = capi.Table(lt.blob)
p, r, acts, aux = tx._c3(70, 9)
h, po, ro, act = td._halves(lt, p, r, acts, aux)
db = upload_halves(table, h, 70, 9, act, po, ro)
plan = table.plan(db).split("[")[0]
db.close()
assert plan in ("cbh_check_flat_kernel_masks", "cbh_check_flat_kernel_any_masks"), plan
if plan == "cbh_check_flat_kernel_masks":
    names = tx._same(table, h, 70, 9, act, po, ro, capi.CX_DERIVED_ROLES, flag_seq=(0, capi.F_WANT_DERIVED_ROLES, capi.F_LENIENT_SCOPE_SEARCH))
    assert names == {"cbh_check_flat_kernel_masks_x"}, names
else:
    assert direct_upload_halves(table, h, 70, 9, act, po, ro, accept=capi.CX_DERIVED_ROLES) is None and "no direct form" in td.table_error()
table.close()
print("masks ok: " + plan)
'''
WALK_MODES = {"staged": (STAGED_BODY, {"CBH_FORCE_STAGED": "1"}, "staged ok"), "masks": (MASKS_BODY, {"CBH_FLAT_MASKS": "1"}, "masks ok")}


# ---- 3. a hand-written derived-role store

HAND_DOCS = [
    {"apiVersion": API, "derivedRoles": {"name": "hand", "definitions": [
        {"name": "owner", "parentRoles": ["user", "manager"], "condition": {"match": {"expr": "R.attr.owner == P.id"}}},           # both halves
        {"name": "senior", "parentRoles": ["user", "manager", "admin"], "condition": {"match": {"expr": "P.attr.level >= 3.5"}}},  # the principal's
        {"name": "public_viewer", "parentRoles": ["guest"], "condition": {"match": {"expr": "R.attr.public == true"}}},            # the resource's
        {"name": "anyone", "parentRoles": ["auditor"]},                                                                            # no condition
        {"name": "colleague", "parentRoles": ["*"], "condition": {"match": {"expr": "P.attr.department == R.attr.department"}}},   # parent *
        {"name": "fragile", "parentRoles": ["user", "guest"], "condition": {"match": {"expr": "P.attr.team == R.attr.team"}}},     # absent on some rows of each side
        {"name": "big", "parentRoles": ["manager"], "condition": {"match": {"expr": "R.attr.amount > 100.5"}}},
        {"name": "opsman", "parentRoles": ["admin"], "condition": {"match": {"expr": 'P.attr.department == "ops"'}}}]}},            # seven distinct conditions: the memo holds four
    {"apiVersion": API, "resourcePolicy": {"resource": "doc", "version": "default", "importDerivedRoles": ["hand"], "rules": [
        {"actions": ["view"], "derivedRoles": ["owner"], "effect": "EFFECT_ALLOW"},
        {"actions": ["edit"], "derivedRoles": ["senior", "big"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": 'R.attr.status == "OPEN"'}}},
        {"actions": ["delete"], "derivedRoles": ["colleague"], "effect": "EFFECT_ALLOW"},
        {"actions": ["approve"], "roles": ["manager"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": "R.attr.owner == P.id"}}},   # a rule shares the definitions' condition
        {"actions": ["view"], "derivedRoles": ["public_viewer", "anyone"], "effect": "EFFECT_ALLOW"},
        {"actions": ["edit"], "derivedRoles": ["fragile"], "effect": "EFFECT_DENY"},
        {"actions": ["delete"], "derivedRoles": ["opsman"], "effect": "EFFECT_ALLOW"}]}},
    {"apiVersion": API, "resourcePolicy": {"resource": "doc", "version": "default", "scope": "acme", "importDerivedRoles": ["hand"], "rules": [
        {"actions": ["view"], "derivedRoles": ["fragile"], "effect": "EFFECT_ALLOW"},
        {"actions": ["approve"], "derivedRoles": ["owner", "senior"], "effect": "EFFECT_ALLOW"},
        {"actions": ["delete"], "roles": ["user"], "effect": "EFFECT_DENY", "condition": {"match": {"expr": "R.attr.public == true"}}},
        {"actions": ["edit"], "derivedRoles": ["anyone", "opsman"], "effect": "EFFECT_ALLOW"},
        {"actions": ["approve"], "derivedRoles": ["big"], "effect": "EFFECT_DENY"}]}},
]


def _hand_halves(n, m, rng):
    roles = ["user", "manager", "admin", "guest", "auditor"]
    ps, rs = [], []
    for i in range(n):
        attr = {"level": float(rng.integers(1, 6)) + 0.25, "department": str(rng.choice(["eng", "ops"])), "team": str(rng.choice(["core", "edge"]))}
        if rng.random() < 0.25:
            del attr["team"]
        if rng.random() < 0.1:
            del attr["level"]
        ps.append({"id": "p%d" % (i % 7), "roles": [str(x) for x in rng.choice(roles, size=int(rng.integers(1, 4)), replace=False)], "attr": attr})
    ps[0]["roles"] = []                # a principal without a role ...
    if n > 1:
        ps[1]["roles"] = roles[:4]     # ... and one with four
    for j in range(m):
        attr = {"owner": "p%d" % rng.integers(0, 7), "amount": float(rng.integers(0, 200)) + 0.5, "status": str(rng.choice(["OPEN", "CLOSED"])),
                "public": bool(rng.random() < 0.5), "department": str(rng.choice(["eng", "ops"])), "team": str(rng.choice(["core", "edge"]))}
        if rng.random() < 0.25:
            del attr["team"]
        if rng.random() < 0.1:
            del attr["owner"]
        rs.append({"kind": "doc", "id": "d%d" % j, "scope": str(rng.choice(["", "acme", "acme"])), "attr": attr})
    return ps, rs


def check_hand_store(capi):
    """two scope levels (the second climb merges two buckets), 70 x 9 and 5 x 70: derived roles on both halves' operands, on either
    side's alone, without a condition, with parent `*`, on an attribute some rows of each side lack (a CEL error: under
    CBH_F_WANT_DERIVED_ROLES flagged even where no rule needed the role); seven distinct conditions in a scope (the memo holds four);
    a condition shared by a rule and both scopes' definitions; a principal without a role and one with four"""
    lt = _lower(HAND_DOCS)
    assert lt.stats["flat"] and lt.stats["flat_closed"], lt.stats
    acts = ["view", "edit", "delete", "approve"]
    table = capi.Table(lt.blob)
    flag_seq = (0, capi.F_WANT_DERIVED_ROLES, capi.F_LENIENT_SCOPE_SEARCH | capi.F_WANT_DERIVED_ROLES)
    try:
        for n, m, seed in ((70, 9, 23), (5, 70, 24)):
            ps, rs = _hand_halves(n, m, np.random.default_rng(seed))
            for sort in (True, False):
                h, po, ro, act = _halves(lt, ps, rs, acts, sort=sort)
                names = _same(table, h, n, m, act, po, ro, capi.CX_DERIVED_ROLES, flag_seq, tiles=((0, m), (1, 6)))
                assert names == {DR_X}, names
            cs = _direct(table, h, n, m, act, po, ro, capi.CX_DERIVED_ROLES)
            a0, f0 = cs.check(0, m, now_ns=NOW, want_flagged=True)
            a1, f1 = cs.check(0, m, flags=capi.F_WANT_DERIVED_ROLES, now_ns=NOW, want_flagged=True)
            cs.close()
            assert a0.any() and f0.any() and (f1 & ~f0).any(), (n, m, _ones(a0), _ones(f0), _ones(f1))   # errors no rule needed: only when the roles are wanted
    finally:
        table.close()


# ---- 4. fuzz with derived roles.  Seeds of tests/test_flat_kernel.py's stores (test_cross_direct._fuzz_case) chosen on the CPU over
# range(60): the docs contain derivedRoles and the materialised product at 40 x 11 is planned cbh_check_flat_kernel_dr (or reads
# compact inputs) - the first eight of the shallow family and the first four of the deep one.  EVERY one of them must go direct.
DR_FUZZ_SEEDS = (0, 1, 2, 3, 6, 7, 8, 9)
DR_DEEP_SEEDS = (3, 4, 5, 6)


def _qualifies(capi, seed, deep=False):
    docs, ps, rs, acts = _fuzz_case(seed, deep)
    if not any("derivedRoles" in d for d in docs):
        return False
    lt = _lower(docs)
    table = capi.Table(lt.blob)
    h, po, ro, act = _halves(lt, ps, rs, acts)
    db = upload_halves(table, h, 40, 11, act, po, ro)
    try:
        plan = table.plan(db)
        return plan == "cbh_check_flat_kernel_dr" or "[compact inputs" in plan
    finally:
        db.close()
        table.close()


def check_fuzz(capi):
    for deep, seeds in ((False, DR_FUZZ_SEEDS), (True, DR_DEEP_SEEDS)):
        assert seeds
        for seed in seeds:
            docs, ps, rs, acts = _fuzz_case(seed, deep)
            lt = _lower(docs)
            table = capi.Table(lt.blob)
            try:
                h, po, ro, act = _halves(lt, ps, rs, acts, sort=seed % 2 == 0)
                _same(table, h, 40, 11, act, po, ro, capi.CX_DERIVED_ROLES,
                      flag_seq=(0, capi.F_LENIENT_SCOPE_SEARCH, capi.F_LENIENT_SCOPE_SEARCH | capi.F_WANT_DERIVED_ROLES))
            finally:
                table.close()


# ---- 5. action groups


def _action_list(acts, a):
    """`a` distinct names: the workload's four among names no policy knows - a known one at position 4, the third group (8 .. 11) of
    unknown names only, the workload's fifth action and the last known one further back"""
    names = [acts[0], acts[1], "zz0", "zz1", acts[2], "zz2", "zz3", "zz4", "zz5", "zz6", "zz7", "zz8", acts[3], "comment", "zz9"]
    names = [x for i, x in enumerate(names) if x not in names[:i]]
    names += ["zy%d" % i for i in range(64)]
    return names[:a]


def check_action_groups(capi):
    """C2 at 70 x 9 with 5, 8, 9, 63 and 64 actions - both planes of every action, planes wider than the tile, without the second
    set of planes; describe reports the groups; C3 with six actions under CX_ALL; four actions through _ex = cbh_cross_upload's planes"""
    lt = _lower(workloads.c2_policies())
    table = capi.Table(lt.blob)
    n, m = 70, 9
    p, r, acts, aux = _halves_of("c2", n, m, seed=31)
    try:
        for a in (5, 8, 9, 63, 64):
            names = _action_list(acts, a)
            assert len(set(names)) == a and names[4] in acts
            h, po, ro, act = _halves(lt, p, r, names, aux)
            assert _same(table, h, n, m, act, po, ro, capi.CX_ACTION_GROUPS, (0, capi.F_LENIENT_SCOPE_SEARCH), tiles=((0, m), (2, 7))) == {"cbh_check_flat_kernel_x"}
            cs = _direct(table, h, n, m, act, po, ro, capi.CX_ACTION_GROUPS)
            assert ", %d action groups]" % ((a + 3) // 4) in cs.describe(0), cs.describe(0)
            w = cs.words(0, m)
            want, want_f = cs.check(0, m, now_ns=NOW, want_flagged=True)
            assert want.any() and not want[2].any()                                   # a known action allows somebody, an unknown one nobody
            if a >= 12:
                assert not want[8:12].any()                                           # the group of unknown names
            wide = (np.full((a, w + 3), FILL, dtype=np.uint64), np.full((a, w + 3), FILL, dtype=np.uint64))
            got, got_f = cs.check(0, m, now_ns=NOW, want_flagged=True, into=wide)     # words_per_plane > W
            assert np.array_equal(got, want) and np.array_equal(got_f, want_f) and (wide[0][:, w:] == FILL).all() and (wide[1][:, w:] == FILL).all()
            only, none = cs.check(0, m, now_ns=NOW, into=(wide[0], None))
            assert none is None and np.array_equal(only, want)
            cs.close()
        # four actions: the same planes by either entry point, and no word of groups
        h, po, ro, act = _halves(lt, p, r, acts, aux)
        old, new = direct_upload_halves(table, h, n, m, act, po, ro), _direct(table, h, n, m, act, po, ro, capi.CX_ALL)
        assert "action groups" not in new.describe(0) and new.describe(0) == old.describe(0)
        for x, y in zip(old.check(0, m, now_ns=NOW, want_flagged=True), new.check(0, m, now_ns=NOW, want_flagged=True)):
            assert np.array_equal(x, y)
        old.close()
        new.close()
    finally:
        table.close()
    lt = _lower(workloads.c3_policies())
    table = capi.Table(lt.blob)
    try:
        p, r, acts, aux = _c3(n, m)
        names = acts + [x for x in workloads.C3_ACTIONS if x not in acts][:1] + ["zz0"]
        assert len(names) == 6
        h, po, ro, act = _halves(lt, p, r, names, aux)
        assert _same(table, h, n, m, act, po, ro, capi.CX_ALL, (0, capi.F_WANT_DERIVED_ROLES)) == {DR_X}
    finally:
        table.close()


# ---- 6. pairs


def _pairs_equal(table, cs, ref_res, n, a, pp, pr, flags):
    """the batch of these pairs decided and downloaded = the rows pair_r * n + pair_p of the materialised product's download"""
    db = cs.pairs_batch(pp, pr)
    try:
        assert db.n_requests == len(pp) and db.n_tuples == len(pp) * a
        table.launch(db, now_ns=NOW, flags=flags)
        got = table.download(db)
        rows = np.asarray(pr, dtype=np.int64) * n + np.asarray(pp, dtype=np.int64)
        for f in ("effect", "status", "policy", "scope"):
            assert np.array_equal(getattr(got, f).reshape(-1, a), getattr(ref_res, f).reshape(-1, a)[rows]), f
        assert np.array_equal(got.edr, ref_res.edr[rows])
    finally:
        db.close()


def check_pairs(capi):
    """On the C3 set at 70 x 9 under CBH_F_WANT_DERIVED_ROLES: the flagged pairs (cross.flagged_pairs) and lists of 1, 63, 64 and 65
    pairs with duplicates in arbitrary order, every field of the download against the materialised product's rows; six actions; the
    trail of a pairs batch against the product's"""
    lt = _lower(workloads.c3_policies())
    table = capi.Table(lt.blob)
    n, m = 70, 9
    p, r, acts, aux = _c3(n, m)
    flags = capi.F_WANT_DERIVED_ROLES
    rng = np.random.default_rng(41)
    try:
        for names in (acts, acts + [x for x in workloads.C3_ACTIONS if x not in acts][:1] + ["zz0"]):
            a = len(names)
            h, po, ro, act = _halves(lt, p, r, names, aux)
            cs = _direct(table, h, n, m, act, po, ro, capi.CX_ALL)
            _named_x(cs.describe(flags))
            ref = upload_halves(table, h, n, m, act, po, ro)
            table.launch(ref, now_ns=NOW, flags=flags)
            want = table.download(ref)
            _, flagged = cs.check(0, m, flags=flags, now_ns=NOW, want_flagged=True)
            pp, pr, mask = flagged_pairs(cs, 0, m, flagged)
            st = want.status.reshape(m, n, a) != 0
            assert pp.size and pp.size == int(st.any(axis=2).sum())
            for q in range(pp.size):                                                  # the decoding: device order, the actions' mask
                assert st[pr[q], pp[q]].any() and int(mask[q]) == sum(1 << k for k in range(a) if st[pr[q], pp[q], k])
            assert (np.diff(pr.astype(np.int64) * n + pp) > 0).all()
            _pairs_equal(table, cs, want, n, a, pp, pr, flags)
            lo, hi = 3, 8                                                             # ... and from a tile's planes
            _, ft = cs.check(lo, hi, flags=flags, now_ns=NOW, want_flagged=True)
            tp, tr, _ = flagged_pairs(cs, lo, hi, ft)
            keep = (pr >= lo) & (pr < hi)
            assert np.array_equal(tp, pp[keep]) and np.array_equal(tr, pr[keep])
            if a == len(acts):
                for cnt in (1, 63, 64, 65):
                    qp, qr = rng.integers(0, n, size=cnt), rng.integers(0, m, size=cnt)
                    if cnt > 2:
                        qp[-1], qr[-1] = qp[0], qr[0]                                # a duplicate
                        qp[1], qr[1] = pp[0], pr[0]                                  # ... and a flagged pair among them
                    _pairs_equal(table, cs, want, n, a, qp, qr, flags)
                # the trail: one group per pair against one group per request of the product
                tflags = capi.F_WANT_EFFECTIVE_POLICIES
                qp, qr = np.concatenate([pp[:20], rng.integers(0, n, size=30)]), np.concatenate([pr[:20], rng.integers(0, m, size=30)])
                db = cs.pairs_batch(qp, qr)
                table.set_trail(db, np.arange(qp.size), qp.size)
                table.launch(db, now_ns=NOW, flags=tflags)
                got_t, got_r = table.trail(db), table.download(db)
                table.set_trail(ref, np.arange(n * m), n * m)
                table.launch(ref, now_ns=NOW, flags=tflags)
                want_t, want_r = table.trail(ref), table.download(ref)
                rows = qr.astype(np.int64) * n + qp
                assert want_t.any() and np.array_equal(got_t, want_t[rows])
                assert np.array_equal(got_r.effect.reshape(-1, a), want_r.effect.reshape(-1, a)[rows])
                db.close()
            ref.close()
            cs.close()
    finally:
        table.close()


# ---- 7. contract


def check_contract(capi):
    import ctypes as C
    lib = capi.load()

    def raw(table, h, n, m, act, po, ro, accept, ex=True):
        a_ids = np.ascontiguousarray(act, dtype=np.uint32)
        pa, ra = np.ascontiguousarray(po, dtype=np.uint32), np.ascontiguousarray(ro, dtype=np.uint32)
        cb = capi.make_cbatch(h, table.num_columns)
        x = capi.CCross(n, m, a_ids.size, a_ids.ctypes.data, pa.ctypes.data, ra.ctypes.data)
        out = C.c_void_p(0xDEAD)
        if ex:
            rc = lib.cbh_cross_upload_ex(table.h, 0, C.byref(cb), C.byref(x), accept, C.byref(out))
        else:
            rc = lib.cbh_cross_upload(table.h, 0, C.byref(cb), C.byref(x), C.byref(out))
        return rc, out, lib.cbh_last_error()

    def refused(lt, ps, rs, acts, aux, accepts, unknown_fails=True):
        """rc 1 with cbh_cross_upload's own text under every one of `accepts`"""
        table = capi.Table(lt.blob)
        h, po, ro, act = _halves(lt, ps, rs, acts, aux)
        rc0, out0, text0 = raw(table, h, len(ps), len(rs), act, po, ro, 0, ex=False)
        assert rc0 == 1 and not out0.value and text0
        for accept in accepts:
            rc, out, text = raw(table, h, len(ps), len(rs), act, po, ro, accept)
            assert rc == 1 and not out.value and text == text0, (accept, rc, text, text0)
        for accept in (4, 0x80000000, capi.CX_ALL | 8):
            rc, out, text = raw(table, h, len(ps), len(rs), act, po, ro, accept)
            assert rc < 0 and not out.value and text, accept                          # a bit this library does not know
        table.close()

    lt3, lt2 = _lower(workloads.c3_policies()), _lower(workloads.c2_policies())
    p3, r3, acts3, aux3 = _halves_of("c3", 6, 5, seed=3)
    p2, r2, acts2, aux2 = _halves_of("c2", 6, 5, seed=3)
    refused(lt3, p3, r3, acts3, aux3, (0, capi.CX_ACTION_GROUPS))                      # derived roles without their bit
    refused(lt2, p2, r2, acts2 + ["extra"], aux2, (0, capi.CX_DERIVED_ROLES))          # five actions without theirs
    p5, r5, acts5, aux5 = _halves_of("c5", 6, 5, seed=3)
    refused(_lower(workloads.c5_policies()), p5, r5, acts5, aux5, (0, capi.CX_ALL))    # not flat
    five = [dict(x) for x in p2]
    five[2] = dict(five[2], roles=["employee", "manager", "admin", "contractor", "auditor"])
    refused(lt2, five, r2, acts2, aux2, (0, capi.CX_ALL))                              # a five-role principal

    table, other = capi.Table(lt3.blob), capi.Table(lt3.blob)
    names = acts3 + ["zz0", "zz1"]
    h, po, ro, act = _halves(lt3, p3, r3, names, aux3)
    a, n, m = len(names), 6, 5
    try:
        cs = _direct(table, h, n, m, act, po, ro, capi.CX_ALL)
        _named_x(cs.describe(0))
        # strict evaluation: 1, nothing written
        assert cs.describe(capi.F_STRICT_EVALUATION).startswith("none")
        w = cs.words(0, m)
        buf, buf_f = np.full((a, w), FILL, dtype=np.uint64), np.full((a, w), FILL, dtype=np.uint64)
        prm = capi.CParams(NOW, capi.F_STRICT_EVALUATION, 0)
        assert lib.cbh_cross_check(table.h, cs.h, C.byref(prm), 0, m, buf.ctypes.data, buf_f.ctypes.data, w) == 1 and lib.cbh_last_error()
        assert (buf == FILL).all() and (buf_f == FILL).all()
        with pytest.raises(capi.DirectFormUnavailable):
            cs.check(0, m, flags=capi.F_STRICT_EVALUATION, now_ns=NOW)
        # pairs: what is refused
        good_p, good_r = np.array([0, 5, 2], dtype=np.uint32), np.array([4, 0, 2], dtype=np.uint32)

        def pairs(t, s, pp, pr, cnt, with_out=True):
            out = C.c_void_p(0xDEAD)
            rc = lib.cbh_cross_pairs_upload(t, s, None if pp is None else pp.ctypes.data, None if pr is None else pr.ctypes.data, cnt,
                                            C.byref(out) if with_out else None)
            return rc, out, lib.cbh_last_error()
        for args in ((None, cs.h, good_p, good_r, 3), (table.h, None, good_p, good_r, 3), (table.h, cs.h, None, good_r, 3), (table.h, cs.h, good_p, None, 3)):
            rc, out, text = pairs(*args)
            assert rc < 0 and not out.value and text, args
        rc, _, text = pairs(table.h, cs.h, good_p, good_r, 3, with_out=False)
        assert rc < 0 and text
        rc, out, text = pairs(table.h, cs.h, good_p, good_r, 0)                        # no pair
        assert rc < 0 and not out.value and text
        rc, out, text = pairs(other.h, cs.h, good_p, good_r, 3)                        # another table's set
        assert rc < 0 and not out.value and b"different table" in text
        for bad_p, bad_r in ((np.array([0, n, 2], dtype=np.uint32), good_r), (good_p, np.array([4, 0, m], dtype=np.uint32)),
                             (np.array([0xFFFFFFFF], dtype=np.uint32), np.array([0], dtype=np.uint32))):
            rc, out, text = pairs(table.h, cs.h, bad_p, bad_r, bad_p.size)
            assert rc < 0 and not out.value and b"outside the set" in text, text
        with pytest.raises(capi.HipEngineError):
            cs.pairs_batch([0, n], [0, 0])
        db = cs.pairs_batch(good_p, good_r)                                            # ... and the set still serves
        assert db.n_tuples == 3 * a
        db.close()
        assert cs.check(0, m, now_ns=NOW)[0].shape == (a, w)
        cs.close()
    finally:
        table.close()
        other.close()


# ---- CPU tier: the simulator


@pytest.fixture()
def engine():
    with sim_engine() as capi:
        yield capi


def test_c3_on_simulator(engine):
    check_c3(engine)


@pytest.mark.parametrize("mode", sorted(WALK_MODES))
def test_c3_by_the_other_walks_on_simulator(mode):
    import test_sim_engine as ts
    body, env, _ = WALK_MODES[mode]
    ts._in_own_process(body, env)


def test_hand_store_on_simulator(engine):
    check_hand_store(engine)


def test_the_listed_seeds_qualify(engine):
    assert all(_qualifies(engine, seed) for seed in DR_FUZZ_SEEDS) and all(_qualifies(engine, seed, deep=True) for seed in DR_DEEP_SEEDS)


def test_fuzz_on_simulator(engine):
    check_fuzz(engine)


def test_action_groups_on_simulator(engine):
    check_action_groups(engine)


def test_pairs_on_simulator(engine):
    check_pairs(engine)


def test_contract_on_simulator(engine):
    check_contract(engine)


def test_failing_allocations_and_copies_are_survived():
    """Fault injection (simulator only): the k-th device allocation - or asynchronous copy - from now on fails, for every k until the
    calls succeed; cbh_cross_upload_ex of a set of three action groups and cbh_cross_pairs_upload either report an error with a text or
    give the right answers, and the set decides correctly afterwards."""
    import test_sim_engine as ts
    ts._in_own_process('''
import ctypes as C
import numpy as np
from cerbos_amd import workloads
from cerbos_amd.cross import direct_upload_halves
import test_cross_direct as td
import test_cross_direct_ex as tx
NOW = td.NOW
lib = capi.load()
lib.cbh_sim_set_alloc_budget.argtypes = [C.c_long]
lib.cbh_sim_set_copy_budget.argtypes = [C.c_long]
lt = td._lower(workloads.c3_policies())
p, r, acts, aux = td._halves_of("c3", 9, 7, seed=4)
names = tx._action_list(acts, 9)
h, po, ro, act = td._halves(lt, p, r, names, aux)
pp, pr = np.array([0, 8, 3, 3, 5], dtype=np.uint32), np.array([6, 0, 2, 2, 4], dtype=np.uint32)
FL = capi.F_WANT_DERIVED_ROLES


def answers(table, cs):
    db = cs.pairs_batch(pp, pr)
    table.launch(db, now_ns=NOW, flags=FL)
    res = table.download(db)
    db.close()
    return res


ref = capi.Table(lt.blob)
cs = direct_upload_halves(ref, h, 9, 7, act, po, ro, accept=capi.CX_ALL)
assert "3 action groups" in cs.describe(0)
want, want_f = cs.check(0, 7, flags=FL, now_ns=NOW, want_flagged=True)
want_r = answers(ref, cs)
cs.close()
for setter in (lib.cbh_sim_set_alloc_budget, lib.cbh_sim_set_copy_budget):
    for phase in ("upload", "pairs"):
        failed = 0
        for k in range(200):
            table = capi.Table(lt.blob)          # (a fresh table: empty pools, every buffer a real allocation)
            cs, got_r = None, None
            if phase == "pairs":
                cs = direct_upload_halves(table, h, 9, 7, act, po, ro, accept=capi.CX_ALL)
            setter(k)
            try:
                if phase == "upload":
                    cs = direct_upload_halves(table, h, 9, 7, act, po, ro, accept=capi.CX_ALL)
                else:
                    db = cs.pairs_batch(pp, pr)
                    setter(-1)
                    table.launch(db, now_ns=NOW, flags=FL)
                    got_r = table.download(db)
                    db.close()
            except capi.HipEngineError as e:
                assert str(e), "an error without a message"
                failed += 1
            finally:
                setter(-1)
            if cs is None:                        # allowed again: as if nothing had happened
                cs = direct_upload_halves(table, h, 9, 7, act, po, ro, accept=capi.CX_ALL)
            got, got_f = cs.check(0, 7, flags=FL, now_ns=NOW, want_flagged=True)      # the set is usable after a failed call
            assert np.array_equal(got, want) and np.array_equal(got_f, want_f)
            got_r = got_r or answers(table, cs)
            for f in ("effect", "status", "policy", "scope", "edr"):
                assert np.array_equal(getattr(got_r, f), getattr(want_r, f)), f
            cs.close()
            table.close()
            if failed == k:                       # the k-th was not reached: the call had enough
                break
        assert failed >= (10 if phase == "upload" else 1) and failed == k, (phase, failed, k)   # (the bound of tests/test_cross_direct.py's check phase)
ref.close()
''', {})


# ---- GPU tier


@pytest.mark.gpu
def test_c3_on_gpu():
    from cerbos_amd import capi
    check_c3(capi)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(WALK_MODES))
def test_c3_by_the_other_walks_on_gpu(mode):
    """the switches are read once per process: a process of its own, as tests/test_cross_direct.py runs one per mode"""
    if os.environ.get("CBH_TEST_SIM_ENGINE"):
        return test_c3_by_the_other_walks_on_simulator(mode)
    body, env, ok = WALK_MODES[mode]
    _gpu_child(body, env, ok)


@pytest.mark.gpu
def test_hand_store_on_gpu():
    from cerbos_amd import capi
    check_hand_store(capi)


@pytest.mark.gpu
def test_fuzz_on_gpu():
    from cerbos_amd import capi
    check_fuzz(capi)


@pytest.mark.gpu
def test_action_groups_on_gpu():
    from cerbos_amd import capi
    check_action_groups(capi)


@pytest.mark.gpu
def test_pairs_on_gpu():
    from cerbos_amd import capi
    check_pairs(capi)


@pytest.mark.gpu
def test_contract_on_gpu():
    from cerbos_amd import capi
    check_contract(capi)
