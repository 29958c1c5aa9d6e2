"""The direct cross road for principals with five to sixteen roles (cerbos_hip.h CBH_CX_ROLE_GROUPS): a set is decided four roles at a
time - ceil(maxr / 4) role groups x ceil(A / 4) action groups of launches of the same `_x` kernel, the later role groups ORing into
the planes what the earlier ones left open (cbh_check_flat.h flat_body CROSS, CrossRoleGroup).

The reference everywhere is the MATERIALISED road on the same table and the same halves (test_cross_direct._reference): for more
than four roles that road takes the walk's kernels, an independent family.  Both kinds of planes are compared bit for bit, whole and
in tiles; every case asserts that cbh_cross_describe names an `_x[direct cross` kernel and the expected ", R role groups".  The
directed store's cells are asserted explicitly as well, and its allow bits against oracle/check.py per tuple.
CPU tier: the library's host side and the kernels' source on the simulator (tests/sim_engine.py).  GPU tier: the same bodies on the device.

Not here: the number of kernel launches per check of a narrow set with and without the bit.  The simulator's stand-in runtime counts
its launches but exposes no counter, so only the planes and `describe` of such a set are compared (check_narrow)."""
import copy
import os

import numpy as np
import pytest

from cerbos_amd import workloads
from cerbos_amd.cross import allow_cube_planes, direct_upload_halves, flagged_pairs, upload_halves
from sim_engine import sim_engine
from test_cross_device import NOW, _halves_of, _lower
from test_cross_direct import FILL, _fuzz_case, _gpu_child, _halves, _named_x, _reference, _words, table_error
import test_cross_direct_ex as tx

API = "api.cerbos.dev/v1"
ACTS = ["view", "edit", "delete", "approve"]
COUNTS = (0, 1, 4, 5, 7, 8, 9, 12, 16)


def _groups(desc):
    """R of ", R role groups" in a describe string (1 = not named)"""
    return int(desc.split(" role groups")[0].rsplit(", ", 1)[1]) if " role groups" in desc else 1


def _same(capi, table, h, n, m, act, po, ro, accept, flag_seq=(0,), tiles=None, groups=None):
    """tx._same under CX_ROLE_GROUPS, and describe's role groups"""
    cs = tx._direct(table, h, n, m, act, po, ro, accept | capi.CX_ROLE_GROUPS)
    try:
        for flags in flag_seq:
            assert _groups(cs.describe(flags)) == groups, (cs.describe(flags), groups)
            assert cs.describe(flags).endswith("]")
    finally:
        cs.close()
    return tx._same(table, h, n, m, act, po, ro, accept | capi.CX_ROLE_GROUPS, flag_seq, tiles)


# ---- 1. a directed store without derived roles

# 20 role names: eight that rules name and twelve that no policy names
DIRECTED_DOCS = [
    {"apiVersion": API, "resourcePolicy": {"resource": "doc", "version": "default", "rules": [
        {"actions": ["view"], "roles": ["key"], "effect": "EFFECT_ALLOW"},
        {"actions": ["edit"], "roles": ["denier"], "effect": "EFFECT_DENY"},
        {"actions": ["edit"], "roles": ["late"], "effect": "EFFECT_ALLOW"},
        {"actions": ["delete"], "roles": ["cond"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": 'R.attr.tag == "x"'}}},
        {"actions": ["delete"], "roles": ["sure"], "effect": "EFFECT_ALLOW"},
        {"actions": ["approve"], "roles": ["manager", "admin"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": "R.attr.amount > 100.5"}}},
        {"actions": ["approve"], "roles": ["user"], "effect": "EFFECT_DENY", "condition": {"match": {"expr": 'P.attr.department == "ops"'}}}]}},
    {"apiVersion": API, "resourcePolicy": {"resource": "doc", "version": "default", "scope": "acme", "rules": [
        {"actions": ["approve"], "roles": ["user"], "effect": "EFFECT_ALLOW"},
        {"actions": ["view"], "roles": ["admin"], "effect": "EFFECT_DENY", "condition": {"match": {"expr": "R.attr.amount > 150.5"}}}]}},
]
NAMED = ["key", "denier", "late", "cond", "sure", "manager", "admin", "user"]
FILLERS = ["f%d" % i for i in range(12)]
# the special principals: index -> (roles, what is asserted)
P_DENY_THEN_ALLOW, P_BEHIND, P_ALONE, P_SWAP_BEHIND, P_SWAP_ALONE = 16, 17, 18, 19, 20


def _directed_halves():
    """70 principals, 9 resources.  Principal k < 16: its k-th role is `key`, the only role of the store that allows `view`, among
    roles no policy names - with the smallest role count of COUNTS that has a k-th role.  16 .. 20: the special cases.  The rest:
    random role counts of COUNTS, random roles of all twenty names.  Resources: every second one lacks `tag`."""
    rng = np.random.default_rng(77)
    f = FILLERS
    ps = []
    for k in range(16):
        cnt = min(c for c in COUNTS if c > k)
        roles = (f + ["denier", "late", "manager", "user"])[:cnt]     # (none of them bears on `view` at any scope)
        roles[k] = "key"
        ps.append(roles)
    ps.append(["denier"] + f[:7] + ["late"])              # denied by a role of group 0, allowed by one of group 2: allowed
    ps.append(["sure"] + f[:3] + ["cond"])                # the erring condition of group 1 behind an allowing role of group 0: not flagged
    ps.append(f[:4] + ["cond"])                           # ... without it: flagged
    ps.append(["cond"] + f[:3] + ["sure"])                # the groups swapped: the condition is evaluated first - flagged, and allowed
    ps.append(["cond"] + f[:4])                           # ... flagged, not allowed
    while len(ps) < 70:
        cnt = int(rng.choice(COUNTS))
        ps.append([str(x) for x in rng.choice(NAMED + FILLERS, size=cnt, replace=False)])
    ps = [{"id": "p%d" % i, "roles": roles, "attr": {"department": "ops" if i % 3 == 0 else "eng"}} for i, roles in enumerate(ps)]
    rs = []
    for j in range(9):
        attr = {"amount": 40.5 * j}
        if j % 2 == 0:
            attr["tag"] = "x" if j % 4 == 0 else "y"
        rs.append({"kind": "doc", "id": "d%d" % j, "scope": "acme" if j % 3 == 2 else "", "attr": attr})
    return ps, rs


def check_directed(capi, kernel="cbh_check_flat_kernel_x", oracle=True):
    lt = _lower(DIRECTED_DOCS)
    assert lt.stats["flat"], lt.stats
    ps, rs = _directed_halves()
    n, m = len(ps), len(rs)
    assert sorted(set(len(p["roles"]) for p in ps)) == list(COUNTS)
    table = capi.Table(lt.blob)
    flag_seq = (0, capi.F_LENIENT_SCOPE_SEARCH)
    try:
        for sort in (False, True):
            h, po, ro, act = _halves(lt, ps, rs, ACTS, sort=sort)
            assert direct_upload_halves(table, h, n, m, act, po, ro, accept=capi.CX_ALL) is None and "more than four roles" in table_error()
            names = _same(capi, table, h, n, m, act, po, ro, 0, flag_seq, tiles=((0, m), (0, 4), (4, 9)), groups=4)
            assert names == {kernel}, names
            cs = tx._direct(table, h, n, m, act, po, ro, capi.CX_ROLE_GROUPS)
            try:
                for flags in flag_seq:
                    allow, flagged = cs.check(0, m, flags=flags, now_ns=NOW, want_flagged=True)
                    A, F = allow_cube_planes(cs, 0, m, allow), allow_cube_planes(cs, 0, m, flagged)     # [n][m][a], the caller's orders
                    view, edit, delete = 0, 1, 2
                    for k in range(16):
                        assert A[k, :, view].all(), (k, flags)                                        # the only allowing role is the k-th
                    assert not A[P_ALONE, :, view].any()
                    assert A[P_DENY_THEN_ALLOW, :, edit].all() and not F[P_DENY_THEN_ALLOW].any()
                    for j in range(m):
                        lacks, hit = "tag" not in rs[j]["attr"], rs[j]["attr"].get("tag") == "x"
                        assert A[P_BEHIND, j, delete] and not F[P_BEHIND, j, delete], (j, flags)
                        assert A[P_ALONE, j, delete] == hit and F[P_ALONE, j, delete] == lacks, (j, flags)
                        assert A[P_SWAP_BEHIND, j, delete] and F[P_SWAP_BEHIND, j, delete] == lacks, (j, flags)
                        assert A[P_SWAP_ALONE, j, delete] == hit and F[P_SWAP_ALONE, j, delete] == lacks, (j, flags)
                    if oracle and flags == 0 and sort:
                        _against_oracle(A, ps, rs)
            finally:
                cs.close()
    finally:
        table.close()


def _against_oracle(cube, ps, rs):
    """the allow bits of every tuple against oracle/check.py on explicit CheckInputs (as test_cross_direct.check_against_oracle)"""
    from cerbos_amd.policy.loader import policies_from_docs
    from cerbos_amd.ruletable.build import rule_table_from_policies
    from oracle.check import EvalParams, RuleTableOracle
    orc = RuleTableOracle(rule_table_from_policies(policies_from_docs(DIRECTED_DOCS)))
    for i, p in enumerate(ps):
        for j, r in enumerate(rs):
            out = orc.check({"principal": p, "resource": r, "actions": ACTS}, EvalParams(now_ns=NOW))
            assert [out["actions"][x]["effect"] == "EFFECT_ALLOW" for x in ACTS] == list(cube[i, j]), (i, j)


DIRECTED_BODY = r'''
import test_cross_direct_roles as tr
tr.check_directed(capi, kernel=%r, oracle=False)
print("directed ok")
'''
WALK_MODES = {"staged": (DIRECTED_BODY % "cbh_check_flat_kernel_staged_x", {"CBH_FORCE_STAGED": "1"}, "directed ok"),
              "masks": (DIRECTED_BODY % "cbh_check_flat_kernel_masks_x", {"CBH_FLAT_MASKS": "1"}, "directed ok")}


# ---- 2. derived roles: test_cross_direct_ex.HAND_DOCS, principals widened to 5 .. 12 roles

def _dr_docs():
    """HAND_DOCS and the rc_all case: `lonely`, whose only parent role is `sixth` and whose condition reads an attribute some resources
    lack; `first` allows every action at the deeper scope"""
    docs = copy.deepcopy(tx.HAND_DOCS)
    docs[0]["derivedRoles"]["definitions"].append({"name": "lonely", "parentRoles": ["sixth"], "condition": {"match": {"expr": 'R.attr.owner == "p1"'}}})
    docs[2]["resourcePolicy"]["rules"].append({"actions": ["view"], "derivedRoles": ["lonely"], "effect": "EFFECT_ALLOW"})   # (a policy's definitions are those its rules name)
    docs[2]["resourcePolicy"]["rules"].append({"actions": list(ACTS), "roles": ["first"], "effect": "EFFECT_ALLOW"})
    return docs


P_RC_ALL = 2


def _dr_halves(n, m, rng):
    ps, rs = tx._hand_halves(n, m, rng)
    fill = ["x%d" % i for i in range(12)]
    for i in range(2, n):                                       # (0: no role, 1: four - as they are)
        cnt = int(rng.integers(5, 13))
        roles = list(ps[i]["roles"]) + fill[:cnt - len(ps[i]["roles"])]
        ps[i]["roles"] = [roles[k] for k in rng.permutation(cnt)]
    if n > P_RC_ALL:
        ps[P_RC_ALL]["roles"] = ["first", "x0", "x1", "x2", "x3", "sixth"]
    rs[0] = {"kind": "doc", "id": "d0", "scope": "acme", "attr": {k: v for k, v in rs[0]["attr"].items() if k != "owner"}}
    return ps, rs


def check_derived(capi):
    """under CX_DERIVED_ROLES | CX_ROLE_GROUPS, the kernel is the memo's instantiation; the rc_all case: every action of principal
    P_RC_ALL on resource 0 (scope acme, no owner) is allowed by its first role at the deeper scope - and flagged exactly when the
    derived roles are wanted, by the definition whose only parent is its sixth role"""
    lt = _lower(_dr_docs())
    assert lt.stats["flat"] and lt.stats["flat_closed"], lt.stats
    table = capi.Table(lt.blob)
    flag_seq = (0, capi.F_WANT_DERIVED_ROLES, capi.F_LENIENT_SCOPE_SEARCH)
    try:
        for n, m, seed in ((70, 9, 23), (5, 70, 24)):
            ps, rs = _dr_halves(n, m, np.random.default_rng(seed))
            maxr = max(len(p["roles"]) for p in ps)
            assert 5 <= maxr <= 12
            for sort in (True, False):
                h, po, ro, act = _halves(lt, ps, rs, ACTS, sort=sort)
                names = _same(capi, table, h, n, m, act, po, ro, capi.CX_DERIVED_ROLES, flag_seq, tiles=((0, m), (1, 6)), groups=(maxr + 3) // 4)
                assert names == {tx.DR_X}, names
            cs = tx._direct(table, h, n, m, act, po, ro, capi.CX_DERIVED_ROLES | capi.CX_ROLE_GROUPS)
            a0, f0 = cs.check(0, m, now_ns=NOW, want_flagged=True)
            a1, f1 = cs.check(0, m, flags=capi.F_WANT_DERIVED_ROLES, now_ns=NOW, want_flagged=True)
            A0, F0, A1, F1 = (allow_cube_planes(cs, 0, m, x) for x in (a0, f0, a1, f1))
            cs.close()
            assert A0[P_RC_ALL, 0].all() and not F0[P_RC_ALL, 0].any() and A1[P_RC_ALL, 0].all() and F1[P_RC_ALL, 0].all()
            assert a0.any() and f0.any() and (f1 & ~f0).any()
    finally:
        table.close()


# ---- 3. both kinds of groups

def check_both_groups(capi):
    """A = 9 with principals of up to 9 roles (the directed store's, cut to their first nine): 3 x 3 launches per check; describe names both counts; the planes stay [A][words]"""
    lt = _lower(DIRECTED_DOCS)
    ps, rs = _directed_halves()
    ps = [dict(p, roles=p["roles"][:9]) for p in ps]
    n, m = len(ps), len(rs)
    assert max(len(p["roles"]) for p in ps) == 9 and n > 64
    names = tx._action_list(ACTS, 9)
    table = capi.Table(lt.blob)
    try:
        h, po, ro, act = _halves(lt, ps, rs, names)
        accept = capi.CX_ACTION_GROUPS | capi.CX_ROLE_GROUPS
        assert direct_upload_halves(table, h, n, m, act, po, ro, accept=capi.CX_ROLE_GROUPS) is None
        assert _same(capi, table, h, n, m, act, po, ro, capi.CX_ACTION_GROUPS, (0, capi.F_LENIENT_SCOPE_SEARCH), tiles=((0, m), (2, 7)), groups=3) == {"cbh_check_flat_kernel_x"}
        cs = tx._direct(table, h, n, m, act, po, ro, accept)
        assert cs.describe(0).endswith(", 3 action groups, 3 role groups]"), cs.describe(0)
        allow, flagged = cs.check(0, m, now_ns=NOW, want_flagged=True)
        assert allow.shape == (9, cs.words(0, m)) and flagged.shape == allow.shape and allow[0].any() and not allow[2].any()
        cs.close()
    finally:
        table.close()


# ---- 4. tiles and reuse

def check_tiles(capi):
    """the tiles (0, m), (0, 4), (4, 9) on ONE set, in that order and in reverse, a check without `flagged` between two with it: the
    device words are reused from tile to tile and no stale one is read; the words beyond W keep the caller's fill"""
    lt = _lower(DIRECTED_DOCS)
    ps, rs = _directed_halves()
    n, m = len(ps), len(rs)
    table = capi.Table(lt.blob)
    try:
        h, po, ro, act = _halves(lt, ps, rs, ACTS)
        want_a, want_f, _, _ = _reference(table, h, n, m, act, po, ro, 0)
        cs = tx._direct(table, h, n, m, act, po, ro, capi.CX_ROLE_GROUPS)
        tiles = ((0, m), (0, 4), (4, 9))
        for seq in (tiles, tiles[::-1]):
            for i, (lo, hi) in enumerate(seq):
                w = cs.words(lo, hi)
                for with_flagged in (True, False, True) if i == 1 else (True,):
                    wide = (np.full((4, w + 2), FILL, dtype=np.uint64), np.full((4, w + 2), FILL, dtype=np.uint64))
                    got, got_f = cs.check(lo, hi, now_ns=NOW, want_flagged=with_flagged, into=wide if with_flagged else (wide[0], None))
                    for k in range(4):
                        assert np.array_equal(got[k], _words(want_a[lo:hi, :, k])), (lo, hi, k)
                        if with_flagged:
                            assert np.array_equal(got_f[k], _words(want_f[lo:hi, :, k])), (lo, hi, k)
                    assert (wide[0][:, w:] == FILL).all() and (wide[1][:, w:] == FILL).all() and (with_flagged or (wide[1] == FILL).all())
        cs.close()
    finally:
        table.close()


# ---- 5. narrow sets under the new bit

def check_narrow(capi):
    """a set whose principals all have at most four roles, uploaded with and without CX_ROLE_GROUPS: the same planes, the same describe"""
    for name, accept in (("c2", 0), ("c3", capi.CX_DERIVED_ROLES)):
        lt = _lower(getattr(workloads, name + "_policies")())
        table = capi.Table(lt.blob)
        n, m = 70, 9
        p, r, acts, aux = _halves_of(name, n, m, seed=31)
        try:
            h, po, ro, act = _halves(lt, p, r, acts, aux)
            old, new = tx._direct(table, h, n, m, act, po, ro, accept), tx._direct(table, h, n, m, act, po, ro, accept | capi.CX_ROLE_GROUPS)
            for flags in (0, capi.F_WANT_DERIVED_ROLES):
                assert "role groups" not in new.describe(flags) and new.describe(flags) == old.describe(flags)
                for x, y in zip(old.check(0, m, flags=flags, now_ns=NOW, want_flagged=True), new.check(0, m, flags=flags, now_ns=NOW, want_flagged=True)):
                    assert np.array_equal(x, y)
            old.close()
            new.close()
        finally:
            table.close()


# ---- 6. pairs

def check_pairs(capi):
    """the flagged pairs of the derived-role set plus chosen wide principals through pairs_batch: every field of the download equals
    the same rows of the materialised product, the resident trail equals the product's, the batch's plan names a walk kernel"""
    lt = _lower(_dr_docs())
    table = capi.Table(lt.blob)
    n, m, a = 70, 9, 4
    ps, rs = _dr_halves(n, m, np.random.default_rng(23))
    flags = capi.F_WANT_DERIVED_ROLES
    rng = np.random.default_rng(43)
    try:
        h, po, ro, act = _halves(lt, ps, rs, ACTS)
        cs = tx._direct(table, h, n, m, act, po, ro, capi.CX_DERIVED_ROLES | capi.CX_ROLE_GROUPS)
        ref = upload_halves(table, h, n, m, act, po, ro)
        table.launch(ref, now_ns=NOW, flags=flags)
        want = table.download(ref)
        _, flagged = cs.check(0, m, flags=flags, now_ns=NOW, want_flagged=True)
        pp, pr, _ = flagged_pairs(cs, 0, m, flagged)
        assert pp.size and pp.size == int((want.status.reshape(m, n, a) != 0).any(axis=2).sum())
        cnt = np.array([len(ps[i]["roles"]) for i in np.asarray(cs.p_order)])          # role counts by device position
        widest, narrow = int(np.argmax(cnt)), int(np.argmin(cnt))
        assert cnt[widest] > 8 and cnt[narrow] == 0
        for qp, qr in ((pp, pr), ([widest], [3]), ([narrow, widest, narrow], [0, 8, 8]), ([narrow, int(np.flatnonzero(cnt == 4)[0])], [1, 2]),
                       (np.concatenate([pp[:20], rng.integers(0, n, size=45)]), np.concatenate([pr[:20], rng.integers(0, m, size=45)]))):
            tx._pairs_equal(table, cs, want, n, a, np.asarray(qp), np.asarray(qr), flags)
        db = cs.pairs_batch([widest, narrow], [0, 1])
        plan = table.plan(db, flags=flags)
        assert "walk2" in plan or plan.startswith("cbh_check_kernel"), plan
        db.close()
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
    assert capi.CX_ROLE_GROUPS == 16 and capi.CX_ALL == 3

    def raw(table, h, n, m, act, po, ro, accept):
        a_ids = np.ascontiguousarray(act, dtype=np.uint32)
        pa, ra = np.ascontiguousarray(po, dtype=np.uint32), np.ascontiguousarray(ro, dtype=np.uint32)
        cb = capi.make_cbatch(h, table.num_columns)
        x = capi.CCross(n, m, a_ids.size, a_ids.ctypes.data, pa.ctypes.data, ra.ctypes.data)
        out = C.c_void_p(0xDEAD)
        rc = lib.cbh_cross_upload_ex(table.h, 0, C.byref(cb), C.byref(x), accept, C.byref(out))
        return rc, out, lib.cbh_last_error()

    lt = _lower(workloads.c2_policies())
    p, r, acts, aux = _halves_of("c2", 6, 5, seed=3)
    wide = [dict(x) for x in p]
    wide[2] = dict(wide[2], roles=["employee", "manager", "admin", "contractor", "auditor"])
    table, other = capi.Table(lt.blob), capi.Table(lt.blob)
    try:
        h, po, ro, act = _halves(lt, wide, r, acts, aux)
        rc0, out0, text0 = raw(table, h, 6, 5, act, po, ro, 0)
        assert rc0 == 1 and not out0.value and b"more than four roles" in text0
        rc, out, text = raw(table, h, 6, 5, act, po, ro, capi.CX_ALL)                   # without the bit: today's text
        assert rc == 1 and not out.value and text == text0
        for accept in (4, 8, capi.CX_ROLE_GROUPS | 4, capi.CX_ROLE_GROUPS | 8, 32, 0x80000000):
            rc, out, text = raw(table, h, 6, 5, act, po, ro, accept)
            assert rc < 0 and not out.value and b"does not know" in text, accept          # still unknown bits
        for accept in (capi.CX_ROLE_GROUPS, capi.CX_ALL | capi.CX_ROLE_GROUPS):
            rc, out, text = raw(table, h, 6, 5, act, po, ro, accept)
            assert rc == 0 and out.value
            lib.cbh_cross_release(out)
        many = [dict(x) for x in p]
        many[4] = dict(many[4], roles=["r%d" % i for i in range(17)])
        h17, po17, ro17, act17 = _halves(lt, many, r, acts, aux)
        rc, out, text = raw(table, h17, 6, 5, act17, po17, ro17, capi.CX_ALL | capi.CX_ROLE_GROUPS)
        assert rc == 1 and not out.value and text and text != text0 and b"16" in text     # a text of its own
        rc, out, text = raw(table, h17, 6, 5, act17, po17, ro17, capi.CX_ALL)
        assert rc == 1 and not out.value and text == text0
        # what else returns 1 does so with the bit too: derived roles without theirs, five actions without theirs, a table that is not flat
        lt3 = _lower(workloads.c3_policies())
        p3, r3, acts3, aux3 = _halves_of("c3", 6, 5, seed=3)
        for ltx, px, rx, ax, auxx, words in ((lt3, p3, r3, acts3, aux3, b"derived roles"), (lt, wide, r, acts + ["extra"], aux, b"more than four actions")):
            t = capi.Table(ltx.blob)
            hx, pox, rox, actx = _halves(ltx, px, rx, ax, auxx)
            rc, out, text = raw(t, hx, 6, 5, actx, pox, rox, capi.CX_ROLE_GROUPS)
            assert rc == 1 and not out.value and words in text, text
            t.close()
        p5, r5, acts5, aux5 = _halves_of("c5", 6, 5, seed=3)
        lt5 = _lower(workloads.c5_policies())
        t = capi.Table(lt5.blob)
        hx, pox, rox, actx = _halves(lt5, p5, r5, acts5, aux5)
        rc, out, text = raw(t, hx, 6, 5, actx, pox, rox, capi.CX_ALL | capi.CX_ROLE_GROUPS)
        assert rc == 1 and not out.value and b"not flat" in text
        t.close()
        # a set of another table, strict evaluation, the trail's flag: as for a narrow set
        cs = tx._direct(table, h, 6, 5, act, po, ro, capi.CX_ROLE_GROUPS)
        assert _groups(cs.describe(0)) == 2 and _named_x(cs.describe(0))
        w = cs.words(0, 5)
        buf, buf_f = np.full((4, w), FILL, dtype=np.uint64), np.full((4, w), FILL, dtype=np.uint64)
        for flags in (capi.F_STRICT_EVALUATION, capi.F_WANT_EFFECTIVE_POLICIES):
            assert cs.describe(flags).startswith("none")
            prm = capi.CParams(NOW, flags, 0)
            assert lib.cbh_cross_check(table.h, cs.h, C.byref(prm), 0, 5, buf.ctypes.data, buf_f.ctypes.data, w) == 1 and lib.cbh_last_error()
            assert (buf == FILL).all() and (buf_f == FILL).all()
            with pytest.raises(capi.DirectFormUnavailable):
                cs.check(0, 5, flags=flags, now_ns=NOW)
        prm = capi.CParams(NOW, 0, 0)
        assert lib.cbh_cross_check(other.h, cs.h, C.byref(prm), 0, 5, buf.ctypes.data, None, w) < 0 and b"different table" in lib.cbh_last_error()
        assert (buf == FILL).all()
        want_a, want_f, _, _ = _reference(table, h, 6, 5, act, po, ro, 0)
        got, got_f = cs.check(0, 5, now_ns=NOW, want_flagged=True)                        # ... and the set still serves
        for k in range(4):
            assert np.array_equal(got[k], _words(want_a[:, :, k])) and np.array_equal(got_f[k], _words(want_f[:, :, k]))
        cs.close()
    finally:
        table.close()
        other.close()


# ---- 8. fuzz.  Seeds of tests/test_flat_kernel.py's stores (test_cross_direct._fuzz_case) whose principals are re-dealt 1 .. 16 roles
# from the store's role names (with repeats: the stores name seven).  Chosen on the simulator among the seeds the narrow modules
# list: shallow stores without and with derived roles, deep stores (more than one scope) without and with.  EVERY one must go direct.
FUZZ = ((4, False), (5, False), (0, False), (1, False), (2, False), (0, True), (1, True), (3, True))


def _fuzz_wide(seed, deep):
    import test_flat_kernel as tfk
    docs, ps, rs, acts = _fuzz_case(seed, deep)
    rng = np.random.default_rng(91_000 + seed)
    ps = [dict(p, roles=[str(x) for x in rng.choice(tfk.ROLES + ["stranger"], size=int(rng.integers(1, 17)))]) for p in ps]
    return docs, ps, rs, acts


def _fuzz_accept(capi):
    return capi.CX_DERIVED_ROLES | capi.CX_ROLE_GROUPS


def check_fuzz_qualifies(capi):
    kinds = set()
    for seed, deep in FUZZ:
        docs, ps, rs, acts = _fuzz_wide(seed, deep)
        lt = _lower(docs)
        table = capi.Table(lt.blob)
        try:
            h, po, ro, act = _halves(lt, ps, rs, acts)
            cs = direct_upload_halves(table, h, 40, 11, act, po, ro, accept=_fuzz_accept(capi))
            assert cs is not None, (seed, deep, table_error())
            assert _groups(cs.describe(0)) == (max(len(p["roles"]) for p in ps) + 3) // 4 > 1, (seed, deep, cs.describe(0))
            cs.close()
            kinds.add((any("derivedRoles" in d for d in docs), len([s for s in lt.scopes]) > 1))
        finally:
            table.close()
    assert any(dr for dr, _ in kinds) and any(sc for _, sc in kinds), kinds


def check_fuzz(capi):
    for seed, deep in FUZZ:
        docs, ps, rs, acts = _fuzz_wide(seed, deep)
        lt = _lower(docs)
        table = capi.Table(lt.blob)
        try:
            h, po, ro, act = _halves(lt, ps, rs, acts, sort=seed % 2 == 0)
            groups = (max(len(p["roles"]) for p in ps) + 3) // 4
            _same(capi, table, h, 40, 11, act, po, ro, capi.CX_DERIVED_ROLES,
                  flag_seq=(0, capi.F_LENIENT_SCOPE_SEARCH, capi.F_LENIENT_SCOPE_SEARCH | capi.F_WANT_DERIVED_ROLES), groups=groups)
        finally:
            table.close()


# ---- CPU tier: the simulator


@pytest.fixture()
def engine():
    with sim_engine() as capi:
        yield capi


def test_directed_store_on_simulator(engine):
    check_directed(engine)


@pytest.mark.parametrize("mode", sorted(WALK_MODES))
def test_directed_store_by_the_other_walks_on_simulator(mode):
    import test_sim_engine as ts
    body, env, _ = WALK_MODES[mode]
    ts._in_own_process(body, env)


def test_derived_roles_on_simulator(engine):
    check_derived(engine)


def test_both_kinds_of_groups_on_simulator(engine):
    check_both_groups(engine)


def test_tiles_and_reuse_on_simulator(engine):
    check_tiles(engine)


def test_narrow_sets_on_simulator(engine):
    check_narrow(engine)


def test_pairs_on_simulator(engine):
    check_pairs(engine)


def test_contract_on_simulator(engine):
    check_contract(engine)


def test_every_listed_seed_goes_direct(engine):
    check_fuzz_qualifies(engine)


def test_fuzz_on_simulator(engine):
    check_fuzz(engine)


def test_failing_allocations_and_copies_are_survived():
    """Fault injection (simulator only): the k-th device allocation - or asynchronous copy - from now on fails, for every k until the
    calls succeed; cbh_cross_upload_ex of a set with three role groups and a check of it either report an error with a text or give
    the reference's planes, and the set decides correctly afterwards."""
    import test_sim_engine as ts
    ts._in_own_process('''
import ctypes as C
import numpy as np
import test_cross_direct as td
import test_cross_direct_ex as tx
import test_cross_direct_roles as tr
NOW = td.NOW
lib = capi.load()
lib.cbh_sim_set_alloc_budget.argtypes = [C.c_long]
lib.cbh_sim_set_copy_budget.argtypes = [C.c_long]
lt = td._lower(tr._dr_docs())
ps, rs = tr._dr_halves(9, 7, np.random.default_rng(5))
h, po, ro, act = td._halves(lt, ps, rs, tr.ACTS)
ACCEPT = capi.CX_DERIVED_ROLES | capi.CX_ROLE_GROUPS
FL = capi.F_WANT_DERIVED_ROLES
ref = capi.Table(lt.blob)
want_a, want_f, _, _ = td._reference(ref, h, 9, 7, act, po, ro, FL)
want = np.stack([td._words(want_a[:, :, k]) for k in range(4)]), np.stack([td._words(want_f[:, :, k]) for k in range(4)])
cs = tx._direct(ref, h, 9, 7, act, po, ro, ACCEPT)
assert tr._groups(cs.describe(0)) > 1
cs.close()
ref.close()
for setter in (lib.cbh_sim_set_alloc_budget, lib.cbh_sim_set_copy_budget):
    for phase in ("upload", "check"):
        failed = 0
        for k in range(200):
            table = capi.Table(lt.blob)          # (a fresh table: empty pools, every buffer a real allocation)
            cs = None
            if phase == "check":
                cs = tx._direct(table, h, 9, 7, act, po, ro, ACCEPT)
            setter(k)
            try:
                if phase == "upload":
                    cs = tx._direct(table, h, 9, 7, act, po, ro, ACCEPT)
                else:
                    cs.check(0, 7, flags=FL, now_ns=NOW, want_flagged=True)
            except capi.HipEngineError as e:
                assert str(e), "an error without a message"
                failed += 1
            finally:
                setter(-1)
            if cs is None:                        # allowed again: as if nothing had happened
                cs = tx._direct(table, h, 9, 7, act, po, ro, ACCEPT)
            got, got_f = cs.check(0, 7, flags=FL, now_ns=NOW, want_flagged=True)      # the set is usable after a failed call
            assert np.array_equal(got, want[0]) and np.array_equal(got_f, want[1])
            cs.close()
            table.close()
            if failed == k:                       # the k-th was not reached: the call had enough
                break
        assert failed >= (10 if phase == "upload" else 1) and failed == k, (phase, failed, k)   # (the bound of tests/test_cross_direct.py)
''', {})


# ---- GPU tier


@pytest.mark.gpu
def test_directed_store_on_gpu():
    from cerbos_amd import capi
    check_directed(capi)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(WALK_MODES))
def test_directed_store_by_the_other_walks_on_gpu(mode):
    """the switches are read once per process: a process of its own, as tests/test_cross_direct.py runs one per mode"""
    if os.environ.get("CBH_TEST_SIM_ENGINE"):
        return test_directed_store_by_the_other_walks_on_simulator(mode)
    body, env, ok = WALK_MODES[mode]
    _gpu_child(body, env, ok)


@pytest.mark.gpu
def test_derived_roles_on_gpu():
    from cerbos_amd import capi
    check_derived(capi)


@pytest.mark.gpu
def test_both_kinds_of_groups_on_gpu():
    from cerbos_amd import capi
    check_both_groups(capi)


@pytest.mark.gpu
def test_tiles_and_reuse_on_gpu():
    from cerbos_amd import capi
    check_tiles(capi)


@pytest.mark.gpu
def test_narrow_sets_on_gpu():
    from cerbos_amd import capi
    check_narrow(capi)


@pytest.mark.gpu
def test_pairs_on_gpu():
    from cerbos_amd import capi
    check_pairs(capi)


@pytest.mark.gpu
def test_contract_on_gpu():
    from cerbos_amd import capi
    check_contract(capi)


@pytest.mark.gpu
def test_fuzz_on_gpu():
    from cerbos_amd import capi
    check_fuzz_qualifies(capi)
    check_fuzz(capi)
