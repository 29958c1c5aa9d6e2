"""The direct cross road (cerbos_hip.h cbh_cross_upload / cbh_cross_check; cbh_check_flat.h flat_body CROSS): N x M x A decided straight
from the N + M halves, tile by tile, one ballot word per 64 pairs and action.

The reference everywhere is the MATERIALISED road on the same table and the same halves (cross.upload_halves -> launch -> download):
the `allow` planes must equal effect == ALLOW regrouped by action, the `flagged` planes status != 0, bit for bit.  Every case asserts
that cbh_cross_describe names an `_x` kernel: a test that passes because something fell back proves nothing.
CPU tier: the library's host side and the kernels' source on the simulator (tests/sim_engine.py).  GPU tier: the same bodies on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cerbos_amd import workloads
from cerbos_amd.cross import (allow_cube_planes, cross_direct_upload, cross_halves, cross_product_batch, direct_upload_halves,
                              effect_cube, upload_halves)
from cerbos_amd.flatten import Flattener
from sim_engine import sim_engine
from test_cross_device import ALLOW, NOW, _halves_of, _lower

API = "api.cerbos.dev/v1"
FILL = 0x5A5A5A5A5A5A5A5A


def _words(bits):
    """bool[...] in tile order -> the uint64 words of one plane"""
    by = np.packbits(np.asarray(bits).reshape(-1), bitorder="little")
    return np.concatenate([by, np.zeros(-by.size % 8, dtype=np.uint8)]).view("<u8")


def _reference(table, h, n, m, act, po, ro, flags):
    """the materialised road: (allowed, flagged) as bool[m][n][a] in device order"""
    db = upload_halves(table, h, n, m, act, po, ro)
    try:
        table.launch(db, now_ns=NOW, flags=flags)
        res = table.download(db)
        a = len(act)
        return res.effect.reshape(m, n, a) == ALLOW, res.status.reshape(m, n, a) != 0, db.p_order, db.r_order
    finally:
        db.close()


def _direct(table, h, n, m, act, po, ro):
    cs = direct_upload_halves(table, h, n, m, act, po, ro)
    assert cs is not None, "the set has no direct form: " + table_error()
    return cs


def table_error():
    from cerbos_amd import capi
    return capi.load().cbh_last_error().decode("utf-8", "replace")


def _named_x(desc):
    assert desc.startswith("cbh_check_flat_kernel") and "_x[direct cross" in desc, desc
    return desc.split("[")[0]


def _same(table, h, n, m, act, po, ro, flag_seq=(0,), tiles=None):
    """the direct set against the materialised product under every flags word: both kinds of planes of the whole (or of `tiles`),
    and the cube in the caller's orders.  Returns the kernels describe named."""
    cs = _direct(table, h, n, m, act, po, ro)
    names = set()
    try:
        assert cs.shape == (n, m, len(act))
        for flags in flag_seq:
            names.add(_named_x(cs.describe(flags)))
            want_a, want_f, dpo, dro = _reference(table, h, n, m, act, po, ro, flags)
            cube = np.empty((n, m, len(act)), dtype=bool)                     # the reference in the caller's orders
            cube[np.ix_(dpo, dro)] = want_a.transpose(1, 0, 2)
            for lo, hi in (tiles or ((0, m),)):
                allow, flagged = cs.check(lo, hi, flags=flags, now_ns=NOW, want_flagged=True)
                assert allow.shape == (len(act), (n * (hi - lo) + 63) // 64) and flagged.shape == allow.shape
                for k in range(len(act)):
                    assert np.array_equal(allow[k], _words(want_a[lo:hi, :, k])), (flags, lo, hi, k, "allow")
                    assert np.array_equal(flagged[k], _words(want_f[lo:hi, :, k])), (flags, lo, hi, k, "flagged")
                only, none = cs.check(lo, hi, flags=flags, now_ns=NOW)       # without the second set of planes
                assert none is None and np.array_equal(only, allow)
                # the tile's cube: its resources are r_order[lo:hi], returned in the caller's resource order
                assert np.array_equal(allow_cube_planes(cs, lo, hi, allow), cube[:, np.sort(np.asarray(dro)[lo:hi])]), (flags, lo, hi)
            allow, _ = cs.check(0, m, flags=flags, now_ns=NOW)
            assert np.array_equal(allow_cube_planes(cs, 0, m, allow), cube), flags
        return names
    finally:
        cs.close()


def _halves(lt, p, r, acts, aux=None, sort=True):
    return cross_halves(Flattener(lt), p, r, acts, aux, "default", "", sort)


# ---- the bodies: the same on the simulator and on the device


def check_workloads(capi):
    """C2 and T at 70 x 9 (waves straddle a resource boundary) and 5 x 70 (a wave spans thirteen resources), C4 at 70 x 9; strict
    evaluation has no direct form.  Returns the kernels named."""
    names = set()
    for name, shapes in (("c2", ((70, 9), (5, 70))), ("t", ((70, 9), (5, 70))), ("c4", ((70, 9),))):
        lt = _lower(getattr(workloads, name + "_policies")())
        table = capi.Table(lt.blob)
        try:
            for n, m in shapes:
                p, r, acts, aux = _halves_of(name, n, m, seed=31)
                h, po, ro, act = _halves(lt, p, r, acts, aux)
                names |= _same(table, h, n, m, act, po, ro, flag_seq=(0, capi.F_WANT_DERIVED_ROLES, capi.F_LENIENT_SCOPE_SEARCH))
        finally:
            table.close()
    return names


def check_against_oracle(capi):
    """C2 at 23 x 17: the planes against oracle/ccheck run on the host-built product, and a corner of the cube against oracle/check.py
    on explicit CheckInputs"""
    from cerbos_amd.policy.loader import policies_from_docs
    from cerbos_amd.ruletable.build import rule_table_from_policies
    from oracle import ccheck
    from oracle.check import EvalParams, RuleTableOracle
    docs = workloads.c2_policies()
    lt = _lower(docs)
    n, m = 23, 17
    p, r, acts, aux = _halves_of("c2", n, m, seed=9)
    fl, table = Flattener(lt), capi.Table(lt.blob)
    cb = cross_product_batch(fl, lt.columns, p, r, acts, aux)
    cs = cross_direct_upload(table, fl, lt.columns, p, r, acts, aux)
    try:
        assert cs is not None
        _named_x(cs.describe(0))
        allow, flagged = cs.check(0, m, now_ns=NOW, want_flagged=True)
        want = ccheck.check(lt, cb, NOW, 0, threads=min(4, os.cpu_count() or 1))
        assert (want.status != capi.ST_UNSUPPORTED).all()
        a = len(acts)
        for k in range(a):
            assert np.array_equal(allow[k], _words(want.effect.reshape(m, n, a)[:, :, k] == ALLOW)), k
            assert np.array_equal(flagged[k], _words(want.status.reshape(m, n, a)[:, :, k] != 0)), k
        cube = allow_cube_planes(cs, 0, m, allow)
        assert np.array_equal(cube, effect_cube(cb, want) == ALLOW)
        orc = RuleTableOracle(rule_table_from_policies(policies_from_docs(docs)))
        for i in range(6):
            for j in range(5):
                out = orc.check({"principal": p[i], "resource": r[j], "actions": acts, **({"auxData": aux[i]} if aux[i] else {})}, EvalParams(now_ns=NOW))
                assert [out["actions"][x]["effect"] == "EFFECT_ALLOW" for x in acts] == list(cube[i, j]), (i, j)
    finally:
        if cs is not None:
            cs.close()
        table.close()


def check_geometry(capi):
    """N = 1, M = 1, A = 1 .. 4, N at, one past and beyond the wave and the workgroup; sorted and unsorted; orders random, reversed,
    one of them only"""
    lt = _lower(workloads.c2_policies())
    table = capi.Table(lt.blob)
    rng = np.random.default_rng(17)
    try:
        for n, m, a in ((1, 50, 4), (50, 1, 4), (1, 1, 1), (64, 3, 2), (65, 3, 3), (130, 5, 1), (257, 2, 4)):
            p, r, acts, aux = _halves_of("c2", n, m, seed=40 + n)
            for sort in (True, False):
                h, po, ro, act = _halves(lt, p, r, acts[:a], aux, sort=sort)
                _same(table, h, n, m, act, po, ro)
            h, _, _, act = _halves(lt, p, r, acts[:a], aux, sort=False)
            for po, ro in ((rng.permutation(n), rng.permutation(m)), (np.arange(n)[::-1], np.arange(m)[::-1]), (rng.permutation(n), None),
                           (None, rng.permutation(m)), (None, None)):
                _same(table, h, n, m, act, po, ro)
    finally:
        table.close()


def check_tiles(capi):
    """C2 at 67 x 13 as [0, 3), [3, 4), [4, 13) equals the whole (both against the reference); an empty range, r_end > M and a short
    buffer fail, and the buffers stay untouched"""
    lt = _lower(workloads.c2_policies())
    table = capi.Table(lt.blob)
    n, m = 67, 13
    p, r, acts, aux = _halves_of("c2", n, m, seed=5)
    h, po, ro, act = _halves(lt, p, r, acts, aux)
    try:
        _same(table, h, n, m, act, po, ro, tiles=((0, 3), (3, 4), (4, 13), (0, 13)))
        rng = np.random.default_rng(29)                                        # ... and with shuffled orders: the tiles' cubes
        _same(table, h, n, m, act, rng.permutation(n), rng.permutation(m), tiles=((0, 3), (3, 4), (4, 13), (2, 11)))
        cs = _direct(table, h, n, m, act, po, ro)
        whole, _ = cs.check(0, m, now_ns=NOW)
        parts = [cs.check(lo, hi, now_ns=NOW)[0] for lo, hi in ((0, 3), (3, 4), (4, 13))]
        bits = [np.unpackbits(np.ascontiguousarray(x).view(np.uint8).reshape(len(act), -1), axis=1, bitorder="little") for x in parts + [whole]]
        sizes = [n * 3, n, n * 9]
        assert np.array_equal(np.concatenate([b[:, :s] for b, s in zip(bits, sizes)], axis=1), bits[3][:, :n * m])
        for lo, hi in ((4, 4), (5, 3), (0, m + 1), (m, m + 1)):
            with pytest.raises(capi.HipEngineError) as e:
                cs.check(lo, hi, now_ns=NOW)
            assert str(e.value)
        w = cs.words(0, m)
        for want_flagged in (False, True):
            short = (np.full((len(act), w - 1), FILL, dtype=np.uint64), np.full((len(act), w - 1), FILL, dtype=np.uint64))
            with pytest.raises(capi.HipEngineError) as e:
                cs.check(0, m, now_ns=NOW, want_flagged=want_flagged, into=short)
            assert str(e.value) and (short[0] == FILL).all() and (short[1] == FILL).all()
        longer = (np.full((len(act), w + 3), FILL, dtype=np.uint64), np.full((len(act), w + 3), FILL, dtype=np.uint64))
        got, gf = cs.check(0, m, now_ns=NOW, want_flagged=True, into=longer)      # planes wider than the tile: the rest is left alone
        assert np.array_equal(got, whole) and (longer[0][:, w:] == FILL).all() and (longer[1][:, w:] == FILL).all() and gf.shape == got.shape
        assert np.array_equal(cs.check(0, m, now_ns=NOW)[0], whole)               # ... and the set still serves
        cs.close()
    finally:
        table.close()


COLUMN_DOCS = [{"apiVersion": API, "resourcePolicy": {"resource": "doc", "version": "default", "rules": [
    {"actions": ["view"], "roles": ["user"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": "R.attr.owner == P.id"}}},
    {"actions": ["edit"], "roles": ["user", "manager"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": "P.id in R.attr.viewers"}}},
    {"actions": ["delete"], "roles": ["manager"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": "P.attr.level >= 3.5"}}},
    {"actions": ["approve"], "roles": ["manager", "admin"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": "R.attr.amount > 100.5"}}},
    {"actions": ["view"], "roles": ["guest"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": 'P.attr.department == "eng"'}}},
    {"actions": ["edit"], "roles": ["guest", "admin"], "effect": "EFFECT_DENY", "condition": {"match": {"expr": 'R.attr.status == "OPEN"'}}},
    {"actions": ["edit"], "roles": ["admin"], "effect": "EFFECT_ALLOW"},
    {"actions": ["approve"], "roles": ["user"], "effect": "EFFECT_ALLOW", "condition": {"match": {"any": {"of": [
        {"expr": 'P.attr.department == "ops"'}, {"expr": 'R.attr.status == "CLOSED"'}, {"expr": "R.attr.amount > 50.5"}]}}}},
    {"actions": ["delete"], "roles": ["auditor"], "effect": "EFFECT_ALLOW", "condition": {"match": {"all": {"of": [
        {"expr": "P.attr.level >= 1.5"}, {"expr": "R.attr.owner == P.id"}, {"expr": 'P.attr.team == "core"'}, {"expr": "R.attr.public == true"}]}}}},
]}}]


def _column_halves(n, m, rng):
    roles = ["user", "manager", "admin", "guest", "auditor"]
    ps, rs = [], []
    for i in range(n):
        attr = {"level": float(rng.integers(1, 6)) + 0.25, "department": str(rng.choice(["eng", "ops"])), "team": str(rng.choice(["core", "edge"]))}
        for k in list(attr):
            if rng.random() < 0.15:
                del attr[k]            # absent on some rows: a CEL error where a rule reads it
        ps.append({"id": "p%d" % (i % 7), "roles": [str(x) for x in rng.choice(roles, size=int(rng.integers(1, 4)), replace=False)], "attr": attr})
    ps[0]["roles"] = []                # one principal without a role ...
    ps[1]["roles"] = roles[:4]         # ... and one with four
    for j in range(m):
        attr = {"owner": "p%d" % rng.integers(0, 7), "viewers": ["p%d" % v for v in rng.choice(7, size=int(rng.integers(0, 4)), replace=False)],
                "amount": float(rng.integers(0, 200)) + 0.5, "status": str(rng.choice(["OPEN", "CLOSED"])), "public": bool(rng.random() < 0.5)}
        for k in list(attr):
            if rng.random() < 0.15:
                del attr[k]
        rs.append({"kind": "doc", "id": "d%d" % j, "attr": attr})
    return ps, rs


def check_columns(capi, mode=None):
    """`mode`: None - the table's own plan (the record walk, MODE 0); "staged" - the process runs under CBH_FORCE_STAGED=1 (MODE 1);
    "masks" - under CBH_FLAT_MASKS=1: the table has a membership leaf, so its plan is cbh_check_flat_kernel_any_masks, which has
    NO direct form - cbh_cross_upload returns 1 and the materialised road serves.
    A hand-written flat policy set: leaves whose operands come from different halves (R.attr.owner == P.id, P.id in R.attr.viewers),
    a double threshold and a string equality on each side, one-level any / all trees mixing both sides; a group of four cached
    columns that mixes sides; on each side a column with high words and a narrow one; attributes absent on some rows of either side
    (flagged has ones); a principal without a role and one with four"""
    lt = _lower(COLUMN_DOCS)
    assert lt.stats["flat"], lt.stats
    roots = [root for root, _ in lt.columns]
    groups = [set("R" if x == "R" else "P" for x in roots[g:g + 4]) for g in range(0, min(len(roots), 16), 4)]
    assert any(len(g) == 2 for g in groups), roots                               # a group of four mixes sides
    rng = np.random.default_rng(23)
    n, m = 70, 9
    ps, rs = _column_halves(n, m, rng)
    acts = ["view", "edit", "delete", "approve"]
    table = capi.Table(lt.blob)
    try:
        if mode == "masks":
            h, po, ro, act = _halves(lt, ps, rs, acts)
            db = upload_halves(table, h, n, m, act, po, ro)
            assert table.plan(db) == "cbh_check_flat_kernel_any_masks", table.plan(db)
            db.close()
            assert direct_upload_halves(table, h, n, m, act, po, ro) is None and "no direct form" in table_error()
            return
        for sort in (True, False):
            h, po, ro, act = _halves(lt, ps, rs, acts, sort=sort)
            # per side: a column whose values have high words (the doubles) and one that is narrow (string ids, bools)
            wide = [(h.col_val[c] >> np.uint64(32)).any() for c in range(len(roots))]
            for side in ("R", "P"):
                mine = [w for w, root in zip(wide, roots) if (root == "R") == (side == "R")]
                assert any(mine) and not all(mine), (side, roots, wide)
            names = _same(table, h, n, m, act, po, ro, flag_seq=(0, capi.F_LENIENT_SCOPE_SEARCH))
            assert names == {"cbh_check_flat_kernel_staged_x" if mode == "staged" else "cbh_check_flat_kernel_x"}, names
            cs = _direct(table, h, n, m, act, po, ro)
            allow, flagged = cs.check(0, m, now_ns=NOW, want_flagged=True)
            cs.close()
            assert flagged.any() and allow.any() and not (allow & flagged).all()
        h, po, ro, act = _halves(lt, ps[:5], (rs * 8)[:70], acts)                   # 5 x 70: a wave spans thirteen resources
        _same(table, h, 5, 70, act, po, ro)
    finally:
        table.close()


# flat fuzz stores (tests/test_flat_kernel.py _store / _requests) at 40 x 11.  The seeds were chosen on the CPU: those whose plan for the
# materialised product contains "[compact inputs" and whose table has no derived roles (_qualifies over range(60), the first twelve
# of the shallow family and the first six of the deep one).
# EVERY one of them must go direct.
FUZZ_SEEDS = (4, 5, 10, 12, 14, 15, 16, 18, 23, 24, 26, 27)
DEEP_SEEDS = (0, 1, 2, 8, 12, 13)


def _fuzz_case(seed, deep=False):
    import test_flat_kernel as tfk
    rng = np.random.default_rng((73_000 if deep else 71_000) + seed)
    docs = tfk._store(rng, deep=deep)
    sample = tfk._requests(rng, 51, deep=deep)
    ps, rs = [s["principal"] for s in sample[:40]], [s["resource"] for s in sample[40:]]
    return docs, ps, rs, tfk.ACTIONS[:4]


def _qualifies(capi, seed, deep=False):
    docs, ps, rs, acts = _fuzz_case(seed, deep)
    if any("derivedRoles" in d for d in docs):
        return False
    lt = _lower(docs)
    table = capi.Table(lt.blob)
    h, po, ro, act = _halves(lt, ps, rs, acts)
    db = upload_halves(table, h, 40, 11, act, po, ro)
    try:
        return "[compact inputs" in table.plan(db)
    finally:
        db.close()
        table.close()


def check_fuzz(capi, seeds):
    assert seeds
    for seed in seeds:
        docs, ps, rs, acts = _fuzz_case(seed)
        lt = _lower(docs)
        table = capi.Table(lt.blob)
        try:
            h, po, ro, act = _halves(lt, ps, rs, acts, sort=seed % 2 == 0)
            _same(table, h, 40, 11, act, po, ro, flag_seq=(0, capi.F_LENIENT_SCOPE_SEARCH))
        finally:
            table.close()


def check_scopes(capi, seeds):
    """flat tables with scope chains more than three deep (the deep family of tests/test_flat_kernel.py): exact and lenient search"""
    assert seeds
    for seed in seeds:
        docs, ps, rs, acts = _fuzz_case(seed, deep=True)
        lt = _lower(docs)
        assert max(len(s.split(".")) for s in lt.scopes if s) >= 3
        table = capi.Table(lt.blob)
        try:
            h, po, ro, act = _halves(lt, ps, rs, acts)
            _same(table, h, 40, 11, act, po, ro, flag_seq=(0, capi.F_LENIENT_SCOPE_SEARCH, capi.F_LENIENT_SCOPE_SEARCH | capi.F_WANT_DERIVED_ROLES))
        finally:
            table.close()


def check_refusals(capi):
    """cbh_cross_upload returns exactly 1 with *out NULL where the set has no direct form; cbh_cross_check returns 1 under strict
    evaluation; null arguments, a non-permutation, a table other than the set's fail with a text"""
    import ctypes as C
    lib = capi.load()

    def raw(table, h, n, m, act, po=None, ro=None, null=None):
        a_ids = np.ascontiguousarray(act, dtype=np.uint32)
        pa = None if po is None else np.ascontiguousarray(po, dtype=np.uint32)
        ra = None if ro is None else np.ascontiguousarray(ro, dtype=np.uint32)
        cb = capi.make_cbatch(h, table.num_columns)
        x = capi.CCross(n, m, a_ids.size, a_ids.ctypes.data if a_ids.size else None, pa.ctypes.data if pa is not None else None,
                        ra.ctypes.data if ra is not None else None)
        out = C.c_void_p(0xDEAD)
        rc = lib.cbh_cross_upload(None if null == "table" else table.h, 0, None if null == "halves" else C.byref(cb),
                                  None if null == "cross" else C.byref(x), None if null == "out" else C.byref(out))
        return rc, out

    def no_direct_form(lt, ps, rs, acts, aux=None, patch=None):
        table = capi.Table(lt.blob)
        h, po, ro, act = _halves(lt, ps, rs, acts, aux)
        if patch:
            patch(h)
        rc, out = raw(table, h, len(ps), len(rs), act, po, ro)
        assert rc == 1 and not out.value and lib.cbh_last_error(), rc
        assert table.cross_upload(h, len(ps), len(rs), act, po, ro) is None
        db = upload_halves(table, h, len(ps), len(rs), act, po, ro)          # the materialised road takes it
        table.launch(db, now_ns=NOW)
        assert table.download(db).effect.size == len(ps) * len(rs) * len(act)
        db.close()
        table.close()

    for name in ("c3", "c5"):                                                 # derived roles; not flat
        p, r, acts, aux = _halves_of(name, 6, 5, seed=3)
        no_direct_form(_lower(getattr(workloads, name + "_policies")()), p, r, acts, aux)
    lt = _lower(workloads.c2_policies())
    p, r, acts, aux = _halves_of("c2", 6, 5, seed=3)
    no_direct_form(lt, p, r, acts + ["extra"], aux)                           # A = 5
    p5 = [dict(x) for x in p]
    p5[2] = dict(p5[2], roles=["employee", "manager", "admin", "contractor", "auditor"])
    no_direct_form(lt, p5, r, acts, aux)                                      # a five-role principal
    lt_cols = _lower(COLUMN_DOCS)
    ps, rs = _column_halves(6, 5, np.random.default_rng(3))
    amount = [i for i, (root, path) in enumerate(lt_cols.columns) if root == "R" and "amount" in str(path)]
    assert len(amount) == 1, lt_cols.columns

    def an_int(h):      # an int where a rule compares a double (JSON brings none: set at the ABI's level): the `_any` variant
        h.col_tag[amount[0], len(ps) + 1], h.col_val[amount[0], len(ps) + 1] = 2, 7      # flatten.T_INT
    no_direct_form(lt_cols, ps, rs, ["view", "edit", "delete", "approve"], patch=an_int)

    table, other = capi.Table(lt.blob), capi.Table(lt.blob)
    h, po, ro, act = _halves(lt, p, r, acts, aux)
    try:
        for what in ("table", "halves", "cross", "out"):
            rc, out = raw(table, h, 6, 5, act, po, ro, null=what)
            assert rc < 0 and lib.cbh_last_error() and (what == "out" or not out.value), what
        for bad_po, bad_ro in (([0, 1, 2, 3, 4, 4], ro), ([0, 1, 2, 3, 4, 6], ro), (po, [1, 1, 2, 3, 4])):
            rc, out = raw(table, h, 6, 5, act, bad_po, bad_ro)
            assert rc < 0 and not out.value and b"permutation" in lib.cbh_last_error()
        rc, out = raw(table, h, 5, 5, act)                                    # n_requests != N + M
        assert rc < 0 and not out.value
        cs = _direct(table, h, 6, 5, act, po, ro)
        _named_x(cs.describe(0))
        assert cs.describe(capi.F_STRICT_EVALUATION).startswith("none")
        with pytest.raises(capi.DirectFormUnavailable):
            cs.check(0, 5, flags=capi.F_STRICT_EVALUATION, now_ns=NOW)
        w = cs.words(0, 5)
        buf = np.full((len(act), w), FILL, dtype=np.uint64)
        prm = capi.CParams(NOW, capi.F_STRICT_EVALUATION, 0)
        assert lib.cbh_cross_check(table.h, cs.h, C.byref(prm), 0, 5, buf.ctypes.data, None, w) == 1 and (buf == FILL).all()
        prm = capi.CParams(NOW, 0, 0)
        assert lib.cbh_cross_check(other.h, cs.h, C.byref(prm), 0, 5, buf.ctypes.data, None, w) < 0 and lib.cbh_last_error()   # another table
        assert lib.cbh_cross_check(None, cs.h, C.byref(prm), 0, 5, buf.ctypes.data, None, w) < 0
        assert lib.cbh_cross_check(table.h, None, C.byref(prm), 0, 5, buf.ctypes.data, None, w) < 0
        assert lib.cbh_cross_check(table.h, cs.h, None, 0, 5, buf.ctypes.data, None, w) < 0
        assert lib.cbh_cross_check(table.h, cs.h, C.byref(prm), 0, 5, None, None, w) < 0
        for lo, hi in ((3, 3), (4, 2), (0, 6), (5, 6)):                         # an empty range, r_end > M: the library's own check
            assert lib.cbh_cross_check(table.h, cs.h, C.byref(prm), lo, hi, buf.ctypes.data, None, w) < 0, (lo, hi)
            assert b"non-empty range" in lib.cbh_last_error(), lib.cbh_last_error()
        assert lib.cbh_cross_check(table.h, cs.h, C.byref(prm), 0, 5, buf.ctypes.data, None, w - 1) < 0 and b"words_per_plane" in lib.cbh_last_error()
        assert (buf == FILL).all()
        assert lib.cbh_cross_check(table.h, cs.h, C.byref(prm), 0, 5, buf.ctypes.data, None, w) == 0 and not (buf == FILL).all()
        lib.cbh_cross_release(None)
        cs.close()
    finally:
        table.close()
        other.close()


STAGED_BODY = r'''
import numpy as np
from cerbos_amd import workloads
import test_cross_direct as td
lt = td._lower(workloads.c2_policies())
table = capi.Table(lt.blob)
p, r, acts, aux = td._halves_of("c2", 70, 9, seed=31)
h, po, ro, act = td._halves(lt, p, r, acts, aux)
names = td._same(table, h, 70, 9, act, po, ro, flag_seq=(0, capi.F_LENIENT_SCOPE_SEARCH))
assert names == {"cbh_check_flat_kernel_staged_x"}, names
table.close()
print("staged ok")
'''


COLUMNS_BODY = r'''
import test_cross_direct as td
td.check_columns(capi, mode=%r)
print("columns ok")
'''
COLUMN_MODES = (("staged", {"CBH_FORCE_STAGED": "1"}), ("masks", {"CBH_FLAT_MASKS": "1"}))


def _gpu_child(body, env, ok):
    """the library reads its switches once per process: a process of its own, as tests/test_gpu_pre_split_modes.py runs one per mode"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    here = os.path.join(root, "tests")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, here, os.environ.get("PYTHONPATH", "")]), **env)
    r = subprocess.run([sys.executable, "-c", "from cerbos_amd import capi\n" + body], env=env, capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0 and ok in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def check_modes(names):
    """between the workloads, MODE 0 and 2 were each named (MODE 1: the child process with CBH_FORCE_STAGED=1)"""
    assert "cbh_check_flat_kernel_x" in names and "cbh_check_flat_kernel_masks_x" in names, names


# ---- CPU tier: the simulator


@pytest.fixture()
def engine():
    with sim_engine() as capi:
        yield capi


def test_workloads_on_simulator(engine):
    check_modes(check_workloads(engine))


def test_staged_walk_on_simulator():
    import test_sim_engine as ts
    ts._in_own_process(STAGED_BODY, {"CBH_FORCE_STAGED": "1"})


def test_against_oracle_on_simulator(engine):
    check_against_oracle(engine)


def test_geometry_on_simulator(engine):
    check_geometry(engine)


def test_tiles_on_simulator(engine):
    check_tiles(engine)


def test_columns_on_simulator(engine):
    check_columns(engine)


@pytest.mark.parametrize("mode,env", COLUMN_MODES)
def test_columns_by_the_other_walks_on_simulator(mode, env):
    import test_sim_engine as ts
    ts._in_own_process(COLUMNS_BODY % mode, env)


def test_the_listed_seeds_qualify(engine):
    """every seed of FUZZ_SEEDS / DEEP_SEEDS: no derived roles, and the plan of the materialised product reads compact inputs"""
    assert all(_qualifies(engine, seed) for seed in FUZZ_SEEDS) and all(_qualifies(engine, seed, deep=True) for seed in DEEP_SEEDS)


def test_fuzz_on_simulator(engine):
    check_fuzz(engine, FUZZ_SEEDS)


def test_scopes_on_simulator(engine):
    check_scopes(engine, DEEP_SEEDS)


def test_refusals_on_simulator(engine):
    check_refusals(engine)


def test_failing_allocations_and_copies_are_survived():
    """Fault injection (simulator only): the k-th device allocation - or asynchronous copy - from now on fails, for every k until the
    calls succeed; cbh_cross_upload and cbh_cross_check either report an error with a text or give the right planes, and a set
    whose check failed decides correctly afterwards."""
    import test_sim_engine as ts
    ts._in_own_process('''
import ctypes as C
import numpy as np
from cerbos_amd import workloads
from cerbos_amd.cross import direct_upload_halves
import test_cross_direct as td
NOW = td.NOW
lib = capi.load()
lib.cbh_sim_set_alloc_budget.argtypes = [C.c_long]
lib.cbh_sim_set_copy_budget.argtypes = [C.c_long]
lt = td._lower(workloads.c2_policies())
p, r, acts, aux = td._halves_of("c2", 9, 7, seed=4)
h, po, ro, act = td._halves(lt, p, r, acts, aux)
ref = capi.Table(lt.blob)
cs = direct_upload_halves(ref, h, 9, 7, act, po, ro)
want, want_f = cs.check(0, 7, now_ns=NOW, want_flagged=True)
cs.close()
for setter in (lib.cbh_sim_set_alloc_budget, lib.cbh_sim_set_copy_budget):
    for phase in ("upload", "check"):
        failed = 0
        for k in range(200):
            table = capi.Table(lt.blob)          # (a fresh table: empty pools, every buffer a real allocation)
            cs = None
            if phase == "check":
                cs = direct_upload_halves(table, h, 9, 7, act, po, ro)
            setter(k)
            try:
                if phase == "upload":
                    cs = direct_upload_halves(table, h, 9, 7, act, po, ro)
                else:
                    cs.check(0, 7, now_ns=NOW, want_flagged=True)
            except capi.HipEngineError as e:
                assert str(e), "an error without a message"
                failed += 1
            finally:
                setter(-1)
            if cs is None:                        # allowed again: as if nothing had happened
                cs = direct_upload_halves(table, h, 9, 7, act, po, ro)
            got, got_f = cs.check(0, 7, now_ns=NOW, want_flagged=True)      # the set is usable after a failed check
            assert np.array_equal(got, want) and np.array_equal(got_f, want_f)
            part, _ = cs.check(2, 5, now_ns=NOW)
            assert part.shape[1] == cs.words(2, 5)
            cs.close()
            table.close()
            if failed == k:                       # the k-th was not reached: the call had enough
                break
        assert failed >= (10 if phase == "upload" else 1) and failed == k, (phase, failed, k)
ref.close()
''', {})


# ---- GPU tier


@pytest.mark.gpu
def test_workloads_on_gpu():
    from cerbos_amd import capi
    check_modes(check_workloads(capi))


@pytest.mark.gpu
def test_staged_walk_on_gpu():
    """CBH_FORCE_STAGED is read once per process: a process of its own, as tests/test_gpu_pre_split_modes.py runs one per mode"""
    if os.environ.get("CBH_TEST_SIM_ENGINE"):
        return test_staged_walk_on_simulator()
    _gpu_child(STAGED_BODY, {"CBH_FORCE_STAGED": "1"}, "staged ok")


@pytest.mark.gpu
def test_against_oracle_on_gpu():
    from cerbos_amd import capi
    check_against_oracle(capi)


@pytest.mark.gpu
def test_geometry_on_gpu():
    from cerbos_amd import capi
    check_geometry(capi)


@pytest.mark.gpu
def test_tiles_on_gpu():
    from cerbos_amd import capi
    check_tiles(capi)


@pytest.mark.gpu
def test_columns_on_gpu():
    from cerbos_amd import capi
    check_columns(capi)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,env", COLUMN_MODES)
def test_columns_by_the_other_walks_on_gpu(mode, env):
    if os.environ.get("CBH_TEST_SIM_ENGINE"):
        return test_columns_by_the_other_walks_on_simulator(mode, env)
    _gpu_child(COLUMNS_BODY % mode, env, "columns ok")


@pytest.mark.gpu
def test_fuzz_on_gpu():
    from cerbos_amd import capi
    check_fuzz(capi, FUZZ_SEEDS)


@pytest.mark.gpu
def test_scopes_on_gpu():
    from cerbos_amd import capi
    check_scopes(capi, DEEP_SEEDS)


@pytest.mark.gpu
def test_refusals_on_gpu():
    from cerbos_amd import capi
    check_refusals(capi)


@pytest.mark.gpu
def test_beyond_the_materialised_limit_on_gpu():
    """N = M = 65 536 (2^32 pairs: cbh_batch_upload_cross refuses the product): the halves are 1 024 flattened C2 rows per side tiled
    with numpy; the direct set decides the tiles [0, 8) and [65 528, 65 536), each equal to the materialised product of those eight
    resources with the same principals"""
    from cerbos_amd import capi
    lt = _lower(workloads.c2_policies())
    base, big = 1024, 65536
    p, r, acts, aux = _halves_of("c2", base, base, seed=13)
    h, _, _, act = _halves(lt, p, r, acts, aux, sort=False)
    rep = big // base
    rows = np.concatenate([np.tile(np.arange(base), rep), base + np.tile(np.arange(base), rep)])      # halves rows of the big set
    hb = _take_rows(h, rows)
    table = capi.Table(lt.blob)
    try:
        with pytest.raises(capi.HipEngineError) as e:
            table.upload_cross(hb, big, big, act)
        assert "2^32" in str(e.value)
        cs = _direct(table, hb, big, big, act, None, None)
        _named_x(cs.describe(0))
        for lo in (0, big - 8):
            allow, flagged = cs.check(lo, lo + 8, now_ns=NOW, want_flagged=True)
            tile = _take_rows(hb, np.concatenate([np.arange(big), big + np.arange(lo, lo + 8)]))
            want_a, want_f, _, _ = _reference(table, tile, big, 8, act, None, None, 0)
            for k in range(len(act)):
                assert np.array_equal(allow[k], _words(want_a[:, :, k])), (lo, k)
                assert np.array_equal(flagged[k], _words(want_f[:, :, k])), (lo, k)
            assert 0.01 < np.unpackbits(allow.view(np.uint8)).mean() < 0.99
        cs.close()
    finally:
        table.close()


def _take_rows(h, rows):
    """a halves batch of the given rows of `h` (roles, heap and strings shared as they are)"""
    import copy
    b = copy.copy(h)
    b.n_requests = int(rows.size)
    b.req_u32 = np.ascontiguousarray(h.req_u32[:, rows])
    b.col_tag = np.ascontiguousarray(h.col_tag[:, rows])
    b.col_val = np.ascontiguousarray(h.col_val[:, rows])
    for f in ("vreq_input", "req_perm", "tuple_perm"):
        if getattr(b, f, None) is not None:
            setattr(b, f, None)
    return b
