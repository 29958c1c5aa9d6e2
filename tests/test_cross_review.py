"""The review of a direct set (cerbos_hip.h cbh_cross_review; cbh_cross.h cbh_cross_review_*_kernel): counts per principal, per
resource and per action, and ordered pair lists, reduced on the device from the planes the `_x` kernels leave there.

The reference in every body is the planes of cs.check(lo, hi, want_flagged=True) on the SAME set, reduced with plain numpy
(unpackbits -> reshape(a, mt, n) -> sum), and cross.flagged_pairs for the lists; that road is itself pinned against the
materialised product and the oracles (tests/test_cross_direct*.py).  Every output of the review must equal that reduction exactly.
CPU tier: the library's host side and the kernels' source on the simulator (tests/sim_engine.py).  GPU tier: the same bodies on the device."""
import ctypes as C

import numpy as np
import pytest

from cerbos_amd import workloads
from cerbos_amd.cross import allow_cube_planes, flagged_pairs, review_counts
from sim_engine import sim_engine
from test_cross_device import NOW, _halves_of, _lower
from test_cross_direct import FILL, _halves, _named_x, _take_rows, check_modes
import test_cross_direct_ex as tx
import test_cross_direct_roles as tr

FILL32 = 0x5A5A5A5A


# ---- the reference: the planes of a check, reduced on the host


def _bits(planes, a, mt, n):
    by = np.ascontiguousarray(planes, dtype="<u8").view(np.uint8).reshape(a, -1)
    return np.unpackbits(by, axis=1, count=n * mt, bitorder="little").reshape(a, mt, n)


class _Ref:
    """what a caller computes today from the planes of one check: counts in device order and, per kind, the full pair list"""

    def __init__(self, cs, lo, hi, flags):
        n, _, a = cs.shape
        self.planes = {}
        self.planes["allowed"], self.planes["flagged"] = cs.check(lo, hi, flags=flags, now_ns=NOW, want_flagged=True)
        ab, fb = (_bits(self.planes[k], a, hi - lo, n) for k in ("allowed", "flagged"))
        self.allow_by_principal, self.flagged_by_principal = ab.sum(axis=1, dtype=np.uint32), fb.sum(axis=1, dtype=np.uint32)
        self.allow_by_resource, self.flagged_by_resource = ab.sum(axis=2, dtype=np.uint32), fb.sum(axis=2, dtype=np.uint32)
        self.totals = np.stack([ab.sum(axis=(1, 2), dtype=np.uint64), fb.sum(axis=(1, 2), dtype=np.uint64)])
        self.lists = {k: flagged_pairs(cs, lo, hi, self.planes[k]) for k in self.planes}     # (the decoding is the same for either kind)

    def pairs(self, kind, sel=None):
        """the pairs with a set bit among the actions `sel`; the mask keeps every action's bit"""
        pp, pr, mask = self.lists[kind]
        if sel is None:
            return pp, pr, mask
        keep = (mask & np.uint64(sum(1 << k for k in sel))) != 0
        return pp[keep], pr[keep], mask[keep]


def _counts_equal(rv, ref, what):
    for f in ("allow_by_principal", "allow_by_resource", "flagged_by_principal", "flagged_by_resource", "totals"):
        got, want = getattr(rv, f), getattr(ref, f)
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (what, f)


def _list_equal(rv, want, what):
    pp, pr, mask = want
    assert rv.n_pairs == pp.size, (what, rv.n_pairs, pp.size)
    assert np.array_equal(rv.pair_p, pp) and np.array_equal(rv.pair_r, pr) and np.array_equal(rv.pair_mask, mask), what
    assert rv.pair_p.dtype == np.uint32 and rv.pair_r.dtype == np.uint32 and rv.pair_mask.dtype == np.uint64


def _review_equals(cs, lo, hi, flags=0, tile=0, sels=(None,)):
    """one review with every count and, per kind and selection, one with the list, against the reduced planes; returns the reference"""
    ref = _Ref(cs, lo, hi, flags)
    rv = cs.review(lo, hi, flags=flags, now_ns=NOW, want_flagged=True, tile_resources=tile)
    _counts_equal(rv, ref, (lo, hi, flags, tile))
    assert rv.pair_p is None and rv.n_pairs == 0
    only = cs.review(lo, hi, flags=flags, now_ns=NOW, tile_resources=tile)               # without the flagged counts
    assert only.flagged_by_principal is None and only.flagged_by_resource is None
    assert np.array_equal(only.allow_by_principal, ref.allow_by_principal) and np.array_equal(only.totals, ref.totals)
    for kind in ("flagged", "allowed"):
        for sel in sels:
            rv = cs.review(lo, hi, flags=flags, now_ns=NOW, want_flagged=True, pairs=kind, pair_actions=sel, tile_resources=tile)
            _counts_equal(rv, ref, (lo, hi, flags, tile, kind, sel))
            _list_equal(rv, ref.pairs(kind, sel), (lo, hi, flags, tile, kind, sel))
    return ref


def _in_callers_orders(cs, lo, hi, flags=0):
    """review_counts against the cubes of allow_cube_planes: counts by the caller's principal and by the tile's resources in the
    caller's resource order, the pairs as caller indices"""
    n, _, a = cs.shape
    ref = _Ref(cs, lo, hi, flags)
    res = np.sort(np.asarray(cs.r_order)[lo:hi])                                          # the tile's resources, caller's order
    for kind in ("allowed", "flagged"):
        cube = allow_cube_planes(cs, lo, hi, ref.planes[kind])                            # [i][j][k]
        out = review_counts(cs, lo, hi, cs.review(lo, hi, flags=flags, now_ns=NOW, want_flagged=True, pairs=kind))
        by_p, by_r = (out.allow_by_principal, out.allow_by_resource) if kind == "allowed" else (out.flagged_by_principal, out.flagged_by_resource)
        assert by_p.shape == (n, a) and np.array_equal(by_p, cube.sum(axis=1)), kind
        assert by_r.shape == (hi - lo, a) and np.array_equal(by_r, cube.sum(axis=0)), kind
        i, j = np.nonzero(cube.any(axis=2))
        assert sorted(zip(out.pair_p.tolist(), out.pair_r.tolist())) == sorted(zip(i.tolist(), res[j].tolist())), kind
        for q in range(out.n_pairs):
            jj = int(np.searchsorted(res, out.pair_r[q]))
            assert int(out.pair_mask[q]) == sum(1 << k for k in range(a) if cube[out.pair_p[q], jj, k]), (kind, q)
        assert np.array_equal(out.totals, ref.totals)


# ---- the bodies: the same on the simulator and on the device


def check_workloads(capi):
    """C2 and T at 70 x 9 and 5 x 70, C4 at 70 x 9 under flags 0, want-derived-roles, lenient; C3 under CX_DERIVED_ROLES with the
    derived roles wanted: the case with flagged tuples.  Returns the kernels named."""
    names = set()
    want_c2 = {(70, 9): (672, (0, 265, 83, 324)), (5, 70): (288, None)}                   # allowed tuples, per action: by oracle/check.py
    for name, shapes in (("c2", ((70, 9), (5, 70))), ("t", ((70, 9), (5, 70))), ("c4", ((70, 9),))):
        lt = _lower(getattr(workloads, name + "_policies")())
        table = capi.Table(lt.blob)
        try:
            for n, m in shapes:
                p, r, acts, aux = _halves_of(name, n, m, seed=31)
                h, po, ro, act = _halves(lt, p, r, acts, aux)
                cs = tx._direct(table, h, n, m, act, po, ro, 0)
                for flags in (0, capi.F_WANT_DERIVED_ROLES, capi.F_LENIENT_SCOPE_SEARCH):
                    names.add(_named_x(cs.describe(flags)))
                    ref = _review_equals(cs, 0, m, flags)
                    assert 0 < int(ref.totals[0].max()) < n * m, ref.totals            # a kernel that writes zeros cannot pass
                    if name == "c2" and flags == 0:
                        total, per_action = want_c2[(n, m)]
                        assert int(ref.totals[0].sum()) == total and (per_action is None or tuple(int(x) for x in ref.totals[0]) == per_action), ref.totals
                        if (n, m) == (70, 9):
                            per_r = ref.allow_by_resource.sum(axis=0)
                            assert 0 < int(per_r.min()) < int(per_r.max()) == 133, per_r       # (14 .. 133: the resources differ)
                cs.close()
        finally:
            table.close()
    lt = _lower(workloads.c3_policies())
    table = capi.Table(lt.blob)
    flags = capi.F_WANT_DERIVED_ROLES
    try:
        for n, m in ((70, 9), (5, 70)):
            p, r, acts, aux = tx._c3(n, m)
            h, po, ro, act = _halves(lt, p, r, acts, aux)
            cs = tx._direct(table, h, n, m, act, po, ro, capi.CX_DERIVED_ROLES)
            assert _named_x(cs.describe(flags)) == tx.DR_X
            ref = _review_equals(cs, 0, m, flags, sels=(None, (1,)))
            assert 0 < int(ref.totals[0].max()) < n * m, ref.totals
            assert (n, m) != (70, 9) or 0 < int(ref.totals[1].max()) < n * m, ref.totals       # (5 x 70 has no flagged tuple)
            if (n, m) == (70, 9):
                assert int(ref.totals[0].sum()) == 684 and int(ref.totals[1].sum()) == 72, ref.totals
                assert (int(ref.allow_by_principal[0].min()), int(ref.allow_by_principal[0].max())) == (0, 7)
            _review_equals(cs, 0, m, 0)
            cs.close()
    finally:
        table.close()
    return names


def check_geometry(capi):
    """N and M of 1, N below, at and one past a word, two words and a bit, four words and a bit, 21 resources to a word; sorted and
    unsorted halves; orders random, reversed, one of them only; the counts and pairs in the caller's orders against the cube"""
    lt = _lower(workloads.c2_policies())
    table = capi.Table(lt.blob)
    rng = np.random.default_rng(17)
    seen = 0
    try:
        for n, m, a in ((1, 50, 4), (50, 1, 4), (1, 1, 1), (63, 5, 2), (64, 3, 2), (65, 3, 3), (130, 5, 1), (257, 2, 4), (3, 200, 4)):
            p, r, acts, aux = _halves_of("c2", n, m, seed=40 + n)
            acts = acts[1:] + acts[:1] if a < 4 else acts                                  # (action 0 allows nobody: not the only one)
            for sort in (True, False):
                h, po, ro, act = _halves(lt, p, r, acts[:a], aux, sort=sort)
                cs = tx._direct(table, h, n, m, act, po, ro, 0)
                seen += int(_review_equals(cs, 0, m).totals[0].sum())
                _in_callers_orders(cs, 0, m)
                cs.close()
            h, _, _, act = _halves(lt, p, r, acts[:a], aux, sort=False)
            for po, ro in ((rng.permutation(n), rng.permutation(m)), (np.arange(n)[::-1], np.arange(m)[::-1]), (rng.permutation(n), None),
                           (None, rng.permutation(m)), (None, None)):
                cs = tx._direct(table, h, n, m, act, po, ro, 0)
                _review_equals(cs, 0, m)
                _in_callers_orders(cs, 0, m)
                if m > 2:
                    _in_callers_orders(cs, 1, m - 1)
                cs.close()
        assert seen > 100
        # 65 words to a resource: a whole wave shares one, a lane takes one word or two (128 principals, repeated)
        n, m = 4100, 3
        p, r, acts, aux = _halves_of("c2", 128, m, seed=7)
        h, po, ro, act = _halves(lt, (p * 33)[:n], r, acts[1:3], (aux * 33)[:n])
        cs = tx._direct(table, h, n, m, act, po, ro, 0)
        assert 0 < int(_review_equals(cs, 0, m, tile=2).totals[0].max()) < n * m
        cs.close()
    finally:
        table.close()


RANGES = ((0, 13), (0, 3), (3, 4), (4, 13), (2, 11))
TILES = (0, 1, 2, 5, 13)


def check_tiles(capi):
    """C2 at 67 x 13: every range with every tile size gives the reference's counts and lists; three adjacent ranges add up to the
    whole; a check between two reviews and a review between two checks still give the right answer (the plane block is shared);
    nine actions in three groups; principals of 5 to 12 roles in role groups, with derived roles; both kinds of groups together"""
    lt = _lower(workloads.c2_policies())
    table = capi.Table(lt.blob)
    n, m = 67, 13
    p, r, acts, aux = _halves_of("c2", n, m, seed=5)
    h, po, ro, act = _halves(lt, p, r, acts, aux)
    try:
        cs = tx._direct(table, h, n, m, act, po, ro, 0)
        refs = {}
        for lo, hi in RANGES:
            for tile in TILES:
                refs[(lo, hi)] = _review_equals(cs, lo, hi, tile=tile, sels=(None, (3,)))
        assert int(refs[(0, 13)].totals[0].sum()) > 0
        parts = [cs.review(lo, hi, now_ns=NOW, want_flagged=True, pairs="allowed", tile_resources=2) for lo, hi in ((0, 3), (3, 4), (4, 13))]
        whole = cs.review(0, 13, now_ns=NOW, want_flagged=True, pairs="allowed")
        assert np.array_equal(sum(x.allow_by_principal for x in parts), whole.allow_by_principal)
        assert np.array_equal(np.concatenate([x.allow_by_resource for x in parts], axis=1), whole.allow_by_resource)
        assert np.array_equal(sum(x.totals for x in parts), whole.totals) and sum(x.n_pairs for x in parts) == whole.n_pairs
        for f in ("pair_p", "pair_r", "pair_mask"):
            assert np.array_equal(np.concatenate([getattr(x, f) for x in parts]), getattr(whole, f)), f
        # the plane block is shared: a larger tile, a smaller one, with and without the second set of planes, in turn
        want_a, want_f = cs.check(0, 13, now_ns=NOW, want_flagged=True)
        part_a, _ = cs.check(4, 13, now_ns=NOW)
        _counts_equal(cs.review(2, 11, now_ns=NOW, want_flagged=True, tile_resources=5), refs[(2, 11)], "between")
        got_a, got_f = cs.check(0, 13, now_ns=NOW, want_flagged=True)
        assert np.array_equal(got_a, want_a) and np.array_equal(got_f, want_f)
        _counts_equal(cs.review(0, 13, now_ns=NOW, want_flagged=True), refs[(0, 13)], "after a check")
        assert np.array_equal(cs.check(4, 13, now_ns=NOW)[0], part_a)
        _counts_equal(cs.review(3, 4, now_ns=NOW, want_flagged=True), refs[(3, 4)], "after a smaller check")
        cs.close()
        rng = np.random.default_rng(29)                                                   # ... and with shuffled orders
        cs = tx._direct(table, h, n, m, act, rng.permutation(n), rng.permutation(m), 0)
        for lo, hi in RANGES:
            _review_equals(cs, lo, hi, tile=2)
            _in_callers_orders(cs, lo, hi)
        cs.close()
        # nine actions: three launches per tile, planes [9][words]
        n, m = 70, 9
        p, r, acts, aux = _halves_of("c2", n, m, seed=31)
        names = tx._action_list(acts, 9)
        h, po, ro, act = _halves(lt, p, r, names, aux)
        cs = tx._direct(table, h, n, m, act, po, ro, capi.CX_ACTION_GROUPS)
        assert ", 3 action groups]" in cs.describe(0)
        for tile in (0, 4):
            ref = _review_equals(cs, 0, m, tile=tile, sels=(None, (4,), (2, 8)))
        assert ref.totals[0][4] > 0 and ref.totals[0][2] == 0                             # a known action behind the first group, an unknown one
        cs.close()
    finally:
        table.close()
    # role groups: derived roles, principals of 5 .. 12 roles (tests/test_cross_direct_roles.py _dr_halves)
    lt = _lower(tr._dr_docs())
    table = capi.Table(lt.blob)
    try:
        ps, rs = tr._dr_halves(70, 9, np.random.default_rng(23))
        h, po, ro, act = _halves(lt, ps, rs, tr.ACTS)
        cs = tx._direct(table, h, 70, 9, act, po, ro, capi.CX_DERIVED_ROLES | capi.CX_ROLE_GROUPS)
        assert tr._groups(cs.describe(0)) > 1
        for flags in (0, capi.F_WANT_DERIVED_ROLES):
            for tile in (0, 4):
                ref = _review_equals(cs, 0, 9, flags, tile=tile)
            assert ref.totals[0].any() and ref.totals[1].any()
        cs.close()
    finally:
        table.close()
    # ... and both kinds of groups: nine actions, nine roles (check_both_groups of that file)
    lt = _lower(tr.DIRECTED_DOCS)
    ps, rs = tr._directed_halves()
    ps = [dict(x, roles=x["roles"][:9]) for x in ps]
    table = capi.Table(lt.blob)
    try:
        h, po, ro, act = _halves(lt, ps, rs, tx._action_list(tr.ACTS, 9))
        cs = tx._direct(table, h, len(ps), len(rs), act, po, ro, capi.CX_ACTION_GROUPS | capi.CX_ROLE_GROUPS)
        assert cs.describe(0).endswith(", 3 action groups, 3 role groups]"), cs.describe(0)
        for tile in (0, 3):
            assert _review_equals(cs, 0, len(rs), tile=tile).totals[0].any()
        cs.close()
    finally:
        table.close()


class _Raw:
    """cbh_cross_review called as a C caller would: every out buffer painted, so that what a call wrote - and what it left - shows"""

    def __init__(self, capi, n, a, mr, cap):
        self.capi = capi
        self.by_p = [np.full((a, n), FILL32, dtype=np.uint32) for _ in range(2)]
        self.by_r = [np.full((a, mr), FILL32, dtype=np.uint32) for _ in range(2)]
        self.totals = np.full((2, a), FILL, dtype=np.uint64)
        self.pp, self.pr = np.full(cap + 3, FILL32, dtype=np.uint32), np.full(cap + 3, FILL32, dtype=np.uint32)
        self.pm = np.full(cap + 3, FILL, dtype=np.uint64)
        self.cap = cap

    def untouched(self, list_from=0):
        return all((x == FILL32).all() for x in self.by_p + self.by_r) and (self.totals == FILL).all() and self.list_untouched(list_from)

    def list_untouched(self, start):
        return (self.pp[start:] == FILL32).all() and (self.pr[start:] == FILL32).all() and (self.pm[start:] == FILL).all()

    def call(self, table_h, cs_h, lo, hi, flags=0, pairs=0, sel=0, tile=0, null_lists=False, null_params=False, null_rv=False, outputs=True):
        capi = self.capi
        ptr = lambda x: x.ctypes.data if outputs else None
        lists = (None, None, None) if null_lists else (self.pp.ctypes.data, self.pr.ctypes.data, self.pm.ctypes.data)
        self.rv = capi.CCrossReview(pairs, tile, sel, self.cap, ptr(self.by_p[0]), ptr(self.by_r[0]), ptr(self.by_p[1]), ptr(self.by_r[1]),
                                    ptr(self.totals), *lists, 0xDEAD)
        prm = capi.CParams(NOW, flags, 0)
        return capi.load().cbh_cross_review(table_h, cs_h, None if null_params else C.byref(prm), lo, hi, None if null_rv else C.byref(self.rv))


def check_pairs(capi):
    """On the C3 set at 70 x 9 under CBH_F_WANT_DERIVED_ROLES - both kinds of planes have ones -: the lists of both kinds for all
    actions, one action, two actions and an action nobody is allowed; caps of 0, 1 and n_pairs - 1 give 2, the reference's prefix and
    nothing behind the cap; n_pairs and more give 0; the flagged list through pairs_batch gives the full results of those pairs"""
    lt = _lower(workloads.c3_policies())
    table = capi.Table(lt.blob)
    n, m = 70, 9
    p, r, acts, aux = tx._c3(n, m)
    flags = capi.F_WANT_DERIVED_ROLES
    try:
        h, po, ro, act = _halves(lt, p, r, acts + ["zz0"], aux)                          # five actions; nobody is allowed the last
        a = len(act)
        cs = tx._direct(table, h, n, m, act, po, ro, capi.CX_ALL)
        ref = _review_equals(cs, 0, m, flags, sels=(None, (1,), (0, 3), (4,)))
        assert ref.totals[0][4] == 0 and ref.pairs("allowed", (4,))[0].size == 0 and ref.pairs("allowed", (1,))[0].size
        assert 0 < ref.pairs("flagged", (1,))[0].size <= ref.pairs("flagged")[0].size
        _review_equals(cs, 2, 7, flags, tile=2, sels=(None, (0, 3)))
        for kind, code in (("flagged", capi.RV_PAIRS_FLAGGED), ("allowed", capi.RV_PAIRS_ALLOWED)):
            pp, pr, mask = ref.pairs(kind)
            total = pp.size
            assert total > 2
            for cap in (0, 1, total - 1, total, total + 2):
                for tile in (0, 2):
                    raw = _Raw(capi, n, a, m, cap)
                    rc = raw.call(table.h, cs.h, 0, m, flags, pairs=code, tile=tile)
                    assert rc == (2 if cap < total else 0), (kind, cap, rc)
                    assert raw.rv.n_pairs == total, (kind, cap, raw.rv.n_pairs)
                    k = min(cap, total)
                    assert np.array_equal(raw.pp[:k], pp[:k]) and np.array_equal(raw.pr[:k], pr[:k]) and np.array_equal(raw.pm[:k], mask[:k]), (kind, cap)
                    assert raw.list_untouched(k), (kind, cap)
                    assert np.array_equal(raw.by_p[0], ref.allow_by_principal) and np.array_equal(raw.by_r[1], ref.flagged_by_resource)   # the counts are complete
                    assert np.array_equal(raw.totals, ref.totals)
            got = cs.review(0, m, flags=flags, now_ns=NOW, pairs=kind, pair_cap=3)          # a cap through the binding: a prefix, the whole count
            assert got.n_pairs == total and np.array_equal(got.pair_p, pp[:3]) and np.array_equal(got.pair_mask, mask[:3])
        cs.close()
        # the flagged list is what pairs_batch takes: the pairs' full results against the materialised product's rows
        h, po, ro, act = _halves(lt, p, r, acts, aux)
        cs = tx._direct(table, h, n, m, act, po, ro, capi.CX_ALL)
        rv = cs.review(0, m, flags=flags, now_ns=NOW, want_flagged=True, pairs="flagged")
        assert rv.n_pairs and rv.pair_p.size == rv.n_pairs
        from cerbos_amd.cross import upload_halves
        prod = upload_halves(table, h, n, m, act, po, ro)
        table.launch(prod, now_ns=NOW, flags=flags)
        want = table.download(prod)
        st = want.status.reshape(m, n, len(act)) != 0
        assert rv.n_pairs == int(st.any(axis=2).sum())
        tx._pairs_equal(table, cs, want, n, len(act), rv.pair_p, rv.pair_r, flags)
        prod.close()
        cs.close()
    finally:
        table.close()


def check_contract(capi):
    """every refusal leaves every out buffer at its fill pattern and a text in cbh_last_error; strict evaluation returns 1 and writes
    nothing; a call without any output is harmless; the set serves afterwards"""
    lib = capi.load()
    lt = _lower(workloads.c2_policies())
    table, other = capi.Table(lt.blob), capi.Table(lt.blob)
    n, m = 6, 5
    p, r, acts, aux = _halves_of("c2", n, m, seed=3)
    h, po, ro, act = _halves(lt, p, r, acts, aux)
    a = len(act)
    try:
        cs = tx._direct(table, h, n, m, act, po, ro, 0)
        ref = _Ref(cs, 0, m, 0)
        FL, AL = capi.RV_PAIRS_FLAGGED, capi.RV_PAIRS_ALLOWED

        def refused(**kw):
            raw = _Raw(capi, n, a, m, 8)
            args = dict(table_h=table.h, cs_h=cs.h, lo=0, hi=m)
            args.update(kw)
            rc = raw.call(**args)
            assert rc < 0 and lib.cbh_last_error() and raw.untouched() and raw.rv.n_pairs == 0xDEAD, (kw, rc, lib.cbh_last_error())

        refused(table_h=None)
        refused(cs_h=None)
        refused(null_params=True)
        refused(null_rv=True)
        refused(table_h=other.h)                                                          # a set of another table
        for lo, hi in ((3, 3), (4, 2), (0, m + 1), (m, m + 1)):                            # an empty range, r_end > M
            refused(lo=lo, hi=hi)
            assert b"non-empty range" in lib.cbh_last_error()
        for pairs in (3, 4, 0xFFFFFFFF):
            refused(pairs=pairs)
        refused(sel=1 << a)                                                                # an action the set does not have
        refused(sel=1 << 63, pairs=AL)
        refused(pairs=FL, null_lists=True)                                                 # a cap without its lists
        refused(pairs=AL, null_lists=True)
        raw = _Raw(capi, n, a, m, 8)                                                       # no direct form under strict evaluation
        assert raw.call(table.h, cs.h, 0, m, flags=capi.F_STRICT_EVALUATION, pairs=AL) == 1 and raw.untouched() and lib.cbh_last_error()
        with pytest.raises(capi.DirectFormUnavailable):
            cs.review(0, m, flags=capi.F_STRICT_EVALUATION, now_ns=NOW)
        with pytest.raises(capi.HipEngineError):
            cs.review(2, 2, now_ns=NOW)
        raw = _Raw(capi, n, a, m, 8)                                                       # nothing wanted: harmless
        assert raw.call(table.h, cs.h, 0, m, outputs=False, null_lists=True) == 0 and raw.untouched() and raw.rv.n_pairs == 0
        raw = _Raw(capi, n, a, m, 0)                                                       # the count alone: null lists with a cap of 0
        total = ref.pairs("allowed")[0].size
        assert total and raw.call(table.h, cs.h, 0, m, pairs=AL, null_lists=True, outputs=False) == 2 and raw.rv.n_pairs == total and raw.untouched()
        raw = _Raw(capi, n, a, m, 0)
        assert ref.pairs("flagged")[0].size == 0 and raw.call(table.h, cs.h, 0, m, pairs=FL, null_lists=True) == 0 and raw.rv.n_pairs == 0
        raw = _Raw(capi, n, a, m, n * m + 5)                                               # everything, through the raw call
        assert raw.call(table.h, cs.h, 0, m, pairs=AL, sel=(1 << a) - 1) == 0 and raw.rv.n_pairs == total
        assert np.array_equal(raw.by_p[0], ref.allow_by_principal) and np.array_equal(raw.by_p[1], ref.flagged_by_principal)
        assert np.array_equal(raw.by_r[0], ref.allow_by_resource) and np.array_equal(raw.by_r[1], ref.flagged_by_resource)
        assert np.array_equal(raw.totals, ref.totals) and np.array_equal(raw.pp[:total], ref.pairs("allowed")[0]) and raw.list_untouched(total)
        _review_equals(cs, 0, m)                                                           # ... and the set still serves
        cs.close()
    finally:
        table.close()
        other.close()


# ---- CPU tier: the simulator


@pytest.fixture()
def engine():
    with sim_engine() as capi:
        yield capi


def test_workloads_on_simulator(engine):
    check_modes(check_workloads(engine))


def test_geometry_on_simulator(engine):
    check_geometry(engine)


def test_tiles_on_simulator(engine):
    check_tiles(engine)


def test_pairs_on_simulator(engine):
    check_pairs(engine)


def test_contract_on_simulator(engine):
    check_contract(engine)


def test_failing_allocations_and_copies_are_survived():
    """Fault injection (simulator only), in the form of tests/test_cross_direct.py: the k-th device allocation - or asynchronous copy -
    from now on fails, for every k until the review succeeds; a failed review reports an error with a text, and the set gives right
    planes and right review results afterwards."""
    import test_sim_engine as ts
    ts._in_own_process('''
import ctypes as C
import numpy as np
from cerbos_amd import workloads
from cerbos_amd.cross import direct_upload_halves
import test_cross_direct as td
import test_cross_review as trv
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
want_rv = trv._Ref(cs, 0, 7, 0)
cs.close()
assert want_rv.pairs("allowed")[0].size > 3
for setter in (lib.cbh_sim_set_alloc_budget, lib.cbh_sim_set_copy_budget):
    for warm in (False, True):
        failed = 0
        for k in range(200):
            table = capi.Table(lt.blob)          # (a fresh table: empty pools, every buffer a real allocation)
            cs = direct_upload_halves(table, h, 9, 7, act, po, ro)
            if warm:                              # the set has its plane block already, of a smaller tile
                cs.check(0, 2, now_ns=NOW)
            setter(k)
            try:
                got = cs.review(0, 7, now_ns=NOW, want_flagged=True, pairs="allowed", pair_cap=80, tile_resources=3)
                trv._counts_equal(got, want_rv, k)
                trv._list_equal(got, want_rv.pairs("allowed"), k)
            except capi.HipEngineError as e:
                assert str(e), "an error without a message"
                failed += 1
            finally:
                setter(-1)
            a2, f2 = cs.check(0, 7, now_ns=NOW, want_flagged=True)      # the set is usable after a failed review
            assert np.array_equal(a2, want) and np.array_equal(f2, want_f)
            trv._review_equals(cs, 0, 7, tile=3)
            trv._review_equals(cs, 1, 6)
            cs.close()
            table.close()
            if failed == k:                       # the k-th was not reached: the call had enough
                break
        assert failed >= 5 and failed == k, (warm, failed, k)      # (at least: five counters' blocks; six copies of counts)
ref.close()
''', {})


# ---- GPU tier


@pytest.mark.gpu
def test_workloads_on_gpu():
    from cerbos_amd import capi
    check_modes(check_workloads(capi))


@pytest.mark.gpu
def test_geometry_on_gpu():
    from cerbos_amd import capi
    check_geometry(capi)


@pytest.mark.gpu
def test_tiles_on_gpu():
    from cerbos_amd import capi
    check_tiles(capi)


@pytest.mark.gpu
def test_pairs_on_gpu():
    from cerbos_amd import capi
    check_pairs(capi)


@pytest.mark.gpu
def test_contract_on_gpu():
    from cerbos_amd import capi
    check_contract(capi)


@pytest.mark.gpu
def test_one_review_over_two_to_the_32_pairs_on_gpu():
    """N = 65 536, M = 65 600 (4.3 G pairs, 17 G decisions): the halves are 1 024 flattened C2 rows per side repeated with numpy, as
    test_beyond_the_materialised_limit_on_gpu builds them.  ONE review of all M resources in the library's own tiles, counts and
    n_pairs only; the expected values come from the 1 024 x 1 024 base product decided by check on the base set: a per-principal
    count is its base column's sum weighted by how often each base resource occurs, a per-resource count 64 times its base row's,
    the totals likewise.  A second review with tiles of 4 096 resources agrees exactly."""
    from cerbos_amd import capi
    lt = _lower(workloads.c2_policies())
    base, big_n, big_m = 1024, 65536, 65600
    p, r, acts, aux = _halves_of("c2", base, base, seed=13)
    h, _, _, act = _halves(lt, p, r, acts, aux, sort=False)
    a = len(act)
    rows = np.concatenate([np.arange(big_n) % base, base + np.arange(big_m) % base])      # halves rows of the big set
    hb = _take_rows(h, rows)
    table = capi.Table(lt.blob)
    try:
        small = tx._direct(table, h, base, base, act, None, None, 0)
        planes = small.check(0, base, now_ns=NOW, want_flagged=True)
        small.close()
        ab, fb = (_bits(x, a, base, base).astype(np.uint64) for x in planes)             # [k][j][i] of the base product
        assert 0.01 < ab.mean() < 0.99
        times_r = np.bincount(np.arange(big_m) % base, minlength=base).astype(np.uint64)   # 65 for the first 64 base resources, 64 for the rest
        assert times_r[0] == 65 and times_r[63] == 65 and times_r[64] == 64
        rep_n = big_n // base
        cs = tx._direct(table, hb, big_n, big_m, act, None, None, 0)
        _named_x(cs.describe(0))
        got = [cs.review(0, big_m, now_ns=NOW, want_flagged=True, pairs="allowed", pair_cap=0, tile_resources=t) for t in (0, 4096)]
        cs.close()
        for rv in got:
            for bits, by_p, by_r, tot in ((ab, rv.allow_by_principal, rv.allow_by_resource, rv.totals[0]), (fb, rv.flagged_by_principal, rv.flagged_by_resource, rv.totals[1])):
                col = (bits * times_r[None, :, None]).sum(axis=1)                          # [k][i]: over the big set's resources
                assert np.array_equal(by_p, np.tile(col, (1, rep_n)).astype(np.uint32))
                row = bits.sum(axis=2) * np.uint64(rep_n)                                   # [k][j]: over the big set's principals
                assert np.array_equal(by_r, row[:, np.arange(big_m) % base].astype(np.uint32))
                assert np.array_equal(tot, col.sum(axis=1) * np.uint64(rep_n))
            any_allowed = ab.any(axis=0).astype(np.uint64)                                 # [j][i]
            assert rv.n_pairs == int((any_allowed * times_r[:, None]).sum()) * rep_n and rv.pair_p.size == 0
        assert big_n * big_m > 2 ** 32 and int(got[0].totals[0].sum()) > 2 ** 31       # (some 3 G allowed tuples of 17 G)
    finally:
        table.close()
