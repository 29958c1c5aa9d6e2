"""The flat walks' own tables at their limits: segments of 63, 64 and 65 records, items and leaf slots, the table-wide leaf pool and its
padding, 15, 16 and 17 complex items, conditions of 1, 4, 5, 8 and 9 leaves, 29 to 64 role and action classes.

What is pinned here (cbh_check_flat.h MODE 2 and its record and staged walks, lower/blob.py _segments and _layout_leaves):
  a segment's 64 bits            record 63 of a segment and record 0 of the next (the masks' high dword: a_hi / d_hi, `below` at bit 63,
                                 whose shift wraps), records 31 and 32 (the dword split), item 63, leaf slot 63
  CBH_FLAT_STAGE_MIN             a bucket of 32 records plans the record walk, one of 33 the mask walk
  the leaf pool                  64 SLOTS, counted after every class's run is padded to a multiple of four: 60 + 4 and 60 + 1 leaves pool,
                                 61 + 1 (62 leaves, 68 slots) do not; a padded copy is referenced by no item
  SEG_COMPLEX                    16 items a segment's wave decides as one; the 17th opens a segment; strips of 8 leaves, a tree of 9 (a program)
  leaves per item                1 .. 4 per lane, 5 .. 8 by the wave, 9 by the evaluator; none(x) is a negated one-leaf item
  segment-local leaves           tables that do not pool, with derived-role conditions (cd masks, rec_d) and a DENY at bit 63 by a derived role
  lanes at different buckets     a child scope of two segments beside a parent of one (the fetch-ahead behind a bucket's last block)
  class counts                   30 classes are flat (the 5-bit fields hold 29 beside the clamp 31), 31 .. 62 walk2, 63 the general walk

The machinery is tests/test_scope_limits.py's: its Case (the oracle's answers under both scope searches, computed once), its compare
(per tuple effect, policy key, scope; per request evaluation errors and effectiveDerivedRoles; nothing UNSUPPORTED), its roads and its
child processes.  The reference is oracle/check.py everywhere.  Every store is built so that the named position DECIDES: the CPU-tier
tests `test_*_decide*` read the position back from the lowered image (segments()), map it to its rule and ask the oracle about the
store without that rule - a compared field of some request must change.  Every case asserts the lowering's statistics and every road
the kernel it ran, so a lowering change that moves a limit fails here instead of un-testing the boundary.

Tiers: *_on_emulator the kernels' source on the wave emulator (every case under the three flat walks, the class cases under walk2 and
the general walk too), *_on_simulator the library's host side (forced variants in one child each), *_four_waves four waves to a
workgroup, *_on_gpu the library on the device.  The direct cross form is not run: test_scope_limits.check_cross puts its resources
at the scopes of a chain, where a store of one scope allows nothing under the strict search.

Mutation check (cbh_check_flat.h MODE 2, each mutant on a scratch copy, the emulator's mask_walk road; "older": the mask-walk, large-
bucket and pooling tests of tests/test_flat_kernel.py and tests/test_scope_limits.py, 32 tests; the first test that fails is named).
   1  d_hi[k] = 0                                       killed: records33.  older: 16 fail
   2  a_hi[k] = 0                                       killed: records63.  older: 4 fail
   3  err takes errrec & below & 0xFFFFFFFF             killed: records33 (the error at bit 60 in front of the DENY at bit 63).  older: 4 fail
   4  `below` is 0 where the first DENY is bit 63       killed: records64.  older: all pass
   5  seg_desc[itx < 63 ? itx : 0]                      killed: items64.  older: all pass
   6  leaf block 15 (slots 60 .. 63) never evaluated    killed: items63.  older: 1 fails
   7  the complex loop stops after 15 items             killed: complex16.  older: all pass
   8  a complex item's cd mask is not applied           killed: complex15.  older: all pass
   9  segment-local leaves of segment 0 kept for all    killed: pad_61_1.  older: 1 fails
  10  a bucket's walk stops after two segments          killed: records129.  older: 2 fail
The file's CPU tier takes 36 s in one process (244 tests), its GPU tier 6 s (33 tests).
"""
import itertools
import os
import struct

import numpy as np
import pytest

import test_scope_limits as ts
from cerbos_amd.engine import effective_policy_keys
from cerbos_amd.lower import blob as B
from cerbos_amd.lower.blob import lower_rule_table
from cerbos_amd.policy.loader import policies_from_docs
from cerbos_amd.ruletable.build import rule_table_from_policies
from oracle.check import EvalParams, RuleTableOracle
from test_scope_limits import API, F_LENIENT, F_WANT_DR, NOW, _flat, _policy, _rule

FLAG, OWNER, LVL2, SX = "R.attr.flag == true", "R.attr.owner == P.id", "P.attr.lvl >= 2.0", 'R.attr.s == "x"'
V10, V20, RANK2, TY, EXTRA2 = "R.attr.v > 10.0", "R.attr.v > 20.0", "R.attr.rank >= 2.0", 'R.attr.t == "y"', "R.attr.extra >= 2.0"
NINE = [FLAG, OWNER, LVL2, SX, V10, V20, RANK2, TY, EXTRA2]
SAT = dict(flag=True, owner="p0", lvl=3.0, s="x", v=25.0, rank=3.0, t="y", extra=3.0)           # every leaf of NINE holds
FAIL = {FLAG: dict(flag=False), OWNER: dict(owner="p1"), LVL2: dict(lvl=1.0), SX: dict(s="y"), V10: dict(v=5.0), V20: dict(v=15.0),
        RANK2: dict(rank=1.0), TY: dict(t="z"), EXTRA2: dict(extra=1.0)}                        # ... all but this one
ROLES5 = ["r0", "r1", "r2", "r3", "r4"]
ACTS = ["a%d" % i for i in range(16)]


def expr(e):
    return {"match": {"expr": e}}


def node(kind, of):
    return {kind: {"of": [x if isinstance(x, dict) else {"expr": x} for x in of]}}


def tree(kind, of):
    return {"match": node(kind, of)}


def pair(k):
    """rule k's own walk: 80 distinct (role, action) pairs"""
    return ROLES5[k % 5], ACTS[(k // 5) % 16]


FILL = [None, expr(FLAG), expr(OWNER), expr(LVL2), expr(SX), tree("any", [FLAG, OWNER]), tree("none", [SX])]


def filler(i):
    """a record that only fills its place: roles r0 .. r3, actions a0 .. a7, conditions of a small pool"""
    return _rule(["a%d" % (i % 8)], "DENY" if i % 9 == 4 else "ALLOW", roles=["r%d" % (i % 4)], cond=FILL[i % 7])


class Reqs:
    """the requests of a case, in lane order"""

    def __init__(self, seed, alternate=None):
        self.rng, self.out, self.alternate = np.random.default_rng(seed), [], alternate

    def add(self, roles, acts, scope=None, kind="doc", pid="p0", lvl=3.0, **rattr):
        i = len(self.out)
        if scope is None:
            scope = self.alternate[i % len(self.alternate)] if self.alternate else ""
        pattr = {"d": "m", "e": "w"}
        if lvl is not None:
            pattr["lvl"] = lvl
        self.out.append({"requestId": "q%d" % i, "actions": list(acts), "principal": {"id": pid, "roles": list(roles), "attr": pattr},
                         "resource": {"kind": kind, "id": "d%d" % i, "attr": {k: v for k, v in rattr.items() if v is not None}, "scope": scope}})
        return i

    def pick(self, vals):
        return vals[int(self.rng.integers(0, len(vals)))]

    def some(self, vals, most=4):
        return [str(x) for x in self.rng.choice(vals, size=int(self.rng.integers(1, min(most, len(vals)) + 1)), replace=False)]

    def draw(self, **over):
        """values for the leaves of NINE: held, not held, or absent (an evaluation error)"""
        d = dict(flag=self.pick([True, False, None, True]), owner=self.pick(["p0", "p1", "p0", None]), s=self.pick(["x", "y", None, "x"]),
                 v=self.pick([25.0, 15.0, 5.0, None, 25.0]), rank=self.pick([3.0, 1.0, None, 3.0]), t=self.pick(["y", "z", None, "y"]),
                 extra=self.pick([3.0, 1.0, None, 3.0]), lvl=self.pick([3.0, 1.0, 3.0, None]))
        d.update(over)
        return d

    def fill(self, count, roles, acts, **over):
        assert len(self.out) <= count, len(self.out)
        while len(self.out) < count:
            self.add(self.some(roles), self.some(acts), kind="other" if self.rng.random() < 0.04 else "doc", **self.draw(**over))
        assert count % 64 and 130 <= count <= 200
        return self.out


class SegCase(ts.Case):
    """a store of one resource kind: {scope: its policy's rules}, the derived-role sets every policy imports"""

    def __init__(self, name, policies, make_requests, drs=(), consent=(), flat=True, n=1):
        self.policies, self.drs, self.consent = policies, list(drs), set(consent)
        super().__init__(name, self.docs(), n, make_requests, flat=flat)
        self.segs = segments(self.lt) if flat else {}
        if flat:
            check_layout(self)

    def docs(self, without=None):
        out = list(self.drs)
        for scope, rules in self.policies.items():
            out.append(_policy("doc", scope, [r for k, r in enumerate(rules) if without != (scope, k)], consent=scope in self.consent,
                               imports=[d["derivedRoles"]["name"] for d in self.drs] or None))
        return out


# ---- the lowered image, read back: what the kernel will find at a segment's bit, item and slot


def _section(lt, sid):
    n = struct.unpack_from("<I", lt.blob, 8)[0]
    for k in range(n):
        s, count, off, size, _ = struct.unpack_from("<IIQQQ", lt.blob, 32 + 32 * k)
        if s == sid:
            return count, np.frombuffer(lt.blob, dtype=np.uint32, count=size // 4, offset=off)
    raise KeyError(sid)


def _bits(m):
    return [k for k in range(64) if (m >> k) & 1]


def segments(lt):
    """{scope: [segment]} of CBH_SEC_SEGS through the directory's B_RESSEG entries (lower/blob.py _segments writes them)"""
    _n, words = _section(lt, B.SEC_SEGS)
    n_slots, slots = _section(lt, B.SEC_HASH)
    pooled = bool(lt.seg_stats["pooled"])
    pool = _section(lt, B.SEC_LEAFPOOL)[1] if pooled else None
    out = {}
    for e in slots[:n_slots * 8].reshape(-1, 8):
        if int(e[0]) != B.B_RESSEG:
            continue
        at, segs = int(e[4]) * 16, []
        for _ in range(int(e[5])):
            w = words[at:]
            h = [int(x) for x in w[:16]]
            n_items, n_records, n_cx, off_cx, off_leaves = h[8], h[11], h[13], h[14] >> 16, h[15]
            n_leaf_slots = lt.seg_stats["pool_slots"] if pooled else h[9]
            leaf_words = pool if pooled else w[off_leaves:off_leaves + 4 * n_leaf_slots]
            rec = w[144:176].tobytes()
            cx = []
            for j in range(n_cx):
                x = [int(v) for v in w[off_cx + 16 * j:off_cx + 16 * j + 16]]
                cx.append({"cc": x[0] | x[1] << 32, "cd": x[2] | x[3] << 32, "how": x[4], "item": x[6], "n_leaves": x[7],
                           "slots": [((x[8] | x[9] << 32) >> (8 * q)) & 0xFF for q in range(min(x[7], 8))]})
            segs.append({
                "allow": h[0] | h[1] << 32, "deny": h[2] | h[3] << 32, "simple_c": h[4] | h[5] << 32, "simple_d": h[6] | h[7] << 32,
                "n_items": n_items, "n_records": n_records, "row_begin": h[12], "rec_c": list(rec[:64]), "rec_d": list(rec[64:]),
                "descs": [([(int(w[176 + 2 * i]) >> (8 * q)) & 0xFF for q in range(int(w[177 + 2 * i]) & 7)], int(w[177 + 2 * i])) for i in range(n_items)],
                "complex": cx, "leaves": [tuple(int(v) for v in leaf_words[4 * s:4 * s + 4]) for s in range(n_leaf_slots)]})
            at += h[10] * 16
        out[lt.scopes[int(e[3])]] = segs
    return out


def check_layout(c):
    """one record per rule, in the rules' order: the record counts and the ALLOW / DENY masks of every bucket say so (under
    REQUIRE_PARENTAL_CONSENT a conditional ALLOW is the DENY of none(its condition): ruletable/build.py)"""
    assert c.lt.stats["rows"] == sum(len(r) for r in c.policies.values()), (c.name, c.lt.stats["rows"])
    for scope, rules in c.policies.items():
        segs = c.segs[scope]
        assert sum(s["n_records"] for s in segs) == len(rules), (c.name, scope)
        k = 0
        for s in segs:
            assert s["row_begin"] == segs[0]["row_begin"] + k
            for b in range(s["n_records"]):
                allow = rules[k + b]["effect"] == "EFFECT_ALLOW" and not (scope in c.consent and "condition" in rules[k + b])
                assert ((s["allow"] >> b) & 1, (s["deny"] >> b) & 1) == (allow, not allow), (c.name, scope, k + b)
            k += s["n_records"]


def rule_of(c, scope, seg, bit):
    """the rule behind bit `bit` of segment `seg`"""
    return sum(s["n_records"] for s in c.segs[scope][:seg]) + bit


def records_of_item(seg, item):
    recs = {k for k in range(seg["n_records"]) if item in (seg["rec_c"][k], seg["rec_d"][k])}
    for e in seg["complex"]:
        if e["item"] == item:
            recs.update(_bits(e["cc"] | e["cd"]))
    return sorted(recs)


def items_of_slot(seg, slot):
    simple = {i for i, (ids, _f) in enumerate(seg["descs"]) if slot in ids}
    return sorted(simple | {e["item"] for e in seg["complex"] if slot in e["slots"]})


def pads_of(seg):
    """(referenced slots, padded copies): a run's padding repeats its last leaf"""
    used = {s for ids, _f in seg["descs"] for s in ids} | {s for e in seg["complex"] for s in e["slots"]}
    pads = {s for s in range(1, len(seg["leaves"])) if seg["leaves"][s] == seg["leaves"][s - 1]}
    return used, pads


def fields(inp, w):
    return (tuple((w["actions"][a]["effect"], w["actions"][a]["policy"], w["actions"][a]["scope"]) for a in inp["actions"]),
            tuple(sorted(w["effectiveDerivedRoles"])), bool(w["evaluationErrors"]))


def decided_by(c, scope, k, what):
    """-> the requests of which a compared field changes when rule k of `scope`'s policy leaves the store (asked of the oracle)"""
    orc = RuleTableOracle(rule_table_from_policies(policies_from_docs(c.docs(without=(scope, k)))))
    out = [i for i, (inp, w) in enumerate(zip(c.inputs, c.want[False])) if fields(inp, orc.check(inp, EvalParams(now_ns=NOW))) != fields(inp, w)]
    assert out, "%s: %s (rule %d of the policy at scope %r) decides no compared field of any request" % (c.name, what, k, scope)
    return out


def effect(c, i, action, lenient=False):
    return c.want[lenient][i]["actions"][action]["effect"]


def errors(c, i):
    return bool(c.want[False][i]["evaluationErrors"])


# ---- 1. record counts


def records_rules(n, child=False):
    """fillers, and: the conditional DENY at each segment's last bit with an ALLOW for its walk in front (5, 6: by ownership) and
    behind (64, 128); an erroring record in front of the DENY (60, 124: reported) and the one behind (never evaluated where the DENY
    holds); record 31 the only ALLOW of the walk (r5, a10), record 32 the only DENY of the walk (r5, a11)"""
    special = {5: _rule(["a8"], "ALLOW", roles=["r4"], cond=expr(OWNER)), 6: _rule(["a9"], "ALLOW", roles=["r4"], cond=expr(OWNER)),
               7: _rule(["a11"], "ALLOW", roles=["r5"]),
               31: _rule(["a10"], "ALLOW", roles=["r5"]), 32: _rule(["a11"], "DENY", roles=["r5"], cond=expr(FLAG)),
               60: _rule(["a8"], "ALLOW", roles=["r4"], cond=expr(RANK2)), 63: _rule(["a8"], "DENY", roles=["r4"], cond=expr(FLAG)),
               64: _rule(["a8"], "ALLOW", roles=["r4"], cond=expr(EXTRA2)),
               124: _rule(["a9"], "ALLOW", roles=["r4"], cond=expr(RANK2)), 127: _rule(["a9"], "DENY", roles=["r4"], cond=expr(FLAG)),
               128: _rule(["a9"], "ALLOW", roles=["r4"], cond=expr(EXTRA2))}
    if child:
        special = {k: special[k] for k in (60, 63, 64)}
    return [special.get(i) or filler(i) for i in range(n)]


def last_bit_requests(q, act, notes, key, **kw):
    notes[key] = dict(
        denied=q.add(["r4"], [act], **dict(SAT, **kw)),                                      # allowed by ownership, then the DENY at bit 63
        behind=q.add(["r4"], [act], **dict(SAT, flag=False, owner="p1", rank=1.0, **kw)),    # only the record behind the DENY allows
        err_before=q.add(["r4"], [act], **dict(SAT, rank=None, **kw)),                       # raised in front of the satisfied DENY: reported
        err_behind=q.add(["r4"], [act], **dict(SAT, extra=None, **kw)),                      # behind it: never evaluated
        err_open=q.add(["r4"], [act], **dict(SAT, flag=False, extra=None, **kw)))            # ... evaluated where the DENY does not hold


def records_case(name, n):
    def make(lt):
        q, notes = Reqs(1000 + n), {}
        last_bit_requests(q, "a8", notes, 63)
        last_bit_requests(q, "a9", notes, 127)
        notes["dwords"] = dict(allow31=q.add(["r5"], ["a10"], **SAT), deny32=q.add(["r5"], ["a11"], **SAT),
                               open32=q.add(["r5"], ["a11"], **dict(SAT, flag=False)))
        for roles in (["r5", "r4"], ["r4", "r5"], ["r0", "r5"], ["r4", "r1", "r5"]):
            for flag in (True, False, None):
                q.add(roles, ["a8", "a9", "a10", "a11"], **dict(SAT, flag=flag))
        return q.fill(163, ["r0", "r1", "r2", "r3", "r4", "r5", "stranger"], ACTS[:12] + ["nothing"]), notes
    return SegCase(name, {"": records_rules(n)}, make)


def check_records(c, n):
    st, segs = c.lt.seg_stats, c.segs[""]
    assert st["pooled"] and st["segments"] == (n + 63) // 64 and [s["n_records"] for s in segs] == [64] * (n // 64) + ([n % 64] if n % 64 else []), (c.name, st)
    assert c.lt.stats["flat_closed"] and not c.lt.stats["derived_roles"]
    for last, act in ((63, "a8"), (127, "a9")):
        if last >= n:
            continue
        seg, nt = segs[last // 64], c.notes[last]
        assert (seg["deny"] >> 63) & 1 and (seg["simple_c"] >> 63) & 1, (c.name, "bit 63 of segment %d is no conditional DENY" % (last // 64))
        assert effect(c, nt["denied"], act) == "EFFECT_DENY" and nt["denied"] in decided_by(c, "", last, "record %d, a segment's bit 63" % last)
        assert errors(c, nt["err_before"]) and effect(c, nt["err_before"], act) == "EFFECT_DENY", (c.name, "the error in front of the DENY at bit 63 is not reported")
        assert not errors(c, nt["err_behind"]) and effect(c, nt["err_behind"], act) == "EFFECT_DENY", (c.name, "an error behind the satisfied DENY at bit 63 is reported")
        if last + 1 < n:
            assert segs[last // 64 + 1]["allow"] & 1, (c.name, "bit 0 of the next segment is no ALLOW")
            assert effect(c, nt["behind"], act) == "EFFECT_ALLOW" and nt["behind"] in decided_by(c, "", last + 1, "record %d, the next segment's bit 0" % (last + 1))
            assert errors(c, nt["err_open"]), (c.name, "the record behind bit 63 raises nothing where the DENY does not hold")
    nt = c.notes["dwords"]
    assert (segs[0]["allow"] >> 31) & 1 and effect(c, nt["allow31"], "a10") == "EFFECT_ALLOW" and nt["allow31"] in decided_by(c, "", 31, "record 31, the low dword's last bit")
    if n > 32:
        assert (segs[0]["deny"] >> 32) & 1 and effect(c, nt["deny32"], "a11") == "EFFECT_DENY" and effect(c, nt["open32"], "a11") == "EFFECT_ALLOW"
        assert nt["deny32"] in decided_by(c, "", 32, "record 32, the high dword's first bit")


# ---- 2. item counts, 3. pool padding


def threshold_rules(n, first=0, denies=True):
    """rule k: its own item and leaf `R.attr.v > k`, its own walk pair(k) - but every eighth is a DENY for the walk of the rule in front"""
    out = []
    for k in range(first, first + n):
        deny = denies and k % 8 == 7
        role, act = pair(k - 1 if deny else k)
        out.append(_rule([act], "DENY" if deny else "ALLOW", roles=[role], cond=expr("R.attr.v > %d.0" % k)))
    return out


def threshold_requests(q, n, **kw):
    for k in range(n):
        role, act = pair(k)
        q.add([role], [act], v=k + 0.5, **kw)        # rule k holds, rule k + 1 does not
        q.add([role], [act], v=k + 1.5, **kw)        # ... both (a DENY behind an ALLOW ends the walk)
    for k in range(0, n, 9):
        q.add([pair(k)[0], pair(k + 1)[0]], [pair(k)[1], pair(k + 1)[1]], v=None if k % 2 else k - 0.5, **kw)


ITEM_STATS = {63: (True, 1, 63, 63), 64: (True, 1, 64, 64), 65: (False, 2, 64, 64)}   # pooled, segments, max_items, max_leaves


def items_case(name, n):
    def make(lt):
        q = Reqs(2000 + n)
        threshold_requests(q, n)
        return q.fill(157, ROLES5, ACTS, v=70.5), {}
    return SegCase(name, {"": threshold_rules(n)}, make)


def check_items(c, n):
    st = c.lt.seg_stats
    assert (st["pooled"], st["segments"], st["max_items"], st["max_leaves"]) == ITEM_STATS[n] and st["items"] == st["leaves"] == n and st["complex_entries"] == 0, (c.name, st)
    seg = c.segs[""][0]
    assert seg["n_items"] == min(n, 64) and len(seg["leaves"]) == 64
    if n >= 64:
        for k in records_of_item(seg, 63):
            decided_by(c, "", rule_of(c, "", 0, k), "item 63 of a segment")
        recs = [k for i in items_of_slot(seg, 63) for k in records_of_item(seg, i)]
        assert recs, (c.name, "no item reads leaf slot 63")
        for k in recs:
            decided_by(c, "", rule_of(c, "", 0, k), "leaf slot 63")
    if n == 65:
        decided_by(c, "", 64, "the one record of the second segment")


def class1_rules(n, first):
    return [_rule([pair(first + j)[1]], "ALLOW", roles=[pair(first + j)[0]], cond=expr('R.attr.s == "x%d"' % j)) for j in range(n)]


def class1_requests(q, n, first, **kw):
    for j in range(n):
        role, act = pair(first + j)
        q.add([role], [act], s="x%d" % j, **kw)
        q.add([role], [act], s="x%d" % (j + 1), **kw)
        q.add([role], [act], **kw)


PAD_STATS = {"pad_60_4": (True, 64, 64, 1, 64), "pad_60_1": (True, 64, 61, 1, 61), "pad_61_1": (False, 0, 62, 2, 61)}   # pooled, pool_slots, leaves, segments, max_leaves


def pad_case(name):
    n2, n1 = (int(x) for x in name.split("_")[1:])

    def make(lt):
        q = Reqs(3000 + 10 * n2 + n1)
        threshold_requests(q, n2, s="zz")
        class1_requests(q, n1, n2, v=-1.0)
        return q.fill(163, ROLES5, ACTS, v=70.5, s="x0"), {}
    return SegCase(name, {"": threshold_rules(n2) + class1_rules(n1, n2)}, make)


def five_classes(g, j):
    """leaf j of inline class (1, 2, 3, 4, 6)[g] -> (its text, resource attributes under which it holds, ... does not); 16 columns in all
    (the inline column cache's)"""
    if g == 0:
        return 'R.attr.s == "x%d"' % j, dict(s="x%d" % j), dict(s="zz")
    if g == 1:
        return "R.attr.v > %d.0" % j, dict(v=j + 0.5), dict(v=j - 0.5)
    if g == 2:
        col, eq, other = "c%d" % (j % 4), (j // 4) % 2 == 0, ("d", "m") if j < 8 else ("e", "w")
        return "R.attr.%s %s P.attr.%s" % (col, "==" if eq else "!=", other[0]), {col: other[1] if eq else "n"}, {col: "n" if eq else other[1]}
    if g == 3:
        col, eq = "o%d" % (j % 7), j < 7
        return "R.attr.%s %s P.id" % (col, "==" if eq else "!="), {col: "p0" if eq else "nobody"}, {col: "nobody" if eq else "p0"}
    return 'R.attr.t in ["a%d", "b%d"]' % (j, j), dict(t="b%d" % j), dict(t="zz")


def pad_five_case(name):
    """13 leaves of each inline class: 65 leaves, every class's run padded to 16 slots - in each segment by itself"""
    rules = [_rule([pair(13 * g + j)[1]], "ALLOW", roles=[pair(13 * g + j)[0]], cond=expr(five_classes(g, j)[0])) for g in range(5) for j in range(13)]

    def make(lt):
        q = Reqs(3500)
        base = dict(s="zz", v=-1.0, t="zz", **{"c%d" % j: "n" for j in range(4)}, **{"o%d" % j: "nobody" for j in range(7)})
        for g in range(5):
            for j in range(13):
                (role, act), (_text, held, not_held) = pair(13 * g + j), five_classes(g, j)
                q.add([role], [act], **{**base, **held})
                q.add([role], [act], **({**base, **not_held} if j % 3 else {k: v for k, v in base.items() if k not in held}))   # not held; absent
        while len(q.out) < 163:
            g, j = int(q.rng.integers(0, 5)), int(q.rng.integers(0, 13))
            q.add(q.some(ROLES5), q.some(ACTS), **{**base, "v": 12.5, **five_classes(g, j)[1]})
        return q.out, {}
    return SegCase(name, {"": rules}, make)


def check_pads(c):
    """a run's padded copies are referenced by no item; the leaf in each class's last real slot decides a tuple"""
    for si, seg in enumerate(c.segs[""] if not c.lt.seg_stats["pooled"] else c.segs[""][:1]):
        used, pads = pads_of(seg)
        assert not (used & pads) and used | pads == set(range(len(seg["leaves"]))), (c.name, si, sorted(used & pads))
        assert len(seg["leaves"]) % 4 == 0 and len(seg["leaves"]) <= 64
        last = {}
        for s in sorted(used):
            last[seg["leaves"][s][0] & 15] = s
        for cls, s in sorted(last.items()):
            assert s + 1 == len(seg["leaves"]) or s + 1 in pads or (seg["leaves"][s + 1][0] & 15) != cls
            for i in items_of_slot(seg, s):
                for k in records_of_item(seg, i):
                    decided_by(c, "", rule_of(c, "", si, k), "the last real leaf of class %d (slot %d of segment %d)" % (cls, s, si))
        yield seg, used, pads, last


def check_pad(c):
    st = c.lt.seg_stats
    if c.name == "pad_five":
        assert not st["pooled"] and st["leaves"] == 65 and st["segments"] == 2 and st["complex_entries"] == 0, (c.name, st)
        got = list(check_pads(c))
        assert c.lt.stats["flat_closed"] and c.lt.stats["columns"] == 16
        assert sorted(got[0][3]) == [1, 2, 3, 4] and sorted(got[1][3]) == [6], (c.name, "the classes of the two segments", [sorted(g[3]) for g in got])
        assert [len(g[0]["leaves"]) for g in got] == [64, 16] and [len(g[2]) for g in got] == [12, 3], (c.name, "every class's run of 13 is padded to 16 slots")
        return
    assert (st["pooled"], st["pool_slots"], st["leaves"], st["segments"], st["max_leaves"]) == PAD_STATS[c.name], (c.name, st)
    n2, n1 = (int(x) for x in c.name.split("_")[1:])
    for seg, used, pads, last in check_pads(c):
        if st["pooled"]:
            assert len(seg["leaves"]) == 64 and len(pads) == 64 - n2 - n1 and last == {1: n1 - 1, 2: 63}, (c.name, sorted(pads), last)


# ---- 4. complex items, 5. leaves per item


DEEP8 = {"match": node("all", [FLAG, OWNER, node("any", [SX, TY, node("all", [V10, V20, RANK2])]), LVL2])}   # two levels down, a strip of 8 leaves
ALL5 = [list(x) for x in itertools.combinations(NINE, 5)]


def complex_conditions(n):
    cx = [DEEP8, tree("any", [FLAG, RANK2, SX, V10, TY]), tree("any", [RANK2, FLAG, SX, V10, TY])]
    if n == 33:
        cx.append(tree("all", NINE))                       # no strip: a program, the table is not closed
    return cx + [tree("all", ALL5[k]) for k in range(len(cx), n)]


def complex_case(name, n):
    """16 fillers, then n rules of one complex condition each (pair(k) is rule k's walk); behind the sixth the two records of the
    derived role `cx`, whose definition's condition is the sixth's own"""
    cx = complex_conditions(n)
    rules = [filler(i) for i in range(16)]
    rules[3] = _rule(["a13"], "ALLOW", roles=["r0"])
    for k, cond in enumerate(cx):
        rules.append(_rule([pair(k)[1]], "ALLOW", roles=[pair(k)[0]], cond=cond))
        if k == 5:
            rules += [_rule(["a12"], "ALLOW", derived=["cx"]), _rule(["a13"], "DENY", derived=["cx"])]
    drs = [{"apiVersion": API, "derivedRoles": {"name": "set_cx", "definitions": [{"name": "cx", "parentRoles": ["r0", "r1"], "condition": cx[5]}]}}]

    def make(lt):
        q, notes = Reqs(4000 + n), {}
        notes["sat_first"] = q.add([pair(1)[0]], [pair(1)[1]], **dict(SAT, rank=None))     # any(held, raises, ...): nothing reported
        notes["err_first"] = q.add([pair(2)[0]], [pair(2)[1]], **dict(SAT, rank=None))     # any(raises, held, ...): reported
        for k in range(n):
            role, act = pair(k)
            q.add([role], [act], **SAT)
            q.add([role], [act], **dict(SAT, **FAIL[LVL2 if k < 4 else ALL5[k][k % 5]]))
        for over in ({}, FAIL[ALL5[5][0]], FAIL[ALL5[5][4]], dict(flag=None)):
            q.add(["r0"], ["a12", "a13"], **dict(SAT, **over))
            q.add(["r3", "r1"], ["a13", "a12"], **dict(SAT, **over))
        return q.fill(min(197, 131 + 2 * n), ROLES5, ACTS), notes
    return SegCase(name, {"": rules}, make, drs=drs, flat=True)


COMPLEX_STATS = {15: (1, 15), 16: (1, 16), 17: (2, 17), 33: (3, 33)}   # segments, complex_entries


def check_complex(c, n):
    st, segs = c.lt.seg_stats, c.segs[""]
    assert st["pooled"] and (st["segments"], st["complex_entries"]) == COMPLEX_STATS[n] and st["items_deeper"] == 1, (c.name, st)
    assert [len(s["complex"]) for s in segs] == [16] * (n // 16) + ([n % 16] if n % 16 else []), (c.name, [len(s["complex"]) for s in segs])
    assert c.lt.stats["flat_closed"] == (n != 33) and c.lt.stats["derived_roles"]
    deep = [e for e in segs[0]["complex"] if (e["how"] & 3) == 2]
    assert len(deep) == 1 and deep[0]["n_leaves"] == 8, (c.name, "the deeper tree has no strip of 8 leaves")
    assert [e["how"] & 3 for s in segs for e in s["complex"]].count(0) == (1 if n == 33 else 0), (c.name, "the 9-leaf tree: a program, and the only one")
    assert any(e["cd"] for e in segs[0]["complex"]), (c.name, "no complex item is a derived-role condition (cd masks)")
    assert not errors(c, c.notes["sat_first"]) and errors(c, c.notes["err_first"]), (c.name, "any(held, raises) / any(raises, held)")
    assert effect(c, c.notes["sat_first"], pair(1)[1]) == effect(c, c.notes["err_first"], pair(2)[1]) == "EFFECT_ALLOW"
    assert len({tuple(w["effectiveDerivedRoles"]) for w in c.want[False]}) == 2
    if n >= 16:
        for k in _bits(segs[0]["complex"][15]["cc"]):
            decided_by(c, "", rule_of(c, "", 0, k), "the 16th complex item of a segment")
    if n >= 17:
        recs = records_of_item(segs[1], 0)
        assert recs and segs[1]["complex"][0]["item"] == 0
        for k in recs:
            decided_by(c, "", rule_of(c, "", 1, k), "the first item of the following segment")


LEAF_STATS = {1: (2, 0, True), 4: (3, 0, True), 5: (3, 3, True), 8: (3, 3, True), 9: (3, 3, False)}   # items, complex_entries, flat_closed


def leaves_case(name, n):
    """all, any and none of the first n leaves of NINE, one level: the walks (r0, a0), (r0, a1), (r0, a2)"""
    rules = [_rule(["a%d" % k], "ALLOW", roles=["r0"], cond=tree(kind, NINE[:n])) for k, kind in enumerate(("all", "any", "none"))]

    def make(lt):
        q = Reqs(5000 + n)
        q.add(["r0"], ["a0", "a1", "a2"], **SAT)
        q.add(["r0"], ["a0", "a1", "a2"], **dict(SAT, flag=False, owner="p1", lvl=1.0, s="y", v=5.0, rank=1.0, t="z", extra=1.0))
        for j in range(n):
            q.add(["r0"], ["a0", "a1", "a2"], **dict(SAT, **FAIL[NINE[j]]))                                      # one leaf not held
            q.add(["r0"], ["a2", "a1", "a0"], **dict(SAT, **{k: None for k in FAIL[NINE[j]]}))                   # ... absent
            q.add(["r1", "r0"], ["a1", "a2"], **{**SAT, **FAIL[NINE[j]], **FAIL[NINE[(j + 1) % 9]]})                # ... two not held
        return q.fill(137, ["r0", "r1"], ["a0", "a1", "a2"]), {}
    return SegCase(name, {"": rules}, make)


def check_leaves(c, n):
    st, seg = c.lt.seg_stats, c.segs[""][0]
    assert (st["items"], st["complex_entries"], c.lt.stats["flat_closed"]) == LEAF_STATS[n] and st["pooled"] and st["segments"] == 1, (c.name, st)
    assert st["items_one_level"] == (0 if n == 9 else st["items"]) and st["leaves"] == (0 if n == 9 else n)
    for k in range(3):
        decided_by(c, "", k, "the %s of %d leaves" % (("all", "any", "none")[k], n))
    if n <= 4:      # the lanes decide these by themselves: count, any, negated in the item's descriptor
        want = [(n, False, False), (n, n > 1, False), (n, n > 1, True)]
        have = [(seg["descs"][seg["rec_c"][k]][1] & 7, bool(seg["descs"][seg["rec_c"][k]][1] & 8), bool(seg["descs"][seg["rec_c"][k]][1] & 16)) for k in range(3)]
        assert have == want and seg["simple_c"] == 7, (c.name, have)
    else:
        assert seg["simple_c"] == 0 and sorted(_bits(e["cc"])[0] for e in seg["complex"]) == [0, 1, 2]


# ---- 6. segments with their own leaves and derived roles, 7. two scopes


def unpooled_case(name):
    """150 rules of the root policy over 102 thresholds (40 to a segment), every third through a derived role whose definition has
    a condition (d2's has five leaves); rule 63 - bit 63 of the first segment - is a DENY through d0 for a walk rule 5 allows.  Two
    small child policies: requests stand at three buckets and have four sets of effective policies."""
    main = []
    for i in range(150):
        leaf, act, eff = expr("R.attr.v > %d.0" % ((i // 64) * 40 + i % 40)), "a%d" % ((i // 4) % 8), "DENY" if i % 7 == 3 else "ALLOW"
        main.append(_rule([act], eff, derived=["d%d" % ((i // 3) % 3)], cond=leaf) if i % 3 == 0 else _rule([act], eff, roles=["r%d" % (i % 4)], cond=leaf))
    main[5] = _rule(["a8"], "ALLOW", roles=["r0"], cond=expr("R.attr.v > 5.0"))
    main[63] = _rule(["a8"], "DENY", derived=["d0"], cond=expr("R.attr.v > 23.0"))
    main[64] = _rule(["a9"], "ALLOW", roles=["r3"], cond=expr("R.attr.v > 64.0"))       # the walks (r3, a9) and (r3, a10): one record each,
    main[128] = _rule(["a10"], "ALLOW", roles=["r3"], cond=expr("R.attr.v > 88.0"))     # the first of the second and of the third segment
    drs =[{"apiVersion": API, "derivedRoles": {"name": "set_a", "definitions": [
        {"name": "d0", "parentRoles": ["r0", "r1"], "condition": expr(OWNER)}, {"name": "d1", "parentRoles": ["*"], "condition": expr(LVL2)}]}},
        {"apiVersion": API, "derivedRoles": {"name": "set_b", "definitions": [
            {"name": "d2", "parentRoles": ["r2"], "condition": tree("all", [FLAG, SX, RANK2, TY, EXTRA2])}]}}]
    policies = {"": main, "s0": [_rule(["a0", "a8"], "ALLOW", roles=["r1"], cond=expr(V20)), _rule(["a1"], "DENY", derived=["d1"], cond=expr(V10))],
                "s0.s1": [_rule(["a0"], "DENY", roles=["r1"], cond=expr(FLAG)), _rule(["a2", "a8"], "ALLOW", derived=["d2"])]}

    def make(lt):
        q, notes = Reqs(6000), {}
        notes["denied"] = q.add(["r0"], ["a8"], **dict(SAT, v=100.5))
        notes["not_owner"] = q.add(["r0"], ["a8"], **dict(SAT, v=100.5, owner="p1"))
        notes["no_owner"] = q.add(["r0"], ["a8"], **dict(SAT, v=100.5, owner=None))
        for v in (100.5, 70.5, 10.5):
            q.add(["r3"], ["a9", "a10"], **dict(SAT, v=v))
        for v in (3.5, 23.5, 39.5, 40.5, 63.5, 79.5, 80.5, 101.5, 120.5):
            for roles in (["r0"], ["r2"], ["r3", "r1"]):
                q.add(roles, ["a0", "a3", "a7", "a8"], **dict(SAT, v=v))
        while len(q.out) < 171:
            q.add(q.some(["r0", "r1", "r2", "r3", "stranger"]), q.some(ACTS[:9]), scope=q.pick(["", "", "", "", "s0", "s0", "s0.s1", "s0.s1", "zz", "s0.zz"]),
                  kind="other" if q.rng.random() < 0.04 else "doc", **q.draw(v=float(q.rng.integers(0, 110)) + 0.5))
        return q.out, notes
    return SegCase(name, policies, make, drs=drs)


def check_unpooled(c):
    st, segs = c.lt.seg_stats, c.segs[""]
    assert not st["pooled"] and st["leaves"] > 64 and st["segments"] == 5 and [s["n_records"] for s in segs] == [64, 64, 22], (c.name, st)
    assert c.lt.stats["flat_closed"] and c.lt.stats["derived_roles"]
    assert all(0 < len(s["leaves"]) <= 64 for s in segs) and len({tuple(s["leaves"]) for s in segs}) == 3, "every segment has leaves of its own"
    assert (segs[0]["deny"] >> 63) & 1 and segs[0]["rec_d"][63] < 64 and (segs[0]["simple_d"] >> 63) & 1, (c.name, "bit 63 of the first segment is no DENY through a derived role")
    assert any(e["cd"] and e["n_leaves"] == 5 for s in segs for e in s["complex"]), (c.name, "no derived-role condition of five leaves")
    nt = c.notes
    assert effect(c, nt["denied"], "a8") == "EFFECT_DENY" and effect(c, nt["not_owner"], "a8") == "EFFECT_ALLOW" and errors(c, nt["no_owner"])
    assert nt["denied"] in decided_by(c, "", 63, "the derived-role DENY at bit 63 of a segment with its own leaves")
    decided_by(c, "", 64, "the first record of the second segment")
    decided_by(c, "", 128, "the first record of the third segment")
    assert len({tuple(w["effectivePolicies"]) for w in c.want[False]}) > 3 and len({tuple(w["effectiveDerivedRoles"]) for w in c.want[False]}) >= 4


def two_scopes_case(name):
    """the child (REQUIRE_PARENTAL_CONSENT, 65 records: two segments) and its parent (33 records); lanes alternate between them"""
    parent = [filler(i) for i in range(33)]
    parent[32] = _rule(["a8"], "ALLOW", roles=["r4"])                      # the consent to the child's ALLOWs: the parent's bit 32

    def make(lt):
        q, notes = Reqs(7000, alternate=("s0", "")), {}
        notes["child"] = dict(                                               # (the child's conditional ALLOWs deny where they do not hold)
            denied=q.add(["r4"], ["a8"], scope="s0", **SAT),                                              # the DENY at bit 63
            behind=q.add(["r4"], ["a8"], scope="s0", **dict(SAT, flag=False, extra=1.0)),                 # the record behind it denies
            consent=q.add(["r4"], ["a8"], scope="s0", **dict(SAT, flag=False)),                           # neither: the parent allows
            err_before=q.add(["r4"], ["a8"], scope="s0", **dict(SAT, rank=None)),                         # raised in front of the satisfied DENY
            err_behind=q.add(["r4"], ["a8"], scope="s0", **dict(SAT, extra=None)),                        # behind it: never evaluated
            err_open=q.add(["r4"], ["a8"], scope="s0", **dict(SAT, flag=False, extra=None)))              # ... evaluated
        notes["parent"] = q.add(["r4"], ["a8"], scope="", **SAT)
        for roles in (["r4", "r0"], ["r0", "r4"], ["r4"]):
            for flag in (True, False, None):
                q.add(roles, ["a8", "a0", "a1", "a5"], scope="s0", **dict(SAT, flag=flag))
                q.add(roles, ["a8", "a0", "a1", "a5"], scope="", **dict(SAT, flag=flag))
        q.fill(167, ["r0", "r1", "r2", "r3", "r4", "stranger"], ACTS[:9] + ["nothing"])
        assert {i["resource"]["scope"] for i in q.out[26:64:2]} == {"s0"} and {i["resource"]["scope"] for i in q.out[27:64:2]} == {""}
        return q.out, notes
    return SegCase(name, {"": parent, "s0": records_rules(65, child=True)}, make, consent=("s0",))


def check_two_scopes(c):
    st = c.lt.seg_stats
    assert st["pooled"] and st["segments"] == 3 and [s["n_records"] for s in c.segs["s0"]] == [64, 1] and [s["n_records"] for s in c.segs[""]] == [33], (c.name, st)
    nt = c.notes["child"]
    assert effect(c, nt["denied"], "a8") == "EFFECT_DENY" and nt["denied"] in decided_by(c, "s0", 63, "bit 63 of the child's first segment")
    assert effect(c, nt["behind"], "a8") == "EFFECT_DENY" and nt["behind"] in decided_by(c, "s0", 64, "the one record of the child's second segment")
    assert effect(c, nt["consent"], "a8") == "EFFECT_ALLOW" and nt["consent"] in decided_by(c, "", 32, "the parent's last record, bit 32 (its consent)")
    assert errors(c, nt["err_before"]) and not errors(c, nt["err_behind"]) and errors(c, nt["err_open"])
    assert effect(c, c.notes["parent"], "a8") == "EFFECT_ALLOW"
    at = c.decided_at()
    assert at.get(0) and at.get(1), (c.name, "tuples are decided at one scope only", at)


# ---- 8. class counts


def classes_case(name):
    """n distinct literal roles and / or actions, one rule each (the first and the last unconditional ALLOWs); behind them the one
    `*`-role rule, which alone decides for a role no rule names"""
    n, dim = int(name[7:9]), name.split("_")[1]
    roles = ["role%02d" % k for k in range(n)] if dim != "actions" else ["r0", "r1"]
    acts = ["act%02d" % k for k in range(n)] if dim != "roles" else ["a0", "a1"]
    rules = []
    for k in range(n):
        plain = k in (0, n - 1)
        rules.append(_rule([acts[k % len(acts)]], "DENY" if k % 7 == 3 and not plain else "ALLOW", roles=[roles[k % len(roles)]],
                           cond=None if plain else [None, expr(FLAG), None, expr(SX)][k % 4]))
    star_act = acts[0] if dim != "roles" else acts[n % 2]                  # (not the action of the last class's rule)
    rules.append(_rule([star_act], "ALLOW", roles=["*"], cond=expr(OWNER)))
    last = (roles[(n - 1) % len(roles)], acts[(n - 1) % len(acts)])

    def make(lt):
        q = Reqs(8000 + n)
        notes = {"last": q.add([last[0]], [last[1]], **SAT), "star": q.add(["x1"], [star_act], **SAT)}
        role_sets = [[roles[0]], [last[0]], ["x1"], ["x2"], ["x3"], [roles[0], last[0]], [last[0], roles[0]], ["x1", last[0]], [roles[0], "x2"], ["x3", "x1"],
                     [roles[len(roles) // 2]], [roles[1], last[0], "x2", roles[0]]]
        act_sets = [[acts[0]], [last[1]], ["y1"], [acts[0], last[1], "y2"], ["y3", last[1]], [star_act, "y1", acts[len(acts) // 2], acts[1]]]
        k = 0
        for rs in role_sets:
            for as_ in act_sets:
                k += 1
                q.add(rs, as_, **dict(SAT, flag=(True, False, None)[k % 3], owner=("p0", "p1")[k % 2], s=("x", "y", "x", None)[k % 4]))
                if k % 2:
                    q.add(rs, list(reversed(as_)), **dict(SAT, flag=(True, False, None)[(k + 1) % 3], owner=("p0", "p1", None)[k % 3]))
        return q.fill(135, roles[:2] + [last[0], "x1", "x2", "x3"], acts[:2] + [last[1], "y1", "y2", "y3"]), notes
    c = SegCase(name, {"": rules}, make, flat=n <= 30)
    c.classes, c.last, c.star_act = n, last, star_act
    return c


def class_family(n):
    """the kernel family of a table of n classes in a dimension: 1 flat, 2 walk2, 0 the general walk (hostsim_last_kind)"""
    return 1 if n <= 30 else 2 if n <= 62 else 0


def check_classes(c):
    n = c.classes
    assert c.lt.stats["flat"] == (n <= 30) and c.lt.stats["walk2"] == (n <= 62), (c.name, c.lt.stats["flat"], c.lt.stats["walk2"], c.lt.stats["walk2_refused"])
    nt = c.notes
    assert effect(c, nt["last"], c.last[1]) == "EFFECT_ALLOW" and nt["last"] in decided_by(c, "", n - 1, "the rule of the highest class (%d)" % (n - 1))
    star = decided_by(c, "", n, "the `*` rule")
    assert effect(c, nt["star"], c.star_act) == "EFFECT_ALLOW" and nt["star"] in star
    outside = [i for i in star if all(r.startswith("x") for r in c.inputs[i]["principal"]["roles"])]
    assert len(outside) >= 3, (c.name, "roles outside the classes are decided through the `*` rule in %d requests only" % len(outside))
    assert any(len(i["principal"]["roles"]) == 1 for i in c.inputs) and any(len(i["principal"]["roles"]) == 2 for i in c.inputs)


# ---- the cases


CLASS_CASES = ["classes%d_%s" % (n, dim) for n in (29, 30, 31, 62, 63, 64) for dim in ("roles", "actions", "both")]
RECORDS = ["records%d" % n for n in (32, 33, 63, 64, 65, 128, 129)]
ITEMS = ["items%d" % n for n in (63, 64, 65)]
PADS = ["pad_60_4", "pad_60_1", "pad_61_1", "pad_five"]
COMPLEX = ["complex%d" % n for n in (15, 16, 17, 33)]
LEAVES = ["leaves%d" % n for n in (1, 4, 5, 8, 9)]
FLAT_CASES = RECORDS + ITEMS + PADS + COMPLEX + LEAVES + ["unpooled_dr", "two_scopes"]


def case(name):
    """the named cases, built once and kept beside test_scope_limits' own (its road bodies look them up by name)"""
    if name not in ts._CASES:
        if name.startswith("records"):
            c = records_case(name, int(name[7:]))
        elif name.startswith("items"):
            c = items_case(name, int(name[5:]))
        elif name == "pad_five":
            c = pad_five_case(name)
        elif name.startswith("pad_"):
            c = pad_case(name)
        elif name.startswith("complex"):
            c = complex_case(name, int(name[7:]))
        elif name.startswith("leaves"):
            c = leaves_case(name, int(name[6:]))
        elif name.startswith("classes"):
            c = classes_case(name)
        else:
            c = {"unpooled_dr": unpooled_case, "two_scopes": two_scopes_case}[name](name)
        assert 130 <= len(c.inputs) <= 200 and len(c.inputs) % 64
        ts._CASES[name] = c
    return ts._CASES[name]


def check_conditions(name):
    c = case(name)
    assert any(w["evaluationErrors"] for w in c.want[False]) and any(e["effect"] == "EFFECT_ALLOW" for w in c.want[False] for e in w["actions"].values())
    if name.startswith("records"):
        check_records(c, int(name[7:]))
    elif name.startswith("items"):
        check_items(c, int(name[5:]))
    elif name.startswith("pad_"):
        check_pad(c)
    elif name.startswith("complex"):
        check_complex(c, int(name[7:]))
    elif name.startswith("leaves"):
        check_leaves(c, int(name[6:]))
    elif name.startswith("classes"):
        check_classes(c)
    else:
        {"unpooled_dr": check_unpooled, "two_scopes": check_two_scopes}[name](c)


# ---- the roads


def trail_matches(c, masks, lenient, what):
    """one group per request: the effective policies (test_scope_limits.compare_trail, whose floor on the number of distinct sets a
    store of one policy cannot meet)"""
    have = [effective_policy_keys(c.lt.policy_keys, row) for row in masks]
    want = [w["effectivePolicies"] for w in c.want[lenient]]
    bad = [k for k in range(len(want)) if have[k] != want[k]]
    assert not bad, (c.name, what, lenient, bad[:3], have[bad[0]], want[bad[0]], c.inputs[bad[0]])
    assert len({tuple(k) for k in have}) >= 2


def check_on_emulator(name, road, monkeypatch, trail=False, kind=None):
    import hostsim_api
    c = case(name)
    ts.check_on_emulator(name, road, monkeypatch, kind=kind)
    if trail:
        groups = np.arange(c.batch.n_requests, dtype=np.uint32)
        for lenient in (False, True):
            flags = F_WANT_DR | (F_LENIENT if lenient else 0)
            res, m = hostsim_api.check_trail(c.lt, c.batch, groups, c.batch.n_requests, NOW, flags)
            assert hostsim_api.last_kind() == 1 and hostsim_api.lib().hostsim_last_masks() == ts.EMULATOR[road][2], (name, road, "trail")
            ts.compare(c, res, lenient, road + ", trail")
            trail_matches(c, m, lenient, road + ", trail")


def check_decisions(capi, name, plan_ok, compact=None):
    case(name)
    ts.check_decisions(capi, name, plan_ok, compact)


def check_trail(capi, name, plan_ok):
    case(name)
    ts.check_trail(capi, name, plan_ok)


# (test_scope_limits.check_cross does not take these stores unchanged: its resources stand at the scopes of a chain, and under the strict
# search a store of one scope then allows nothing - its own floor on the ALLOWs it must see fails.  The cross form is not run here.)


def _record_walk(p):
    return _flat(p, no=("_any", "_dr", "_staged", "_masks"))


def _masks(p):
    return _flat(p, "_masks", no=("_any",))


def _staged(p):
    return _flat(p, "_staged", no=("_any",))


def _class_plan(n):
    return {1: _record_walk, 2: lambda p: p.endswith("cbh_walk2_kernel"), 0: lambda p: p.startswith("cbh_check_kernel*")}[class_family(n)]


def _forced(plan_ok):
    return [(check_decisions, ("records64", plan_ok, True)), (check_decisions, ("records129", plan_ok, True)), (check_decisions, ("items63", plan_ok, True)),
            (check_decisions, ("complex16", plan_ok, True)), (check_decisions, ("leaves4", plan_ok, True)), (check_decisions, ("leaves5", plan_ok, True)),
            (check_decisions, ("leaves8", plan_ok, True)), (check_decisions, ("classes30_both", plan_ok, True))]


LIBRARY = {   # road -> (environment, [(body, arguments)])
    "default": ({}, [
        (check_decisions, ("records32", _record_walk, True)),
        (check_decisions, ("records33", _masks, True)),
        (check_decisions, ("records65", _masks, True)),
        (check_decisions, ("items64", _masks, True)),
        (check_decisions, ("items65", _masks, True)),
        (check_decisions, ("pad_61_1", _masks, True)),
        (check_decisions, ("pad_five", _masks, True)),
        (check_decisions, ("complex17", _masks, True)),          # (the mask and staged walks read compact inputs with derived roles too)
        (check_decisions, ("complex33", lambda p: _flat(p, "_any_masks"), False)),
        (check_decisions, ("leaves9", lambda p: _flat(p, "_any", no=("_staged", "_masks")), False)),
        (check_decisions, ("unpooled_dr", _masks, True)),
        (check_decisions, ("two_scopes", _masks, True)),
        (check_trail, ("unpooled_dr", lambda p: p == "cbh_check_flat_trail_kernel*_masks")),
    ] + [(check_decisions, (name, _class_plan(int(name[7:9])), True if int(name[7:9]) <= 30 else None)) for name in CLASS_CASES]),
    "mask_walk": ({"CBH_FLAT_MASKS": "1"}, _forced(_masks)),
    "staged_walk": ({"CBH_FORCE_STAGED": "1"}, _forced(_staged)),
    "four_waves_mask_walk": ({"CBH_FLAT_MASKS": "1"}, [
        (check_decisions, ("two_scopes", _masks, True)),
        (check_decisions, ("unpooled_dr", _masks, True)),
        (check_trail, ("unpooled_dr", lambda p: p == "cbh_check_flat_trail_kernel*_masks")),
    ]),
}
DEFAULT_IDS = ["%s-%s" % (b.__name__, a[0]) for b, a in LIBRARY["default"][1]]


def run_road(capi, road, only=None):
    for k, (body, args) in enumerate(LIBRARY[road][1]):
        if only is None or k in only:
            body(capi, *args)


def check_in_child(sim, road, lib=None, limit=600):
    ts.check_in_child(sim, road, lib=lib, limit=limit, module="test_segment_limits", library=LIBRARY)


# ---- CPU tier: the conditions the stores must meet (no kernel runs)


@pytest.mark.parametrize("name", FLAT_CASES)
def test_the_named_positions_decide(name):
    check_conditions(name)


@pytest.mark.parametrize("name", CLASS_CASES)
def test_the_highest_class_and_the_star_rule_decide(name):
    check_conditions(name)


def test_none_of_one_leaf_is_a_negated_one_leaf_item():
    lt = lower_rule_table(rule_table_from_policies(policies_from_docs([_policy("doc", "", [_rule(["a0"], "ALLOW", roles=["r0"], cond=tree("none", [FLAG]))])])))
    st, seg = lt.seg_stats, segments(lt)[""][0]
    assert st["items"] == st["items_one_level"] == 1 and st["complex_entries"] == 0, st
    assert seg["descs"] == [([0], 1 | 16)] and seg["simple_c"] == 1 and seg["rec_c"][0] == 0, seg["descs"]


# ---- CPU tier: the wave emulator


@pytest.mark.parametrize("road", ["record_walk", "staged_walk", "mask_walk"])
@pytest.mark.parametrize("name", FLAT_CASES)
def test_limits_on_emulator(name, road, monkeypatch):
    check_on_emulator(name, road, monkeypatch, trail=name in ("unpooled_dr", "records65", "complex17"))


@pytest.mark.parametrize("road", ["record_walk", "staged_walk", "mask_walk", "walk2", "general_walk"])
@pytest.mark.parametrize("name", CLASS_CASES)
def test_class_counts_on_emulator(name, road, monkeypatch):
    fam = class_family(int(name[7:9]))
    kind = {"walk2": 2 if fam else 0, "general_walk": 0}.get(road, fam)
    check_on_emulator(name, road, monkeypatch, kind=None if kind == ts.EMULATOR[road][1] else kind)


def test_a_bucket_of_33_records_takes_the_mask_walk_by_itself_on_emulator():
    """CBH_FLAT_STAGE_MIN: 32 records plan the record walk, 33 the mask walk, nothing forced"""
    import hostsim_api
    assert not any(k in os.environ for k in ("CBH_FLAT_MASKS", "CBH_FORCE_STAGED", "CBH_NO_FLAT"))
    for name, masks in (("records32", 0), ("records33", 1), ("classes30_both", 0), ("leaves9", 0), ("items64", 1)):
        c = case(name)
        res = hostsim_api.check(c.lt, c.batch, NOW, F_WANT_DR)
        assert hostsim_api.last_kind() == 1 and hostsim_api.lib().hostsim_last_masks() == masks, (name, hostsim_api.lib().hostsim_last_masks())
        ts.compare(c, res, False, "as planned")


# ---- CPU tier: the library's host side on the simulator


@pytest.fixture()
def engine():
    from sim_engine import sim_engine
    with sim_engine() as capi:
        yield capi


@pytest.mark.parametrize("k", range(len(DEFAULT_IDS)), ids=DEFAULT_IDS)
def test_as_planned_on_simulator(engine, k):
    run_road(engine, "default", only=(k,))


@pytest.mark.parametrize("road", ["mask_walk", "staged_walk"])
def test_forced_variant_on_simulator(road):
    check_in_child(True, road)


def test_four_waves_to_a_workgroup():
    from sim_engine import build_four_waves
    check_in_child(True, "four_waves_mask_walk", lib=build_four_waves())


# ---- GPU tier


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(DEFAULT_IDS)), ids=DEFAULT_IDS)
def test_as_planned_on_gpu(k):
    from cerbos_amd import capi
    run_road(capi, "default", only=(k,))


@pytest.mark.gpu
@pytest.mark.parametrize("road", ["mask_walk", "staged_walk"])
def test_forced_variant_on_gpu(road):
    # the same road's child on the simulator: 1.4 s (mask_walk), 4.6 s (staged_walk), most of it building the eight cases; on the
    # device the runtime's start and the first launch's code load come on top, tens of seconds at the worst
    check_in_child(os.environ.get("CBH_TEST_SIM_ENGINE") == "1", road, limit=120)
