"""cbh_walk2_kernel at its own fixed sizes: 15, 16 and 17 glob patterns in a dimension, 31, 32 and 33 role policies at one (version, scope),
15 .. 257 evaluation sites on one request's path, the shapes 8 x 4, 8 x 8 and 16 x 4 and what no shape holds, parent roles, principal
policies lane by lane, 64 derived roles.

What is pinned here (cbh_check_walk2.h, cbh_vm.h cbh_w2_class, cbh_image.h, lower/blob.py x_masks and the slots of the evaluation sites):
  CBH_W2_MAX_GLOBS              16 match bits per action and per role, two to a dword (gap[], rgp[]: bit 15 of an odd action or role is bit 31),
                                the `unsigned short` copies in LDS for the table's own strings up to CBH_W2_LDS_GLOB_STRINGS = 1024 of them,
                                global memory above; the bits of the batch's own strings; the parents' bits ORed in; a role policy's allow list
  CBH_W2_MAX_RP_ROLES           32 roles with a role policy at one (version, scope): place 31 of the CBH_B_RPROLES list is the only one that
                                denies; a slot's own role is met before its parents, those in name order; the note of a DENY keeps the lowest role
  CBH_W2_MAX_GSLOTS             256 slots, 16 to a 64-bit word (gacc, gres, site_cnt / site_list, w2_gwords), filed by both forms of the pre-pass,
                                read by the walk; generic sites in front of open ones, which a batch of plain scalars does not file
  cbh_w2_class                  8 x 4, 8 x 8, 16 x 4 and the general walk's share, by every bound; bit NA r + k of a 32- or 64-bit walk vector
  class masks                   62 role classes, parents and derived-role parent roles in the high dword (rs_hi, rm_hi)
  the principal pass            lanes grouped by principal, 56 groups in two waves
The reference is oracle/check.py everywhere, per tuple (effect, policy key, scope string) and per request (effectiveDerivedRoles, whether
evaluation errors were recorded; on the trail road the effective policies), with test_scope_limits.compare: nothing may be flagged
CBH_ST_UNSUPPORTED and no input is left out.  Every store is the smallest that reaches its position, every batch 130 .. 200 requests in
lane order.  `test_the_named_positions_decide` runs no kernel: it reads each position back from the lowered image (the glob index from
CBH_SEC_GBITS, the role's place from CBH_B_RPROLES, a site's slot from CBH_SEC_ROWX / _RPX / _DRX, classes from CBH_SEC_ROLE_CLASS),
finds the rule behind it and asks the oracle about the store without that rule - a compared field of a named request must change.
Every road asserts the kernels it ran: hostsim_last_kind / _walk_wide / _pre_split on the emulator (and its count of result words),
the plan's whole text on the library.

Tiers: *_on_emulator the kernels' source on the wave emulator - through walk2, through the general walk (CBH_NO_WALK2=1) and under both
forms of the pre-pass; *_on_simulator the library's host side (tests/sim_engine.py) as planned, with the trail where the case has role
policies, CBH_PRE_SPLIT=0 and =1 in a child process each, and four waves to a workgroup; *_on_gpu the same bodies on the device.
sites_mixed is not run on the general walk: its table has policy variables, whose failures that walk leaves to the trace pass.

What was found.  A store of 257 sites lowers for the general walk (stats["walk2_refused"]), but the image still carried M_GSLOTS_ALL = 257
and cbh_parse_image refused it ("blob evaluation-site slots out of range"): the table could not be loaded at all.  The loader now holds
the count to CBH_W2_MAX_GSLOTS only for an image flagged CBH_MF_WALK2 - the walk is the slots' one reader; images are unchanged.
On the parent test_*[sites_257] fail with that message (test_the_named_positions_decide[sites_257] passes), nothing else does.

Mutation check (each mutant on a scratch copy, the emulator's tests of this file; "older": tests/test_walk2.py, test_capacity_limits.py,
test_role_policy_base.py, test_glob_syntax.py, test_fuzz_parity.py, test_effective_policies.py, test_hostsim_golden.py and the emulator
tests of test_segment_limits.py).  w2 = test_walk2_on_emulator, pre = test_both_forms_of_the_pre_pass_on_emulator, words =
test_words_of_site_results_on_emulator.
   1  action glob bit 15 masked in act_bits16           killed: w2[globs_a16 | globs_1024 | globs_1025].  older: 1 of 549 fail (test_glob_syntax.py::test_kernel_source_decides_exotic_globs_like_the_oracle)
   2  role glob bit 15 masked in match_roles            killed: w2[globs_r16 | globs_1024 | globs_1025].  older: all 549 pass
   3  the LDS copies of the glob bits kept as 8 bits    killed: w2[globs_a15 | globs_a16 | globs_r15 | globs_r16 | globs_1024]; 1025 strings read global memory and pass.  older: all 549 pass
   4  the parents' glob bits not ORed in                killed: w2[globs_r15 | globs_r16 | globs_1024 | globs_1025].  older: all 549 pass
   5  n_rp capped at 31                                 killed: w2[rolepol_32 | rolepol_32_two | globs_1024 | globs_1025 (16 + 16 role policies)], pre[rolepol_32-*].  older: all 549 pass
   6  phase 1 of the role-policy visit (~own) skipped   killed: w2[rolepol_31 | rolepol_32 | rolepol_32_two], pre[rolepol_32-*].  older: 62 of 549 fail (in test_effective_policies.py, test_hostsim_golden.py, test_walk2.py)
   7  15 slots to a word where results are filed        killed: w2[sites_16 | sites_17 | sites_255 | sites_256 | split_16_1_plain | split_16_1_ints]; under the collector the
                                                        interpreter then writes beyond gres and the emulator aborts.  older: 5 of 549 fail (in test_effective_policies.py, test_hostsim_golden.py, test_walk2.py)
   8  the walk reads slot gslot & 0x7F                  killed: w2, pre and words[sites_255 | sites_256].  older: all 549 pass
   9  filed = gslot <= b.n_gslots                       survives, and must: `filed` is consulted for a site the inline code left open; n_gslots is either every slot or the
                                                        generic ones, and slot n_gslots is then the first OPEN site - a classified leaf over the inline columns (at most 16,
                                                        all among the 32 a launch scans for ints and lists), which a batch of plain scalars always decides inline.  No request
                                                        reaches the difference; a store built for it (an int in column 33) lowers that leaf as a generic site.  older: all 549 pass
  10  w2_gwords always from gslots_generic              killed: words[split_16_1_ints | split_15_2_ints] (the count of result words itself).  older: all 549 pass
  11  cbh_w2_class with < for <=                        act_cnt <= NA: w2[rolepol_31 | rolepol_32 | rolepol_32_two | shape_8x5 | shape_8x8], pre[rolepol_32-*].  older: all 549 pass
                                                        role_cnt <= NR (base): w2[shape_8x4_16x4] - only a batch whose wider walk is the 16 x 4 one leaves such a request undecided.  older: all 549 pass
                                                        role_cnt <= WIDE_NR: w2[globs_r15 | globs_r16 | rolepol_31 | rolepol_32 | rolepol_32_two | shape_8x8].  older: 3 of 549 fail (in test_effective_policies.py, test_walk2.py)
                                                        act_cnt <= AWIDE_NA: w2[globs_a15 | globs_a16 | shape_16x4].  older: all 549 pass
                                                        role_cnt <= NR (16 x 4): w2[shape_9x4 | shape_16x4].  older: all 549 pass
  12  the note's comparison r < (old >> 28) turned      killed: w2[globs_* | rolepol_* | shape_8x4 | shape_8x5 | shape_8x8 | shape_9x4 | shape_16x4 | shape_all], pre[rolepol_32-*].  older: 67 of 549 fail (in test_fuzz_parity.py, test_walk2.py)
  13  rs_hi dropped from match_roles                    killed: w2[globs_r15 | globs_r16 | globs_1024 | globs_1025 | rolepol_* | parents | derived], pre and words[derived].  older: 177 of 549 fail (in test_effective_policies.py, test_fuzz_parity.py, test_glob_syntax.py, test_segment_limits.py, test_walk2.py)
  14  the principal pass leaves after its first group   killed: w2[principals], pre[principals-*].  older: 57 of 549 fail (in test_effective_policies.py, test_fuzz_parity.py, test_walk2.py)
The file's CPU tier takes 66 s in one process (211 tests; the simulator libraries built - the four-wave one takes 35 s more where it is not), its
GPU tier 10 s (53 tests).
"""
import os
import struct

import numpy as np
import pytest

import test_scope_limits as ts
from cerbos_amd.engine import effective_policy_keys
from cerbos_amd.flatten import Flattener
from cerbos_amd.lower import blob as B
from cerbos_amd.lower.blob import lower_rule_table
from cerbos_amd.policy.loader import policies_from_docs
from cerbos_amd.ruletable.build import rule_table_from_policies
from oracle.check import EvalParams, RuleTableOracle
from test_scope_limits import API, F_LENIENT, F_WANT_DR, F_WANT_EP, NOW, _policy, _rule

A8 = ["a%d" % i for i in range(8)]


def expr(e):
    return {"match": {"expr": e}}


def role_policy(role, rules, scope="", parents=None):
    rp = {"role": role, "rules": rules}
    if parents:
        rp["parentRoles"] = list(parents)
    if scope:
        rp["scope"] = scope
    return {"apiVersion": API, "rolePolicy": rp}


def allows(actions, kind="doc", cond=None):
    r = {"resource": kind, "allowActions": list(actions)}
    if cond:
        r["condition"] = cond
    return r


def derived_roles(name, definitions):
    return {"apiVersion": API, "derivedRoles": {"name": name, "definitions": definitions}}


def principal_policy(principal, rules, scope=""):
    pp = {"principal": principal, "version": "default", "rules": rules}
    if scope:
        pp["scope"] = scope
    return {"apiVersion": API, "principalPolicy": pp}


def without(docs, key):
    """the store without one document (("doc", d)), without rule r of document d ((d, r): a resource policy's rule, a role policy's,
    a derived-role definition - which is kept, for nobody) or without action a of a principal policy's rule ((d, r, a))"""
    out = []
    for d, doc in enumerate(docs):
        if key[0] == "doc":
            if d != key[1]:
                out.append(doc)
            continue
        if d != key[0]:
            out.append(doc)
            continue
        (what, body), = [(k, v) for k, v in doc.items() if k != "apiVersion"]
        field = "definitions" if what == "derivedRoles" else "rules"
        items = list(body[field])
        if len(key) == 3:
            items[key[1]] = dict(items[key[1]], actions=[a for k, a in enumerate(items[key[1]]["actions"]) if k != key[2]])
        elif what == "derivedRoles":        # (rules name it: the definition stays, for a parent role no request has)
            items[key[1]] = dict(items[key[1]], parentRoles=["nobody at all"])
        else:
            del items[key[1]]
        out.append({"apiVersion": doc["apiVersion"], what: dict(body, **{field: items})})
    return out


class Reqs:
    """the requests of a case, in lane order"""

    def __init__(self, seed):
        self.rng, self.out = np.random.default_rng(seed), []

    def add(self, roles, acts, scope="", kind="doc", pid="p0", pattr=None, pscope=None, **rattr):
        i = len(self.out)
        p = {"id": pid, "roles": list(roles), "attr": dict(pattr or {})}
        if pscope:
            p["scope"] = pscope
        self.out.append({"requestId": "q%d" % i, "actions": list(acts), "principal": p,
                         "resource": {"kind": kind, "id": "d%d" % i, "attr": {k: v for k, v in rattr.items() if v is not None}, "scope": scope}})
        return i

    def pick(self, vals):
        return vals[int(self.rng.integers(0, len(vals)))]

    def some(self, vals, least=1, most=4):
        return [str(x) for x in self.rng.choice(vals, size=int(self.rng.integers(least, min(most, len(vals)) + 1)), replace=False)]

    def done(self, count=None):
        n = len(self.out)
        assert 130 <= n <= 200 and n % 64 and (count is None or n == count), n
        return self.out


class Case:
    """a store, its lowering, 130 .. 200 requests flattened in their own order (lane = index), and the oracle's answers under both
    scope searches - computed once, shared by every road, never changed (test_scope_limits.Case without the flat kernels' batch shape)"""

    def __init__(self, name, docs, make_requests, refused=None, lenient=(False, True)):
        self.name, self.docs, self.lenient = name, docs, lenient
        self.rt = rule_table_from_policies(policies_from_docs(docs))
        self.lt = lower_rule_table(self.rt)
        st = self.lt.stats
        assert not st["flat"], (name, "the table is flat")
        if refused is None:
            assert st["walk2"], (name, st["walk2_refused"])
        else:
            assert not st["walk2"] and refused in st["walk2_refused"], (name, st["walk2_refused"])
        self.kind = 2 if refused is None else 0
        self.inputs, self.notes = make_requests(self)
        self.batch = Flattener(self.lt).flatten(self.inputs, sort=False)
        assert self.batch.n_requests == len(self.inputs) and self.batch.tuple_perm is None
        self.orc = RuleTableOracle(self.rt)
        self.want = {len_: [self.orc.check(i, EvalParams(now_ns=NOW, lenient_scope_search=len_)) for i in self.inputs] for len_ in lenient}
        self.asm = ts._Assembler(self.lt)
        self.shapes = {(int(a), int(r)) for a, r in zip(self.batch.req_u32[9], self.batch.req_u32[7])}


# ---- the lowered image, read back


def section(lt, sid, dtype=np.uint32):
    n = struct.unpack_from("<I", lt.blob, 8)[0]
    for k in range(n):
        s, count, off, size, _ = struct.unpack_from("<IIQQQ", lt.blob, 32 + 32 * k)
        if s == sid:
            return count, np.frombuffer(lt.blob, dtype=dtype, count=size // np.dtype(dtype).itemsize, offset=off)
    raise KeyError(sid)


def directory(lt, what):
    """the directory's entries of one kind: [(k1, k2, k3, v0, v1, v2, v3)]"""
    n, slots = section(lt, B.SEC_HASH)
    return [tuple(int(x) for x in e[1:]) for e in slots[:n * 8].reshape(-1, 8) if int(e[0]) == what]


def glob_bits(lt, dim, string):
    """the match bits the image keeps for one of its own strings (CBH_SEC_GBITS: [dimension][string])"""
    k = lt.stats["strings"]
    return int(section(lt, B.SEC_GBITS, np.uint64)[1][dim * k + lt.string_ids[string]])


def glob_index(lt, dim, string):
    """the index of the one pattern that matches a string of the table"""
    bits = glob_bits(lt, dim, string)
    assert bits and not bits & (bits - 1), (string, bin(bits))
    return bits.bit_length() - 1


def rows_of(lt, kind, scope=""):
    """(first record, records) of a resource policy's bucket: one record per rule, in the rules' order"""
    (e,) = [e for e in directory(lt, B.B_RESOURCE) if e[1] == lt.string_ids[kind] and e[2] == lt.scope_index[scope]]
    return e[3], e[4]


def rowx(lt):
    return section(lt, B.SEC_ROWX)[1].reshape(-1, 8)


def fields(inp, w):
    return (tuple((w["actions"][a]["effect"], w["actions"][a]["policy"], w["actions"][a]["scope"]) for a in inp["actions"]),
            tuple(sorted(w["effectiveDerivedRoles"])), bool(w["evaluationErrors"]), tuple(w["effectivePolicies"]))


def decided_by(c, key, what, lenient=False):
    """-> the requests of which a compared field changes when `key` (see without()) leaves the store (asked of the oracle)"""
    orc = RuleTableOracle(rule_table_from_policies(policies_from_docs(without(c.docs, key))))
    out = [i for i, (inp, w) in enumerate(zip(c.inputs, c.want[lenient]))
           if fields(inp, orc.check(inp, EvalParams(now_ns=NOW, lenient_scope_search=lenient))) != fields(inp, w)]
    assert out, "%s: %s (%r) decides no compared field of any request" % (c.name, what, key)
    return out


def answer(c, i, action, lenient=False):
    e = c.want[lenient][i]["actions"][action]
    return e["effect"][7:], e["policy"]


def errors(c, i):
    return bool(c.want[c.lenient[0]][i]["evaluationErrors"])


# ---- 1. glob bits


def glob_docs(na, nr, pad=0):
    """kind `doc`: na action patterns g<i>:* - rule i names pattern i alone for r0, every fifth (i % 5 == 3) as the DENY of what the
    first rule allows by name; role lim<i> may do everything by the resource policy and pattern i alone by its role policy.  Kind
    `rep`: nr role patterns team<i>:* - rule i allows a0 to pattern i, every fifth denies a1, which the first rule allows to all;
    role kid<i> (a literal) has the table string team<i>:boss as its parent.  Every pattern matches one string the table holds
    (g<i>:lit, team<i>:boss) - its bit is read back from there - and strings only requests bring.  `pad`: constants of a condition of kind
    `pad`, which fill the table's strings (a literal action or role would take a class each, of which there are 62)."""
    docs = []
    if na:
        deny = [i for i in range(na) if i % 5 == 3]
        rules = [_rule(["g%02d:lit" % i for i in deny], "ALLOW", roles=["r0"]),
                 _rule(["g%02d:lit" % i for i in range(na) if i not in deny], "DENY", roles=["nobody"]),
                 _rule(["*"], "ALLOW", roles=["lim%02d" % i for i in range(na)])]
        rules += [_rule(["g%02d:*" % i], "DENY" if i in deny else "ALLOW", roles=["r0"]) for i in range(na)]
        docs.append(_policy("doc", "", rules))
        docs += [role_policy("lim%02d" % i, [allows(["g%02d:*" % i])]) for i in range(na)]
    if nr:
        rules = [_rule(["a1"], "ALLOW", roles=["*"])]
        rules += [_rule(["a1"] if i % 5 == 3 else ["a0"], "DENY" if i % 5 == 3 else "ALLOW", roles=["team%02d:*" % i]) for i in range(nr)]
        docs.append(_policy("rep", "", rules))
        docs += [role_policy("kid%02d" % i, [allows(["a0", "a1", "a2"], kind="rep")], parents=["team%02d:boss" % i]) for i in range(nr)]
    if pad:
        docs.append(_policy("pad", "", [_rule(["a0"], "ALLOW", roles=["r0"], cond=expr("R.attr.s in [%s]" % ", ".join('"f%04d"' % i for i in range(pad))))]))
    return docs


def glob_case(name, na, nr, strings=None, refused=None):
    docs = glob_docs(na, nr)
    if strings:     # fill the table to exactly `strings` strings
        have = lower_rule_table(rule_table_from_policies(policies_from_docs(glob_docs(na, nr, pad=1)))).stats["strings"]
        docs = glob_docs(na, nr, pad=1 + strings - have)

    def make(c):
        q, notes, lt = Reqs(100 * na + nr), {}, c.lt
        other = ["h:x", "g99:x", "g1:x", "zz"]
        if na:
            ix = {glob_index(lt, B.DIM_ACTION, "g%02d:lit" % i): i for i in range(na)}
            assert sorted(ix) == list(range(na)), ix
            top = ix[min(15, na - 1)]              # the pattern of index 15 (14 where there are 15)
            notes["a_top"], t_x, t_lit = top, "g%02d:x" % top, "g%02d:lit" % top
            for i in range(na):
                q.add(["r0"], ["g%02d:x" % i])
                q.add(["r0"], ["g%02d:lit" % i, "g%02d:x" % ((i + 1) % na)])
                q.add(["lim%02d" % i], ["g%02d:x" % i, "g%02d:x" % ((i + 1) % na), "g%02d:lit" % i])
            notes["a_odd"] = [q.add(["r0"], other[:k] + [t] + other[k:3]) for k in (1, 3) for t in (t_x, t_lit)]      # bit 31 of a gap dword
            notes["a_even"] = [q.add(["r0"], other[:k] + [t] + other[k:3]) for k in (0, 2) for t in (t_x, t_lit)]
            notes["a_last8"] = q.add(["r0"], ["n%d" % k for k in range(7)] + [t_x])
            notes["a_last16"] = [q.add(["nobody", "r0"], ["n%d" % k for k in range(15)] + [t]) for t in (t_x, t_lit)]
            notes["a_lim"] = q.add(["x0", "lim%02d" % top], ["zz", t_x, "g%02d:x" % ix[0]])
            q.add(["r0", "lim%02d" % top], ["zz", t_lit, "g%02d:x" % ix[0]])
        if nr:
            ix = {glob_index(lt, B.DIM_ROLE, "team%02d:boss" % i): i for i in range(nr)}
            assert sorted(ix) == list(range(nr)), ix
            top = ix[min(15, nr - 1)]
            notes["r_top"], t_x, t_boss, t_kid = top, "team%02d:x" % top, "team%02d:boss" % top, "kid%02d" % top
            for i in range(nr):
                q.add(["team%02d:x" % i], ["a0", "a1"], kind="rep")
                q.add(["x0", "team%02d:boss" % i], ["a1", "a0", "a2"], kind="rep")
                q.add(["kid%02d" % i], ["a0", "a1", "a2"], kind="rep")
            notes["r_odd"] = [q.add(["x0", "x1", "x2"][:k] + [t], ["a0", "a1"], kind="rep") for k in (1, 3) for t in (t_x, t_boss, t_kid)]      # bit 31 of an rgp dword
            notes["r_even"] = [q.add(["x0", "x1", "x2"][:k] + [t], ["a0", "a1"], kind="rep") for k in (0, 2) for t in (t_x, t_boss, t_kid)]
            notes["r_last8"] = [q.add(["x%d" % k for k in range(7)] + [t], ["a2", "a1", "a0"], kind="rep") for t in (t_x, t_boss, t_kid)]
            q.add(["team:x", "team99:x", "kid", "x0"], ["a0", "a1"], kind="rep")
        while len(q.out) < (197 if na and nr else 137 if na + nr < 17 else 139):
            if na and (not nr or q.rng.random() < 0.5):
                q.add(q.some(["r0", "nobody", "x0"] + ["lim%02d" % i for i in range(na)], most=3),
                      q.some(["g%02d:%s" % (i, s) for i in range(na) for s in ("x", "lit", "")] + other, most=8 if q.rng.random() < 0.8 else 12))
            else:
                q.add(q.some(["team%02d:%s" % (i, s) for i in range(nr) for s in ("x", "boss")] + ["kid%02d" % i for i in range(nr)] + ["x0", "x1"], most=5),
                      q.some(["a0", "a1", "a2", "zz"], most=4), kind="rep")
        return q.done(), notes
    c = Case(name, docs, make, refused=refused, lenient=(False,))
    assert c.lt.stats["globs"][:2] == [na, nr], c.lt.stats["globs"]
    if strings:
        assert c.lt.stats["strings"] == strings
    return c


def doc_index(c, what, name):
    (d,) = [d for d, doc in enumerate(c.docs) if what in doc and name in (doc[what].get("role"), doc[what].get("resource"), doc[what].get("principal"), doc[what].get("name"))
            and not doc[what].get("scope")]
    return d


def check_globs(c):
    nt = c.notes
    assert any(errors(c, i) for i in range(len(c.inputs))) is False       # (no conditions in these stores)
    if "a_top" in nt:
        top, d = nt["a_top"], doc_index(c, "resourcePolicy", "doc")
        rule = [k for k, r in enumerate(c.docs[d]["resourcePolicy"]["rules"]) if r["actions"] == ["g%02d:*" % top]]
        first, count = rows_of(c.lt, "doc")
        assert count == len(c.docs[d]["resourcePolicy"]["rules"]) and len(rule) == 1
        if c.kind == 2:
            want_bit = min(15, c.lt.stats["globs"][0] - 1)
            assert int(rowx(c.lt)[first + rule[0], 1]) == 1 << want_bit, "the rule of pattern %d does not carry glob bit %d" % (top, want_bit)
            rp = section(c.lt, B.SEC_RPX)[1].reshape(-1, 16)
            assert sum(int(r[6]) == 1 << want_bit for r in rp) == 1, "no role-policy rule allows by glob bit %d" % want_bit
        by_rule = decided_by(c, (d, rule[0]), "the rule of the action pattern at the highest index")
        for i in nt["a_odd"] + nt["a_even"] + [nt["a_last8"]] + nt["a_last16"]:
            t = [a for a in c.inputs[i]["actions"] if a.startswith("g%02d:" % top)][0]
            if top % 5 != 3 or t.endswith("lit"):      # (a string only the DENY's pattern matches is denied with or without it)
                assert i in by_rule and answer(c, i, t)[0] == ("DENY" if top % 5 == 3 else "ALLOW"), (c.name, i, t)
        by_rp = decided_by(c, (doc_index(c, "rolePolicy", "lim%02d" % top), 0), "the role policy's allowActions pattern at the highest index")
        assert nt["a_lim"] in by_rp and [answer(c, nt["a_lim"], a) for a in c.inputs[nt["a_lim"]]["actions"]] == \
            [("DENY", "role.lim%02d.vdefault" % top), ("ALLOW", "resource.doc.vdefault"), ("DENY", "role.lim%02d.vdefault" % top)]
        assert len(c.inputs[nt["a_last16"][0]]["actions"]) == 16 and len(c.inputs[nt["a_last8"]]["actions"]) == 8
    if "r_top" in nt:
        top, d = nt["r_top"], doc_index(c, "resourcePolicy", "rep")
        rule = [k for k, r in enumerate(c.docs[d]["resourcePolicy"]["rules"]) if r["roles"] == ["team%02d:*" % top]]
        first, count = rows_of(c.lt, "rep")
        assert count == len(c.docs[d]["resourcePolicy"]["rules"]) and len(rule) == 1
        if c.kind == 2:
            want_bit = min(15, c.lt.stats["globs"][1] - 1)
            assert int(rowx(c.lt)[first + rule[0], 1]) == 1 << (16 + want_bit), "the rule of role pattern %d does not carry glob bit %d" % (top, want_bit)
        by_rule = decided_by(c, (d, rule[0]), "the rule of the role pattern at the highest index")
        act, eff = ("a1", "DENY") if top % 5 == 3 else ("a0", "ALLOW")
        for i in nt["r_odd"] + nt["r_even"] + nt["r_last8"]:
            assert i in by_rule and answer(c, i, act)[0] == eff, (c.name, i)
        assert len(c.inputs[nt["r_last8"][0]]["principal"]["roles"]) == 8


GLOB_CASES = {"globs_a15": (15, 0), "globs_a16": (16, 0), "globs_r15": (0, 15), "globs_r16": (0, 16), "globs_1024": (16, 16, 1024), "globs_1025": (16, 16, 1025),
              "globs_a17": (17, 0, None, "more than 16 glob patterns in a dimension"), "globs_r17": (0, 17, None, "more than 16 glob patterns in a dimension")}


# ---- 2. role policies in one scope


def minus(*acts):
    return [a for a in A8 if a not in acts]


def rolepol_docs(n, two_scopes=False):
    """Roles rp00 .. with a role policy each at scope "" (and at s0); the resource policy allows everything to everybody (at s0: a0 ..
    a3 only, the rest is decided one scope up).  Every role policy allows all eight actions, but: the LAST role in name order lacks
    a1 and a5 (at s0: a2) - the only one that denies those; rp10 lacks a6, its parents rp05 (lacks a6, a7) and rp20 (lacks a7) are
    defined at scope "" only; rp03 allows a3 under a condition that is an evaluation site."""
    roles = ["rp%02d" % i for i in range(n)]
    last = sorted(roles)[-1]
    docs = [_policy("doc", "", [_rule(["*"], "ALLOW", roles=["*"])])]
    if two_scopes:
        docs.append(_policy("doc", "s0", [_rule(A8[:4], "ALLOW", roles=["*"])]))
    lacks = {last: ("a1", "a5"), "rp10": ("a6",), "rp05": ("a6", "a7"), "rp20": ("a7",)}
    for r in roles:
        rules = [allows(["a3"], cond=expr("R.attr.picks.exists(x, x == 3)")), allows(minus("a3"))] if r == "rp03" else [allows(minus(*lacks.get(r, ())))]
        docs.append(role_policy(r, rules, parents=["rp05", "rp20"] if r == "rp10" else None))
        if two_scopes:
            docs.append(role_policy(r, [allows(minus("a2") if r == last else A8)], scope="s0"))
    return docs


def rolepol_case(name, n, two_scopes=False, refused=None):
    last = "rp%02d" % (n - 1)

    def make(c):
        q, nt = Reqs(200 + n), {}
        scopes = ("", "s0") if two_scopes else ("",)
        nt["last"] = [q.add([last], ["a0", "a1", "a5", "a2"], scope=s, picks=[3]) for s in scopes]
        nt["own"] = q.add(["rp10"], ["a6", "a7", "a0"], picks=[3])              # its own policy denies a6; of its parents' rp05's is met first
        nt["parent_only"] = q.add(["rp10"], ["a7"], picks=[3])                  # ... which its own allows: only the second phase denies
        q.add(["rp20"], ["a7", "a6"], picks=[3])
        q.add(["rp05", "rp20"], ["a6", "a7"], picks=[3])
        nt["site"] = [q.add(["rp03"], ["a3", "a0"], picks=p) for p in ([3], [4, 5], None, [5, 3])]
        if two_scopes:
            nt["other_scope"] = q.add(["rp10"], ["a6", "a7", "a0"], scope="s0", picks=[3])      # the parents are defined at "" only
        pool = ["rp%02d" % i for i in range(n)]
        for k in range(1, 9):                           # one to eight roles, of which none, one or several have a policy
            for with_policy in (0, 1, min(k, 3), k):
                others = [str(r) for r in q.rng.permutation(pool[:-1])[:max(0, with_policy - 1)]]
                roles = ["plain%d" % j for j in range(k - with_policy)] + ([last] if with_policy else []) + others
                q.add([str(r) for r in q.rng.permutation(roles)], ["a1", "a5", "a6", "a3"], scope=q.pick(scopes), picks=q.pick([[3], [4], None]))
        while len(q.out) < 167:
            q.add(q.some(pool + [last, "rp10", "rp03", "rp05", "plain0", "plain1"], most=4), q.some(A8 + ["zz"], most=8), scope=q.pick(scopes + ("zz",) if two_scopes else scopes),
                  kind="other" if q.rng.random() < 0.04 else "doc", picks=q.pick([[3], [4], None, [3, 4]]))
        return q.done(), nt
    return Case(name, rolepol_docs(n, two_scopes), make, refused=refused, lenient=(False, True) if two_scopes else (False,))


def rp_roles(lt, scope=""):
    """the roles with a role policy at (default, scope) as the image lists them (CBH_B_RPROLES -> the pool)"""
    (e,) = [e for e in directory(lt, B.B_RPROLES) if e[0] == lt.string_ids["default"] and e[1] == lt.scope_index[scope]]
    pool = section(lt, B.SEC_U32POOL)[1]
    return [lt.strings[int(s)] for s in pool[e[3]:e[3] + e[4]]]


def rp_doc(c, role, scope=""):
    (d,) = [d for d, doc in enumerate(c.docs) if doc.get("rolePolicy", {}).get("role") == role and doc["rolePolicy"].get("scope", "") == scope]
    return d


def check_rolepol(c):
    n, nt = int(c.name.split("_")[1]), c.notes
    two = "other_scope" in nt
    last = sorted("rp%02d" % i for i in range(n))[-1]
    for scope in ("", "s0") if two else ("",):
        listed = rp_roles(c.lt, scope)
        assert len(listed) == n and listed == sorted(listed) and listed[n - 1] == last, (c.name, scope, listed)
    i = nt["last"][0]
    assert i in decided_by(c, ("doc", rp_doc(c, last)), "the role policy at place %d of the scope's list" % (n - 1))
    assert [answer(c, i, a) for a in ("a0", "a1", "a5")] == [("ALLOW", "resource.doc.vdefault"), ("DENY", "role.%s.vdefault" % last), ("DENY", "role.%s.vdefault" % last)]
    if two:
        i = nt["last"][1]
        assert i in decided_by(c, ("doc", rp_doc(c, last, "s0")), "the role policy at place %d of the list at s0" % (n - 1))
        assert i in decided_by(c, ("doc", rp_doc(c, last)), "the role policy at place %d of the list at the root, from s0" % (n - 1))
        assert [answer(c, i, a) for a in ("a0", "a1", "a5", "a2")] == [("ALLOW", "resource.doc.vdefault/s0"), ("ALLOW", "resource.doc.vdefault/s0"),
                                                                       ("DENY", "role.%s.vdefault" % last), ("DENY", "role.%s.vdefault/s0" % last)], c.want[False][i]
        assert [answer(c, nt["other_scope"], a)[0] for a in ("a6", "a7", "a0")] == ["DENY", "ALLOW", "ALLOW"], "parents defined at another scope count"
    assert [answer(c, nt["own"], a) for a in ("a6", "a7", "a0")] == [("DENY", "role.rp10.vdefault"), ("DENY", "role.rp05.vdefault"), ("ALLOW", "resource.doc.vdefault")]
    assert nt["own"] in decided_by(c, (rp_doc(c, "rp10"), 0), "the slot's own role policy") and nt["own"] in decided_by(c, ("doc", rp_doc(c, "rp05")), "the first parent's")
    assert answer(c, nt["parent_only"], "a7") == ("DENY", "role.rp05.vdefault")
    rpx = section(c.lt, B.SEC_RPX)[1].reshape(-1, 16)
    if c.kind == 2:
        slots = [int(r[3]) & 0xFFFF for r in rpx if int(r[2]) != B.NONE]
        assert slots == [0] * len(slots) and c.lt.stats["gslots"] == (1, 1), (c.name, "the role-policy condition is no site", slots)
    assert [(answer(c, i, "a3")[0], errors(c, i)) for i in nt["site"]] == [("ALLOW", False), ("DENY", False), ("DENY", True), ("ALLOW", False)]
    assert nt["site"][0] in decided_by(c, (rp_doc(c, "rp03"), 0), "the role-policy rule whose condition is a site")
    assert len({len(i["principal"]["roles"]) for i in c.inputs}) == 8


ROLEPOL_CASES = {"rolepol_31": (31,), "rolepol_32": (32,), "rolepol_32_two": (32, True), "rolepol_33": (33, False, "more than 32 role policies in one scope")}


# ---- 3. evaluation sites


def pick_cond(k):
    """site k: satisfied by the requests whose `picks` hold k (bump = 0); no `picks`: an evaluation error; a list for `bump`: outside
    the device subset (the arithmetic + is handed a list)"""
    return expr("R.attr.picks.exists(x, x + R.attr.bump == %d)" % k)


def site_pair(k):
    return "r%d" % ((k // 8) % 4), A8[k % 8]


def site_denies(k):
    return k % 3 == 2 and k >= 32        # (rule k - 32, of the same walk, allows)


def site_docs(n):
    """rule 0 allows everything to `boss`; rule 1 + k is site k: the walk site_pair(k) under pick_cond(k).  Sites k, k + 32, k + 64 ...
    lie on one walk; k and k + 16 on the same action of two roles."""
    rules = [_rule(["*"], "ALLOW", roles=["boss"])]
    rules += [_rule([site_pair(k)[1]], "DENY" if site_denies(k) else "ALLOW", roles=[site_pair(k)[0]], cond=pick_cond(k)) for k in range(n)]
    return [_policy("doc", "", rules)]


def rule_slots(lt, kind="doc", scope=""):
    """the evaluation-site slot of every rule's own condition, in the rules' order (CBH_SEC_ROWX, dword 0, low half)"""
    first, count = rows_of(lt, kind, scope)
    return [int(x) & 0xFFFF for x in rowx(lt)[first:first + count, 0]]


NEAR = (-128, -16, 16, 128)


def site_case(name, n, everyone=False, refused=None):
    def make(c):
        q, nt = Reqs(300 + n + everyone), {}
        slots = rule_slots(c.lt)
        assert len(slots) == n + 1 and slots[0] == B.GSLOT_NONE
        if refused is None:
            assert sorted(slots[1:]) == list(range(n)), (name, "one slot per site")
            rule_of = {s: k for k, s in enumerate(slots[1:])}
        else:
            assert set(slots) == {B.GSLOT_NONE}
            rule_of = {k: k for k in range(n)}
        nt["rule_of"] = rule_of
        if everyone:        # every request reaches site 0's slot: its list is filled to the batch's size, from three waves
            while len(q.out) < 163:
                q.add(["r0"] + q.some(["r1", "r2", "r3", "boss"], 0, 2), ["a0"] + q.some(A8[1:], 0, 5), picks=[int(x) for x in q.rng.choice(n, size=int(q.rng.integers(0, 5)))] or None, bump=0)
            return q.done(163), nt
        for s in sorted({0, 14, 15, 16, n - 2, n - 1} | ({127, 128} if n > 128 else set())):
            if s >= n:
                continue
            k = rule_of[s]
            role, act = site_pair(k)
            sat = [k, k - 32] if site_denies(k) else [k]
            nt[s] = dict(sat=q.add([role], [act], picks=sat, bump=0), unsat=q.add([role], [act], picks=[k + 1000] + sat[1:], bump=0),
                         err=q.add([role], [act], bump=0), unsup=q.add(["boss", role], [act], picks=sat, bump=[1]))
        for s in [s for s in (0, 1, 15, 16, 17, 31, 112, 127, 128, 143, 144, 239, 240, n - 1) if s < n]:
            k = rule_of[s]
            role, act = site_pair(k)
            near = [rule_of[s + d] for d in NEAR if 0 <= s + d < n]
            q.add([role] + [site_pair(j)[0] for j in near if site_pair(j)[0] != role][:3], [act], picks=[k], bump=0)        # site k alone holds ...
            q.add([role] + [site_pair(j)[0] for j in near if site_pair(j)[0] != role][:3], [act], picks=near or [n + 5], bump=0)   # ... the sites 16 and 128 slots away do
        for j in range(6):
            q.add(["r0", "r1", "r2", "r3"], A8, picks=[int(x) for x in q.rng.choice(n, size=4 * j)] or None, bump=0 if j != 3 else None)     # every site of the table
        while len(q.out) < 163:
            q.add(q.some(["r0", "r1", "r2", "r3", "boss", "x0"], most=3), q.some(A8, most=4), picks=[int(x) for x in q.rng.choice(n + 3, size=int(q.rng.integers(0, 9)))] or None,
                  bump=q.pick([0, 0, 0, 0, 0, None, 1]))
        return q.done(163), nt
    return Case(name, site_docs(n), make, refused=refused, lenient=(False,))


def check_sites(c):
    n, nt = int(c.name.split("_")[1]), c.notes
    assert c.lt.stats["gslots"] == (n, n)
    if c.name.endswith("_all"):
        assert all("r0" in i["principal"]["roles"] and "a0" in i["actions"] for i in c.inputs) and len(c.inputs) > 128
        decided_by(c, (0, 1), "the site every request reaches")
        assert any(errors(c, i) for i in range(len(c.inputs)))
        return
    for s, at in nt.items():
        if s == "rule_of":
            continue
        k = nt["rule_of"][s]
        act, decides = site_pair(k)[1], decided_by(c, (0, 1 + k), "the site of slot %d (rule %d)" % (s, k))
        assert at["sat"] in decides and answer(c, at["sat"], act)[0] == ("DENY" if site_denies(k) else "ALLOW"), (c.name, s)
        assert answer(c, at["unsat"], act)[0] == ("ALLOW" if site_denies(k) else "DENY") and not errors(c, at["unsat"]), (c.name, s)
        assert errors(c, at["err"]) and answer(c, at["err"], act)[0] == "DENY", (c.name, s)
        assert not errors(c, at["unsup"]) and answer(c, at["unsup"], act)[0] == "ALLOW", (c.name, s)      # (behind the role that allowed: never evaluated by the reference)
    assert {0, 15, 16, n - 1} & set(nt) == {s for s in (0, 15, 16, n - 1) if s < n}


def split_docs(n_generic, n_open):
    """generic sites (a string function: evaluated by the pre-pass for every batch) in front of open ones (an ordering leaf, decided
    inline unless the batch brings an int or a list): the generic / open split at a word boundary of the site results"""
    rules = [_rule([site_pair(k)[1]], "ALLOW", roles=[site_pair(k)[0]], cond=expr('R.attr.code.contains("<%d>")' % k)) for k in range(n_generic)]
    rules += [_rule([site_pair(k)[1]], "ALLOW", roles=[site_pair(k)[0]], cond=expr("R.attr.v > %d.0" % k)) for k in range(n_generic, n_generic + n_open)]
    return [_policy("doc", "", rules)]


def split_case(name, n_generic, n_open, ints):
    n = n_generic + n_open

    def make(c):
        q, nt = Reqs(400 + 10 * n_generic + ints), {}
        slots = rule_slots(c.lt)
        assert sorted(slots[:n_generic]) == list(range(n_generic)) and sorted(slots[n_generic:]) == list(range(n_generic, n)), (name, slots)
        nt["rule_of"] = rule_of = {s: k for k, s in enumerate(slots)}
        num = (lambda x: int(x)) if ints else float
        for s in (0, n_generic - 1, n_generic, n - 1):
            k = rule_of[s]
            role, act = site_pair(k)
            nt[s] = dict(sat=q.add([role], [act], code="<%d>" % k, v=num(k + 1)), unsat=q.add([role], [act], code="<%d>" % (k + 16), v=num(k - 1)),
                         err=q.add([role], [act]))
        for k in range(n):
            role, act = site_pair(k)
            q.add([role, site_pair(k + 16)[0]], [act], code="<%d>" % k, v=num(k + 1) if k % 2 else float(k + 1))
            q.add([role, site_pair(k + 16)[0]], [act, A8[(k + 1) % 8]], code="<%d><%d>" % (k + 16, k + 1), v=float(k) + 0.5)
        while len(q.out) < 137:
            q.add(q.some(["r0", "r1", "r2", "x0"], most=3), q.some(A8, most=8), code="".join("<%d>" % x for x in q.rng.choice(n + 2, size=int(q.rng.integers(0, 4)))) or None,
                  v=q.pick([None, 3.5, 15.5, 16.5, 17.5] + ([4, 16, 17, [17.5]] if ints else [])))
        return q.done(137), nt
    c = Case(name, split_docs(n_generic, n_open), make, lenient=(False,))
    c.words, c.ints = ((n if ints else n_generic) + 15) // 16, ints
    return c


def check_split(c):
    n_generic, n_open = (int(x) for x in c.name.split("_")[1:3])
    assert c.lt.stats["gslots"] == (n_generic, n_generic + n_open)
    tags = {type(i["resource"]["attr"].get("v")) for i in c.inputs}
    assert (int in tags and list in tags) == c.ints, tags
    for s, at in c.notes.items():
        if s == "rule_of":
            continue
        k = c.notes["rule_of"][s]
        act = site_pair(k)[1]
        assert at["sat"] in decided_by(c, (0, k), "the site of slot %d (rule %d)" % (s, k)) and answer(c, at["sat"], act)[0] == "ALLOW"
        assert answer(c, at["unsat"], act)[0] == "DENY" and not errors(c, at["unsat"]) and errors(c, at["err"])


def mixed_docs():
    """a site on each carrier: a derived role's definition (100), a role-policy rule (101), a principal-policy rule (102), the probe
    of a policy's variables (`first` fails for an empty list; rule 1 reads it: 103) and a rule (104)"""
    return [derived_roles("dr_sites", [{"name": "picker", "parentRoles": ["r0"], "condition": pick_cond(100)}]),
            {"apiVersion": API, "resourcePolicy": {"resource": "doc", "version": "default", "importDerivedRoles": ["dr_sites"], "variables": {"local": {"first": "R.attr.picks[0]"}}, "rules": [
                _rule(["a0"], "ALLOW", derived=["picker"]), _rule(["a3"], "ALLOW", roles=["r1"], cond=expr("V.first == 103")),
                _rule(["a4"], "ALLOW", roles=["r1"], cond=pick_cond(104)), _rule(["*"], "ALLOW", roles=["rp"])]}},
            role_policy("rp", [allows(["a1"], cond=pick_cond(101)), allows(["a5"])]),
            principal_policy("p7", [{"resource": "doc", "actions": [{"action": "a2", "effect": "EFFECT_ALLOW", "condition": pick_cond(102)}, {"action": "a6", "effect": "EFFECT_DENY"}]}])]


def mixed_case(name):
    def make(c):
        q, nt = Reqs(500), {}
        nt["dr"] = [q.add(["r0"], ["a0"], picks=p, bump=0) for p in ([100], [101], None)]
        nt["rp"] = [q.add(["rp"], ["a1", "a5"], picks=p, bump=0) for p in ([101], [100], None)]
        nt["pp"] = [q.add(["x0"], ["a2", "a6"], pid="p7", picks=p, bump=0) for p in ([102], [101], None)]
        nt["var"] = [q.add(["r1"], ["a3"], picks=p, bump=0) for p in ([103], [102, 103], [])]
        nt["rule"] = [q.add(["r1"], ["a4"], picks=p, bump=0) for p in ([7, 104], [7], None)]
        while len(q.out) < 141:
            q.add(q.some(["r0", "r1", "rp", "x0"], most=4), q.some(A8, most=8), pid=q.pick(["p0", "p7", "p7"]),
                  picks=q.pick([None, []]) if q.rng.random() < 0.2 else [int(x) for x in q.rng.choice(range(99, 106), size=int(q.rng.integers(1, 4)))], bump=q.pick([0, 0, 0, None]))
        return q.done(141), nt
    return Case(name, mixed_docs(), make, lenient=(False,))


def check_mixed(c):
    nt, lt = c.notes, c.lt
    first, count = rows_of(lt, "doc")
    rx = rowx(lt)[first:first + count]
    drx = section(lt, B.SEC_DRX)[1].reshape(-1, 16)
    rpx = section(lt, B.SEC_RPX)[1].reshape(-1, 16)
    pp = {int(rowx(lt)[e[3], 0]) & 0xFFFF for e in directory(lt, B.B_PRINCIPAL)}
    assert len(pp) == 1 and len(drx) == 1
    # (the definition's condition has two: one where a rule names the derived role, one where the scope's derived roles are evaluated)
    slots = {"rule": int(rx[2, 0]) & 0xFFFF, "var": int(rx[1, 0]) & 0xFFFF, "probe": int(rx[1, 6]) & 0xFFFF, "dr": int(drx[0, 5]) & 0xFFFF,
             "dr on its rule": int(rx[0, 0]) >> 16, "rp": int(rpx[0, 3]) & 0xFFFF, "pp": pp.pop()}
    total = lt.stats["gslots"][1]
    assert all(s < total for s in slots.values()) and len(set(slots.values())) == len(slots) == total, (slots, lt.stats["gslots"])
    for what, key in (("dr", (0, 0)), ("rp", (2, 0)), ("pp", (3, 0, 0)), ("var", (1, 1)), ("rule", (1, 2))):
        assert nt[what][0] in decided_by(c, key, "the site on " + what), what
    assert [errors(c, i) for i in nt["var"]] == [False, False, True] and [errors(c, i) for i in nt["pp"]] == [False, False, True]
    assert [answer(c, i, "a2")[0] for i in nt["pp"]] == ["ALLOW", "DENY", "DENY"] and [answer(c, i, "a1")[0] for i in nt["rp"]] == ["ALLOW", "DENY", "DENY"]
    assert c.want[False][nt["dr"][0]]["effectiveDerivedRoles"] == ["picker"] and not c.want[False][nt["dr"][1]]["effectiveDerivedRoles"]


SITE_CASES = {"sites_15": (15,), "sites_16": (16,), "sites_17": (17,), "sites_255": (255,), "sites_256": (256,), "sites_16_all": (16, True),
              "sites_257": (257, False, "more than 256 evaluation sites on one request's path")}
SPLIT_CASES = {"split_16_1_plain": (16, 1, False), "split_16_1_ints": (16, 1, True), "split_15_2_plain": (15, 2, False), "split_15_2_ints": (15, 2, True)}


# ---- 4. shapes


SHAPES = [(8, 4), (8, 5), (8, 8), (9, 4), (16, 4), (9, 5), (8, 9), (17, 4)]


def w2_class(na, nr):
    """cbh_vm.h cbh_w2_class: 0 the base walk, 1 the one with more roles, 2 the one with more actions, 3 the general walk"""
    if na <= 8:
        return 0 if nr <= 4 else 1 if nr <= 8 else 3
    return 2 if na <= 16 and nr <= 4 else 3


def shape_docs():
    """the one walk (key, hit) allows (h1 .. h16 are key's too: the trail's requests); lim and lim2 may do everything by the resource policy and `ok` (lim2: `ok2` too) by their role
    policies - whatever else they ask for is denied in the name of the FIRST of them among the request's roles"""
    return [_policy("doc", "", [_rule(["hit"], "ALLOW", roles=["key"]), _rule(["*"], "ALLOW", roles=["lim", "lim2"]), _rule(["h%d" % i for i in range(1, 17)], "ALLOW", roles=["key"])]),
            role_policy("lim", [allows(["ok"])]), role_policy("lim2", [allows(["ok", "ok2"])])]


def shape_requests(q, na, nr, nt):
    xs, ns = ["x%d" % i for i in range(nr)], ["n%d" % i for i in range(na)]
    at = nt.setdefault((na, nr), {})
    at["top"] = q.add(xs[:nr - 1] + ["key"], ns[:na - 1] + ["hit"])                    # the highest bit of the walk vector decides
    at["bit0"] = q.add(["key"] + xs[:nr - 1], ["hit"] + ns[:na - 1])
    at["deny_last"] = q.add(xs[:nr - 1] + ["lim"], ns[:na - 1] + ["ok"])               # a role-policy DENY of the last role (8 roles: index 7)
    at["deny_both"] = (q.add(["lim"] + xs[:nr - 2] + ["lim2"], ns[:na - 2] + ["ok2", "ok"]), q.add(["lim2"] + xs[:nr - 2] + ["lim"], ["ok2", "ok"] + ns[:na - 2]))
    hits = ["hit"] + ["h%d" % i for i in range(1, na)]      # everything the first / the last role allows: the roles behind it are never walked
    at["trail"] = (q.add(["key"] + xs[:nr - 2] + ["lim"], hits), q.add(["lim"] + xs[:nr - 2] + ["key"], hits))


def shape_case(name, shapes, tiny=False):
    def make(c):
        q, nt = Reqs(600 + 17 * len(shapes) + shapes[0][0]), {}
        if tiny:        # fewer than four tuples in the batch: no speculative load of four action ids
            nt["tiny"] = [q.add(["x0", "key"], ["n0", "hit"]), q.add(["lim"], ["zz"])]
            return q.out, nt
        if len(shapes) == len(SHAPES):     # requests of four actions at act_off == 4 * req (the first three) and elsewhere; the batch's last
            for roles in (["key"], ["lim"], ["x0", "key"]):
                q.add(roles, ["n0", "hit", "ok", "n1"])
            q.add(["key"], ["hit"])
            nt["four"] = [q.add(["x0", "key", "lim"], ["n0", "n1", "ok", "hit"]), q.add(["lim2", "key"], ["hit", "n0", "ok2", "n1"])]
        for na, nr in shapes:
            shape_requests(q, na, nr, nt)
        pool_r, pool_a = ["key", "lim", "lim2"] + ["x%d" % i for i in range(9)], ["hit", "ok", "ok2"] + ["n%d" % i for i in range(17)]
        while len(q.out) < (162 if len(shapes) == len(SHAPES) else 137):
            na, nr = shapes[int(q.rng.integers(0, len(shapes)))]
            q.add([str(r) for r in q.rng.permutation(pool_r)[:nr]], [str(a) for a in q.rng.permutation(pool_a)[:na]])
        if len(shapes) == len(SHAPES):
            nt["last"] = q.add(["x0", "x1", "key"], ["n0", "n1", "n2", "hit"])
        return q.done(), nt
    return Case(name, shape_docs(), make, lenient=(False,))


def check_shapes(c):
    nt = c.notes
    off, cnt = c.batch.req_u32[8].astype(np.int64), c.batch.req_u32[9].astype(np.int64)
    if "tiny" in nt:
        assert c.batch.n_tuples == 3 and answer(c, nt["tiny"][0], "hit")[0] == "ALLOW" and answer(c, nt["tiny"][1], "zz") == ("DENY", "role.lim.vdefault")
        return
    if "four" in nt:
        assert all(cnt[i] == 4 and off[i] == 4 * i for i in range(3)) and all(cnt[i] == 4 and off[i] != 4 * i for i in nt["four"] + [nt["last"]])
        assert nt["last"] == len(c.inputs) - 1 and off[nt["last"]] + 4 == c.batch.n_tuples
        assert c.shapes >= set(SHAPES)
    else:
        assert len(c.shapes) == len([k for k in nt if isinstance(k, tuple)]) <= 2
    by_rule = decided_by(c, (0, 0), "the rule of the one walk")
    by_lim = decided_by(c, ("doc", 1), "lim's role policy")
    for (na, nr), at in [(k, v) for k, v in nt.items() if isinstance(k, tuple)]:
        top, bit0 = c.inputs[at["top"]], c.inputs[at["bit0"]]
        assert (len(top["actions"]), len(top["principal"]["roles"])) == (na, nr) and top["actions"][-1] == "hit" and top["principal"]["roles"][-1] == "key"
        assert at["top"] in by_rule and at["bit0"] in by_rule and answer(c, at["top"], "hit")[0] == answer(c, at["bit0"], "hit")[0] == "ALLOW"
        assert [answer(c, at["top"], a)[0] for a in top["actions"]] == ["DENY"] * (na - 1) + ["ALLOW"] and bit0["actions"][0] == "hit" and bit0["principal"]["roles"][0] == "key"
        i = at["deny_last"]
        assert i in by_lim and [answer(c, i, a) for a in c.inputs[i]["actions"]] == [("DENY", "role.lim.vdefault")] * (na - 1) + [("ALLOW", "resource.doc.vdefault")]
        a, b = at["deny_both"]
        assert answer(c, a, "n0") == ("DENY", "role.lim.vdefault") and answer(c, b, "n0") == ("DENY", "role.lim2.vdefault") and answer(c, a, "ok2")[0] == answer(c, b, "ok2")[0] == "ALLOW"
        a, b = at["trail"]       # the first allowing role is the first / the last: the walks of the roles behind it are not the reference's
        assert (c.want[False][a]["effectivePolicies"], c.want[False][b]["effectivePolicies"]) == (["resource.doc.vdefault"], ["resource.doc.vdefault", "role.lim.vdefault"])
        assert all(e["effect"] == "EFFECT_ALLOW" for i in (a, b) for e in c.want[False][i]["actions"].values())


SHAPE_CASES = dict([("shape_%dx%d" % s, ([s],)) for s in SHAPES] + [("shape_all", (SHAPES,)), ("shape_8x4_16x4", ([(8, 4), (16, 4)],)), ("shape_8x4_8x8", ([(8, 4), (8, 8)],)), ("shape_tiny", ([(2, 2)], True))])


# ---- 5. parent roles


N_ANC = 57      # anc00 .. anc56 take the role classes 0 .. 56, the five kids 57 .. 61: all 62 there are


def parents_docs():
    """Rule j allows act<j> to anc<j> alone.  anc00 .. anc19 each have the next as their parent: anc00 has a chain of 20 ancestors.  kid1
    has one parent (anc56: class 56, the mask's high dword), kid3 three (anc31 .. anc33: both dwords), kid4 four, kid30 thirty (anc27 ..
    anc56); far's parent anc50 is defined at scope `far` only.  Every role policy allows every action."""
    docs = [_policy("doc", "", [_rule(["act%02d" % j], "ALLOW", roles=["anc%02d" % j]) for j in range(N_ANC)])]
    docs += [role_policy("anc%02d" % j, [allows(["*"])], parents=["anc%02d" % (j + 1)]) for j in range(20)]
    kids = {"kid1": [56], "kid3": [31, 32, 33], "kid4": [40, 41, 42, 43], "kid30": list(range(27, 57))}
    docs += [role_policy(k, [allows(["*"])], parents=["anc%02d" % j for j in p]) for k, p in kids.items()]
    docs.append(role_policy("far", [allows(["*"])], scope="far", parents=["anc50"]))
    return docs, kids


def parents_case(name):
    docs, kids = parents_docs()

    def make(c):
        q, nt = Reqs(700), {}
        acts = lambda js: ["act%02d" % j for j in js]
        for k, p in kids.items():
            nt[k] = q.add([k], acts(dict.fromkeys([p[0], p[-1], p[0] - 1, (p[-1] + 1) % N_ANC])))       # the first and the last parent's; their neighbours'
        nt["kid30_all"] = [q.add(["kid30"], acts(range(27 + 8 * g, 35 + 8 * g))) for g in range(3)] + [q.add(["x0", "kid30"], acts(range(41, 57)))]
        nt["chain"] = [q.add(["anc00"], acts([0, 1, 10, 19, 20, 21, 22])), q.add(["anc05"], acts([4, 5, 20, 21])), q.add(["anc20"], acts([19, 20, 21]))]
        nt["far"] = [q.add(["far"], acts([50, 49]), scope=s) for s in ("", "far", "far.er", "zz")]
        for k in range(5, 9):
            q.add(["x%d" % j for j in range(k - 2)] + ["kid3", "kid1"], acts([31, 33, 56, 2]))
        pool = list(kids) + ["far", "anc00", "anc10", "anc19", "anc20", "anc40", "anc56", "x0"]
        while len(q.out) < 151:
            q.add(q.some(pool, most=4), acts(q.rng.choice(N_ANC, size=int(q.rng.integers(1, 9)), replace=False)), scope=q.pick(["", "", "far", "far.er", "zz"]))
        return q.done(151), nt
    return Case(name, docs, make)


def check_parents(c):
    nt, lt = c.notes, c.lt
    cls = section(lt, B.SEC_ROLE_CLASS, np.uint8)[1]
    assert [int(cls[lt.string_ids["anc%02d" % j]]) for j in range(N_ANC)] == list(range(N_ANC)), "anc<j> is not role class j"
    assert sorted(int(cls[lt.string_ids[k]]) for k in ("kid1", "kid3", "kid4", "kid30", "far")) == list(range(57, 62)), "the 62 role classes are not all taken"
    par = {(lt.scopes[e[0]], lt.strings[e[1]]): (e[4], e[5] | e[6] << 32) for e in directory(lt, B.B_PARENTS)}       # (scope, role) -> ancestors, the OR of their classes
    want = {"kid1": 1, "kid3": 3, "kid4": 4, "kid30": 30, "anc00": 20}
    assert {k: par[("", k)][0] for k in want} == want, {k: par[("", k)][0] for k in want}
    assert par[("", "kid30")][1] == sum(1 << j for j in range(27, 57)) and par[("", "anc00")][1] == sum(1 << j for j in range(1, 21)) and par[("", "kid1")][1] == 1 << 56
    assert ("far", "far") in par and ("", "far") not in par
    for k, p in (("kid1", [56]), ("kid3", [31, 32, 33]), ("kid4", [40, 41, 42, 43]), ("kid30", list(range(27, 57)))):
        i = nt[k]
        assert [answer(c, i, a)[0] for a in c.inputs[i]["actions"]] == ["ALLOW" if int(a[3:]) in p else "DENY" for a in c.inputs[i]["actions"]], (k, c.want[False][i])
        assert i in decided_by(c, (0, p[-1]), "the rule of %s's last parent" % k)
    assert all(e["effect"] == "EFFECT_ALLOW" for i in nt["kid30_all"] for e in c.want[False][i]["actions"].values())
    i = nt["chain"][0]
    assert [answer(c, i, a)[0] for a in c.inputs[i]["actions"]] == ["ALLOW"] * 5 + ["DENY"] * 2 and i in decided_by(c, (0, 20), "the rule of the 20th ancestor of a chain")
    for lenient in (False, True):     # parents count at the request's own scope only: not one level down either, whichever the scope search
        assert [answer(c, i, "act50", lenient)[0] for i in nt["far"]] == ["DENY", "ALLOW", "DENY", "DENY"], (lenient, [c.want[lenient][i] for i in nt["far"]])


# ---- 6. principal policies


N_PRINCIPALS = 70


def principals_docs():
    """u00 .. u69, every fifth without a policy; u<i>'s policy decides the one action a<i % 8> (odd i: ALLOW, even: DENY) - u07's
    under a condition that is an evaluation site; the resource policy allows everything to r0"""
    docs = [_policy("doc", "", [_rule(["*"], "ALLOW", roles=["r0"])])]
    for i in range(N_PRINCIPALS):
        if i % 5 != 4:
            act = {"action": A8[i % 8], "effect": "EFFECT_ALLOW" if i % 2 else "EFFECT_DENY"}
            if i == 7:
                act["condition"] = pick_cond(7)
            docs.append(principal_policy("u%02d" % i, [{"resource": "doc", "actions": [act]}]))
    return docs


def principals_case(name):
    def make(c):
        q, nt = Reqs(800), {}
        for i in range(163):        # lane i of the first wave: principal i; the principals 64 .. 69 stand in the second wave
            u = i % N_PRINCIPALS
            q.add(["r0"] if (i // N_PRINCIPALS) != 1 else ["x0"], [A8[u % 8], A8[(u + 1) % 8]], pid="u%02d" % u, picks=[[7], [8], None][(i // N_PRINCIPALS) % 3], bump=0)
        nt["site"] = [7, 7 + N_PRINCIPALS, 7 + 2 * N_PRINCIPALS]
        return q.done(163), nt
    return Case(name, principals_docs(), make, lenient=(False,))


def check_principals(c):
    nt, lt = c.notes, c.lt
    have = {lt.strings[e[2]] for e in directory(lt, B.B_PRINCIPAL)} - {""}      # (the empty principal's bucket is every policy's rows)
    assert have == {"u%02d" % i for i in range(N_PRINCIPALS) if i % 5 != 4}, "one directory entry per principal with a policy"
    assert len({i["principal"]["id"] for i in c.inputs[:64]}) == 64 and {i["principal"]["id"] for i in c.inputs[64:70]} == {"u%02d" % i for i in range(64, 70)}
    docs = {doc["principalPolicy"]["principal"]: d for d, doc in enumerate(c.docs) if "principalPolicy" in doc}
    for i in (0, 1, 62, 63, 65, 66, 68):
        u = "u%02d" % i
        assert i in decided_by(c, ("doc", docs[u]), "the policy of the principal in lane %d" % (i % 64)), u
        assert answer(c, i, A8[i % 8]) == ("ALLOW" if i % 2 else "DENY", "principal.%s.vdefault" % u) and answer(c, i, A8[(i + 1) % 8]) == ("ALLOW", "resource.doc.vdefault")
    assert answer(c, 64, "a0") == ("ALLOW", "resource.doc.vdefault") and answer(c, 64 + N_PRINCIPALS, "a0")[0] == "DENY"
    assert [(answer(c, i, "a7")[0], errors(c, i)) for i in nt["site"]] == [("ALLOW", False), ("DENY", False), ("ALLOW", True)], [c.want[False][i] for i in nt["site"]]
    assert nt["site"][0] in decided_by(c, ("doc", docs["u07"]), "the principal policy whose rule's condition is a site") and lt.stats["gslots"] == (1, 1)


# ---- 7. derived roles


def derived_docs():
    """64 derived roles, each named by a rule (the table keeps no other): d<i> is active for role r<i % 4> where R.attr.n is "<i>".  The rule of a7 names forty roles first, so that
    the definitions' parent roles take the classes 40 .. 43, and `elder`'s parent role f35 class 35: the mask's high dword."""
    defs = [{"name": "d%02d" % i, "parentRoles": ["r%d" % (i % 4)], "condition": expr('R.attr.n == "%d"' % i)} for i in range(64)]
    drs = [derived_roles("dr_a", defs[:32]), derived_roles("dr_b", defs[32:63] + [{"name": "elder", "parentRoles": ["f35"], "condition": expr('R.attr.n == "35"')}])]
    rules = [_rule(["a7"], "ALLOW", roles=["f%02d" % j for j in range(40)]), _rule(["a0"], "ALLOW", derived=["d%02d" % i for i in range(63)]),
             _rule(["a1"], "ALLOW", derived=["elder"]), _rule(["a0"], "DENY", derived=["d62"], cond=expr("R.attr.flag == true")), _rule(["a2"], "ALLOW", roles=["r0", "r1", "r2", "r3"])]
    return drs + [_policy("doc", "", rules, imports=["dr_a", "dr_b"])]


def derived_case(name):
    def make(c):
        q, nt = Reqs(900), {}
        nt["bits"] = {i: q.add(["r%d" % (i % 4)], ["a0", "a2"], n=str(i), flag=False) for i in (0, 31, 32, 62)}
        nt["wrong_role"] = q.add(["r1"], ["a0", "a2"], n="0", flag=False)
        nt["elder"] = [q.add(["f35"], ["a1", "a7"], n="35"), q.add(["f34"], ["a1", "a7"], n="35"), q.add(["f35"], ["a1", "a7"], n="34")]
        nt["deny"] = q.add(["r2"], ["a0"], n="62", flag=True)
        q.add(["r0", "r1", "r2", "r3"], ["a0", "a1", "a2"], n="32")
        q.add(["r2"], ["a0"], n="62")                                 # the DENY's condition fails: an evaluation error
        while len(q.out) < 139:
            q.add(q.some(["r0", "r1", "r2", "r3", "f35", "f00", "x0"], most=4), q.some(["a0", "a1", "a2", "a7"], most=4), n=str(int(q.rng.integers(0, 66))), flag=q.pick([True, False, None]))
        return q.done(139), nt
    return Case(name, derived_docs(), make, lenient=(False,))


def check_derived(c):
    nt, lt = c.notes, c.lt
    drx = section(lt, B.SEC_DRX)[1].reshape(-1, 16)
    assert sorted(int(d[4]) for d in drx) == list(range(64)) and len(lt.dr_names) == 64, "64 names, one bit of the mask each"
    bit = {lt.dr_names[int(d[4])]: int(d[4]) for d in drx}
    for i in (0, 31, 32, 63):
        name = lt.dr_names[i]
        req = [k for k, w in enumerate(c.want[False]) if name in w["effectiveDerivedRoles"]]
        assert req, "no request activates bit %d of the mask (%s)" % (i, name)
    cls = section(lt, B.SEC_ROLE_CLASS, np.uint8)[1]
    assert int(cls[lt.string_ids["f35"]]) == 35 and sorted(int(cls[lt.string_ids["r%d" % k]]) for k in range(4)) == [40, 41, 42, 43]
    (elder,) = [d for d in drx if int(d[4]) == bit["elder"]]
    assert (int(elder[0]), int(elder[1])) == (0, 1 << 3), "elder's parent roles are not in the class mask's high dword"
    for i, at in nt["bits"].items():
        assert c.want[False][at]["effectiveDerivedRoles"] == ["d%02d" % i] and answer(c, at, "a0")[0] == "ALLOW"
        assert at in decided_by(c, (0 if i < 32 else 1, i % 32), "the definition of d%02d" % i)
    assert not c.want[False][nt["wrong_role"]]["effectiveDerivedRoles"] and answer(c, nt["wrong_role"], "a0")[0] == "DENY"
    assert [(answer(c, i, "a1")[0], c.want[False][i]["effectiveDerivedRoles"]) for i in nt["elder"]] == [("ALLOW", ["elder"]), ("DENY", []), ("DENY", [])]
    assert nt["elder"][0] in decided_by(c, (1, 31), "the definition whose parent role has class 35")
    assert answer(c, nt["deny"], "a0")[0] == "DENY" and any(errors(c, i) for i in range(len(c.inputs)))


MORE_CASES = {"parents": (parents_case, check_parents), "principals": (principals_case, check_principals), "derived": (derived_case, check_derived)}


# ---- the cases


FAMILIES = [(GLOB_CASES, glob_case, check_globs), (ROLEPOL_CASES, rolepol_case, check_rolepol), (SITE_CASES, site_case, check_sites), (SPLIT_CASES, split_case, check_split),
            ({"sites_mixed": ()}, mixed_case, check_mixed), (SHAPE_CASES, shape_case, check_shapes)] + [({k: ()}, make, check) for k, (make, check) in MORE_CASES.items()]
BUILD = {name: (make, args, check) for cases, make, check in FAMILIES for name, args in cases.items()}
CASES = list(BUILD)
REFUSED = [name for name, (_m, args, _c) in BUILD.items() if args and isinstance(args[-1], str)]
WITH_SITES = list(SITE_CASES) + list(SPLIT_CASES) + ["sites_mixed", "rolepol_32", "principals", "derived"]          # (derived: open sites only, none filed for its batch)
WITH_ROLE_POLICIES = list(ROLEPOL_CASES) + ["globs_a16", "globs_1025", "shape_8x4", "shape_8x8", "shape_16x4", "shape_all", "parents", "sites_mixed"]
NO_GENERAL_WALK = ["sites_mixed"]       # (a table with policy variables: the general walk leaves a failing variable to the trace pass, CBH_MF_TRACE_ALL)
_CASES = {}


def case(name):
    """the named cases, built once"""
    if name not in _CASES:
        make, args, _check = BUILD[name]
        _CASES[name] = make(name, *args)
    return _CASES[name]


# ---- the roads.  The emulator: the kernels' source on the wave emulator; asserts hostsim_last_kind / _walk_wide / _pre_split


def wide_bits(c):
    """which of the wider walks a batch of these shapes launches (cbh_plan: by the batch's maxima)"""
    if c.kind != 2:
        return 0
    return (1 if max(r for _a, r in c.shapes) > 4 else 0) | (2 if max(a for a, _r in c.shapes) > 8 else 0)


def sites_filed(c):
    """how many evaluation sites a launch files results for: none off the walk, the generic ones for a batch of plain scalars, else all"""
    brings = any(isinstance(v, list) or (isinstance(v, int) and not isinstance(v, bool)) for i in c.inputs for v in i["resource"]["attr"].values())
    return 0 if c.kind != 2 else c.lt.stats["gslots"][1 if brings else 0]


def trail_matches(c, masks, lenient, what):
    have = [effective_policy_keys(c.lt.policy_keys, row) for row in masks]
    want = [w["effectivePolicies"] for w in c.want[lenient]]
    bad = [k for k in range(len(want)) if have[k] != want[k]]
    assert not bad, (c.name, what, lenient, bad[:3], have[bad[0]], want[bad[0]], c.inputs[bad[0]])
    assert len({tuple(k) for k in have}) >= 2


def check_on_emulator(c, monkeypatch, general=False, trail=False, pre_split=None):
    import hostsim_api
    if general:
        monkeypatch.setenv("CBH_NO_WALK2", "1")
    if pre_split is not None:
        monkeypatch.setenv("CBH_PRE_SPLIT", "1" if pre_split else "0")
    for lenient in c.lenient:
        flags = F_WANT_DR | (F_LENIENT if lenient else 0)
        res = hostsim_api.check(c.lt, c.batch, NOW, flags)
        assert hostsim_api.last_kind() == (0 if general else c.kind), (c.name, hostsim_api.last_kind())
        if not general:
            assert hostsim_api.last_walk_wide() == wide_bits(c), (c.name, hostsim_api.last_walk_wide(), sorted(c.shapes))
        if pre_split is not None and not general:
            assert hostsim_api.last_pre_split() == (pre_split and sites_filed(c) > 0), (c.name, "the pre-pass's form")
        ts.compare(c, res, lenient, "general walk" if general else "walk2")
        if trail:
            groups = np.arange(c.batch.n_requests, dtype=np.uint32)
            res, m = hostsim_api.check_trail(c.lt, c.batch, groups, c.batch.n_requests, NOW, flags)
            assert hostsim_api.last_kind() == (0 if general else c.kind), (c.name, "trail")
            ts.compare(c, res, lenient, "trail")
            trail_matches(c, m, lenient, "trail")


# ---- the library: cbh_check_batch, the resident path, the trail; asserts the plan's text


def plan_ok(c, plan, trail=False):
    """the kernels of the plan, in cbh_plan_describe's order: the general walk's share, the wider walks, the pre-pass in the process's
    form, the walk"""
    if c.kind != 2:
        return plan == ("cbh_check_trail_kernel" if trail else "cbh_check_kernel*")
    t = "_trail" if trail else ""
    na, nr = max(a for a, _r in c.shapes), max(r for _a, r in c.shapes)       # (cbh_plan goes by the batch's maxima, as wide_bits does)
    assert any(w2_class(a, r) == 3 for a, r in c.shapes) <= (w2_class(na, nr) == 3)
    want = "cbh_check_kernel*(wide requests)+" if w2_class(na, nr) == 3 else ""
    want += "cbh_walk2_wide%s_kernel(5-8 roles)+" % t if wide_bits(c) & 1 else ""
    want += "cbh_walk2_awide%s_kernel(9-16 actions)+" % t if wide_bits(c) & 2 else ""
    if sites_filed(c):
        want += "cbh_walk2_pre_kernel+" if os.environ.get("CBH_PRE_SPLIT") == "0" else "cbh_walk2_collect_kernel+cbh_walk2_interp_kernel+"
    return plan == want + "cbh_walk2%s_kernel" % t


def check_decisions(capi, name):
    """one-shot and resident (upload / launch / download), each against the oracle"""
    ts._flags(capi)
    c = case(name)
    table = capi.Table(c.lt.blob)         # (sites_257: the image the loader used to refuse)
    db = table.upload(c.batch)
    try:
        for lenient in c.lenient:
            flags = F_WANT_DR | (F_LENIENT if lenient else 0)
            ts.compare(c, table.check(c.batch, now_ns=NOW, flags=flags), lenient, "cbh_check_batch")
            table.launch(db, now_ns=NOW, flags=flags)
            ts.compare(c, table.download(db), lenient, "resident")
        plan = table.plan(db, flags=F_WANT_DR)
        assert plan_ok(c, plan), (name, plan, sorted(c.shapes)[-3:], sites_filed(c))
    finally:
        db.close()
        table.close()


def check_trail(capi, name):
    """cbh_check_batch_trail and the resident trail, one group per request"""
    ts._flags(capi)
    c = case(name)
    table = capi.Table(c.lt.blob)
    db = table.upload(c.batch)
    groups = np.arange(c.batch.n_requests, dtype=np.uint32)
    try:
        plan = table.plan(db, flags=F_WANT_DR | F_WANT_EP)
        assert plan_ok(c, plan, trail=True), (name, plan)
        for lenient in c.lenient:
            flags = F_WANT_DR | (F_LENIENT if lenient else 0)
            res, masks = table.check_trail(c.batch, groups, c.batch.n_requests, now_ns=NOW, flags=flags)
            ts.compare(c, res, lenient, "cbh_check_batch_trail")
            trail_matches(c, masks, lenient, "cbh_check_batch_trail")
            table.set_trail(db, groups, c.batch.n_requests)
            table.launch(db, now_ns=NOW, flags=flags | F_WANT_EP)
            trail_matches(c, table.trail(db), lenient, "resident trail")
            ts.compare(c, table.download(db), lenient, "resident trail")
    finally:
        db.close()
        table.close()


FORMS = [(check_decisions, (name,)) for name in WITH_SITES if name != "derived"] + [(check_trail, ("rolepol_32",)), (check_trail, ("sites_mixed",))]
LIBRARY = {   # road -> (environment, [(body, arguments)])
    "default": ({}, [(check_decisions, (name,)) for name in CASES if name != "shape_tiny"] + [(check_trail, (name,)) for name in WITH_ROLE_POLICIES]),
    "pre_split_0": ({"CBH_PRE_SPLIT": "0"}, FORMS),
    "pre_split_1": ({"CBH_PRE_SPLIT": "1"}, FORMS),
    "four_waves": ({}, [(check_decisions, (name,)) for name in ("globs_1024", "globs_1025", "rolepol_32_two", "sites_256", "sites_16_all", "split_15_2_ints", "shape_all", "parents",
                                                                "principals", "derived")] + [(check_trail, ("rolepol_32_two",)), (check_trail, ("shape_all",))]),
}
DEFAULT_IDS = ["%s-%s" % (b.__name__, a[0]) for b, a in LIBRARY["default"][1]]


def run_road(capi, road, only=None):
    for k, (body, args) in enumerate(LIBRARY[road][1]):
        if only is None or k in only:
            body(capi, *args)


def check_in_child(sim, road, lib=None, limit=600):
    ts.check_in_child(sim, road, lib=lib, limit=limit, module="test_walk2_limits", library=LIBRARY)


# ---- CPU tier: the conditions the stores must meet (no kernel runs)


@pytest.mark.parametrize("name", CASES)
def test_the_named_positions_decide(name):
    c = case(name)
    BUILD[name][2](c)
    assert (c.kind == 0) == (name in REFUSED)
    if name != "shape_tiny":
        assert any(e["effect"] == "EFFECT_ALLOW" for w in c.want[False] for e in w["actions"].values()) and any(e["effect"] == "EFFECT_DENY" for w in c.want[False] for e in w["actions"].values())


def test_the_refusals_name_their_limit():
    """17 patterns, 33 role policies, 257 sites: the lowering says which limit keeps the table off the walk - and nothing else does"""
    assert {name: [r for r in case(name).lt.stats["walk2_refused"] if "more than" in r] for name in REFUSED} == {
        "globs_a17": ["more than 16 glob patterns in a dimension"], "globs_r17": ["more than 16 glob patterns in a dimension"],
        "rolepol_33": ["more than 32 role policies in one scope"], "sites_257": ["more than 256 evaluation sites on one request's path"]}
    assert case("sites_257").lt.stats["gslots"] == (257, 257) and case("rolepol_33").lt.stats["walk2_refused"] == ["more than 32 role policies in one scope"]


# ---- CPU tier: the wave emulator


@pytest.mark.parametrize("name", CASES)
def test_walk2_on_emulator(name, monkeypatch):
    check_on_emulator(case(name), monkeypatch, trail=name in WITH_ROLE_POLICIES)


@pytest.mark.parametrize("name", [n for n in CASES if n not in NO_GENERAL_WALK])
def test_general_walk_on_emulator(name, monkeypatch):
    check_on_emulator(case(name), monkeypatch, general=True)


@pytest.mark.parametrize("split", [False, True], ids=["fused", "collector"])
@pytest.mark.parametrize("name", WITH_SITES)
def test_both_forms_of_the_pre_pass_on_emulator(name, split, monkeypatch):
    check_on_emulator(case(name), monkeypatch, pre_split=split, trail=name in WITH_ROLE_POLICIES)


@pytest.mark.parametrize("name", list(SPLIT_CASES) + ["sites_15", "sites_16", "sites_17", "sites_255", "sites_256", "derived"])
def test_words_of_site_results_on_emulator(name, monkeypatch, capfd):
    """16 slots to a 64-bit word; a batch of plain scalars files the generic sites only (16 + 1 and 15 + 2: one word, not two)"""
    import hostsim_api
    c = case(name)
    monkeypatch.setenv("CBH_HOSTSIM_REPORT", "1")
    capfd.readouterr()
    ts.compare(c, hostsim_api.check(c.lt, c.batch, NOW, F_WANT_DR), False, "walk2")
    assert "hostsim: kernel kind 2, %d result words\n" % ((sites_filed(c) + 15) // 16) in capfd.readouterr().err
    if name in SPLIT_CASES:
        assert (sites_filed(c) + 15) // 16 == c.words == (2 if c.ints else 1)


# ---- CPU tier: the library's host side on the simulator


@pytest.fixture()
def engine():
    from sim_engine import sim_engine
    with sim_engine() as capi:
        yield capi


@pytest.mark.parametrize("k", range(len(DEFAULT_IDS)), ids=DEFAULT_IDS)
def test_as_planned_on_simulator(engine, k):
    assert "CBH_PRE_SPLIT" not in os.environ
    run_road(engine, "default", only=(k,))


def test_fewer_than_four_tuples_on_simulator(engine):
    check_decisions(engine, "shape_tiny")


@pytest.mark.parametrize("road", ["pre_split_0", "pre_split_1"])
def test_both_forms_of_the_pre_pass_on_simulator(road):
    check_in_child(True, road)


def test_four_waves_to_a_workgroup():
    from sim_engine import build_four_waves
    check_in_child(True, "four_waves", lib=build_four_waves())


# ---- GPU tier


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(DEFAULT_IDS)), ids=DEFAULT_IDS)
def test_as_planned_on_gpu(k):
    from cerbos_amd import capi
    assert "CBH_PRE_SPLIT" not in os.environ
    run_road(capi, "default", only=(k,))


@pytest.mark.gpu
def test_fewer_than_four_tuples_on_gpu():
    from cerbos_amd import capi
    check_decisions(capi, "shape_tiny")


@pytest.mark.gpu
@pytest.mark.parametrize("road", ["pre_split_0", "pre_split_1"])
def test_both_forms_of_the_pre_pass_on_gpu(road):
    # a fresh child process for each form (the library reads the switch once); on the simulator the same child takes about ten seconds,
    # most of it building the cases
    check_in_child(os.environ.get("CBH_TEST_SIM_ENGINE") == "1", road, limit=180)
