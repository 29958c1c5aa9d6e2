"""Glob, `matches` and the string functions at the sizes their code has built in.

Every string comparison on the device that is not a comparison of ids runs byte by byte through hand-written code, and that code
has fixed sizes.  Restated here, from the headers, and used to BUILD the inputs - the set of flagged requests follows from these
numbers alone, never from what the code answers:
  WINDOW_MAX = 0x7FFE   cbh_vm.h CBH_ROPE_WINDOW_MAX.  A window of a string (substring / charAt / trim, the pieces replace() and split()
                        keep) is 15 bits of first byte and 15 bits of length + 1 (rope_window, part_span): first byte <= 0x7FFE and
                        length <= 0x7FFE bytes, or the tuple is CBH_ST_UNSUPPORTED; replace() and split() take strings of at most
                        0x7FFE bytes (every piece must be a window)
  ARENA = 48            cbh_blob.h CBH_ARENA_ENTRIES, values per lane.  replace(): the replacement takes one entry per hit, the bytes
                        before a hit (if any) one more; the loop wants room for two before every hit and for one after the last.
                        split(): two entries per piece
  16-bit lengths        a batch the device flattened keeps (offset, length & 0xFFFF) per string in str_keys (str_span, the glob kernel):
                        65 535 bytes is the longest string of the device road
  512 positions         8 state words per glob dimension (lower/globs.py GlobNFA.MAX_WORDS, cbh_kernels.h NFA_MAXW); position 511 can
                        only be an accept position (a star or a byte element needs the position after it)
  1024 states           per `matches` automaton (lower/regex.py), 8-bit byte classes
  star runs             lower/globs.py collapses adjacent star elements (a run with a `**` is one `**`, a run of `*` one `*`), so that
                        the kernel's closure loop - at most 8 rounds, one star position per round - is complete after one

What was found.  Without the collapse, a pattern with nine or more consecutive star positions was decided differently for strings
of the table (bits from GlobNFA._closure, a fixpoint) and strings only the request brings (bits from the kernel's eight rounds):
`a*****************b` DENIED the action `ab`, status OK.  test_star_runs_* fail on the parent with exactly that difference.

The references are oracle/check.py with oracle/globmatch.glob_match for globs and oracle/celeval._re for `matches`, per action,
exactly.  Never GlobNFA.match_bits or regex.compile_regex(...).search: those share the device's design.

Tiers.  *_on_simulator: the library built against the simulator (tests/sim_engine.py) - the ONLY CPU tier on which the glob kernel's
own source runs.  *_on_emulator: the decision kernels on the wave emulator (HostSimEvaluator's road, tests/hostsim_api.py); its glob
bits come from the host's GlobNFA.match_bits, so it cannot see a difference between kernel and lowering - it checks the lowering,
the interpreter and the byte loops.  *_on_gpu: the same bodies on the device (CBH_TEST_SIM_ENGINE=1: on the simulator).
Roads, on the library: the dict road (Flattener -> cbh_check_batch), the device road in steps (cbh_wire_flatten -> cbh_check_resident
-> download; lengths from str_keys) and in one call (cbh_wire_check_pb: effects and CBI_OUT_* flags of the serialized outputs).
Every road asserts the kernel family it ran (the plan's text, hostsim_last_kind) and, for globs, that the automaton has words and
the subjects are NOT strings of the table (such a string gets its bits at lowering time, the kernel never sees it); the subjects
listed in TABLE_SIDE are in the table on purpose.

Per layer: the oracle decides every request, without an evaluation error except the intended ones (substring / charAt beyond the end
of the string: CBH_ST_CEL_ERROR there and nowhere else); per condition and length class the decided requests hold an ALLOW and a DENY;
exactly the (request, action) pairs built to exceed a limit come back CBH_ST_UNSUPPORTED.

Mutation check (each mutant on a scratch copy, CPU tier, never committed).  "older" = the CPU tier of test_glob_syntax, test_regex,
test_string_functions, test_string_views_network, test_hierarchy, test_capacity_limits and test_math_bind_split (17 tests).
   1  closure cap 8 -> 1                  passes after the collapse, and must: no star position follows another, so the first round
                                          completes the closure (the invariant GlobNFA asserts) - an equivalent mutant now.  On the
                                          parent's lowering it fails test_star_runs_on_simulator (`ab` against the seventeen asterisks:
                                          DENY where ALLOW is wanted), as the unmutated parent does.  The cap 8 -> 0 (no closure at all)
                                          is killed: test_star_runs_on_simulator, test_word_boundaries_on_simulator[words_a | words_b |
                                          words_c], test_on_simulator[long_subjects].  older: all pass, either way
   2  carry = adv >> 63 -> 0              killed: test_star_runs_on_simulator (the store's automaton has more than one word),
                                          test_word_boundaries_on_simulator[words_a | words_b | words_c].  older: all pass
   3  the closure's c2 dropped            killed: test_star_runs_on_simulator, test_word_boundaries_on_simulator[words_a] (the star on
                                          bit 63).  older: all pass
   4  flags[s] & 2u ignored               killed: test_on_emulator / test_on_simulator[matches | random_patterns].  older:
                                          test_regex.py::test_matches_kernel_source_vs_oracle fails too
   5  the flags & 1 early exit removed    passes, as it must (the control: the exit saves time, the answer is the same).  older: all pass
   6  part_span's length mask 0x3FFF      killed: test_on_emulator / test_on_simulator[windows].  older: all pass
   7  > CBH_ROPE_WINDOW_MAX -> >=         killed: test_on_emulator / test_on_simulator[windows] (charAt and substring with a first byte
      (substring / charAt / trim)         or a length of exactly 0x7FFE come back flagged).  older: all pass
   8  str_span's & 0xFFFF -> & 0x7FFF     killed on the device road only, as it must be: test_on_simulator[matches | windows |
                                          byte_loops] at "device road, cbh_check_resident".  older: all pass
   9  ap + 2 > CBH_ARENA_ENTRIES -> + 3   killed: test_on_emulator / test_on_simulator[arena].  older: all pass
"""
import os

import numpy as np
import pytest

from cerbos_amd import wire
from cerbos_amd.flatten import Flattener
from cerbos_amd.lower.blob import lower_rule_table
from cerbos_amd.policy.loader import policies_from_docs
from cerbos_amd.ruletable.build import rule_table_from_policies
from oracle import celeval
from oracle.check import EvalParams, RuleTableOracle
from oracle.globmatch import glob_match

API = "api.cerbos.dev/v1"
NOW = 1_700_000_000_000_000_000
WINDOW_MAX = 0x7FFE
ARENA = 48
MAX_DEVICE_STRING = 0xFFFF
GLOB_POSITIONS = 512
REGEX_STATES = 1024
EFFECT_ALLOW, ST_CEL_ERROR, ST_UNSUPPORTED = 1, 1, 2     # cerbos_amd/capi.py, asserted in _constants()
F_WANT_DR = 4
OUT_UNSUPPORTED = 1                                      # include/cerbos_ingest.h CBI_OUT_UNSUPPORTED


def _constants(capi):
    assert (capi.EFFECT_ALLOW, capi.ST_CEL_ERROR, capi.ST_UNSUPPORTED, capi.F_WANT_DERIVED_ROLES) == (EFFECT_ALLOW, ST_CEL_ERROR, ST_UNSUPPORTED, F_WANT_DR)


def header_value(name, header):
    """the number a header defines for `name` (the restated limits are compared with the source, not assumed)"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "cerbos_amd", "csrc", header)) as fh:
        m = re.search(r"#define\s+%s\s+(0x[0-9A-Fa-f]+|\d+)u?\b" % name, fh.read())
    return int(m.group(1), 0)


def _interprets(plan):
    """the kernels with the operand-stack interpreter: the general walk, or walk2 with its interpreter pass"""
    return plan.startswith("cbh_check_kernel") or "cbh_walk2_interp_kernel" in plan


# ---- a layer: one store, its requests, the oracle's answers - computed once, shared by every road, never changed


def cond_store(kind, conds):
    return [{"apiVersion": API, "resourcePolicy": {"resource": kind, "version": "default", "rules": [
        {"actions": [n], "roles": ["*"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": e}}} for n, e in conds.items()]}}]


def request(rid, kind, actions, roles=("user",), pattr=None, rattr=None):
    return {"requestId": rid, "actions": list(actions), "principal": {"id": "p", "roles": list(roles), "attr": dict(pattr or {})},
            "resource": {"kind": kind, "id": "r", "attr": dict(rattr or {})}}


class Layer:
    """over: the (request id, action) pairs built to exceed a limit - they, and nothing else, come back CBH_ST_UNSUPPORTED;
    groups: {label: [(request id, action)]} - the decided pairs of every label hold an ALLOW and a DENY;
    loud: the store has a pattern the lowering had to flag (every request equals the oracle or is flagged, no exact set);
    kinds: the hostsim_last_kind values the emulator may report; plan_ok: the plan's text on the library"""

    def __init__(self, name, docs, inputs, over=(), groups=None, loud=False, kinds=(0, 2), plan_ok=None, refused=0, errors=()):
        self.name, self.inputs, self.over, self.groups, self.loud, self.kinds = name, inputs, set(over), groups or {}, loud, kinds
        self.errors = set(errors)      # the (request id, action) pairs whose condition fails to evaluate, on purpose
        self.plan_ok = plan_ok or _interprets
        self.rt = rule_table_from_policies(policies_from_docs(docs))
        self.lt = lower_rule_table(self.rt)
        assert len(self.lt.unsupported) == refused or loud, (name, self.lt.unsupported)
        assert len({i["requestId"] for i in inputs}) == len(inputs)
        orc = RuleTableOracle(self.rt)
        self.want = [orc.check(i, EvalParams(now_ns=NOW)) for i in inputs]
        self.batch = Flattener(self.lt).flatten(inputs, sort=False)
        assert self.batch.n_requests == len(inputs)
        self.data, self.off = wire.pack_messages([wire.encode_check_input(i) for i in inputs])
        self.string_bytes = sum(len(v.encode()) for i in inputs for part in (i["principal"]["attr"], i["resource"]["attr"]) for v in part.values() if isinstance(v, str)) + \
            sum(len(a.encode()) for i in inputs for a in i["actions"]) + sum(len(r.encode()) for i in inputs for r in i["principal"]["roles"])

    def allow(self, rid, action):
        k = next(k for k, i in enumerate(self.inputs) if i["requestId"] == rid)
        return self.want[k]["actions"][action]["effect"] == "EFFECT_ALLOW"

    def check_oracle(self):
        """on the CPU: the oracle decides everything, the groups discriminate, the sizes are what the issue asks for"""
        for inp, w in zip(self.inputs, self.want):
            assert bool(w["evaluationErrors"]) == (inp["requestId"] in {r for r, _ in self.errors}), (self.name, inp["requestId"], w["evaluationErrors"])
        ids = {(i["requestId"], a) for i in self.inputs for a in i["actions"]}
        assert self.over <= ids, (self.name, sorted(self.over - ids)[:3])
        index = {i["requestId"]: k for k, i in enumerate(self.inputs)}
        for label, pairs in self.groups.items():
            seen = {self.want[index[r]]["actions"][a]["effect"] for r, a in pairs if (r, a) not in self.over}
            assert seen or self.over, (self.name, label)
            assert not seen or seen == {"EFFECT_ALLOW", "EFFECT_DENY"}, (self.name, label, "the decided requests do not discriminate", seen)
        assert len(self.inputs) <= 700 and self.string_bytes < 12 << 20, (self.name, len(self.inputs), self.string_bytes)


def judge(layer, effect, status, what):
    """per tuple, in input order: flagged exactly where the layer says, equal to the oracle everywhere else"""
    flagged, t = set(), 0
    for inp, w in zip(layer.inputs, layer.want):
        for a in inp["actions"]:
            if int(status[t]) & ST_UNSUPPORTED:
                flagged.add((inp["requestId"], a))
            else:
                want = w["actions"][a]["effect"] == "EFFECT_ALLOW"
                assert (int(effect[t]) == EFFECT_ALLOW) == want, (layer.name, what, inp["requestId"], a[:60], len(a), "ALLOW" if want else "DENY", "is wanted")
                assert bool(int(status[t]) & ST_CEL_ERROR) == ((inp["requestId"], a) in layer.errors), (layer.name, what, inp["requestId"], a[:60], "evaluation error")
            t += 1
    assert t == len(effect)
    if layer.loud:
        assert flagged and t > len(flagged), (layer.name, what, len(flagged), t)
    else:
        assert flagged == layer.over, (layer.name, what, "flagged but not built to be", sorted(flagged - layer.over)[:4], "built to be flagged but decided", sorted(layer.over - flagged)[:4])


def judge_outputs(layer, raw, flags, what):
    """the serialized CheckOutputs of the device road: CBI_OUT_UNSUPPORTED per request, effects of the others"""
    over = {r for r, _ in layer.over}
    assert len(raw) == len(layer.inputs)
    n_flagged = 0
    for inp, w, r, f in zip(layer.inputs, layer.want, raw, flags):
        if int(f) & OUT_UNSUPPORTED:
            n_flagged += 1
            assert layer.loud or inp["requestId"] in over, (layer.name, what, inp["requestId"], "flagged but not built to be")
            continue
        assert layer.loud or inp["requestId"] not in over, (layer.name, what, inp["requestId"], "built to be flagged but decided")
        out = wire.decode_check_output(r)
        for a in inp["actions"]:
            assert out["actions"][a]["effect"] == w["actions"][a]["effect"], (layer.name, what, inp["requestId"], a[:60], len(a))
    assert not layer.loud or 0 < n_flagged < len(raw)


def run_on_emulator(layer):
    import hostsim_api
    res = hostsim_api.check(layer.lt, layer.batch, NOW, F_WANT_DR)
    assert hostsim_api.last_kind() in layer.kinds, (layer.name, hostsim_api.last_kind())
    judge(layer, res.effect, res.status, "emulator")


def run_on_library(capi, layer):
    _constants(capi)
    table = capi.Table(layer.lt.blob)
    try:
        res = table.check(layer.batch, now_ns=NOW, flags=F_WANT_DR)
        judge(layer, res.effect, res.status, "dict road, cbh_check_batch")
        db = table.wire_flatten(layer.data, layer.off)
        try:
            assert db.wire_info["n_host"] == 0, db.wire_info
            table.launch(db, now_ns=NOW, flags=F_WANT_DR)
            res = table.download(db)
            judge(layer, res.effect, res.status, "device road, cbh_check_resident")
            plan = table.plan(db, flags=F_WANT_DR)
            assert layer.plan_ok(plan), (layer.name, plan)    # a test that passes because another kernel decided proves nothing
        finally:
            db.close()
        raw, flags = table.wire_check_pb(layer.data, layer.off, now_ns=NOW, flags=F_WANT_DR)
        judge_outputs(layer, raw, flags, "device road, cbh_wire_check_pb")
    finally:
        table.close()


_LAYERS = {}


def layer(name):
    if name not in _LAYERS:
        _LAYERS[name] = MAKERS[name]()
    return _LAYERS[name]


# ---- 1. the glob automaton


DIM_ACTION, DIM_ROLE = 0, 1
STAR_RUNS = (1, 2, 8, 9, 10, 20)
TABLE_SIDE = "y"        # subjects with this in the star's place are ALSO literal actions of a rule: strings of the table


def star_run(n, form):
    """n consecutive star positions: `all` n times `**`; `one` n - 1 times `**` and a `*`; `single` n times `*` (each in braces of
    its own: two adjacent asterisks would read as `**`)"""
    return {"all": "*" * (2 * n), "one": "*" * (2 * n - 1), "single": "{*}" * n}[form]


def star_patterns():
    """[(pattern, pre, post, x's in the long subject)]: the runs between literals, at the start, at the end"""
    out = []
    for n in STAR_RUNS:
        for form in ("all", "one") + (("single",) if n in (2, 9) else ()):
            run = star_run(n, form)
            for pre, post in (("a", "b"), ("", "b"), ("a", "")):
                out.append((pre + run + post, pre, post, 6 if form == "single" else 30))    # (nine `[^:]*` in a row: the oracle backtracks)
    return out


def star_subjects(pre, post, many=30):
    """the run matches empty, one byte, a separator, many bytes with separators; a table-side string; two that must not match"""
    return [pre + post, pre + "x" + post, pre + ":" + post, pre + "x" * many + ":y:" + "z" * 7 + post, pre + "é日" + post,
            pre + TABLE_SIDE + post, "c" + pre + post + "c", "c" + pre + "x:x" + post + "c"]


def _nine_star_case():
    """the case the issue was opened with, as it was reported"""
    docs = [{"apiVersion": API, "resourcePolicy": {"resource": "issue", "version": "default", "rules": [
        {"actions": ["a" + "*" * 17 + "b"], "roles": ["*"], "effect": "EFFECT_ALLOW"}]}}]
    return docs, [request("issue", "issue", ["ab", "axb", "a:b", "b"])]


def make_star_runs():
    """kind k<i>: pattern i as the rule's action (the subjects are the request's actions); kind r<i>: pattern i as the rule's role
    (the subject is the principal's role); role policies rp<i>: the pattern in allowActions, for the runs of 9 and 20 between
    literals.  One kind per pattern, so that every decision is one pattern's."""
    pats = star_patterns()
    docs, inputs, groups = [], [], {}
    docs0, inputs0 = _nine_star_case()
    docs += docs0
    inputs += inputs0
    for i, (pat, pre, post, many) in enumerate(pats):
        subs = star_subjects(pre, post, many)
        docs.append({"apiVersion": API, "resourcePolicy": {"resource": "k%d" % i, "version": "default", "rules": [
            {"actions": [pat], "roles": ["*"], "effect": "EFFECT_ALLOW"}]}})
        inputs.append(request("act%d" % i, "k%d" % i, subs))
        groups["action " + pat] = [("act%d" % i, s) for s in subs]
        if pre and post:
            docs.append({"apiVersion": API, "resourcePolicy": {"resource": "r%d" % i, "version": "default", "rules": [
                {"actions": ["go"], "roles": [pat], "effect": "EFFECT_ALLOW"}]}})
            for k, s in enumerate(subs):
                inputs.append(request("role%d_%d" % (i, k), "r%d" % i, ["go"], roles=[s]))
            groups["role " + pat] = [("role%d_%d" % (i, k), "go") for k in range(len(subs))]
        if pre and post and pat.count("*") in (17, 18, 39, 40):
            docs.append({"apiVersion": API, "rolePolicy": {"role": "rp%d" % i, "rules": [{"resource": "rk", "allowActions": [pat]}]}})
            inputs.append(request("rp%d" % i, "rk", subs, roles=["rp%d" % i]))
            groups["allowActions " + pat] = [("rp%d" % i, s) for s in subs]
    docs.append({"apiVersion": API, "resourcePolicy": {"resource": "rk", "version": "default", "rules": [{"actions": ["*"], "roles": ["*"], "effect": "EFFECT_ALLOW"}]}})
    table_side = sorted({pre + TABLE_SIDE + post for _, pre, post, _ in pats})
    docs.append({"apiVersion": API, "resourcePolicy": {"resource": "lit", "version": "default", "rules": [
        {"actions": table_side, "roles": [s for s in table_side], "effect": "EFFECT_DENY"}]}})
    lay = Layer("star_runs", docs, inputs, groups=groups, kinds=(0, 2), plan_ok=_walks)
    lay.kernel_subjects = [s for _, pre, post, many in pats for s in star_subjects(pre, post, many) if s != pre + TABLE_SIDE + post]
    lay.table_subjects = table_side
    return lay


def _walks(plan):
    return "cbh_walk2_kernel" in plan or plan.startswith("cbh_check_kernel")


def check_glob_kernel_decides(lay):
    """the automaton has words, the kernel-side subjects are no strings of the table, the table-side ones are"""
    assert lay.lt.nfas[DIM_ACTION].words >= 1
    assert all(lay.lt.sid(s) is None for s in lay.kernel_subjects), [s[:40] for s in lay.kernel_subjects if lay.lt.sid(s) is not None][:5]
    assert all(lay.lt.sid(s) is not None for s in getattr(lay, "table_subjects", ()))


def lit(k, n):
    """n literal bytes that begin with pattern k's own two"""
    assert n >= 2
    return ("%c%c" % (chr(65 + k), chr(97 + k)) + "q" * n)[:n]


class Dim:
    """the patterns of one dimension in the order the lowering numbers them: `pos` = positions used so far (a linear pattern of n
    elements owns n + 1)"""

    def __init__(self):
        self.pos, self.pats, self.marks = 0, [], []

    def add(self, pat, elements, subjects, mark=None):
        if mark is not None:
            self.marks.append((self.pos + mark[0], mark[1]))
        self.pats.append((pat, subjects))
        self.pos += elements + 1

    def pad_to(self, total, k):
        """a last pattern `<literals>*` that fills the dimension to `total` positions"""
        n = total - self.pos - 2
        L = lit(k, n)
        self.add(L + "*", n + 1, [L, L + "xyz", L + "é😀", L + ":", L[:-1], L[:-1] + "x"], mark=(n, "star"))
        assert self.pos == total


MB = ("é", "日", "😀")     # 2, 3 and 4 bytes


def dim_star_on_bit_63(total=GLOB_POSITIONS):
    """`<literals>*z`: the star on bit 63 of words 0 .. 6 (the closure carries into the next word), `z` on bit 0 of the next"""
    d = Dim()
    for k in range(7):
        n = 64 * k + 63 - d.pos
        L = lit(k, n)
        d.add(L + "*z", n + 2, [L + "z", L + "mmz", L + "m:z", L + "zy", L[:-1] + "z"] + [L + c + "z" for c in MB], mark=(n, "star"))
    d.pad_to(total, 7)
    return d


def dim_star_on_bit_0():
    """`*<literals>` first (the star on bit 0 of word 0), then `<literals>*z` with the star on bit 0 of words 1 .. 7: the last literal
    advances from bit 63 (the carry of the step)"""
    d = Dim()
    L = lit(0, 4)
    d.add("*" + L, 5, [L, "xx" + L, "x:" + L, "日" + L, L + "x"], mark=(0, "star"))
    for k in range(1, 8):
        n = 64 * k - d.pos
        L = lit(k, n)
        d.add(L + "*z", n + 2, [L + "z", L + "mmz", L + "m:z", L + "zy", L[:-1] + "z"] + [L + c + "z" for c in MB], mark=(n, "star"))
    d.pad_to(GLOB_POSITIONS, 8)
    return d


def dim_class_on_bit_63(cls):
    """`**<literals>?z` / `**<literals>[!a-c]z`: the one-code-point element on bit 63 of words 0 .. 6 - its lead byte advances into
    the next word, the continuation bytes loop THERE (bit << 1)"""
    d = Dim()
    for k in range(7):
        n = 64 * k + 63 - d.pos - 1
        L = lit(k, n)
        subs = [L + c + "z" for c in MB] + [L + "mz", "pre:" + L + "éz", L + "éez", L + "😀😀z", L + "z", L + ":z", L + "az", L + "é"]
        d.add("**" + L + cls + "z", n + 3, subs, mark=(n + 1, "byte"))
    d.pad_to(GLOB_POSITIONS, 7)
    return d


def dim_literals_across():
    """`<70 literals>*`: a literal run across every word boundary"""
    d = Dim()
    for k in range(7):
        L = lit(k, 70)
        assert d.pos <= 64 * (k + 1) - 3 and d.pos + 70 >= 64 * (k + 1) + 3
        d.add(L + "*", 71, [L, L + "tail", L + ":", L[:62] + "x" + L[63:], L[:-1], L[:63] + "日" + L[64:]])
    d.pad_to(GLOB_POSITIONS, 7)
    return d


def boundary_layer(name, action_dim, role_dim=None, loud=False):
    """every pattern of `action_dim` an action of ONE rule list (kind `w`), in order; every pattern of `role_dim` the role of a rule
    of kind `v`.  Patterns begin with their own two bytes, so a subject is one pattern's."""
    docs, inputs, groups, subjects = [], [], {}, []
    docs.append({"apiVersion": API, "resourcePolicy": {"resource": "w", "version": "default", "rules": [
        {"actions": [p], "roles": ["*"], "effect": "EFFECT_ALLOW"} for p, _ in action_dim.pats]}})
    for i, (p, subs) in enumerate(action_dim.pats):
        inputs.append(request("act%d" % i, "w", subs))
        groups["action %d" % i] = [("act%d" % i, s) for s in subs]
        subjects += subs
    if role_dim is not None:
        docs.append({"apiVersion": API, "resourcePolicy": {"resource": "v", "version": "default", "rules": [
            {"actions": ["go"], "roles": [p], "effect": "EFFECT_ALLOW"} for p, _ in role_dim.pats]}})
        for i, (p, subs) in enumerate(role_dim.pats):
            for k, s in enumerate(subs):
                inputs.append(request("role%d_%d" % (i, k), "v", ["go"], roles=[s]))
            groups["role %d" % i] = [("role%d_%d" % (i, k), "go") for k in range(len(subs))]
            subjects += subs
    if loud:
        inputs.append(request("stranger", "no_such_kind", ["go"]))      # reaches no rule: decided whatever the lowering flagged
    lay = Layer(name, docs, inputs, groups=groups, loud=loud, kinds=(0, 2), plan_ok=_walks)
    lay.kernel_subjects = subjects
    for d, dim in ((DIM_ACTION, action_dim), (DIM_ROLE, role_dim)):
        if dim is None or loud:
            continue
        nfa = lay.lt.nfas[d]
        assert nfa.nbits == dim.pos == GLOB_POSITIONS and nfa.words == 8, (name, d, nfa.nbits, dim.pos)
        for bit, what in dim.marks:   # the layout the generator claims, read off the lowering's own tables
            assert bool((nfa.star >> bit) & 1) == (what == "star"), (name, d, bit, what)
            assert what == "star" or (nfa.self_[0x80] >> (bit + 1)) & 1, (name, d, bit, "no continuation-byte loop after it")
    return lay


LONG = (3_000, MAX_DEVICE_STRING)


def make_long_subjects():
    """actions and roles of 3 000 and 65 535 bytes, decided by the last byte; a `:` inside a `*` (no match) and inside a `**`"""
    docs = [{"apiVersion": API, "resourcePolicy": {"resource": "long", "version": "default", "rules": [
        {"actions": ["one:*z"], "roles": ["*"], "effect": "EFFECT_ALLOW"}, {"actions": ["two**z"], "roles": ["*"], "effect": "EFFECT_ALLOW"}]}},
        {"apiVersion": API, "resourcePolicy": {"resource": "longrole", "version": "default", "rules": [
            {"actions": ["go"], "roles": ["one:*z"], "effect": "EFFECT_ALLOW"}, {"actions": ["go"], "roles": ["two**z"], "effect": "EFFECT_ALLOW"}]}}]
    inputs, groups, subjects = [], {}, []
    for n in LONG:
        subs = []
        for head in ("one:", "two:"):
            body = n - len(head) - 1
            subs += [head + "x" * body + "z", head + "x" * body + "y", head + "x" * (body // 2) + ":" + "x" * (body - body // 2 - 1) + "z",
                     head + "é" * (body // 2) + "x" * (body % 2) + "z"]
        assert all(len(s.encode()) == n for s in subs)
        inputs.append(request("act%d" % n, "long", subs))
        groups["action %d" % n] = [("act%d" % n, s) for s in subs]
        for k, s in enumerate(subs):
            inputs.append(request("role%d_%d" % (n, k), "longrole", ["go"], roles=[s]))
        groups["role %d" % n] = [("role%d_%d" % (n, k), "go") for k in range(len(subs))]
        subjects += subs
    lay = Layer("long_subjects", docs, inputs, groups=groups, kinds=(0, 2), plan_ok=_walks)
    lay.kernel_subjects = subjects
    return lay


# ---- 2. `matches`


def cel_string(s):
    return '"' + s.replace("\\", "\\\\").replace('"', '\\"') + '"'


BIG = r"(a|b)*a(a|b){8}$"                      # 514 states
TOO_BIG = r"(a|b)*a(a|b){9}$"                  # beyond 1024: refused by the lowering, flagged, never answered
CLASSES = "^[a-b][c-d][e-f][g-h][i-j][k-l][m-n][o-p][q-r][s-t][u-v][w-x][y-z][0-1][2-3][4-5][6-7][8-9]+é日😀$"   # 18 ASCII ranges + non-ASCII
MATCH_LENGTHS = (300, 4_096, 40_000, MAX_DEVICE_STRING)
MATCH_CONDS = {
    "end": 'R.attr.s.matches("ab$")',               # bit 1 of the state's flags: decided at the last byte
    "head": 'R.attr.s.matches("^ab")',              # bit 0: the early exit
    "only": 'R.attr.s.matches("^[a-x]*yz$")',       # the only match ends at the final byte
    "dot": 'R.attr.s.matches("^.{3}$")', "any": 'R.attr.s.matches("^.$")', "not_a": 'R.attr.s.matches("^[^a]+$")', "dots": 'R.attr.s.matches("^x.*.y$")', "blank": 'R.attr.s.matches("^b*$")',
    "big": "R.attr.s.matches(%s)" % cel_string(BIG), "too_big": "R.attr.s.matches(%s)" % cel_string(TOO_BIG),
    "classes": "R.attr.s.matches(%s)" % cel_string(CLASSES),
}
CLASS_HIT = "acegikmoqsuwy02468"


def make_matches():
    conds = dict(MATCH_CONDS)
    const = "x" * (4_096 - 2) + "ab"
    conds["const"] = "R.attr.s == %s" % cel_string(const)    # makes `const` a string of the table: str_span's other branch
    inputs, groups = [], {k: [] for k in ("empty", "utf8", "classes", "table side")}
    small = [a for a in conds if a != "too_big"]

    def add(rid, s, label, acts, ask=None):
        inputs.append(request(rid, "text", ask or list(conds), rattr={"s": s}))
        for a in acts:
            groups.setdefault("%s %s" % (a, label), []).append((rid, a))

    for n in MATCH_LENGTHS:
        for k, s in enumerate(("x" * (n - 2) + "ab", "x" * (n - 2) + "ac", "ab" + "x" * (n - 2), "ac" + "x" * (n - 2), "c" * (n - 2) + "yz", "c" * (n - 2) + "yy",
                               "x" + "😀" * ((n - 2) // 4) + "é" * ((n - 2) % 4 // 2) + "y", "x" + "😀" * ((n - 2) // 4) + "é" * ((n - 2) % 4 // 2) + "z")):
            assert len(s.encode()) == n or n % 2, (n, k)
            add("len%d_%d" % (n, k), s, n, ("end", "head", "only", "dots"), ask=("end", "head", "only", "dots", "blank", "not_a", "too_big", "const"))
    for k, s in enumerate(("", "a", "😀", "😀😀", "😀😀😀", "😀a😀", "😀😀😀😀", "é日😀", "a😀", "\n", "ab", "yz")):
        add("utf8_%d" % k, s, "utf8", ())
        groups["utf8"] += [("utf8_%d" % k, a) for a in ("dot", "any", "not_a")]
        if not s:
            groups["empty"] += [("utf8_0", a) for a in small]
    rng = np.random.default_rng(514)
    for n in (9, 10, 300, 4_096):
        for k in range(6 if n < 4_096 else 2):     # (the oracle's `re` backtracks over (a|b)* from every start: quadratic)
            s = "".join(rng.choice(list("ab"), n))
            s = s[:n - 9] + "ab"[k % 2] + s[n - 8:]           # the byte that decides: nine from the end
            add("ab%d_%d" % (n, k), s, n, ("big",))
    for k, s in enumerate((CLASS_HIT + "é日😀", CLASS_HIT + "999é日😀", CLASS_HIT[:-1] + "7é日😀", CLASS_HIT + "é日", "b" + CLASS_HIT[1:] + "é日😀", "c" + CLASS_HIT[1:] + "é日😀",
                           CLASS_HIT + "é日😀x", CLASS_HIT[:9] + "p" + CLASS_HIT[10:] + "é日😀", CLASS_HIT + "é本😀")):
        add("cls%d" % k, s, "classes", ())
        groups["classes"].append(("cls%d" % k, "classes"))
    add("const0", const, "const", ())
    add("const1", const[:-1] + "c", "const", ())
    groups["table side"] = [(r, a) for r in ("const0", "const1") for a in ("end", "const")]
    over = {(i["requestId"], "too_big") for i in inputs if "too_big" in i["actions"]}
    lay = Layer("matches", cond_store("text", conds), inputs, over=over, groups={k: v for k, v in groups.items() if v}, refused=1)
    assert lay.lt.sid(const) is not None and lay.lt.sid(const[:-1] + "c") is None
    return lay


def random_pattern_layer():
    """tests/test_regex.py's random layer with subjects of 0 - 300 bytes, through the device: 60 patterns the lowering accepts as the
    conditions of one store, 140 subjects, every pair checked (8 400 checks; the floor stays 8 000)"""
    from cerbos_amd.lower import regex
    from test_regex import _random_pattern
    rng = np.random.default_rng(11)
    pats = []
    while len(pats) < 60:
        p = ("^" if rng.random() < 0.3 else "") + _random_pattern(rng) + ("$" if rng.random() < 0.3 else "")
        try:
            regex.compile_regex(p)
            celeval._re(p)
        except Exception:    # (the generator can stack two repetition operators: invalid RE2)
            continue
        if p not in pats:
            pats.append(p)
    conds = {"p%d" % i: "R.attr.s.matches(%s)" % cel_string(p) for i, p in enumerate(pats)}
    alphabet = list("abcx.1 _é\n")
    inputs = []
    for k in range(140):
        n = int(rng.integers(0, 8)) if k % 4 == 0 else int(rng.integers(0, 301))
        s = "".join(str(rng.choice(alphabet)) for _ in range(n))
        s = s.encode()[:300].decode("utf-8", "ignore")
        inputs.append(request("q%d" % k, "text", list(conds), rattr={"s": s}))
    lay = Layer("random_patterns", cond_store("text", conds), inputs, groups={"all": [(i["requestId"], a) for i in inputs for a in conds]})
    assert len(inputs) * len(conds) >= 8_000
    assert max(len(i["resource"]["attr"]["s"].encode()) for i in inputs) > 250
    return lay


# ---- 3. windows, ropes and the byte loops


HEAD = "é" * 5 + "日" * 5      # 25 bytes, 10 code points: byte offsets and code-point indices differ from here on
HEAD_BYTES, HEAD_CPS = 25, 10


def window_ok(first, length):
    return first <= WINDOW_MAX and length <= WINDOW_MAX


def cp_to_byte(s, i):
    return len(s[:i].encode())


def near(s):
    """differs from s in its last byte"""
    return s[:-1] + ("#" if s[-1:] != "#" else "%") if s else "#"


WINDOW_CONDS = {
    "sub1": "R.attr.s.substring(int(P.attr.i)) == P.attr.x",
    "sub2": "R.attr.s.substring(int(P.attr.i), int(P.attr.j)) == P.attr.x",
    "chr": "R.attr.s.charAt(int(P.attr.i)) == P.attr.x",
    "trim": "R.attr.s.trim() == P.attr.x",
    "rep": 'R.attr.s.replace("ab", "X") == P.attr.x',
    "spl": 'R.attr.s.split(",")[1] == P.attr.x',
    "spln": 'R.attr.s.split(",", 2)[1] == P.attr.x',
}
WINDOW_LENGTHS = (WINDOW_MAX - 1, WINDOW_MAX, WINDOW_MAX + 1, WINDOW_MAX + 2, MAX_DEVICE_STRING)
assert WINDOW_LENGTHS == (32_765, 32_766, 32_767, 32_768, 65_535)


def make_windows():
    """every case twice: the expected value, and one that differs in its last byte.  `over` from window_ok alone."""
    inputs, over, groups = [], set(), {}
    sides = {}    # condition -> {"first" / "length" / "string": set of (value at or beyond the limit)}

    def add(cond, label, s, want, first, length, whole=None, **params):
        ok = window_ok(first, length) and (whole is None or whole <= WINDOW_MAX)
        for tag, x in (("eq", want), ("ne", near(want))):
            rid = "%s_%s_%d_%s" % (cond, label, len(inputs), tag)
            inputs.append(request(rid, "text", [cond], pattr=dict(params, x=x), rattr={"s": s}))
            groups.setdefault("%s %s" % (cond, label), []).append((rid, cond))
            if not ok:
                over.add((rid, cond))
        sides.setdefault(cond, set()).update({("first", first), ("length", length), ("string", whole)})

    for n in WINDOW_LENGTHS:
        s = HEAD + "x" * (n - HEAD_BYTES - 4) + "日" + "w"
        assert len(s.encode()) == n
        cps = len(s)
        for i in (0, 1, 5, 6):                       # substring(i): first = the bytes before code point i, length = the rest
            b0 = cp_to_byte(s, i)
            add("sub1", n, s, s[i:], b0, n - b0, i=float(i))
        if n == MAX_DEVICE_STRING:
            for b0 in (WINDOW_MAX - 1, WINDOW_MAX, WINDOW_MAX + 1, WINDOW_MAX + 2):
                i = HEAD_CPS + b0 - HEAD_BYTES
                assert cp_to_byte(s, i) == b0
                for ln in (WINDOW_MAX - 1, WINDOW_MAX, WINDOW_MAX + 1):      # substring(i, j) in the ASCII filler: bytes = code points
                    if b0 + ln <= n - 4:
                        add("sub2", "first%d" % b0, s, s[i:i + ln], b0, ln, i=float(i), j=float(i + ln))
                add("sub2", "first%d" % b0, s, s[i:i + 9], b0, 9, i=float(i), j=float(i + 9))
                add("chr", "first%d" % b0, s, s[i], b0, 1, i=float(i))
            i = cps - 2                               # the 3-byte character near the end
            add("chr", "last", s, s[i], cp_to_byte(s, i), 3, i=float(i))
            add("sub1", "tail", s, s[i:], cp_to_byte(s, i), 4, i=float(i))
        for ln in (0, 1, 7):
            add("sub2", n, s, s[2:2 + ln], 4, cp_to_byte(s, 2 + ln) - 4, i=2.0, j=float(2 + ln))
        add("sub2", n, s, s[3:cps - 1], 6, n - 7, i=3.0, j=float(cps - 1))
    s = HEAD + "x" * (2 * WINDOW_MAX - HEAD_BYTES - 4) + "日" + "w"      # substring(i) with first byte AND length at the limit: 2 * WINDOW_MAX bytes
    for b0 in (WINDOW_MAX - 1, WINDOW_MAX, WINDOW_MAX + 1):
        i = HEAD_CPS + b0 - HEAD_BYTES
        add("sub1", "twice", s, s[i:], b0, 2 * WINDOW_MAX - b0, i=float(i))
        add("sub2", "twice", s, s[i:], b0, 2 * WINDOW_MAX - b0, i=float(i), j=float(len(s)))
    for n in (WINDOW_MAX - 1, WINDOW_MAX, WINDOW_MAX + 1, WINDOW_MAX + 2):      # trim(): the body's length
        body = "é" + "b" * (n - 5) + "日"
        lead, trail = "　\t  ", "  \n "
        s = lead + body + trail
        assert len(body.encode()) == n
        add("trim", n, s, body, len(lead.encode()), n)
    for b0 in (WINDOW_MAX - 1, WINDOW_MAX, WINDOW_MAX + 1):                     # trim(): the body's first byte
        lead = "\u3000" * (b0 // 3) + " " * (b0 % 3)
        assert len(lead.encode()) == b0
        add("trim", "first%d" % b0, lead + "éb日" + "\u2003\n", "éb日", b0, 6)
    for n in WINDOW_LENGTHS[:4]:                     # replace() and split(): the string's length
        s = "ab" + HEAD + "c" * (n - HEAD_BYTES - 11) + "ab,日,ab"
        assert len(s.encode()) == n
        add("rep", n, s, s.replace("ab", "X"), 0, 0, whole=n)
        add("spl", n, s, s.split(",")[1], 0, 0, whole=n)
        add("spln", n, s, s.split(",", 1)[1], 0, 0, whole=n)
    errors = set()
    for n in (WINDOW_MAX, MAX_DEVICE_STRING):        # substring / charAt beyond the end: an evaluation error, whatever the length (no window is made)
        s = HEAD + "x" * (n - HEAD_BYTES)
        for cond, i in (("sub1", len(s) + 1), ("chr", len(s) + 1), ("sub2", len(s))):
            rid = "%s_beyond_%d" % (cond, n)
            inputs.append(request(rid, "text", [cond], pattr={"i": float(i), "j": float(len(s) + 1), "x": ""}, rattr={"s": s}))
            errors.add((rid, cond))
    lay = Layer("windows", cond_store("text", WINDOW_CONDS), inputs, over=over, groups=groups, errors=errors)
    for cond, seen in sides.items():    # both sides of the boundary are there, for every condition, as the quantity the condition can reach
        for what in ("first", "length", "string"):
            vals = {v for w, v in seen if w == what and v is not None}
            if max(vals, default=0) > WINDOW_MAX:
                assert {WINDOW_MAX, WINDOW_MAX + 1} <= vals, (cond, what, sorted(vals))
    assert {c for _, c in over} == set(WINDOW_CONDS)
    return lay


def replace_fits(s, old):
    """ARENA restated: one entry per hit, one more for the bytes before it; room for two before every hit, for one after the last"""
    ap = frm = i = 0
    while i + len(old) <= len(s):
        if s[i:i + len(old)] != old:
            i += 1
            continue
        if ap + 2 > ARENA:
            return False
        ap += 1 + (i > frm)
        i += len(old)
        frm = i
    return ap + 1 <= ARENA


ARENA_CONDS = {
    "rep": 'R.attr.s.replace("ab", "X") == P.attr.x',
    "rep_aa": 'R.attr.s.replace("aa", "b") == P.attr.x',
    "rep_size": 'size(R.attr.s.replace("ab", "")) == int(P.attr.z)',
    "spl": 'R.attr.s.split(",")[int(P.attr.k)] == P.attr.x',
}


def make_arena():
    inputs, over, groups = [], set(), {}

    def add(cond, label, s, old, new, fits=None):
        want = s.replace(old, new)
        fits = replace_fits(s, old) if fits is None else fits
        for tag, x in (("eq", want), ("ne", near(want))):
            rid = "%s_%s_%s" % (cond, label, tag)
            inputs.append(request(rid, "text", [cond], pattr={"x": x, "z": float(len(want) + (tag == "ne")), "k": 0.0}, rattr={"s": s}))
            groups.setdefault(cond, []).append((rid, cond))
            if not fits:
                over.add((rid, cond))
        return fits

    edge = {}
    for shape, unit, tail in (("adjacent", "ab", ""), ("gaps", "ab.", ""), ("gaps_tail", ".ab", "."), ("ends", "ab..", "ab")):
        fitting = [k for k in range(1, 60) if replace_fits(unit * k + tail, "ab")]
        top = max(fitting)
        assert fitting == list(range(1, top + 1))
        edge[shape] = top
        for k in (1, top - 1, top, top + 1, top + 2):
            assert add("rep", "%s%d" % (shape, k), unit * k + tail, "ab", "X") == (k <= top)
            add("rep_size", "%s%d" % (shape, k), unit * k + tail, "ab", "")
    assert edge == {"adjacent": 47, "gaps": 24, "gaps_tail": 23, "ends": 23}, edge     # (what the rule above gives for 48 entries)
    for k in (2, 3, 4, 5, 94, 95, 96, 97):            # "aaa".replace("aa", ...): not overlapping
        add("rep_aa", "a%d" % k, "a" * k, "aa", "b")
    assert replace_fits("a" * 95, "aa") and not replace_fits("a" * 96, "aa")
    for k in (2, ARENA // 2 - 1, ARENA // 2, ARENA // 2 + 1, ARENA // 2 + 2):       # split: two entries per piece
        s = ",".join("p%d" % j for j in range(k))
        for tag, x in (("eq", "p0"), ("ne", "p1")):
            rid = "spl_%d_%s" % (k, tag)
            inputs.append(request(rid, "text", ["spl"], pattr={"x": x, "z": 0.0, "k": 0.0}, rattr={"s": s}))
            groups.setdefault("spl", []).append((rid, "spl"))
            if 2 * k > ARENA:
                over.add((rid, "spl"))
    return Layer("arena", cond_store("text", ARENA_CONDS), inputs, over=over, groups=groups)


LOOP_CONDS = {
    "starts": "R.attr.s.startsWith(P.attr.n)", "ends": "R.attr.s.endsWith(P.attr.n)", "has": "R.attr.s.contains(P.attr.c)",
    "idx": "R.attr.s.indexOf(P.attr.c) == int(P.attr.i)", "lidx": "R.attr.s.lastIndexOf(P.attr.c) == int(P.attr.i)",
    "size": "size(R.attr.s) == int(P.attr.z)", "lt": "R.attr.s < P.attr.n", "ge": "R.attr.s >= P.attr.n",
    "lower": "R.attr.s.lowerAscii() == P.attr.n.lowerAscii()", "upper": "R.attr.s.upperAscii() == P.attr.n.upperAscii()",
    "anc": "hierarchy(R.attr.s).ancestorOf(hierarchy(P.attr.n))", "sib": "hierarchy(R.attr.s).siblingOf(hierarchy(P.attr.n))",
    "parent": "hierarchy(R.attr.s).immediateParentOf(hierarchy(P.attr.n))", "overlaps": "hierarchy(R.attr.s).overlaps(hierarchy(P.attr.n))",
    "common": "hierarchy(R.attr.s).commonAncestors(hierarchy(P.attr.n)) == hierarchy(P.attr.h)",
    "rope_has": "R.attr.s.lowerAscii().contains(P.attr.rc)", "rope_ends": "R.attr.s.lowerAscii().endsWith(P.attr.rc)",
    "sub_eq": "R.attr.s.substring(1) == P.attr.n.substring(1)", "rep_eq": 'R.attr.s.replace("日", "ab") == P.attr.n.replace("日", "ab")',
}
LOOP_LENGTHS = (4_096, MAX_DEVICE_STRING)


def make_byte_loops():
    """s = <head> Abcdefg.Abcdefg. ... .uVZ of n bytes, `Z` only at its end; the other operand is s itself, s with another last byte
    (greater, smaller, the other case), s without its last / first byte, s with another first byte; `child`: the subject is s
    without its last segment, the other operand s.  No operand is longer than the device road's 65 535 bytes."""
    inputs, groups = [], {}
    for n in LOOP_LENGTHS:
        seg = "Abcdefg."
        body = n - HEAD_BYTES - 1
        s = HEAD + (seg * (body // len(seg) + 1))[:body - 3] + ".uV" + "Z"
        assert len(s.encode()) == n and s.count("Z") == 1 and "z" not in s
        parent = s.rsplit(".", 1)[0]
        if n == LOOP_LENGTHS[0]:
            table_side = s
        cases = [   # name, subject, other, c (contains / indexOf), i, rope c, size
            ("same", s, s, "Z", len(s) - 1, "vz", len(s)),
            ("smaller", s, s[:-1] + "Y", "Y", len(s) - 1, "VZ", len(s) + 1),
            ("greater", s, s[:-1] + "a", "VZ", len(s) - 2, "uvz", len(s) - 1),
            ("case", s, s[:-1] + "z", "z", -1, "uvZ", len(s)),
            ("prefix", s, s[:-1], "uVZ", len(s) - 3, ".uvz", len(s)),
            ("suffix", s, s[1:], "ZZ", len(s) - 1, "uvzz", 0),
            ("head", s, "f" + s[1:], "gA", 6, "g.uvz", len(s)),
            ("child", parent, s, ".uV", len(parent), "fg", len(parent)),
        ]
        for name, subject, other, c, i, rc, z in cases:
            assert max(len(subject.encode()), len(other.encode())) <= MAX_DEVICE_STRING
            rid = "%s_%d" % (name, n)
            acts = [a for a in LOOP_CONDS if not (n > WINDOW_MAX and a in ("sub_eq", "rep_eq"))] + (["const"] if n == LOOP_LENGTHS[0] else [])
            inputs.append(request(rid, "text", acts, pattr={"n": other, "c": c, "rc": rc, "i": float(i), "z": float(z), "h": parent}, rattr={"s": subject}))
            for a in acts:
                groups.setdefault("%s %d" % (a, n), []).append((rid, a))
    conds = dict(LOOP_CONDS, const="P.attr.n == %s" % cel_string(table_side))     # the 4 096-byte subject is ALSO a string of the table
    lay = Layer("byte_loops", cond_store("text", conds), inputs, groups=groups)
    assert lay.lt.sid(table_side) is not None and lay.lt.sid(table_side[:-1] + "Y") is None
    return lay


MAKERS = {
    "star_runs": make_star_runs,
    "words_a": lambda: boundary_layer("words_a", dim_star_on_bit_63(), dim_star_on_bit_0()),
    "words_b": lambda: boundary_layer("words_b", dim_class_on_bit_63("?"), dim_literals_across()),
    "words_c": lambda: boundary_layer("words_c", dim_class_on_bit_63("[!a-c]")),
    "words_513": lambda: boundary_layer("words_513", dim_star_on_bit_63(GLOB_POSITIONS + 1), loud=True),
    "long_subjects": make_long_subjects,
    "matches": make_matches,
    "random_patterns": random_pattern_layer,
    "windows": make_windows,
    "arena": make_arena,
    "byte_loops": make_byte_loops,
}
GLOB_LAYERS = ("star_runs", "words_a", "words_b", "words_c", "long_subjects")
LAYERS = tuple(MAKERS)


# ---- CPU tier: what the generators must make happen


def test_the_limits_are_the_headers():
    assert header_value("CBH_ROPE_WINDOW_MAX", "cbh_vm.h") == WINDOW_MAX
    assert header_value("CBH_ARENA_ENTRIES", "cbh_blob.h") == ARENA
    assert header_value("NFA_MAXW", "cbh_kernels.h") * 64 == GLOB_POSITIONS
    from cerbos_amd.lower.globs import GlobNFA
    assert GlobNFA.MAX_WORDS * 64 == GLOB_POSITIONS


@pytest.mark.parametrize("name", LAYERS)
def test_the_oracle_decides_and_the_requests_discriminate(name):
    lay = layer(name)
    if not lay.loud:
        lay.check_oracle()
    if name in GLOB_LAYERS:
        check_glob_kernel_decides(lay)


def test_the_glob_reference_is_glob_match():
    """the layer's expectations are glob_match's own, pattern by pattern (oracle/check.py goes through it)"""
    lay = layer("star_runs")
    for i, (pat, pre, post, many) in enumerate(star_patterns()):
        for s in star_subjects(pre, post, many):
            assert lay.allow("act%d" % i, s) == glob_match(pat, s), (pat, s)
    assert glob_match("a" + "*" * 17 + "b", "ab") and lay.allow("issue", "ab") and not lay.allow("issue", "b")


def test_star_runs_collapse_in_the_lowering():
    from cerbos_amd.lower.globs import GlobNFA, parse_glob
    for n in STAR_RUNS:
        for form in ("all", "one", "single"):
            for pre, post in (("a", "b"), ("", "b"), ("a", "")):
                seq, = parse_glob(pre + star_run(n, form) + post)
                assert [e[0] for e in seq] == ["B"] * len(pre) + ["S"] + ["B"] * len(post)
                assert (ord(":") in seq[len(pre)][1]) == (form == "all" or (form == "one" and n > 1))
    assert [len(s) for s in parse_glob("*{*,a}{**,b*}")] == [1, 3, 3, 4]     # alternatives are expanded first
    nfa = GlobNFA(["a" + "*" * 17 + "b", "x{*}{*}", "**"])
    assert not nfa.star & (nfa.star << 1) and nfa.nbits == 4 + 3 + 2


def test_the_large_automata_are_what_the_text_says():
    from cerbos_amd.lower import regex
    assert regex.compile_regex(BIG).n_states == 514 and regex.compile_regex(CLASSES).n_classes >= 20
    with pytest.raises(regex.Unsupported):
        regex.compile_regex(TOO_BIG)
    lay = layer("matches")
    assert len(lay.lt.unsupported) == 1 and str(REGEX_STATES) in lay.lt.unsupported[0][1]
    for pat, subject in ((BIG, "ab" * 20 + "a"), (CLASSES, CLASS_HIT + "é日😀")):
        assert celeval._re(pat).search(subject) is not None


# ---- CPU tier: the kernels on the wave emulator (glob bits from the host: see the module's text)


@pytest.mark.parametrize("name", LAYERS)
def test_on_emulator(name):
    run_on_emulator(layer(name))


# ---- CPU tier: the library on the simulator - the glob kernel's own source


@pytest.fixture()
def engine():
    from sim_engine import sim_engine
    with sim_engine() as capi:
        yield capi


@pytest.mark.parametrize("name", ["star_runs"])
def test_star_runs_on_simulator(engine, name):
    run_on_library(engine, layer(name))


@pytest.mark.parametrize("name", ["words_a", "words_b", "words_c", "words_513"])
def test_word_boundaries_on_simulator(engine, name):
    run_on_library(engine, layer(name))


@pytest.mark.parametrize("name", [n for n in LAYERS if n != "star_runs" and not n.startswith("words")])
def test_on_simulator(engine, name):
    run_on_library(engine, layer(name))


# ---- GPU tier


@pytest.mark.gpu
@pytest.mark.parametrize("name", LAYERS)
def test_on_gpu(name):
    from cerbos_amd import capi       # (CBH_TEST_SIM_ENGINE=1, the developer's aid of tests/conftest.py: the simulator)
    run_on_library(capi, layer(name))
