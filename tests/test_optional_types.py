"""cel-go optional values (cel.OptionalTypes(): `e.?f`, `e[?k]`, `[?e]`, `{?k: v}`, optional.of / none / ofNonZeroValue, hasValue,
value, orValue, or, optMap, optFlatMap, optional equality) on values the request supplies.

Two independent checks:

* desugared twins - every optional condition beside cel-go's definition of it written without optional syntax (`a.?f` is
  `has(a.f) ? optional.of(a.f) : optional.none()`, a chain the conjunction of its presence tests, `xs[?i]` a bounds test ...): the
  device decides the optional store, the oracle the twin store, over requests whose attributes are present, absent, null, of
  the wrong type and nested.  Per action: effect; per request: whether evaluation errors were recorded, and - through the trace
  pass - which;
* known answers written here for constant forms and request values.

Optional qualifiers on an operand that is neither a map nor a list (cel-go's answer is not pinned here) are flagged for the
caller's engine, never answered.  CPU tier: the kernel source on the host simulator; GPU tier: the kernel."""
import numpy as np
import pytest

from cerbos_amd import capi, workloads
from cerbos_amd.cel import parser as celparser
from cerbos_amd.engine import Conf, HipEvaluator
from cerbos_amd.flatten import Flattener
from cerbos_amd.lower.blob import lower_rule_table
from cerbos_amd.policy.loader import policies_from_docs
from cerbos_amd.ruletable.build import rule_table_from_policies
from cerbos_amd.ruletable.proto import decode_rule_table, encode_rule_table
from helpers import norm_actions
from oracle.check import EvalParams, RuleTableOracle

API = "api.cerbos.dev/v1"
NOW = 1_700_000_000_000_000_000


def _of(a, f):
    return "(has(%s.%s) ? optional.of(%s.%s) : optional.none())" % (a, f, a, f)


# action: (condition with optional syntax, its twin without)
TWINS = {
    "sel_or": ("R.attr.?x.orValue(5.0) > 3.0", "(has(R.attr.x) ? R.attr.x : 5.0) > 3.0"),
    "sel_has": ("R.attr.?x.hasValue()", "has(R.attr.x)"),
    "sel_value": ("R.attr.?x.value() > 1.0", "(has(R.attr.x) ? R.attr.x : optional.none().value()) > 1.0"),
    "sel_of": ("R.attr.?x.orValue(0.0) == R.attr.?y.orValue(0.0)", "%s.orValue(0.0) == %s.orValue(0.0)" % (_of("R.attr", "x"), _of("R.attr", "y"))),
    "chain": ('R.attr.?m.k.orValue("none") == "a"', '(has(R.attr.m) && has(R.attr.m.k) ? R.attr.m.k : "none") == "a"'),
    "chain_has": ("R.attr.?m.?k.hasValue()", "has(R.attr.m) && has(R.attr.m.k)"),
    "before_opt": ('R.attr.m.?k.orValue("z") == "z"', '(has(R.attr.m.k) ? R.attr.m.k : "z") == "z"'),
    "idx_map": ('R.attr.lim[?"export"].orValue(0.0) >= 10.0', '("export" in R.attr.lim ? R.attr.lim["export"] : 0.0) >= 10.0'),
    "idx_key": ("R.attr.lim[?R.attr.which].orValue(-1.0) > 0.0", "(R.attr.which in R.attr.lim ? R.attr.lim[R.attr.which] : -1.0) > 0.0"),
    "idx_list": ("R.attr.xs[?1].orValue(-1.0) > 0.0", "(size(R.attr.xs) > 1 ? R.attr.xs[1] : -1.0) > 0.0"),
    "idx_list_dyn": ("R.attr.xs[?int(R.attr.n)].hasValue()", "int(R.attr.n) >= 0 && int(R.attr.n) < size(R.attr.xs)"),
    "or": ("R.attr.?x.or(R.attr.?y).orValue(0.0) == 2.0", "(has(R.attr.x) ? R.attr.x : has(R.attr.y) ? R.attr.y : 0.0) == 2.0"),
    "or_none": ("optional.none().or(R.attr.?y).hasValue()", "has(R.attr.y)"),
    "nonzero": ('optional.ofNonZeroValue(R.attr.s).orValue("empty") == "empty"',
                '(R.attr.s == "" || R.attr.s == 0.0 || R.attr.s == false || R.attr.s == null || R.attr.s == [] || R.attr.s == {} '
                '? "empty" : R.attr.s) == "empty"'),
    "of_value": ("optional.of(R.attr.x).value() == 2.0", "R.attr.x == 2.0"),
    "opt_eq": ("R.attr.?x == R.attr.?y", "%s == %s" % (_of("R.attr", "x"), _of("R.attr", "y"))),
    "opt_ne_const": ("R.attr.?x != optional.of(2.0)", "%s != optional.of(2.0)" % _of("R.attr", "x")),
    "opt_eq_none": ("R.attr.?x == optional.none()", "!has(R.attr.x)"),
    "opt_map": ("R.attr.?x.optMap(v, v * 2.0).orValue(0.0) > 5.0", "(has(R.attr.x) ? R.attr.x * 2.0 : 0.0) > 5.0"),
    "opt_flat_map": ("R.attr.?m.optFlatMap(v, v.?k).hasValue()", "has(R.attr.m) && has(R.attr.m.k)"),
    "comp_local": ('R.attr.items.exists(it, it.?tag.orValue("") == "red")', 'R.attr.items.exists(it, (has(it.tag) ? it.tag : "") == "red")'),
    "bind_opt": ("cel.bind(o, R.attr.?x, o.hasValue() && o.value() > 2.0)", "has(R.attr.x) && R.attr.x > 2.0"),
    "bind_local": ('cel.bind(mm, R.attr.m, mm.?k.orValue("z") == "a")', '(has(R.attr.m.k) ? R.attr.m.k : "z") == "a"'),
    "principal": ('P.attr.?department.orValue("") == R.attr.department', '(has(P.attr.department) ? P.attr.department : "") == R.attr.department'),
    "tern_opt": ("(R.attr.flag == true ? R.attr.?x : R.attr.?y).orValue(1.0) == 1.0",
                 "(R.attr.flag == true ? (has(R.attr.x) ? R.attr.x : 1.0) : (has(R.attr.y) ? R.attr.y : 1.0)) == 1.0"),
}

RENAME = {t: o for o, t in TWINS.values()}
XV = [2.0, 3.5, -1.0, 0.0, 1.0, 6.0, "2", None, True]


def _docs(conds, kind):
    return [{"apiVersion": API, "resourcePolicy": {"resource": kind, "version": "default", "rules": [
        {"actions": [n], "roles": ["*"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": e}}} for n, e in conds.items()]}}]


def _inputs(actions, n=500, seed=760):
    rng = np.random.default_rng(seed)
    out = []
    for r in range(n):
        attr = {"x": XV[int(rng.integers(0, len(XV)))], "y": XV[int(rng.integers(0, len(XV)))],
                "lim": {k: float(rng.integers(0, 20)) for k in rng.choice(["export", "import", "read"], size=int(rng.integers(0, 3)), replace=False)},
                "which": str(rng.choice(["export", "import", "nope"])),
                "xs": [float(v) for v in rng.choice([1.0, -2.0, 3.0], size=int(rng.integers(0, 4)))],
                "n": float(rng.choice([0, 1, 2, 5, -1])),
                "m": {"k": str(rng.choice(["a", "b"]))} if rng.random() < 0.5 else {"j": 1.0},
                "s": [None, "", "x", 0.0, 3.0, False, True, [], ["a"], {}, {"a": 1.0}][int(rng.integers(0, 11))],
                "items": [{"tag": str(rng.choice(["red", "blue"]))} if rng.random() < 0.6 else {"other": 1.0} for _ in range(int(rng.integers(0, 3)))],
                "department": str(rng.choice(["eng", "ops", ""])), "flag": bool(rng.random() < 0.5)}
        for k in ("x", "y", "m", "lim", "s", "n"):   # absent now and then
            if rng.random() < 0.2:
                del attr[k]
        pattr = {"department": str(rng.choice(["eng", "ops"]))} if rng.random() < 0.7 else {}
        out.append({"requestId": "o%d" % r, "actions": list(actions), "principal": {"id": "p", "roles": ["user"], "attr": pattr},
                    "resource": {"kind": "opt", "id": "o%d" % r, "attr": attr}})
    return out


def _run(ev, lt, inputs, close):
    try:
        batch = Flattener(lt).flatten(inputs)
        res = ev.table.check(batch, now_ns=NOW, flags=0)
        outs, bad = ev.assemble(inputs, batch, res, "default", allow_unsupported=True)
        touts, tbad, incomplete = ev.check(inputs, now_ns=NOW, allow_unsupported=True, trace=True)
    finally:
        if close:
            ev.close()
    return res, outs, bad, touts, tbad, incomplete


def _lower(docs):
    rt = rule_table_from_policies(policies_from_docs(docs))
    return rt, lower_rule_table(rt)


def _errors(errs, rename):
    """Evaluation errors as text, a twin's expression named by the optional condition it stands for."""
    out = []
    for e in errs or []:
        if isinstance(e, dict) and "celError" in e:
            e = dict(e, celError=dict(e["celError"], expression=rename.get(e["celError"]["expression"], e["celError"]["expression"])))
        out.append(str(e))
    return sorted(out)


def _compare_twins(make, close, opt_docs, twin_docs, actions, inputs, min_discriminating, min_errors=1, lowered=None, rename=None):
    """The device on the optional store against the oracle on its twin (`rename`: twin expression -> optional expression)."""
    _, lt = lowered or _lower(opt_docs)
    assert not lt.unsupported, lt.unsupported
    orc = RuleTableOracle(rule_table_from_policies(policies_from_docs(twin_docs)))
    res, outs, bad, touts, tbad, incomplete = _run(make(lt), lt, inputs, close)
    assert not bad and not tbad, [inputs[i]["resource"]["attr"] for i in bad[:5]]
    assert not (res.status == capi.ST_UNSUPPORTED).any()
    allowed, denied, t, named = dict.fromkeys(actions, 0), dict.fromkeys(actions, 0), 0, 0
    for i, (inp, have) in enumerate(zip(inputs, outs)):
        want = orc.check(inp, EvalParams(now_ns=NOW))
        ctx = (inp["resource"].get("attr"), inp["principal"].get("attr"))
        assert norm_actions(have) == norm_actions(want), (ctx, have["actions"], want["actions"])
        assert norm_actions(touts[i]) == norm_actions(want), ctx
        na = len(inp["actions"])
        assert bool((res.status[t:t + na] == capi.ST_CEL_ERROR).any()) == bool(want.get("evaluationErrors")), (ctx, want.get("evaluationErrors"))
        t += na
        if "errors" not in incomplete.get(i, ()):
            assert _errors(touts[i]["evaluationErrors"], {}) == _errors(want.get("evaluationErrors"), rename or {}), ctx
            named += bool(want.get("evaluationErrors"))
        for a, e in want["actions"].items():
            allowed[a] += e["effect"] == "EFFECT_ALLOW"
            denied[a] += e["effect"] != "EFFECT_ALLOW"
    assert sum(allowed[a] > 0 and denied[a] > 0 for a in actions) >= min_discriminating, (allowed, denied)
    assert named >= min_errors, named


def _twins(make, close):
    opt = {a: c for a, (c, _) in TWINS.items()}
    twin = {a: c for a, (_, c) in TWINS.items()}
    _compare_twins(make, close, _docs(opt, "opt"), _docs(twin, "opt"), list(TWINS), _inputs(TWINS), len(TWINS) - 3, 50, rename=RENAME)


def _through_proto(make, close):
    """A store lowered from the serialized RuleTable keeps its optional conditions and decides the same."""
    opt = {a: c for a, (c, _) in TWINS.items()}
    twin = {a: c for a, (_, c) in TWINS.items()}
    rt = decode_rule_table(encode_rule_table(rule_table_from_policies(policies_from_docs(_docs(opt, "opt")))))
    _compare_twins(make, close, None, _docs(twin, "opt"), list(TWINS), _inputs(TWINS, n=150, seed=761), len(TWINS) - 6, 10,
                   lowered=(rt, lower_rule_table(rt)), rename=RENAME)


def _roles_and_variables(make, close):
    """A derived role whose condition uses optional syntax, and a policy variable that holds an optional."""
    def docs(owner, lim):
        return [{"apiVersion": API, "derivedRoles": {"name": "own", "definitions": [
                    {"name": "owner", "parentRoles": ["user"], "condition": {"match": {"expr": owner}}}]}},
                {"apiVersion": API, "resourcePolicy": {"resource": "opt", "version": "default", "importDerivedRoles": ["own"],
                 "variables": {"local": {"lim": lim}},
                 "rules": [{"actions": ["view"], "derivedRoles": ["owner"], "effect": "EFFECT_ALLOW"},
                           {"actions": ["big"], "roles": ["user"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": "V.lim.orValue(0.0) > 2.0"}}},
                           {"actions": ["val"], "roles": ["user"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": "V.lim.value() != 3.5"}}}]}}]
    rng = np.random.default_rng(762)
    inputs = []
    for n in range(300):
        attr = {"owner": str(rng.choice(["p", "q"])), "x": XV[int(rng.integers(0, len(XV)))]}
        for k in ("owner", "x"):
            if rng.random() < 0.25:
                del attr[k]
        inputs.append({"requestId": "v%d" % n, "actions": ["view", "big", "val"], "principal": {"id": "p", "roles": ["user"]},
                       "resource": {"kind": "opt", "id": "v%d" % n, "attr": attr}})
    pairs = [('R.attr.?owner.orValue("") == P.id', '(has(R.attr.owner) ? R.attr.owner : "") == P.id'), ("R.attr.?x", _of("R.attr", "x"))]
    _compare_twins(make, close, docs(*[o for o, _ in pairs]), docs(*[t for _, t in pairs]), ["view", "big", "val"], inputs, 3, 10,
                   rename={t: o for o, t in pairs})


# known answers: (condition, effect when R.attr = {"x": 2.0, "m": {"k": "a"}, "xs": [1.0]}) - cel-go's results, written out
KATS = {
    "k1": ("optional.none().orValue(1) == 1", True), "k2": ("optional.of(1) == optional.of(1)", True),
    "k3": ("optional.none() == optional.none()", True), "k4": ("optional.of(1) != optional.none()", True),
    "k5": ("optional.ofNonZeroValue(0).hasValue()", False), "k6": ("optional.none().or(optional.of(2)).value() == 2", True),
    "k7": ("optional.of(3).optMap(v, v + 1).value() == 4", True), "k8": ('{"a": {"b": 1}}.?a.?c.hasValue()', False),
    "k9": ('[?optional.none(), 1, ?optional.of(2)] == [1, 2]', True), "k10": ('{?"a": optional.of(1), ?"b": optional.none()} == {"a": 1}', True),
    "r1": ("R.attr.?x.orValue(1.0) == 2.0", True), "r2": ("R.attr.?nope.orValue(1.0) == 1.0", True),
    "r3": ("R.attr.?m.?k.value() == 'a'", True), "r4": ("R.attr.?nope.k.hasValue()", False),
    "r5": ("R.attr.xs[?0] == optional.of(1.0)", True), "r6": ("R.attr.xs[?3] == optional.none()", True),
    "r7": ("R.attr.?nope.value() == 1.0", False), "r8": ("R.attr.?m.optMap(v, v.k).orValue('') == 'a'", True),
}


def _kats(make, close):
    _, lt = _lower(_docs({a: c for a, (c, _) in KATS.items()}, "opt"))
    assert not lt.unsupported, lt.unsupported
    inputs = [{"requestId": "k", "actions": list(KATS), "principal": {"id": "p", "roles": ["user"]},
               "resource": {"kind": "opt", "id": "k", "attr": {"x": 2.0, "m": {"k": "a"}, "xs": [1.0]}}}]
    res, outs, bad, touts, _, _ = _run(make(lt), lt, inputs, close)
    assert not bad and not (res.status == capi.ST_UNSUPPORTED).any()
    for a, (_, allow) in KATS.items():
        assert (outs[0]["actions"][a]["effect"] == "EFFECT_ALLOW") == allow, (a, outs[0]["actions"][a])
    assert [e["celError"]["message"] for e in touts[0]["evaluationErrors"]] == ["optional.none() dereference"], touts[0]["evaluationErrors"]


def _flagged(make, close):
    """An optional qualifier on a string, a number or null, or a list indexed by a string, is left to the caller's engine."""
    conds = {"str": "R.attr.s.?x.hasValue()", "num": 'R.attr.n[?"a"].orValue(1) == 1', "null": "R.attr.z.?x.hasValue()",
             "list_str": 'R.attr.xs[?"a"].hasValue()', "chain": "R.attr.?s.x.hasValue()", "ok": "R.attr.?s.hasValue()"}
    _, lt = _lower(_docs(conds, "opt"))
    assert not lt.unsupported, lt.unsupported
    inputs = [{"requestId": "f", "actions": list(conds), "principal": {"id": "p", "roles": ["user"]},
               "resource": {"kind": "opt", "id": "f", "attr": {"s": "text", "n": 3.0, "z": None, "xs": [1.0]}}}]
    res, _, bad, _, _, _ = _run(make(lt), lt, inputs, close)
    st = dict(zip(conds, res.status[:len(conds)]))
    assert bad == [0]
    for a in conds:
        assert (st[a] == capi.ST_UNSUPPORTED) == (a != "ok"), (a, st[a])


def _c2_twin_policies(rename=None):
    docs = workloads.c2_policies()
    for r in docs[0]["resourcePolicy"]["rules"]:
        o = workloads.C2_OPTIONAL[r["condition"]["match"]["expr"]]
        head, tail = o.split(".orValue(", 1)
        root, f = head.split(".?")
        dflt, rest = tail.split(")", 1)
        r["condition"] = {"match": {"expr": "(has(%s.%s) ? %s.%s : %s)%s" % (root, f, root, f, dflt, rest)}}
        if rename is not None:
            rename[r["condition"]["match"]["expr"]] = o
    return docs


def _c2(make, close, n=2000):
    inputs = workloads.c2_requests(n_requests=n).to_inputs()
    rename = {}
    twin = _c2_twin_policies(rename)
    _compare_twins(make, close, workloads.c2_optional_policies(), twin, workloads.C2_ACTIONS, inputs, 4, 0, rename=rename)


def test_parse_optional_syntax():
    for text in ("a.?b", "a[?1]", "[?a]", "{?'k': a}"):
        with pytest.raises(celparser.CELSyntaxError):
            celparser._Parser(text).parse()
    assert celparser.parse("a.?b") == ("optsel", ("ident", "a"), "b")
    assert celparser.parse("a[?1]") == ("optindex", ("ident", "a"), ("lit", "int", 1))
    assert celparser.parse("[?a, b]") == ("list", (("optelem", ("ident", "a")), ("ident", "b")))
    assert celparser.parse("{?'k': a}") == ("map", ((("lit", "string", "k"), ("optelem", ("ident", "a"))),))


def test_store_with_every_form_compiles():
    conds = {"a": "R.attr.?x.orValue(1) == 1", "b": "R.attr.m[?'k'].hasValue()", "c": "[?R.attr.?x, 1].size() == 1",
             "d": "{?'k': R.attr.?x}.size() == 1", "e": "R.attr.?x.optMap(v, v).hasValue()", "f": "R.attr.?x.optFlatMap(v, optional.of(v)).hasValue()",
             "g": "optional.ofNonZeroValue(R.attr.x).hasValue()", "h": "R.attr.?x.or(R.attr.?y).hasValue()"}
    _, lt = _lower(_docs(conds, "opt"))
    # non-constant optional list / map entries are flagged per tuple, the rest of the table serves
    assert sorted(t for t, _ in lt.unsupported) == sorted([conds["c"], conds["d"]]), lt.unsupported


def test_optional_residual_is_the_planners_unsupported_error():
    """A residual that keeps an optional form: the planner's "unsupported expression" error over the C ABI, not an exception."""
    import ctypes as C
    import __graft_entry__
    from test_planner_cabi import LIB, _plan
    __graft_entry__.build_lower()
    so = C.CDLL(LIB)
    so.cbl_planner_open.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_void_p)]
    so.cbl_planner_open.restype = C.c_int
    so.cbl_planner_plan_pb.argtypes = [C.c_uint64, C.c_char_p, C.c_size_t, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p)]
    so.cbl_planner_plan_pb.restype = C.c_int
    so.cbl_planner_close.argtypes = [C.c_uint64]
    so.cbl_free.argtypes = [C.c_void_p]
    rt = rule_table_from_policies(policies_from_docs(_docs({"view": "R.attr.?x.orValue(0) > 1"}, "opt")))
    pb = encode_rule_table(rt)
    h, err = C.c_uint64(), C.c_void_p()
    assert so.cbl_planner_open(pb, len(pb), C.byref(h), C.byref(err)) == 0
    try:
        st, out = _plan(so, h.value, {"requestId": "r", "principal": {"id": "p", "roles": ["user"]},
                                      "resource": {"kind": "opt"}, "actions": ["view"]}, {"nowNs": NOW})
        assert st != 0 and "unsupported expression" in out, (st, out)
    finally:
        so.cbl_planner_close(h.value)


GROUPS = [_twins, _through_proto, _roles_and_variables, _kats, _flagged, _c2]


@pytest.mark.parametrize("group", GROUPS, ids=[g.__name__.strip("_") for g in GROUPS])
def test_kernel_source_vs_oracle(group):
    from test_hostsim_golden import HostSimEvaluator
    group(lambda lt: HostSimEvaluator(lt, Conf()), False)


def test_c2_optional_is_decided_by_a_flat_kernel():
    import hostsim_api
    from test_hostsim_golden import HostSimEvaluator
    _, lt = _lower(workloads.c2_optional_policies())
    ev = HostSimEvaluator(lt, Conf())
    inputs = workloads.c2_requests(n_requests=200).to_inputs()
    ev.effective_policies(inputs, now_ns=NOW, per_input=True)
    assert hostsim_api.last_kind() == 1, "a flat kernel decides this"


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS, ids=[g.__name__.strip("_") for g in GROUPS])
def test_on_gpu(group):
    if group is _c2:
        return _c2(lambda lt: HipEvaluator(lt, Conf()), True, n=250_000)
    group(lambda lt: HipEvaluator(lt, Conf()), True)
