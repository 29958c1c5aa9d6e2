"""cel-go ext.Math, s.split(sep[, n]) and cel.bind on values the request supplies, against the oracle over generated inputs:

* every Math function on int, uint and double operands (JSON numbers arrive as doubles: int() / uint() reach the other two),
  NaN and the infinities made in the expression, INT64_MIN, shift offsets -1, 0, 63, 64, strings and missing attributes where
  numbers belong; greatest / least over a request list, an arena list and mixed scalar arguments; Math on comprehension locals;
* split with and without a limit, with an empty separator, on non-ASCII text, followed by indexing, size, `in` and
  comprehensions; the JWT recipe (docs/modules/recipes/pages/jwt-claims.adoc) verbatim;
* cel.bind nested, holding a split list, inside a comprehension body; a derived role and a policy variable that use Math.

Per action: effect; per request: whether evaluation errors were recorded, and - through the trace pass - which.  No tuple is left
to the caller's engine except the splits built to overflow the lane's arena, which must be.  CPU tier: the kernel source on the host
simulator; GPU tier: the kernel."""
import numpy as np
import pytest

from cerbos_amd import capi
from cerbos_amd.engine import Conf, HipEvaluator
from cerbos_amd.flatten import Flattener
from cerbos_amd.lower.blob import lower_rule_table
from cerbos_amd.policy.loader import policies_from_docs
from cerbos_amd.ruletable.build import rule_table_from_policies
from helpers import norm_actions
from oracle.check import EvalParams, RuleTableOracle

API = "api.cerbos.dev/v1"
NOW = 1_700_000_000_000_000_000
X, I, U, K, Q = "R.attr.x", "int(R.attr.i)", "uint(R.attr.u)", "int(R.attr.k)", "(R.attr.a / R.attr.b)"
MATH_CONDS = {
    "abs": "math.abs(%s) < 10.0" % X, "abs_int": "math.abs(%s) > 3" % I, "abs_min": "math.abs(%s * 2) > 0" % I,
    "abs_uint": "math.abs(%s) == %s" % (U, U),
    "sign": "math.sign(%s) == -1.0" % X, "sign_int": "math.sign(%s) >= 0" % I, "sign_uint": "math.sign(%s) == 1u" % U,
    "ceil": "math.ceil(%s) == 3.0" % X, "floor": "math.floor(%s) <= -1.0" % X, "round": "math.round(%s) == R.attr.y" % X,
    "trunc": "math.trunc(%s) == R.attr.y" % X, "round_int": "math.round(%s) == 1.0" % I,
    "sqrt": "math.sqrt(%s) < 2.0" % X, "sqrt_int": "math.sqrt(%s) >= 1.5" % I, "sqrt_uint": "math.sqrt(%s) > 2.0" % U,
    "nan": "math.isNaN(%s)" % Q, "inf": "math.isInf(%s)" % Q, "finite": "math.isFinite(%s)" % Q,
    "round_nan": "math.isNaN(math.round(%s)) || math.isInf(math.ceil(%s))" % (Q, Q), "floor_q": "math.floor(%s) < 0.0" % Q,
    "bitand": "math.bitAnd(%s, int(R.attr.j)) == 2" % I, "bitor_u": "math.bitOr(%s, 5u) > 6u" % U,
    "bitxor": "math.bitXor(%s, int(R.attr.j)) < 0" % I, "bitnot": "math.bitNot(%s) == -1 - %s" % (I, I),
    "bitnot_u": "math.bitNot(%s) > 100u" % U, "bit_mixed": "math.bitAnd(%s, %s) == 0" % (I, U),
    "shl": "math.bitShiftLeft(%s, %s) > 100" % (I, K), "shr": "math.bitShiftRight(%s, %s) > 100" % (I, K),
    "shl_u": "math.bitShiftLeft(%s, %s) == 0u" % (U, K), "shr_u": "math.bitShiftRight(%s, %s) >= 2u" % (U, K),
    "greatest_list": "math.greatest(R.attr.xs) > 5.0", "least_list": "math.least(R.attr.xs) < 0.0",
    "greatest_arena": "math.greatest(R.attr.xs.map(v, v * 2.0)) > 10.0", "least_arena": "math.least(R.attr.xs.filter(v, v > 0.0)) < 2.0",
    "greatest_args": "math.greatest(%s, %s, 2u) > 3" % (X, I), "least_args": "math.least(%s, R.attr.y) <= -2.5" % I,
    "least_one": "math.least(%s) == %s" % (X, X), "greatest_nan": "math.greatest(%s, %s) > 0.0" % (Q, X),
    "least_nan": "math.least(%s, %s) < 0.0" % (X, Q),
    "all_abs": "R.attr.xs.all(v, math.abs(v) < 10.0)", "exists_floor": "R.attr.xs.exists(v, math.floor(v) == v)",
}
SPLIT_CONDS = {
    "first": 'R.attr.s.split(",")[0] == R.attr.t', "size": "size(R.attr.s.split(R.attr.sep)) == 3",
    "in": 'R.attr.t in R.attr.s.split(" ")', "lim_exists": 'R.attr.s.split(",", int(R.attr.n)).exists(p, p == R.attr.t)',
    "lim_size": "size(R.attr.s.split(R.attr.sep, int(R.attr.n))) >= 2", "empty_sep": 'R.attr.s.split("")[1] == "é"',
    "empty_sep_lim": 'size(R.attr.s.split("", int(R.attr.n))) == 2', "rest": 'R.attr.s.split(",", 2)[1].contains(",")',
    "starts": 'R.attr.s.split(",").exists(p, p.startsWith("é"))', "filter": 'size(R.attr.s.split(",").filter(p, p != "")) == 1',
    "rope_in": 'R.attr.t.substring(0) in R.attr.s.split(",")', "piece_size": 'size(R.attr.s.split(",")[0]) == 2',
    "all_in": 'R.attr.s.split(",").all(p, p in ["a", "b", "é"])', "sep_attr": 'R.attr.s.split(R.attr.sep).exists(p, p == "")',
    "exists_one": 'R.attr.s.split(",").exists_one(p, p == "日")', "last": 'R.attr.s.split(",", -1)[size(R.attr.s.split(","))-1] == "a"',
}
BIND_CONDS = {
    "bind_math": "cel.bind(d, math.abs(R.attr.x - R.attr.y), d > 1.0 && d < 5.0)",
    "bind_nested": "cel.bind(a, R.attr.x * 2.0, cel.bind(b, a + R.attr.y, b > a))",
    "bind_split": 'cel.bind(parts, R.attr.s.split(","), size(parts) == 2 && parts[1] == R.attr.t)',
    "bind_in_comp": "R.attr.xs.exists(v, cel.bind(w, math.round(v), w == 3.0 || w == -3.0))",
    "bind_error": "cel.bind(z, R.attr.missing, true)",
    "bind_unused_false": "cel.bind(z, R.attr.x, false) || R.attr.y > 0.0",
}
JWT_CONDS = {"jwt_scope": '"read:documents" in request.auxData.jwt.scope.split(" ")'}
XS = [1.0, -2.5, 2.5, 0.5, 7.0, -0.5, 3.0, 12.0, 9.5]
XVALS = [0.5, -0.5, 1.5, 2.5, -2.5, 0.49999999999999994, -0.49999999999999994, 4503599627370497.0, -4503599627370497.0,
         9007199254740993.0, 1e300, -1e300, -0.0, 0.0, 2.0000000000000004, 3.7, -3.2, 9.99, 10.0, -10.0, 4.0, 3.999]
IVALS = [0.0, 1.0, -1.0, 2.0, 3.0, -3.0, 6.0, 7.0, -8.0, 1024.0, -4611686018427387904.0, 4611686018427387903.0, 9e18, -9e18]
KVALS = [-1.0, 0.0, 1.0, 3.0, 63.0, 64.0, 65.0, 200.0, -2.0]


def _go_round(d):
    import math
    t = float(math.trunc(d))
    if abs(d - t) >= 0.5:
        t += math.copysign(1.0, d)
    return math.copysign(t, d)


def _docs(conds, kind):
    return [{"apiVersion": API, "resourcePolicy": {"resource": kind, "version": "default", "rules": [
        {"actions": [n], "roles": ["*"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": e}}} for n, e in conds.items()]}}]


def _math_inputs():
    rng = np.random.default_rng(750)
    inputs = []
    for n in range(700):
        x = float(rng.choice(XVALS)) if rng.random() < 0.5 else float(np.round(rng.uniform(-12, 12), 2))
        y = _go_round(x) if rng.random() < 0.3 else (float(np.trunc(x)) if rng.random() < 0.3 else float(rng.choice(XVALS)))
        attr = {"x": x, "y": y, "i": float(rng.choice(IVALS)) if rng.random() < 0.6 else float(rng.integers(-20, 21)),
                "j": float(rng.integers(-8, 9)), "u": float(rng.choice([0.0, 1.0, 2.0, 5.0, 7.0, 255.0, -1.0, 1e19])),
                "k": float(rng.choice(KVALS)), "a": float(rng.choice([0.0, 1.0, -1.0, 3.0])), "b": float(rng.choice([0.0, 0.0, 2.0])),
                "xs": [float(v) for v in rng.choice(XS, size=int(rng.integers(0, 5)))]}
        r = rng.random()
        if r < 0.04:
            attr["x"] = "3"
        elif r < 0.07:
            attr["xs"] = ["a", 1.0]
        elif r < 0.10:
            del attr[str(rng.choice(["x", "i", "xs", "k", "u", "b"]))]
        elif r < 0.12:
            attr["i"] = 2.5
        inputs.append({"requestId": "m%d" % n, "actions": list(MATH_CONDS), "principal": {"id": "p", "roles": ["user"]},
                       "resource": {"kind": "num", "id": "n%d" % n, "attr": attr}})
    return inputs


def _split_inputs(actions, kind="text"):
    rng = np.random.default_rng(751)
    pieces = ["a", "b", "é", "日", ",", " ", ",,", "ab", "a,b", "", "x y"]
    inputs = []
    for n in range(600):
        s = "".join(str(rng.choice(pieces)) for _ in range(int(rng.integers(0, 6))))
        attr = {"s": s, "sep": str(rng.choice([",", " ", "", "é", ",,", "b"])), "n": float(rng.choice([-1, 0, 1, 2, 3, 5])),
                "t": str(rng.choice(["a", "b", "é", "日", "", "ab", "x"])), "x": float(rng.choice(XVALS)), "y": float(rng.choice(XVALS)),
                "xs": [float(v) for v in rng.choice(XS, size=int(rng.integers(0, 4)))]}
        r = rng.random()
        if r < 0.04:
            attr["s"] = 7.0
        elif r < 0.06:
            attr["sep"] = 1.0
        elif r < 0.08:
            del attr["s"]
        elif r < 0.10:
            attr["n"] = 1.5
        inputs.append({"requestId": "s%d" % n, "actions": list(actions), "principal": {"id": "p", "roles": ["user"]},
                       "resource": {"kind": kind, "id": "t%d" % n, "attr": attr}})
    return inputs


def _jwt_inputs():
    scopes = ["read:documents", "read:documents write:documents", "write:documents", "", "read:documents  admin", "read:documentsx",
              " read:documents", "ré:documents read:documents", None, 3.0]
    out = []
    for n, sc in enumerate(scopes):
        jwt = {} if sc is None else {"scope": sc}
        out.append({"requestId": "j%d" % n, "actions": list(JWT_CONDS), "principal": {"id": "p", "roles": ["user"]},
                    "resource": {"kind": "doc", "id": "d%d" % n, "attr": {}}, "auxData": {"jwt": jwt}})
    return out


def _run(make, close, lt, inputs):
    ev = make(lt)
    try:
        batch = Flattener(lt).flatten(inputs)
        res = ev.table.check(batch, now_ns=NOW, flags=0)
        outs, bad = ev.assemble(inputs, batch, res, "default", allow_unsupported=True)
        touts, tbad, incomplete = ev.check(inputs, now_ns=NOW, allow_unsupported=True, trace=True)
    finally:
        if close:
            ev.close()
    return res, outs, bad, touts, tbad, incomplete


def _compare(make, close, docs, actions, inputs, min_discriminating, min_errors=1):
    rt = rule_table_from_policies(policies_from_docs(docs))
    lt = lower_rule_table(rt)
    assert not lt.unsupported, lt.unsupported
    res, outs, bad, touts, tbad, incomplete = _run(make, close, lt, inputs)
    assert not bad and not tbad, [inputs[i]["resource"]["attr"] for i in bad[:5]]
    assert not (res.status == capi.ST_UNSUPPORTED).any()
    orc = RuleTableOracle(rt)
    allowed, denied, t, named = dict.fromkeys(actions, 0), dict.fromkeys(actions, 0), 0, 0
    for i, (inp, have) in enumerate(zip(inputs, outs)):
        want = orc.check(inp, EvalParams(now_ns=NOW))
        ctx = (inp["resource"].get("attr"), inp.get("auxData"))
        assert norm_actions(have) == norm_actions(want), (ctx, have["actions"], want["actions"])
        assert norm_actions(touts[i]) == norm_actions(want), ctx
        na = len(inp["actions"])
        assert bool((res.status[t:t + na] == capi.ST_CEL_ERROR).any()) == bool(want.get("evaluationErrors")), (ctx, want.get("evaluationErrors"))
        t += na
        if "errors" not in incomplete.get(i, ()):
            assert sorted(map(str, touts[i]["evaluationErrors"])) == sorted(map(str, want.get("evaluationErrors") or [])), ctx
            named += bool(want.get("evaluationErrors"))
        for a, e in want["actions"].items():
            allowed[a] += e["effect"] == "EFFECT_ALLOW"
            denied[a] += e["effect"] != "EFFECT_ALLOW"
    assert sum(allowed[a] > 0 and denied[a] > 0 for a in actions) >= min_discriminating, (allowed, denied)
    assert named >= min_errors, named
    return lt


def _math(make, close):
    _compare(make, close, _docs(MATH_CONDS, "num"), MATH_CONDS, _math_inputs(), len(MATH_CONDS) - 2, 50)


def _split(make, close):
    _compare(make, close, _docs(SPLIT_CONDS, "text"), SPLIT_CONDS, _split_inputs(SPLIT_CONDS), len(SPLIT_CONDS) - 1, 10)


def _bind(make, close):
    _compare(make, close, _docs(BIND_CONDS, "text"), BIND_CONDS, _split_inputs(BIND_CONDS), len(BIND_CONDS) - 1, 10)


def _jwt(make, close):
    _compare(make, close, _docs(JWT_CONDS, "doc"), JWT_CONDS, _jwt_inputs(), 1, 0)


def _roles_and_variables(make, close):
    """A derived role whose condition uses Math, a policy variable that does, and the negative shift offset's error named."""
    docs = [{"apiVersion": API, "derivedRoles": {"name": "near", "definitions": [
                {"name": "close_by", "parentRoles": ["user"], "condition": {"match": {"expr": "math.abs(R.attr.x - P.attr.x) <= 2.0"}}}]}},
            {"apiVersion": API, "resourcePolicy": {"resource": "spot", "version": "default", "importDerivedRoles": ["near"],
             "variables": {"local": {"lim": "math.greatest(R.attr.xs)", "sh": "math.bitShiftLeft(1, int(R.attr.k))"}},
             "rules": [{"actions": ["view"], "derivedRoles": ["close_by"], "effect": "EFFECT_ALLOW"},
                       {"actions": ["big"], "roles": ["user"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": "V.lim >= 5.0"}}},
                       {"actions": ["shift"], "roles": ["user"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": "V.sh > 4"}}}]}}]
    rng = np.random.default_rng(752)
    inputs = []
    for n in range(300):
        attr = {"x": float(rng.choice(XVALS)), "xs": [float(v) for v in rng.choice(XS, size=int(rng.integers(0, 4)))],
                "k": float(rng.choice(KVALS + [-5.0]))}
        if rng.random() < 0.05:
            del attr["x"]
        inputs.append({"requestId": "v%d" % n, "actions": ["view", "big", "shift"],
                       "principal": {"id": "p", "roles": ["user"], "attr": {"x": float(rng.choice(XVALS))}},
                       "resource": {"kind": "spot", "id": "v%d" % n, "attr": attr}})
    _compare(make, close, docs, ["view", "big", "shift"], inputs, 3, 10)


def _arena_overflow(make, close):
    """Splits whose pieces the lane's arena cannot hold are flagged for the caller's engine, never answered; the rest decide."""
    conds = {"count": 'size(R.attr.s.split(",")) > 3', "member": '"z" in R.attr.s.split(",")'}
    rt = rule_table_from_policies(policies_from_docs(_docs(conds, "text")))
    lt = lower_rule_table(rt)
    assert not lt.unsupported, lt.unsupported
    sizes = [0, 1, 5, 23, 24, 25, 40]
    inputs = [{"requestId": "o%d" % k, "actions": list(conds), "principal": {"id": "p", "roles": ["user"]},
               "resource": {"kind": "text", "id": "o%d" % k, "attr": {"s": ",".join(["a"] * k + ["z"])}}} for k in sizes]
    res, outs, bad, _, _, _ = _run(make, close, lt, inputs)
    orc = RuleTableOracle(rt)
    for r, (k, inp) in enumerate(zip(sizes, inputs)):
        st = res.status[2 * r:2 * r + 2]
        if k + 1 > 24:   # two arena entries per piece, 48 entries
            assert (st == capi.ST_UNSUPPORTED).all() and r in bad, (k, st)
        else:
            assert not (st == capi.ST_UNSUPPORTED).any() and r not in bad, (k, st)
            assert norm_actions(outs[r]) == norm_actions(orc.check(inp, EvalParams(now_ns=NOW))), k


GROUPS = [_math, _split, _bind, _jwt, _roles_and_variables, _arena_overflow]


@pytest.mark.parametrize("group", GROUPS, ids=[g.__name__.strip("_") for g in GROUPS])
def test_kernel_source_vs_oracle(group):
    from test_hostsim_golden import HostSimEvaluator
    group(lambda lt: HostSimEvaluator(lt, Conf()), False)


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS, ids=[g.__name__.strip("_") for g in GROUPS])
def test_on_gpu(group):
    group(lambda lt: HipEvaluator(lt, Conf()), True)
