"""Partial evaluation of a CEL condition for the query planner: everything the request gives - principal, globals, constants, the
resource's kind / scope / the attributes the caller did supply - is evaluated, what reads the resource's unknown attributes is kept as
a RESIDUAL expression.  What the reference does with cel-go's partial evaluation and AST pruning
(internal/ruletable/planner/planner.go:370-470 evaluateConditionExpression / evalPartially / residualExpr): a known sub-expression
becomes its value; `&&` / `||` / the ternary collapse where a known operand decides them; everything else keeps its shape with its
known parts replaced by literals.  The evaluator of known parts is the lowering's constant folder (cerbos_amd/cel/fold.py)."""
from __future__ import annotations

from ..cel import fold
from ..cel.fold import FoldError, NotConst, PartialMap, Unknown, to_ast


class Ts(int):
    """google.protobuf.Timestamp: nanoseconds since the epoch"""


class Dur(int):
    """google.protobuf.Duration: nanoseconds"""


_UNITS = {"ns": 1, "us": 1000, "\u00b5s": 1000, "ms": 10**6, "s": 10**9, "m": 60 * 10**9, "h": 3600 * 10**9}


def parse_duration(text):
    """Go time.ParseDuration: a sign, then one or more <decimal number><unit> groups"""
    import re
    m = re.fullmatch(r"([+-])?((?:\d*\.?\d*(?:ns|us|\u00b5s|ms|s|m|h))+)", text)
    if not m or not text.strip("+-"):
        raise FoldError("invalid duration")
    total = 0
    for num, unit in re.findall(r"(\d*\.?\d*)(ns|us|\u00b5s|ms|s|m|h)", m.group(2)):
        if num in ("", "."):
            raise FoldError("invalid duration")
        total += int(round(float(num) * _UNITS[unit]))
    return Dur(-total if m.group(1) == "-" else total)


def parse_timestamp(text):
    import re
    from datetime import datetime, timedelta, timezone
    m = re.fullmatch(r"(\d{4})-(\d\d)-(\d\d)T(\d\d):(\d\d):(\d\d)(\.\d+)?(Z|[+-]\d\d:\d\d)", text, re.ASCII)
    if not m:
        raise FoldError("invalid timestamp")
    y, mo, d, h, mi, sec = (int(m.group(i)) for i in range(1, 7))
    frac = int(((m.group(7) or ".0")[1:] + "000000000")[:9])
    tz = m.group(8)
    off = 0
    if tz != "Z":
        off = (int(tz[1:3]) * 60 + int(tz[4:6])) * (1 if tz[0] == "+" else -1)
    try:
        base = datetime(y, mo, d, h, mi, sec, tzinfo=timezone.utc) - timedelta(minutes=off)
    except ValueError:
        raise FoldError("invalid timestamp")
    return Ts(int((base - datetime(1970, 1, 1, tzinfo=timezone.utc)).total_seconds()) * 10**9 + frac)


def format_duration(d):
    sec, ns = divmod(abs(int(d)), 10**9)
    body = "%d" % sec if ns == 0 else ("%d.%09d" % (sec, ns)).rstrip("0")
    return ("-" if d < 0 else "") + body + "s"


def format_timestamp(t):
    from datetime import datetime, timezone
    sec, ns = divmod(int(t), 10**9)
    base = datetime.fromtimestamp(sec, tz=timezone.utc).strftime("%Y-%m-%dT%H:%M:%S")
    frac = ("." + ("%09d" % ns).rstrip("0")) if ns else ""
    return base + frac + "Z"


_DUR_MIN, _DUR_MAX = -(1 << 63), (1 << 63) - 1


def time_since(now_ns, ts):
    """conditions/cerbos_lib.go timeSince: now.Sub(ts), and Go's Time.Sub saturates at the largest and smallest Duration"""
    return Dur(max(_DUR_MIN, min(_DUR_MAX, now_ns - ts)))


class _Eval(fold._Eval):
    """The constant folder plus what only a request has: the call's clock, timestamps and durations (conditions/cerbos_lib.go now /
    timeSince; cel-go's timestamp / duration conversions and arithmetic)."""

    def __init__(self, now_ns):
        super().__init__()
        self.now_ns = now_ns

    def call(self, n, env):
        _, name, target, args = n
        if target is None:
            if name == "now" and not args and self.now_ns is not None:
                return Ts(self.now_ns)
            if name in ("timestamp", "duration", "timeSince") and len(args) == 1:
                v = self.ev(args[0], env)
                if name == "timestamp":
                    return v if isinstance(v, Ts) else parse_timestamp(fold._need(v, str))
                if name == "duration":
                    return v if isinstance(v, Dur) else parse_duration(fold._need(v, str))
                if self.now_ns is None:
                    raise NotConst("now")
                return time_since(self.now_ns, fold._need(v, Ts))
        elif name == "timeSince" and not args and self.now_ns is not None:
            return time_since(self.now_ns, fold._need(self.ev(target, env), Ts))
        return super().call(n, env)

    def binop(self, op, a, b):
        ta, tb = isinstance(a, (Ts, Dur)), isinstance(b, (Ts, Dur))
        if ta or tb:
            if op in ("==", "!="):
                eq = type(a) is type(b) and int(a) == int(b)
                return eq if op == "==" else not eq
            if type(a) is type(b) and op in ("<", "<=", ">", ">="):
                x, y = int(a), int(b)
                return {"<": x < y, "<=": x <= y, ">": x > y, ">=": x >= y}[op]
            if op == "+" and isinstance(a, Ts) and isinstance(b, Dur) or op == "+" and isinstance(a, Dur) and isinstance(b, Ts):
                return Ts(int(a) + int(b))
            if op == "+" and isinstance(a, Dur) and isinstance(b, Dur):
                return Dur(int(a) + int(b))
            if op == "-" and isinstance(a, Ts) and isinstance(b, Ts):
                return Dur(int(a) - int(b))
            if op == "-" and isinstance(a, Ts) and isinstance(b, Dur):
                return Ts(int(a) - int(b))
            if op == "-" and isinstance(a, Dur) and isinstance(b, Dur):
                return Dur(int(a) - int(b))
            if op == "in" and isinstance(b, list):
                return any(type(a) is type(x) and int(a) == int(x) for x in b)
            raise FoldError("no such overload")
        return super().binop(op, a, b)


def value_ast(v):
    """A value as the residual expression shows it (fold.to_ast; a timestamp / duration as the conversion call that makes it)."""
    if isinstance(v, Dur):
        return ("call", "duration", None, (("lit", "string", format_duration(v)),))
    if isinstance(v, Ts):
        return ("call", "timestamp", None, (("lit", "string", format_timestamp(v)),))
    if isinstance(v, list):
        elems = [value_ast(x) for x in v]
        return None if any(e is None for e in elems) else ("list", tuple(elems))
    if isinstance(v, dict) and any(isinstance(x, (Ts, Dur, list, dict)) for x in v.values()):
        ents = []
        for k, x in v.items():
            e = value_ast(x)
            if e is None or not isinstance(k, str):
                return None
            ents.append((("lit", "string", k), e))
        return ("map", tuple(ents))
    return to_ast(v)


def _right_nested(op, opts):
    """mkLogicalOr / mkLogicalAnd (struct_matcher.go:214-236): a op (b op (c ...))"""
    out = opts[-1]
    for o in reversed(opts[:-1]):
        out = (op, o, out)
    return out


class CelEvalError(Exception):
    """A known (sub-)expression fails to evaluate: the condition is false, its error reported (planner.go:404-413)."""


_ABBREV = {"R": ("request", "resource"), "P": ("request", "principal"), "G": ("globals",), "C": ("constants",), "V": ("variables",)}


def to_cel(v, partial_paths=()):
    """JSON-shaped value -> the folder's values (numbers are doubles: structpb)."""
    if isinstance(v, bool) or v is None or isinstance(v, str):
        return v
    if isinstance(v, (int, float)):
        return float(v)
    if isinstance(v, list):
        return [to_cel(x) for x in v]
    if isinstance(v, dict):
        return {str(k): to_cel(x) for k, x in v.items()}
    raise TypeError(type(v).__name__)


def request_env(principal, resource, aux_data, globals_, constants):
    """The identifiers a condition can read (conditions/cel.go:30-63): request / R / P / G / C and their long names."""
    from .. import namer
    p = {"id": principal.get("id", ""), "roles": list(principal.get("roles") or []), "attr": to_cel(principal.get("attr") or {}),
         "policyVersion": principal.get("policyVersion", ""), "scope": namer.scope_value(principal.get("scope", "") or "")}
    p["policy_version"] = p["policyVersion"]
    # of the resource the partial evaluator knows kind, scope and the attributes the caller supplied (planner.go:532-577 newEvaluator);
    # id and policyVersion stay residual
    r = PartialMap({"kind": resource.get("kind", ""), "scope": namer.scope_value(resource.get("scope", "") or ""),
                    "attr": PartialMap(to_cel(resource.get("attr") or {}))})
    aux = aux_data or {}
    req = {"principal": p, "resource": r,
           "auxData": {"jwt": to_cel(aux.get("jwt") or {}), "jwts": {k: {"claims": to_cel((v or {}).get("claims") or {})} for k, v in (aux.get("jwts") or {}).items()}}}
    req["aux_data"] = req["auxData"]
    g, c = to_cel(globals_ or {}), to_cel_consts(constants or {})
    return {"request": req, "R": r, "P": p, "G": g, "globals": g, "C": c, "constants": c}


def to_cel_consts(consts):
    return to_cel(consts)


def substitute(n, repl):
    """Replace sub-trees: `repl(node)` -> a tree, or None to descend."""
    r = repl(n)
    if r is not None:
        return r
    kids = fold._children(n)
    if not kids:
        return n
    return fold._rebuild(n, [substitute(c, repl) for c in kids])


def inline_variables(n, variables):
    """V.x / variables.x -> the variable's expression (planner ast.go:235-254 replaceVars); a name a comprehension binds shadows nothing
    here: variables are selected from V / variables."""
    def repl(x):
        if x[0] == "select" and x[1][0] == "ident" and x[1][1] in ("V", "variables") and x[2] in variables:
            return variables[x[2]]
        return None
    return substitute(n, repl)


class Partial:
    def __init__(self, env, now_ns=None):
        self.env = env
        self.now_ns = now_ns

    # -> ("k", value) | ("r", ast)
    def pe(self, n, env=None):   # noqa: C901
        env = self.env if env is None else env
        k = n[0]
        if k == "lit":
            return ("k", _Eval(self.now_ns).ev(n, env))
        if k in ("and", "or"):
            # operand by operand: a deciding operand absorbs the other's error (false && error = false), which the constant
            # folder - written for the lowering, where such a node is left to the device - does not do
            return self._logical(n, env)
        try:
            v = _Eval(self.now_ns).ev(n, env)
            if isinstance(v, PartialMap):
                return ("r", n)      # the request's partly known parts stay paths
            return ("k", v)
        except Unknown:
            pass
        except NotConst:
            pass
        except FoldError as e:
            if not self._reads_unknown(n, env):
                raise CelEvalError(str(e))
        except (RecursionError, OverflowError, ValueError) as e:
            raise CelEvalError(str(e))
        # structural
        if k == "not":
            a = self.pe(n[1], env)
            if a[0] == "k":
                if not isinstance(a[1], bool):
                    raise CelEvalError("no such overload")
                return ("k", not a[1])
            return ("r", ("not", a[1]))
        if k == "tern":
            c = self.pe(n[1], env)
            if c[0] == "k":
                if not isinstance(c[1], bool):
                    raise CelEvalError("no such overload")
                return self.pe(n[2] if c[1] else n[3], env)
            return ("r", ("tern", c[1], self.ast(self.pe(n[2], env), n[2], env), self.ast(self.pe(n[3], env), n[3], env)))
        if k == "bind":
            init = self.pe(n[2], env)
            if init[0] == "k":
                return self.pe(n[3], dict(env, **{n[1]: init[1]}))
            body = substitute(n[3], lambda x: init[1] if x == ("ident", n[1]) else None)
            return self.pe(body, env)
        if k == "comp":
            return self.comp(n, env)
        if k == "ident":
            return ("r", n)
        kids = fold._children(n)
        if k == "call" and n[2] is not None and n[2][0] == "ident" and n[2][1] not in env and n[2][1] in (
                "sets", "math", "lists", "base64", "strings", "regex", "optional", "ip", "cidr"):
            new = [n[2]] + [self.ast(self.pe(c, env), c, env) for c in kids[1:]]     # a namespace, not a value
        else:
            new = [self.ast(self.pe(c, env), c, env) for c in kids]
        return ("r", fold._rebuild(n, new))

    def _logical(self, n, env):
        k = n[0]
        a, b = self.pe_guard(n[1], env), self.pe_guard(n[2], env)
        absorbing = (k == "or")
        for x, other in ((a, b), (b, a)):
            if x[0] == "k" and isinstance(x[1], bool):
                if x[1] == absorbing:
                    return ("k", absorbing)
                if other[0] == "k" and not isinstance(other[1], bool):
                    raise CelEvalError("no such overload")
                return other if other[0] != "e" else self._raise(other)
        if a[0] == "e" and b[0] == "e":
            self._raise(a)
        if (a[0] == "k" or b[0] == "k") and a[0] != "r" and b[0] != "r":
            # a known operand that is not a bool beside another known operand or an error: no such overload.  Beside an
            # UNKNOWN one the unknown outranks it as it outranks any error (evalAnd / evalOr): the residual below carries the
            # non-bool operand as its literal, as the pruner does (`P.attr.num && R.attr.flag` with P.attr.num = 1 plans `1 && R.attr.flag`)
            raise CelEvalError("no such overload")
        # an error beside an unknown: cel-go answers unknown (interpretable.go evalAnd / evalOr: an unknown operand outranks an
        # error), and the pruner has no value to put in the failing operand's place - the residual keeps it as written
        # (`R.attr.a && P.attr.missing`).  Dropping it would make an `&&` filter wider than Check, where true && error is an error.
        if a[0] == "e":
            a = ("r", n[1])
        if b[0] == "e":
            b = ("r", n[2])
        return ("r", (k, self.ast(a, n[1], env), self.ast(b, n[2], env)))

    def pe_guard(self, n, env):
        try:
            return self.pe(n, env)
        except CelEvalError as e:
            return ("e", e)

    @staticmethod
    def _raise(x):
        raise x[1]

    def ast(self, x, orig=None, env=None):
        """A result as an expression: a residual as it is, a value as its literal - or, for a value without one (a hierarchy, an
        address), the expression that makes it, its own operands evaluated."""
        if x[0] == "r":
            return x[1]
        lit = value_ast(x[1])
        if lit is not None:
            return lit
        if orig is None or not fold._children(orig):
            raise CelEvalError("a value without a literal form in a residual expression")
        env = self.env if env is None else env
        kids = fold._children(orig)
        if orig[0] == "call" and orig[2] is not None and orig[2][0] == "ident" and orig[2][1] not in env:
            new = [orig[2]] + [self.ast(self.pe(c, env), c, env) for c in kids[1:]]
        else:
            new = [self.ast(self.pe(c, env), c, env) for c in kids]
        return fold._rebuild(orig, new)

    def _reads_unknown(self, n, env):
        """Does the expression touch an unknown part of the request?  (An evaluation error in a sub-expression that does not is the
        condition's; one that does may only be the evaluator giving up on a partial value.)"""
        if n[0] in ("select", "index", "has"):
            try:
                _Eval(self.now_ns).ev(n, env)
            except Unknown:
                return True
            except Exception:
                pass
        return any(self._reads_unknown(c, env) for c in fold._children(n))

    # ---- what the reference does to the ROOT of a residual expression (planner.go:415-438 evaluateUnknown; struct_matcher.go)
    def process_root(self, n, env=None):
        env = self.env if env is None else env
        out = self._struct_index(n) or self._in_struct_index(n) or self._unroll(n, env)
        if out is None:
            return ("r", n)
        return self.pe(out, env)

    @staticmethod
    def _known_only(n):
        if n[0] == "lit":
            return True
        if n[0] == "list":
            return all(Partial._known_only(e) for e in n[1])
        if n[0] == "map":
            return all(Partial._known_only(a) and Partial._known_only(b) for a, b in n[1])
        return False

    @staticmethod
    def _indexed_struct(n):
        """struct[indexer] or struct[indexer].field with `struct` a map literal and `indexer` a selection -> (map, indexer, field)"""
        field = None
        if n[0] == "select":
            field, n = n[2], n[1]
        if n[0] == "index" and n[1][0] == "map" and n[2][0] == "select":
            return n[1], n[2], field
        return None

    @staticmethod
    def _options(m, mk):
        ents = list(m[1])
        if all(k[0] == "lit" and k[1] == "string" for k, _ in ents):
            ents.sort(key=lambda kv: kv[0][2])
        opts = [mk(k, v) for k, v in ents]
        if not opts:
            return None
        return _right_nested("or", opts)

    def _struct_index(self, n):
        """{..}[R.attr.x](.f) <op> const -> OR over the entries of (R.attr.x == key && const <op> value(.f))  (struct_matcher.go:128-170)"""
        if n[0] != "bin" or n[1] not in ("==", "!=", "<", "<=", ">", ">=") or n[3][0] != "lit":
            return None
        hit = self._indexed_struct(n[2])
        if hit is None:
            return None
        m, indexer, field = hit
        return self._options(m, lambda k, v: ("and", ("bin", "==", indexer, k), ("bin", n[1], n[3], ("select", v, field) if field else v)))

    def _in_struct_index(self, n):
        """const in {..}[R.attr.x](.f)"""
        if n[0] != "bin" or n[1] != "in" or n[2][0] != "lit":
            return None
        hit = self._indexed_struct(n[3])
        if hit is None:
            return None
        m, indexer, field = hit
        return self._options(m, lambda k, v: ("and", ("bin", "==", indexer, k), ("bin", "in", n[2], ("select", v, field) if field else v)))

    def _unroll(self, n, env):
        """exists / all over a known list or map of at most ten entries: one residual per entry, OR-ed / AND-ed (struct_matcher.go:300-390)"""
        if n[0] != "comp" or n[1] not in ("exists", "all") or n[2][0] not in ("list", "map") or not self._known_only(n[2]):
            return None
        _, kind, target, vars_, args = n
        items = list(target[1])
        if len(items) > 10:
            return None
        opts = []
        for i, it in enumerate(items):
            e = dict(env)
            if target[0] == "list":
                v = _Eval(self.now_ns).ev(it, env)
                if len(vars_) == 2:
                    e[vars_[0]], e[vars_[1]] = i, v
                else:
                    e[vars_[0]] = v
            else:
                e[vars_[0]] = _Eval(self.now_ns).ev(it[0], env)
                if len(vars_) == 2:
                    e[vars_[1]] = _Eval(self.now_ns).ev(it[1], env)
            opts.append(self.ast(self.pe(args[0], e)))
        if not opts:
            return None
        return _right_nested("or" if kind == "exists" else "and", opts)

    def comp(self, n, env):
        """A comprehension over an unknown range stays a comprehension: its range and its body partially evaluated with the iteration
        variables unknown (planner.go:598-650 evalComprehensionBody)."""
        _, kind, target, vars_, args = n
        rng = self.pe(target, env)
        inner = {k: v for k, v in env.items() if k not in vars_}
        new_args = tuple(self.ast(self.pe(a, inner), a, inner) for a in args)
        return ("r", ("comp", kind, self.ast(rng, target, env), vars_, new_args))
