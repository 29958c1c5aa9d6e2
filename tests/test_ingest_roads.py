"""CPU tier: the roads through libcerbos_ingest.so that share one rule each - the action fold, the part split, the
assembler's write bound and the refusals the Go integration surfaces.  Results are made up in numpy (no device, no
simulator): what is pinned is the host code between the bytes and the arrays."""
import copy

import numpy as np
import pytest

from cerbos_amd import capi, wire
from cerbos_amd.engine import Conf
from cerbos_amd.ingest import IngestError, IngestTable, load, trace_pb
from cerbos_amd.lower.blob import lower_rule_table
from helpers import long_key_inputs, store_rule_table
from test_hostsim_golden import GLOBALS, HostSimEvaluator
from test_ingest import ARRAYS, _request_of

EFFECT_NUM = {"EFFECT_ALLOW": 1, "EFFECT_DENY": 2}
A, D = capi.EFFECT_ALLOW, capi.EFFECT_DENY
OUT_FLAG = {capi.ST_OK: 0, capi.ST_CEL_ERROR: 2, capi.ST_UNSUPPORTED: 1, capi.ST_WANTS_TRACE: 16}   # CBI_OUT_* of cerbos_ingest.h


@pytest.fixture(scope="module")
def lt():
    return lower_rule_table(store_rule_table(), GLOBALS)


def encode_check_output(o):
    """engine.proto CheckOutput: 1 request_id, 2 resource_id, 3 actions map<string, ActionEffect{1 effect, 2 policy, 3 scope}>,
    4 effective_derived_roles - the bytes the Python assembler's dict stands for, entries in first-appearance order."""
    out = wire._string(1, o["requestId"]) + wire._string(2, o["resourceId"])
    for name, e in o["actions"].items():
        eff = wire._varint(1 << 3 | 0) + wire._varint(EFFECT_NUM[e["effect"]])
        out += wire._ld(3, wire._ld(1, name.encode()) + wire._ld(2, eff + wire._string(2, e["policy"]) + wire._string(3, e["scope"])))
    return out + b"".join(wire._ld(4, n.encode()) for n in o["effectiveDerivedRoles"])


def device_result(batch, effect, policy, scope, status, edr):
    """Input-order per-tuple arrays (+ per-device-request edr) -> the device-order ``capi.Result`` the assembler takes."""
    res = capi.Result(batch.n_tuples, batch.n_requests, {"policy", "scope", "status", "edr"})
    tp = batch.tuple_perm
    res.effect[:], res.policy[:], res.scope[:], res.status[:] = effect[tp], policy[tp], scope[tp], status[tp]
    res.edr[:] = edr
    return res


def python_bytes(lt, inputs, batch, res, dver="default"):
    batch.actions_per_request = [list(i.get("actions") or []) for i in inputs]
    outs, _ = HostSimEvaluator(lt, Conf(globals_=GLOBALS)).assemble(inputs, batch, copy.copy(res).to_input_order(batch), dver, allow_unsupported=True)
    return [encode_check_output(o) for o in outs]


def expected_flags(inputs, status):
    flags, t = [], 0
    for i in inputs:
        f = 0
        for _ in i["actions"]:
            f |= OUT_FLAG[int(status[t])]
            t += 1
        flags.append(f)
    return flags


def made_up(lt, n_tuples, seed):
    """Per-tuple results covering every policy word kind and both scope forms; effects / statuses are the caller's."""
    rng = np.random.default_rng(seed)
    ns, nk = len(lt.scopes), len(lt.policy_keys)
    assert ns > 1 and nk > 0
    kinds = rng.integers(0, 6, size=n_tuples)
    ident = np.where(kinds == capi.P_TABLE, rng.integers(0, nk, size=n_tuples), rng.integers(0, ns, size=n_tuples))
    policy = (kinds.astype(np.uint32) << 28) | ident.astype(np.uint32)
    scope = np.where(rng.integers(0, 2, size=n_tuples) == 0, capi.NONE, rng.integers(0, ns, size=n_tuples)).astype(np.uint32)
    return policy, scope


def fold_inputs():
    principal = {"id": "alice", "roles": ["employee", "manager"], "policyVersion": "20210210"}

    def inp(k, actions):
        return {"requestId": "fold", "principal": principal, "actions": actions,
                "resource": {"kind": "leave_request", "id": "res%d" % k, "policyVersion": "" if k % 2 else "v%d" % k}}
    inputs, effects = [], []
    orders = [(x, y) for x in (A, D) for y in (A, D)] + [(x, y, z) for x in (A, D) for y in (A, D) for z in (A, D)]
    for order in orders:
        # the repeated action between two others, and again with the repeats apart
        inputs.append(inp(len(inputs), ["first"] + ["dup"] * len(order) + ["last"]))
        effects += [A] + list(order) + [D]
        apart, apart_effects = [], []
        for j, e in enumerate(order):
            apart += ["dup", "other%d" % j]
            apart_effects += [e, A if j % 2 else D]
        inputs.append(inp(len(inputs), apart[:-1]))
        effects += apart_effects[:-1]
    inputs.append(inp(len(inputs), []))
    for na in (64, 65, 128, 129):      # chunks of 64 actions, a duplicate in the first and the last chunk
        acts = ["act%d" % (j if j not in (7, na - 1) else 3) for j in range(na)]
        inputs.append(inp(len(inputs), acts))
        effects += [D if j in (3, 7) else A for j in range(na)]
    inputs.append(inp(len(inputs), ["a", "b", "c", "d"]))
    effects += [A, D, A, D]
    return inputs, np.array(effects, dtype=np.uint8)


def test_assembly_with_spans_and_by_walking_gives_the_same_bytes(lt):
    inputs, effect = fold_inputs()
    T = len(effect)
    assert T == sum(len(i["actions"]) for i in inputs)
    it = IngestTable(lt.blob)
    data, off = wire.pack_messages([wire.encode_check_input(i) for i in inputs])
    with_spans = it.flatten_pb(data, off)
    walked = it.flatten_request_pb(wire.encode_check_resources_request(_request_of(inputs)))
    for name in ARRAYS + ("tuple_perm", "vreq_input"):
        assert np.array_equal(getattr(with_spans, name), getattr(walked, name)), name
    assert with_spans.n_requests > len(inputs) and not np.array_equal(with_spans.tuple_perm, np.arange(T))
    policy, scope = made_up(lt, T, 1)
    status = np.zeros(T, dtype=np.uint8)
    status[-4:] = [capi.ST_OK, capi.ST_CEL_ERROR, capi.ST_UNSUPPORTED, capi.ST_WANTS_TRACE]
    status[[1, 2]] = [capi.ST_WANTS_TRACE, capi.ST_CEL_ERROR]      # on a duplicate that the fold drops: the flag stays
    edr = np.random.default_rng(2).integers(0, 1 << 62, size=with_spans.n_requests, dtype=np.uint64)
    raws = []
    for batch in (with_spans, walked):
        res = device_result(batch, effect, policy, scope, status, edr)
        raw, flags = it.assemble_pb(batch, res, data, off)
        assert list(flags) == expected_flags(inputs, status)
        raws.append(raw)
    assert raws[0] == raws[1]
    assert raws[0] == python_bytes(lt, inputs, with_spans, device_result(with_spans, effect, policy, scope, status, edr))
    statuses_seen = {f for f in expected_flags(inputs, status)}
    assert {0, 1 | 2 | 16, 2 | 16} <= statuses_seen
    it.close()


@pytest.mark.parametrize("n", [1023, 1024, 2047, 2048, 4097])
def test_part_boundaries_give_the_same_batch_and_bytes(lt, n):
    """One part below 2048 inputs, two from 2048, four at 4097 (none below 1024): later slices bring strings of their own
    and strings an earlier slice saw first, so the merge has to remap both."""
    inputs = [{"requestId": "q%d" % (i % 5), "principal": {"id": "p%d" % (i % 700), "roles": ["employee", "role%d" % (i // 900)]},
               "resource": {"kind": "leave_request", "id": "r%d" % i, "attr": {"owner": "p%d" % ((i * 7) % 1300), "status": "s%d" % (i // 512)}},
               "actions": ["view", "act%d" % (i // 1000)] if i % 3 else ["view"]} for i in range(n)]
    it = IngestTable(lt.blob)
    data, off = wire.pack_messages([wire.encode_check_input(i) for i in inputs])
    for sort in (True, False):
        one, four = it.flatten_pb(data, off, sort=sort, threads=1), it.flatten_pb(data, off, sort=sort, threads=4)
        for name in ARRAYS + ("tuple_perm", "vreq_input"):
            assert np.array_equal(getattr(one, name), getattr(four, name)), (name, sort)
        T = one.n_tuples
        policy, scope = made_up(lt, T, n)
        rng = np.random.default_rng(n)
        effect = rng.integers(1, 3, size=T).astype(np.uint8)
        status = rng.integers(0, 4, size=T).astype(np.uint8)
        edr = rng.integers(0, 1 << 62, size=one.n_requests, dtype=np.uint64)
        res = device_result(one, effect, policy, scope, status, edr)
        raw1, flags1 = it.assemble_pb(one, res, data, off, threads=1)
        raw4, flags4 = it.assemble_pb(four, res, data, off, threads=4)
        assert raw1 == raw4 and np.array_equal(flags1, flags4)
        assert list(flags1) == expected_flags(inputs, status)
    it.close()


@pytest.mark.parametrize("kind", [capi.P_RESOURCE, capi.P_PRINCIPAL])
def test_long_policy_keys_at_the_writers_allowance(lt, kind):
    """Policy key + scope of 223 .. 226 bytes (the assembler's per-action allowance ends at 224) and of about 1000, on 1 to
    64 actions of one input, keys changing from action to action."""
    scope_ix = max(range(len(lt.scopes)), key=lambda s: len(lt.scopes[s]))
    scope_s = lt.scopes[scope_ix]
    assert scope_s
    inputs, policy, scope = long_key_inputs(scope_s, kind == capi.P_RESOURCE), [], []
    for i in inputs:
        for j in range(len(i["actions"])):      # the long key on the even actions, a short table key between them
            policy.append((kind << 28) | scope_ix if j % 2 == 0 else (capi.P_TABLE << 28))
            scope.append(scope_ix if j % 2 == 0 else capi.NONE)
    policy, scope = np.array(policy, dtype=np.uint32), np.array(scope, dtype=np.uint32)
    T = len(policy)
    it = IngestTable(lt.blob)
    data, off = wire.pack_messages([wire.encode_check_input(i) for i in inputs])
    batch = it.flatten_pb(data, off)
    res = device_result(batch, np.full(T, A, dtype=np.uint8), policy, scope, np.zeros(T, dtype=np.uint8), np.zeros(batch.n_requests, dtype=np.uint64))
    raw, _ = it.assemble_pb(batch, res, data, off)
    want = python_bytes(lt, inputs, batch, res)
    assert raw == want
    lengths = {len(e["policy"]) + len(e["scope"]) for r in raw for e in wire.decode_check_output(r)["actions"].values()}
    assert {223, 224, 225, 226, 1000} <= lengths
    if kind == capi.P_RESOURCE:      # one principal: the request form, whose batch has no spans - the road that walks the messages again
        walked = it.flatten_request_pb(wire.encode_check_resources_request(_request_of(inputs)))
        res = device_result(walked, np.full(T, A, dtype=np.uint8), policy, scope, np.zeros(T, dtype=np.uint8), np.zeros(walked.n_requests, dtype=np.uint64))
        assert it.assemble_pb(walked, res, data, off)[0] == want
    it.close()


def test_refusals_keep_their_texts(lt):
    inputs = [{"requestId": "e", "principal": {"id": "p", "roles": ["employee"]}, "resource": {"kind": "leave_request", "id": "r%d" % i},
               "actions": ["view", "edit"]} for i in range(3)]
    it = IngestTable(lt.blob)
    data, off = wire.pack_messages([wire.encode_check_input(i) for i in inputs])
    fewer = wire.pack_messages([wire.encode_check_input(i) for i in inputs[:-1]])
    request = wire.encode_check_resources_request(_request_of(inputs))
    request_fewer = wire.encode_check_resources_request(_request_of(inputs[:-1]))
    batch, rbatch = it.flatten_pb(data, off), it.flatten_request_pb(request)
    T = batch.n_tuples

    def res_of(b, policy=capi.P_NO_MATCH << 28, scope=capi.NONE):
        return device_result(b, np.full(T, A, dtype=np.uint8), np.full(T, policy, dtype=np.uint32), np.full(T, scope, dtype=np.uint32),
                             np.zeros(T, dtype=np.uint8), np.zeros(b.n_requests, dtype=np.uint64))
    it.assemble_pb(batch, res_of(batch), data, off)
    it.assemble_response_pb(rbatch, res_of(rbatch), request)
    with pytest.raises(IngestError, match="^batch does not belong to these inputs$"):
        it.assemble_pb(batch, res_of(batch), *fewer)
    with pytest.raises(IngestError, match="^batch does not belong to these inputs$"):      # the road that walks the messages
        it.assemble_pb(rbatch, res_of(rbatch), *fewer)
    with pytest.raises(IngestError, match="^batch does not belong to this request$"):
        it.assemble_response_pb(rbatch, res_of(rbatch), request_fewer)
    if it.trace_scope():
        with pytest.raises(IngestError, match="^batch does not belong to these inputs$"):
            trace_pb(it, batch, res_of(batch), np.zeros((0, capi.TRACE_RECORD_WORDS), dtype=np.uint32), *fewer)
    for word, scope, text in (((capi.P_TABLE << 28) | len(lt.policy_keys), capi.NONE, "policy id out of range"),
                              ((capi.P_RESOURCE << 28) | len(lt.scopes), capi.NONE, "scope index out of range"),
                              ((capi.P_PRINCIPAL << 28) | len(lt.scopes), capi.NONE, "scope index out of range"),
                              (capi.P_NO_MATCH << 28, len(lt.scopes), "scope index out of range"),
                              (7 << 28, capi.NONE, "unknown policy word")):
        with pytest.raises(IngestError, match="^%s$" % text):
            it.assemble_pb(batch, res_of(batch, word, scope), data, off)
        with pytest.raises(IngestError, match="^%s$" % text):
            it.assemble_response_pb(rbatch, res_of(rbatch, word, scope), request)      # include_meta: the keys are built
    # a permutation entry outside the batch, written into the batch's own array
    for b, call in ((batch, lambda: it.assemble_pb(batch, res_of(batch), data, off)),
                    (rbatch, lambda: it.assemble_response_pb(rbatch, res_of(rbatch), request))):
        perm = load().cbi_batch_tuple_perm(b.native.h)
        keep, perm[1] = perm[1], T
        with pytest.raises(IngestError, match="^corrupt tuple permutation$"):
            call()
        perm[1] = keep
        call()
    it.close()
