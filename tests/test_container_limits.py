"""Lists and maps the REQUEST brings, on every road: indexing, selection, size, equality, nesting, and what the wire can say that no dict can.

The pieces of code this module aims at, none of which had a module of its own:
  cbh_interp.h   OP_INDEX (a list by an int, a uint, a double; a map by a key), OP_SELECT / OP_HASSEL (a map by a key of the policy),
                 OP_SIZE
  cbh_vm.h       map_find (every lookup in a map: OP_SELECT, OP_HASSEL, OP_INDEX, `in`), val_equal (`==`, `!=`, `in` of containers)
  the encoders   flatten.py (dict road), Encoder::enc / enc_map of cbi_flatten.h (host wire road), w_container_walk_fn of
                 cbh_wire.h (device road).  They lay a nested value out in three heap orders - the host sides write a container's
                 children first, the device writes a container's own entries first and every nested container behind what was
                 allocated before it - and a decision kernel must read all three alike.
The limits, restated from the headers (test_the_limits_are_the_headers) and used to BUILD the inputs:
  WIRE_MAX_DEPTH = 8            cbh_wire.h CBH_WIRE_MAX_DEPTH: containers nested deeper are the host flattener's (WireStats.n_host)
  WIRE_MAX_VALUE_ENTRIES        cbh_wire.h: heap entries of one attribute value on the device road (0xFFFFF)
  WIRE_MAX_MAP_ENTRIES = 256    cbh_wire.h CBH_WIRE_MAX_MAP_ENTRIES: wire entries of ONE map written to the heap on the device road; a wider
                                map is the host flattener's (it bounds the device flattener's search for a repeated key: layer `wide`)
  list index                    an int, a uint below 2^62 or an integral double in [0, 4e18) that is below the length (OP_INDEX compares
                                64 bits BEFORE it narrows: 2^32 is no index of any list, never element 0)

What is decided and what is flagged (val_equal), the rule the predicted flagged set follows - from the inputs, never from an answer:
two lists of EQUAL length are compared element by element, in order, and the comparison ends at the first unequal pair of scalars;
a pair in which either element is a list or a map, met before that, leaves the tuple to the caller's engine (CBH_ST_UNSUPPORTED).
Two maps: always.  Lists of different lengths, a list against a map, a container against a scalar: decided (unequal).

What was found.
  1  A map on the heap kept every wire entry of a repeated key, and map_find returns the FIRST: on the two wire roads
     `R.attr.m.k` (a constant path, resolved by the flatteners: the last entry, as protobuf maps decode) and `R.attr.m[P.attr.key]`
     read different values of ONE message, and size(), comprehensions and exists_one counted the key twice.  Now a map on the heap
     holds a key once: the host flattener keeps the last entry of a key (cbi_flatten.h map_tape), and the device flattener leaves a
     message with such a map to the host flattener (n_host: counted, never guessed).  map_find is the parent's: scanning from the
     end cost cbh_check_kernel two registers and with them a wave of occupancy (profiles/container_limits_kernel_resources.txt),
     and with one entry per key there is nothing left for it to decide.  On the parent test_*[dup_keys_*] fail, and the
     layers that hold a map of more than 256 entries (select, sizes, flat, wide) in their n_host alone - the bound is this change's.
  2  oracle/celeval.py _index called int() on a NaN / an infinite double index, which raises ValueError / OverflowError, no
     CelError: the reference itself fell over.  It now reports cel-go's evaluation error.

The reference per (request, action) is oracle/check.py: effect, policy key, and CBH_ST_CEL_ERROR exactly where the oracle reports an
evaluation error for that action's expression.  Where the wire bytes say what no dict can (a key twice, odd Value encodings), the
module decodes the message itself the protobuf way (pb_check_input below: the last entry of a key wins, the last field of a Value
wins, a field with another wire type than its declaration's is unknown) and hands THAT dict to the oracle;
test_the_decoder_reads_as_protobuf_does pins the decoder with hand-worked expectations.

Stores: `w` (cbh_walk2_kernel with cbh_walk2_interp_kernel), `g` (the general walk cbh_check_kernel*, forced by a neighbouring kind
of 17 action globs), `f` (a flat store whose leaf conditions need the evaluator call: cbh_check_flat_kernel_any*).  Every run
asserts the kernel it meant to reach.  Tiers: *_on_emulator (the kernels on the wave emulator; dict road, host wire road =
libcerbos_ingest's cbi_flatten_pb, device road = the parser kernels of cbh_wire.h on the emulator), *_on_simulator (the library on
tests/sim_engine.py: cbh_check_batch of the dict batch and of IngestTable.flatten_pb's, cbh_wire_flatten -> cbh_check_resident,
cbh_wire_check_pb), *_on_gpu (the same body on the device).  A layer whose messages the device flattener must leave to the host
(nine containers deep; a key twice; a map of more than 256 entries) asserts n_host = exactly those messages, and cbh_wire_check_pb's answer - HostFlattenerNeeded,
then the same bytes through the host flattener, INTEGRATION.md's road - is judged like every other.

Two protobuf merge cases neither flattener reads as protobuf does: two struct_value / list_value in ONE Value and
two value fields in ONE entry are merged by protobuf; both flatteners take the last occurrence whole.  test_*[merge_cases_*] pins
that reading on both wire roads alike (the decoder here reads the same way, on purpose, and says so).

Mutation check (each mutant on a scratch copy, CPU tier, never committed):
   a  the parent's cbi_flatten.h, cbh_wire.h      killed: test_on_emulator / test_on_simulator[dup_keys_w | dup_keys_g], and nothing else - this IS the parent
      (first-wins map_find is the code's)        with the module added.  Host wire road: `d_idx`, `d_sel`, `size`, `one`, `count` and the t_* of a repeated
                                                 key; device road: n_host is 0 where the messages with a repeated key are wanted
   b  OP_INDEX (u64)k < cont_len -> <=           killed: test_on_emulator / test_on_simulator[access_* | sizes_* | wire_forms_* | dup_keys_* | merge_cases_*]
                                                 (index = length: the heap entry behind the list is answered where an error is wanted)
   c  d == trunc(d) dropped                      killed: test_on_emulator / test_on_simulator[access_*] (0.5, len - 0.5)
   d  d >= 0 dropped                             an equivalent mutant: a negative integral double converts to a negative k, which `k >= 0` refuses; -0.0
                                                 is >= 0 already.  Every test passes, and must
   e  (u32)k before the range test               killed: test_on_emulator / test_on_simulator[access_*] (2^32 reads element 0, 2^32 + 1 element 1)
   f  OP_HASSEL: a null value as an absent key   killed: test_on_emulator / test_on_simulator[select_* | paths_* | wire_forms_* | dup_keys_*]
   g  off2 = fr.slot + 1 (a nested container      killed: test_on_emulator / test_on_simulator[depth_* | select_*] (device road) - the issue's own mutant: the
      placed before its parent's siblings)       slots are taken inside the parent's run, whose later siblings then overwrite them.  Two more of the kind:
   g' the device walker's `used`: a nested map   killed: test_on_emulator / test_on_simulator[select_* | paths_* | depth_*] (device road: a sibling behind
      counted as a list (used += n2)             a nested container reads the container's entries);  `used` begun at n0 for a map (every nested
                                                 container allocated inside its parent's entries): [select_* | paths_* | flat_f | wire_forms_* | merge_cases_*]
   h  items.size() / 2 -> items.size()           killed: test_on_emulator / test_on_simulator[select_* | paths_* | sizes_* | wire_forms_* | dup_keys_* |
                                                 merge_cases_*] (host wire road)
   i  the duplicate removal keeps the first      killed: test_on_emulator / test_on_simulator[dup_keys_*] (host wire road), nothing else
   j  val_equal answers nested lists             killed: test_on_emulator / test_on_simulator[equality_* | flat_f] (the predicted flagged set comes back decided)
   k  the device walker finds the repeated key   killed: test_on_emulator / test_on_simulator[dup_keys_* | wide_*] (n_host), nothing else
   m  CBH_WIRE_MAX_MAP_ENTRIES one more          killed: test_on_emulator / test_on_simulator[wide_*] (257 entries stay on the device road)
      and does not route
"""
import struct

import numpy as np
import pytest

from cerbos_amd import wire
from cerbos_amd.flatten import Flattener
from cerbos_amd.lower.blob import lower_rule_table
from cerbos_amd.policy.loader import policies_from_docs
from cerbos_amd.ruletable.build import rule_table_from_policies
from oracle.check import EvalParams, RuleTableOracle
from test_comprehension_limits import expressions, general_walk_doc, judge
from test_string_limits import API, F_WANT_DR, NOW, Layer, _constants, cond_store, header_value, judge_outputs, request

KIND = "c"
WIRE_MAX_DEPTH = 8
WIRE_MAX_VALUE_ENTRIES = 0xFFFFF
WIRE_MAX_MAP_ENTRIES = 256
LENGTHS = (0, 1, 2, 63, 64, 65, 300)
MAP_SIZES = (0, 1, 2, 64, 65, 300)
_ld, _varint = wire._ld, wire._varint


def test_the_limits_are_the_headers():
    assert header_value("CBH_WIRE_MAX_DEPTH", "cbh_wire.h") == WIRE_MAX_DEPTH
    assert header_value("CBH_WIRE_MAX_VALUE_ENTRIES", "cbh_wire.h") == WIRE_MAX_VALUE_ENTRIES
    assert header_value("CBH_WIRE_MAX_MAP_ENTRIES", "cbh_wire.h") == WIRE_MAX_MAP_ENTRIES


# ---- the protobuf way to read a CheckInput: what the oracle is given where no dict can say what the bytes say


def pb_fields(buf):
    """(number, wire type, value) of every field of a message: a varint's value, the 8 / 4 bytes of a fixed one, a length-delimited
    payload.  A length varint may be longer than it needs to be."""
    i, n = 0, len(buf)

    def varint():
        nonlocal i
        v = shift = 0
        while True:
            b = buf[i]
            i += 1
            v |= (b & 0x7F) << shift
            shift += 7
            if not b & 0x80:
                return v
    while i < n:
        key = varint()
        num, wt = key >> 3, key & 7
        if wt == 0:
            yield num, wt, varint()
        elif wt == 1:
            yield num, wt, bytes(buf[i:i + 8])
            i += 8
        elif wt == 5:
            yield num, wt, bytes(buf[i:i + 4])
            i += 4
        else:
            assert wt == 2, wt
            ln = varint()
            assert i + ln <= n
            yield num, wt, bytes(buf[i:i + ln])
            i += ln


VALUE_WIRE_TYPES = {1: 0, 2: 1, 3: 2, 4: 0, 5: 2, 6: 2}      # google/protobuf/struct.proto: null, number, string, bool, struct, list


def pb_value(buf):
    """google.protobuf.Value: a oneof - the last member on the wire is the value; a field whose wire type is not its declaration's is
    an unknown field; no member at all reads as null (cel-go's view of a Value without a kind).  (Two struct_value / list_value
    members: protobuf MERGES them; this reads the last one whole, as both flatteners do - DESIGN.md 4.9, test_*[merge_cases_*].)"""
    out = None
    for num, wt, v in pb_fields(buf):
        if VALUE_WIRE_TYPES.get(num) != wt:
            continue
        if num == 1:
            out = None
        elif num == 2:
            out = struct.unpack("<d", v)[0]
        elif num == 3:
            out = v.decode("utf-8")
        elif num == 4:
            out = bool(v)
        elif num == 5:
            out = pb_map(e for n2, w2, e in pb_fields(v) if n2 == 1 and w2 == 2)
        else:
            out = [pb_value(e) for n2, w2, e in pb_fields(v) if n2 == 1 and w2 == 2]
    return out


def pb_map(entries):
    """map<string, Value>: an entry without a key has the key "", one without a value a Value without a kind (null); a key that
    comes again replaces the entry (a Go map: one key, the last value)"""
    out = {}
    for ent in entries:
        key, val = "", None
        for num, wt, v in pb_fields(ent):
            if num == 1 and wt == 2:
                key = v.decode("utf-8")
            elif num == 2 and wt == 2:
                val = pb_value(v)
        out.pop(key, None)
        out[key] = val
    return out


def pb_check_input(msg):
    inp = {"requestId": "", "actions": [], "principal": {"id": "", "roles": [], "attr": {}}, "resource": {"kind": "", "id": "", "attr": {}}}
    for num, wt, v in pb_fields(msg):
        if wt != 2:
            continue
        if num == 1:
            inp["requestId"] = v.decode()
        elif num == 4:
            inp["actions"].append(v.decode())
        elif num in (2, 3):
            part = inp["resource" if num == 2 else "principal"]
            names = {1: "kind", 3: "id"} if num == 2 else {1: "id"}
            attrs = []
            for n2, w2, x in pb_fields(v):
                if w2 != 2:
                    continue
                if n2 in names:
                    part[names[n2]] = x.decode()
                elif n2 == 3 and num == 3:
                    part["roles"].append(x.decode())
                elif n2 == 4:
                    attrs.append(x)
            part["attr"] = pb_map(attrs)
    return inp


def num(x):
    return _varint(2 << 3 | 1) + struct.pack("<d", x)


def ent(key, value_bytes, field=1):
    """a map entry as every encoder writes it"""
    return _ld(field, (_ld(1, key.encode()) if key is not None else b"") + (_ld(2, value_bytes) if value_bytes is not None else b""))


def raw_message(rid, actions, pattr, attr_entries):
    """a CheckInput whose Resource.attr is the given entries (field 4 each), byte for byte"""
    res = wire._string(1, KIND) + wire._string(3, "r") + b"".join(attr_entries)
    return wire._string(1, rid) + _ld(2, res) + _ld(3, wire.encode_principal({"id": "p", "roles": ["user"], "attr": pattr})) + \
        b"".join(_ld(4, a.encode()) for a in actions)


def test_the_decoder_reads_as_protobuf_does():
    """hand-worked: every expectation below follows from the protobuf encoding rules alone"""
    one, two = num(1.0), num(2.0)
    assert one == b"\x11" + bytes(6) + b"\xf0\x3f"
    assert pb_value(b"") is None and pb_value(b"\x08\x00") is None                        # no member; null_value
    assert pb_value(one) == 1.0 and pb_value(b"\x20\x01") is True and pb_value(b"\x1a\x01k") == "k"
    assert pb_value(one + b"\x1a\x01k") == "k" and pb_value(b"\x1a\x01k" + one) == 1.0      # two kinds: the last
    assert pb_value(b"\x18\x05") is None and pb_value(one + b"\x18\x05") == 1.0             # string_value as a varint: unknown
    assert pb_value(b"\x1a\x81\x00k") == "k"                                               # a length of two bytes for 1
    assert pb_value(_ld(6, _ld(1, one) + b"\x48\x07" + _ld(1, two))) == [1.0, 2.0]           # an unknown field among the values
    assert pb_value(_ld(6, b"")) == [] and pb_value(_ld(5, b"")) == {}
    m = _ld(5, ent("k", one) + ent("j", two) + ent("k", two))
    assert pb_value(m) == {"j": 2.0, "k": 2.0} and list(pb_value(m)) == ["j", "k"]           # a key twice: one key, the last value
    assert pb_value(_ld(5, ent("k", None))) == {"k": None} and pb_value(_ld(5, ent(None, one))) == {"": 1.0}
    assert pb_value(_ld(5, _ld(1, _ld(2, one) + _ld(1, b"k")))) == {"k": 1.0}                # the fields in the order 2, 1
    msg = raw_message("q", ["a", "b"], {"key": "k"}, [ent("m", m, 4), ent("m", one, 4)])
    got = pb_check_input(msg)
    assert got == {"requestId": "q", "actions": ["a", "b"], "principal": {"id": "p", "roles": ["user"], "attr": {"key": "k"}},
                   "resource": {"kind": KIND, "id": "r", "attr": {"m": 1.0}}}
    plain = request("x", KIND, ["a"], pattr={"z": [1.5, {"q": None}]}, rattr={"m": {"": "s", "t": True}})
    assert pb_check_input(wire.encode_check_input(plain)) == plain


# ---- a layer: the requests once, a store per road, the oracle's answers once


class Spec:
    """conds: {action: expression}; inputs: dicts, or messages: bytes (then inputs = what protobuf reads from them);
    over: the pairs built to be flagged; groups: {label: pairs}; wire_only: no dict road; host: the request ids whose messages the
    device flattener must leave to the host flattener; roads: the stores the layer runs against"""

    def __init__(self, name, conds, inputs=None, messages=None, over=(), groups=None, wire_only=False, host=(), roads=("w", "g")):
        self.name, self.conds, self.over, self.groups, self.wire_only, self.host, self.roads = name, conds, set(over), groups or {}, wire_only, set(host), roads
        if messages is None:
            messages = [wire.encode_check_input(i) for i in inputs]
        else:
            assert inputs is None
            inputs = [pb_check_input(m) for m in messages]
        self.inputs, self.messages = inputs, messages
        self.host |= {i["requestId"] for i, m in zip(inputs, messages) if has_wide_map(m, "t_idx" in conds)}
        self.layers = {}

    def layer(self, road):
        if road not in self.layers:
            self.layers[road] = ContainerLayer(self, road)
        return self.layers[road]


def has_wide_map(msg, reads_attr_whole):
    """whether a map of the message's Resource.attr that reaches the heap has more than WIRE_MAX_MAP_ENTRIES entries ON THE WIRE: the
    device flattener leaves such a message to the host flattener (the bound of its search for a repeated key).  Every attribute of these
    stores is read whole; R.attr itself only by the stores with `t_idx`."""
    def wide(value):
        last = None
        for n_, w_, x in pb_fields(value):
            if VALUE_WIRE_TYPES.get(n_) == w_:
                last = (n_, x)
        if last is None or last[0] < 5:
            return False
        kids = [e for n_, w_, e in pb_fields(last[1]) if n_ == 1 and w_ == 2]
        if last[0] == 6:
            return any(wide(k) for k in kids)
        return len(kids) > WIRE_MAX_MAP_ENTRIES or any(wide(v) for k in kids for v in [x for n_, w_, x in pb_fields(k) if n_ == 2 and w_ == 2][-1:])
    resource = [v for n_, w_, v in pb_fields(msg) if n_ == 2 and w_ == 2][-1]
    attrs = [v for n_, w_, v in pb_fields(resource) if n_ == 4 and w_ == 2]
    return (reads_attr_whole and len(attrs) > WIRE_MAX_MAP_ENTRIES) or any(wide(v) for a in attrs for v in [x for n_, w_, x in pb_fields(a) if n_ == 2 and w_ == 2][-1:])


class Part:
    """the messages of a layer the device flattener keeps, as a layer of their own (same store, same answers)"""

    def __init__(self, layer):
        keep = [k for k, i in enumerate(layer.inputs) if i["requestId"] not in layer.spec.host]
        self.name, self.lt, self.loud, self.plan_ok, self.kinds = layer.name + ", without the host flattener's", layer.lt, False, layer.plan_ok, layer.kinds
        self.inputs, self.want = [layer.inputs[k] for k in keep], [layer.want[k] for k in keep]
        ids = {i["requestId"] for i in self.inputs}
        self.over, self.errors = {p for p in layer.over if p[0] in ids}, {p for p in layer.errors if p[0] in ids}
        self.data, self.off = wire.pack_messages([layer.spec.messages[k] for k in keep])


def _is_flat_any(plan):
    name = plan.split("[")[0]
    return name.startswith("cbh_check_flat_kernel") and "_any" in name


PLAN_OK = {"w": lambda plan: "cbh_walk2_interp_kernel" in plan and "cbh_walk2_kernel" in plan, "g": lambda plan: plan.startswith("cbh_check_kernel"), "f": _is_flat_any}
KINDS = {"w": (2,), "g": (0,), "f": (1,)}      # hostsim_last_kind: the general walk, the flat kernels, walk2


class ContainerLayer(Layer):
    def __init__(self, spec, road):
        self.spec, self.road = spec, road
        self.name, self.inputs, self.over, self.groups, self.loud = "%s_%s" % (spec.name, road), spec.inputs, spec.over, spec.groups, False
        docs = [{"apiVersion": API, "resourcePolicy": {"resource": KIND, "version": "default", "rules": [
            {"actions": [a], "roles": ["*"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": m} if isinstance(m, str) else m}} for a, m in spec.conds.items()]}}]
        docs += [general_walk_doc()] if road == "g" else []
        self.rt = rule_table_from_policies(policies_from_docs(docs))
        self.lt = lower_rule_table(self.rt)
        assert not self.lt.unsupported, (self.name, self.lt.unsupported)
        if road == "f":
            assert self.lt.stats["flat"] and not self.lt.stats["flat_closed"] and not self.lt.stats["generic_programs"], (self.name, self.lt.stats)
        else:
            assert self.lt.stats["generic_programs"] and bool(self.lt.walk2_refused) == (road == "g"), (self.name, self.lt.walk2_refused)
        self.kinds, self.plan_ok = KINDS[road], PLAN_OK[road]
        assert len({i["requestId"] for i in self.inputs}) == len(self.inputs)
        if not hasattr(spec, "want"):    # (the other road's store differs in a kind no request names)
            orc = RuleTableOracle(self.rt)
            spec.want = [orc.check(i, EvalParams(now_ns=NOW)) for i in self.inputs]
            by_expr = {e: a for a, m in spec.conds.items() for e in expressions(m)}
            assert len(by_expr) == len(spec.conds)      # an evaluation error names its expression: one action each
            spec.errors = {(i["requestId"], by_expr[e["celError"]["expression"]]) for i, w in zip(self.inputs, spec.want) for e in w["evaluationErrors"]}
        self.want, self.errors = spec.want, spec.errors
        self.batch = None if spec.wire_only else Flattener(self.lt).flatten(self.inputs, sort=False)
        self.data, self.off = wire.pack_messages(spec.messages)

    def check_oracle(self):
        ids = {(i["requestId"], a) for i in self.inputs for a in i["actions"]}
        assert self.over <= ids and self.errors <= ids, (self.name, sorted(self.over - ids)[:3])
        assert not self.over & self.errors, (self.name, sorted(self.over & self.errors)[:3])
        assert 4 * len(self.over) <= len(ids), (self.name, "more than a quarter of the pairs is built to be flagged", len(self.over), len(ids))
        index = {i["requestId"]: k for k, i in enumerate(self.inputs)}
        for label, pairs in self.groups.items():
            seen = {self.want[index[r]]["actions"][a]["effect"] for r, a in pairs if (r, a) not in self.over}
            assert seen == {"EFFECT_ALLOW", "EFFECT_DENY"}, (self.name, label, "the decided pairs do not discriminate", seen)
        grouped = {p for pairs in self.groups.values() for p in pairs}
        assert ids - self.over <= grouped | self.errors, (self.name, "decided pairs in no group", sorted(ids - self.over - grouped - self.errors)[:4])
        assert len(self.inputs) <= 700 and len(self.spec.conds) <= 64, (self.name, len(self.inputs), len(self.spec.conds))
        assert self.spec.host <= set(index)


def host_messages(layer):
    """the layer's messages through libcerbos_ingest's flattener, in input order"""
    from cerbos_amd.ingest import IngestTable
    it = IngestTable(layer.lt.blob)
    try:
        hb = it.flatten_pb(layer.data, layer.off, sort=False)
    finally:
        it.close()
    assert hb.n_requests == len(layer.inputs)
    return hb


def run_on_emulator(layer):
    import hostsim_api
    import wire_device_util as wu
    from cerbos_amd import capi

    def decide(batch, what):
        res = hostsim_api.check(layer.lt, batch, NOW, F_WANT_DR)
        assert hostsim_api.last_kind() in layer.kinds, (layer.name, what, hostsim_api.last_kind())
        judge(capi, layer, res, what)
    if layer.batch is not None:
        decide(layer.batch, "emulator, dict road")
    decide(host_messages(layer), "emulator, host wire road")
    rc, wb = wu.sim_flatten(layer.lt, layer.data, layer.off)
    assert rc == 0 and wb.stats["first_bad"] == 0xFFFFFFFF, (layer.name, rc)
    assert wb.stats["n_host"] == len(layer.spec.host), (layer.name, "messages left to the host flattener", wb.stats["n_host"], len(layer.spec.host))
    if len(layer.spec.host) == len(layer.inputs):
        return
    if layer.spec.host:       # the others, on their own, are the device flattener's
        layer = Part(layer)
        rc, wb = wu.sim_flatten(layer.lt, layer.data, layer.off)
        assert rc == 0 and wb.stats["first_bad"] == 0xFFFFFFFF and wb.stats["n_host"] == 0, (layer.name, rc, wb.stats)
    decide(wu.to_batch(layer.lt, wb), "emulator, device road")


def run_on_library(capi, layer):
    _constants(capi)
    table = capi.Table(layer.lt.blob)
    try:
        if layer.batch is not None:
            judge(capi, layer, table.check(layer.batch, now_ns=NOW, flags=F_WANT_DR), "dict road, cbh_check_batch")
        hb = host_messages(layer)
        judge(capi, layer, table.check(hb, now_ns=NOW, flags=F_WANT_DR), "host wire road, cbi_flatten_pb -> cbh_check_batch")
        db = table.upload(hb)
        try:
            assert layer.plan_ok(table.plan(db, flags=F_WANT_DR)), (layer.name, table.plan(db, flags=F_WANT_DR))    # a test that passes because another kernel decided proves nothing
        finally:
            db.close()
        if layer.spec.host:
            with pytest.raises(capi.HostFlattenerNeeded):
                table.wire_flatten(layer.data, layer.off)
            with pytest.raises(capi.HostFlattenerNeeded):     # ... and the caller takes the same bytes through the host flattener: judged above
                table.wire_check_pb(layer.data, layer.off, now_ns=NOW, flags=F_WANT_DR)
            assert table.last_wire_info["n_host"] == len(layer.spec.host), (layer.name, table.last_wire_info, len(layer.spec.host))
            if len(layer.spec.host) == len(layer.inputs):
                return
            layer = Part(layer)       # the others, on their own, are the device flattener's
        db = table.wire_flatten(layer.data, layer.off)
        try:
            assert db.wire_info["n_host"] == 0, db.wire_info
            table.launch(db, now_ns=NOW, flags=F_WANT_DR)
            judge(capi, layer, table.download(db), "device road, cbh_check_resident")
            assert layer.plan_ok(table.plan(db, flags=F_WANT_DR)), (layer.name, table.plan(db, flags=F_WANT_DR))
        finally:
            db.close()
        raw, flags = table.wire_check_pb(layer.data, layer.off, now_ns=NOW, flags=F_WANT_DR)
        judge_outputs(layer, raw, flags, "device road, cbh_wire_check_pb")
    finally:
        table.close()


def grouped(groups, label, rid, actions):
    for a in actions:
        groups.setdefault("%s %s" % (a, label), []).append((rid, a))


# ---- 1. access: a list by an int, a uint, a double


ACCESS_CONDS = {"int": "R.attr.l[int(R.attr.i)] == P.attr.w", "uint": "R.attr.l[uint(R.attr.i)] == P.attr.w", "dbl": "R.attr.l[R.attr.i] == P.attr.w",
                "plain": "R.attr.l[R.attr.i] != P.attr.w"}
BELOW_4E18 = float(np.nextafter(4e18, 0.0))


def element(j):
    return float(j) + 0.25 if j % 3 else "e%d" % j


def access_indices(n):
    """in range: 0, -0.0, 1, n - 1; errors: n, n + 1, -1, halves, and what a narrowing cast, a conversion or a comparison could fold back
    into the range"""
    inside = [x for x in (0.0, -0.0, 1.0, float(n - 1)) if 0 <= x < n]
    outside = [float(n), float(n + 1), -1.0, 0.5, n - 0.5, 2.0 ** 31, 2.0 ** 32, 2.0 ** 32 + 1, 2.0 ** 53, 4e18, BELOW_4E18, 2.0 ** 62, 2.0 ** 63, 1e300]
    return inside, outside


def make_access():
    inputs, over, groups = [], set(), {}
    k = 0

    def add(l, i, w, label):
        nonlocal k
        rid = "a%d" % k
        k += 1
        rattr = {}
        if l is not ABSENT:
            rattr["l"] = l
        if i is not ABSENT:
            rattr["i"] = i
        inputs.append(request(rid, KIND, list(ACCESS_CONDS), pattr={"w": w}, rattr=rattr))
        grouped(groups, label, rid, ACCESS_CONDS)
        if isinstance(i, str):       # int() / uint() of a STRING are conversions the device leaves to the caller's engine (OP_TOINT)
            over.update({(rid, "int"), (rid, "uint")})
    for n in LENGTHS:
        l = [element(j) for j in range(n)]
        inside, outside = access_indices(n)
        for x in inside:
            add(l, x, l[int(x)], "")
            add(l, x, element(int(x) + 1), "")
        for x in outside:
            add(l, x, l[0] if l else 0.25, "")
    l = [element(j) for j in range(5)]
    for x in ("1", True, None, [1.0], {"a": 1.0}, ABSENT):       # what is no number
        add(l, x, l[1], "")
    for v in ("abc", 7.0, None, True, ABSENT):                   # what is no list
        add(v, 0.0, "a", "")
    return Spec("access", ACCESS_CONDS, inputs, over=over, groups=groups)


ABSENT = object()


def make_access_wire():
    """NaN and the infinities as an index: raw number_value bits, the wire roads only"""
    inputs, groups = [], {}
    specials = [float("nan"), -float("nan"), float("inf"), float("-inf"), struct.unpack("<d", struct.pack("<Q", 0x7FF0000000000001))[0]]
    for n in (0, 1, 65):
        l = [element(j) for j in range(n)]
        for k, x in enumerate(specials + [0.0, 0.0]):      # (the controls: element 0, wanted and not)
            rid = "n%d_%d" % (n, k)
            inputs.append(request(rid, KIND, list(ACCESS_CONDS), pattr={"w": l[0] if l and k <= len(specials) else "e1"}, rattr={"l": l, "i": x}))
            grouped(groups, "", rid, ACCESS_CONDS)
    return Spec("access_wire", ACCESS_CONDS, inputs, groups=groups, wire_only=True)


# ---- 2. select: a map by a key, beside the constant path of the same access


SELECT_CONDS = {
    # the constant paths: resolved by the flatteners, a column each
    "c_sel": "R.attr.m.k == P.attr.w", "c_has": "has(R.attr.m.k)", "c_idx": 'R.attr.m["k"] == P.attr.w', "c_kk": "R.attr.m.kk == P.attr.w",
    "c_empty": 'R.attr.m[""] == P.attr.w', "c_deep": "R.attr.m.k.a == P.attr.w", "c_has_deep": "has(R.attr.m.k.a)",
    # the same accesses through a base that is no constant path: OP_SELECT / OP_HASSEL / OP_INDEX
    "d_sel": "cel.bind(x, R.attr.m, x.k) == P.attr.w", "d_has": "cel.bind(x, R.attr.m, has(x.k))", "d_kk": "cel.bind(x, R.attr.m, x.kk) == P.attr.w",
    "d_idx": "R.attr.m[P.attr.key] == P.attr.w", "d_in": "P.attr.key in R.attr.m", "d_deep": "cel.bind(x, R.attr.m, x.k.a) == P.attr.w",
    "d_has_deep": "cel.bind(x, R.attr.m, has(x.k.a))", "d_idx_k": 'cel.bind(x, R.attr.m, x["k"]) == P.attr.w', "d_idx_empty": 'cel.bind(x, R.attr.m, x[""]) == P.attr.w',
    # an element of a list, a loop variable
    "l_sel": "R.attr.l[0].k == P.attr.w", "l_has": "has(R.attr.l[0].k)", "l_loop": "R.attr.l.exists(e, e.k == P.attr.w)", "l_idx": "R.attr.l[0][P.attr.key] == P.attr.w",
    "l_all_has": "R.attr.l.all(e, has(e.k))",
}
ONLY_REQUEST = "a key no policy names"     # a batch-local id; "k", "kk", "a", "" are strings of the table
VALUES = (1.5, "s", None, True, [1.5, "s"], {"a": 1.5}, {"a": None}, "")


def make_select():
    inputs, groups = [], {}
    n_req = 0

    def add(m, key, w, label="", l=ABSENT):
        nonlocal n_req
        rid = "s%d" % n_req
        n_req += 1
        rattr = {}
        if m is not ABSENT:
            rattr["m"] = m
        rattr["l"] = [m, {"k": "behind"}] if l is ABSENT and m is not ABSENT else ([] if l is ABSENT else l)
        inputs.append(request(rid, KIND, list(SELECT_CONDS), pattr={"key": key, "w": w}, rattr=rattr))
        grouped(groups, label, rid, SELECT_CONDS)
    for n in MAP_SIZES:       # the wanted key first, last, absent; the principal's key is "k" or the key only the request knows
        for where in ("first", "last", "absent"):
            for kv, v in enumerate(VALUES[:3] if n > 2 else VALUES):
                filler = [("f%03d" % j, float(j)) for j in range(max(n - 1, 0))]
                if n == 0 or where == "absent":
                    items = filler + ([("f_last", -1.0)] if n else [])
                else:
                    items = ([("k", v)] + filler) if where == "first" else (filler + [("k", v)])
                m = dict(items)
                assert len(m) == n
                for key in ("k", ONLY_REQUEST):
                    mm = dict(m)
                    if key == ONLY_REQUEST and where != "absent" and n:
                        mm = {(ONLY_REQUEST if a == "k" else a): b for a, b in items}
                    good = (kv + n) % 2 == 0
                    if isinstance(v, dict):
                        w = v["a"] if good else 2.5
                    else:
                        w = v if good else (2.5 if v != 2.5 else 3.5)
                    add(mm, key, w)
    # a key that is a prefix of another, the empty key, both orders
    for m in ({"k": 1.5, "kk": 2.5}, {"kk": 2.5, "k": 1.5}, {"kk": 2.5}, {"": 1.5, "k": 2.5}, {"k": 2.5, "": 1.5}, {"": None}):
        for key in ("k", "kk", "", "kkk"):
            for w in (1.5, 2.5):
                add(m, key, w)
    for key in (1.0, True, None, ["k"], 0.0):         # what is no string, as a key
        add({"k": 1.5, "1": 2.5, "true": 3.5}, key, 1.5)
    for v in (None, [1.5], ["k"], "k", 7.0, ABSENT):    # what is no map
        add(v, "k", 1.5)
    add({"k": 1.5}, "k", 1.5, l=[])                   # l[0] of an empty list; of a list whose first element is no map
    add({"k": 1.5}, "k", 1.5, l=[1.5, {"k": 1.5}])
    add({"k": 1.5}, "k", 1.5, l=[{"j": 1.5}, {"k": 1.5}])
    return Spec("select", SELECT_CONDS, inputs, groups=groups)


PATH_CONDS = {     # a constant path whose intermediate is missing, null, a list, a string, a map without the key
    "p3": "R.attr.a.b.c == P.attr.w", "p3_has": "has(R.attr.a.b.c)", "p2": "R.attr.a.b == P.attr.w", "p2_has": "has(R.attr.a.b)",
    "d3": "cel.bind(x, R.attr.a, x.b.c) == P.attr.w", "d3_has": "cel.bind(x, R.attr.a, has(x.b.c))", "d2_has": "cel.bind(x, R.attr.a, has(x.b))",
}


def make_paths():
    inputs, groups = [], {}
    shapes = [ABSENT, None, [1.5], "s", {}, {"b": None}, {"b": [1.5]}, {"b": "s"}, {"b": {}}, {"b": {"c": 1.5}}, {"b": {"c": None}}, {"b": {"d": 1.5}}, {"b": 1.5},
              {"z": {"q": [1.5]}, "b": {"y": [2.5], "c": 1.5}}]
    for k, a in enumerate(shapes):
        for w in (1.5, None):
            rid = "p%d_%s" % (k, w)
            inputs.append(request(rid, KIND, list(PATH_CONDS), pattr={"w": w}, rattr={} if a is ABSENT else {"a": a}))
            grouped(groups, "", rid, PATH_CONDS)
    return Spec("paths", PATH_CONDS, inputs, groups=groups)


# ---- 3. depth: one value nested 1, 2, 7, 8 and 9 containers deep


def nested(depth, leaf, siblings):
    """level 1 (the outermost) is a list, level 2 a map, in turn.  A list: [a container, THE CHILD, the sibling]; a map:
    {"z": a container, "a": THE CHILD, "b": the sibling} - above the deepest level the sibling sits behind two nested containers, so a
    walker that allocates a nested container's slots from a stale count, or a tape offset that forgets a child, moves it.  (The
    deepest level has scalars on both sides of the leaf: the value is `depth` containers deep, no more.)"""
    v = leaf
    for level in range(depth, 0, -1):
        sib, deepest = siblings[level - 1], level == depth
        if level % 2:
            v = [float(level) if deepest else [float(level), "x"], v, sib]
        else:
            v = {"z": float(level) if deepest else {"q": float(level), "r": "x"}, "a": v, "b": sib}
    return v


def container_depth(v):
    kids = v if isinstance(v, list) else list(v.values()) if isinstance(v, dict) else None
    return 0 if kids is None else 1 + max([container_depth(k) for k in kids] or [0])


def chain(attr, levels):
    e = "R.attr." + attr
    for level in range(1, levels + 1):
        e += "[1]" if level % 2 else ".a"
    return e


def depth_conds(depths):
    conds = {}
    for d in depths:
        conds["leaf%d" % d] = '%s == "leaf"' % chain("v%d" % d, d)
        for level in range(1, d + 1):
            conds["sib%d_%d" % (d, level)] = '%s%s == "after%d"' % (chain("v%d" % d, level - 1), "[2]" if level % 2 else ".b", level)
    return conds


def make_depth(name, depths, host):
    conds = depth_conds(depths)
    inputs, groups = [], {}
    for k in range(70):      # more than a wave; the requests differ in which leaf and which sibling is the wanted one
        rattr = {}
        for d in depths:
            sibs = ["after%d" % (lv + 1) if (k + lv + d) % 3 else "other" for lv in range(d)]
            rattr["v%d" % d] = nested(d, "leaf" if (k + d) % 2 else "fool", sibs)
            assert container_depth(rattr["v%d" % d]) == d
        rid = "d%d" % k
        inputs.append(request(rid, KIND, list(conds), rattr=rattr))
        grouped(groups, "", rid, conds)
    return Spec(name, conds, inputs, groups=groups, host={i["requestId"] for i in inputs} if host else ())


# ---- 4. size and equality


SIZE_CONDS = {"size_l": "size(R.attr.l) == int(P.attr.n)", "size_m": "R.attr.m.size() == int(P.attr.n)", "size_bind": "cel.bind(x, R.attr.m, size(x)) == int(P.attr.n)",
              "size_in": "R.attr.l[0].size() == int(P.attr.n)"}


def make_sizes():
    inputs, groups = [], {}
    for n in LENGTHS:
        for bump in (0, 1):
            rid = "z%d_%d" % (n, bump)
            l = [element(j) for j in range(n)]
            m = {"f%03d" % j: element(j) for j in range(n)}
            inputs.append(request(rid, KIND, list(SIZE_CONDS), pattr={"n": float(n + bump)}, rattr={"l": [l, m] if bump else [m, l], "m": m} if n % 2 else {"l": l, "m": m}))
            grouped(groups, "", rid, SIZE_CONDS)
    for k, v in enumerate((None, 7.0, True, ABSENT)):       # (a string has a size)
        rid = "zz%d" % k
        inputs.append(request(rid, KIND, list(SIZE_CONDS), pattr={"n": 0.0}, rattr={} if v is ABSENT else {"l": v, "m": v}))
        grouped(groups, "", rid, SIZE_CONDS)
    return Spec("sizes", SIZE_CONDS, inputs, groups=groups)


EQ_CONDS = {"eq": "R.attr.a == R.attr.b", "ne": "R.attr.a != R.attr.b", "eq_int": "R.attr.a == [1]", "eq_uint": "[1u] == R.attr.a", "ne_mixed": "R.attr.a != [1u, 2.5]",
            "eq_empty": "R.attr.a == []", "in": "R.attr.a in R.attr.b",
            # the same through the operand-stack interpreter (the conditions above are leaves of the register evaluator)
            "eq_bind": "cel.bind(x, R.attr.a, x == R.attr.b)", "ne_bind": "cel.bind(x, R.attr.a, x != R.attr.b)", "in_bind": "cel.bind(x, R.attr.b, R.attr.a in x)",
            "eq_int_bind": "cel.bind(x, R.attr.a, [1] == x)"}
EQ_LITERALS = {"eq_int": [1.0], "eq_uint": [1.0], "ne_mixed": [1.0, 2.5], "eq_empty": [], "eq_int_bind": [1.0]}      # (the literals' numbers, as doubles: equal across the numeric types)


def is_container(v):
    return isinstance(v, (list, dict))


def same(a, b):
    """equality of the values this module builds: doubles, strings, bools, nulls and lists of them (NaN equals nothing)"""
    if is_container(a) or is_container(b):
        return isinstance(a, list) and isinstance(b, list) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def equality_is_flagged(a, b):
    """the module's rule, from the two values alone"""
    if isinstance(a, dict) and isinstance(b, dict):
        return True
    if not (isinstance(a, list) and isinstance(b, list)) or len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if is_container(x) or is_container(y):
            return True
        if not same(x, y):
            return False
    return False


EQ_PAIRS = [
    ([1.0], [1.0]), ([1.0], [2.0]), ([1.0, 2.5], [1.0, 2.5]), ([1.0, 2.5], [1.0, 2.0]), ([], []), ([], [1.0]), ([1.0], [1.0, 2.5]), ([1.0, 2.5, 3.0], [1.0, 2.5]),
    (["s", None, True], ["s", None, True]), (["s", None, True], ["s", None, False]), (["1"], [1.0]), ([None], [False]),
    ([1.0], {"a": 1.0}), ({"a": 1.0}, [1.0]), ([], {}), ([1.0], 1.0), (1.0, [1.0]), ({"a": 1.0}, 1.0), ("s", ["s"]), (None, []), ([None], None), (1.0, 1.0), ("s", "s"), (1.0, 2.0),
    ([[1.0]], [[1.0]]), ([[1.0]], [[2.0]]), ([1.0, [2.0]], [1.0, [2.0]]), ([1.0, [2.0]], [2.0, [2.0]]), ([[1.0]], [1.0]), ([1.0], [[1.0]]), ([{"a": 1.0}], [{"a": 1.0}]),
    ([[1.0]], [[1.0], 2.0]), ({"a": 1.0}, {"a": 1.0}), ({"a": 1.0}, {"a": 2.0}), ({}, {}), ({"a": 1.0}, {"a": 1.0, "b": 2.0}),
    ([float(j) for j in range(300)], [float(j) for j in range(300)]), ([float(j) for j in range(300)], [float(j) for j in range(299)] + [-1.0]),
    ([float(j) for j in range(65)], [float(j) for j in range(64)]),
]


def in_is_flagged(a, b):
    """`a in b`: b a list - a is compared with its elements in order until one is equal; b a map - a lookup by key, never flagged"""
    if not isinstance(b, list):
        return False
    for y in b:
        if equality_is_flagged(a, y):
            return True
        if same(a, y):
            return False
    return False


def eq_flagged(c, x, y):
    if c in EQ_LITERALS:
        return equality_is_flagged(x, EQ_LITERALS[c])
    return in_is_flagged(x, y) if c.startswith("in") else equality_is_flagged(x, y)


def make_equality(name, pairs, wire_only=False, conds=EQ_CONDS, roads=("w", "g"), flagged=eq_flagged):
    inputs, over, groups = [], set(), {}
    for k, (a, b) in enumerate(pairs):
        for swap in (False, True):
            x, y = (b, a) if swap else (a, b)
            rid = "e%d_%d" % (k, swap)
            inputs.append(request(rid, KIND, list(conds), rattr={"a": x, "b": y}))
            for c in conds:
                if flagged(c, x, y):
                    over.add((rid, c))
            grouped(groups, "", rid, conds)
    return Spec(name, conds, inputs, over=over, groups=groups, wire_only=wire_only, roads=roads)


NAN = float("nan")
EQ_WIRE_PAIRS = [(1.0, [NAN, 1.0]), (NAN, [1.0, NAN]), ([NAN], [NAN]), ([1.0, NAN], [1.0, NAN]), ([NAN], [1.0]), (NAN, [NAN]), ([1.0], [1.0]), ([1.0], [2.0]), ([], []), ([1.0, 2.5], [1.0, 2.5]), ([1.0, 2.5], [1.0, 2.0])]


# ---- the flat store: leaf conditions that need the evaluator call


FLAT_CONDS = {"eq": "R.attr.a == R.attr.b", "in": "R.attr.a in R.attr.b", "c_sel": 'R.attr.b["k"] != R.attr.a', "key_in": "P.attr.key in R.attr.b"}    # (four: the flat batch shape)


def flat_flagged(c, x, y):
    if c == "c_sel":       # b.k against a
        return isinstance(y, dict) and "k" in y and equality_is_flagged(y["k"], x)
    return c != "key_in" and eq_flagged(c, x, y)


def make_flat():
    pairs = EQ_PAIRS + [("k", {"k": "k"}), ("k", {"j": 1.0, "k": 2.5}), (2.5, {"j": 1.0, "k": 2.5}), ("k", {}), (1.5, {"f%03d" % j: float(j) for j in range(299)} | {"k": 1.5}),
                        ("k", ["j", "k"]), (ONLY_REQUEST, {ONLY_REQUEST: 1.0}), (ONLY_REQUEST, [1.0, ONLY_REQUEST]), (1.0, [1, 2.0][1:] + [1.0]), ([1.0], [[2.0], [1.0]][:0] + [1.0])]
    spec = make_equality("flat", pairs, conds=FLAT_CONDS, roads=("f",), flagged=flat_flagged)
    for k, i in enumerate(spec.inputs):
        a = i["resource"]["attr"]["a"]
        i["principal"]["attr"]["key"] = a if isinstance(a, str) else ("k", "j", ONLY_REQUEST)[k % 3]
    spec.messages = [wire.encode_check_input(i) for i in spec.inputs]
    return spec


# ---- 5. wire forms: what only bytes can say


WIRE_CONDS = {
    "c_sel": "R.attr.m.k == P.attr.w", "c_has": "has(R.attr.m.k)", "d_idx": "R.attr.m[P.attr.key] == P.attr.w", "d_has": "cel.bind(x, R.attr.m, has(x.k))",
    "d_sel": "cel.bind(x, R.attr.m, x.k) == P.attr.w", "in": "P.attr.key in R.attr.m", "size": "size(R.attr.m) == int(P.attr.n)",
    "one": "R.attr.m.exists_one(x, x == P.attr.key)", "count": "R.attr.m.filter(x, true).size() == int(P.attr.n)",
    "t_idx": "R.attr[P.attr.tkey] == P.attr.tw", "t_size": "size(R.attr) == int(P.attr.tn)", "t_in": "P.attr.tkey in R.attr", "t_one": "R.attr.exists_one(x, x == P.attr.tkey)",
    "l_size": "size(R.attr.l) == int(P.attr.ln)", "l_first": "R.attr.l[0] == P.attr.w", "l_last": "R.attr.l[int(P.attr.ln) - 1] == P.attr.w",
}


def wire_spec(name, cases, host_if=None):
    """cases: [(label, [attr entry bytes])].  Per case the principal's values come from what PROTOBUF reads out of the bytes (the
    decoder above), a right and a wrong one each, with the key `k` and with a key only the request knows where the map has one"""
    messages, groups, host = [], {}, set()
    for label, entries in cases:
        entries = entries + ([ent("s", num(9.5), 4)] if entries else [])      # (a scalar beside them, for R.attr[...])
        attr = pb_map(e[2] for e in pb_fields(b"".join(entries)))
        m, l = attr.get("m"), attr.get("l")
        keys = ["k"] + ([x for x in m if x != "k"][:1] if isinstance(m, dict) else []) + ["a key of no map"]
        for key in keys:
            for good in (True, False):
                mv = m.get(key) if isinstance(m, dict) else None
                w = mv if good else (2.5 if mv != 2.5 else 3.5)
                if not isinstance(m, dict):
                    w = (l[0] if isinstance(l, list) and l else 1.0) if good else "no"
                tkey = "s" if key == "k" and "s" in attr else "m" if "m" in attr else next(iter(attr), "m")
                tv = attr.get(tkey)
                pattr = {"key": key, "w": None if is_container(w) else w, "n": float((len(m) if isinstance(m, dict) else 0) + (not good)),
                         "tkey": tkey if key != keys[-1] else key, "tw": "no" if is_container(tv) or not good else tv,
                         "tn": float(len(attr) + (not good)), "ln": float((len(l) if isinstance(l, list) else 0) + (not good))}
                rid = "%s/%s/%s" % (label, key, good)
                messages.append(raw_message(rid, list(WIRE_CONDS), pattr, entries))
                grouped(groups, "", rid, WIRE_CONDS)
                if host_if is not None and host_if(entries):
                    host.add(rid)
    return Spec(name, WIRE_CONDS, messages=messages, groups=groups, wire_only=True, host=host)


def struct_of(*entries):
    return _ld(5, b"".join(entries))


def list_of(*values):
    return _ld(6, b"".join(_ld(1, v) for v in values))


S = _ld(3, b"s")          # string_value "s"
LONG1 = b"\x81\x00"       # the length 1 in two bytes


def long_ld(field, payload):
    """a length-delimited field whose length varint has a byte more than it needs"""
    assert len(payload) < 0x80
    return _varint(field << 3 | 2) + bytes([len(payload) | 0x80, 0]) + payload


def make_wire_forms():
    one, two, three = num(1.5), num(2.5), num(3.5)
    unknown = b"\x48\x07" + _ld(12, b"zzz") + _varint(10 << 3 | 1) + bytes(8) + _varint(11 << 3 | 5) + bytes(4)
    plain = struct_of(ent("j", two), ent("k", one))
    cases = [
        ("plain", [ent("m", plain, 4), ent("l", list_of(one, two), 4)]),
        ("value without a kind", [ent("m", struct_of(ent("k", b""), ent("j", one)), 4), ent("l", list_of(b"", one), 4)]),
        ("null_value", [ent("m", struct_of(ent("k", b"\x08\x00"), ent("j", one)), 4), ent("l", list_of(b"\x08\x00"), 4)]),
        ("two kinds, the string last", [ent("m", struct_of(ent("k", one + S), ent("j", one)), 4), ent("l", list_of(one + S, S + one), 4)]),
        ("two kinds, the number last", [ent("m", struct_of(ent("k", S + one), ent("j", one)), 4), ent("l", list_of(S + one), 4)]),
        ("two kinds, a list then a number", [ent("m", struct_of(ent("k", list_of(two) + one), ent("j", one)), 4), ent("l", list_of(list_of(two) + one), 4)]),
        ("two kinds, a number then a map", [ent("m", struct_of(ent("j", one + struct_of(ent("q", two))), ent("k", one)), 4), ent("l", list_of(one + struct_of(ent("q", two)), two), 4)]),
        ("two kinds at the top", [ent("m", one + plain, 4), ent("l", S + list_of(one), 4)]),
        ("two kinds at the top, the scalar last", [ent("m", plain + one, 4), ent("l", list_of(one) + S, 4)]),
        ("an entry without a value", [ent("m", struct_of(ent("k", None), ent("j", one)), 4), ent("l", list_of(one), 4)]),
        ("an entry without a key", [ent("m", struct_of(ent(None, two), ent("k", one)), 4), ent("l", list_of(one), 4)]),
        ("an empty entry", [ent("m", struct_of(_ld(1, b""), ent("k", one)), 4), ent("l", list_of(one), 4)]),
        ("the fields in the order 2, 1", [ent("m", struct_of(_ld(1, _ld(2, one) + _ld(1, b"k")), _ld(1, _ld(2, two) + _ld(1, b"j"))), 4), _ld(4, _ld(2, list_of(one)) + _ld(1, b"l"))]),
        ("an unknown field in a Struct", [ent("m", struct_of(unknown, ent("k", one), unknown, ent("j", two)), 4), ent("l", list_of(one), 4)]),
        ("an unknown field in a ListValue", [ent("m", plain, 4), ent("l", _ld(6, unknown + _ld(1, one) + unknown + _ld(1, two) + unknown), 4)]),
        ("an unknown field in an entry", [ent("m", struct_of(_ld(1, unknown + _ld(1, b"k") + unknown + _ld(2, one) + unknown), ent("j", two)), 4), ent("l", list_of(one), 4)]),
        ("an unknown field in a Value", [ent("m", struct_of(ent("k", unknown + one + unknown), ent("j", unknown)), 4), ent("l", list_of(unknown + one, one + unknown), 4)]),
        ("a key with the wrong wire type", [ent("m", struct_of(_ld(1, b"\x08\x05" + _ld(2, two)), ent("k", one)), 4), ent("l", list_of(one), 4)]),
        ("a value with the wrong wire type", [ent("m", struct_of(_ld(1, _ld(1, b"k") + b"\x10\x05"), ent("j", one)), 4), ent("l", list_of(one), 4)]),
        ("a string_value as a varint", [ent("m", struct_of(ent("k", b"\x18\x05"), ent("j", one + b"\x18\x05")), 4), ent("l", list_of(b"\x18\x05", one), 4)]),
        ("a number_value as a varint", [ent("m", struct_of(ent("k", b"\x10\x05"), ent("j", S + b"\x10\x05")), 4), ent("l", list_of(b"\x10\x05"), 4)]),
        ("a struct_value as a varint", [ent("m", struct_of(ent("k", one), ent("j", b"\x28\x05")), 4), ent("l", list_of(b"\x30\x05", one), 4)]),
        ("a values field with the wrong wire type", [ent("m", plain, 4), ent("l", _ld(6, b"\x08\x05" + _ld(1, one)), 4)]),
        ("a fields field with the wrong wire type", [ent("m", _ld(5, b"\x08\x05" + ent("k", one)), 4), ent("l", list_of(one), 4)]),
        ("a long length: the key", [ent("m", struct_of(_ld(1, long_ld(1, b"k") + _ld(2, one)), ent("j", two)), 4), ent("l", list_of(one), 4)]),
        ("a long length: the value", [ent("m", struct_of(_ld(1, _ld(1, b"k") + long_ld(2, one)), ent("j", two)), 4), ent("l", list_of(one), 4)]),
        ("a long length: the entry", [ent("m", struct_of(long_ld(1, _ld(1, b"k") + _ld(2, one)), ent("j", two)), 4), ent("l", _ld(6, long_ld(1, one)), 4)]),
        ("a long length: the string", [ent("m", struct_of(ent("k", long_ld(3, b"s")), ent("j", two)), 4), ent("l", list_of(long_ld(3, b"s")), 4)]),
        ("a long length: the struct", [ent("m", long_ld(5, ent("k", one)), 4), ent("l", long_ld(6, _ld(1, one)), 4)]),
        ("a long length: the attribute", [long_ld(4, _ld(1, b"m") + _ld(2, plain)), long_ld(4, long_ld(1, b"l") + long_ld(2, list_of(one)))]),
        ("a bool of two bytes", [ent("m", struct_of(ent("k", b"\x20\x81\x00"), ent("j", b"\x20\x80\x00")), 4), ent("l", list_of(b"\x20\x81\x00"), 4)]),
        ("no map at all", [ent("l", list_of(three), 4)]),
        ("nothing", []),
    ]
    return wire_spec("wire_forms", cases)


def make_dup_keys():
    """a key twice or three times: equal and different values, first / last, side by side / apart; in the nested map and at the top"""
    one, two, three = num(1.5), num(2.5), num(3.5)
    other = ONLY_REQUEST
    L = ent("l", list_of(one), 4)

    def m(*entries):
        return ent("m", struct_of(*entries), 4)
    cases = [
        ("control", [m(ent("j", two), ent("k", one)), L]),
        ("twice, equal, side by side", [m(ent("k", one), ent("k", one), ent("j", two)), L]),
        ("twice, different, side by side, first", [m(ent("k", one), ent("k", two), ent("j", three)), L]),
        ("twice, different, side by side, last", [m(ent("j", three), ent("k", one), ent("k", two)), L]),
        ("twice, different, apart", [m(ent("k", one), ent("j", three), ent("k", two)), L]),
        ("twice, equal, apart", [m(ent("k", one), ent("j", three), ent(other, two), ent("k", one)), L]),
        ("three times", [m(ent("k", one), ent("k", two), ent("j", two), ent("k", three)), L]),
        ("three times, the first and the last equal", [m(ent("k", one), ent("j", two), ent("k", two), ent("k", one)), L]),
        ("only the key, twice", [m(ent("k", one), ent("k", two)), L]),
        ("a key only the request knows, twice", [m(ent(other, one), ent("k", two), ent(other, three)), L]),
        ("the empty key twice", [m(ent("", one), ent("k", two), ent(None, three)), L]),
        ("null then a value", [m(ent("k", b""), ent("j", one), ent("k", two)), L]),
        ("a value then null", [m(ent("k", two), ent("j", one), ent("k", b"\x08\x00")), L]),
        ("a container then a scalar", [m(ent("k", list_of(one, two)), ent("j", one), ent("k", two)), L]),
        ("a scalar then a container", [m(ent("k", two), ent("j", one), ent("k", struct_of(ent("q", one)))), L]),
        ("containers, then a sibling behind them", [m(ent("k", list_of(one, list_of(two))), ent("k", list_of(three)), ent("j", struct_of(ent("q", list_of(one))))), L]),
        ("in a map inside a list", [m(ent("j", two), ent("k", one)), ent("l", list_of(struct_of(ent("q", one), ent("q", two)), two), 4)]),
        ("in a map inside the map", [m(ent("j", struct_of(ent("q", one), ent("r", two), ent("q", three))), ent("k", one)), L]),
        ("sixty-five entries of one key", [m(*([ent("j", two)] + [ent("k", num(float(i))) for i in range(65)])), L]),
        ("the last of many", [m(*([ent("f%03d" % i, num(float(i))) for i in range(40)] + [ent("k", one), ent("f005", three), ent("k", two)])), L]),
        ("at the top: m twice", [m(ent("k", one)), L, m(ent("k", two), ent("j", one))]),
        ("at the top: m twice, side by side, a scalar last", [m(ent("k", one)), ent("m", two, 4), L]),
        ("at the top: l three times", [ent("l", list_of(one), 4), m(ent("k", one)), ent("l", list_of(two, one), 4), ent("l", list_of(one, two, three), 4)]),
        ("at the top and below", [m(ent("k", one), ent("k", two)), L, m(ent("k", three), ent("j", one), ent("k", one))]),
    ]

    def has_repeated_key(entries):
        """whether any map of the message holds a key twice (every map of these stores reaches the heap: R.attr is read whole)"""
        def in_map(ents):
            keys = []
            for e in ents:
                key, vals = b"", []
                for n_, w_, v in pb_fields(e):
                    if n_ == 1 and w_ == 2:
                        key = v
                    elif n_ == 2 and w_ == 2:
                        vals.append(v)
                keys.append(key)
                if any(in_value(v) for v in vals[-1:]):
                    return True
            return len(set(keys)) != len(keys)

        def in_value(v):
            last = None
            for n_, w_, x in pb_fields(v):
                if VALUE_WIRE_TYPES.get(n_) == w_:
                    last = (n_, x)
            if last is None or last[0] < 5:
                return False
            kids = [e for n_, w_, e in pb_fields(last[1]) if n_ == 1 and w_ == 2]
            return in_map(kids) if last[0] == 5 else any(in_value(k) for k in kids)
        return in_map([e[2] for e in pb_fields(b"".join(entries))])
    spec = wire_spec("dup_keys", cases, host_if=has_repeated_key)
    assert len(spec.host) == len(spec.inputs) - 6, (len(spec.host), len(spec.inputs))       # all but the control's messages (a wide map among them: one reason or the other)
    return spec


WIDE_CONDS = {k: WIRE_CONDS[k] for k in ("c_sel", "c_has", "d_idx", "d_sel", "d_has", "size", "one")}
WIDE_MAPS = ((255, False), (255, True), (256, False), (256, True), (256, None), (257, False), (1000, False), (1000, True), (1000, None), (5000, False), (5000, True))   # (None: without the key `k`)


def make_wide():
    """maps of thousands of distinct keys, without a repeat and with ONE at the very end (the wanted key, first on the wire, comes
    again with another value): the device flattener's search for a repeated key is bounded by WIRE_MAX_MAP_ENTRIES wire entries per map,
    a wider map is the host flattener's whether it repeats a key or not - what stays on the device road is 255 and 256 distinct keys"""
    one, two = num(1.5), num(2.5)
    messages, groups, host = [], {}, set()
    for n, repeat in WIDE_MAPS:
        entries = [ent("k" if repeat is not None else "q", one)] + [ent("w%05d" % j, num(float(j))) for j in range(n - 1)] + ([ent("k", two)] if repeat else [])
        attr = [ent("m", struct_of(*entries), 4)]
        for key, w in (("k", 2.5 if repeat else 1.5), ("k", 3.5), ("w%05d" % (n - 2), float(n - 2)), ("w%05d" % n, 1.5)):
            rid = "wide%d_%s/%s/%s" % (n, repeat, key, w)
            messages.append(raw_message(rid, list(WIDE_CONDS), {"key": key, "w": w, "n": float(n if w != 3.5 else n + 1)}, attr))
            grouped(groups, "", rid, WIDE_CONDS)
            if repeat or n + bool(repeat) > WIRE_MAX_MAP_ENTRIES:
                host.add(rid)
    spec = Spec("wide", WIDE_CONDS, messages=messages, groups=groups, wire_only=True, host={r for r in host if r.startswith("wide255_")})
    assert spec.host == host and len(host) == 4 * 8, len(spec.host)      # (the repeat within the bound handed over; the wide ones by has_wide_map and by the line above)
    return spec


def make_merge_cases():
    """protobuf MERGES two struct_value / list_value members of one Value and two value fields of one entry; both flatteners take the
    last occurrence whole, and so does the decoder above: this layer pins that the two wire roads read such bytes ALIKE"""
    one, two, three = num(1.5), num(2.5), num(3.5)
    cases = [
        ("two struct_value members", [ent("m", struct_of(ent("j", two)) + struct_of(ent("k", one)), 4), ent("l", list_of(one), 4)]),
        ("two struct_value members, nested", [ent("m", struct_of(ent("k", struct_of(ent("a", one)) + struct_of(ent("b", two))), ent("j", one)), 4), ent("l", list_of(one), 4)]),
        ("two list_value members", [ent("m", struct_of(ent("k", one)), 4), ent("l", list_of(one, two) + list_of(three), 4)]),
        ("two value fields in an entry", [ent("m", struct_of(_ld(1, _ld(1, b"k") + _ld(2, struct_of(ent("a", one))) + _ld(2, struct_of(ent("b", two)))), ent("j", one)), 4),
                                          _ld(4, _ld(1, b"l") + _ld(2, list_of(one, two)) + _ld(2, list_of(three)))]),
        ("two struct_value members, the key in the first", [ent("m", struct_of(ent("k", one)) + struct_of(ent("j", two)), 4), ent("l", list_of(one) + list_of(), 4)]),
        ("control", [ent("m", struct_of(ent("j", two), ent("k", one)), 4), ent("l", list_of(one, two), 4)]),
    ]
    return wire_spec("merge_cases", cases)


MAKERS = {
    "access": make_access, "access_wire": make_access_wire, "select": make_select, "paths": make_paths,
    "depth": lambda: make_depth("depth", (1, 2, 7, 8), False), "depth9": lambda: make_depth("depth9", (9,), True),
    "sizes": make_sizes, "equality": lambda: make_equality("equality", EQ_PAIRS), "equality_wire": lambda: make_equality("equality_wire", EQ_WIRE_PAIRS, wire_only=True),
    "flat": make_flat, "wire_forms": make_wire_forms, "dup_keys": make_dup_keys, "wide": make_wide, "merge_cases": make_merge_cases,
}
_SPECS = {}


def spec_of(name):
    if name not in _SPECS:
        _SPECS[name] = MAKERS[name]()
    return _SPECS[name]


def layer(name, road):
    return spec_of(name).layer(road)


CASES = [(name, road) for name in MAKERS for road in (("f",) if name == "flat" else ("w", "g"))]
IDS = ["%s_%s" % c for c in CASES]


# ---- CPU tier: what the generators must make happen


@pytest.mark.parametrize("name,road", CASES, ids=IDS)
def test_the_oracle_decides_and_the_pairs_discriminate(name, road):
    layer(name, road).check_oracle()


def test_errors_are_where_cel_puts_them():
    """hand-worked corners of the oracle's answers, so that the reference is not taken on trust where the kernels are most likely to
    differ: which indices are errors, what `has` says of a null value, what a repeated key reads as"""
    lay = layer("access", "w")
    for inp, w in zip(lay.inputs, lay.want):
        l, i = inp["resource"]["attr"].get("l"), inp["resource"]["attr"].get("i")
        ok = isinstance(l, list) and isinstance(i, float) and i == int(i) and 0 <= i < len(l)
        assert ((inp["requestId"], "dbl") in lay.errors) == (not ok), (inp["requestId"], i, len(l) if isinstance(l, list) else l)
    lay = layer("access_wire", "w")
    for inp in lay.inputs:
        i = inp["resource"]["attr"]["i"]
        assert ((inp["requestId"], "dbl") in lay.errors) == (i != 0.0 or not inp["resource"]["attr"]["l"]), inp["requestId"]
    lay = layer("select", "w")
    for inp, w in zip(lay.inputs, lay.want):
        m = inp["resource"]["attr"].get("m")
        if isinstance(m, dict):
            for a in ("c_has", "d_has"):       # has() of a key whose value is null is TRUE
                assert (w["actions"][a]["effect"] == "EFFECT_ALLOW") == ("k" in m), (inp["requestId"], a)
            assert (w["actions"]["d_in"]["effect"] == "EFFECT_ALLOW") == (isinstance(inp["principal"]["attr"]["key"], str) and inp["principal"]["attr"]["key"] in m), inp["requestId"]
    lay = layer("dup_keys", "w")
    want = {"twice, different, side by side, first/k/True": 2.5, "three times/k/True": 3.5, "twice, different, apart/k/True": 2.5}
    for inp in lay.inputs:
        if inp["requestId"] in want:
            assert inp["resource"]["attr"]["m"]["k"] == want.pop(inp["requestId"]) == inp["principal"]["attr"]["w"]
            assert inp["principal"]["attr"]["n"] == 2.0
    assert not want


def test_the_flagged_set_is_the_rule():
    """the predicted flagged pairs, hand-worked for the corners of the rule"""
    assert equality_is_flagged([[1.0]], [[1.0]]) and equality_is_flagged([1.0, [2.0]], [1.0, [2.0]]) and equality_is_flagged({}, {})
    assert not equality_is_flagged([1.0, [2.0]], [2.0, [2.0]])       # left at the first unequal pair
    assert not equality_is_flagged([[1.0]], [[1.0], 2.0]) and not equality_is_flagged([1.0], {"a": 1.0}) and not equality_is_flagged([[1.0]], 1.0)
    assert equality_is_flagged([[1.0]], [1.0]) and not in_is_flagged([1.0], [[1.0]]) and in_is_flagged([[1.0]], [[[1.0]]])
    assert not in_is_flagged(1.0, [1.0, [2.0]]) and not in_is_flagged(1.0, [2.0, [1.0]]) and in_is_flagged([1.0], [[1.0, 2.0], [[1.0]], [1.0]])
    lay = layer("equality", "w")
    assert {a for _, a in lay.over} >= {"eq", "ne", "eq_int", "in"} and lay.over


# ---- CPU tier: the kernels on the wave emulator; the library on the simulator


@pytest.mark.parametrize("name,road", CASES, ids=IDS)
def test_on_emulator(name, road):
    run_on_emulator(layer(name, road))


@pytest.fixture()
def engine():
    from sim_engine import sim_engine
    with sim_engine() as capi:
        yield capi


@pytest.mark.parametrize("name,road", CASES, ids=IDS)
def test_on_simulator(engine, name, road):
    run_on_library(engine, layer(name, road))


# ---- 6. trace: the text of `no such key`


TRACE_CONDS = {"sel": "cel.bind(x, R.attr.m, x.known) == 1.5", "idx": "R.attr.m[P.attr.key] == 1.5", "l_sel": "R.attr.l[0].known == 1.5", "l_idx": "R.attr.l[0][P.attr.key] == 1.5"}
TRACE_KEYS = ("known", ONLY_REQUEST, "", "j", 1.0, True)      # a string of the table; a batch-local id in the error's detail bits; found; no strings
TRACE_INCOMPLETE = {4, 5}                                        # a key that is no string: CBH_ERR_OTHER, reported incomplete - never a wrong text


def trace_layer():
    if "trace" not in _SPECS:
        rt = rule_table_from_policies(policies_from_docs(cond_store(KIND, TRACE_CONDS)))
        inputs = [request("t%d" % k, KIND, list(TRACE_CONDS), pattr={"key": key}, rattr={"m": {"j": 1.5}, "l": [{"j": 1.5}, {"known": 1.5}]}) for k, key in enumerate(TRACE_KEYS)]
        orc = RuleTableOracle(rt)
        want = [orc.check(i, EvalParams(now_ns=NOW)) for i in inputs]
        _SPECS["trace"] = (lower_rule_table(rt), inputs, want)
    return _SPECS["trace"]


def test_trace_the_oracle_names_the_keys():
    """hand-worked: what the texts must be"""
    _, inputs, want = trace_layer()
    texts = [{e["celError"]["expression"]: e["celError"]["message"] for e in w["evaluationErrors"]} for w in want]
    assert texts[0] == {TRACE_CONDS[a]: "no such key: known" for a in TRACE_CONDS}
    assert texts[1] == {TRACE_CONDS[a]: "no such key: " + (ONLY_REQUEST if "idx" in a else "known") for a in TRACE_CONDS}
    assert texts[2][TRACE_CONDS["idx"]] == "no such key: " and set(texts[3]) == {TRACE_CONDS["sel"], TRACE_CONDS["l_sel"]}
    assert texts[4][TRACE_CONDS["idx"]] == "no such key: 1" and texts[5][TRACE_CONDS["l_idx"]] == "no such key: true"


def check_trace(ev):
    """cbh_trace_batch through trace.py (check) and through cbi_trace_pb (check_pb): the oracle's evaluation_errors, or incomplete"""
    _, inputs, want = trace_layer()
    outs, bad, incomplete = ev.check(inputs, now_ns=NOW, allow_unsupported=True, trace=True)
    assert not bad and {i: set(w) for i, w in incomplete.items()} == {i: {"errors"} for i in TRACE_INCOMPLETE}, (bad, incomplete)
    data, off = wire.pack_messages([wire.encode_check_input(i) for i in inputs])
    raw, flags = ev.check_pb(data, off, now_ns=NOW, trace=True)
    for k, (have, w) in enumerate(zip(outs, want)):
        pb = wire.decode_check_output(raw[k])
        for got, what in ((have, "trace.py"), (pb, "cbi_trace_pb")):
            assert {a: e["effect"] for a, e in got["actions"].items()} == {a: e["effect"] for a, e in w["actions"].items()}, (k, what)
        assert bool(int(flags[k]) & 4) == (k in TRACE_INCOMPLETE) and not int(flags[k]) & 1, (k, int(flags[k]))     # CBI_TRACE_ERRORS_INCOMPLETE, never CBI_OUT_UNSUPPORTED
        if k not in TRACE_INCOMPLETE:
            assert have["evaluationErrors"] == w["evaluationErrors"], (k, "trace.py", have["evaluationErrors"])
            assert (pb.get("evaluationErrors") or []) == w["evaluationErrors"], (k, "cbi_trace_pb", pb.get("evaluationErrors"))
        else:       # what IS reported is the oracle's, the rest is missing and said to be
            assert all(e in w["evaluationErrors"] for e in have["evaluationErrors"]) and len(have["evaluationErrors"]) < len(w["evaluationErrors"]), k


def test_trace_on_emulator():
    import test_trace_pass as tp
    from cerbos_amd.engine import Conf
    assert header_value("CBI_TRACE_ERRORS_INCOMPLETE", "../../include/cerbos_ingest.h") == 4
    check_trace(tp._HostSimBytes(trace_layer()[0], Conf()))


@pytest.mark.gpu
def test_trace_on_gpu():
    from cerbos_amd.engine import Conf, HipEvaluator
    ev = HipEvaluator(trace_layer()[0], Conf())
    try:
        check_trace(ev)
    finally:
        ev.close()


# ---- GPU tier


@pytest.mark.gpu
@pytest.mark.parametrize("name,road", CASES, ids=IDS)
def test_on_gpu(name, road):
    from cerbos_amd import capi       # (CBH_TEST_SIM_ENGINE=1, the developer's aid of tests/conftest.py: the simulator)
    run_on_library(capi, layer(name, road))
