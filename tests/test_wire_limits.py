"""The wire kernels of cbh_wire.h at their byte boundaries: serialized CheckInputs in, serialized CheckOutputs out, against a plain reader.

What is aimed at: the way in (cbh_wire_count_kernel, cbh_wire_scan_kernel, w_stage_block, cbh_wire_fill_kernel / cbh_wire_fill_lds_kernel)
and the way back (w_output, WSink, cbh_wire_out_size_kernel, cbh_wire_out_scan_kernel, cbh_wire_out_write_kernel).  The tests the suite had
compare the device writer with the project's own host writer and the device flattener with the host flattener: a rule both sides got wrong
is invisible to them.  Here NOTHING of the project decodes or encodes on the reference side:

  pb_fields / read_input / read_output   a protobuf-way reader (varints, the four wire types, the last field wins, unknown fields skipped):
                                         the bytes of a CheckInput -> the dict oracle/check.py takes; the bytes of a CheckOutput ->
                                         request id, resource id, the actions in wire order, the derived roles
  encode_output                          CheckOutput with minimal varints: fields 1, 2, 3 (the map entry: key, ActionEffect{effect, policy,
                                         scope}) and 4; empty strings and a zero effect are left out, a map entry always has its two fields

Per input of every call (judge): the device's bytes decode to what the oracle says for the DECODED input (effect, policy key, scope,
effectiveDerivedRoles; an action named twice folded as check.go:513-530 - the oracle's set_effect); the device's bytes ARE the plain
encoder's (canonical form, first-appearance order, no stray byte); the offsets are the running sum of the sizes; the flags are what the
statuses predict (the oracle's evaluationErrors -> CBI_OUT_CEL_ERROR; on the emulator also the fold of the kernels' own statuses); and the
host road (cbi_flatten_pb -> the decision kernels -> cbi_assemble_pb) gives the same bytes.  Every call asserts how many inputs it decided.
effectiveDerivedRoles: the reference ranges over a Go map (check.go:86-88), so any order is its order; the project writes the
roles in the order of their definitions, and that is the order the expectation puts the oracle's SET in (from the documents, not the table).

Stores (the module's own): MAIN - flat tables for the kinds `k`, `t` (typed attribute), kinds whose names give the policy key every length
the varint steps ask for, a kind with scoped policies of 1, 127, 128, 16 383 and 16 384 bytes, a policy version and a principal id of the pre-0.30 form;
DR3 - four derived roles whose names are 127, 128, 16 383 and 16 384 bytes; DR63 / DR64 - exactly 63 and 64 derived roles.  Conditions read
P.attr.first - the FIRST field of every message the module builds - and R.attr.last - its LAST bytes: a block staged one chunk short or
read at a wrong bias changes a decision, not only a span.

Tiers.  test_on_emulator: the kernels' source on tests/hostsim (CBH_WIRE_LDS_CAP sets both staging caps; the output buffer at every
offset 0..15).  test_on_simulator: the library on tests/sim_engine.py for the calls whose point is the library's own choice of a cap
(wire_lds_cap, wire_fill_lds_cap, the count kernel's estimate).  test_on_gpu: every call through the C ABI (cbh_wire_flatten ->
cbh_check_resident -> cbh_wire_outputs, and cbh_wire_check_pb into the caller's buffers); CBH_TEST_SIM_ENGINE=1 runs these bodies on the
simulator build.  Results cannot be handed to the library from outside, so the cases that need made-up results - every order of ALLOW and
DENY among repeats of one action, statuses of dropped duplicates, a derived-role bit the table has no name for, CBH_WO_MAX_OUTPUT - run on
the emulator alone (test_made_up_*); a repeated action the road itself decides gets one effect at every place.
WHICH messages a call leaves to the host flattener is checked on the emulator, by their status bytes; the C ABI gives the count alone
(cbh_wire_info.n_host), so the library tiers assert the count, that the call returns 1, and that every other message alone is decided.

What the road's limits do not allow, said here and not skipped silently:
  * a wave total of 1 byte: the smallest CheckOutput that is not empty has 3 bytes (`0A 01 x`); 3 stands in for 1.
  * one byte behind the last field of a message: a protobuf field has at least two; the trailing bytes are 0 and 2..8.
  * a run of forbidden bytes at the START of a name that is rewritten: every segment of a name of the pre-0.30 form begins with a letter
    (w_kind_needs_rewrite: `if (seg_start) { if (!alpha) return false; ..`), so a name that begins with such a run is not rewritten at all;
    the version `--rc:x` is asserted to be written as it is.  Runs inside, next to each other and at the end are rewritten.
  * a run of bytes >= 0x80 in a name that is rewritten: such a byte makes the name NOT of the pre-0.30 form (w_kind_needs_rewrite), the
    name is written as it is - that is what is asserted.
  * CBH_WO_MAX_OUTPUT (0xFFFFFF) is NOT reachable through the road's limits: the lowering writes every policy key with a 16-bit length
    (lower/blob.py _names), so the key of a policy that can match - kind, version and scope together - has at most 65 535 bytes, its scope
    fewer, and 64 actions come to less than 64 * (3 * 65 535 + 40) = 12.6 MB.  The bound and its error are asserted with made-up results
    on the emulator (test_made_up_output_too_large: a key built from a 65 535-byte kind AND version of the message, which no table holds);
    the largest output the module sends down the real road is the 4 MB one (64 actions of 65 535 bytes).  The largest key a table can
    hold (65 535 bytes) is in the length call.

What was found.  The kernels wrote no wrong byte.  The HOST writer refused a call in which no input has an action (the scan and skew
calls: every CheckOutput is a request id): cbi_assemble_pb answered "null argument" to the empty effect array where the device writer
writes the outputs; it, cbi_assemble_wire_pb and cbi_assemble_response_pb now want the array only when there are tuples.

Mutation check (each mutant on a scratch copy of cbh_wire.h, CPU tier, never committed).  Killed:
   a  w_varint_size `>=` as `>`                      test_on_emulator[lengths | rewritten_lengths], test_made_up_folds_across_the_register_file
   b  `k < CBH_WO_FAST_ACTIONS` as `<=`, each site   kf / jf and eff_of: test_on_emulator[lengths | largest | rewritten | actions | limits], the made-up folds;
                                                     id_of: test_on_emulator[actions], the folds; the status read: the folds alone (a dropped duplicate's flag)
   c  `a.n_dr >= 64u` as `>`                         test_on_emulator[derived_roles_64], test_made_up_derived_role_masks[64]
   d  out_len replaced by len (w_policy_key_len)     test_on_emulator[rewritten | rewritten_lengths], the made-up folds
   e  the fold's `||` as `&&`                        test_made_up_folds_across_the_register_file
   f  the copy-out without `o16 >= skew`             test_on_emulator[skews_* | staging_* | mixed_staging | offsets | windows | scan_*] (the wave before loses its tail)
   g  `o16 + 16u <= end` as `o16 <= end`             test_on_emulator[skews_* | staging_* | rewritten | derived_roles_64 ..] (bytes behind the outputs: the guard bytes of
                                                     wire_device_util.sim_outputs, and the next wave's head)
   h  the first / last chunk one byte short          test_on_emulator[skews_* | staging_* | offsets | windows ..]
   i  the out scan's sixteenth sum kept out of `p`   test_on_emulator[scan_1025]; the sixteenth sum kept out of `s`: the process aborts on scan_961 (the
                                                     outputs overrun the buffer the short total sized)
   j  the in scan's fourth W_STORE4 dropped          test_on_emulator[scan_449 | scan_512 | scan_513]; its eighth sum dropped: the process aborts (arrays sized by
                                                     the short totals are overrun)
   k  w_varint_long: the ninth byte's bits dropped   test_on_emulator[windows]
   l  the simulator's w_stage_block one chunk short  nearly every test_on_emulator case (R.attr.last is in the last chunk)
   m  na > 64 / nr > 255 / len > 65 535 as `>=`      test_on_emulator[limits | largest | actions | lengths]
   n  `sz > CBH_WO_MAX_OUTPUT` as `>=`               test_made_up_output_too_large
Survive, and must - both sides of the condition give the same bytes, so no comparison of outputs can tell them apart:
   o  the `+ 16u` dropped from either staging bound (count kernel, fill kernel) and from `total + skew + 16u <= lds_cap`: the margin is
      for whole 16-byte chunks at the block's end; the block is parsed / written alike staged or in place, and the simulator's LDS is
      larger than any cap (on the device the chunk would leave the kernel's allocation by up to 15 bytes)
   p  `o16 + 16u <= end` as `<`, `o16 >= skew` as `>`: the chunk goes the byte-wise way, which writes the same bytes
   q  the scans' `w + 16u <= hi` / `w + 8u <= hi` as `<`: the last full round is done by the one-at-a-time loop behind it
   r  `staged` as `hi64 >= lo64`, `fits` as `hi64 > lo64`: a wave of empty messages has nothing to parse either way
   s  lo16 without its mask (both kernels), skew without out_bias: on the simulator a copy is a copy at any alignment
Lines inside `#ifndef CBH_HOSTSIM` cannot be mutated on the CPU and are covered by the GPU run alone: w_stage_block's
`global_load_lds` loop and its wait, the `v4` LDS-to-global copy of cbh_wire_out_write_kernel, W_LOAD4 / W_STORE4 as 16-byte accesses at
4-byte alignment, the 16-byte loads of w_output's spans and of w_table_sid, the count kernel's 16-byte wavesum store; and (s) - the
alignment of the staged block and of the copy-out only matters there.
"""
import os
import re
import struct

import numpy as np
import pytest

import hostsim_api
import wire_device_util as wu
from cerbos_amd.ingest import IngestTable
from cerbos_amd.lower.blob import lower_rule_table
from cerbos_amd.policy.loader import policies_from_docs
from cerbos_amd.ruletable.build import rule_table_from_policies
from helpers import load_json
from oracle.check import EvalParams, RuleTableOracle
from test_string_limits import header_value

API = "api.cerbos.dev/v1"
NOW = 1_700_000_000_000_000_000
F_WANT_DR = 4
ALLOW, DENY = 1, 2
EFFECT = {"EFFECT_ALLOW": ALLOW, "EFFECT_DENY": DENY}
ST_OK, ST_CEL_ERROR, ST_UNSUPPORTED, ST_WANTS_TRACE = 0, 1, 2, 3
OUT_FLAG = {ST_OK: 0, ST_CEL_ERROR: 2, ST_UNSUPPORTED: 1, ST_WANTS_TRACE: 16}      # include/cerbos_ingest.h CBI_OUT_*
P_RESOURCE, NONE = 2, 0xFFFFFFFF
MAX_STRLEN, MAX_ACTIONS, MAX_ROLES, FAST_ACTIONS, MAX_OUTPUT, SLACK = 0xFFFF, 64, 255, 4, 0xFFFFFF, 8
STEPS = (127, 128, 16383, 16384)


def test_the_limits_are_the_headers():
    assert header_value("CBH_WIRE_MAX_STRLEN", "cbh_wire.h") == MAX_STRLEN and header_value("CBH_WIRE_MAX_ROLES", "cbh_wire.h") == MAX_ROLES
    assert header_value("CBH_WO_FAST_ACTIONS", "cbh_wire.h") == FAST_ACTIONS and header_value("CBH_WO_MAX_OUTPUT", "cbh_wire.h") == MAX_OUTPUT
    assert header_value("CBH_WIRE_SLACK", "cbh_wire.h") == SLACK
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "cerbos_hip.h")) as fh:
        assert int(re.search(r"#define\s+CBH_MAX_ACTIONS_PER_REQUEST\s+(\d+)", fh.read()).group(1)) == MAX_ACTIONS


# ---- the reference: a plain reader and a plain encoder


def pb_fields(buf):
    """(number, wire type, value) of every field: a varint's value, the 8 / 4 bytes of a fixed one, a length-delimited payload"""
    i, n = 0, len(buf)

    def varint_at():
        nonlocal i
        v = shift = 0
        while True:
            b = buf[i]
            i += 1
            v |= (b & 0x7F) << shift
            shift += 7
            if not b & 0x80:
                return v & ((1 << 64) - 1)
    while i < n:
        key = varint_at()
        num, wt = key >> 3, key & 7
        if wt == 0:
            yield num, wt, varint_at()
        elif wt == 1:
            yield num, wt, bytes(buf[i:i + 8])
            i += 8
        elif wt == 5:
            yield num, wt, bytes(buf[i:i + 4])
            i += 4
        else:
            assert wt == 2, wt
            ln = varint_at()
            assert i + ln <= n
            yield num, wt, bytes(buf[i:i + ln])
            i += ln


VALUE_WIRE_TYPES = {1: 0, 2: 1, 3: 2, 4: 0, 5: 2, 6: 2}      # google/protobuf/struct.proto: null, number, string, bool, struct, list


def read_value(buf):
    out = None
    for num, wt, v in pb_fields(buf):
        if VALUE_WIRE_TYPES.get(num) != wt:
            continue
        if num == 1:
            out = None
        elif num == 2:
            out = struct.unpack("<d", v)[0]
        elif num == 3:
            out = v.decode()
        elif num == 4:
            out = bool(v)
        elif num == 5:
            out = read_map(e for n2, w2, e in pb_fields(v) if n2 == 1 and w2 == 2)
        else:
            out = [read_value(e) for n2, w2, e in pb_fields(v) if n2 == 1 and w2 == 2]
    return out


def read_map(entries):
    out = {}
    for ent in entries:
        key, val = "", None
        for num, wt, v in pb_fields(ent):
            if num == 1 and wt == 2:
                key = v.decode()
            elif num == 2 and wt == 2:
                val = read_value(v)
        out.pop(key, None)
        out[key] = val
    return out


def read_input(msg):
    """engine.proto CheckInput {1 request_id, 2 resource {1 kind, 2 policy_version, 3 id, 4 attr, 5 scope}, 3 principal {1 id,
    2 policy_version, 3 roles, 4 attr, 5 scope}, 4 actions} -> the oracle's dict"""
    inp = {"requestId": "", "actions": [], "principal": {"id": "", "policyVersion": "", "scope": "", "roles": [], "attr": {}},
           "resource": {"kind": "", "policyVersion": "", "id": "", "scope": "", "attr": {}}}
    for num, wt, v in pb_fields(msg):
        if wt != 2:
            continue
        if num == 1:
            inp["requestId"] = v.decode()
        elif num == 4:
            inp["actions"].append(v.decode())
        elif num in (2, 3):
            part = inp["resource" if num == 2 else "principal"]
            part.update({"roles": [], "attr": {}} if num == 3 else {"attr": {}})      # (a part that comes twice: this reads the last whole; no message here has two)
            names = {1: "kind", 2: "policyVersion", 3: "id", 5: "scope"} if num == 2 else {1: "id", 2: "policyVersion", 5: "scope"}
            attrs = []
            for n2, w2, x in pb_fields(v):
                if w2 != 2:
                    continue
                if n2 in names:
                    part[names[n2]] = x.decode()
                elif n2 == 3:
                    part["roles"].append(x.decode())
                elif n2 == 4:
                    attrs.append(x)
            part["attr"] = read_map(attrs)
    return inp


def read_output(buf):
    """engine.proto CheckOutput -> request id, resource id, [(action, effect, policy, scope)] in wire order, derived roles"""
    out = {"requestId": "", "resourceId": "", "actions": [], "effectiveDerivedRoles": []}
    for num, wt, v in pb_fields(buf):
        if wt != 2:
            continue
        if num == 1:
            out["requestId"] = v.decode()
        elif num == 2:
            out["resourceId"] = v.decode()
        elif num == 4:
            out["effectiveDerivedRoles"].append(v.decode())
        elif num == 3:
            name, eff = "", (0, "", "")
            for n2, w2, x in pb_fields(v):
                if n2 == 1 and w2 == 2:
                    name = x.decode()
                elif n2 == 2 and w2 == 2:
                    e, p, s = 0, "", ""
                    for n3, w3, y in pb_fields(x):
                        if n3 == 1 and w3 == 0:
                            e = y
                        elif n3 == 2 and w3 == 2:
                            p = y.decode()
                        elif n3 == 3 and w3 == 2:
                            s = y.decode()
                    eff = (e, p, s)
            out["actions"].append((name,) + eff)
    return out


def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def ld(num, payload):
    return varint(num << 3 | 2) + varint(len(payload)) + payload


def text(num, s):
    """a string field as a marshaller writes it: not at all when it is empty"""
    s = s.encode() if isinstance(s, str) else s
    return ld(num, s) if s else b""


def encode_output(rid, resid, actions, roles):
    out = text(1, rid) + text(2, resid)
    for name, effect, policy, scope in actions:
        ae = (b"\x08" + varint(effect) if effect else b"") + text(2, policy) + text(3, scope)
        out += ld(3, ld(1, name.encode()) + ld(2, ae))
    return out + b"".join(ld(4, r.encode()) for r in roles)


def enc_value(v):
    if v is None:
        return b"\x08\x00"
    if isinstance(v, bool):
        return b"\x20" + (b"\x01" if v else b"\x00")
    if isinstance(v, (int, float)):
        return b"\x11" + struct.pack("<d", float(v))
    if isinstance(v, str):
        return ld(3, v.encode())
    if isinstance(v, list):
        return ld(6, b"".join(ld(1, enc_value(x)) for x in v))
    return ld(5, b"".join(ld(1, ld(1, k.encode()) + ld(2, enc_value(x))) for k, x in v.items()))


def attr_entry(key, value_bytes):
    return ld(4, ld(1, key.encode()) + ld(2, value_bytes))


def build_input(inp):
    """a CheckInput dict in the fields' declared order (the pin test's writer; the calls build theirs with message())"""
    p, r = inp.get("principal") or {}, inp.get("resource") or {}
    res = text(1, r.get("kind", "")) + text(2, r.get("policyVersion", "")) + text(3, r.get("id", "")) + \
        b"".join(attr_entry(k, enc_value(v)) for k, v in (r.get("attr") or {}).items()) + text(5, r.get("scope", ""))
    pri = text(1, p.get("id", "")) + text(2, p.get("policyVersion", "")) + b"".join(ld(3, x.encode()) for x in p.get("roles") or []) + \
        b"".join(attr_entry(k, enc_value(v)) for k, v in (p.get("attr") or {}).items()) + text(5, p.get("scope", ""))
    return text(1, inp.get("requestId", "")) + ld(2, res) + ld(3, pri) + b"".join(ld(4, a.encode()) for a in inp.get("actions") or [])


def test_the_reader_and_the_encoder_on_the_golden_fixtures():
    """hand-worked bytes first, then the reference's engine cases (tests/golden/engine_cases.json): every input read back from bytes is the
    fixture, every wanted output survives encode -> read, and - in this test alone - the project's codec agrees on both"""
    from cerbos_amd import wire
    assert varint(127) == b"\x7f" and varint(128) == b"\x80\x01" and varint(16383) == b"\xff\x7f" and varint(16384) == b"\x80\x80\x01"
    assert encode_output("q", "", [("a", ALLOW, "p", "")], ["d"]) == b"\x0a\x01q\x1a\x0a\x0a\x01a\x12\x05\x08\x01\x12\x01p\x22\x01d"
    assert encode_output("", "", [("", 0, "", "")], []) == b"\x1a\x04\x0a\x00\x12\x00"
    assert read_output(b"\x0a\x01x\x0a\x01q\x78\x05\x1a\x0a\x0a\x01a\x12\x05\x08\x02\x1a\x01s") == \
        {"requestId": "q", "resourceId": "", "actions": [("a", DENY, "", "s")], "effectiveDerivedRoles": []}      # last wins; field 15 skipped
    assert read_input(b"\x22\x01a\x0a\x01x\x22\x01b\x1a\x07\x1a\x01r\x0a\x02id")["actions"] == ["a", "b"]
    assert read_input(b"\x1a\x07\x1a\x01r\x0a\x02id")["principal"] == {"id": "id", "policyVersion": "", "scope": "", "roles": ["r"], "attr": {}}
    n_in = n_out = 0
    for case in load_json("engine_cases.json"):
        for inp in case["inputs"]:
            if "auxData" in inp:
                continue
            want = read_input(b"")
            want.update(requestId=inp.get("requestId", ""), actions=list(inp.get("actions") or []))
            for part in ("principal", "resource"):
                want[part].update(inp.get(part) or {})
            assert read_input(build_input(inp)) == want and read_input(wire.encode_check_input(inp)) == want
            n_in += 1
        for out in case.get("wantOutputs") or []:
            acts = [(a, EFFECT[e["effect"]], e.get("policy", ""), e.get("scope", "")) for a, e in out["actions"].items()]
            raw = encode_output(out.get("requestId", ""), out.get("resourceId", ""), acts, out.get("effectiveDerivedRoles") or [])
            back = read_output(raw)
            assert back["actions"] == acts and back["effectiveDerivedRoles"] == (out.get("effectiveDerivedRoles") or [])
            theirs = wire.decode_check_output(raw)
            assert theirs["requestId"] == out.get("requestId", "") and {a: EFFECT[e["effect"]] for a, e in theirs["actions"].items()} == {a: e for a, e, _, _ in acts}
            n_out += 1
    assert n_in > 40 and n_out > 40, (n_in, n_out)


# ---- stores


COND_LAST, COND_FIRST = 'R.attr.last == "yes"', 'P.attr.first == "no"'
PLAIN_RULES = [{"actions": ["*"], "roles": ["*"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": COND_LAST}}},
               {"actions": ["*"], "roles": ["*"], "effect": "EFFECT_DENY", "condition": {"match": {"expr": COND_FIRST}}}]
KEY_LENGTHS = (123, 124, 127, 128, 8190, 16378, 16379, 16383, 16384, MAX_STRLEN)      # policy keys `resource.<kind>.vdefault`: pol_l, eff_len, ent_len at their steps
OLD_VERSION, OLD_PRINCIPAL = "rc:v2024-01//b", "ali:ce@@x--"      # pre-0.30 forms (namer.go:213-218): runs inside, next to each other, at the end (a segment begins with a letter)
START_RUN = "--rc:x"      # a run at the START: the first segment does not begin with a letter, so the name is not of the old form
SCOPES = ("a", "b" * 127, "c" * 128, "d" * 16383, "e" * 16384)


def kind_of_key(n):
    return "K" * (n - 18)


def resource_policy(kind, rules=None, version="default", scope="", imports=()):
    body = {"resource": kind, "version": version, "rules": rules or PLAIN_RULES}
    if scope:
        body["scope"] = scope
    if imports:
        body["importDerivedRoles"] = list(imports)
    return {"apiVersion": API, "resourcePolicy": body}


class Store:
    def __init__(self, docs):
        self.rt = rule_table_from_policies(policies_from_docs(docs))
        self.lt = lower_rule_table(self.rt)
        assert not self.lt.unsupported, self.lt.unsupported
        self.orc = RuleTableOracle(self.rt)
        self.dr_order = [d["name"] for doc in docs if "derivedRoles" in doc for d in doc["derivedRoles"]["definitions"]]
        self.cache = {}

    def want(self, msg, dver):
        """the plain encoder's bytes of the oracle's answer to the DECODED message, and the flag its evaluation errors predict"""
        got = self.cache.get((msg, dver))
        if got is None:
            out = self.orc.check(read_input(msg), EvalParams(now_ns=NOW, default_policy_version=dver))
            acts = [(a, EFFECT[e["effect"]], e["policy"], e["scope"]) for a, e in out["actions"].items()]
            roles = sorted(out["effectiveDerivedRoles"], key=self.dr_order.index)
            got = self.cache[(msg, dver)] = (encode_output(out["requestId"], out["resourceId"], acts, roles), OUT_FLAG[ST_CEL_ERROR] if out["evaluationErrors"] else 0)
        return got


def main_docs():
    typed = [{"actions": ["b"], "roles": ["*"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": "R.attr.last == true"}}},
             {"actions": ["n"], "roles": ["*"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": "R.attr.last == 2.5"}}},
             {"actions": ["s"], "roles": ["*"], "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": 'R.attr.last in ["1234567", "12345678", "123456789"]'}}}]
    docs = [resource_policy("k"), resource_policy("t", typed), resource_policy("k", version=OLD_VERSION), resource_policy("k", version="a-é:x"), resource_policy("k", version=START_RUN)]
    docs += [resource_policy(kind_of_key(n)) for n in KEY_LENGTHS]
    docs += [resource_policy(kind, scope=s) for kind in ("s", kind_of_key(16384)) for s in ("",) + SCOPES if not (kind != "s" and s == "")]
    docs.append({"apiVersion": API, "principalPolicy": {"principal": OLD_PRINCIPAL, "version": "default", "rules": [
        {"resource": "pk", "actions": [{"action": "*", "effect": "EFFECT_ALLOW", "condition": {"match": {"expr": COND_LAST}}}]}]}})
    return docs


def dr_docs(names):
    defs = [{"name": n, "parentRoles": ["role%02d" % i], "condition": {"match": {"expr": COND_LAST}}} for i, n in enumerate(names)]
    rules = PLAIN_RULES + [{"actions": ["edit"], "derivedRoles": [n], "effect": "EFFECT_ALLOW"} for n in names]
    return [{"apiVersion": API, "derivedRoles": {"name": "many", "definitions": defs}}, resource_policy("k", rules, imports=["many"])]


DR3_NAMES = ("y" * 127, "x" * 128, "w" * 16383, "v" * 16384)      # (declared against the alphabet: the order written is the definitions', not a sort)
_STORES = {}
STORE_MAKERS = {"main": lambda: Store(main_docs()), "dr3": lambda: Store(dr_docs(DR3_NAMES)),
                "dr63": lambda: Store(dr_docs(["dr%02d" % i for i in range(63)])), "dr64": lambda: Store(dr_docs(["dr%02d" % i for i in range(64)]))}


def store(name):
    if name not in _STORES:
        _STORES[name] = STORE_MAKERS[name]()
    return _STORES[name]


# ---- messages: P.attr.first opens the message, R.attr.last closes it


def message(rid="q", actions=("view", "edit"), kind="k", res_id="r", first="yes", last="yes", roles=("user",), pid="p", pver="", rver="", rscope="",
            tail=None, junk=b""):
    """tail: the bytes of the Value of R.attr.last (else the string `last`; None for both: no such attribute); junk: an unknown field behind it"""
    principal = (attr_entry("first", ld(3, first.encode())) if first is not None else b"") + text(1, pid) + text(2, pver) + b"".join(ld(3, r.encode()) for r in roles)
    value = tail if tail is not None else (ld(3, last.encode()) if last is not None else None)
    resource = text(1, kind) + text(2, rver) + text(3, res_id) + text(5, rscope) + (attr_entry("last", value) if value is not None else b"")
    return ld(3, principal) + text(1, rid) + b"".join(ld(4, a.encode()) for a in actions) + ld(2, resource) + junk


def padded(total, **kw):
    """message(**kw) of exactly `total` bytes, by the length of its request id"""
    base = len(message(rid="", **kw))
    for n in (total - base - 2, total - base - 3, total - base - 4):
        if n >= 1 and len(message(rid="i" * n, **kw)) == total:
            return message(rid="i" * n, **kw)
    raise AssertionError("no request id makes %d bytes of %d" % (total, base))


def yes_no(k):
    return ("yes", "no")[k & 1], ("yes", "no")[(k >> 1) & 1]


def block(total, n=64, k0=0, **kw):
    """n messages of `total` bytes together: ordinary ones (both attributes, every combination of yes / no), the last one padded - its
    R.attr.last ends on the block's last byte"""
    full = max(1, min(n, (total - 100) // 80))      # (messages of some 70 bytes; where fewer fit, empty ones lead the wave)
    msgs = [b""] * (n - full)
    for k in range(full - 1):
        f, la = yes_no(k0 + k)
        msgs.append(message(rid="m%d" % k, first=f, last=la, **kw))
    f, la = yes_no(k0 + n)
    msgs.append(padded(total - sum(len(m) for m in msgs), first=f, last=la, **kw))
    return msgs


def sized(size):
    """a message whose CheckOutput has exactly `size` bytes: none, or a request id"""
    assert size == 0 or 3 <= size <= 129, size
    return text(1, "i" * (size - 2)) if size else b""


def wave_of_output(total):
    """64 messages whose outputs add up to `total` bytes (each 0 or 3..129)"""
    sizes, left = [], total
    while left > 0:
        s = min(left, 129)
        if 0 < left - s < 3:
            s = left - 3
        sizes.append(s)
        left -= s
    assert len(sizes) <= 64 and all(3 <= s <= 129 for s in sizes), total
    return [sized(s) for s in sizes + [0] * (64 - len(sizes))]


# ---- calls


class Call:
    """msgs: the serialized CheckInputs; host: the indices built to exceed a limit of the road (the call comes back 1 with n_host = their
    count, the others are then decided alone); cap: CBH_WIRE_LDS_CAP on the emulator, and - lds: "out" / "in" - the cap the library must
    choose by its own rule; biases: offsets of the output buffer on the emulator; decided: the inputs the call decides"""

    def __init__(self, store_name, msgs, dver="default", host=(), cap=16384, lds=None, biases=(0,)):
        self.store_name, self.msgs, self.dver, self.host, self.cap, self.lds, self.biases = store_name, list(msgs), dver, sorted(host), cap, lds, biases
        self.decided = len(self.msgs) - len(self.host)

    def store(self):
        return store(self.store_name)

    def packed(self, msgs=None):
        msgs = self.msgs if msgs is None else msgs
        off = np.zeros(len(msgs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(m) for m in msgs])
        return np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8)[:int(off[-1])].copy(), off

    def kept(self):
        return [m for i, m in enumerate(self.msgs) if i not in set(self.host)]


def wire_lds_cap(want):
    """cbh_host_wire.h:10-14 wire_lds_cap: a power of two from 4 096 to 49 152"""
    c = 4096
    while c < want and c < 49152:
        c <<= 1
    return min(c, 49152)


def out_lds_cap(total, n):
    """cbh_host_wire.h:566: 80 times the mean output size plus 256"""
    return wire_lds_cap(total // n * 80 + 256) if n else wire_lds_cap(0)


def fill_lds_cap(max_block, most=32768):
    """cbh_host_wire.h:19-24 wire_fill_lds_cap: max_block + 16 + CBH_WIRE_SLACK rounded up to 1 KB; 0 (parse in place) above 32 768"""
    if max_block == 0 or max_block > most:
        return 0
    c = (max_block + 16 + SLACK + 1023) & ~1023
    return 0 if c > most else c


def blocks_of(msgs):
    """per wave of 64 messages: the bytes from the 16-byte boundary below its first message to the end of its last (WireStats.max_block)"""
    off = np.concatenate([[0], np.cumsum([len(m) for m in msgs])])
    return [int(off[min(w + 64, len(msgs))]) - (int(off[w]) & ~15) for w in range(0, len(msgs), 64)]


def call_lengths():
    """A1: every length field of an output at 127 / 128 and 16 383 / 16 384 (strings up to 65 535), one at a time, then together"""
    msgs = []
    for n in STEPS + (MAX_STRLEN,):
        msgs.append(message(rid="i" * n))
        msgs.append(message(res_id="r" * n, last="no"))
        msgs.append(message(actions=("view", "n" * n, "edit")))
    for n in KEY_LENGTHS:      # pol_l, eff_len (2 + 1 + its varint + pol_l) at their steps
        msgs.append(message(kind=kind_of_key(n), last=("yes", "no")[n & 1]))
    for n in (100, 101):       # ent_len = 127 / 128 under `resource.k.vdefault` (eff_len 23)
        msgs.append(message(actions=("n" * n,)))
    for n in (8182, 8183):     # ent_len = 16 383 / 16 384 while its parts do not cross: name 8 18x, eff_len 8 195
        msgs.append(message(kind=kind_of_key(8190), actions=("view", "n" * n)))
    for s in SCOPES:
        msgs.append(message(kind="s", rscope=s))
        msgs.append(message(kind="s", rscope=s, last="no"))
    msgs.append(message(rid="i" * 16384, res_id="r" * 16384, kind=kind_of_key(16384), rscope="e" * 16384, actions=("n" * 128, "o" * 16384, "p" * MAX_STRLEN, "view", "q" * 127)))
    return Call("main", msgs)


def test_the_length_call_reaches_its_steps():
    """the expectation's own bytes: every varint step the issue names is met by some length field of some expected output"""
    c, d = call_lengths(), call_dr_names()
    seen = {"ent": set(), "eff": set(), "pol": set(), "name": set(), "scope": set(), "rid": set(), "res": set(), "role": set()}
    for cc, m in [(c, m) for m in c.msgs] + [(d, m) for m in d.msgs]:
        raw, _ = cc.store().want(m, cc.dver)
        for num, _, v in pb_fields(raw):
            if num == 4:
                seen["role"].add(len(v))
            if num in (1, 2):
                seen["rid" if num == 1 else "res"].add(len(v))
            if num == 3:
                seen["ent"].add(len(v))
                f = {n2: x for n2, _, x in pb_fields(v)}
                seen["name"].add(len(f[1]))
                seen["eff"].add(len(f[2]))
                for n3, w3, y in pb_fields(f[2]):
                    if w3 == 2:
                        seen["pol" if n3 == 2 else "scope"].add(len(y))
    for what, got in seen.items():
        want = {1} | set(STEPS) if what == "scope" else set(STEPS)
        assert want <= got, (what, sorted(want - got))
    assert MAX_STRLEN in seen["rid"] and MAX_STRLEN in seen["res"] and MAX_STRLEN in seen["name"]


def call_largest():
    """one input of 64 actions of 65 535 bytes: an output of 4 MB, the largest the module sends down the road"""
    return Call("main", [message(rid="first"), message(actions=["%02d" % k + "n" * (MAX_STRLEN - 2) for k in range(64)]), message(rid="last", last="no")])


def call_rewritten():
    """A2: keys that change length when written.  The version and the principal id of the pre-0.30 form, as the message's own and as the
    call's default; a name with a byte >= 0x80 stays as it is; kinds that make the key 127 / 128 bytes only AFTER the rewrite"""
    msgs = [message(rver=OLD_VERSION), message(rver=OLD_VERSION, last="no"), message(), message(rver="a-é:x"), message(rver=START_RUN), message(rver=START_RUN, last="no"),
            message(kind="pk", pid=OLD_PRINCIPAL, pver="default"), message(kind="pk", pid=OLD_PRINCIPAL, pver="default", last="no", actions=("a", "b", "c", "d", "e"))]
    return Call("main", msgs, dver=OLD_VERSION)


def rewritten_docs():
    # `resource.<kind>.v<version>`: the version's 14 bytes are written as 13; the kind of n + 7 bytes with three runs is written as n + 5
    kinds = ["Z" * n + ":a--b@@" for n in (98, 99)]
    return [resource_policy(k, version=OLD_VERSION) for k in kinds] + [resource_policy("k")], kinds


STORE_MAKERS["rewritten"] = lambda: Store(rewritten_docs()[0])
STORE_MAKERS["huge"] = lambda: Store([resource_policy("k"), resource_policy("k", scope="z" * 65000)])


def call_rewritten_lengths():
    kinds = rewritten_docs()[1]
    c = Call("rewritten", [message(kind=k, rver=OLD_VERSION, last=la) for k in kinds for la in ("yes", "no")] + [message()], dver="default")
    keys = sorted({len(a[2]) for m in c.msgs[:4] for a in read_output(c.store().want(m, c.dver)[0])["actions"]})
    assert keys == [127, 128] and [len("resource.%s.v%s" % (k, OLD_VERSION)) for k in kinds] == [130, 131], keys      # `len` against `out_len`
    return c


def call_old_kinds():
    """kinds of the old form the table does not hold rewritten: the host flattener's, in a call of their own"""
    return Call("main", [message(), message(kind="zz:top"), message(kind="k"), message(kind="a-b:c")], host=(1, 3))


def call_actions():
    """A3: 0, 1, 4, 5 and 64 actions; an action repeated on both sides of index 4 (the road decides every place alike); a missing attribute
    (CBI_OUT_CEL_ERROR) on a duplicate"""
    acts = ["a%d" % k for k in range(64)]
    msgs = [message(actions=acts[:n], last=la) for n in (0, 1, 4, 5, 64) for la in ("yes", "no")]
    for rep in ((1, 5), (3, 4), (0, 6), (2, 4, 6), (0, 3, 5), (4, 5, 6), (0, 1, 2)):
        a = ["u%d" % k for k in range(7)]
        for at in rep:
            a[at] = "dup"
        msgs += [message(actions=a, last=la) for la in ("yes", "no")]
    msgs.append(message(actions=("dup", "x", "y", "z", "dup"), last=None))
    return Call("main", msgs)


def call_derived_roles(n):
    """A4: mask bits 0, n - 2, n - 1 alone, all, none; n = 63 / 64 (`n_dr >= 64`)"""
    def m(roles, last="yes"):
        return message(actions=("edit", "view"), roles=roles, last=last)
    every = ["role%02d" % i for i in range(n)]
    msgs = [m([every[0]]), m([every[n - 2]]), m([every[n - 1]]), m(every), m(["user"]), m(every, last="no"), m(every[1:] + ["user"]), m(every[::2])]
    return Call("dr%d" % n, msgs)


def call_dr_names():
    return Call("dr3", [message(actions=("edit",), roles=["role%02d" % i for i in r]) for r in ((0,), (1,), (2,), (3,), (0, 1, 2, 3), (3, 0), ())])


def call_skews(cap):
    """A5: for every skew 0..15 (made by the bytes of the waves before) a wave whose total is one below, at and one above what fits
    (total + skew + 16 <= cap); then totals of 0, 3, 15, 16 and 17 bytes, a block that ends on a 16-byte boundary, a last wave of one lane.
    The fillers pin the mean output size, so the library chooses `cap` itself (out_lds_cap)"""
    msgs, at = [], 0

    def wave(total):
        nonlocal at
        msgs.extend(wave_of_output(total))
        at += total

    def skew_to(s):
        f = (s - at) % 16
        wave(f + 16 if f in (1, 2) else f)
        assert at % 16 == s
    for s in range(16):
        for delta in (-1, 0, 1):
            skew_to(s)
            wave(cap - 16 - s + delta)
    for total in (0, 3, 15, 16, 17):
        wave(total)
    skew_to(5)
    wave(16 * 20 - 5)
    assert at % 16 == 0
    wave(40)
    msgs.append(sized(7))
    c = Call("main", msgs, cap=cap, lds="out", biases=range(16) if cap == 4096 else (0,))
    assert out_lds_cap(at + 7, len(msgs)) == cap, (at, len(msgs))
    return c


def call_scan(waves, tuples=False):
    """A6: minimal messages whose request id is the decimal index - the sizes differ and a wrong prefix moves every later output.
    tuples (the input scan adds up actions and roles): 0 to 2 actions and 0 or 1 role as well, so a wrong prefix moves every later
    tuple and role (no resource: the answers are NO_MATCH under the action's own name)"""
    def m(i):
        if not tuples:
            return text(1, str(i))
        return text(1, str(i)) + b"".join(ld(4, b"a%d" % k) for k in range(i % 3)) + (ld(3, ld(3, b"user")) if i % 2 else b"")
    return Call("main", [m(i) for i in range(64 * waves - 63)], cap=4096)


def call_staging(max_block, cap, small=False):
    """B7: the largest block of the call at `max_block` bytes (the second wave: its first message does not start on a 16-byte boundary);
    the library gives the fill kernel `cap` bytes for it (0: parsed in place)"""
    first = block(16 * 56 + 7)
    msgs = first + block(max_block - 7, k0=1) + block(800, n=30, k0=2)
    assert max(blocks_of(msgs)) == max_block and fill_lds_cap(max_block) == cap
    return Call("main", msgs, cap=cap if cap else 32768, lds="in")


def call_mixed_staging():
    """the count kernel's estimate (1.5 times the mean block plus 256) stages the ordinary waves and not the large one; `need` of 1 023,
    1 024 and 1 025 bytes and one below 16; a wave of 64 empty messages between two full ones (`staged` against `fits`)"""
    msgs = []

    def add(need, **kw):      # a wave whose block - from the 16-byte boundary below its first message - has `need` bytes
        msgs.extend(block(need - sum(len(m) for m in msgs) % 16, **kw))
    for need in (1023, 1024, 1025):
        add(need, k0=need)
    msgs.extend([b""] * 64)
    add(1008, k0=3)      # (ends on a 16-byte boundary)
    msgs.extend([text(1, "a"), text(1, "b"), text(1, "c")] + [b""] * 61)      # a block of less than 16 bytes
    add(5000, k0=4)
    add(900, n=17, k0=5)
    c = Call("main", msgs, cap=2048, lds="mixed")
    n, total = len(msgs), sum(len(m) for m in msgs)
    est = fill_lds_cap((total // n * 64) * 3 // 2 + 256)
    sizes = blocks_of(msgs)
    assert any(b + 24 <= est for b in sizes if b) and any(b + 24 > est for b in sizes), (est, sizes)
    assert {1023, 1024, 1025} <= set(sizes) and 9 in sizes, sizes
    return c


def call_offsets():
    """B8: every start offset modulo 16 of a wave's first message (each wave is one byte over a multiple of 16); every wave's last
    message ends on its block's last byte - the last wave's too, where the call's tail strings follow"""
    msgs = []
    for w in range(18):
        msgs += block(16 * 70 + 1, n=64 if w < 17 else 9, k0=w)
    starts = {int(x) % 16 for x in np.cumsum([0] + [len(m) for m in msgs])[::64]}
    assert starts == set(range(16))
    return Call("main", msgs, cap=2048)


TAILS = {"b": [b"\x20\x01", b"\x20\x00", b"\x20" + b"\x80" * 8 + b"\x01", b"\x20" + b"\x80" * 8 + b"\x00", b"\x20" + b"\x81" + b"\x80" * 7 + b"\x00",
               b"\x20" + b"\x80" * 9 + b"\x01", b"\x20" + b"\x80" * 9 + b"\x00", b"\x20" + b"\x81" + b"\x80" * 8 + b"\x00"],
         "s": [ld(3, s) for s in (b"1234567", b"12345678", b"123456789", b"1234568", b"12345679", b"123456780")],
         "n": [b"\x11" + struct.pack("<d", x) for x in (2.5, 2.25)]}
JUNK = [b""] + [b"\x78" + b"\x80" * (k - 2) + b"\x00" for k in range(2, 9)]      # an unknown varint field of 2..8 bytes


def call_windows():
    """B9: the last field of a block's last message - a one-byte bool, a nine- and a ten-byte varint (the true ones true by their ninth /
    tenth byte alone), strings of 7, 8 and 9 bytes, a double - ends 0 and 2..8 bytes before the block's end; one wave per case"""
    msgs = []
    for action, tails in TAILS.items():
        for tail in tails:
            for junk in JUNK:
                msgs += [message(rid="f%d" % k, kind="t", actions=(action,), tail=tails[k % len(tails)]) for k in range(7)]
                msgs.append(message(rid="end", kind="t", actions=(action,), tail=tail, junk=junk))
                msgs += [b""] * 56
    return Call("main", msgs, cap=1024)


def _limit_messages(over):
    d = 1 if over else 0
    return [message(actions=["a%d" % k for k in range(MAX_ACTIONS + d)]), message(roles=["r%d" % k for k in range(MAX_ROLES + d)]),
            message(last="y" * (MAX_STRLEN + d))]


def call_limits():
    """B10: 64 actions, 255 roles, a compared attribute of 65 535 bytes: decided"""
    return Call("main", [message()] + _limit_messages(False) + [message(last="no")])


def call_over_counts():
    """65 actions, 256 roles: the count kernel leaves exactly these to the host flattener"""
    return Call("main", [message()] + _limit_messages(True)[:2] + [message(last="no")], host=(1, 2))


def call_over_string():
    """a compared attribute of 65 536 bytes: the fill kernel leaves it to the host flattener"""
    return Call("main", [message(), _limit_messages(True)[2], message(last="no")], host=(1,))


CALLS = {"lengths": call_lengths, "largest": call_largest, "rewritten": call_rewritten, "rewritten_lengths": call_rewritten_lengths,
         "old_kinds": call_old_kinds, "actions": call_actions, "derived_roles_63": lambda: call_derived_roles(63),
         "derived_roles_64": lambda: call_derived_roles(64), "derived_role_names": call_dr_names,
         "skews_4096": lambda: call_skews(4096), "skews_8192": lambda: call_skews(8192),
         "staging_1000": lambda: call_staging(1000, 1024), "staging_1001": lambda: call_staging(1001, 2048),
         "staging_32744": lambda: call_staging(32744, 32768), "staging_32745": lambda: call_staging(32745, 0),
         "mixed_staging": call_mixed_staging, "offsets": call_offsets, "windows": call_windows,
         "limits": call_limits, "over_counts": call_over_counts, "over_string": call_over_string}
OUT_SCAN, IN_SCAN = (960, 961, 1024, 1025), (448, 449, 512, 513)      # sixteen / eight sums per round trip start at runs of 16 / 8 waves per lane
for _w in OUT_SCAN + IN_SCAN:
    CALLS["scan_%d" % _w] = (lambda w: lambda: call_scan(w, w in IN_SCAN))(_w)
CPU_CALLS = list(CALLS)      # (all eight scan calls: with them the module stays well below the slowest CPU module)
LIBRARY_CHOICES = ["skews_4096", "skews_8192", "staging_1000", "staging_1001", "staging_32744", "staging_32745", "mixed_staging", "over_counts", "over_string"]
_CALLS = {}


def call(name):
    if name not in _CALLS:
        _CALLS[name] = CALLS[name]()
    return _CALLS[name]


# ---- the judge


def judge(c, msgs, outs, flags, offsets, what):
    st = c.store()
    assert len(outs) == len(msgs) == c.decided, (what, len(outs), len(msgs), c.decided)
    at = 0
    for i, (m, got) in enumerate(zip(msgs, outs)):
        want, flag = st.want(m, c.dver)
        if got != want:
            assert read_output(got) == read_output(want), (what, i, "decision")
            assert got == want, (what, i, "bytes", len(got), len(want))
        assert int(flags[i]) == flag, (what, i, "flags", int(flags[i]), flag)
        if offsets is not None:
            assert int(offsets[i]) == at, (what, i, "offset", int(offsets[i]), at)
        at += len(got)
    if offsets is not None:
        assert int(offsets[len(msgs)]) == at, (what, "total")


def predicted_flags(msgs, status):
    """CBI_OUT_* per input from the kernels' per-tuple statuses: every action's status counts, a dropped duplicate's too"""
    flags, t = [], 0
    for m in msgs:
        f = 0
        for _ in read_input(m)["actions"]:
            f |= OUT_FLAG[int(status[t])]
            t += 1
        flags.append(f)
    assert t == len(status)
    return flags


def run_on_emulator(c, monkeypatch):
    monkeypatch.setenv("CBH_WIRE_LDS_CAP", str(c.cap))
    lt = c.store().lt
    msgs = c.msgs
    if c.host:
        data, off = c.packed()
        rc, wb = wu.sim_flatten(lt, data, off, c.dver)
        assert rc == 0 and wb.stats["first_bad"] == NONE and wb.stats["n_host"] == len(c.host), wb.stats
        assert all(int(wb.status[i]) in (0, 2) and (int(wb.status[i]) == 0 or i in c.host) for i in range(len(msgs)))
        msgs = c.kept()
    data, off = c.packed(msgs)
    rc, wb = wu.sim_flatten(lt, data, off, c.dver)
    assert rc == 0 and wb.stats["first_bad"] == NONE and wb.stats["n_host"] == 0, wb.stats
    res = hostsim_api.check(lt, wu.to_batch(lt, wb), now_ns=NOW, flags=F_WANT_DR, device_order=True)
    first = None
    for bias in c.biases:
        outs, flags, offsets = wu.sim_outputs(lt, res, wb.n, bias=bias, with_offsets=True)
        if first is None:
            judge(c, msgs, outs, flags, offsets, "emulator, bias %d" % bias)
            assert [int(f) for f in flags] == predicted_flags(msgs, res.status)
            first = (outs, list(flags), list(offsets))
        else:
            assert (outs, list(flags), list(offsets)) == first, ("emulator, bias %d" % bias)
    it = IngestTable(lt.blob)
    try:
        hb = it.flatten_pb(data, off, c.dver)
        hres = hostsim_api.check(lt, hb, now_ns=NOW, flags=F_WANT_DR, device_order=True)
        houts, hflags = it.assemble_pb(hb, hres, data, off, c.dver)
    finally:
        it.close()
    assert houts == first[0] and [int(f) for f in hflags] == [int(f) for f in first[1]], "host road"


def run_on_library(capi, c):
    lt = c.store().lt
    table, it = capi.Table(lt.blob), IngestTable(lt.blob)
    try:
        msgs = c.msgs
        if c.host:
            data, off = c.packed()
            with pytest.raises(capi.HostFlattenerNeeded):
                table.wire_check_pb(data, off, now_ns=NOW, flags=F_WANT_DR, default_policy_version=c.dver)
            assert table.last_wire_info["n_host"] == len(c.host), table.last_wire_info
            msgs = c.kept()
        data, off = c.packed(msgs)
        db = table.wire_flatten(data, off, c.dver)
        try:
            assert db.wire_info["n_host"] == 0 and db.wire_info["n_requests"] == len(msgs), db.wire_info
            table.launch(db, now_ns=NOW, flags=F_WANT_DR)
            outs, flags = table.wire_outputs(db)
        finally:
            db.close()
        judge(c, msgs, outs, flags, None, "library, cbh_wire_outputs")
        n = len(msgs)
        mine = (np.empty(sum(len(o) for o in outs) + 64, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint8))
        outs2, flags2 = table.wire_check_pb(data, off, now_ns=NOW, flags=F_WANT_DR, default_policy_version=c.dver, out=mine)
        judge(c, msgs, outs2, flags2, mine[1], "library, cbh_wire_check_pb")
        hb = it.flatten_pb(data, off, c.dver)
        hres = table.check(hb, now_ns=NOW, flags=F_WANT_DR, device_order=True)
        houts, hflags = it.assemble_pb(hb, hres, data, off, c.dver)
        assert houts == outs and [int(f) for f in hflags[:n]] == [int(f) for f in flags[:n]], "host road"
    finally:
        table.close()
        it.close()


@pytest.mark.parametrize("name", CPU_CALLS)
def test_on_emulator(name, monkeypatch):
    run_on_emulator(call(name), monkeypatch)


@pytest.fixture(scope="module")
def engine():
    from sim_engine import sim_engine
    with sim_engine() as capi:
        yield capi


@pytest.mark.parametrize("name", LIBRARY_CHOICES)
def test_on_simulator(engine, name):
    run_on_library(engine, call(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CALLS))
def test_on_gpu(name):
    from cerbos_amd import capi
    run_on_library(capi, call(name))


# ---- made-up results (emulator only: the library takes no results from outside)


def old_form(s):
    """namer.go:213-218: a name of the pre-0.30 form has every run of characters outside [0-9A-Za-z_.] replaced by one '_'"""
    if re.fullmatch(r"[A-Za-z][0-9A-Za-z_@.\-/]*(:[A-Za-z][0-9A-Za-z_@.\-/]*)*", s):
        return re.sub(r"[^0-9A-Za-z_.]+", "_", s)
    return s


def made_up_want(st, msg, dver, results, edr):
    """the plain fold (check.go:513-530) and the plain encoder over made-up per-action results (effect, scope index of a resource policy
    word, scope index or None)"""
    inp = read_input(msg)
    scopes = list(st.lt.scopes)
    folded = {}
    for name, (effect, key_scope, scope) in zip(inp["actions"], results):
        cur = folded.get(name)
        if effect == DENY or cur is None or cur[0] != DENY:
            key = "resource.%s.v%s" % (old_form(inp["resource"]["kind"]), old_form(inp["resource"]["policyVersion"] or dver))
            folded[name] = (effect, key + ("/" + scopes[key_scope] if scopes[key_scope] else ""), "" if scope is None else scopes[scope])
    roles = [n for b, n in enumerate(st.dr_order) if edr >> b & 1]
    return encode_output(inp["requestId"], inp["resource"]["id"], [(a,) + e for a, e in folded.items()], roles)


def made_up_run(st, msgs, dver, results, status, edr, monkeypatch, cap=16384):
    from cerbos_amd import capi
    monkeypatch.setenv("CBH_WIRE_LDS_CAP", str(cap))
    c = Call("main", msgs, dver=dver)
    data, off = c.packed()
    rc, wb = wu.sim_flatten(st.lt, data, off, dver)
    assert rc == 0 and wb.stats["n_host"] == 0 and wb.stats["first_bad"] == NONE and wb.n_tuples == sum(len(r) for r in results)
    res = capi.Result(wb.n_tuples, wb.n, ("policy", "scope", "status", "edr"))
    flat = [r for per in results for r in per]
    res.effect[:] = [r[0] for r in flat]
    res.policy[:] = [(P_RESOURCE << 28) | r[1] for r in flat]
    res.scope[:] = [NONE if r[2] is None else r[2] for r in flat]
    res.status[:] = status
    res.edr[:] = edr
    return wu.sim_outputs(st.lt, res, wb.n, with_offsets=True)


def test_made_up_folds_across_the_register_file(monkeypatch):
    """every order of ALLOW and DENY among two and three repeats of an action at places on both sides of index 4, every tuple with a key
    and a scope of its own (a result taken from the wrong place shows); the statuses of dropped duplicates still set the flags"""
    st = store("main")
    n_scopes = len(st.lt.scopes)
    assert list(st.lt.scopes) == [""] + list(SCOPES)
    msgs, results, status = [], [], []
    places = ((1, 5), (3, 4), (0, 6), (2, 3), (4, 5), (2, 4, 6), (0, 3, 5), (4, 5, 6), (0, 1, 2), (3, 4, 5))
    for rep in places:
        orders = [(x, y) for x in (ALLOW, DENY) for y in (ALLOW, DENY)] if len(rep) == 2 else [(x, y, z) for x in (ALLOW, DENY) for y in (ALLOW, DENY) for z in (ALLOW, DENY)]
        for order in orders:
            acts = ["u%d" % k for k in range(7)]
            per = [((ALLOW, DENY)[k & 1], k % n_scopes, (None, 1, 2, 3)[k % 4]) for k in range(7)]
            for at, e in zip(rep, order):
                acts[at] = "dup"
                per[at] = (e, per[at][1], per[at][2])
            msgs.append(message(rid="f%d" % len(msgs), actions=acts, rver=(OLD_VERSION, "")[len(msgs) & 1]))
            results.append(per)
            stat = [ST_OK] * 7
            stat[rep[0]] = (ST_OK, ST_CEL_ERROR, ST_WANTS_TRACE, ST_UNSUPPORTED)[len(msgs) % 4]      # on a duplicate the fold may drop
            status += stat
    edr = np.zeros(len(msgs), dtype=np.uint64)
    outs, flags, offsets = made_up_run(st, msgs, "default", results, status, edr, monkeypatch)
    assert [int(f) for f in flags] == predicted_flags(msgs, status) and {1, 2, 16} <= {int(f) for f in flags}
    for i, (m, per) in enumerate(zip(msgs, results)):
        want = made_up_want(st, m, "default", per, 0)
        assert read_output(outs[i]) == read_output(want) and outs[i] == want, (i, read_input(m)["actions"], per)
    assert [int(x) for x in offsets] == [0] + list(np.cumsum([len(o) for o in outs]))


@pytest.mark.parametrize("n", [63, 64])
def test_made_up_derived_role_masks(n, monkeypatch):
    """mask bits 0, 62 and 63 alone, all and none - 63 names: bit 63 has no name and is not written; 64: `n_dr >= 64` takes the mask whole"""
    st = store("dr%d" % n)
    masks = [1, 1 << 62, 1 << 63, (1 << 64) - 1, 0, (1 << 63) | 1, (1 << 62) | (1 << 61)]
    msgs = [message(rid="d%d" % k, actions=("view",)) for k in range(len(masks))]
    results = [[(ALLOW, 0, None)] for _ in masks]
    outs, flags, _ = made_up_run(st, msgs, "default", results, [ST_OK] * len(masks), np.array(masks, dtype=np.uint64), monkeypatch)
    for i, (m, mask) in enumerate(zip(msgs, masks)):
        want = made_up_want(st, m, "default", results[i], mask & ((1 << n) - 1))
        assert outs[i] == want, (n, i, read_output(outs[i])["effectiveDerivedRoles"])
    assert len(read_output(outs[3])["effectiveDerivedRoles"]) == n and read_output(outs[2])["effectiveDerivedRoles"] == (["dr63"] if n == 64 else [])


def test_made_up_output_too_large(monkeypatch):
    """CBH_WO_MAX_OUTPUT: an output of exactly 0xFFFFFF bytes is written, one byte more is the call's named error.  60 actions under a key
    of a 65 535-byte kind and version and a 65 000-byte scope, and that scope again (made-up results; the refused call runs the size kernel alone)"""
    st = store("huge")
    big = "z" * 65000
    assert list(st.lt.scopes) == ["", big]
    results = [[(ALLOW, 1, 1)] * 60]

    def one(total):
        names = ["%02d" % k + "n" * 17000 for k in range(60)]
        for _ in range(6):
            m = message(rid="big", kind="K" * MAX_STRLEN, rver="V" * MAX_STRLEN, actions=names)
            size = len(made_up_want(st, m, "default", results[0], 0))
            if size == total:
                return m
            each, rest = divmod(total - size, 60) if abs(total - size) >= 60 else (0, total - size)
            names = [nm + "n" * each for nm in names] if each >= 0 else [nm[:each] for nm in names]
            names[0] = names[0] + "n" * rest if rest >= 0 else names[0][:rest]
            assert all(len(nm) <= MAX_STRLEN for nm in names)
        raise AssertionError(size)
    fits = one(MAX_OUTPUT)
    outs, _, _ = made_up_run(st, [fits], "default", results, [ST_OK] * 60, np.zeros(1, np.uint64), monkeypatch)
    assert outs[0] == made_up_want(st, fits, "default", results[0], 0) and len(outs[0]) == MAX_OUTPUT
    with pytest.raises(RuntimeError, match="an output too large"):
        made_up_run(st, [one(MAX_OUTPUT + 1)], "default", results, [ST_OK] * 60, np.zeros(1, np.uint64), monkeypatch)


def test_the_host_writers_take_a_call_without_tuples(monkeypatch):
    """inputs none of which has an action: no tuple, so the result's effect array is empty - a null pointer.  cbi_assemble_pb,
    cbi_assemble_wire_pb and cbi_assemble_response_pb write the outputs all the same (each refused the call as "null argument")"""
    from cerbos_amd import capi, wire
    monkeypatch.setenv("CBH_WIRE_LDS_CAP", "16384")
    st = store("main")
    c = Call("main", [text(1, "a"), b"", message(rid="none", actions=()), text(1, "b" * 128)])
    data, off = c.packed()
    want = [st.want(m, "default")[0] for m in c.msgs]
    assert all(not read_output(w)["actions"] for w in want) and want[2] == b"\x0a\x04none\x12\x01r"
    it = IngestTable(st.lt.blob)
    try:
        hb = it.flatten_pb(data, off)
        res = capi.Result(0, hb.n_requests, ("policy", "scope", "status", "edr"))
        assert hb.n_tuples == 0 and not res.c.effect
        outs, flags = it.assemble_pb(hb, res, data, off)
        assert outs == want and not flags.any()
        rc, wb = wu.sim_flatten(st.lt, data, off)
        assert rc == 0 and wb.n_tuples == 0
        res = capi.Result(0, wb.n, ("policy", "scope", "status", "edr"))
        spans = (np.ascontiguousarray(wb.in_span), np.zeros((1, 2), np.uint32)[:0], np.zeros(wb.n + 1, dtype=np.uint32))
        outs, flags = it.assemble_wire_pb(res, data, off, spans)
        assert outs == want and not flags.any()
        inputs = [read_input(m) for m in c.msgs[:3]]
        req = wire.encode_check_resources_request({"requestId": "call", "principal": inputs[2]["principal"],
                                                   "resources": [{"actions": [], "resource": dict(i["resource"], id="r%d" % k)} for k, i in enumerate(inputs)]})
        rb = it.flatten_request_pb(req)
        res = capi.Result(0, rb.n_requests, ("policy", "scope", "status", "edr"))
        assert rb.n_tuples == 0
        raw, flags = it.assemble_response_pb(rb, res, req)
        top = list(pb_fields(raw))      # CheckResourcesResponse {1 request_id, 2 results {1 resource {1 id ..}, 2 actions ..}}
        assert [v for n_, _, v in top if n_ == 1] == [b"call"] and not flags.any()
        entries = [v for n_, _, v in top if n_ == 2]
        assert [[x for n2, _, x in pb_fields(dict((a, b) for a, _, b in pb_fields(e))[1]) if n2 == 1] for e in entries] == [[b"r0"], [b"r1"], [b"r2"]]
        assert all(not [1 for n2, _, _ in pb_fields(e) if n2 == 2] for e in entries)
    finally:
        it.close()
