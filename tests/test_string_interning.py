"""String ids on the device road: every string comparison of a decision there is a comparison of ids (cbh_wire.h: the table's hash
index w_table_sid, the batch-local dictionary w_intern_fn with its one compare-and-swap per claim), so a wrong id is a wrong decision
without a crash.  This module decides on strings that were chosen to be confused: distinct strings of equal length and equal 32-bit
cbh_wire_hash (found by a numpy restatement of the hash that is first pinned against the compiled function), near-collisions that
differ in the last byte only and share the dictionary's 16 hash bits and its first slot, the empty string, strings of 65 535 and
65 536 bytes - one member in the table and the other only in the request, both in one message, in neighbouring messages, in
different waves; as principal id, role, action, attribute value, list element, map key, resource kind and scope.

References: oracle.check.RuleTableOracle on the dict inputs (strings by value: it cannot share an interning bug) for every effect and
for whether a CEL error was recorded - exactly; the host road (cbi_flatten_pb -> cbh_check_batch) as the second one on the library.

Where the ids are consumed (every run asserts the kernel it meant to reach: STORES' plan checks):
  flat    cbh_check_flat_kernel (closed leaves: column == constant, == P.id, == column, != column)
  derived cbh_check_flat_kernel_dr (a derived role on R.attr.owner == P.id)
  eval    cbh_walk2_kernel with the evaluator: `in` a list, exists(), a map lookup, startsWith / size (the bytes behind a batch-local id,
          BatchDev.str_keys), exact and glob actions and roles (cbh_resolve_globs_kernel reads the dictionary), a kind and a scope
          that collide with the table's
Tiers: *_on_emulator = the kernels' source on the host wave emulator (tests/hostsim: the device flattener against cbi_flatten_pb value
by value, "equal strings <=> equal ids", the whole dictionary downloaded); *_on_simulator = the library's host side on the simulator
(tests/sim_engine.py); *_on_gpu = libcerbos_hip.so.  test_lost_claims_on_emulator makes every k-th probe of the dictionary read EMPTY
(cbh_wire.h's test switch): the claim behind it is lost and w_intern_fn must go on with what the compare-and-swap returned - the
branch a single-threaded simulator never takes otherwise; the counter behind the switch shows that it was taken.
test_contended_claims_on_gpu is what no simulator schedules: 250 000 messages claiming the same slots at once.  What cbh_wire_req.h
does with a principal's strings: nothing - the split kernel copies the principal's BYTES into the CheckInput of every resource entry,
and the fill kernel's lane for that CheckInput interns principal and resource strings alike.  So the principal id of a request with
4 000 entries is claimed by one of 4 000 lanes in 63 waves and found by the others through a byte comparison against ANOTHER
message's copy; those ids meet the ids of the entry's own attribute values in `R.attr.a == P.id`.
The 65 536-byte policy constant: w_intern_fn asks the table before it looks at the length, the lowering accepts the constant, the
message stays on the device (test_length_limits_*).

Mutation check (on a scratch copy, never committed; the CPU tier of this module under each mutant - every mutant fails at least the tests
named, every other test of the module passes under it):
  (a) w_table_sid without w_bytes_eq              test_ids_on_emulator[flat | derived | eval], test_ids_on_simulator[flat | derived | eval],
                                                  test_lost_claims_on_emulator, test_regrowth_twin_on_emulator, test_regrowth_on_simulator,
                                                  test_regrowth_in_slices_on_simulator
  (b) w_intern_fn's dictionary match without it   the same ten, test_contended_claims_body_on_simulator (its decisions hinge on the pairs)
  (c) `cur = key` after a lost compare-and-swap   test_lost_claims_on_emulator (nothing else loses a claim)
  (d) w_bytes_eq's tail mask one byte short       the ten of (a), test_length_limits_on_emulator, test_length_limits_on_simulator,
                                                  test_contended_claims_body_on_simulator
  (e) `slots *= 4` without the statistics reset   cbh_host_wire.h: test_regrowth_on_simulator, test_regrowth_in_slices_on_simulator; with n_host left
      (cbh_host_wire.h wire_flatten_stages) / a stale n_host           stale in hostsim.cpp's own loop: test_regrowth_twin_on_emulator, test_lost_claims_on_emulator
      (hostsim.cpp's loop)
  (f) str_span's length mask 15 bits wide         test_length_limits_on_simulator
  (g) `len >= CBH_WIRE_MAX_STRLEN`                test_length_limits_on_emulator, test_length_limits_on_simulator
What the suite caught before this module - tests/test_wire_device.py, tests/test_request_road.py and tests/test_sim_engine.py (62 tests)
under the same mutants:
  (a), (b)   none of the 62
  (c), (f), (g)   cannot be caught there: no claim is lost, no string is longer than a few hundred bytes
  (d)   13: test_wire_device.py test_golden_store_inputs, test_policy_test_framework_inputs, test_the_whole_token_as_a_value,
        test_varints_longer_than_they_need_to_be, test_mutated_messages_both_flatteners_agree; test_request_road.py
        test_requests_down_the_device_road_on_the_simulator[cr_case_03 | 06 | 07 | 08], test_every_request_s_audit_trail_beside_its_outputs;
        test_sim_engine.py test_request_road_service_cases, test_request_road_audit_trail_golden_store, test_the_roads_in_slices
  (e)   hostsim.cpp's loop: test_wire_device.py test_fuzz_inputs[0 - 5]; cbh_host_wire.h's loop: none of the 62"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from cerbos_amd import wire
from cerbos_amd.ingest import IngestTable
from cerbos_amd.lower.blob import lower_rule_table
from cerbos_amd.policy.loader import policies_from_docs
from cerbos_amd.ruletable.build import rule_table_from_policies
from oracle.check import EvalParams, RuleTableOracle

API = "api.cerbos.dev/v1"
NOW = 1_700_000_000_000_000_000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EFFECT_ALLOW, ST_CEL_ERROR, ST_UNSUPPORTED, F_WANT_DERIVED_ROLES = 1, 1, 2, 4   # cerbos_amd/capi.py
LENGTHS = (5, 8, 9, 16)          # on both sides of the 8-byte window of w_bytes_eq / w_hash
MAX_STRLEN = 0xFFFF              # cbh_wire.h CBH_WIRE_MAX_STRLEN
ALPHABET = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789", dtype=np.uint8)   # plain in a kind, a scope, an action, a glob
LAST = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789_-", dtype=np.uint8)


# ---- part 1: the hash, restated; strings that collide
def wire_hash_np(a):
    """cbh_wire.h cbh_wire_hash over the rows of uint8[N][L] -> uint32[N]"""
    a = np.asarray(a, dtype=np.uint8)
    h = np.full(a.shape[0], 0x811C9DC5 ^ a.shape[1], dtype=np.uint32)
    for i in range(a.shape[1]):
        h ^= a[:, i]
        h *= np.uint32(0x01000193)
    return _finish(h)


def _finish(h):
    h = h ^ (h >> np.uint32(15))
    h = h * np.uint32(0x2C1B3C6D)
    h = h ^ (h >> np.uint32(12))
    h = h * np.uint32(0x297A2D39)
    return h ^ (h >> np.uint32(15))


def compiled_hash(s):
    import hostsim_api
    lib = hostsim_api.lib()
    lib.hostsim_wire_hash.argtypes = [C.c_char_p, C.c_uint32]
    lib.hostsim_wire_hash.restype = C.c_uint32
    return int(lib.hostsim_wire_hash(bytes(s), len(s)))


def _candidates(length, count):
    """`count` DISTINCT strings of `length` bytes over ALPHABET: the index times a fixed multiplier modulo 36^k, written in base 36
    (an injection: the multiplier is prime to 36).  Lengths above 9: one fixed head, eight bytes that vary - members of a collision
    then differ beyond byte 8 only."""
    k = length if length <= 9 else 8
    idx = (np.arange(count, dtype=np.uint64) * np.uint64(4_000_037) + np.uint64(977 + length)) % np.uint64(36 ** k)
    assert count < 36 ** k and 4_000_037 % 2 and 4_000_037 % 3 and count * 4_000_037 < 2 ** 63
    out = np.empty((count, length), dtype=np.uint8)
    out[:, :length - k] = np.frombuffer(b"samehead"[:length - k], dtype=np.uint8)
    for j in range(k):
        out[:, length - 1 - j] = ALPHABET[(idx % np.uint64(36)).astype(np.int64)]
        idx //= np.uint64(36)
    return out


_PAIRS, _NEAR = {}, {}


def collisions(length, count=600_000):
    """[(x, y)]: distinct strings of `length` bytes with cbh_wire_hash(x) == cbh_wire_hash(y), all 32 bits.  Expected count^2 / 2^33 = 42."""
    if length not in _PAIRS:
        cand = _candidates(length, count)
        h = wire_hash_np(cand)
        order = np.argsort(h, kind="stable")
        same = np.flatnonzero(h[order][1:] == h[order][:-1])
        pairs, last = [], -2
        for i in same:
            if i != last + 1:   # (of three equal hashes: the first two)
                x, y = cand[order[i]].tobytes(), cand[order[i + 1]].tobytes()
                assert x != y and len(x) == len(y) == length and compiled_hash(x) == compiled_hash(y) == int(h[order[i]])
                pairs.append((x.decode(), y.decode()))
            last = i
        assert len(pairs) >= 8, "the search found %d colliding pairs of length %d" % (len(pairs), length)
        if length > 9:
            assert all(x[:8] == y[:8] for x, y in pairs)
        _PAIRS[length] = pairs
    return _PAIRS[length]


def near_collisions(length, bases=800_000):
    """[(x, y)] that differ in the LAST byte only (a full collision of such a pair cannot exist: one round of the hash is a bijection)
    and agree in what the dictionary looks at before it compares bytes: (h >> 16) | 0x8000 (the key's hash bits), the length, h & 4095 (the slot)."""
    if length not in _NEAR:
        head = _candidates(length, bases)[:, :length - 1]
        state = np.full(bases, 0x811C9DC5 ^ length, dtype=np.uint32)
        for i in range(length - 1):
            state ^= head[:, i]
            state *= np.uint32(0x01000193)
        sig = np.empty((len(LAST), bases), dtype=np.uint32)
        for j, c in enumerate(LAST):
            h = _finish((state ^ np.uint32(c)) * np.uint32(0x01000193))
            sig[j] = (((h >> np.uint32(16)) & np.uint32(0x7FFF)) << np.uint32(12)) | (h & np.uint32(4095))
        order = np.argsort(sig, axis=0, kind="stable")
        srt = np.take_along_axis(sig, order, axis=0)
        pairs = []
        for j, b in zip(*np.nonzero(srt[1:] == srt[:-1])):
            x = head[b].tobytes() + bytes([LAST[order[j, b]]])
            y = head[b].tobytes() + bytes([LAST[order[j + 1, b]]])
            hx, hy = compiled_hash(x), compiled_hash(y)
            assert x != y and x[:-1] == y[:-1] and (hx >> 16) | 0x8000 == (hy >> 16) | 0x8000 and hx & 4095 == hy & 4095
            pairs.append((x.decode(), y.decode()))
        assert len(pairs) >= 2, "the search found %d near-collisions of length %d" % (len(pairs), length)
        _NEAR[length] = pairs
    return _NEAR[length]


def test_restated_hash_is_the_compiled_one():
    rng = np.random.default_rng(20261017)
    lengths = [0, 7, 8, 9] * 50 + list(rng.integers(0, 41, size=3000))
    for n in sorted(set(lengths)):
        rows = rng.integers(0, 256, size=(lengths.count(n), n), dtype=np.uint8)
        for row, h in zip(rows, wire_hash_np(rows)):
            assert compiled_hash(row.tobytes()) == int(h), (n, row.tobytes())


@pytest.mark.parametrize("length", LENGTHS)
def test_collision_search(length):
    pairs = collisions(length)
    assert len(pairs) >= 8 and len({s for p in pairs for s in p}) == 2 * len(pairs)
    if length in (9, 16):
        assert len(near_collisions(length)) >= 2


# ---- part 2: stores whose decisions depend on ids
def _rule(action, expr=None, roles=("*",)):
    r = {"actions": [action], "roles": list(roles), "effect": "EFFECT_ALLOW"}
    if expr is not None:
        r["condition"] = {"match": {"expr": expr}}
    return r


def _policy(kind, rules, **kw):
    return {"apiVersion": API, "resourcePolicy": dict({"resource": kind, "version": "default", "rules": rules}, **kw)}


def _flat_plan(plan, *suffixes, no=()):
    name = plan.split("[")[0]
    return name.startswith("cbh_check_flat_kernel") and all(s in name for s in suffixes) and not any(s in name for s in no)


class Names:
    """the strings of one length: T in the table with U colliding (only in requests); V, W colliding, neither in the table; R2 a
    role of the table with E colliding (E is a role of every message of its length; the length-8 E of every message); K a kind of the table with KU colliding; N1, N2 a near-collision"""

    def __init__(self, length):
        p = collisions(length)
        (self.T, self.U), (self.V, self.W), (self.R2, self.E), (self.K, self.KU) = p[0], p[1], p[2], p[3]
        self.pool = [self.T, self.U, self.V, self.W, ""]
        if length in (9, 16):
            self.N1, self.N2 = near_collisions(length)[0]
            self.pool += [self.N1, self.N2]
        self.length = length


class Store:
    """which: flat | derived | eval.  One kind per length; requests: every (a, x) of the length's pool, twice over (the second
    copy lies waves behind the first), a = the resource's attribute value / owner / list element / map key, x = the principal's id,
    role and attribute, R.attr.b and one action."""

    def __init__(self, which):
        self.which = which
        self.names = {n: Names(n) for n in LENGTHS}
        self.everywhere = self.names[8].E     # ONE colliding string that every message carries as a role (eval: its partner is a role of the table)
        docs, self.actions = [], {}
        for n, s in self.names.items():
            kind = "k%d" % n
            if which == "flat":
                rules = [_rule("const", 'R.attr.a == "%s"' % s.T), _rule("pid", "R.attr.a == P.id"), _rule("ab", "R.attr.a == R.attr.b"), _rule("ne", "R.attr.a != P.attr.n")]
            elif which == "derived":
                docs.append({"apiVersion": API, "derivedRoles": {"name": "defs%d" % n, "definitions": [
                    {"name": "owner%d" % n, "parentRoles": ["*"], "condition": {"match": {"expr": "R.attr.owner == P.id"}}}]}})
                rules = [{"actions": ["own"], "derivedRoles": ["owner%d" % n], "effect": "EFFECT_ALLOW"}, _rule("const", 'R.attr.a == "%s"' % s.T)]
            else:
                rules = [_rule("member", "P.id in R.attr.members"), _rule("exists", "R.attr.tags.exists(t, t == P.attr.team)"),
                         _rule("map", 'R.attr.m[P.id] == "x"'), _rule("starts", "R.attr.a.startsWith(P.attr.pre)"), _rule("size", "size(R.attr.a) == %d" % n),
                         _rule("role", roles=[s.T]), _rule("role2", roles=[s.R2]), _rule("rglob", roles=["*" + s.V[-4:]]),
                         _rule(s.T), _rule("*" + s.W[-4:])]
            self.actions[kind] = [r["actions"][0] for r in rules]
            docs.append(_policy(kind, rules, **({"importDerivedRoles": ["defs%d" % n]} if which == "derived" else {})))
            if which == "eval":
                docs.append(_policy(s.K, [_rule("any")]))                                  # a kind that collides with a request's
        if which == "eval":
            s5 = self.names[5]
            docs.append(_policy("k5", [_rule("scoped")], scope=s5.T))                      # a scope that collides with a request's
        self.rt = rule_table_from_policies(policies_from_docs(docs))
        self.lt = lower_rule_table(self.rt)
        assert not self.lt.unsupported, self.lt.unsupported
        self.inputs, self.labels = [], []
        for copy in range(2):
            for n, s in self.names.items():
                for a in s.pool:
                    for j, x in enumerate(s.pool):
                        self._add("k%d" % n, s, a, x, j + copy)
        if which == "eval":
            for n, s in self.names.items():
                for kind in (s.K, s.KU):
                    self._add(kind, s, s.T, s.U, 0, actions=["any"])
            s5 = self.names[5]
            for scope in (s5.T, s5.U, "", s5.T + "." + s5.U):
                self._add("k5", s5, s5.V, s5.W, 0, actions=["scoped", "member"], scope=scope)
        self.want = self._expected()

    def _add(self, kind, s, a, x, j, actions=None, scope=None):
        if actions is None:
            actions = list(self.actions[kind])
            if self.which == "eval":   # the request's own action: a member, the table's or not (labels: what the coverage check counts)
                actions[-2:] = [x or "none", s.W if j % 2 else s.V]
        labels = list(self.actions.get(kind, actions)) if len(actions) == len(self.actions.get(kind, ())) else list(actions)
        res = {"kind": kind, "id": "r%d" % len(self.inputs), "attr": {
            "a": a, "b": x, "owner": a, "members": [s.U, a], "tags": [a, s.W], "m": {a: "x" if j % 2 else "y", s.R2: "x"}}}
        if scope is not None:
            res["scope"] = scope
        self.inputs.append({"requestId": "q%d" % len(self.inputs), "actions": actions,
                            "principal": {"id": x, "roles": [x or "norole", s.E] + ([self.everywhere] if s.E != self.everywhere else []) + ([s.R2] if j % 4 == 3 else []),
                                          "attr": {"n": x, "team": x, "pre": x[:-1] if x else x}},
                            "resource": res})
        self.labels.append(labels)

    def _expected(self):
        """[(allow per action, CEL error)] by the oracle; every condition's action is allowed somewhere and denied somewhere"""
        orc = RuleTableOracle(self.rt)
        out, seen = [], {}
        for inp, labels in zip(self.inputs, self.labels):
            o = orc.check(inp, EvalParams(now_ns=NOW))
            allow = [o["actions"][a]["effect"] == "EFFECT_ALLOW" for a in inp["actions"]]
            out.append((allow, bool(o.get("evaluationErrors"))))
            for lab, al in zip(labels, allow):
                seen.setdefault(lab, set()).add(al)
        assert all(v == {True, False} for v in seen.values()), {k: v for k, v in seen.items() if v != {True, False}}
        return out

    def plan_ok(self, plan):
        if self.which == "flat":
            return _flat_plan(plan, no=("_any", "_dr"))
        if self.which == "derived":
            return _flat_plan(plan, "_dr")
        return plan.split("[")[0].strip().endswith("cbh_walk2_kernel")

    kind_on_emulator = property(lambda self: 2 if self.which == "eval" else 1)

    def messages(self):
        return wire.pack_messages([wire.encode_check_input(i) for i in self.inputs])


_STORES = {}


def store(which):
    if which not in _STORES:
        _STORES[which] = Store(which)
    return _STORES[which]


def compare(inputs, want, res, what):
    """`res` (input order) against [(allow per action, CEL error)]"""
    assert not (res.status == ST_UNSUPPORTED).any(), (what, "flagged for the CPU path")
    t = 0
    for i, (inp, (allow, err)) in enumerate(zip(inputs, want)):
        na = len(allow)
        have = [int(e) == EFFECT_ALLOW for e in res.effect[t:t + na]]
        p, r = inp["principal"], inp["resource"]
        assert have == allow, (what, i, inp["actions"], r["kind"], r.get("scope"), p["id"], r["attr"]["a"], have, allow)
        assert bool((res.status[t:t + na] == ST_CEL_ERROR).any()) == err, (what, "error", i, p["id"], r["attr"]["a"])
        t += na
    assert t == res.effect.size


def compare_outputs(inputs, want, raw, flags, what):
    """serialized CheckOutputs and their flags (cerbos_ingest.h: 2 = a CEL error was absorbed, nothing else)"""
    assert len(raw) == len(inputs)
    for i, (r, inp, (allow, err)) in enumerate(zip(raw, inputs, want)):
        out = wire.decode_check_output(r)
        assert [out["actions"][a]["effect"] == "EFFECT_ALLOW" for a in inp["actions"]] == allow, (what, i)
        assert int(flags[i]) == (2 if err else 0), (what, i, int(flags[i]))


def one_slot_per_string(wb):
    """over the WHOLE downloaded dictionary, not only the ids in use: no string owns two slots; every key's fields are its string's"""
    seen = {}
    for slot in np.flatnonzero(wb.dict):
        key = int(wb.dict[slot])
        off, ln = key & 0xFFFFFFFF, (key >> 32) & 0xFFFF
        s = wb.msg[off:off + ln]
        assert key >> 48 == (compiled_hash(s) >> 16) | 0x8000, (slot, s[:40])
        assert seen.setdefault(s, int(slot)) == int(slot), "two dictionary slots for %r" % s[:40]
    return len(seen)


def flatten_on_emulator(lt, inputs, **kw):
    """cbi_flatten_pb against the device flattener's kernels (tests/test_wire_device.py _compare: value by value, equal strings <=>
    equal ids), then the whole dictionary"""
    from test_wire_device import _compare
    hb, wb = _compare(lt, inputs, **kw)
    one_slot_per_string(wb)
    return hb, wb


def check_ids_on_emulator(which, **kw):
    import hostsim_api
    import wire_device_util as wu
    s = store(which)
    hb, wb = flatten_on_emulator(s.lt, s.inputs, **kw)
    compare(s.inputs, s.want, hostsim_api.check(s.lt, hb, NOW, F_WANT_DERIVED_ROLES), which + ", host flattener")
    compare(s.inputs, s.want, hostsim_api.check(s.lt, wu.to_batch(s.lt, wb), NOW, F_WANT_DERIVED_ROLES), which + ", device flattener")
    assert hostsim_api.last_kind() == s.kind_on_emulator, (which, hostsim_api.last_kind())
    return wb


def both_roads(capi, lt, inputs, want, what, plan_ok=None, min_fill_runs=1):
    """the host road (cbi_flatten_pb -> cbh_check_batch) and the device road (cbh_wire_flatten -> cbh_check_resident ->
    cbh_wire_outputs) against the oracle and against each other -> the device batch's wire_info"""
    data, off = wire.pack_messages([wire.encode_check_input(i) for i in inputs])
    table, it = capi.Table(lt.blob), IngestTable(lt.blob)
    try:
        hb = it.flatten_pb(data, off)
        host_dev = table.check(hb, now_ns=NOW, flags=F_WANT_DERIVED_ROLES, device_order=True)
        host_out, host_flags = it.assemble_pb(hb, host_dev, data, off)
        host = host_dev.to_input_order(hb)
        compare(inputs, want, host, what + ", host road")
        db = table.wire_flatten(data, off)
        try:
            info = db.wire_info
            assert info["n_host"] == 0 and info["fill_runs"] >= min_fill_runs, info
            table.launch(db, now_ns=NOW, flags=F_WANT_DERIVED_ROLES)
            have = table.download(db)
            compare(inputs, want, have, what + ", device road")
            for f in ("effect", "policy", "scope", "status", "edr"):
                assert np.array_equal(getattr(host, f), getattr(have, f)), (what, f)
            if plan_ok is not None:
                plan = table.plan(db, flags=F_WANT_DERIVED_ROLES)
                assert plan_ok(plan), (what, plan)   # a test that passes because another kernel decided proves nothing
            dev_out, dev_flags = table.wire_outputs(db)
            assert dev_out == host_out and np.array_equal(dev_flags, host_flags), what
            compare_outputs(inputs, want, dev_out, dev_flags, what + ", cbh_wire_outputs")
        finally:
            db.close()
        return info
    finally:
        table.close()
        it.close()


def check_ids_on_library(capi, which):
    s = store(which)
    both_roads(capi, s.lt, s.inputs, s.want, which, s.plan_ok)
    table = capi.Table(s.lt.blob)
    try:
        raw, flags = table.wire_check_pb(*s.messages(), now_ns=NOW, flags=F_WANT_DERIVED_ROLES)
        compare_outputs(s.inputs, s.want, raw, flags, which + ", cbh_wire_check_pb")
    finally:
        table.close()


# ---- part 3: the lost claim
def check_lost_claims():
    """every k-th probe reads EMPTY: the stores above, the golden store's inputs, two fuzz seeds"""
    import hostsim_api
    from helpers import load_json, store_rule_table
    from test_fuzz_parity import _policies, _requests
    from test_hostsim_golden import GLOBALS
    lib = hostsim_api.lib()
    lib.hostsim_wire_stale_reads.argtypes = [C.c_uint32]
    lib.hostsim_wire_stale_reads.restype = C.c_uint32
    golden = lower_rule_table(store_rule_table(), GLOBALS)
    golden_inputs = [inp for case in load_json("engine_cases.json") for inp in case["inputs"]]
    fuzz = []
    for seed in (0, 2):
        rng = np.random.default_rng(10_000 + seed)
        lt = lower_rule_table(rule_table_from_policies(policies_from_docs(_policies(rng))))
        fuzz.append((lt, [i for i in _requests(rng, 300) if len(i.get("actions") or []) <= 64 and ":" not in i["resource"]["kind"]]))
    lost = {}
    try:
        for k in (1, 2, 7):
            lib.hostsim_wire_stale_reads(k)
            for which in ("flat", "derived", "eval"):
                check_ids_on_emulator(which)
            flatten_on_emulator(golden, golden_inputs)
            for lt, inputs in fuzz:
                flatten_on_emulator(lt, inputs)
                flatten_on_emulator(lt, inputs, dict_slots=16, heap=1)
            lost[k] = int(lib.hostsim_wire_stale_reads(0))
    finally:
        lib.hostsim_wire_stale_reads(0)
    # `cur = prev` of w_intern_fn ran: claims were lost (k = 1: every string's second occurrence loses one)
    assert all(v > 100 for v in lost.values()), lost
    check_ids_on_emulator("flat")
    assert int(lib.hostsim_wire_stale_reads(0)) == 0, "a claim was lost with the switch off"


# ---- part 4: regrowth
def dict_slots_for(n):
    """cbh_wire_host.h cbh_wire_dict_slots: the library's first guess"""
    c = 4096
    while c < 8 * n and c < 1 << 30:
        c <<= 1
    return c


def regrowth_inputs(n=160, per=110, heavy=range(0, 10 ** 9), bools=0):
    """`n` messages of two kinds; those in `heavy` carry a list of 60 strings (`in` over more than 64 elements is not decided on the
    device) and a map of 2 * per - 60 keys that nobody else has (2 * per * n unknown strings: more than max(4096, 8 n) slots hold), now
    and then the principal's id among them; `bools`: a list of that many booleans as one value of the map - heap entries of four message
    bytes each, where the heap's first guess is an entry to eight bytes."""
    s = store("eval")
    out = []
    for i in range(n):
        nm = s.names[(5, 8)[i % 2]]
        pid = "u%dx%d" % (i, 7) if i % 3 else nm.V
        big = i in heavy
        members = ["m%d_%d" % (i, j) for j in range(min(per, 60) if big else 2)] + ([pid] if i % 4 == 0 else [nm.W])
        m = {"key%d_%d" % (i, j): "x" if j % 2 else "y" for j in range(2 * per - min(per, 60) if big else 2)}
        if i % 5 == 0:
            m[pid] = "x"
        if bools:
            m["flags"] = [True, False] * (bools // 2)
        kind = "k%d" % nm.length
        actions = list(s.actions[kind])
        actions[-2:] = ["m%d_0" % i, nm.W]
        out.append({"requestId": "g%d" % i, "actions": actions,
                    "principal": {"id": pid, "roles": ["user", nm.E], "attr": {"team": "m%d_1" % i if i % 2 else nm.W, "pre": nm.T[:3]}},
                    "resource": {"kind": kind, "id": "r%d" % i, "attr": {"a": nm.T if i % 7 else nm.U, "members": members, "tags": members[:3], "m": m}}})
    return s, out


def oracle_answers(rt, inputs):
    orc = RuleTableOracle(rt)
    out = []
    for inp in inputs:
        o = orc.check(inp, EvalParams(now_ns=NOW))
        out.append(([o["actions"][a]["effect"] == "EFFECT_ALLOW" for a in inp["actions"]], bool(o.get("evaluationErrors"))))
    return out


def _request_of(inputs):
    return {"requestId": inputs[0]["requestId"], "principal": inputs[0]["principal"], "resources": [{"actions": i["actions"], "resource": i["resource"]} for i in inputs]}


def host_road_outputs(capi, lt, inputs):
    """the host road's serialized CheckOutputs and flags (cbi_flatten_pb -> cbh_check_batch -> cbi_assemble_pb), in input order"""
    data, off = wire.pack_messages([wire.encode_check_input(i) for i in inputs])
    table, it = capi.Table(lt.blob), IngestTable(lt.blob)
    try:
        hb = it.flatten_pb(data, off)
        return it.assemble_pb(hb, table.check(hb, now_ns=NOW, flags=F_WANT_DERIVED_ROLES, device_order=True), data, off)
    finally:
        table.close()
        it.close()


def check_regrowth_on_library(capi, n=160, per=110):
    """cbh_wire_flatten's retry loops (cbh_host_wire.h: wf_fill, wire_flatten_stages): the dictionary quadrupled - twice -, the scan and the fill run again, the
    routing kernels again behind them; then the same with a heap guess that is short as well.  The grouped order itself is not
    something the library hands out: what can be held against the host road's routing sort is the number of routes (wire_info's
    n_routes, as tests/test_gpu_wire.py does) and the answers in input order, byte for byte."""
    s, inputs = regrowth_inputs(n, per)
    want = oracle_answers(s.rt, inputs)
    assert n >= 128 and 2 * per * n > max(4096, 8 * n) and {True, False} == {a for al, _ in want for a in al[:3]}
    info = both_roads(capi, s.lt, inputs, want, "regrowth", s.plan_ok, min_fill_runs=2)
    assert info["fill_runs"] > 1 and info["dict_slots"] > dict_slots_for(n), info
    assert info["n_routes"] == 2, info                     # grouped by route behind the LAST fill: two kinds, as the host road sorts them
    # ... and the heap's guess short too: both loops, one inside the other
    _, inputs2 = regrowth_inputs(n, per, bools=900)
    total = sum(len(wire.encode_check_input(i)) for i in inputs2)
    want2 = oracle_answers(s.rt, inputs2)
    info2 = both_roads(capi, s.lt, inputs2, want2, "regrowth, heap too", s.plan_ok, min_fill_runs=3)
    assert info2["heap_len"] > total // 8 + 4096 and info2["dict_slots"] > dict_slots_for(n) and info2["fill_runs"] >= 3, (info2, total)
    table = capi.Table(s.lt.blob)
    try:
        # the request road: every principal with its own entries (cbh_wire_check_requests_pb)
        reqs = [wire.encode_check_resources_request(_request_of([i])) for i in inputs]
        outs, flags, _ = table.wire_check_requests_pb(reqs, now_ns=NOW, flags=F_WANT_DERIVED_ROLES)
        rinfo = table.last_wire_info
        assert rinfo["fill_runs"] > 1 and rinfo["dict_slots"] > dict_slots_for(n), rinfo
        flat = [o for per_req in outs for o in per_req]
        compare_outputs(inputs, want, flat, flags, "regrowth, request road")
        host_out, host_flags = host_road_outputs(capi, s.lt, inputs)
        assert flat == host_out and np.array_equal(flags, host_flags), "regrowth, request road against the host road"
    finally:
        table.close()


def check_regrowth_in_slices(capi, n=640, per=110):
    """cbh_wire_check_pb cut into four slices (CBH_WIRE_SLICE_MIN: read once per process), the third of which overflows its dictionary"""
    cut = n // 4
    s, inputs = regrowth_inputs(n, per, heavy=range(2 * cut, 3 * cut))
    want = oracle_answers(s.rt, inputs)
    table = capi.Table(s.lt.blob)
    try:
        raw, flags = table.wire_check_pb(*wire.pack_messages([wire.encode_check_input(i) for i in inputs]), now_ns=NOW, flags=F_WANT_DERIVED_ROLES)
        info = table.last_wire_info
        first = dict_slots_for(cut)     # (the slices' sum: three slices at their first guess, one grown)
        assert info["fill_runs"] > 1 and info["dict_slots"] > 4 * first and info["dict_slots"] - 3 * first in (4 * first, 16 * first, 64 * first), info
        compare_outputs(inputs, want, raw, flags, "regrowth in slices")
        host_out, host_flags = host_road_outputs(capi, s.lt, inputs)
        assert raw == host_out and np.array_equal(flags, host_flags), "regrowth in slices against the host road"
    finally:
        table.close()


CHILD = """
import sys
sys.path[:0] = [%(tests)r, %(root)r]
import test_string_interning as t
if %(sim)r:
    from sim_engine import sim_engine
    with sim_engine() as capi:
        t.check_regrowth_in_slices(capi, %(n)d)
else:
    from cerbos_amd import capi
    t.check_regrowth_in_slices(capi, %(n)d)
print("string interning: ok")
"""


def regrowth_in_slices_in_child(sim, n, slice_min):
    """a fresh process: the library reads its slice sizes once.  A child that a signal ended fails the test."""
    r = subprocess.run([sys.executable, "-c", CHILD % {"tests": os.path.join(ROOT, "tests"), "root": ROOT, "sim": sim, "n": n}],
                       env=dict(os.environ, CBH_WIRE_SLICE_MIN=str(slice_min)), cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode >= 0, "the child was ended by signal %d\n%s" % (-r.returncode, r.stderr[-4000:])
    assert r.returncode == 0 and "string interning: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]


# ---- part 5: the length limit
def length_limit_store():
    """-> (rule table, lowered table, inputs, oracle's answers): strings of 65 535 bytes the table does not know, a 65 536-byte
    constant the table holds"""
    if "limits" not in _STORES:
        const = "c" * (MAX_STRLEN + 1)
        docs = [_policy("big", [_rule("ab", "R.attr.a == R.attr.b"), _rule("pid", "R.attr.a == P.id"), _rule("size", "size(R.attr.a) == %d" % MAX_STRLEN),
                                _rule("starts", "R.attr.a.startsWith(P.attr.pre)"), _rule("const", 'R.attr.a == "%s"' % const)])]
        rt = rule_table_from_policies(policies_from_docs(docs))
        lt = lower_rule_table(rt)
        assert not lt.unsupported and const in lt.string_ids
        s = "s" * MAX_STRLEN
        other = s[:-1] + "t"
        rows = [(s, s, s, s), (s, other, other, other), (other, s, "p", s[:-1]), (s, "b", s, "s" * 9), (const, const, "p", "c"), (const[:-1], const, "p", const[:-1]),
                ("short", "short", "short", "sh")]
        inputs = [{"requestId": "L%d" % i, "actions": ["ab", "pid", "size", "starts", "const"], "principal": {"id": pid, "roles": ["user"], "attr": {"pre": pre}},
                   "resource": {"kind": "big", "id": "r", "attr": {"a": a, "b": b}}} for i, (a, b, pid, pre) in enumerate(rows)]
        want = oracle_answers(rt, inputs)
        assert [al for al, _ in want][:3] == [[True, True, True, True, False], [False, False, True, False, False], [False, False, True, True, False]]
        assert want[4][0] == [True, False, False, True, True] and want[5][0] == [False, False, True, True, False]
        _STORES["limits"] = (rt, lt, inputs, want)
    return _STORES["limits"]


def too_long_input():
    """one unknown string of 65 536 bytes: a message for the host flattener"""
    rt, lt, inputs, _ = length_limit_store()
    s = "s" * (MAX_STRLEN + 1)
    more = [dict(inputs[0], resource={"kind": "big", "id": "r", "attr": {"a": s, "b": s}}), dict(inputs[1], principal={"id": s[:-1] + "t", "roles": ["user"], "attr": {"pre": s[:-1]}},
                                                                                                 resource={"kind": "big", "id": "r", "attr": {"a": s, "b": "x"}})]
    return rt, lt, inputs + more


def check_length_limits_on_emulator():
    import hostsim_api
    import wire_device_util as wu
    rt, lt, inputs, want = length_limit_store()
    hb, wb = flatten_on_emulator(lt, inputs)     # both flatteners: the same requests, value by value
    lens = sorted((int(k) >> 32) & 0xFFFF for k in wb.dict if k)
    assert lens.count(MAX_STRLEN) == 3, lens[-5:]     # s, `other` and the constant less one byte, each once, the length intact in its 16 bits
    compare(inputs, want, hostsim_api.check(lt, hb, NOW, F_WANT_DERIVED_ROLES), "limits, host flattener")
    compare(inputs, want, hostsim_api.check(lt, wu.to_batch(lt, wb), NOW, F_WANT_DERIVED_ROLES), "limits, device flattener")
    _, _, longer = too_long_input()
    data, off = wire.pack_messages([wire.encode_check_input(i) for i in longer])
    rc, wb2 = wu.sim_flatten(lt, data, off)
    assert rc == 0 and wb2.stats["n_host"] == 2 and wb2.stats["first_bad"] == 0xFFFFFFFF
    it = IngestTable(lt.blob)     # cbi_flatten_pb has no such limit: the host road decides them
    try:
        hb2 = it.flatten_pb(data, off, sort=False)
        compare(longer, oracle_answers(rt, longer), hostsim_api.check(lt, hb2, NOW, F_WANT_DERIVED_ROLES), "limits, 65 536 bytes by the host flattener")
    finally:
        it.close()


def check_length_limits_on_library(capi):
    from cerbos_amd.engine import Conf, HipEvaluator
    rt, lt, inputs, want = length_limit_store()
    info = both_roads(capi, lt, inputs, want, "limits")
    assert info["n_host"] == 0
    _, _, longer = too_long_input()
    data, off = wire.pack_messages([wire.encode_check_input(i) for i in longer])
    table = capi.Table(lt.blob)
    try:
        with pytest.raises(capi.HostFlattenerNeeded):
            table.wire_flatten(data, off)
    finally:
        table.close()
    ev = HipEvaluator(lt, Conf())
    try:
        want_longer = oracle_answers(rt, longer)
        raw, flags = ev.check_pb(data, off, now_ns=NOW)
        assert ev.last_road == "host"
        compare_outputs(longer, want_longer, raw, flags, "limits, the evaluator's fallback")
        raw, flags = ev.check_pb(*wire.pack_messages([wire.encode_check_input(i) for i in inputs]), now_ns=NOW)
        assert ev.last_road == "device"
        compare_outputs(inputs, want, raw, flags, "limits, the evaluator's device road")
    finally:
        ev.close()


# ---- part 6: contention (GPU only)
def check_contended_claims(capi, n=250_000, per_principal=4_000, oracle_stride=1):
    """Every message carries the same four unknown strings - a colliding pair V, W and a near-collision N1, N2 - so every wave claims
    the same slots at once, and every message's decisions hinge on keeping each pair APART: tags = [W, N2] against a team that is V, W,
    N1 or another string by group (`exists` holds for W alone: a lane that took W's slot for V, or N2's for N1, allows what the oracle
    denies), members = [V, N1] against a principal id that is W, V, N2 or the group's own (`in` holds for V alone).  Beside them a
    string of its own (R.attr.a, against P.attr.mine) and a string it shares with exactly one message half the batch away (R.attr.b,
    against P.attr.twin).  Request road: principals of `per_principal` resource entries each.
    The oracle is SAMPLED at the GPU size (`oracle_stride` > 1): it answers the first eight entries of every group - the only ones
    `mine` and `twin` can name - and every `oracle_stride`-th input; the others repeat their group's answers for exists / member (same
    principal, same tags and members in every entry: asserted on each sampled one) and are denied own / twin.  The strings meant to
    be confused are in every message, so they are in every message the oracle sees.  The host road answers all of them."""
    nm = Names(9)
    docs = [_policy("doc", [_rule("exists", "R.attr.tags.exists(t, t == P.attr.team)"), _rule("member", "P.id in R.attr.members"),
                            _rule("own", 'R.attr.a == P.attr.mine'), _rule("twin", "R.attr.b == P.attr.twin")])]
    rt = rule_table_from_policies(policies_from_docs(docs))
    lt = lower_rule_table(rt)
    half = n // 2
    groups = []
    for g0 in range(0, n, per_principal):
        g = g0 // per_principal
        pid = (nm.W, nm.V, nm.N2, "principal%d" % g, "principal%d" % g)[g % 5]
        team = (nm.V, nm.W, nm.N1, "team%d" % g)[g % 4]
        pr = {"id": pid, "roles": ["user"], "attr": {"team": team, "mine": "own%d" % (g0 + g % 7), "twin": "twin%d" % ((g0 + 3) % half)}}
        groups.append([{"requestId": "c%d" % g, "actions": ["exists", "member", "own", "twin"], "principal": pr,
                        "resource": {"kind": "doc", "id": "r", "attr": {"tags": [nm.W, nm.N2], "members": [nm.V, nm.N1],
                                                                         "a": "own%d" % i, "b": "twin%d" % (i % half)}}} for i in range(g0, min(n, g0 + per_principal))])
    assert len(groups) >= 8     # every team and every principal id above occurs
    inputs = [i for g in groups for i in g]
    orc = RuleTableOracle(rt)
    want = []
    for g in groups:
        base = None
        for j, inp in enumerate(g):
            if j < 8 or base is None or (len(want) % oracle_stride == 0):
                o = orc.check(inp, EvalParams(now_ns=NOW))
                al = [o["actions"][a]["effect"] == "EFFECT_ALLOW" for a in inp["actions"]]
                assert not o.get("evaluationErrors")
                if j >= 8:
                    assert al == base, (len(want), al, base)
                elif j == 7:
                    base = al[:2] + [False, False]
            else:
                al = base
            want.append((al, False))
    seen = [{al[k] for al, _ in want} for k in range(4)]
    assert all(v == {True, False} for v in seen), seen
    table, it = capi.Table(lt.blob), IngestTable(lt.blob)
    try:
        reqs = [wire.encode_check_resources_request(_request_of(g)) for g in groups]
        outs, flags, _ = table.wire_check_requests_pb(reqs, now_ns=NOW, flags=F_WANT_DERIVED_ROLES)
        flat = [b for o in outs for b in o]
        compare_outputs(inputs, want, flat, flags, "contended claims, request road")
        data, off = wire.pack_messages([wire.encode_check_input(i) for i in inputs])
        hb = it.flatten_pb(data, off)
        host = table.check(hb, now_ns=NOW, flags=F_WANT_DERIVED_ROLES, device_order=True)
        host_out, host_flags = it.assemble_pb(hb, host, data, off)
        compare(inputs, want, host.to_input_order(hb), "contended claims, host road")
        assert flat == host_out and np.array_equal(flags, host_flags)
        db = table.wire_flatten(data, off)
        try:
            table.launch(db, now_ns=NOW, flags=F_WANT_DERIVED_ROLES)
            compare(inputs, want, table.download(db), "contended claims, cbh_wire_flatten")
            assert db.wire_info["n_host"] == 0
        finally:
            db.close()
    finally:
        table.close()
        it.close()


# ---- CPU tier: the emulator ...
@pytest.mark.parametrize("which", ["flat", "derived", "eval"])
def test_ids_on_emulator(which):
    check_ids_on_emulator(which)


def test_lost_claims_on_emulator():
    check_lost_claims()


def test_regrowth_twin_on_emulator():
    """hostsim.cpp's own retry loop from sixteen slots and a heap of one entry: the part 2 store, every id and decision as before"""
    wb = check_ids_on_emulator("eval", dict_slots=16, heap=1)
    assert wb.fill_runs > 2 and wb.dict_slots > 16, (wb.fill_runs, wb.dict_slots)


def test_length_limits_on_emulator():
    check_length_limits_on_emulator()


# ---- ... and the simulator build of the library
@pytest.fixture()
def engine():
    from sim_engine import sim_engine
    with sim_engine() as capi:
        yield capi


@pytest.mark.parametrize("which", ["flat", "derived", "eval"])
def test_ids_on_simulator(engine, which):
    check_ids_on_library(engine, which)


def test_regrowth_on_simulator(engine):
    check_regrowth_on_library(engine)


def test_regrowth_in_slices_on_simulator():
    regrowth_in_slices_in_child(True, 512, 128)


def test_length_limits_on_simulator(engine):
    check_length_limits_on_library(engine)


def test_contended_claims_body_on_simulator(engine):
    """the body of the GPU test at a size the fiber scheduler finishes (it proves the test, not the hardware)"""
    check_contended_claims(engine, n=1_200, per_principal=150)


# ---- GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["flat", "derived", "eval"])
def test_ids_on_gpu(which):
    from cerbos_amd import capi
    check_ids_on_library(capi, which)


@pytest.mark.gpu
def test_regrowth_on_gpu():
    from cerbos_amd import capi
    check_regrowth_on_library(capi, n=320, per=150)


@pytest.mark.gpu
def test_regrowth_in_slices_on_gpu():
    sim = os.environ.get("CBH_TEST_SIM_ENGINE") == "1"
    regrowth_in_slices_in_child(sim, 512 if sim else 2048, 128 if sim else 512)


@pytest.mark.gpu
def test_length_limits_on_gpu():
    from cerbos_amd import capi
    check_length_limits_on_library(capi)


@pytest.mark.gpu
def test_contended_claims_on_gpu():
    """Run once.  Under CBH_TEST_SIM_ENGINE=1 the same body at a size the simulator finishes."""
    from cerbos_amd import capi
    if os.environ.get("CBH_TEST_SIM_ENGINE") == "1":
        check_contended_claims(capi, n=1_200, per_principal=150)
    else:
        check_contended_claims(capi, n=250_000, per_principal=4_000, oracle_stride=16)
