#!/usr/bin/env python3
"""End-to-end rate of a cross-product review (N principals x M resources x A actions), halves already flattened:

  host leg    what a caller had before cbh_batch_upload_cross: cross_product_batch (numpy lays out N * M rows on the host) +
              Table.upload (all N * M rows cross the link) + launch + download(want=()) (one byte per tuple back)
  device leg  upload_cross (N + M rows up, the device expands them) + launch + download_allow_bits (one bit per tuple back)
  direct leg  cross_upload (N + M rows up, nothing expanded) + CrossSet.check over all M resources (one bit per tuple back, as planes);
              timed ALTERNATING with the device leg, repetition by repetition, in the same process

per configuration: 3 warm-ups, then at least 10 timed repetitions of each leg, wall clock from a synchronised device to the last
byte on the host; min / median / max in decisions per second.  Plus the launch alone for both batches (the resident batch is the
same, so it must not differ).

  python tools/cross_bench.py                      both legs, C2 and T, 1024 x 1024 and 4096 x 1024, A = 4
  python tools/cross_bench.py --host-only          the host leg alone: runs on a commit that has no device leg (the baseline; this
                                                   file is the only one copied over)
  python tools/cross_bench.py --profile c2:1024:1024
                                                   ONE device leg and nothing else, for a kernel trace (rocprofv3 --kernel-trace --stats
                                                   -- python tools/cross_bench.py --profile ...); prints the bytes the expansion
                                                   and cbh_compact_pack_kernel write, to be divided by the trace's kernel times
  python tools/cross_bench.py --profile-direct c2:4096:1024
                                                   ONE direct leg and nothing else, for a kernel trace
  python tools/cross_bench.py --skip-host --configs c3:4096:1024,c2:4096:1024:16
                                                   a configuration is NAME:N:M or NAME:N:M:A - C3 (derived roles) and more than four
                                                   actions go direct through cbh_cross_upload_ex (every `accept` bit set); A > 4 takes
                                                   the workload's further actions, then names no policy knows.  --skip-host: without
                                                   the host leg (numpy lays out N * M * A on the host: minutes at 4096 x 1024 x 16)
  python tools/cross_bench.py --skip-host --configs c2:4096:1024:r8
                                                   a last field rR gives EVERY principal R roles (5 .. 16): the workload's own first,
                                                   then roles no policy names, then one role an ALLOW rule names - the deciding
                                                   role sits in the last group of four.  The direct legs pass every `accept` bit,
                                                   CX_ROLE_GROUPS among them; the device leg's product takes the walk's kernels
  python tools/cross_bench.py --check-alone c3:4096:1024
                                                   the direct check alone (inputs resident, planes copied to the host), one line: for an
                                                   A/B of two builds or switches (CBH_CROSS_DR_MEMO=0), one process per repetition
  python tools/cross_bench.py --pairs c3:4096:1024:65536
                                                   CrossSet.pairs_batch of that many random pairs, wall clock (under rocprofv3
                                                   --kernel-trace --stats: the device time of cbh_cross_gather_kernel)
  python tools/cross_bench.py --review c2:4096:1024
                                                   what a review costs, inputs resident, four bodies ALTERNATING in one process, wall
                                                   clock in ms: (a) check with both kinds of planes + the numpy reduction to counts +
                                                   cross.flagged_pairs - what a caller did before cbh_cross_review; (b) that check
                                                   alone; (c) CrossSet.review, every count, no list; (d) review with the flagged list, in one call (pair_cap = twice the list's length).
                                                   C3 runs under F_WANT_DERIVED_ROLES (its flagged list is not empty)
  python tools/cross_bench.py --profile-review c2:4096:1024
                                                   body (c) three times and nothing else, for rocprofv3 --kernel-trace --stats
One JSON line per configuration on stdout."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cerbos_amd import capi, cross, workloads  # noqa: E402
from cerbos_amd.flatten import Flattener  # noqa: E402
from cerbos_amd.lower.blob import lower_rule_table  # noqa: E402
from cerbos_amd.policy.loader import policies_from_docs  # noqa: E402
from cerbos_amd.ruletable.build import rule_table_from_policies  # noqa: E402

NOW = 1_700_000_000_000_000_000


class Flattened:
    """the halves flattened ONCE, before any clock starts: cross.py asks its flattener for them on every call"""

    def __init__(self, fl):
        self.fl, self.h = fl, None

    def flatten(self, inputs, default_policy_version="default", default_scope="", sort=True):
        if self.h is None:
            self.h = self.fl.flatten(inputs, default_policy_version, default_scope, sort=sort)
        return self.h


def stats(times, decisions):
    t = np.sort(np.asarray(times))
    return {"min": decisions / t[-1], "median": decisions / float(np.median(t)), "max": decisions / t[0], "reps": int(t.size)}


def timed(table, reps, warmup, body):
    out = []
    for k in range(warmup + reps):
        table.synchronize()
        t0 = time.perf_counter()
        keep = body()
        table.synchronize()
        dt = time.perf_counter() - t0
        if keep is not None:
            keep.close()
        if k >= warmup:
            out.append(dt)
    return out


ACCEPT = capi.CX_ALL | capi.CX_ROLE_GROUPS
ROLES = [None]   # the rR suffix of the configuration being run (parse)


def parse(cfg):
    """NAME:N:M[:A][:rR] -> (name, n, m, a or None); R is left in ROLES for setup"""
    f = cfg.split(":")
    ROLES[0] = int(f.pop()[1:]) if f[-1].startswith("r") else None
    return f[0], int(f[1]), int(f[2]), (int(f[3]) if len(f) > 3 else None)


def widen(docs, principals, r):
    """every principal with r roles: its own first, roles no policy names, and last a role an ALLOW rule names (one it does not hold
    yet, else its own last role moved there)"""
    allowing = []
    for d in docs:
        for rule in d.get("resourcePolicy", {}).get("rules", []):
            if rule.get("effect") == "EFFECT_ALLOW":
                allowing += [x for x in rule.get("roles", []) if x not in allowing and x != "*"]
    out = []
    for p in principals:
        own = list(p["roles"])[:r - 1]
        new = [x for x in allowing if x not in own]
        last = new[0] if new else own.pop()
        out.append(dict(p, roles=own + ["norole%02d" % i for i in range(r - 1 - len(own))] + [last]))
    return out


def setup(name, n, m, a=None):
    docs = getattr(workloads, name + "_policies")()
    lt = lower_rule_table(rule_table_from_policies(policies_from_docs(docs)))
    ins = getattr(workloads, name + "_requests")(n + m, seed=17).to_inputs()
    principals, resources, actions = [i["principal"] for i in ins[:n]], [i["resource"] for i in ins[n:]], list(ins[0]["actions"])
    if ROLES[0]:
        principals = widen(docs, principals, ROLES[0])
    if a is not None:     # the workload's own actions first, then its further ones, then names no policy knows
        more = [x for x in getattr(workloads, name.upper() + "_ACTIONS", []) if x not in actions]
        actions = (actions + more + ["unknown%02d" % i for i in range(64)])[:a]
    fl = Flattened(Flattener(lt))
    table = capi.Table(lt.blob)
    table.set_resident_streams(1)
    return lt, table, fl, principals, resources, actions


def host_leg(lt, table, fl, p, r, a):
    def body():
        cb = cross.cross_product_batch(fl, lt.columns, p, r, a)
        db = table.upload(cb)
        table.launch(db, now_ns=NOW)
        table.download(db, want=())
        return db
    return body


def device_leg(lt, table, fl, p, r, a):
    def body():
        db = cross.cross_product_upload(table, fl, lt.columns, p, r, a)
        table.launch(db, now_ns=NOW)
        table.download_allow_bits(db)
        return db
    return body


def direct_leg(lt, table, fl, p, r, a):
    def body():
        cs = cross.cross_direct_upload(table, fl, lt.columns, p, r, a, accept=ACCEPT)
        if cs is None:
            raise SystemExit("the set has no direct form")
        cs.check(0, len(r), now_ns=NOW)
        return cs
    return body


def timed_alternating(table, reps, warmup, bodies):
    """the bodies in turn, repetition by repetition: what drifts over the run (clocks, the pool) drifts for all of them"""
    out = [[] for _ in bodies]
    for k in range(warmup + reps):
        for i, body in enumerate(bodies):
            dt = timed(table, 1, 0, body)[0]
            if k >= warmup:
                out[i].append(dt)
    return out


def review_bodies(cs, n, m, a, flags, cap):
    """(a) .. (d) of --review; each returns None (nothing to close)"""
    def reduce_on_host():
        allow, flagged = cs.check(0, m, flags=flags, now_ns=NOW, want_flagged=True)
        for planes in (allow, flagged):
            by = np.ascontiguousarray(planes, dtype="<u8").view(np.uint8).reshape(a, -1)
            bits = np.unpackbits(by, axis=1, count=n * m, bitorder="little").reshape(a, m, n)
            bits.sum(axis=1, dtype=np.uint32), bits.sum(axis=2, dtype=np.uint32), bits.sum(axis=(1, 2), dtype=np.uint64)
        cross.flagged_pairs(cs, 0, m, flagged)

    def check_alone():
        cs.check(0, m, flags=flags, now_ns=NOW, want_flagged=True)

    def review_counts():
        cs.review(0, m, flags=flags, now_ns=NOW, want_flagged=True)

    def review_list():
        cs.review(0, m, flags=flags, now_ns=NOW, want_flagged=True, pairs="flagged", pair_cap=cap)     # (one call: a cap the caller knows to be enough)
    return [reduce_on_host, check_alone, review_counts, review_list]


def ms(times):
    return {"min": min(times) * 1e3, "median": float(np.median(times)) * 1e3, "max": max(times) * 1e3, "reps": len(times)}


def launch_alone(table, db, reps, warmup):
    def body():
        table.launch(db, now_ns=NOW)
    return timed(table, reps, warmup, body)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="c2:1024:1024,c2:4096:1024,t:1024:1024,t:4096:1024")
    ap.add_argument("--profile", default=None, metavar="NAME:N:M")
    ap.add_argument("--profile-direct", default=None, metavar="NAME:N:M[:A][:rR]")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--check-alone", default=None, metavar="NAME:N:M[:A][:rR]")
    ap.add_argument("--pairs", default=None, metavar="NAME:N:M:COUNT")
    ap.add_argument("--review", default=None, metavar="NAME:N:M[:A]")
    ap.add_argument("--profile-review", default=None, metavar="NAME:N:M[:A]")
    args = ap.parse_args()
    if args.reps < 10:
        ap.error("at least 10 timed repetitions")
    capi.init(0)
    if args.check_alone:
        name, n, m, na = parse(args.check_alone)
        lt, table, fl, p, r, a = setup(name, n, m, na)
        cs = direct_leg(lt, table, fl, p, r, a)()
        t = timed(table, args.reps, args.warmup, lambda: cs.check(0, m, now_ns=NOW) and None)
        print(json.dumps({"check_alone": args.check_alone, "kernel": cs.describe(), "a": len(a),
                          "direct_check_alone": stats(t, n * m * len(a)), "median_ms": float(np.median(t)) * 1e3}), flush=True)
        cs.close()
        table.close()
        return
    if args.review or args.profile_review:
        name, n, m, na = parse(args.review or args.profile_review)
        lt, table, fl, p, r, a = setup(name, n, m, na)
        cs = direct_leg(lt, table, fl, p, r, a)()
        flags = capi.F_WANT_DERIVED_ROLES if name == "c3" else 0
        rv = cs.review(0, m, flags=flags, now_ns=NOW, want_flagged=True, pairs="flagged")
        bodies = review_bodies(cs, n, m, len(a), flags, max(1024, 2 * rv.n_pairs))
        if args.profile_review:
            for _ in range(3):
                bodies[2]()
            print(json.dumps({"profile_review": args.profile_review, "kernel": cs.describe(flags), "reviews": 3,
                              "plane_bytes_read_per_review": 2 * len(a) * ((n * m + 63) // 64) * 8}), flush=True)
        else:
            t = timed_alternating(table, args.reps, args.warmup, bodies)
            line = {"review": args.review, "kernel": cs.describe(flags), "a": len(a), "decisions": n * m * len(a), "unit": "ms, wall clock",
                    "allowed": int(rv.totals[0].sum()), "flagged": int(rv.totals[1].sum()), "flagged_pairs": rv.n_pairs,
                    "a_check_numpy_counts_and_pairs": ms(t[0]), "b_check_alone": ms(t[1]), "c_review_counts": ms(t[2]), "d_review_counts_and_list": ms(t[3])}
            line["c_median_over_b_median"] = line["c_review_counts"]["median"] / line["b_check_alone"]["median"]
            line["a_median_over_c_median"] = line["a_check_numpy_counts_and_pairs"]["median"] / line["c_review_counts"]["median"]
            line["a_median_over_d_median"] = line["a_check_numpy_counts_and_pairs"]["median"] / line["d_review_counts_and_list"]["median"]
            print(json.dumps(line), flush=True)
        cs.close()
        table.close()
        return
    if args.pairs:
        name, n, m, cnt = parse(args.pairs)
        lt, table, fl, p, r, a = setup(name, n, m)
        cs = direct_leg(lt, table, fl, p, r, a)()
        rng = np.random.default_rng(5)
        pp, pr = rng.integers(0, n, size=cnt).astype(np.uint32), rng.integers(0, m, size=cnt).astype(np.uint32)
        t = timed(table, args.reps, args.warmup, lambda: cs.pairs_batch(pp, pr))
        db = cs.pairs_batch(pp, pr)
        t2 = launch_alone(table, db, args.reps, args.warmup)
        print(json.dumps({"pairs": args.pairs, "columns": len(lt.columns), "plan": table.plan(db),
                          "pairs_batch_ms": {"min": min(t) * 1e3, "median": float(np.median(t)) * 1e3, "max": max(t) * 1e3},
                          "launch_alone": stats(t2, cnt * len(a)),
                          "cbh_cross_gather_kernel_bytes_written": cnt * (64 + 9 * len(lt.columns))}), flush=True)
        db.close()
        cs.close()
        table.close()
        return
    if args.profile_direct:
        name, n, m, na = parse(args.profile_direct)
        lt, table, fl, p, r, a = setup(name, n, m, na)
        cs = direct_leg(lt, table, fl, p, r, a)()
        print(json.dumps({"profile_direct": args.profile_direct, "kernel": cs.describe(), "columns": len(lt.columns),
                          "plane_bytes_written": len(a) * ((n * m + 63) // 64) * 8}))
        cs.close()
        table.close()
        return
    if args.profile:
        name, n, m = args.profile.split(":")
        n, m = int(n), int(m)
        lt, table, fl, p, r, a = setup(name, n, m)
        db = device_leg(lt, table, fl, p, r, a)()
        plan = table.plan(db)
        ncol, nm, A = len(lt.columns), n * m, len(a)
        narrow = bin(int(plan.split("narrow columns 0x")[1].split("]")[0], 16)).count("1") if "narrow columns" in plan else 0
        print(json.dumps({"profile": args.profile, "plan": plan, "columns": ncol,
                          "cbh_cross_expand_kernel_bytes_written": nm * (64 + 9 * ncol),
                          "cbh_cross_actions_kernel_bytes_written": nm * A * 4,
                          "cbh_compact_pack_kernel_bytes_written": nm * (16 + 4 * narrow),
                          "cbh_allow_bits_kernel_bytes_written": (nm * A + 63) // 64 * 8}))
        db.close()
        table.close()
        return
    for cfg in args.configs.split(","):
        name, n, m, na = parse(cfg)
        lt, table, fl, p, r, a = setup(name, n, m, na)
        decisions = n * m * len(a)
        line = {"workload": name, "n": n, "m": m, "a": len(a), "decisions": decisions, "columns": len(lt.columns),
                "unit": "decisions per second, end to end (min / median / max over the timed repetitions)"}
        if not args.skip_host:
            line["host_leg"] = stats(timed(table, args.reps, args.warmup, host_leg(lt, table, fl, p, r, a)), decisions)
            hb = table.upload(cross.cross_product_batch(fl, lt.columns, p, r, a))
            line["host_batch_plan"] = table.plan(hb)
            line["host_batch_launch_alone"] = stats(launch_alone(table, hb, args.reps, args.warmup), decisions)
            hb.close()
        if not args.host_only:
            dev_t, dir_t = timed_alternating(table, args.reps, args.warmup, [device_leg(lt, table, fl, p, r, a), direct_leg(lt, table, fl, p, r, a)])
            line["device_leg"] = stats(dev_t, decisions)
            line["direct_leg"] = stats(dir_t, decisions)
            cs = cross.cross_direct_upload(table, fl, lt.columns, p, r, a, accept=ACCEPT)
            line["direct_kernel"] = cs.describe()

            def check_alone():
                cs.check(0, m, now_ns=NOW)
            line["direct_check_alone"] = stats(timed(table, args.reps, args.warmup, check_alone), decisions)
            cs.close()
            db = cross.cross_product_upload(table, fl, lt.columns, p, r, a)
            line["device_batch_plan"] = table.plan(db)
            line["device_batch_launch_alone"] = stats(launch_alone(table, db, args.reps, args.warmup), decisions)
            db.close()
            if not args.skip_host:
                line["device_slowest_over_host_fastest"] = line["device_leg"]["min"] / line["host_leg"]["max"]
        table.close()
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
