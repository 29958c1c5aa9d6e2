#!/usr/bin/env python3
"""Resident decision rate of C2 written in CEL optional syntax (workloads.c2_optional_policies) against plain C2.

Both tables decide the same resident batches (4 seeded batches of 250k requests, bench.py's C2 batch size) with the same flags;
the two are timed in alternating rounds so that clock and thermal drift fall on both.  Both flatten through the general
Flattener: the columnar route has no whole-attribute-map column, which the presence leaf `"x" in R.attr` reads.  Prints one JSON line: per
table the best and median rate over the rounds, the kernels cbh_check_resident launches (cbh_plan_describe), and the ratio.
usage: python tools/bench_optional_c2.py [--rounds 5] [--steps 10] [--batches 4]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--requests", type=int, default=250_000)
    args = ap.parse_args()

    import __graft_entry__
    __graft_entry__.build()
    from cerbos_amd import capi, workloads
    from cerbos_amd.flatten import Flattener
    from cerbos_amd.lower.blob import lower_rule_table
    from cerbos_amd.policy.loader import policies_from_docs
    from cerbos_amd.ruletable.build import rule_table_from_policies

    capi.init(0)
    now, flags = 1_700_000_000_000_000_000, capi.F_WANT_DERIVED_ROLES
    inputs = [workloads.c2_requests(args.requests, seed=2 + 1000 * k).to_inputs() for k in range(args.batches)]
    legs = {}
    for name, pol in (("C2", workloads.c2_policies), ("C2_optional", workloads.c2_optional_policies)):
        lt = lower_rule_table(rule_table_from_policies(policies_from_docs(pol())))
        table, fl = capi.Table(lt.blob), Flattener(lt)
        host = [fl.flatten(inp) for inp in inputs]
        db = [table.upload(b) for b in host]
        for _ in range(2):
            table.launch_many(db, now_ns=now, flags=flags)
        table.synchronize()
        res = table.download(db[0])
        assert (res.status != capi.ST_UNSUPPORTED).all()
        legs[name] = {"table": table, "db": db, "tuples": host[0].n_tuples * len(db), "rates": [], "kernel": table.plan(db[0], flags)}
    for _ in range(args.rounds):
        for leg in legs.values():
            t0 = time.perf_counter()
            for _ in range(args.steps):
                leg["table"].launch_many(leg["db"], now_ns=now, flags=flags)
            leg["table"].synchronize()
            leg["rates"].append(leg["tuples"] * args.steps / (time.perf_counter() - t0))
    out = {name: {"best_decisions_per_s": max(leg["rates"]), "median_decisions_per_s": statistics.median(leg["rates"]),
                  "rounds": leg["rates"], "kernel": leg["kernel"]} for name, leg in legs.items()}
    out["optional_over_plain_best"] = out["C2_optional"]["best_decisions_per_s"] / out["C2"]["best_decisions_per_s"]
    out["optional_over_plain_median"] = out["C2_optional"]["median_decisions_per_s"] / out["C2"]["median_decisions_per_s"]
    print(json.dumps(out, default=str))


if __name__ == "__main__":
    main()
