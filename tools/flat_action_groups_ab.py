#!/usr/bin/env python3
"""A/B of the flat kernels' action groups (cerbos_hip.h CBH_HAS_FLAT_ACTION_GROUPS) against the plan without them
(CBH_FLAT_ACTION_GROUPS=0: the walk's kernels and the general walk), resident and synchronised.

C2's and C3's tables, --requests requests (default 250 000) per batch at three action distributions:
  all8     every request asks for 8 actions
  all16    every request asks for 16
  ui       uniform over 1 .. 10 actions, 1 % of the requests at 40
and, with --dists, any of: allN (every request N actions), uiN (uniform over 1 .. 10, 1 % at N) - the shapes between and beyond
the three, for the plan's bounds on the group count.
The switch is read once per process, so every repetition of either setting is a child process of its own; the two settings
alternate, --reps repetitions each, in this one call, so that clock and thermal drift fall on both.  A child uploads the six
batches, warms each up, then times --steps launches of each followed by cbh_synchronize, and prints one JSON line per shape.
The parent prints the children's lines as they come and, at the end, per shape the decisions/s min - max of both settings and
whether the ranges lie apart (the slowest repetition with action groups beats the fastest without).
usage: python tools/flat_action_groups_ab.py [--requests 250000] [--reps 5] [--steps 10] [--dists all8,all16,ui]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NOW = 1_700_000_000_000_000_000
DISTS = ("all8", "all16", "ui")


def _counts(dist, n, rng):
    import numpy as np
    if dist.startswith("all"):
        return np.full(n, int(dist[3:]))
    cnt = rng.integers(1, 11, n)
    cnt[rng.random(n) < 0.01] = int(dist[2:] or 40)
    return cnt


def _requests(name, dist, n):
    """the workload's requests with the action lists re-dealt: distinct names per request, the workload's own first (in random
    order), then names no rule has"""
    import numpy as np
    from cerbos_amd import workloads
    from cerbos_amd.columnar import Ragged
    cr = getattr(workloads, name + "_requests")(n)
    own = list(cr.actions.values)
    names = own + ["other%02d" % i for i in range(64 - len(own))]
    rng = np.random.default_rng(len(dist) * 1000 + len(own))
    cnt = _counts(dist, n, rng)
    off = np.concatenate([[0], np.cumsum(cnt)])
    flat = np.empty(int(off[-1]), dtype=np.int64)
    head = np.argsort(rng.random((n, len(own))), axis=1)                  # a permutation of the workload's own actions per request
    pos = np.arange(int(off[-1])) - np.repeat(off[:-1], cnt)              # index of an action within its request
    req = np.repeat(np.arange(n), cnt)
    inner = pos < len(own)
    flat[inner] = head[req[inner], pos[inner]]
    flat[~inner] = pos[~inner]
    cr.actions = Ragged(names, off, flat)
    return cr


def child(args):
    from cerbos_amd import capi, workloads          # (the built library: a missing one is an error here, nothing is compiled in a timed child)
    from cerbos_amd.flatten import Flattener
    from cerbos_amd.lower.blob import lower_rule_table
    from cerbos_amd.policy.loader import policies_from_docs
    from cerbos_amd.ruletable.build import rule_table_from_policies
    capi.init(0)
    flags = capi.F_WANT_DERIVED_ROLES
    for name in ("c2", "c3"):
        lt = lower_rule_table(rule_table_from_policies(policies_from_docs(getattr(workloads, name + "_policies")())))
        table, fl = capi.Table(lt.blob), Flattener(lt)
        table.set_resident_streams(1)
        for dist in args.dists.split(","):
            host = _requests(name, dist, args.requests).to_batch(fl)
            db = table.upload(host)
            for _ in range(2):
                table.launch(db, now_ns=NOW, flags=flags)
            table.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                table.launch(db, now_ns=NOW, flags=flags)
            table.synchronize()
            dt = time.perf_counter() - t0
            print(json.dumps({"table": name.upper(), "dist": dist, "action_groups": os.environ.get("CBH_FLAT_ACTION_GROUPS", "1") != "0",
                              "requests": host.n_requests, "tuples": host.n_tuples, "decisions_per_s": host.n_tuples * args.steps / dt,
                              "plan": table.plan(db, flags)}), flush=True)
            db.close()
        table.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=250_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--dists", default=",".join(DISTS))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    rates = {}
    for rep in range(args.reps):
        for switch in ("1", "0"):
            env = dict(os.environ, CBH_FLAT_ACTION_GROUPS=switch)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--requests", str(args.requests), "--steps", str(args.steps), "--dists", args.dists],
                               env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                sys.exit("a child process failed (exit %d)" % r.returncode)
            for line in r.stdout.splitlines():
                if not line.startswith("{"):
                    continue
                print(line, flush=True)
                d = json.loads(line)
                rates.setdefault((d["table"], d["dist"]), {True: [], False: []})[d["action_groups"]].append(d["decisions_per_s"])
    for (table, dist), r in sorted(rates.items()):
        on, off = r[True], r[False]
        print(json.dumps({"summary": "%s %s" % (table, dist), "groups_min": min(on), "groups_max": max(on), "without_min": min(off), "without_max": max(off),
                          "ranges_apart": min(on) > max(off), "ratio_of_medians": sorted(on)[len(on) // 2] / sorted(off)[len(off) // 2]}), flush=True)


if __name__ == "__main__":
    main()
