"""The compact flat kernels' prologue, read off the shipped library's machine code (tools/audit_prologue_waits.py; no GPU): how many
trips to memory it makes, and whether the copies of its first trip go out back to back.

Before the chain's first scope came with the record (cbh_vm.h cbh_creq_first) the three compact instantiations showed 4 / 5 / 5 trips
that carry loads up to the scan's limit - one of them the record with the columns' and the tags' copies, three of them chain_first's
per-lane loads of the scope arrays - and four scalar-memory waits inside the first trip, with cc_fill_compact's loops still loops
(ten backward branches in static order; a wait per tag group and per column when executed, about ten on C2).
Now ONE trip in all three (the bound asked for: 1 / 2 / 2), and no backward branch: every copy is issued once, in unrolled code.

Scalar-memory waits inside the first trip: at most one was asked for.  Reached: 3 / 4 / 3 in static order, each executed ONCE per wave
(none per column), all between the record's load and the first copy: one is cc_fill_compact's own read-once of its three counts,
the other two are the compiler's - it reads arguments the walk needs later (`s_load_dwordx4 .. 0x10`, `0x20`, `0x154`) at that place
in order to spill them, and re-reads the sixteen dwords at 0x238 it had at the kernel's entry.  With the copies in FRONT of the
record's load the count is 1 / 3 / 1 (0 / 2 / 0 with vector addresses) - and the launch is slower:
the record, the largest item of the trip, then leaves last (profiles/compact_first_trip_ab.txt has both builds and the excerpt).  The
counts reached are pinned; a source that brings them to the one asked for may lower the pins."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cerbos_amd", "libcerbos_hip.so")


def _audit(kernel, trips, waits):
    assert os.path.exists(LIB), "build the library first (__graft_entry__.build)"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_prologue_waits.py"), "--max-trips", str(trips),
                        "--max-first-trip-scalar-waits", str(waits), kernel], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    return r


@pytest.mark.parametrize("kernel,trips,waits", [("cbh_check_flat_kernel_c10", 1, 3), ("cbh_check_flat_kernel_masks_c10", 2, 4),
                                                ("cbh_check_flat_kernel_staged_c10", 2, 3)])
def test_compact_prologue_is_one_trip_without_a_loop(kernel, trips, waits):
    r = _audit(kernel, trips, waits)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lds-copy" in r.stdout.split("trip 1:")[1].splitlines()[0], r.stdout          # the copies ARE in the first trip
    assert " 0 backward branches" in r.stdout, r.stdout


def test_the_new_options_can_fail():
    """the wide-input flat kernel makes more than one trip, and the compact one has more than zero scalar-memory waits: the options
    that pin the compact kernels are not vacuous"""
    r = _audit("cbh_check_flat_kernel10", 1, 8)
    assert r.returncode == 1 and "trips that carry loads (more than 1)" in r.stdout, r.stdout + r.stderr
    r = _audit("cbh_check_flat_kernel_c10", 1, 0)
    assert r.returncode == 1 and "scalar-memory waits, or a loop, inside the first trip" in r.stdout, r.stdout + r.stderr
