"""The planner's slot residency (csrc/residency.hpp) on a host model (no GPU).

Which sections of the arena the device still holds, which K0 runs (every row,
the changed columns and rows only, or none) and how little goes up per tick
is decided by plain host arithmetic.  tools/encode_stats' `residency` mode
drives it with the real encoder over ticks of fresh snapshots -- a 16-candidate
prefix and the every-candidate input on two slots over one encoder, pods added
one at a time, in bursts and all removed again, the spot order moving -- and
executes the staging writes and the listed copies on two plain buffers, the
models of the pinned staging arena and of the device arena.  Every tick it
checks that staging equals the workload, that after a K0 run (its node and
pod patches applied) the device arena does too, that a K0-less run differs
only in the nodes and pods handed to K2 as patches, that an incremental K0's
column and row lists cover everything that changed since the last K0 run, and
that bytes_uploaded is the sum of the counted copies.  By tick number it
injects a prepare that is never run, a moved staging, arena and tables
allocation, and a failing encode."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "k8s-spot-rescheduler_amd")
TOOL = os.path.join(PKG, "bin", "encode_stats")

SUMMARY = re.compile(
    r"residency check: (\d+) ticks \((\d+) full K0, (\d+) incremental, (\d+) K0-less\), never run (\d+), "
    r"arena moved (\d+), tables moved (\d+), staging moved (\d+), list reorders (\d+), encode errors (\d+), "
    r"spot order moved (\d+), violations (\d+)")
FIELDS = ("ticks", "full", "incremental", "k0_less", "never_run", "arena_moved", "tables_moved", "staging_moved",
          "reorders", "encode_errors", "spot_moved", "violations")


@pytest.fixture(scope="module")
def tool():
    subprocess.run(["make", "-C", PKG, "-j8", "tools"], check=True, stdout=subprocess.DEVNULL)
    return TOOL


@pytest.mark.parametrize("config", [2, 3, 5])
def test_residency_model(tool, config):
    """Zero violations over 60 ticks of two inputs each, with each K0 mode and
    each injected event seen at least once."""
    run = subprocess.run([tool, str(config), "100000", "residency", "60", "24"], capture_output=True, text=True,
                         timeout=600)
    m = SUMMARY.search(run.stdout)
    assert m, run.stdout + run.stderr
    r = dict(zip(FIELDS, map(int, m.groups())))
    assert r["violations"] == 0 and run.returncode == 0, run.stdout
    assert r["ticks"] == 119, run.stdout  # 60 ticks x 2 inputs, one of them failing its encode
    for seen in ("full", "incremental", "k0_less", "never_run", "arena_moved", "tables_moved", "staging_moved",
                 "encode_errors", "spot_moved"):
        assert r[seen] >= 1, (seen, run.stdout)
    if config == 3:  # the one list long enough to be reordered by cost (more than 1,024 entries)
        assert r["reorders"] >= 1, run.stdout
