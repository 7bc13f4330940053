"""The host tables of the streaming aggregate restriction (csrc/coarse_plan.cpp: the interior rows grouped by aggregate
and their cut into pieces of at most kCoarsePieceCap = 2048 rows) on the CPU, under the address and undefined-behaviour
sanitizers: tests/drivers/row_pieces_driver.cpp deals rows to aggregates of given sizes interleaved, plans the tables
and checks that every row of every aggregate lies in exactly one piece, that no piece exceeds the cap, and that the
pieces of an aggregate are consecutive in table order -- for aggregates of 0, 1, cap - 1, cap, cap + 1 and 2 cap + 1 rows
among others.  Pattern: tests/test_coarse_plan.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "schwarz-lib_amd")
DRIVER = os.path.join(PKG, "build", "row_pieces_driver")
CAP = 2048
CASES = ["edge_sizes", "edge_sizes_first_agg_40", "one_long_aggregate", "empty_aggregates_only", "refusals"]
CHECKS = ["rows_grouped_by_aggregate_ascending", "every_row_in_exactly_one_piece", "no_piece_longer_than_the_cap",
          "pieces_of_an_aggregate_consecutive_in_table_order"]


@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-C", PKG, "-s", "row_pieces_driver"])  # (nothing to do after build())
    return DRIVER


def run(driver, case):
    r = subprocess.run([driver, case], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert not r.stderr.strip(), r.stderr[-4000:]  # a sanitizer report
    assert r.returncode == 0, "%s: exit %d\n%s" % (case, r.returncode, r.stdout[-4000:])
    return r.stdout.splitlines()


def verdicts(lines):
    return {ln.split()[1]: ln.split()[2] for ln in lines if ln.startswith("check ")}


def figure(lines):
    f = [ln.split()[1:] for ln in lines if ln.startswith("figure ")][0]
    return {f[k]: int(f[k + 1]) for k in range(0, len(f), 2)}


def test_case_list(driver):
    listed = subprocess.run([driver, "--list"], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    assert listed == CASES


@pytest.mark.parametrize("case", CASES[:4])
def test_tables_hold_every_row_once(driver, case):
    lines = run(driver, case)
    print("\n".join(lines))
    got = verdicts(lines)
    assert sorted(got) == sorted(CHECKS)
    assert all(v == "pass" for v in got.values()), got


def test_shapes_of_the_cases(driver):
    """The piece counts follow from the sizes: 0 rows no piece, up to cap rows one, cap + 1 two, 2 cap + 1 three; the
    rows of no aggregate of the interleaved cases are one contiguous run."""
    sizes = [0, 1, CAP, CAP + 1, 2 * CAP + 1, 0, 2, 63, 64, 65, 255, 256, 257, CAP - 1, 0]
    f = figure(run(driver, "edge_sizes"))
    assert f == dict(rows=sum(sizes), aggregates=15, pieces=sum(-(-s // CAP) for s in sizes), longest=CAP, contiguous=0)
    assert f["pieces"] == 1 + 1 + 2 + 3 + 8
    f = figure(run(driver, "edge_sizes_first_agg_40"))
    assert f == dict(rows=4 * CAP + 3, aggregates=5, pieces=3 + 0 + 1 + 2 + 1, longest=CAP, contiguous=0)
    assert figure(run(driver, "one_long_aggregate")) == dict(rows=5 * CAP + 7, aggregates=1, pieces=6, longest=CAP,
                                                             contiguous=1)
    assert figure(run(driver, "empty_aggregates_only")) == dict(rows=0, aggregates=3, pieces=0, longest=0, contiguous=0)


def test_bad_tables_are_refused(driver):
    assert verdicts(run(driver, "refusals")) == {"bad_tables_are_refused_and_empty_ones_planned": "pass"}
