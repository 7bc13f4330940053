"""The uneven cuts of the z-sweep walks' segment tables (walk_segment_table, csrc/coding_plan.cpp) on the CPU, under the
address and undefined-behaviour sanitizers: tests/drivers/walk_trim_driver.cpp calls the function on geometry alone --
the flagship's three tables, the 512 x 512 x 64 slab, two-run chains, other CU counts, a run just under and one just at
the 16-position threshold -- for the trims 0, the library's defaults and 300 per mille, and checks coverage, the
unchanged size and band placement of the table, trim 0 against the equal-pieces formula, late pieces no longer than
early ones, the planner's floor and the threshold.  Here: the driver ends clean on every case, and what it prints for
the flagship says what SCHWZ_SWEEP_TRIM is documented to do."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "schwarz-lib_amd")
DRIVER = os.path.join(PKG, "build", "walk_trim_driver")


@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-C", PKG, "-s", "walk_trim_driver"])  # (nothing to do after build())
    return DRIVER


def run(driver, *args):
    env = dict(os.environ)
    env.pop("SCHWZ_SWEEP_TRIM", None)
    r = subprocess.run([driver, *args], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, "exit %d\n%s" % (r.returncode, r.stderr[-4000:])
    assert not r.stderr.strip(), r.stderr[-4000:]  # a sanitizer report
    return r.stdout.splitlines()


def pieces(lines, case, trim):
    """lengths of the pieces of `case` at `trim`, runs separated by None"""
    hit = [l for l in lines if l.startswith("%s trim %d:" % (case, trim))]
    assert hit, (case, trim)
    m = re.search(r"pieces ([0-9 |]+),", hit[0])
    return [None if t == "|" else int(t) for t in m.group(1).split()]


@pytest.fixture(scope="module")
def lines(driver):
    return run(driver)


def test_every_case_holds_its_invariants(driver, lines):
    cases = run(driver, "--list")
    assert len(cases) >= 10
    for c in cases:
        assert sum(l.startswith(c + " trim ") for l in lines) == 3, c
    print("\n".join(lines))


def test_flagship_tables_lose_positions_where_the_late_round_is(lines):
    # 256 positions: six / eight / twelve pieces per band; the last 256 entries are the last two / four / two pieces
    assert pieces(lines, "cube_update", 0) == [43] * 5 + [41]
    assert pieces(lines, "cube_direction", 0) == [32] * 8
    assert pieces(lines, "cube_first", 0) == [22] * 11 + [14]
    for case, n, late in (("cube_update", 6, 2), ("cube_direction", 8, 4), ("cube_first", 12, 2)):
        p = pieces(lines, case, 300)
        assert len(p) == n and sum(p) == 256
        early, tail = p[:n - late], p[n - late:]
        assert max(early) - min(early) <= 1 and max(tail) - min(tail) <= 1
        # len_late ~ 0.7 len_early, to the rounding of whole positions (one position either way)
        e = 256.0 / (n - late + 0.7 * late)
        assert abs(sum(tail) - 0.7 * e * late) <= 1.0 and abs(sum(early) - e * (n - late)) <= 1.0, (case, p)


def test_slab_second_piece_is_the_late_one(lines):
    assert pieces(lines, "slab_update", 0) == [32, 32]
    p = pieces(lines, "slab_update", 300)
    assert sum(p) == 64 and p[0] > p[1] and abs(p[1] - 0.7 * 64 / 1.7) <= 1.0
    # six workgroups per CU there: pieces of 11 positions, below the threshold
    assert pieces(lines, "slab_first", 300) == pieces(lines, "slab_first", 0)


def test_threshold(lines):
    assert pieces(lines, "below_threshold", 300) == pieces(lines, "below_threshold", 0) == [15] * 6
    assert pieces(lines, "at_threshold", 0) == [16] * 6
    assert pieces(lines, "at_threshold", 300) != [16] * 6


def test_shapes_of_the_gpu_test_move_their_cut_by_two_positions(driver):
    """tests/test_gpu_walk_trim.py: 40 planes, pieces of 20, three CUs, 200 per mille"""
    for case in ("gpu_256x4x40", "gpu_200x9x40", "gpu_200x9x40_direction"):
        assert pieces(run(driver, case, "0"), case, 0) == [20, 20]
        assert pieces(run(driver, case, "200"), case, 200) == [22, 18]


def test_switch_sets_one_or_three_trims(driver):
    """SCHWZ_SWEEP_TRIM as coding_options_from_env reads it: the driver echoes the options with --env"""
    def got(value):
        env = dict(os.environ, SCHWZ_SWEEP_TRIM=value)
        r = subprocess.run([driver, "--env"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
        return [int(t) for t in r.stdout.split()]
    assert got("0") == [0, 0, 0]
    assert got("70") == [70, 70, 70]
    assert got("90,50,200") == [90, 50, 200]
    assert got("90,50") == [90, 50, 0]
