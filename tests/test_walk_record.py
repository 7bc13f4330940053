"""What the z-sweep walk kernels read at entry (plan_walk, csrc/coding_plan.cpp) on the CPU, under the address and
undefined-behaviour sanitizers: tests/drivers/walk_record_driver.cpp plans the codings of 256 x 4 x 12, 200 x 9 x 11, the
middle slab's local matrix of 256 x 4 x 36 cut in three with overlap 2, and a 256 x 4 x 40 cube planned for three CUs with
a trim of 200 per mille, and checks for every slot of the three segment tables that the record repeats the int4 entry
and carries chain_plane[z0 - 1 + k], k = 0 .. 4, -1 included, that empty slots have z0 == z1, and for every pattern and
slot of both ready tables that the value is the table's bit for bit where the mask has the bit and has all 64 bits clear
where it has not.  Here: the driver ends clean on every case, and the lines it prints say that each case met what it
is there for -- segments that begin at a chain end, -1 behind the chain inside the lookahead, empty slots, unequal
segments, absent slots.

(The slab's local matrix has ONE chain: its two appended overlap planes are the chain's ends, 12, 0 .. 11, 13.  The -1
inside the lookahead is the one behind the chain and the entries appended to chain_plane, met by the last segment of two
positions.)"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "schwarz-lib_amd")
DRIVER = os.path.join(PKG, "build", "walk_record_driver")
CASES = ["cube_256x4x12", "cube_200x9x11", "slab_256x4x36_P3_me1", "cube_256x4x40_trimmed"]


@pytest.fixture(scope="module")
def seen():
    subprocess.check_call(["make", "-C", PKG, "-s", "walk_record_driver"])  # (nothing to do after build())
    r = subprocess.run([DRIVER], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, "exit %d\n%s" % (r.returncode, r.stderr[-4000:])
    assert not r.stderr.strip(), r.stderr[-4000:]  # a sanitizer report
    print(r.stdout)
    out = {}
    for line in r.stdout.splitlines():
        name, rest = line.split(":", 1)
        tables = {}
        for part in rest.split(";"):
            words = part.split()
            if not words:
                continue
            nums = {}
            k = 1
            while k < len(words) and words[k] != "lengths":
                nums[words[k]] = int(words[k + 1])
                k += 2
            nums["lengths"] = [int(w) for w in words[k + 1:]]
            tables[words[0]] = nums
        out[name] = tables
    return out


def test_every_case_holds_its_invariants(seen):
    r = subprocess.run([DRIVER, "--list"], stdout=subprocess.PIPE, text=True, check=True)
    assert r.stdout.split() == CASES == list(seen)
    for name in CASES:
        assert set(seen[name]) == {"update", "direction", "first", "ready"}, name
        for table in ("update", "direction", "first"):
            t = seen[name][table]
            assert t["slots"] > t["empty"] and t["slots"] % 8 == 0 and t["minus_first"] > 0, (name, table, t)
        assert seen[name]["ready"]["absent"] > 0 and seen[name]["ready"]["sym_absent"] > 0, name


def test_cases_reach_what_they_are_for(seen):
    # short segments, and empty slots in every table
    assert seen["cube_256x4x12"]["update"]["lengths"] == [4]
    assert all(seen["cube_256x4x12"][t]["empty"] > 0 for t in ("update", "direction", "first"))
    # a last segment of two positions (one per band): its last two plane fields are -1, the last from the appended entries
    slab = seen["slab_256x4x36_P3_me1"]["update"]
    assert slab["lengths"] == [2, 4] and slab["minus_ahead"] == 4 and slab["minus_appended"] == 2
    # 40 positions in two pieces, the late one shorter (tests/test_walk_trim.py: 22 + 18)
    assert seen["cube_256x4x40_trimmed"]["update"]["lengths"] == [18, 22]
    # the boundary patterns of a Laplacian lack slots; the slab's chained overlap planes add patterns
    assert seen["cube_256x4x12"]["ready"]["npat"] == 27 and seen["slab_256x4x36_P3_me1"]["ready"]["npat"] > 27
