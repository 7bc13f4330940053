"""The plans of the matrix codings (csrc/coding_plan.cpp) on the CPU, under the address and undefined-behaviour
sanitizers: tests/drivers/coding_plan_driver.cpp plans one case, checks that the pair coding is lossless and that
every segment table covers every row exactly once, and prints a digest of every array and every scalar an upload
would send.  The digests must equal tests/golden/coding_plan_parent.json -- recorded once, on an MI355X (256 CUs),
from the uploads of the commit BEFORE the plans were split from the uploads (its upload helpers printing the same
lines): the refactor must plan what that commit planned, array for array."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "schwarz-lib_amd")
DRIVER = os.path.join(PKG, "build", "coding_plan_driver")
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "coding_plan_parent.json")))
NO_RECORD = ["default_128x128x64_cus64"]  # another device's CU count: invariants and sanitizers only


@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-C", PKG, "-s", "coding_plan_driver"])  # (nothing to do after build())
    return DRIVER


def plan_lines(driver, case, threads=None):
    env = dict(os.environ)
    env.pop("SCHWZ_SETUP_THREADS", None)
    if threads:
        env["SCHWZ_SETUP_THREADS"] = str(threads)
    r = subprocess.run([driver, case], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, "%s: exit %d\n%s" % (case, r.returncode, r.stderr[-4000:])
    assert not r.stderr.strip(), r.stderr[-4000:]  # a sanitizer report
    return sorted(r.stdout.splitlines())


def test_case_lists_agree(driver):
    listed = subprocess.run([driver, "--list"], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    assert sorted(listed) == sorted(list(GOLDEN) + NO_RECORD)


@pytest.mark.parametrize("case", sorted(GOLDEN))
def test_plan_equals_the_parent_commit(driver, case):
    got, want = plan_lines(driver, case), GOLDEN[case]
    assert len(want) >= 40, "record of %s is incomplete" % case
    diff = sorted(set(got) ^ set(want))
    assert not diff, "%s: lines that differ from the parent commit's upload:\n%s" % (case, "\n".join(diff))


@pytest.mark.parametrize("case", NO_RECORD)
def test_invariants_with_another_cu_count(driver, case):
    lines = plan_lines(driver, case)
    assert "scalar bound_sweep_seg 1" in lines
    # fewer CUs, longer segments: not the 256-CU plan
    assert [l for l in lines if l.startswith("array sweep_seg ")] != [l for l in GOLDEN["default_128x128x64"] if l.startswith("array sweep_seg ")]


def test_plan_does_not_depend_on_the_thread_count(driver):
    one, eight = plan_lines(driver, "default_128x128x64", 1), plan_lines(driver, "default_128x128x64", 8)
    assert one == eight
    assert not set(one) ^ set(GOLDEN["default_128x128x64"])
