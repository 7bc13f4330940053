"""The compiled form of the fp32-basis passes of the outer FGMRES (csrc/outer.hip, outer_dots_f32_kernel and
outer_sub_f32_kernel) is part of their contract: a lane holds up to 32 columns (128 VGPRs) beside 64 VGPRs of
accumulators, and a register set kept in scratch memory would multiply the bytes the pass moves.
tools/kernel_resources.py compiles outer.hip once (device only, nothing runs); every instantiation of the new kernels
must have no scratch and an occupancy not below that of the fp64 kernel with the same number of register blocks -- the
fp64 kernels are the parent's code, read in the same call.  Only the compiler's resource remarks are read."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_resources import kernel_resources  # noqa: E402

F32 = ["outer_dots_f32_kernel<%d>" % nb for nb in (1, 2, 3, 4)] + \
      ["outer_sub_f32_kernel<%d, %s>" % (nb, d) for nb in (1, 2, 3, 4) for d in ("true", "false")]
OTHER = ["outer_scale_f32_kernel", "outer_widen_kernel", "outer_narrow_kernel", "outer_residual_kernel<true>",
         "outer_residual_kernel<false>"]


@pytest.fixture(scope="module")
def table():
    got = kernel_resources(os.path.join(ROOT, "schwarz-lib_amd", "csrc", "outer.hip"), "outer_")
    return {re.sub(r"^schwz::", "", k): v for k, v in got.items()}


def test_every_new_kernel_is_there(table):
    assert set(F32 + OTHER) <= set(table), sorted(set(F32 + OTHER) - set(table))
    assert [k for k in table if "_f32_kernel" in k and k not in F32 + OTHER] == []


@pytest.mark.parametrize("name", F32 + OTHER)
def test_no_scratch(table, name):
    assert table[name]["scratch"] == 0, table[name]


@pytest.mark.parametrize("name", F32)
def test_occupancy_not_below_the_fp64_kernel(table, name):
    g, p = table[name], table[name.replace("_f32_kernel", "_kernel")]
    print("%-36s VGPRs %3d (fp64 %3d)  SGPRs %3d (%3d)  occupancy %d (%d)  LDS %d (%d)" % (
        name, g["vgprs"] + g["agprs"], p["vgprs"] + p["agprs"], g["sgprs"], p["sgprs"], g["occupancy"], p["occupancy"],
        g["lds"], p["lds"]))
    assert p["scratch"] == 0
    assert g["occupancy"] >= p["occupancy"], (g, p)
    assert g["lds"] == p["lds"]
