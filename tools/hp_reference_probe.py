"""How far the kernels are from the extended-precision references of tests/hp_reference.py, case by case: the
numbers behind DESIGN.md "Extended-precision references" (profiles/r06_hp_reference.txt).

  python tools/hp_reference_probe.py [out.txt]

Runs tests/test_gpu_gmres.py and tests/test_gpu_trs.py in this process (one GPU) and prints what their
comparisons recorded: for GMRES the distance of the device iterate and residual norm from the longdouble
reference in units of dev (the distance of the float64 run of the same reference text, floored at
iters * 2^-52; the tests allow 32), for the triangular solves the largest componentwise error in units of the
derived bound (the tests allow 2).  The suite times and the sensitivity spot check at the end of the profile
file are written by hand.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")


def main():
    import pytest
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    rc = pytest.main(["-q", "-p", "no:cacheprovider", os.path.join(TESTS, "test_gpu_gmres.py"),
                      os.path.join(TESTS, "test_gpu_trs.py")])
    gm, tr = sys.modules["test_gpu_gmres"], sys.modules["test_gpu_trs"]
    w = out.write
    w("Kernels against the extended-precision references (tools/hp_reference_probe.py, one MI355X).\n")
    w("pytest exit status of the two modules: %d\n\n" % int(rc))
    w("GMRES: |x_gpu - x_ld|_inf and |resn_gpu - resn_ld| in units of dev = max(|f64 - ld|, iters * 2^-52); limit 32\n")
    w("  (f64-ld x: the unfloored distance of the float64 reference run, relative to |x_ld|_inf)\n")
    w("  %-36s %5s  %9s  %9s  %8s  %9s  %8s\n" % ("case", "iters", "f64-ld x", "dev x", "x / dev", "dev resn", "r / dev"))
    for tag, iters, rx, rr, dx, dr, raw in gm.RATIOS:
        w("  %-36s %5d  %9.2e  %9.2e  %8.2f  %9.2e  %8.2f\n" % (tag, iters, raw, dx, rx, dr, rr))
    if gm.RATIOS:
        w("  largest: x %.2f dev, resn %.2f dev\n" % (max(r[2] for r in gm.RATIOS), max(r[3] for r in gm.RATIOS)))
    w("\nTriangular solves: max_i |y_gpu - y_ld|_i / bound_i (bound: Higham Thm 8.5, any summation order); limit 2\n")
    w("  %-52s %8s\n" % ("case", "err/bound"))
    for tag, worst in tr.RATIOS:
        w("  %-52s %8.3f\n" % (tag, worst))
    if tr.RATIOS:
        w("  largest: %.3f\n" % max(r[1] for r in tr.RATIOS))
    if out is not sys.stdout:
        out.close()
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
