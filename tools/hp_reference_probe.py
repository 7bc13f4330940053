"""How far the kernels are from the extended-precision references of tests/hp_reference.py, case by case: the
numbers behind DESIGN.md "Extended-precision references" (profiles/r06_hp_reference.txt, r08_cg_reference.txt).

  python tools/hp_reference_probe.py [out.txt] [--cg]

Runs tests/test_gpu_gmres.py and tests/test_gpu_trs.py -- with --cg: tests/test_gpu_cg.py instead -- in this
process (one GPU) and prints what their comparisons recorded: for GMRES and CG the distance of the device iterate
and residual norm from the longdouble reference in units of dev (the distance of the float64 run of the same
reference text, floored at iters * 2^-52; the tests allow 32), for the triangular solves the largest componentwise
error in units of the derived bound (the tests allow 2); for CG also the flavour of every solve, the separation
the reference gave every tolerance stop, the free HBM the large cases saw and the wall time of the module.  The
suite times and the seeded-defect tables at the end of the profile files are written by hand.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")


def cg_report(out, extra):
    """The CG module alone (it takes minutes); `extra`: further pytest arguments (-k ...)."""
    import time
    import pytest
    t0 = time.time()
    rc = pytest.main(["-q", "-p", "no:cacheprovider", "--durations=15", os.path.join(TESTS, "test_gpu_cg.py")] + extra)
    cg_write(out, int(rc), time.time() - t0)
    return int(rc)


def cg_write(out, rc, wall):
    """What a run of tests/test_gpu_cg.py in this process recorded."""
    cg = sys.modules["test_gpu_cg"]
    w = out.write
    w("CG against the extended-precision reference hp.pcg (tools/hp_reference_probe.py --cg, one MI355X).\n")
    w("pytest exit status of tests/test_gpu_cg.py: %d, wall time %.0f s\n" % (int(rc), wall))
    for note in cg.NOTES:
        w("  %s\n" % note)
    w("\n|x_gpu - x_ld|_inf / |x_ld|_inf and |resn_gpu - resn_ld| / resn_ld in units of dev = max(|f64 - ld|, floor),\n")
    w("floor = iters * 2^-52; limit %g.  (r / dev -1: not compared, see the test)\n" % cg.MARGIN)
    w("  %-44s %9s %5s %4s  %9s  %9s  %8s  %9s  %8s\n" %
      ("case", "rows", "iters", "flav", "f64-ld x", "floor", "x / dev", "dev resn", "r / dev"))
    for tag, n, iters, fl, dx, floor, rx, dr, rr, raw in cg.RATIOS:
        w("  %-44s %9d %5d %4d  %9.2e  %9.2e  %8.2f  %9.2e  %8.2f\n" % (tag, n, iters, fl, raw, floor, rx, dr, rr))
    if cg.RATIOS:
        w("  largest: x %.2f dev, resn %.2f dev; flavours seen: %s\n" %
          (max(r[6] for r in cg.RATIOS), max(r[8] for r in cg.RATIOS), sorted({r[3] for r in cg.RATIOS})))
    w("\nTolerance stops: rtol from the longdouble history; the device stopped at the same update in every case\n")
    w("  %-28s %5s  %10s  %14s  %16s\n" % ("case", "stop", "rtol", "red(stop)/rtol", "red(before)/rtol"))
    for tag, t, rtol, at, before in cg.SEPARATION:
        w("  %-28s %5d  %10.3e  %14.6f  %16.6f\n" % (tag, t, rtol, at, before))


def main():
    import pytest
    args = [a for a in sys.argv[1:] if not a.startswith("-")]
    out = open(args[0], "w") if args else sys.stdout
    if "--cg" in sys.argv[1:]:
        sys.path.insert(0, TESTS)
        rc = cg_report(out, [a for a in sys.argv[1:] if a.startswith("-k") or a.startswith("--deselect")])
        if out is not sys.stdout:
            out.close()
        return rc
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
