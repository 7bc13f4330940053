"""Same bits as before the plain-CSR tile pipeline was written once (csrc/stream_pipeline.hpp).  The three kernels
that share it sum every row in CSR order with contraction off, so what they compute is fixed bit for bit:
tests/golden/stream_pipeline_digests.json holds the sha256 of every result of tests/golden/
make_stream_pipeline_digests.py, recorded with the library of the commit named in the file (each kernel still had
its own copy of the pipeline), and the library under test must reproduce them.

Cases: tridiagonal matrices of a single tile and on both sides of the tile edge; ragged rows with empty ones for every
masked-add count (8 / 16 / 32), and one without empty rows whose diagonal varies, which Jacobi Chebyshev takes; a
wrapping band whose tiles are limited by their nonzeros (most lanes past the last row); laplacian2d(1280), 6400 tiles: past 6144, where Chebyshev's workgroups take more than three tiles and the fp32
kernel runs its persistent form.  Per case: y = A x (variant 6), the stored-q CG (start residual, q = A p with p.q),
a local residual norm, Chebyshev with fixed work and with a tolerance (the NORM forms), the fp32 product and solve."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RECORD = json.load(open(os.path.join(GOLDEN_DIR, "stream_pipeline_digests.json")))
_spec = importlib.util.spec_from_file_location("make_stream_pipeline_digests",
                                               os.path.join(GOLDEN_DIR, "make_stream_pipeline_digests.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)
CASES = dict(maker.cases())


def test_the_record_covers_every_case():
    assert sorted(RECORD["cases"]) == sorted(CASES) and len(RECORD["commit"]) == 40
    for name, rec in RECORD["cases"].items():
        assert len(rec) >= 20, name
        # only Jacobi Chebyshev is refused, and only where empty rows leave the diagonal incomplete
        refused = [k for k, v in rec.items() if v.startswith("refused")]
        assert refused == (["cheb1.fixed3"] if name in [r[0] for r in maker.RAGGED] else []), (name, refused)


def test_short_lived_workgroups_of_one_two_and_three_tiles_occur():
    """The driver loop of the pipeline goes through its tiles in pairs, with an odd tail: workgroups of one tile (tail
    alone), two (a pair) and three (a pair and the tail) all occur among the ragged cases, in the kernels that take
    three consecutive slots per workgroup (Chebyshev, fp32).  From the tile counts of a Python copy of the library's
    tiling and deal (maker.workgroup_tile_counts), without a GPU run: the library reports neither, so the copy can drift
    from csrc/kernels.hip and has to be kept in step by hand."""
    seen = set()
    for name, n, max_len in maker.RAGGED:
        rp, col, _ = CASES[name]()
        assert int((rp[1:] - rp[:-1]).max()) == max_len
        ntiles, counts = maker.workgroup_tile_counts(rp, col)
        print(name, ntiles, sorted(counts))
        seen |= counts
    assert seen == {1, 2, 3}


@pytest.mark.parametrize("name", list(CASES))
def test_same_bits_as_the_recorded_commit(schwz, torch_cuda, name):
    got = maker.case_digests(schwz, torch_cuda, *CASES[name]())
    want = RECORD["cases"][name]
    diff = {k: (want.get(k), got.get(k)) for k in sorted(set(want) | set(got)) if want.get(k) != got.get(k)}
    assert not diff, "%s differs from commit %s: %s" % (name, RECORD["commit"][:12], diff)
