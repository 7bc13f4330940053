"""The same RAS run on the GPU whatever form the matrix arrives in: a Matrix-Market file written four ways (general and
shuffled, the lower triangle of a symmetric file, every off-diagonal value as two halves, the symmetric form with CRLF
line ends and comments) and caller arrays that hold a column twice give the iteration count, both residual histories
and the solution of initialize(matrix=(rp, col, val)) on the plain arrays, bit for bit.  Halving and adding the halves
back is exact, so every form describes the same matrix in the same bits; what differs is only what the ingest has to
sort, mirror and sum.  All files are written into tmp_path."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
P = 3


def _is_symmetric_and_free_of_duplicates(rp, col, val):
    n = len(rp) - 1
    entries = {}
    for i in range(n):
        row = col[rp[i]:rp[i + 1]]
        if np.any(np.diff(row) <= 0):
            return False
        for j, v in zip(row, val[rp[i]:rp[i + 1]]):
            entries[(i, int(j))] = float(v)
    return all(entries.get((j, i)) == v for (i, j), v in entries.items())


@pytest.fixture(scope="module")
def matrix(schwz):
    """tests/golden/ani3_crop.npz if it is symmetric bit for bit, else the 7-point Laplacian on 12 x 12 x 12 (the
    matrix of lap3d_12x12x12.npz): the symmetric file forms hold one triangle only."""
    g = np.load(os.path.join(G, "ani3_crop.npz"))
    rp, col, val = g["rp"].astype(np.int64), g["col"].astype(np.int32), g["val"].astype(np.float64)
    if not _is_symmetric_and_free_of_duplicates(rp, col, val):
        rp, col, val = schwz.Problem.laplacian(3, 12, 12, 12).to_csr()
        assert len(rp) - 1 == len(np.load(os.path.join(G, "lap3d_12x12x12.npz"))["x_ones"])
    assert _is_symmetric_and_free_of_duplicates(rp, col, val)
    assert np.all(val / 2 + val / 2 == val)  # the halves add back exactly
    return rp, col, val


def _run(schwz, matrix=None, path=None):
    s = schwz.Settings(overlap=2) if path is None else \
        schwz.Settings(overlap=2, matrix_filename=str(path), explicit_laplacian=False)
    m = schwz.Metadata(num_subdomains=P, local_precond="block-jacobi", precond_max_block_size=1,
                       local_solver_tolerance=0.0, local_max_iters=10, max_iters=8, tolerance=1e-14)
    solver = schwz.SolverRAS(s, m, comm=schwz.InProcessComm(P), quiet=True)
    solver.initialize(matrix=matrix)
    out = solver.run()
    ppd = m.post_process_data
    return (out["iter_count"], np.array(ppd["global_residual_vector_out"]), np.array(ppd["local_residual_vector_out"]),
            out["solution"].copy())


@pytest.fixture(scope="module")
def reference(schwz, torch_cuda, matrix):
    ref = _run(schwz, matrix=matrix)
    assert ref[0] == 8 and ref[1].size and ref[2].size and np.all(np.isfinite(ref[3])) and np.any(ref[3] != 0.0)
    return ref


def _same(run, ref):
    assert run[0] == ref[0]
    for a, b in zip(run[1:], ref[1:]):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()


def _entries(matrix, lower_only=False):
    rp, col, val = matrix
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    return [(int(r) + 1, int(c) + 1, float(v)) for r, c, v in zip(rows, col, val) if not lower_only or c <= r]


def _write(path, symmetry, n, entries, eol="\n", comments=()):
    lines = ["%%MatrixMarket matrix coordinate real " + symmetry] + list(comments) + ["%d %d %d" % (n, n, len(entries))]
    lines += ["%d %d %.17g" % e for e in entries]
    path.write_bytes((eol.join(lines) + eol).encode())
    return path


@pytest.mark.parametrize("form", ["general_shuffled", "symmetric_lower_triangle", "general_off_diagonal_in_two_halves",
                                  "symmetric_crlf_with_comments"])
def test_a_run_from_a_file_equals_the_run_from_the_arrays(schwz, torch_cuda, tmp_path, matrix, reference, form):
    n = len(matrix[0]) - 1
    if form == "general_shuffled":
        e = _entries(matrix)
        e = [e[k] for k in np.random.default_rng(1).permutation(len(e))]
        path = _write(tmp_path / "m.mtx", "general", n, e)
    elif form == "symmetric_lower_triangle":
        path = _write(tmp_path / "m.mtx", "symmetric", n, _entries(matrix, lower_only=True))
    elif form == "general_off_diagonal_in_two_halves":
        e = []
        for r, c, v in _entries(matrix):
            e += [(r, c, v)] if r == c else [(r, c, v / 2), (r, c, v / 2)]
        path = _write(tmp_path / "m.mtx", "general", n, e)
    else:
        path = _write(tmp_path / "m.mtx", "symmetric", n, _entries(matrix, lower_only=True), eol="\r\n",
                      comments=("% written by the test", "%", ""))
    _same(_run(schwz, path=path), reference)


@pytest.mark.parametrize("split", ["off_diagonal", "every_entry"])
def test_a_run_from_arrays_that_hold_a_column_twice_equals_the_run_from_the_arrays(schwz, torch_cuda, matrix, reference,
                                                                                  split):
    """initialize(matrix=...) on CSR arrays in which every off-diagonal value v -- and, for "every_entry", the
    diagonal too -- is stored as the two entries v / 2, v / 2.  Both cases fail on the commit before the ingest summed
    duplicates (so does the file form with the halves, and the CRLF form was refused): the arrays went to the subdomains
    as they were; with "every_entry" the Jacobi diagonal was the LAST stored entry of column i in row i, half the
    diagonal, while SpMV summed both, so the preconditioner belonged to another matrix than the operator; with
    "off_diagonal" the local matrices were other, longer arrays.  Either way the residual histories left the
    reference's bits within the first three iterations."""
    rp, col, val = matrix
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    twice = (rows != col) | (split == "every_entry")
    reps = np.where(twice, 2, 1)
    col2 = np.repeat(col, reps)
    val2 = np.repeat(np.where(twice, val / 2, val), reps)
    rp2 = np.zeros(len(rp), dtype=np.int64)
    np.add.at(rp2, rows + 1, reps)
    rp2 = np.cumsum(rp2)
    assert rp2[-1] == len(col2) > len(col)
    _same(_run(schwz, matrix=(rp2, col2.astype(np.int32), val2)), reference)
