"""schwz_csr_spmv (y = alpha A x + beta y) row by row against the longdouble row sums of hp_reference.py, at the
derived bound hp.axpby_bound -- gamma(k_i + 2) (|alpha| sum_j |a_ij x_j| + |beta| |y0_i|) per row, valid for any
order of a row's additions, nothing in it measured on a kernel -- on matrices built to reach every tile branch of
spmv_tiled2_kernel (aligned window, unaligned staging, one long row reduced by the workgroup), the three masked-add
forms of the stream kernel, rectangular shapes, badly scaled rows (a tolerance relative to max |y| is blind to a
wrong term in a small row; CPU pin: test_hp_reference.py) and the coded forms (row pairs, row patterns, per-entry
dictionaries).  Each matrix asserts through a restatement of the tile rule of schwz_csr_create that the branch it
is built for occurs.

Per matrix and (alpha, beta): every variant of the product library meets the bound; all variants return the same
bits (variant 9, the tiled kernel, is the anchor); with beta = 0 a y prefilled with NaN comes back
finite with the bits of the run from y = 0 (y is not read).

SCHWZ_SPMV_STREAM is read once per process and not toggled: variant 6 against variant 9 separates the stream kernel
from the tiled one wherever hp.stream_cap says the stream kernel applies."""
import numpy as np
import pytest

import cg_child as cc
import hp_reference as hp

pytestmark = pytest.mark.gpu

VARIANTS = (0, 6, 7, 8, 9)
PATTERN = {"SCHWZ_SPMV_PAIR": "0", "SCHWZ_SPMV_PATTERN": "2"}

# case id -> (matrix of hp.rowsum_case, switches at upload, schwz_csr_format)
CASES = {name: (name, cc.PLAIN, 0) for name in hp.ROWSUM_CASES if name not in ("lap3d", "lap2d", "ani4_crop")}
CASES.update({
    "lap3d_pairs": ("lap3d", cc.PAIRS, 3),
    "lap2d_patterns": ("lap2d", PATTERN, 2),
    "lap2d_dictionary": ("lap2d", cc.DICT, 1),
    "ani4_crop_patterns": ("ani4_crop", PATTERN, 2),
    "ani4_crop_dictionary": ("ani4_crop", cc.DICT, 1),
})

_refs = {}


def reference(name):
    """The case with its longdouble results and bounds per (alpha, beta): computed once, never written to."""
    if name not in _refs:
        hp.require_extended_precision()
        c = hp.rowsum_case(name)
        a = (c["rp"], c["col"], c["val"], c["x"])
        c["ref"] = {ab: hp.axpby(*a, ab[0], ab[1], c["y0"]) for ab in hp.ALPHA_BETA}
        c["bound"] = {ab: hp.axpby_bound(*a, ab[0], ab[1], c["y0"]) for ab in hp.ALPHA_BETA}
        for v in list(c["ref"].values()) + list(c["bound"].values()):
            v.setflags(write=False)
        _refs[name] = c
    return _refs[name]


def worst_row(got, ref, bound):
    """(largest error / bound, its row); a row with a zero bound (an empty row, beta = 0) must be exact."""
    err = np.abs(got.astype(hp.LD) - ref)
    zero = bound == 0
    assert (err[zero] == 0).all(), "rows with a zero bound: %s" % np.nonzero(zero & (err != 0))[0][:8]
    q = np.zeros(len(err), dtype=hp.LD)
    q[~zero] = err[~zero] / bound[~zero]
    i = int(np.argmax(q)) if len(q) else 0
    return float(q[i]) if len(q) else 0.0, i


@pytest.mark.parametrize("case", sorted(CASES))
def test_spmv_meets_the_row_wise_bound_and_all_variants_agree(schwz, torch_cuda, case):
    torch = torch_cuda
    name, env, fmt = CASES[case]
    c = reference(name)
    rp, n = c["rp"], len(c["rp"]) - 1
    branches = hp.tile_branches(rp)
    assert c["branches"] <= set(branches), (case, sorted(set(branches)))
    if name.startswith("scaled"):
        assert hp.stream_cap(rp) == int(name[6:])        # variants 0 / 6 run the stream kernel, 9 the tiled one
    with cc.upload_env(env):
        A = schwz.Csr(rp, c["col"], c["val"], ncols=c["ncols"])
    assert A.format() == fmt, (case, A.format())
    d_x = torch.from_numpy(c["x"]).cuda()
    worst = (-1.0, None)
    for ab in hp.ALPHA_BETA:
        alpha, beta = ab
        ys = {}
        for variant in VARIANTS:
            d_y = torch.from_numpy(c["y0"]).cuda()
            A.spmv(d_x.data_ptr(), d_y.data_ptr(), alpha, beta, variant=variant)
            torch.cuda.synchronize()
            ys[variant] = d_y.cpu().numpy()
            q, row = worst_row(ys[variant], c["ref"][ab], c["bound"][ab])
            assert q <= 1.0, ("%s variant %d alpha %g beta %g: row %d (%d entries, tile branch %s) is %.3g times its "
                              "bound off: got %r, reference %r" %
                              (case, variant, alpha, beta, row, rp[row + 1] - rp[row],
                               branches[int(np.searchsorted(hp.tiles_of(rp), row, side="right")) - 1], q,
                               ys[variant][row], c["ref"][ab][row]))
            if q > worst[0]:
                worst = (q, (variant, ab, row))
        for variant in VARIANTS:
            same = ys[variant].view(np.int64) == ys[9].view(np.int64)
            assert same.all(), ("%s alpha %g beta %g: variant %d differs from variant 9 in rows %s" %
                                (case, alpha, beta, variant, np.nonzero(~same)[0][:8]))
        if beta == 0.0:
            for variant in VARIANTS:
                d_y = torch.full((max(n, 1),), float("nan"), dtype=torch.float64, device="cuda")
                A.spmv(d_x.data_ptr(), d_y.data_ptr(), alpha, beta, variant=variant)
                d_z = torch.zeros(max(n, 1), dtype=torch.float64, device="cuda")
                A.spmv(d_x.data_ptr(), d_z.data_ptr(), alpha, beta, variant=variant)
                torch.cuda.synchronize()
                y, z = d_y.cpu().numpy()[:n], d_z.cpu().numpy()[:n]
                assert np.isfinite(y).all(), (case, variant, "y was read although beta == 0")
                assert np.array_equal(y.view(np.int64), z.view(np.int64)), (case, variant)
    print("\nrowsum %-22s n %5d nnz %6d branches %s stream_cap %2d: max error / bound %.3f (variant, (alpha, beta), row) %s"
          % (case, n, rp[-1], "".join(sorted(set(branches))), hp.stream_cap(rp), worst[0], worst[1]))
