#!/usr/bin/env python3
"""Digests of what the three kernels of the plain-CSR tile pipeline (csrc/stream_pipeline.hpp: spmv_stream_kernel,
cheb_stream_kernel, f32_spmv_stream_kernel) compute, case by case: sha256 of the result arrays' bytes.  The
arithmetic is in a fixed order with contraction off, so a refactor of the pipeline must reproduce them bit for bit.

Recorded once with the library of the commit before the pipeline was written once (SCHWZ_HIP_LIB pointing at a
build of that commit):

    SCHWZ_HIP_LIB=<parent build>/libschwz_hip.so python tests/golden/make_stream_pipeline_digests.py \
        --commit <parent hash> > tests/golden/stream_pipeline_digests.json

tests/test_gpu_stream_pipeline.py recomputes them with the library under test."""
import argparse
import hashlib
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CODINGS_OFF = ("SCHWZ_SPMV_PAIR", "SCHWZ_SPMV_PATTERN", "SCHWZ_SPMV_DICT")
K_TILE_ROWS, K_TILE_NNZ, K_XCDS = 256, 2048, 8   # csrc/schwz_internal.hpp


def _csr(a):
    a = a.tocsr()
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(np.float64)


def tridiagonal(n):
    import scipy.sparse as sp
    return _csr(sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n)) if n > 1 else sp.csr_matrix(np.array([[2.0]])))


def laplacian2d(n):
    import scipy.sparse as sp
    t = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n), format="csr")
    eye = sp.identity(n, format="csr")
    return _csr(sp.kron(eye, t) + sp.kron(t, eye))


def wrapping_band(n=256, half=15):
    """2 half + 1 entries per row, columns wrapping round: tiles limited by their nonzeros, most lanes past the last row"""
    rp = np.arange(n + 1, dtype=np.int32) * (2 * half + 1)
    col = np.empty(rp[-1], dtype=np.int32)
    val = np.empty(rp[-1])
    for i in range(n):
        c = np.sort((i + np.arange(-half, half + 1)) % n)
        col[rp[i]:rp[i + 1]] = c
        val[rp[i]:rp[i + 1]] = np.where(c == i, 2.0 * half + 2.0, -1.0)
    return rp, col, val


def ragged(n, max_len, seed, empty_rows=True):
    """Ragged rows, a tenth of them empty (unless empty_rows is False); every other row holds its diagonal, which
    dominates the row and differs from row to row"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, max_len + 1, size=n)
    if empty_rows:
        lens[rng.integers(0, n, size=n // 10)] = 0
    lens[n // 3] = max_len
    rp = np.zeros(n + 1, dtype=np.int32)
    rp[1:] = np.cumsum(lens)
    col = np.zeros(rp[-1], dtype=np.int32)
    val = rng.standard_normal(rp[-1])
    for i in range(n):
        if lens[i] == 0:
            continue
        c = rng.choice(n, size=lens[i], replace=False)
        if i not in c:
            c[0] = i
        c = np.sort(c)
        col[rp[i]:rp[i + 1]] = c
        v = val[rp[i]:rp[i + 1]]
        v[c == i] = np.abs(v).sum() + 1.0
    return rp, col, val


RAGGED = [("ragged_%d_len%d" % (n, m), n, m) for m in (8, 16, 32) for n in (7001, 9001)]


def cases():
    """(name, builder) in a fixed order"""
    out = [("tridiagonal_%d" % n, (lambda n=n: tridiagonal(n))) for n in (1, 255, 256, 257, 513)]
    out += [(name, (lambda n=n, m=m: ragged(n, m, 1000 * m + n))) for name, n, m in RAGGED]
    out += [("wrapping_band_256x31", wrapping_band), ("laplacian2d_1280", lambda: laplacian2d(1280))]
    # no empty rows, a diagonal that varies: the one ragged matrix Jacobi takes (Chebyshev refuses a missing diagonal),
    # so that the dinv operand and its select are in the digests with values that matter, at CAP = 16
    out += [("ragged_full_5003_len16", lambda: ragged(5003, 16, 77, empty_rows=False))]
    return out


def workgroup_tile_counts(rp, col, seq=3):
    """Tiles per short-lived workgroup of `seq` slots, from the tiling and the block-cyclic deal of schwz_csr_create
    (csrc/kernels.hip) repeated here: the set of counts > 0 that occur.  The library does not report its tile count or
    the run length of its deal, so nothing ties this copy to it: if the tiling or the deal in kernels.hip changes, this
    function must change with it, or the claim it supports goes stale while its assertion still passes."""
    n = len(rp) - 1
    tiles, r = [0], 0
    while r < n:
        e = r
        while e < n and e - r < K_TILE_ROWS and rp[e + 1] - rp[r] <= K_TILE_NNZ - 2:
            e += 1
        e = max(e, r + 1)
        tiles.append(e)
        r = e
    ntl = len(tiles) - 1
    step = n // 4096 if n > 4096 else 1
    bws = sorted(max(i - col[rp[i]], col[rp[i + 1] - 1] - i) for i in range(0, n, step) if rp[i + 1] > rp[i])
    bw = max(0, int(bws[len(bws) // 2])) if bws else 0
    b = max(1, min(bw // max(1, n // max(1, ntl)) // K_XCDS, (ntl + K_XCDS - 1) // K_XCDS))
    sh = 0
    while (2 << sh) <= b:
        sh += 1
    nslots = ((ntl + (K_XCDS << sh) - 1) >> (sh + 3)) << sh
    counts = set()
    for xcd in range(K_XCDS):
        for w in range((nslots + seq - 1) // seq):
            js = range(w * seq, min((w + 1) * seq, nslots))
            counts.add(sum(((j >> sh) << (sh + 3)) + (xcd << sh) + (j & ((1 << sh) - 1)) < ntl for j in js))
    return ntl, counts - {0}


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def _num(v):
    return struct.pack("<d", float(v)).hex()


def case_digests(schwz, torch, rp, col, val):
    """{what: digest} of one matrix with the library `schwz` has loaded; codings off, so every product is plain CSR"""
    saved = {k: os.environ.get(k) for k in CODINGS_OFF}
    os.environ.update({k: "0" for k in CODINGS_OFF})
    try:
        return _case_digests(schwz, torch, rp, col, val)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _case_digests(schwz, torch, rp, col, val):
    c = schwz.capi
    n = len(rp) - 1
    rng = np.random.default_rng(n)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    x0, b = dev(rng.standard_normal(n)), dev(rng.standard_normal(n))
    out = {}

    def attempt(key, fn):
        # a solver that refuses the matrix (a missing diagonal under Jacobi) must refuse it before and after
        try:
            out.update(fn())
        except schwz.SchwzError as e:
            out[key] = "refused: %d" % e.code

    A = schwz.Csr(rp, col, val)
    assert A.format() == 0
    y = torch.zeros(n, dtype=torch.float64, device="cuda")
    A.spmv(x0.data_ptr(), y.data_ptr(), 1.0, 0.0, variant=6)
    torch.cuda.synchronize()
    out["spmv6.y"] = _sha(y)

    def pcg(precond):
        def run():
            x = x0.clone()
            it, rn = schwz.Pcg(A, precond).solve(b.data_ptr(), x.data_ptr(), 0.0, 5)
            return {"pcg%d.x" % precond: _sha(x), "pcg%d.norm" % precond: _num(rn), "pcg%d.iters" % precond: str(it)}
        return run

    def cheb(precond, rtol, iters, tag):
        def run():
            x = x0.clone()
            it, rn = schwz.Chebyshev(A, precond).solve(b.data_ptr(), x.data_ptr(), rtol, iters)
            key = "cheb%d.%s" % (precond, tag)
            return {key + ".x": _sha(x), key + ".norm": _num(rn), key + ".iters": str(it)}
        return run

    def f32(precond):
        def run():
            s = schwz.PcgF32(A, precond)
            p = dev(rng.standard_normal(n).astype(np.float32))
            q = torch.zeros(n, dtype=torch.float32, device="cuda")
            pq = s.spmv(p.data_ptr(), q.data_ptr())
            torch.cuda.synchronize()
            x = x0.clone()
            it, rn = s.solve(b.data_ptr(), x.data_ptr(), 0.0, 3)
            key = "f32_%d" % precond
            return {key + ".q": _sha(q[:n]), key + ".pq": _num(pq), key + ".x": _sha(x), key + ".norm": _num(rn)}
        return run

    def resid():
        prob = schwz.Problem.from_csr(rp, col, val)
        sd = schwz.Subdomain(prob, 1, 0, 2, schwz.partition_regular(prob.N, 1))
        sd.to_device(b.cpu().numpy(), spmv_variant=6)
        px, cnt = sd.vector(0)
        assert cnt >= n
        idx = torch.arange(n, dtype=torch.int32, device="cuda")
        schwz.scatter(n, idx.data_ptr(), x0.data_ptr(), px)
        torch.cuda.synchronize()
        return {"residnorm": _num(sd.local_residual())}

    for precond in (c.PRECOND_NONE, c.PRECOND_JACOBI):
        attempt("pcg%d" % precond, pcg(precond))
        attempt("cheb%d.fixed3" % precond, cheb(precond, 0.0, 3, "fixed3"))
        attempt("f32_%d" % precond, f32(precond))
    attempt("cheb0.tol", cheb(c.PRECOND_NONE, 0.5, 40, "tol"))
    attempt("residnorm", resid)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose library is loaded")
    ap.add_argument("--only", default="", help="cases whose name contains this")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "schwarz-lib_amd"))
    import torch
    import schwz_amd
    torch.cuda.set_device(0)
    print("library:", schwz_amd.capi.LIB_PATH, file=sys.stderr, flush=True)
    rec = {"commit": args.commit, "cases": {}}
    for name, build in cases():
        if args.only in name:
            rec["cases"][name] = case_digests(schwz_amd, torch, *build())
            print(name, len(rec["cases"][name]), file=sys.stderr, flush=True)
    json.dump(rec, sys.stdout, indent=1, sort_keys=True)
    print()
    return 0


if __name__ == "__main__":
    sys.exit(main())
