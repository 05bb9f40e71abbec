"""MINRES against cg (as it runs by default) and cg(posdef=False) on Hermitian indefinite systems, one process.

Writes profiles/minres.json: per case and method the iterations, operator applies, ms per solve and ms per
iteration, the true relative residual and whether the run converged.  Systems:
  banded   the `c3` banded shape (DIA band, half bandwidth --hb) symmetrised, diagonal of alternating sign
  dense    a batch of dense Hermitian operators shifted into their spectrum
  laplace  the 7-point Laplacian of an m^3 grid shifted between two of its eigenvalues
The kernel shares (step kernels against the operator apply) come from a separate run of this script under
`rocprofv3 --kernel-trace --stats -- python scripts/minres_bench.py --case ... --method minres --no-json`.

    python scripts/minres_bench.py [--case banded --case dense --case laplace] [--rtol 1e-8] [--reps 3]
"""
import argparse
import json
import math
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import xitorch_amd as xa  # noqa: E402
from xitorch_amd.linalg import native_krylov as nk  # noqa: E402

DEV = torch.device("cuda:0")


def banded_case(args):
    g = torch.Generator().manual_seed(1)
    B, n, hb = args.banded_batch, args.banded_n, args.hb
    band = torch.zeros(B, 2 * hb + 1, n, dtype=torch.float64)
    d = 1.0 + 2.0 * torch.rand(B, n, dtype=torch.float64, generator=g)
    d[:, ::3] *= -1
    band[:, hb] = d
    for j in range(1, hb + 1):
        o = (0.3 / hb) * torch.randn(B, n - j, dtype=torch.float64, generator=g)
        band[:, hb + j, :n - j] = o
        band[:, hb - j, j:] = o
    A = xa.BandedLinearOperator(band.to(DEV), is_hermitian=True)
    return A, torch.randn(B, n, 1, dtype=torch.float64, generator=g).to(DEV), None


def dense_case(args):
    g = torch.Generator().manual_seed(2)
    B, n = args.dense_batch, args.dense_n
    ev = torch.linspace(0.1, 30.0, n, dtype=torch.float64) - 3.05          # 10 % negative eigenvalues
    mats = []
    for _ in range(B):
        Q, _ = torch.linalg.qr(torch.randn(n, n, dtype=torch.float64, generator=g))
        A = (Q * ev) @ Q.T
        mats.append((A + A.T) / 2)
    A = xa.LinearOperator.m(torch.stack(mats).to(DEV), is_hermitian=True)
    return A, torch.randn(B, n, 2, dtype=torch.float64, generator=g).to(DEV), None


def laplace_case(args):
    m = args.grid
    n = m ** 3
    i = torch.arange(n)
    x, y, z = i // (m * m), (i // m) % m, i % m
    rows, cols, vals = [i], [i], [torch.full((n,), 6.0, dtype=torch.float64)]
    for coord, step in ((x, m * m), (y, m), (z, 1)):
        up = coord + 1 < m
        rows += [i[up], i[up] + step]
        cols += [i[up] + step, i[up]]
        vals += [torch.full((int(up.sum()),), -1.0, dtype=torch.float64)] * 2
    t = torch.sparse_coo_tensor(torch.stack([torch.cat(rows), torch.cat(cols)]), torch.cat(vals), (n, n)).coalesce()
    t = t.to_sparse_csr()
    A = xa.SparseLinearOperator(t.crow_indices().to(DEV), t.col_indices().to(DEV), t.values().to(DEV), (n, n),
                                is_hermitian=True)
    # eigenvalues 6 - 2 sum cos(pi k / (m + 1)), many of them degenerate: the shift sits in the middle of the widest
    # gap between two neighbours among the lowest 40 (never on an eigenvalue: that system would be inconsistent)
    c = 2 * torch.cos(math.pi * torch.arange(1, m + 1, dtype=torch.float64) / (m + 1))
    lam = torch.sort((6 - (c[:, None, None] + c[None, :, None] + c[None, None, :])).reshape(-1)).values
    k = int((lam[1:41] - lam[:40]).argmax())
    sigma = float((lam[k] + lam[k + 1]) / 2)
    g = torch.Generator().manual_seed(3)
    return A, torch.randn(n, 2, dtype=torch.float64, generator=g).to(DEV), torch.full((2,), sigma, dtype=torch.float64,
                                                                                      device=DEV)


CASES = {"banded": banded_case, "dense": dense_case, "laplace": laplace_case}
METHODS = {"minres": (nk.minres, {}), "cg": (nk.cg, {}), "cg_normal": (nk.cg, {"posdef": False})}


def run(A, B, E, name, args):
    fn, extra = METHODS[name]
    best, tr = None, {}
    for _ in range(args.reps + 1):                       # the first call warms up
        tr = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            X = fn(A, B, E, None, rtol=args.rtol, max_niter=args.max_niter, trace=tr, **extra)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    R = A.mm(X) - B
    if E is not None:
        R = R - X * E.unsqueeze(-2)
    rel = float((R.norm(dim=-2) / B.norm(dim=-2)).max())
    return {"method": name, "niter": tr["niter"], "napply": tr["napply"], "converged": bool(tr["converged"]),
            "ms_per_solve": best, "ms_per_iter": best / max(tr["niter"], 1), "true_rel_resid": rel,
            "nrestart": tr.get("nrestart")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=sorted(CASES))
    ap.add_argument("--method", action="append", choices=sorted(METHODS))
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--max-niter", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--banded-batch", type=int, default=64)
    ap.add_argument("--banded-n", type=int, default=65536)
    ap.add_argument("--hb", type=int, default=63)
    ap.add_argument("--dense-batch", type=int, default=8)
    ap.add_argument("--dense-n", type=int, default=1000)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--no-json", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minres.json"))
    args = ap.parse_args()
    out = {"rtol": args.rtol, "device": torch.cuda.get_device_name(0), "cases": {}}
    for cname in args.case or sorted(CASES):
        A, B, E = CASES[cname](args)
        rows = [run(A, B, E, m, args) for m in (args.method or ["minres", "cg", "cg_normal"])]
        out["cases"][cname] = {"shape": list(A.shape), "ncols": B.shape[-1], "rows": rows}
        for r in rows:
            print(cname, json.dumps(r), flush=True)
    if not args.no_json:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
