"""Times fsai_lu() and what it buys gmres on one MI355X and writes profiles/fsai_lu.json (reads nothing outside the
repository).

Problem: the variable-coefficient convection-diffusion operator of the tests (tests/fsai_lu_cases.convdiff, built here
in torch ops) on an n x n grid at scripts/fsai_profile.py's size: n = 1024, N = 2^20 rows, fp64, convection strength
pe = 0.5, batch 1.  Measured:
  * the build time of fsai_lu(A, power=1) and fsai_lu(A, power=2): the whole call, the pattern alone (torch ops), and
    xk_fsai_lu_build alone;
  * time-to-tolerance of gmres(restart=--restart) without a preconditioner and with each of the two, one right-hand
    side: Arnoldi steps, applies, restarts, device-synchronised wall time (warm-up call, then the median of --reps calls).

    python scripts/fsai_lu_profile.py [--n 1024] [--pe 0.5] [--reps 5] [--rtol 1e-8] [--restart 50] [--max-niter 5000]
                                      [--out profiles/fsai_lu.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                     # noqa: E402
from xitorch_amd import kernels as K                             # noqa: E402
from xitorch_amd.linop import SparseLinearOperator               # noqa: E402
from xitorch_amd.linalg import fsai_lu, host_precond             # noqa: E402
from xitorch_amd.linalg import native_krylov                     # noqa: E402


def convdiff_operator(n, pe, dev, seed=0):
    """SparseLinearOperator (N, N), fp64, columns ascending: harmonic means of the cell conductances exp(U(-1.5, 1.5))
    on the edges, convection +-pe / 2 (half of it in the second direction) on the off-diagonals, 0.01 on the diagonal"""
    g = torch.Generator().manual_seed(seed)
    N = n * n
    kc = torch.exp(3.0 * torch.rand((n, n), dtype=torch.float64, generator=g) - 1.5)
    idx = torch.arange(N).reshape(n, n)
    hm = lambda a, b: 2 * a * b / (a + b)
    kd, kr = hm(kc[:-1], kc[1:]), hm(kc[:, :-1], kc[:, 1:])         # edges to the next row / the next column
    diag = torch.full((n, n), 0.01, dtype=torch.float64)
    # the reference form adds the cell's own conductance for an edge that leaves the grid
    diag[:-1] += kd
    diag[-1] += kc[-1]
    diag[1:] += kd
    diag[0] += kc[0]
    diag[:, :-1] += kr
    diag[:, -1] += kc[:, -1]
    diag[:, 1:] += kr
    diag[:, 0] += kc[:, 0]
    rows = torch.cat([idx.reshape(-1), idx[:-1].reshape(-1), idx[1:].reshape(-1), idx[:, :-1].reshape(-1),
                      idx[:, 1:].reshape(-1)])
    cols = torch.cat([idx.reshape(-1), idx[1:].reshape(-1), idx[:-1].reshape(-1), idx[:, 1:].reshape(-1),
                      idx[:, :-1].reshape(-1)])
    vals = torch.cat([diag.reshape(-1), (-kd + pe / 2).reshape(-1), (-kd - pe / 2).reshape(-1),
                      (-kr + pe / 4).reshape(-1), (-kr - pe / 4).reshape(-1)])
    order = torch.argsort(rows * N + cols)
    rows, cols, vals = rows[order], cols[order], vals[order]
    crow = torch.zeros(N + 1, dtype=torch.int64)
    crow[1:] = torch.cumsum(torch.bincount(rows, minlength=N), 0)
    return SparseLinearOperator(crow.to(dev), cols.to(dev), vals.to(dev), (N, N))


def timed(fn_, reps):
    fn_()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn_()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--pe", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--restart", type=int, default=50)
    ap.add_argument("--max-niter", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fsai_lu.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N = args.n * args.n
    A = convdiff_operator(args.n, args.pe, dev)
    B = torch.randn((N, 1), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    cases = []
    pre = {None: None}
    vals = A.values.reshape(-1, A.nnz)
    for power in (1, 2):
        ms, all_ms = timed(lambda: fsai_lu(A, power=power), args.reps)
        P = fsai_lu(A, power=power)
        pre[power] = P
        G = P.GL
        kms, kall = timed(lambda: K.fsai_lu_build(A.crow, A.col, vals, G.crow, G.col, N, check_pattern=False), args.reps)
        pms, _ = timed(lambda: host_precond.fsai_pattern(A._pattern.row_of, A.col, N, power, 32, full=True), args.reps)
        cases.append({"what": "build", "n": args.n, "pe": args.pe, "power": power, "nnz_A": A.nnz, "nnz_G": G.nnz,
                      "max_row": int((G.crow[1:] - G.crow[:-1]).max()), "nfallback": int(P.nfallback.sum()),
                      "fsai_lu_ms_median": ms, "fsai_lu_ms_all": all_ms, "kernel_ms_median": kms, "kernel_ms_all": kall,
                      "pattern_ms_median": pms})
        print(cases[-1], flush=True)
    for power, P in pre.items():
        trace = {}

        def run():
            with warnings.catch_warnings(), torch.no_grad():
                warnings.simplefilter("ignore")
                return native_krylov.gmres(A, B, posdef=True, rtol=args.rtol, atol=0.0, max_niter=args.max_niter,
                                           restart=args.restart, precond_r=P, trace=trace)

        ms, all_ms = timed(run, args.reps)
        X = run()
        res = float(((A.mm(X) - B).norm(dim=-2) / B.norm(dim=-2)).max())
        cases.append({"what": "gmres", "n": args.n, "pe": args.pe, "restart": args.restart,
                      "precond": "none" if power is None else "fsai_lu(power=%d)" % power, "rtol": args.rtol,
                      "ms_median": ms, "ms_all": all_ms, "arnoldi_steps": trace.get("arnoldi_steps"),
                      "restarts": trace.get("restarts"), "napply": trace.get("napply"),
                      "converged": trace.get("converged"), "true_rel_resid": res})
        print(cases[-1], flush=True)
    result = {"device": torch.cuda.get_device_name(0), "dtype": "float64", "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
