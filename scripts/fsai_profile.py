"""Times fsai() and what it buys cg on one MI355X and writes profiles/fsai.json (reads nothing outside the repository).

Problem: the 5-point diffusion operator on an n x n grid with Dirichlet boundaries and edge conductances exp(1.5 g),
g ~ N(0, 1) (the tests' problem at the project's size: n = 1024, N = 2^20 rows, fp64), batch 1 and 8 with different
conductances per member.  Measured per batch size:
  * the build time of fsai(A, power=1) and fsai(A, power=2): pattern (torch ops) + xk_fsai_build, and the kernel alone;
  * time-to-tolerance of solve(method="cg") without a preconditioner and with each of the two, one right-hand side per
    member: iterations, applies, device-synchronised wall time (warm-up call, then the median of --reps calls).

    python scripts/fsai_profile.py [--n 1024] [--reps 5] [--rtol 1e-8] [--max-niter 20000] [--out profiles/fsai.json]
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
from xitorch_amd.linalg import solve, fsai                       # noqa: E402
from xitorch_amd.linalg import host_precond                      # noqa: E402


def grid_operator(n, nb, dev, seed=0):
    """SparseLinearOperator (nb, N, N), fp64, both triangles stored, columns ascending"""
    g = torch.Generator().manual_seed(seed)
    N = n * n
    k = torch.arange(N).reshape(n, n)
    rows = torch.cat([k.reshape(-1), k[:, 1:].reshape(-1), k[:, :-1].reshape(-1), k[1:].reshape(-1), k[:-1].reshape(-1)])
    cols = torch.cat([k.reshape(-1), k[:, :-1].reshape(-1), k[:, 1:].reshape(-1), k[:-1].reshape(-1), k[1:].reshape(-1)])
    vals = []
    for _ in range(nb):
        cx = torch.exp(1.5 * torch.randn((n, n + 1), dtype=torch.float64, generator=g))
        cy = torch.exp(1.5 * torch.randn((n + 1, n), dtype=torch.float64, generator=g))
        d = cx[:, :-1] + cx[:, 1:] + cy[:-1] + cy[1:]
        vals.append(torch.cat([d.reshape(-1), -cx[:, 1:-1].reshape(-1), -cx[:, 1:-1].reshape(-1),
                               -cy[1:-1].reshape(-1), -cy[1:-1].reshape(-1)]))
    order = torch.argsort(rows * N + cols)
    rows, cols = rows[order], cols[order]
    vals = torch.stack(vals)[:, order]
    crow = torch.zeros(N + 1, dtype=torch.int64)
    crow[1:] = torch.cumsum(torch.bincount(rows, minlength=N), 0)
    return SparseLinearOperator(crow.to(dev), cols.to(dev), vals.to(dev), (nb, N, N), is_hermitian=True)


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--max-niter", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fsai.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N = args.n * args.n
    cases = []
    for nb in (1, 8):
        A = grid_operator(args.n, nb, dev)
        B = torch.randn((nb, N, 1), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
        pre = {None: None}
        for power in (1, 2):
            ms, all_ms = timed(lambda: fsai(A, power=power), args.reps)
            P = fsai(A, power=power)
            pre[power] = P
            G = P.G
            vals = A.values.reshape(-1, A.nnz)
            kms, kall = timed(lambda: K.fsai_build(A.crow, A.col, vals, G.crow, G.col, N, check_pattern=False), args.reps)
            pms, _ = timed(lambda: host_precond.fsai_pattern(A._pattern.row_of, A.col, N, power, 32), args.reps)
            cases.append({"what": "build", "batch": nb, "n": args.n, "power": power, "nnz_A": A.nnz, "nnz_G": G.nnz,
                          "max_row": int((G.crow[1:] - G.crow[:-1]).max()), "nfallback": int(P.nfallback.sum()),
                          "fsai_ms_median": ms, "fsai_ms_all": all_ms, "kernel_ms_median": kms, "kernel_ms_all": kall,
                          "pattern_ms_median": pms})
            print(cases[-1], flush=True)
        for power, P in pre.items():
            trace = {}

            def run():
                with warnings.catch_warnings(), torch.no_grad():
                    warnings.simplefilter("ignore")
                    return solve(A, B, method="cg", posdef=True, rtol=args.rtol, atol=0.0, max_niter=args.max_niter,
                                 precond=P, trace=trace)

            ms, all_ms = timed(run, args.reps)
            X = run()
            res = float(((A.mm(X) - B).norm(dim=-2) / B.norm(dim=-2)).max())
            cases.append({"what": "cg", "batch": nb, "n": args.n, "precond": "none" if power is None else "fsai(power=%d)" % power,
                          "rtol": args.rtol, "ms_median": ms, "ms_all": all_ms, "niter": trace.get("niter"),
                          "napply": trace.get("napply"), "converged": trace.get("converged"), "true_rel_resid": res})
            print(cases[-1], flush=True)
    result = {"device": torch.cuda.get_device_name(0), "dtype": "float64", "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
