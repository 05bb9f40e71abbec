"""Times svd(method="gkl") against svd(method="davidson") (the A^H A route) on the same operator in one process on one
MI355X and writes profiles/gkl.json (reads nothing outside the repository).

Shapes: dense fp64 and fp32 operators Bt x m x n with a slowly decaying spectrum, k in {6, 16}, both methods asked for
the same relative accuracy.  Per case: warm-up call, then the median of --reps (>= 5) timed calls (device-synchronised
wall time), restart cycles, applies, and the error of the returned values against torch.linalg.svdvals.  Also the rate of
xk_gkl_sweep at j = 16 / 63 rows (bytes read: (j + 1) N s, written: N s) against kernels.stream_read in this very run.

    python scripts/gkl_profile.py [--reps 5] [--m 16384] [--n 8192] [--batch 2] [--quick]
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
import xitorch_amd as xa                                         # noqa: E402
from xitorch_amd import kernels as K                             # noqa: E402
from xitorch_amd.linalg import svd                               # noqa: E402
from xitorch_amd.linalg._panel import pad_len                    # noqa: E402


def operator(B, m, n, dtype, dev):
    """B matrices U diag((1 + i)^-1/2) V^T with random orthonormal factors"""
    g = torch.Generator(device=dev).manual_seed(1)
    r = min(m, n)
    U = torch.linalg.qr(torch.randn((B, m, r), dtype=torch.float64, device=dev, generator=g))[0]
    V = torch.linalg.qr(torch.randn((B, n, r), dtype=torch.float64, device=dev, generator=g))[0]
    s = (1.0 + torch.arange(r, dtype=torch.float64, device=dev)) ** -0.5
    return ((U * s) @ V.transpose(-2, -1)).to(dtype).contiguous()


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


def kernel_rate(fn_, nbytes, reps=20):
    for _ in range(3):
        fn_()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record()
        fn_()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return nbytes / (statistics.median(ts) * 1e-3) / 1e9


def sweep_rates(dev, N, Bt):
    out = []
    for dtype in (torch.float64, torch.float32):
        s = torch.empty((), dtype=dtype).element_size()
        ld = pad_len(N)
        for j in (16, 63):
            Q = torch.randn((Bt, j + 1, ld), dtype=dtype, device=dev)
            coef = torch.randn((Bt, j), dtype=torch.float64, device=dev) * 1e-3
            part = torch.zeros((Bt * K.gkl_nval(j, dtype) * K.gkl_chunks(N, dtype),), dtype=torch.float64, device=dev)
            w = Q[:, j]
            nbytes = Bt * (j + 2) * N * s
            rate = kernel_rate(lambda: K.gkl_sweep(Q, j, w, w, coef, None, part, N), nbytes)
            buf = torch.empty((Bt * (j + 2), ld), dtype=dtype, device=dev)
            ref = kernel_rate(lambda: K.stream_read(buf), buf.numel() * s)
            out.append({"dtype": str(dtype), "Bt": Bt, "N": N, "rows": j, "bytes": nbytes, "sweep_GBps": rate,
                        "stream_read_GBps": ref})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--m", type=int, default=16384)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if args.quick:
        args.m, args.n, args.reps = 2048, 1024, 5
    dev = torch.device("cuda:0")
    cases = []
    for dtype in (torch.float64, torch.float32):
        A = operator(args.batch, args.m, args.n, dtype, dev)
        true = torch.linalg.svdvals(A.double())
        eps = 100 * torch.finfo(dtype).eps
        for k in (6, 16):
            want = true[:, :k].flip(-1)
            for method, opts in (("gkl", {"min_eps": eps}), ("davidson", {"min_eps": eps})):
                trace = {}
                op = xa.LinearOperator.m(A)

                def run():
                    with warnings.catch_warnings(), torch.no_grad():
                        warnings.simplefilter("ignore")
                        return svd(op, k=k, mode="uppest", method=method, trace=trace, **opts)

                ms, all_ms = timed(run, args.reps)
                _, s, _ = run()
                cases.append({"dtype": str(dtype), "shape": [args.batch, args.m, args.n], "k": k, "method": method,
                              "ms_median": ms, "ms_all": all_ms, "niter": trace.get("niter"),
                              "napply": trace.get("napply"), "panel_kernel": trace.get("panel_kernel"),
                              "max_abs_err_over_u_smax": float((s.double() - want).abs().max()
                                                               / (torch.finfo(dtype).eps * true.max()))})
                print(cases[-1], flush=True)
    result = {"device": torch.cuda.get_device_name(0), "cases": cases,
              "sweep": sweep_rates(dev, args.m, args.batch)}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "gkl.json"), "w") as f:
        json.dump(result, f, indent=1)
    print("wrote profiles/gkl.json")


if __name__ == "__main__":
    main()
