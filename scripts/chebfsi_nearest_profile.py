"""Times symeig(mode="nearest", method="chebfsi") in one process on one MI355X and writes
profiles/chebfsi_nearest.json (reads nothing outside the repository).

Per case (a dense symmetric operator with a graded spectrum, sigma inside it): a warm-up call, then the median of
--reps (>= 5) timed calls (device-synchronised wall time), outer iterations, applies, the degrees taken and the time per
outer iteration.  The same pairs by the folded-operator route — chebfsi(mode="lowest") on (A - sigma)^2 through
`A.matmul`, which squares the condition number and doubles every apply — on the same inputs, to the residual it reaches.
Also the rate of xk_cheb_clenshaw (5 arrays, and 4 where gamma = 0) and of xk_cheb_step at its own bytes against
kernels.stream_read measured in this very run, on panels of 256 MiB each (--rate-n columns of 64 vectors: far beyond
the last-level cache, so the figures are HBM rates and not launch overheads).

    python scripts/chebfsi_nearest_profile.py [--reps 5] [--n 2048] [--rate-n 65536] [--quick]
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
from xitorch_amd.linalg import symeig                            # noqa: E402
from xitorch_amd.linalg._panel import pad_len                    # noqa: E402


def operator(B, n, dtype, dev):
    """B symmetric matrices with a graded spectrum: a random symmetric perturbation of diag(0 .. n-1) / 8"""
    g = torch.Generator(device=dev).manual_seed(1)
    R = torch.randn((B, n, n), dtype=dtype, device=dev, generator=g) * 0.02
    A = (R + R.transpose(-2, -1)) * 0.5
    A.diagonal(dim1=-2, dim2=-1).add_(torch.arange(n, dtype=dtype, device=dev) / 8)
    return A


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--rate-n", type=int, default=65536, help="vector length of the panels of the streaming rates")
    ap.add_argument("--quick", action="store_true", help="neig = 8 only, no folded-operator route")
    ap.add_argument("--no-json", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    reps = max(5, args.reps)
    out = {"device": torch.cuda.get_device_name(0), "n": args.n, "reps": reps, "cases": [], "stream": {}}
    warnings.simplefilter("ignore", xa.ConvergenceWarning)
    for dtype, B, eps_ in ((torch.float32, 4, 2e-3), (torch.float64, 2, 1e-8)):
        A = operator(B, args.n, dtype, dev)
        op = xa.LinearOperator.m(A, True)
        sigma = args.n / 8 * 0.371 + 0.03                        # inside the spectrum, off the diagonal's grid
        for neig in ((8,) if args.quick else (8, 32)):
            tr = {}
            with torch.no_grad():
                ms, all_ms = timed(lambda: symeig(op, neig, "nearest", method="chebfsi", sigma=sigma, min_eps=eps_,
                                                  trace=tr), reps)
            rec = {"dtype": str(dtype), "B": B, "neig": neig, "route": "nearest", "sigma": sigma, "min_eps": eps_,
                   "ms": ms, "ms_all": all_ms, "niter": tr.get("niter"), "napply": tr.get("napply"),
                   "degrees": tr.get("degrees"), "columns": tr.get("w"), "ms_per_outer_iteration": ms / tr["niter"],
                   "best_resid": tr.get("best_resid"), "degree_capped": tr.get("degree_capped"),
                   "panel_kernel": tr.get("panel_kernel"), "small_eigh": tr.get("small_eigh")}
            print(json.dumps({k: v for k, v in rec.items() if k != "ms_all"}), flush=True)
            out["cases"].append(rec)
            if args.quick:
                continue
            # the folded operator (A - sigma)^2, lowest pairs: every apply is two applies of A
            shifted = xa.LinearOperator.m(A - sigma * torch.eye(args.n, dtype=dtype, device=dev), True)
            folded = shifted.matmul(shifted, is_hermitian=True)
            tr = {}
            with torch.no_grad():
                ms, all_ms = timed(lambda: symeig(folded, neig, "lowest", method="chebfsi", min_eps=eps_, max_niter=60,
                                                  trace=tr), reps)
            rec = {"dtype": str(dtype), "B": B, "neig": neig, "route": "folded (A - sigma)^2, mode lowest",
                   "sigma": sigma, "min_eps": eps_, "ms": ms, "ms_all": all_ms, "niter": tr.get("niter"),
                   "napply_folded": tr.get("napply"), "napply_A": 2 * (tr.get("napply") or 0), "columns": tr.get("w"),
                   "ms_per_outer_iteration": ms / max(1, tr.get("niter") or 1), "best_resid": tr.get("best_resid"),
                   "panel_kernel": tr.get("panel_kernel")}
            print(json.dumps({k: v for k, v in rec.items() if k != "ms_all"}), flush=True)
            out["cases"].append(rec)
        # streaming rates: 64-column blocks of vectors of length --rate-n, 256 MiB per array at the default
        del A, op
        torch.cuda.empty_cache()
        s = torch.empty((), dtype=dtype).element_size()
        p, ld = 64, pad_len(args.rate_n)
        B = 64 // s                                              # 16 members in fp32, 8 in fp64
        panels = [torch.randn((B, p, ld), dtype=dtype, device=dev) for _ in range(5)]
        coef4 = torch.tensor([[0.5, -0.25, 0.125, 0.0625]] * B, dtype=torch.float64, device=dev)
        coef4_first = torch.tensor([[0.5, -0.25, 0.0, 0.0625]] * B, dtype=torch.float64, device=dev)
        coef3 = coef4[:, :3].contiguous()
        one = B * p * ld * s
        big = torch.empty((5 * one // s,), dtype=dtype, device=dev).view(-1, ld)
        rates = {
            "bytes_per_array": one, "B": B, "p": p, "N": args.rate_n,
            "stream_read_GBs": kernel_rate(lambda: K.stream_read(big), 5 * one),
            "cheb_clenshaw_GBs": kernel_rate(lambda: K.cheb_clenshaw(panels[0], panels[1], panels[2], panels[3], coef4,
                                                                     out=panels[4]), 5 * one),
            "cheb_clenshaw_inplace_GBs": kernel_rate(lambda: K.cheb_clenshaw(panels[0], panels[1], panels[2], panels[3],
                                                                             coef4), 5 * one),
            "cheb_clenshaw_gamma0_GBs": kernel_rate(lambda: K.cheb_clenshaw(panels[0], panels[1], panels[2], panels[3],
                                                                            coef4_first, out=panels[4]), 4 * one),
            "cheb_step_GBs": kernel_rate(lambda: K.cheb_step(panels[0], panels[1], panels[2], coef3, out=panels[4]),
                                         4 * one),
        }
        rates["cheb_clenshaw_over_stream_read"] = rates["cheb_clenshaw_GBs"] / rates["stream_read_GBs"]
        rates["cheb_clenshaw_over_cheb_step"] = rates["cheb_clenshaw_GBs"] / rates["cheb_step_GBs"]
        print(json.dumps(rates), flush=True)
        out["stream"][str(dtype)] = rates
        del panels, big
        torch.cuda.empty_cache()
    if not args.no_json:
        path = os.path.join(ROOT, "profiles", "chebfsi_nearest.json")
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
        print("wrote", path)


if __name__ == "__main__":
    main()
