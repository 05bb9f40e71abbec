"""Times symeig(method="chebfsi") against method="davidson" in one process on one MI355X and writes
profiles/chebfsi.json (reads nothing outside the repository).

Shapes: dense exactly symmetric fp32 16 x 8192^2 and fp64 8 x 8192^2, neig in {16, 64, 128}, both methods to the same
min_eps.  Per case: warm-up call, then the median of --reps (>= 5) timed calls (device-synchronised wall time), applies x
columns, and the panel kernel that served the applies (PanelOperator.last_kernel through trace["panel_kernel"]).  Also
the rate of xk_cheb_step and of xk_lincomb at the same bytes against kernels.stream_read measured in this very run.

    python scripts/chebfsi_profile.py [--reps 5] [--n 8192] [--quick]
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
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--quick", action="store_true", help="neig = 16 only")
    ap.add_argument("--no-json", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "n": args.n, "reps": max(5, args.reps), "cases": [], "stream": {}}
    warnings.simplefilter("ignore", xa.ConvergenceWarning)
    for dtype, B, eps_ in ((torch.float32, 16, 2e-3), (torch.float64, 8, 1e-8)):
        A = operator(B, args.n, dtype, dev)
        op = xa.LinearOperator.m(A, True)
        for neig in ((16,) if args.quick else (16, 64, 128)):
            for meth in ("chebfsi", "davidson"):
                tr = {}
                with torch.no_grad():
                    ms, all_ms = timed(lambda: symeig(op, neig, "lowest", method=meth, min_eps=eps_, trace=tr),
                                       max(5, args.reps))
                # chebfsi applies the whole block every time; davidson applies only its unconverged columns and its
                # trace carries no column count: the field stays empty there
                cols = tr.get("w")
                rec = {"dtype": str(dtype), "B": B, "neig": neig, "method": meth, "min_eps": eps_, "ms": ms,
                       "ms_all": all_ms, "niter": tr.get("niter"), "napply": tr.get("napply"), "columns": cols,
                       "apply_columns": (tr.get("napply") or 0) * cols if cols else None, "best_resid": tr.get("best_resid"),
                       "panel_kernel": tr.get("panel_kernel"), "small_eigh": tr.get("small_eigh")}
                print(json.dumps({k: v for k, v in rec.items() if k != "ms_all"}), flush=True)
                out["cases"].append(rec)
        # streaming rates at the bytes of a 64-column block of this dtype
        p, ld = 64, pad_len(args.n)
        s = A.element_size()
        panels = [torch.randn((B, p, ld), dtype=dtype, device=dev) for _ in range(4)]
        coef = torch.tensor([[0.5, -0.25, 0.125]] * B, dtype=torch.float64, device=dev)
        nbytes = 4 * B * p * ld * s
        big = torch.empty((nbytes // s,), dtype=dtype, device=dev).view(-1, ld)
        KL = 24
        assert KL * ((p + 7) // 8) + p == 4 * p
        C = torch.randn((B, KL, p), dtype=dtype, device=dev)
        rates = {
            "bytes": nbytes,
            "stream_read_GBs": kernel_rate(lambda: K.stream_read(big), nbytes),
            "cheb_step_GBs": kernel_rate(lambda: K.cheb_step(panels[0], panels[1], panels[2], coef, out=panels[3]),
                                         nbytes),
            # xk_lincomb at the SAME bytes: k = 24 rows combined into p = 64 columns reads the 24 rows once per group
            # of 8 columns and writes 64 rows: 24 * 8 + 64 = 256 rows moved = cheb_step's 4 p
            "lincomb_GBs": kernel_rate(lambda: K.lincomb(panels[0], C, panels[3], KL, p, coef_layout="ac"), nbytes),
        }
        rates["cheb_step_over_stream_read"] = rates["cheb_step_GBs"] / rates["stream_read_GBs"]
        rates["cheb_step_over_lincomb"] = rates["cheb_step_GBs"] / rates["lincomb_GBs"]
        print(json.dumps(rates), flush=True)
        out["stream"][str(dtype)] = rates
        del A, op, panels, big
        torch.cuda.empty_cache()
    if not args.no_json:
        path = os.path.join(ROOT, "profiles", "chebfsi.json")
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
        print("wrote", path)


if __name__ == "__main__":
    main()
