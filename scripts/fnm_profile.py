"""Times `linalg.funm_multiply` (two-pass Lanczos on the xk_slq_* and xk_fnm_* kernels) on one MI355X and writes
profiles/fnm.json (reads nothing outside the repository).

Cases: funm_multiply(A, B, "sqrt") on a dense fp64 operator Bt x n x n (A = G G^T / n + I) with 32 columns and 50 steps:
a warm-up call, then the median of --reps timed calls (device-synchronised wall time), beside `logdet` with 32 probes on
the same operator in the same run.  Then the kernels alone: xk_fnm_step over its six array passes (W, r2, r1, X read;
r1, X written: 6 N s bytes per system) against kernels.stream_read over the same number of bytes in this very run
(`stream_read_GBps`), and xk_fnm_eig at S = 64 and 2048, m = 50 and 128.

    python scripts/fnm_profile.py [--reps 5] [--n 16384] [--batch 2] [--cols 32] [--vec 1048576] [--quick] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                     # noqa: E402
import xitorch_amd as xa                                         # noqa: E402
from xitorch_amd import kernels as K                             # noqa: E402
from xitorch_amd.linalg import funm_multiply, logdet             # noqa: E402
from xitorch_amd.linalg._panel import pad_len, kry_blocks        # noqa: E402


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


def kernel_ms(fn_, reps=20):
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
    return statistics.median(ts)


def step_rates(dev, N, S):
    out = []
    for dtype in (torch.float64, torch.float32):
        s = torch.empty((), dtype=dtype).element_size()
        ld, nblk = pad_len(N), kry_blocks(N, dtype)
        W, r2, r1, X = (torch.randn((S, ld), dtype=dtype, device=dev) for _ in range(4))
        state = K.slq_state(S, dev)
        state[:, :, 3] = 50.0                                    # every system runs all 50 steps
        Tal = torch.ones((S, 50), dtype=torch.float64, device=dev)
        Tbe = torch.ones((S, 50), dtype=torch.float64, device=dev)
        C = torch.full((S, 50), 1e-3, dtype=torch.float64, device=dev)
        nbytes = 6 * S * N * s
        ms = kernel_ms(lambda: K.fnm_step(W, r2, r1, X, C, Tal, Tbe, state, S, N, ld, nblk, 50, 3, 0))
        buf = torch.empty((6 * S, N), dtype=dtype, device=dev)      # the same bytes, rows as long as the vectors
        ref = kernel_ms(lambda: K.stream_read(buf))
        out.append({"dtype": str(dtype), "S": S, "N": N, "bytes": nbytes, "ms": ms, "GBps": nbytes / ms / 1e6,
                    "stream_read_GBps": nbytes / ref / 1e6})
        print(out[-1], flush=True)
    return out


def eig_times(dev):
    out = []
    for S in (64, 2048):
        for m in (50, 128):
            g = torch.Generator(device=dev).manual_seed(3)
            Tal = 2.0 + torch.rand((S, m), dtype=torch.float64, device=dev, generator=g)
            Tbe = 0.5 * torch.rand((S, m), dtype=torch.float64, device=dev, generator=g)
            state = K.slq_state(S, dev)
            state[:, :, 3], state[:, :, 6] = float(m), 1.0
            ms = kernel_ms(lambda: K.fnm_eig(Tal, Tbe, state, 0), reps=5)
            theta, Qt, flag = K.fnm_eig(Tal, Tbe, state, 0)
            msc = kernel_ms(lambda: K.fnm_coeff(Qt, theta, state, flag, 0, K.SLQ_FN["sqrt"]), reps=5)
            out.append({"S": S, "m": m, "eig_ms": ms, "coeff_ms": msc})
            print(out[-1], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--cols", type=int, default=32)
    ap.add_argument("--nsteps", type=int, default=50)
    ap.add_argument("--vec", type=int, default=1 << 20)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fnm.json"))
    args = ap.parse_args()
    if args.quick:
        args.n, args.vec, args.reps = 2048, 1 << 14, 3
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    G = torch.randn((args.batch, args.n, args.n), dtype=torch.float64, device=dev, generator=g)
    A = G @ G.transpose(-2, -1) / args.n
    del G
    A.diagonal(dim1=-2, dim2=-1).add_(1.0)
    A = ((A + A.transpose(-2, -1)) / 2).contiguous()
    op = xa.LinearOperator.m(A, is_hermitian=True)
    B = torch.randn((args.n, args.cols), dtype=torch.float64, device=dev, generator=g)
    trace = {}

    def run():
        with torch.no_grad():
            return funm_multiply(op, B, "sqrt", nsteps=args.nsteps, trace=trace)

    ms, all_ms = timed(run, args.reps)
    X = run()
    with torch.no_grad():
        X2 = funm_multiply(op, X, "sqrt", nsteps=args.nsteps)     # sqrt(A) sqrt(A) B = A B
        resid = float(((X2 - A @ B).norm() / (A @ B).norm()))
    ld_ms, _ = timed(lambda: logdet(op, probes=args.cols, nsteps=args.nsteps), args.reps)
    case = {"operator": "dense", "shape": list(op.shape), "dtype": str(op.dtype), "cols": args.cols,
            "nsteps": args.nsteps, "ms_median": ms, "ms_all": all_ms, "napply": trace.get("napply"),
            "tail_max": float(trace["tail"].max()), "sqrt_twice_vs_AB": resid, "logdet_ms_same_run": ld_ms}
    print(case, flush=True)
    result = {"device": torch.cuda.get_device_name(0), "cases": [case],
              "step": step_rates(dev, args.vec, args.cols), "eig": eig_times(dev)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
