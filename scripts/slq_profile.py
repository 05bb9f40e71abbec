"""Times `linalg.logdet` (stochastic Lanczos quadrature on the xk_slq_* kernels) on one MI355X and writes
profiles/slq.json (reads nothing outside the repository).

Cases: a dense fp64 operator Bt x n x n (A = G G^T / n + I) with 32 probes, beside torch.logdet of the same matrices, and
a CSR 5-point grid operator of order 2^20.  Per case: a warm-up call, then the median of --reps timed calls
(device-synchronised wall time), the time per Lanczos step, applies and host reads.  Then the kernels alone:
xk_slq_step over its four array passes (W, r2, r1 read; r1 written: 4 N s bytes per system) against
kernels.stream_read over the same number of bytes in this very run (`stream_read_GBps`), and xk_slq_quad at
S = 64 * 32, m = 50.

    python scripts/slq_profile.py [--reps 5] [--n 16384] [--batch 2] [--probes 32] [--grid 1024] [--quick] [--out FILE]
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
from xitorch_amd.linalg import logdet                            # noqa: E402
from xitorch_amd.linalg._panel import pad_len, kry_blocks        # noqa: E402
from xitorch_amd.linop import SparseLinearOperator               # noqa: E402


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


def grid_operator(g, dev):
    """5-point operator of a g x g grid plus 0.1 I (symmetric positive definite), CSR on the device"""
    N = g * g
    idx = torch.arange(N, device=dev).reshape(g, g)
    rows = [idx.reshape(-1), idx[:, 1:].reshape(-1), idx[:, :-1].reshape(-1), idx[1:].reshape(-1), idx[:-1].reshape(-1)]
    cols = [idx.reshape(-1), idx[:, :-1].reshape(-1), idx[:, 1:].reshape(-1), idx[:-1].reshape(-1), idx[1:].reshape(-1)]
    vals = [torch.full((N,), 4.1, dtype=torch.float64, device=dev)] + \
        [torch.full((r.numel(),), -1.0, dtype=torch.float64, device=dev) for r in rows[1:]]
    rows, cols, vals = torch.cat(rows), torch.cat(cols), torch.cat(vals)
    order = torch.argsort(rows * N + cols)
    rows, cols, vals = rows[order], cols[order], vals[order]
    crow = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    crow[1:] = torch.cumsum(torch.bincount(rows, minlength=N), 0)
    return SparseLinearOperator(crow, cols, vals, (N, N), is_hermitian=True)


def step_rates(dev, N, S):
    out = []
    for dtype in (torch.float64, torch.float32):
        s = torch.empty((), dtype=dtype).element_size()
        ld, nblk = pad_len(N), kry_blocks(N, dtype)
        W, r2, r1 = (torch.randn((S, ld), dtype=dtype, device=dev) for _ in range(3))
        Pa, Pin, Pout = (torch.zeros((S, 64), dtype=dtype, device=dev) for _ in range(3))
        Pa[:, :nblk] = 1.0 / nblk
        Pin[:, :nblk] = 1.0 / nblk
        state = K.slq_state(S, dev)
        state[:, :, [0, 1, 4, 5, 6]] = 1.0                       # a running mid-iteration state in both slots
        state[:, :, 3] = 3.0
        Tal, Tbe = torch.zeros((S, 50), dtype=torch.float64, device=dev), torch.zeros((S, 50), dtype=torch.float64,
                                                                                      device=dev)
        nbytes = 4 * S * N * s
        ms = kernel_ms(lambda: K.slq_step(W, r2, r1, Pa, Pin, Pout, state, Tal, Tbe, S, N, ld, nblk, 50, 0))
        buf = torch.empty((4 * S, N), dtype=dtype, device=dev)      # the same bytes, rows as long as the vectors
        ref = kernel_ms(lambda: K.stream_read(buf))
        out.append({"dtype": str(dtype), "S": S, "N": N, "bytes": nbytes, "ms": ms, "GBps": nbytes / ms / 1e6,
                    "stream_read_GBps": nbytes / ref / 1e6})
        print(out[-1], flush=True)
    return out


def quad_time(dev, S=64 * 32, m=50):
    g = torch.Generator(device=dev).manual_seed(3)
    Tal = 2.0 + torch.rand((S, m), dtype=torch.float64, device=dev, generator=g)
    Tbe = 0.5 * torch.rand((S, m), dtype=torch.float64, device=dev, generator=g)
    state = K.slq_state(S, dev)
    state[:, :, 3], state[:, :, 6] = float(m), 1.0
    ms = kernel_ms(lambda: K.slq_quad(Tal, Tbe, state, 0, K.SLQ_FN["log"]))
    out = {"S": S, "m": m, "ms": ms}
    print(out, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--probes", type=int, default=32)
    ap.add_argument("--nsteps", type=int, default=50)
    ap.add_argument("--grid", type=int, default=1024)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slq.json"))
    args = ap.parse_args()
    if args.quick:
        args.n, args.grid, args.reps = 2048, 128, 3
    dev = torch.device("cuda:0")
    cases = []
    g = torch.Generator(device=dev).manual_seed(1)
    G = torch.randn((args.batch, args.n, args.n), dtype=torch.float64, device=dev, generator=g)
    A = G @ G.transpose(-2, -1) / args.n
    del G
    A.diagonal(dim1=-2, dim2=-1).add_(1.0)
    A = ((A + A.transpose(-2, -1)) / 2).contiguous()
    for name, op in (("dense", xa.LinearOperator.m(A, is_hermitian=True)), ("csr_grid", grid_operator(args.grid, dev))):
        trace = {}

        def run():
            with torch.no_grad():
                return logdet(op, probes=args.probes, nsteps=args.nsteps, trace=trace)

        ms, all_ms = timed(run, args.reps)
        est = run()
        case = {"operator": name, "shape": list(op.shape), "dtype": str(op.dtype), "probes": args.probes,
                "nsteps": args.nsteps, "ms_median": ms, "ms_all": all_ms, "ms_per_step": ms / args.nsteps,
                "napply": trace.get("napply"), "host_reads": trace.get("host_reads"), "logdet": est.tolist(),
                "stderr": trace["stderr"].tolist()}
        if name == "dense":
            ref_ms, _ = timed(lambda: torch.logdet(A), max(1, args.reps // 2))
            case.update(torch_logdet_ms=ref_ms, torch_logdet=torch.logdet(A).tolist())
        cases.append(case)
        print(case, flush=True)
    result = {"device": torch.cuda.get_device_name(0), "cases": cases,
              "step": step_rates(dev, args.n, args.batch * args.probes) +
              step_rates(dev, args.grid * args.grid, args.probes), "quad": quad_time(dev)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
