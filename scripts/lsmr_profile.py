"""Times `linalg.lstsq` (LSMR on the xk_lsmr_* kernels) on one MI355X and writes profiles/lsmr.json (reads nothing
outside the repository).

Per case (dense fp64 and fp32 operators Bt x m x n with singular values log-spaced in [1 / kappa, 1], ncols columns):
a warm-up call, then the median of --reps timed calls (device-synchronised wall time), iterations, applies, host reads,
restarts and the time per iteration.  Then the three streaming passes alone, on vectors of the same shape: the rate of
xk_lsmr_bidiag (u half and v half: bytes read 2 N s, written N s) and xk_lsmr_update (read 4 N s, written 3 N s)
against kernels.stream_read over the same number of bytes in this very run (`stream_read_GBps`).

    python scripts/lsmr_profile.py [--reps 5] [--m 16384] [--n 8192] [--batch 2] [--ncols 4] [--quick] [--out FILE]
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
from xitorch_amd.linalg import lstsq                             # noqa: E402
from xitorch_amd.linalg.native_lsmr import _Side                 # noqa: E402


def operator(B, m, n, kappa, dtype, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    r = min(m, n)
    U = torch.linalg.qr(torch.randn((B, m, r), dtype=torch.float64, device=dev, generator=g))[0]
    V = torch.linalg.qr(torch.randn((B, n, r), dtype=torch.float64, device=dev, generator=g))[0]
    s = torch.logspace(0, -torch.log10(torch.tensor(kappa)).item(), r, dtype=torch.float64, device=dev)
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


def pass_rates(dev, m, n, Bt, nc):
    out = []
    for dtype in (torch.float64, torch.float32):
        s = torch.empty((), dtype=dtype).element_size()
        S = Bt * nc
        U, V = _Side(m, Bt, nc, dtype, dev), _Side(n, Bt, nc, dtype, dev)
        rnd = lambda side: torch.randn(side.shape, dtype=dtype, device=dev)
        opu, uh, opv, vh, h, hbar, x = rnd(U), rnd(U), rnd(V), rnd(V), rnd(V), rnd(V), rnd(V)
        Pu, Pv, Px0, Px1, run = (V.partial() for _ in range(5))
        Pu[:, :U.nblk] = 1.0 / U.nblk
        Pv[:, :V.nblk] = 1.0 / V.nblk
        state = K.lsmr_state(S, dev)
        state[:, :, [0, 1, 2, 3, 4, 5, 6, 9, 11, 15, 20, 26]] = 1.0           # a running mid-iteration state in both slots
        state[:, :, 17] = 1e100
        state[:, :, 18] = 3.0
        passes = (
            ("bidiag_u", lambda: K.lsmr_bidiag(opu, uh, Pv, Pu, state, 0, S, m, U.ld, U.nblk, V.nblk, 0), 3 * S * m * s),
            ("bidiag_v", lambda: K.lsmr_bidiag(opv, vh, Pu, Pv, state, 1, S, n, V.ld, V.nblk, U.nblk, 0), 3 * S * n * s),
            ("update", lambda: K.lsmr_update(vh, h, hbar, x, Pu, Pv, Px0, Px1, state, run, S, n, V.ld, V.nblk,
                                             U.nblk, 0, damp=0.0, atol=0.0, btol=0.0, conlim=1e300), 7 * S * n * s))
        for name, fn_, nbytes in passes:
            rate = kernel_rate(fn_, nbytes)
            buf = torch.empty((nbytes // s,), dtype=dtype, device=dev)
            ref = kernel_rate(lambda: K.stream_read(buf), buf.numel() * s)
            out.append({"dtype": str(dtype), "S": S, "m": m, "n": n, "pass": name, "bytes": nbytes, "GBps": rate,
                        "stream_read_GBps": ref})
            print(out[-1], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--m", type=int, default=16384)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--ncols", type=int, default=4)
    ap.add_argument("--kappa", type=float, default=1e2)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lsmr.json"))
    args = ap.parse_args()
    if args.quick:
        args.m, args.n, args.reps = 2048, 1024, 3
    dev = torch.device("cuda:0")
    cases = []
    for dtype in (torch.float64, torch.float32):
        A = operator(args.batch, args.m, args.n, args.kappa, dtype, dev)
        g = torch.Generator(device=dev).manual_seed(2)
        B = torch.randn((args.m, args.ncols), dtype=torch.float64, device=dev, generator=g).to(dtype)
        tol = 1e-10 if dtype == torch.float64 else 1e-4
        for damp in (0.0, 1e-2):
            trace = {}
            op = xa.LinearOperator.m(A)

            def run():
                with warnings.catch_warnings(), torch.no_grad():
                    warnings.simplefilter("ignore")
                    return lstsq(op, B, damp=damp, atol=tol, btol=tol, max_niter=4000, trace=trace)

            ms, all_ms = timed(run, args.reps)
            x = run()
            r = B - A @ x
            gopt = A.transpose(-2, -1) @ r - damp * damp * x
            cases.append({"dtype": str(dtype), "shape": [args.batch, args.m, args.n], "ncols": args.ncols,
                          "kappa": args.kappa, "damp": damp, "atol": tol, "ms_median": ms, "ms_all": all_ms,
                          "niter": trace.get("niter"), "napply": trace.get("napply"),
                          "host_reads": trace.get("host_reads"), "restarts": trace.get("restarts"),
                          "ms_per_iteration": ms / max(1, trace.get("niter") or 1),
                          "panel_kernel": trace.get("panel_kernel"),
                          "max_opt_resid": float(torch.linalg.vector_norm(gopt.double(), dim=-2).max())})
            print(cases[-1], flush=True)
    result = {"device": torch.cuda.get_device_name(0), "cases": cases,
              "passes": pass_rates(dev, args.m, args.n, args.batch, args.ncols)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
