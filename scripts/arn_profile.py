"""Times eigs(method="arnoldi") in one process on one MI355X and writes profiles/arn.json (reads nothing outside the
repository).

Dense fp64 operator B x n x n = R / sqrt(n) + U diag(lambda) U^T: a circular-law bulk of radius ~1 and eight outliers of
modulus 1.5 .. 2; neig = 6, ncv = 20.  Per call: warm-up call, then the median of --reps (>= 5) timed calls
(device-synchronised wall time), restart cycles, applies, host reads.  The pieces of one cycle are timed on their own
with HIP events (3 warm-up launches, the median of 20): one apply of one column, one CGS2 orthogonalisation (three
sweeps, three finishes, the scaling sweep) against 13 rows (the middle of a restarted cycle), one xk_arn_schur; the
shares are these times multiplied by their counts per cycle over their sum, NOT a trace of the call.  xk_arn_schur alone
at m = 20, 48 (= xk_arn_max_rows()) for Bt = 2 and 64 on random real matrices, and for scale torch.linalg.eig on one
4096 x 4096 member in the same run (on the device if the library serves it there, else in host memory: the entry says
which).

    python scripts/arn_profile.py [--reps 5] [--n 16384] [--batch 2] [--quick]
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
from xitorch_amd.linalg import eigs                              # noqa: E402
from xitorch_amd.linalg._panel import RectPanelOperator          # noqa: E402
from xitorch_amd.linalg.native_arnoldi import _State             # noqa: E402


def operator(B, n, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    A = torch.randn((B, n, n), dtype=torch.float64, device=dev, generator=g) / n ** 0.5
    U = torch.linalg.qr(torch.randn((B, n, 8), dtype=torch.float64, device=dev, generator=g))[0]
    lam = torch.linspace(2.0, 1.5, 8, dtype=torch.float64, device=dev)
    return (A + (U * lam) @ U.transpose(-2, -1)).contiguous()


def event_ms(fn_, reps=20):
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


def schur_alone(dev, m, Bt):
    g = torch.Generator(device=dev).manual_seed(m + Bt)
    H = torch.randn((Bt, m + 1, m), dtype=torch.float64, device=dev, generator=g)
    Hn = torch.empty_like(H)
    neig = 6
    out = K.arn_schur(H, neig, neig + (m - neig) // 2, Hnext=Hn)
    ms = event_ms(lambda: K.arn_schur(H, neig, neig + (m - neig) // 2, Hnext=Hn, out=out))
    return {"m": m, "Bt": Bt, "ms": ms, "qr_iterations_max": int(out[4][:, 1].max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if args.quick:
        args.n = 2048
    dev = torch.device("cuda:0")
    neig, ncv = 6, 20
    A = operator(args.batch, args.n, dev)
    op = xa.LinearOperator.m(A)
    trace = {}

    def run():
        with warnings.catch_warnings(), torch.no_grad():
            warnings.simplefilter("ignore")
            return eigs(op, neig, "LM", ncv=ncv, min_eps=1e-8, trace=trace)

    run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(max(args.reps, 5)):
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    call = {"shape": [args.batch, args.n, args.n], "dtype": "float64", "neig": neig, "ncv": ncv,
            "ms_median": statistics.median(ts), "ms_all": ts, "niter": trace["niter"], "napply": trace["napply"],
            "host_reads": trace["host_reads"], "converged": trace["converged"],
            "ms_per_cycle": statistics.median(ts) / trace["niter"], "resid_max": float(trace["resid"].max())}
    print(call, flush=True)
    # the pieces of a cycle
    st = _State(args.batch, ncv, args.n, neig, torch.float64, dev)
    st.V.panel.normal_()
    pop = RectPanelOperator(op, [args.batch], args.batch)
    j = 13
    t_apply = event_ms(lambda: pop.apply(st.V.panel[:, j:j + 1], st.V.panel[:, j + 1:j + 2]))
    t_orth = event_ms(lambda: st.orthogonalise(j))
    st.H.normal_()
    keep = neig + (ncv - neig) // 2
    t_schur = event_ms(lambda: K.arn_schur(st.H, neig, keep, Hnext=st.Hnext, out=st.out))
    steps = ncv - keep
    tot = steps * (t_apply + t_orth) + t_schur
    pieces = {"apply_ms": t_apply, "orthogonalise_ms_at_13_rows": t_orth, "schur_ms": t_schur, "steps_per_cycle": steps,
              "share_apply": steps * t_apply / tot, "share_sweeps": steps * t_orth / tot, "share_schur": t_schur / tot,
              "sum_ms_per_cycle": tot}
    print(pieces, flush=True)
    schur = [schur_alone(dev, m, Bt) for m in (20, K.arn_max_rows()) for Bt in (2, 64)]
    print(schur, flush=True)
    n4 = 1024 if args.quick else 4096
    M = A[0, :n4, :n4].contiguous()
    try:
        where = "device"
        torch.linalg.eigvals(M[:64, :64])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch.linalg.eig(M)
        torch.cuda.synchronize()
    except RuntimeError:
        where = "host"
        Mh = M.cpu()
        t0 = time.perf_counter()
        torch.linalg.eig(Mh)
    dense = {"n": n4, "where": where, "ms": (time.perf_counter() - t0) * 1e3}
    print(dense, flush=True)
    result = {"device": torch.cuda.get_device_name(0), "call": call, "cycle_pieces": pieces, "schur_alone": schur,
              "torch_linalg_eig": dense}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "arn.json"), "w") as f:
        json.dump(result, f, indent=1)
    print("wrote profiles/arn.json")


if __name__ == "__main__":
    main()
