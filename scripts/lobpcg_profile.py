"""Time `symeig(method="lobpcg")` and its rotation kernel on one MI355X, against `davidson` on the same inputs.

  dense:  2 x 8192^2 fp64, spectrum 0, 1, 2, ..: neig = 6 lowest, no preconditioner
  grid:   CSR 2-D variable-coefficient grid (tests/fsai_cases.py, 192 x 192) with M = I + 0.3 L / 4 (L the 5-point
          matrix) and precond = fsai(A): neig = 6 lowest
  rotate: xk_lobpcg_rotate alone on fp64 stacks of N = 2^20 (Bt = 2), w = 4, 8, 16, 32 with and without M S: median of
          20 launches, GB/s over the bytes the contract moves ((k + q) rows read and written per stack, + w residual
          rows), beside `stream_read` of the same stacks

One process, a warm-up then the median of 3 solves.  Writes profiles/lobpcg.json.  Run from the repository root:
    python scripts/lobpcg_profile.py
"""
import json
import os
import sys
import time
import warnings
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import xitorch_amd as xa                                            # noqa: E402
from xitorch_amd import kernels as K                                 # noqa: E402
from xitorch_amd.linalg import symeig, fsai                          # noqa: E402
from xitorch_amd.linalg._panel import pad_len                        # noqa: E402

DEV = torch.device("cuda:0")


def timed(fn, reps=3):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2], out


def solve_both(name, op, neig, min_eps, **kw):
    res = {"case": name}
    for meth, extra in (("lobpcg", dict(kw, max_niter=300)), ("davidson", {k: v for k, v in kw.items()})):
        tr = {}

        def go():
            tr.clear()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return symeig(op, neig, "lowest", method=meth, min_eps=min_eps, trace=tr, **extra)
        try:
            t, (ev, X) = timed(go)
        except Exception as e:                                       # (davidson may refuse an option: say so)
            res[meth] = {"error": "%s: %s" % (type(e).__name__, e)}
            continue
        res[meth] = {"seconds": t, "niter": tr.get("niter"), "napply": tr.get("napply"),
                     "ms_per_iter": 1e3 * t / max(1, tr.get("niter") or 1), "best_resid": tr.get("best_resid"),
                     "evals": ev.flatten()[:neig].tolist()}
    return res


def dense_case():
    n = 8192
    g = torch.Generator().manual_seed(5)
    spec = torch.arange(n, dtype=torch.float64)
    v = torch.randn(2, n, 1, dtype=torch.float64, generator=g)
    v = v / torch.linalg.vector_norm(v, dim=-2, keepdim=True)
    D = torch.diag(spec).expand(2, n, n)
    HD = D - 2.0 * v * (v.transpose(-2, -1) @ D)                     # A = H D H, H = I - 2 v v^T
    A = HD - 2.0 * (HD @ v) * v.transpose(-2, -1)
    A = (A + A.transpose(-2, -1)) * 0.5
    return solve_both("dense fp64 2 x 8192^2", xa.LinearOperator.m(A.to(DEV), True), 6, 1e-8)


def grid_case():
    from tests import fsai_cases as fc
    n = 192
    A, _ = fc.grid_operator(n, seed=0, nmembers=1, dtype=torch.float64, device=DEV, batch=False)
    crow, col, _ = fc.grid_csr(n, seed=0)
    crow, col = torch.as_tensor(crow), torch.as_tensor(col)
    rows = torch.arange(n * n).repeat_interleave(crow[1:] - crow[:-1])
    # M = I + 0.3 L / 4 on the grid's own pattern, L the 5-point matrix (4 on the diagonal, -1 beside it)
    mvals = torch.where(rows == col, 1.3, -0.075).to(torch.float64)
    M = xa.SparseLinearOperator(crow.to(DEV), col.to(DEV), mvals.to(DEV),
                                (n * n, n * n), is_hermitian=True)
    return solve_both("CSR grid 192^2 with M and fsai", A, 6, 1e-8, M=M, precond=fsai(A))


def rotate_case():
    out = []
    N, Bt = 1 << 20, 2
    ld = pad_len(N)
    for w in (4, 8, 16, 32):
        for with_m in (False, True):
            k, q = 3 * w, 2 * w
            stacks = [torch.randn((Bt, k, ld), dtype=torch.float64, device=DEV) for _ in range(3 if with_m else 2)]
            S, AS = stacks[0], stacks[1]
            MS = stacks[2] if with_m else None
            C = torch.linalg.qr(torch.randn((Bt, k, q), dtype=torch.float64, device=DEV))[0].contiguous()
            lam = torch.rand((Bt, w), dtype=torch.float64, device=DEV)
            ts = []
            for i in range(22):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                K.lobpcg_rotate(S, AS, MS, C, lam, k, q, w, N=N)
                e1.record()
                torch.cuda.synchronize()
                if i >= 2:
                    ts.append(e0.elapsed_time(e1) * 1e-3)
            t = sorted(ts)[len(ts) // 2]
            ns = len(stacks)
            moved = (ns * (k + q) + w) * N * Bt * 8
            ts = []
            for i in range(12):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for s_ in stacks:
                    K.stream_read(s_)
                e1.record()
                torch.cuda.synchronize()
                if i >= 2:
                    ts.append(e0.elapsed_time(e1) * 1e-3)
            tr = sorted(ts)[len(ts) // 2]
            out.append({"w": w, "k": k, "q": q, "with_m": with_m, "seconds": t, "bytes_moved": moved,
                        "GBps": moved / t / 1e9, "flop": 2.0 * ns * k * q * N * Bt, "GFLOPs": 2.0 * ns * k * q * N * Bt / t / 1e9,
                        "stream_read_GBps_of_the_stacks": ns * k * ld * Bt * 8 / tr / 1e9})
            del stacks, S, AS, MS
    return out


if __name__ == "__main__":
    res = {"device": torch.cuda.get_device_name(0), "rotate_fp64": rotate_case(), "solves": [grid_case(), dense_case()]}
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "lobpcg.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
