"""Record of the CSR operator (xk_csr_mm) on the MI355X: kernel time and HBM fraction on algorithmic bytes by
workload, torch.sparse.mm on the same CSR where it runs, and cg on the 7-point Poisson problem with the share of time
spent in the operator product.

    python scripts/sparse_bench.py --out profiles/csr_mm.json             timed record (HIP events)
    python scripts/sparse_bench.py --pmc-only --only I                      one launch of workload I, for
                                                                            rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE
    python scripts/sparse_bench.py --merge-pmc <dir> --out <f>              add measured / algorithmic traffic
    python scripts/sparse_bench.py --probe-interleaved <lib> --out <f>      gather option (b) on a measurement build

Algorithmic bytes of one apply: (M+1)*4 + nnz*4 + B*nnz*s + B*P*N*s + B*P*M*s (8 TB/s peak)."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 8e12


def poisson7(n, dev):
    import torch
    N = n ** 3
    ar = torch.arange(N, device=dev)
    z, y, x = ar // (n * n), (ar // n) % n, ar % n
    cols, ok = [], []
    for dz, dy, dx in ((-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0)):
        ok.append((z + dz >= 0) & (z + dz < n) & (y + dy >= 0) & (y + dy < n) & (x + dx >= 0) & (x + dx < n))
        cols.append(ar + dz * n * n + dy * n + dx)
    ok = torch.stack(ok, 1)
    col = torch.stack(cols, 1)[ok].to(torch.int32)
    val = torch.where(col.to(torch.int64) == torch.repeat_interleave(ar, ok.sum(1)), 6.0, -1.0).double()
    crow = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    crow[1:] = torch.cumsum(ok.sum(1), 0)
    return crow, col, val


def random_pattern(N, per_row, dev, seed=0):
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    crow = torch.arange(N + 1, device=dev, dtype=torch.int64) * per_row
    col = torch.randint(0, N, (N * per_row,), generator=g, device=dev, dtype=torch.int32)
    return crow, col


def powerlaw_pattern(N, dev, seed=1):
    """Pareto row lengths 4 (1 - r)^(-1/1.5) (r uniform): mean ~12, a tail up to ~1e5, and one full row"""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    r = torch.rand(N, generator=g, device=dev, dtype=torch.float64)
    lens = (4 * (1 - r).clamp(min=1e-12) ** (-1 / 1.5)).long().clamp(max=N)
    lens[N // 2] = N
    crow = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    crow[1:] = torch.cumsum(lens, 0)
    col = torch.randint(0, N, (int(crow[-1]),), generator=g, device=dev, dtype=torch.int32)
    return crow, col


def _timed(fn, calls, warmup):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def workloads(dev):
    import torch
    crow, col, val = poisson7(256, dev)
    for P in (1, 6, 16):
        yield "poisson7_256^3_P%d" % P, crow, col, val.unsqueeze(0), 1, P
    N = 1 << 22
    crow, col = random_pattern(N, 32, dev)
    g = torch.Generator(device=dev).manual_seed(3)
    for B in (1, 8):
        yield "random32_2^22_B%d" % B, crow, col, torch.randn(B, col.numel(), generator=g, device=dev,
                                                              dtype=torch.float64), B, 1
    N = 1 << 21
    crow, col = powerlaw_pattern(N, dev)
    yield "powerlaw_2^21", crow, col, torch.randn(1, col.numel(), generator=g, device=dev, dtype=torch.float64), 1, 1


def run(args):
    import torch
    from xitorch_amd import kernels as K
    from xitorch_amd.linop import SparseLinearOperator
    from xitorch_amd.linalg._panel import pad_len
    dev = torch.device("cuda:0")
    rec = {"peak_bytes_per_s": HBM, "gather_form": "element gathers straight from the panel vectors (option a)",
           "kernel": [], "solver": []}
    for wi, (name, crow, col, val, B, P) in enumerate(workloads(dev)):
        if args.only is not None and wi != args.only:
            continue
        M = N = crow.numel() - 1
        A = SparseLinearOperator(crow, col, val[0] if val.shape[0] == 1 else val, (M, N))
        pat = A._pattern
        nnz = col.numel()
        X = torch.randn(B, P, pad_len(N), dtype=torch.float64, device=dev)[:, :, :N]
        Y = torch.empty(B, P, pad_len(M), dtype=torch.float64, device=dev)[:, :, :M]
        fn = lambda: K.csr_mm(pat, val, X, out=Y)
        if args.pmc_only:
            fn()
            torch.cuda.synchronize()
            continue
        ms = _timed(fn, args.calls, args.warmup)
        s = 8
        alg = (M + 1) * 4 + nnz * 4 + B * nnz * s + B * P * N * s + B * P * M * s
        row = {"workload": name, "M": M, "nnz": nnz, "B": B, "P": P, "bins": pat.csr().bin_counts,
               "ms": round(ms, 4), "alg_bytes": alg, "TB_s": round(alg / ms / 1e9, 3),
               "frac_of_8TBs": round(alg / (ms * 1e-3) / HBM, 3)}
        if B == 1:
            try:
                S = torch.sparse_csr_tensor(crow, col.to(torch.int64), val[0], (M, N))
                xd = X[0].transpose(0, 1).contiguous()
                tms = _timed(lambda: torch.sparse.mm(S, xd), args.calls, args.warmup)
                row["torch_sparse_mm_ms"] = round(tms, 4)
            except Exception as e:          # recorded, not fatal: the library baseline is optional
                row["torch_sparse_mm"] = "did not run: %s" % str(e).splitlines()[0][:160]
        rec["kernel"].append(row)
        print(json.dumps(row), flush=True)
        del A, pat, X, Y
    if args.pmc_only:
        return
    rec["solver"] = solver_runs(dev)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


def solver_runs(dev):
    import torch
    from xitorch_amd.linop import SparseLinearOperator
    from xitorch_amd.linalg import native_krylov as nk
    out = []
    n = 256
    crow, col, val = poisson7(n, dev)
    A = SparseLinearOperator(crow, col, val, (n ** 3, n ** 3), is_hermitian=True)
    b = torch.ones(n ** 3, 1, dtype=torch.float64, device=dev)
    for phase in ("warm", "timed"):
        tr = {"k1_events": []}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        nk.cg(A, b, rtol=1e-8, atol=0.0, max_niter=5000, trace=tr)
        e1.record()
        e1.synchronize()
    tot = e0.elapsed_time(e1)
    op = sum(a.elapsed_time(z) for a, z, *_ in tr["k1_events"])
    row = {"solver": "cg poisson7 256^3 fp64 rtol 1e-8", "iterations": tr.get("niter"), "ms": round(tot, 2),
           "iterations_per_s": round(tr["niter"] / tot * 1e3, 1), "share_in_csr_mm": round(op / tot, 3)}
    print(json.dumps(row), flush=True)
    out.append(row)
    del A, crow, col, val
    torch.cuda.empty_cache()
    # the closed-form eigenproblem of tests/test_gpu_sparse.py: A = P Q D Q^T P^T at N = 2^22
    from xitorch_amd.linalg.native_eig import davidson
    from tests.test_gpu_sparse import rotated_diagonal, lowest_diagonal_start
    A, d = rotated_diagonal(1 << 22, dev)
    V0 = lowest_diagonal_start(A, 12)
    for phase in ("warm", "timed"):
        tr = {"k1_events": []}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ev, _ = davidson(A, 6, "lowest", min_eps=1e-9, precond="diag", V0=V0, max_niter=200, trace=tr)
        e1.record()
        e1.synchronize()
    tot = e0.elapsed_time(e1)
    op = sum(a.elapsed_time(z) for a, z, *_ in tr["k1_events"])
    row = {"solver": "davidson neig 6, precond diag, lowest-diagonal start, rotated diagonal 2^22 fp64",
           "iterations": tr.get("niter"), "ms": round(tot, 2),
           "iterations_per_s": round(tr["niter"] / tot * 1e3, 1) if tr.get("niter") else None,
           "share_in_csr_mm": round(op / tot, 3), "max_eval_err": float((ev - d[:6]).abs().max())}
    print(json.dumps(row), flush=True)
    out.append(row)
    return out


def probe_interleaved(path, calls, warmup):
    """gather option (b): the panel staged once into an interleaved (N, P) array, every nonzero then fetches P
    contiguous elements.  `path`: a measurement build of the library with -DXK_CSR_PROBE_INTERLEAVED (same ABI, the
    kernel reads X[j*ldx + c]).  Times the staging copy and the apply separately on the 7-point case."""
    import ctypes
    import torch
    from xitorch_amd import _capi, kernels as K
    from xitorch_amd.linop import SparseLinearOperator
    from xitorch_amd.linalg._panel import pad_len
    L = ctypes.CDLL(path)
    f = L.xk_csr_mm_f64
    f.restype, f.argtypes = _capi.lib().xk_csr_mm_f64.restype, _capi.lib().xk_csr_mm_f64.argtypes
    dev = torch.device("cuda:0")
    crow, col, val = poisson7(256, dev)
    N = crow.numel() - 1
    A = SparseLinearOperator(crow, col, val, (N, N))
    v, vals = A._pattern.csr(), val.unsqueeze(0)
    P_ = _capi.ptr
    out = []
    for P in (6, 16):
        X = torch.randn(1, P, pad_len(N), dtype=torch.float64, device=dev)[:, :, :N]
        Yref = K.csr_mm(A._pattern, vals, X)
        Xi = torch.empty(N, P, dtype=torch.float64, device=dev)
        Y = torch.empty(1, P, N, dtype=torch.float64, device=dev)
        stage = lambda: Xi.copy_(X[0].transpose(0, 1))

        def apply():
            rc = f(P_(v.ptr), P_(v.idx), None, P_(vals), 0, P_(v.rows), v.bin_off, None, None, 0, None, P_(Xi),
                   P_(Y), 1, N, N, P, P, 0, N, 0, _capi.stream_ptr())
            _capi.check(rc, "probe xk_csr_mm")
        stage()
        apply()
        ok = bool(torch.allclose(Y, Yref, rtol=1e-13, atol=1e-13))
        row = {"workload": "poisson7_256^3_P%d interleaved (option b)" % P, "same_result": ok,
               "ms_stage": round(_timed(stage, calls, warmup), 4), "ms_apply": round(_timed(apply, calls, warmup), 4),
               "ms_option_a": round(_timed(lambda: K.csr_mm(A._pattern, vals, X, out=Yref), calls, warmup), 4)}
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def merge_pmc(root, out):
    """HBM traffic of each workload's xk_csr_mm launches from separate FETCH_SIZE / WRITE_SIZE passes
    (root/{FETCH_SIZE,WRITE_SIZE}_<i>/.../*counter_collection.csv, one process per workload, --pmc-only --only i),
    against the algorithmic bytes of the timed record.  FETCH_SIZE counts 64 B per L2 read request; gfx950 tallies a
    128-B streaming request as one (MI355X_MICROARCH.md), so the raw figure is a lower bound and twice it an upper
    bound of the bytes read."""
    import glob
    rec = json.load(open(out))
    rows = []

    def total(kind, i):
        fs = glob.glob(os.path.join(root, "%s_%d" % (kind, i), "**", "*counter_collection.csv"), recursive=True)
        if not fs:
            return None
        tot = 0.0
        for r in csv.DictReader(open(fs[0])):
            if "csr_mm" in r["Kernel_Name"]:
                tot += float(r["Counter_Value"]) * 1024
        return tot
    for i, k in enumerate(rec["kernel"]):
        f, w = total("FETCH_SIZE", i), total("WRITE_SIZE", i)
        if f is None or w is None:
            continue
        rows.append({"workload": k["workload"], "alg_bytes": k["alg_bytes"], "fetch_bytes_raw": f, "write_bytes": w,
                     "measured_over_alg_raw": round((f + w) / k["alg_bytes"], 3),
                     "measured_over_alg_fetch_x2": round((2 * f + w) / k["alg_bytes"], 3)})
        print(json.dumps(rows[-1]))
    rec["pmc"] = rows
    json.dump(rec, open(out, "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pmc-only", action="store_true")
    ap.add_argument("--only", type=int, help="run workload number ONLY (0-based), with --pmc-only")
    ap.add_argument("--merge-pmc")
    ap.add_argument("--probe-interleaved", help="measurement build (-DXK_CSR_PROBE_INTERLEAVED) to compare against")
    a = ap.parse_args()
    if a.probe_interleaved:
        rows = probe_interleaved(a.probe_interleaved, a.calls, a.warmup)
        if a.out:
            rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
            rec["gather_option_b_probe"] = rows
            json.dump(rec, open(a.out, "w"), indent=1)
    elif a.merge_pmc:
        merge_pmc(a.merge_pmc, a.out)
    else:
        run(a)
