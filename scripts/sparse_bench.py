"""Record of the CSR operator (xk_csr_mm) on the MI355X: kernel time and HBM fraction on algorithmic bytes by
workload, torch.sparse.mm on the same CSR where it runs, and cg on the 7-point Poisson problem with the share of time
spent in the operator product.

    python scripts/sparse_bench.py --out profiles/csr_mm.json             timed record (HIP events)
    python scripts/sparse_bench.py --pmc-only --only I                      one launch of workload I, for
                                                                            rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE
    python scripts/sparse_bench.py --merge-pmc <dir> --out <f>              add measured / algorithmic traffic
    python scripts/sparse_bench.py --probe-interleaved <lib> --out <f>      gather option (b) on a measurement build
    python scripts/sparse_bench.py --dtype c128 --dtype c64 --out profiles/csr_mm_complex.json
                                                                            complex values: the native apply against
                                                                            the torch expression (csr_apply_torch, what
                                                                            a complex operator ran before the complex
                                                                            kernels) and torch.sparse.mm, same process
    python scripts/sparse_bench.py --davidson native|torch-expression       one complex davidson call, for
                                                                            rocprofv3 --kernel-trace --stats

Algorithmic bytes of one apply: (M+1)*4 + nnz*4 + B*nnz*s + B*P*N*s + B*P*M*s (8 TB/s peak), s = 8 / 16 / 8 bytes
for f64 / c128 / c64."""
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


DTYPES = {"f64": ("float64", 8), "c128": ("complex128", 16), "c64": ("complex64", 8)}


def _randn(shape, g, dev, dtype):
    import torch
    if dtype.is_complex:
        return torch.view_as_complex(torch.randn(*shape, 2, generator=g, device=dev, dtype=torch.float64)).to(dtype)
    return torch.randn(*shape, generator=g, device=dev, dtype=torch.float64).to(dtype)


def phase_poisson7(n, dev, dtype):
    """the 7-point operator with a complex phase on every hop (Peierls phases of a uniform field): Hermitian,
    diagonal 6, hop (i -> j) = -exp(i theta_ij), theta_ji = -theta_ij"""
    import torch
    crow, col, val = poisson7(n, dev)
    N = n ** 3
    rows = torch.repeat_interleave(torch.arange(N, device=dev), (crow[1:] - crow[:-1]))
    d = col.to(torch.int64) - rows
    theta = 0.05 * torch.sign(d).double() * ((rows + col.to(torch.int64)) % n).double()      # antisymmetric in (i, j)
    v = torch.where(d == 0, torch.full_like(theta, 6.0).to(torch.complex128), -torch.exp(1j * theta))
    return crow, col, v.to(dtype)


def workloads(dev, dtype_name="f64"):
    import torch
    dtype = getattr(torch, DTYPES[dtype_name][0])
    if dtype.is_complex:
        crow, col, val = phase_poisson7(256, dev, dtype)
    else:
        crow, col, val = poisson7(256, dev)
    for P in (1, 6, 16):
        yield "poisson7_256^3_P%d" % P, crow, col, val.unsqueeze(0), 1, P
    if dtype.is_complex:
        yield "poisson7_256^3_P6_B8", crow, col, val.unsqueeze(0).repeat(8, 1), 8, 6
    N = 1 << 22
    crow, col = random_pattern(N, 32, dev)
    g = torch.Generator(device=dev).manual_seed(3)
    for B in (1, 8):
        yield "random32_2^22_B%d" % B, crow, col, _randn((B, col.numel()), g, dev, dtype), B, 1
    N = 1 << 21
    crow, col = powerlaw_pattern(N, dev)
    yield "powerlaw_2^21", crow, col, _randn((1, col.numel()), g, dev, dtype), 1, 1


def run(args):
    import torch
    from xitorch_amd import kernels as K
    from xitorch_amd.linop import SparseLinearOperator
    from xitorch_amd.linalg._panel import pad_len
    dev = torch.device("cuda:0")
    rec = {"peak_bytes_per_s": HBM, "gather_form": "element gathers straight from the panel vectors (option a)",
           "kernel": [], "solver": []}
    dtypes = args.dtype or ["f64"]
    gx = torch.Generator(device=dev).manual_seed(11)
    for dtype_name in dtypes:
        run_dtype(args, rec, dev, dtype_name, gx)
    if args.pmc_only:
        return
    if dtypes == ["f64"]:
        rec["solver"] = solver_runs(dev)
    else:
        rec["device"] = torch.cuda.get_device_name(0)
        rec["method"] = ("HIP events around one call, median of %d after %d warm-up calls, one process, nothing "
                         "else running on the device" % (args.calls, args.warmup))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


def run_dtype(args, rec, dev, dtype_name, gx):
    import torch
    from xitorch_amd import kernels as K
    from xitorch_amd.linop import SparseLinearOperator, csr_apply_torch
    from xitorch_amd.linalg._panel import pad_len
    dtype, s = getattr(torch, DTYPES[dtype_name][0]), DTYPES[dtype_name][1]
    for wi, (name, crow, col, val, B, P) in enumerate(workloads(dev, dtype_name)):
        if args.only is not None and wi != args.only:
            continue
        M = N = crow.numel() - 1
        A = SparseLinearOperator(crow, col, val[0] if val.shape[0] == 1 else val, (M, N))
        pat = A._pattern
        nnz = col.numel()
        X = _randn((B, P, pad_len(N)), gx, dev, dtype)[:, :, :N]
        Y = torch.empty(B, P, pad_len(M), dtype=dtype, device=dev)[:, :, :M]
        fn = lambda: K.csr_mm(pat, val, X, out=Y)
        if args.pmc_only:
            fn()
            torch.cuda.synchronize()
            continue
        ms = _timed(fn, args.calls, args.warmup)
        alg = (M + 1) * 4 + nnz * 4 + B * nnz * s + B * P * N * s + B * P * M * s
        row = {"workload": name, "dtype": dtype_name, "M": M, "nnz": nnz, "B": B, "P": P, "bins": pat.csr().bin_counts,
               "ms": round(ms, 4), "alg_bytes": alg, "TB_s": round(alg / ms / 1e9, 3),
               "frac_of_8TBs": round(alg / (ms * 1e-3) / HBM, 3)}
        if B == 1:
            try:
                S = torch.sparse_csr_tensor(crow, col.to(torch.int64), val[0], (M, N))
                xd = X[0].transpose(0, 1).contiguous()
                tms = _timed(lambda: torch.sparse.mm(S, xd), args.calls, args.warmup)
                row["torch_sparse_mm_ms"] = round(tms, 4)
                del S, xd
            except Exception as e:          # recorded, not fatal: the library baseline is optional
                row["torch_sparse_mm"] = "did not run: %s" % str(e).splitlines()[0][:160]
        if dtype.is_complex:
            # the path a complex operator took before the complex kernels: the torch expression on the (N, P) view of
            # the same panel, result copied back into the panel (what PanelOperator's generic branch does)
            xv = X.transpose(1, 2)
            vals = val[0] if val.shape[0] == 1 else val

            def torch_expr():
                y = csr_apply_torch(crow, col, vals, xv, M, N, False, row_of=pat.row_of)
                Y.copy_(y.transpose(1, 2))
            row["torch_expr_temp_bytes"] = B * nnz * P * s
            try:
                tms = _timed(torch_expr, max(3, args.calls // 4), 1)
                row["torch_expr_ms"] = round(tms, 4)
                row["native_over_torch_expr"] = round(ms / tms, 4)
            except Exception as e:          # out of memory: the (B, nnz, P) temporary does not fit
                row["torch_expr"] = "did not run: %s" % str(e).splitlines()[0][:160]
            torch.cuda.empty_cache()
        rec["kernel"].append(row)
        print(json.dumps(row), flush=True)
        del A, pat, X, Y


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


def davidson_run(which, n=128, neig=6, niter=40):
    """One complex128 davidson call (lowest `neig` of the complex-phase 7-point operator on an n^3 grid, `niter`
    iterations, no stopping before) for a kernel trace.  which = "native": the SparseLinearOperator as it is;
    "torch-expression": the same operator applied by csr_apply_torch through the generic panel branch, the path
    complex CSR operators took before the complex kernels."""
    import time
    import torch
    from xitorch_amd.linop import LinearOperator, SparseLinearOperator, csr_apply_torch
    from xitorch_amd.linalg.native_eig import davidson
    dev = torch.device("cuda:0")
    crow, col, val = phase_poisson7(n, dev, torch.complex128)
    N = n ** 3
    A = SparseLinearOperator(crow, col, val, (N, N), is_hermitian=True)
    if which != "native":
        pat = A._pattern

        class TorchExpression(LinearOperator):
            def __init__(self):
                super().__init__((N, N), is_hermitian=True, dtype=val.dtype, device=val.device)

            def _mv(self, x):
                return self._mm(x.unsqueeze(-1)).squeeze(-1)

            def _mm(self, x):
                return csr_apply_torch(pat.crow, pat.col, val, x, N, N, False, row_of=pat.row_of)

            def _getparamnames(self, prefix=""):
                return []
        A = TorchExpression()
    out = None
    for phase in ("warm", "timed"):
        tr = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev, _ = davidson(A, neig, "lowest", min_eps=0.0, max_niter=niter, trace=tr)
        torch.cuda.synchronize()
        out = {"solver": "davidson lowest %d, complex-phase 7-point %d^3 c128, %d iterations" % (neig, n, niter),
               "operator": which, "panel_kernel": tr["panel_kernel"], "napply": tr["napply"],
               "ms": round((time.perf_counter() - t0) * 1e3, 2), "lowest": float(ev.min())}
    print(json.dumps(out), flush=True)
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
    ap.add_argument("--dtype", action="append", choices=sorted(DTYPES),
                    help="value type of the timed record (repeatable; default f64)")
    ap.add_argument("--davidson", choices=["native", "torch-expression"],
                    help="one complex128 davidson call on the complex-phase 7-point operator, nothing else")
    a = ap.parse_args()
    if a.davidson:
        row = davidson_run(a.davidson)
        if a.out:
            rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
            rec.setdefault("solver", []).append(row)
            json.dump(rec, open(a.out, "w"), indent=1)
    elif a.probe_interleaved:
        rows = probe_interleaved(a.probe_interleaved, a.calls, a.warmup)
        if a.out:
            rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
            rec["gather_option_b_probe"] = rows
            json.dump(rec, open(a.out, "w"), indent=1)
    elif a.merge_pmc:
        merge_pmc(a.merge_pmc, a.out)
    else:
        run(a)
