"""Record of the complex Hermitian block Davidson (native_eig_herm.py) on the MI355X: median ms per call, iterations,
operator products, the operator product's HBM rate, and device exacteig (torch.linalg.eigh) on the same batch.

    python scripts/herm_davidson_bench.py --out profiles/herm_davidson.json            timed record (HIP events)
    python scripts/herm_davidson_bench.py --calls 1 --warmup 0 --out <f>                 one call per workload (profiler)
    python scripts/herm_davidson_bench.py --merge-stats <kernel_stats.csv> --out <f>     add the time split of a
                                                                                        rocprofv3 --kernel-trace --stats run

Workloads: 16 operators of order 8192 (17.2 GB) and 64 of order 2048, complex128, lowest 6 pairs, min_eps 1e-8."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = [(16, 8192), (64, 2048)]
NEIG, MIN_EPS, HBM = 6, 1e-8, 8e12


def _operator(B, N, dev):
    """A = Q diag(d) Q^H, Q a product of three Householder reflectors (closed-form spectrum), built on the device"""
    import torch
    g = torch.Generator(device=dev).manual_seed(N)
    d = torch.linspace(-1.0, 1.0, N, dtype=torch.float64, device=dev)
    d[:NEIG] = torch.tensor([-5.0, -4.3, -3.7, -3.2, -2.8, -2.5], dtype=torch.float64, device=dev)
    A = torch.diag_embed(d.to(torch.complex128)).unsqueeze(0).repeat(B, 1, 1)
    for _ in range(3):
        u = torch.randn(B, N, 1, dtype=torch.complex128, device=dev, generator=g)
        u = u / torch.linalg.vector_norm(u, dim=-2, keepdim=True)
        A -= 2 * torch.matmul(u, torch.matmul(u.transpose(-2, -1).conj(), A))
        A -= 2 * torch.matmul(torch.matmul(A, u), u.transpose(-2, -1).conj())
    A = (A + A.transpose(-2, -1).conj()) * 0.5
    return A, d


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
    return ts[len(ts) // 2], ts


def run(args):
    import torch
    import xitorch_amd as xa
    from xitorch_amd.linalg.native_eig import davidson
    from xitorch_amd.linalg._panel import PanelOperator
    assert torch.cuda.is_available(), "this record needs a HIP device"
    dev = torch.device("cuda:0")
    rec = {"what": "complex128 Hermitian block Davidson (native_eig_herm.py), lowest %d pairs, min_eps %g" % (NEIG, MIN_EPS),
           "device": torch.cuda.get_device_name(0), "workloads": []}
    for B, N in WORKLOADS:
        A, d = _operator(B, N, dev)
        op = xa.LinearOperator.m(A, is_hermitian=True)
        tr = {}
        with torch.no_grad():
            lam, _ = davidson(op, NEIG, "lowest", min_eps=MIN_EPS, trace=tr)
        err = (lam - d[:NEIG]).abs().max().item()
        ms, all_ms = _timed(lambda: davidson(op, NEIG, "lowest", min_eps=MIN_EPS), args.calls, args.warmup)
        # the operator product alone (2p real columns over the (N, 2N) interleaved matrix), timed the same way
        pop = PanelOperator(op, [B], B, N)
        X = torch.randn(B, NEIG, N, dtype=torch.complex128, device=dev)
        Y = torch.empty_like(X)
        prod_ms, _ = _timed(lambda: pop.apply(X, Y), max(args.calls, 5), args.warmup)
        op_bytes = B * N * N * 16
        ex_ms, _ = _timed(lambda: torch.linalg.eigh(A), 2, min(args.warmup, 1))
        rec["workloads"].append({
            "B": B, "N": N, "operator_bytes_per_product": op_bytes, "median_ms_per_call": ms, "ms_per_call": all_ms,
            "niter": tr["niter"], "napply": tr["napply"], "basis_size": tr["basis_size"], "rr_native": tr["rr_native"],
            "rr_library": tr["rr_library"], "max_abs_eval_error": err,
            "operator_product_ms": prod_ms, "operator_product_hbm_fraction": op_bytes / (prod_ms * 1e-3) / HBM,
            "exacteig_device_ms": ex_ms})
        print(json.dumps(rec["workloads"][-1]), flush=True)
        del A, op, pop
        torch.cuda.empty_cache()
    return rec


def merge_stats(rec, path):
    """time split by kernel family from rocprofv3's kernel_stats.csv (one profiled call per workload plus set-up)"""
    split = {"k1_products": 0.0, "chain": 0.0, "rayleigh_ritz": 0.0, "other": 0.0}
    with open(path) as f:
        for row in csv.DictReader(f):
            name, ns = row.get("Name", ""), float(row.get("TotalDurationNs", 0) or 0)
            if "herm_eigh" in name:
                split["rayleigh_ritz"] += ns
            elif "herm_ritz" in name or "herm_gram" in name or "herm_cholqr" in name:
                split["chain"] += ns
            elif "dense" in name or "wide" in name:
                split["k1_products"] += ns
            else:
                split["other"] += ns
    rec["rocprof_split_ms"] = {k: v * 1e-6 for k, v in split.items()}
    rec["rocprof_note"] = ("one profiled run of both workloads (one call each, plus the timed operator products and "
                           "eigh of that run): K1 products include the tall Gram / projection products")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "herm_davidson.json"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--merge-stats", default=None)
    args = ap.parse_args()
    if args.merge_stats:
        rec = json.load(open(args.out))
        rec = merge_stats(rec, args.merge_stats)
    else:
        rec = run(args)
        rec["date"] = time.strftime("%Y-%m-%d")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
