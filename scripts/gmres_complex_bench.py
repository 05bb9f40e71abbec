"""Measurements of the complex GMRES -> profiles/gmres_complex.json.  One process, a warm-up, HIP event
timing, three repeats, the spread reported.

  1. complex128 against real fp64 per Arnoldi step at basis widths 8 / 32 / 128, at equal bytes: complex order N against
     real order 2 N, the same S, the cheapest operator there is (a diagonal one, in CSR) so that the basis work
     dominates.  Both run one `restart=width` cycle of exactly `width` steps (rtol = 0 never stops them).
  2. achieved fraction of HBM of xk_gmres_gram_c128 at width 128 from the byte formula (kq N + N) * 16 B per system,
     next to the real K1 Gram product on the same bytes.
  3. the Helmholtz CSR case: iterations, applies and time of gmres(restart=40) and of complex bicgstab.

    python scripts/gmres_complex_bench.py [--out profiles/gmres_complex.json] [--n 1048576] [--s 4]
"""
import argparse
import json
import os
import sys
import warnings
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import xitorch_amd as xa                                           # noqa: E402
from xitorch_amd import kernels as K                               # noqa: E402
from xitorch_amd.linalg import solve                               # noqa: E402

DEV = torch.device("cuda:0")
HBM_PEAK = 8.0e12                                                  # B/s, MI355X


def timed(f, repeats=3):
    f()                                                            # warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e-3)
    return out


def diag_operator(n, dtype, S):
    idx = torch.arange(n, dtype=torch.int32, device=DEV)
    crow = torch.arange(n + 1, dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(1)
    vals = (1.0 + torch.rand(S, n, generator=g, dtype=torch.float64)).to(dtype).to(DEV)
    if dtype.is_complex:
        vals = vals * (1.0 + 0.3j)
    return xa.SparseLinearOperator(crow, idx, vals, (S, n, n), is_hermitian=False)


def per_step(dtype, n, S, width):
    A = diag_operator(n, dtype, S)
    g = torch.Generator().manual_seed(2)
    B = torch.randn(S, n, 1, generator=g, dtype=torch.float64).to(dtype).to(DEV)
    tr = {}

    def run():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            solve(A, B, method="gmres", posdef=True, rtol=0.0, atol=0.0, restart=width, max_niter=width + 1,
                  resid_calc_every=width, trace=tr)
    ts = timed(run)
    return dict(dtype=str(dtype), n=n, S=S, width=width, steps=tr["arnoldi_steps"], seconds=ts,
                per_step_us=[t / tr["arnoldi_steps"] * 1e6 for t in ts])


def gram_fraction(n, S, kq):
    torch.manual_seed(3)
    Q = torch.randn(S, kq + 1, n, dtype=torch.complex128, device=DEV)
    c = torch.zeros(S, kq + 2, dtype=torch.complex128, device=DEV)
    scr = torch.zeros(S * K.gmres_gram_tiles(n, torch.complex128) * (kq + 1) * 2, dtype=torch.float64, device=DEV)
    ts = timed(lambda: K.gmres_gram_c(Q, Q[:, kq], c, scr, kq, n))
    nbytes = S * (kq * n + n) * 16
    del Q
    Qr = torch.randn(S, kq + 1, 2 * n, dtype=torch.float64, device=DEV)
    tr_ = timed(lambda: K.dense_mm(Qr[:, :kq + 1], Qr[:, kq:kq + 1]))
    rbytes = S * ((kq + 1) * 2 * n + 2 * n) * 8
    return dict(n=n, S=S, kq=kq, complex_seconds=ts, complex_bytes=nbytes,
                complex_fraction_of_hbm=[nbytes / t / HBM_PEAK for t in ts],
                real_k1_seconds=tr_, real_k1_bytes=rbytes, real_k1_fraction_of_hbm=[rbytes / t / HBM_PEAK for t in tr_])


def helmholtz(n=64, k2=0.9, eta=0.3):
    idx = torch.arange(n ** 3).reshape(n, n, n)
    rows, cols, vals = [idx.reshape(-1)], [idx.reshape(-1)], [torch.full((n ** 3,), 6.0)]
    for d in range(3):
        a, b = idx.narrow(d, 0, n - 1).reshape(-1), idx.narrow(d, 1, n - 1).reshape(-1)
        rows += [a, b]
        cols += [b, a]
        vals += [torch.full((a.numel(),), -1.0)] * 2
    t = torch.sparse_coo_tensor(torch.stack([torch.cat(rows), torch.cat(cols)]), torch.cat(vals).to(torch.complex128),
                                (n ** 3, n ** 3)).coalesce().to_sparse_csr()
    A = xa.SparseLinearOperator(t.crow_indices().to(DEV), t.col_indices().to(DEV), t.values().to(DEV), tuple(t.shape),
                                is_hermitian=True)
    g = torch.Generator().manual_seed(4)
    B = torch.complex(torch.randn(n ** 3, 1, generator=g, dtype=torch.float64),
                      torch.randn(n ** 3, 1, generator=g, dtype=torch.float64)).to(DEV)
    E = torch.tensor([complex(k2, eta)], dtype=torch.complex128, device=DEV)
    out = {}
    for meth, kw in (("gmres", dict(restart=40, max_niter=20000)), ("bicgstab", dict(max_niter=20000))):
        tr = {}

        def run():
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                solve(A, B, E, method=meth, posdef=True, rtol=1e-8, atol=1e-30, trace=tr, **kw)
        ts = timed(run)
        out[meth] = dict(n=n ** 3, converged=tr["converged"], niter=tr["niter"], napply=tr["napply"],
                         best_resid=tr["best_resid"], seconds=ts)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/gmres_complex.json")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--s", type=int, default=4)
    args = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), per_step=[], note="three timed repeats after one warm-up each")
    for width in (8, 32, 128):
        c = per_step(torch.complex128, args.n, args.s, width)
        r = per_step(torch.float64, 2 * args.n, args.s, width)
        ratio = [a / b for a, b in zip(sorted(c["seconds"]), sorted(r["seconds"]))]
        res["per_step"].append(dict(width=width, complex128=c, float64=r, ratio_sorted_repeats=ratio))
        print(json.dumps(res["per_step"][-1]), flush=True)
    res["gram"] = gram_fraction(args.n, args.s, 128)
    print(json.dumps(res["gram"]), flush=True)
    res["helmholtz"] = helmholtz()
    print(json.dumps(res["helmholtz"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
