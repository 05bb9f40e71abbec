"""-m gpu: the LDS-resident parallel Jacobi eigensolver (K3, xk_small_eigh_*) against spectra that are known exactly
(tests/jacobi_cases.py), at every workgroup-size / blocks-per-thread boundary of the kernel, at scales whose squares
leave the floating-point range, with a truncated sweep count, and bit-reproducibly.

K3 has no failure flag and its callers read nothing but lam and Y, so whatever it returns is taken as right: every
bound here is  c k u  times the natural scale, c = 8 x the error of CPU LAPACK in the same precision on the same
matrices (jacobi_cases.LAPACK_RATIO, asserted by test_jacobi_cases.py).

Every call gets T inside a larger NaN-filled allocation (ldt > k, sT > k ldt, nonzero storage offset, NaN strict upper
triangle), a NaN-filled workspace, and NaN / -1 sentinels in lam, Y and sweeps."""
import json
import os
import pytest
import torch
from xitorch_amd import kernels as K
from xitorch_amd._capi import fn
from tests import jacobi_cases as jc

pytestmark = pytest.mark.gpu

F64 = torch.float64
DTYPES = [torch.float64, torch.float32]
NAN = float("nan")
WORST = {}          # (dtype name, quantity) -> worst error in its unit (jacobi_cases.ratios) over this run


def _run(Ts, k, p, uppest, dtype, dev, max_sweeps=16):
    """K3 on the (k, k) float64 matrices Ts (exact in dtype): float64 CPU copies of lam (B, p), Y (B, p, k) and the
    sweep counts, plus the device outputs themselves"""
    B = len(Ts)
    ldt, off = k + 3, 5
    sT = k * ldt + 7
    buf = torch.full((off + B * sT,), NAN, dtype=dtype)
    Tv = buf.as_strided((B, k, k), (sT, ldt, 1), off)
    low = torch.tril(torch.ones(k, k, dtype=torch.bool))
    for b in range(B):
        Tv[b][low] = Ts[b].to(dtype)[low]
    Td = buf.to(dev).as_strided((B, k, k), (sT, ldt, 1), off)
    nws = fn("xk_small_eigh_workspace_elems")(B, k, max_sweeps)
    K._workspace(nws, dtype, dev).fill_(NAN)
    out = (torch.full((B, p), NAN, dtype=dtype, device=dev), torch.full((B, p, k), NAN, dtype=dtype, device=dev),
           torch.full((B,), -1, dtype=torch.int32, device=dev))
    lam, Y, sweeps = K.small_eigh(Td, k, p, uppest=uppest, max_sweeps=max_sweeps, method="jacobi", out=out)
    assert lam.data_ptr() == out[0].data_ptr() and Y.data_ptr() == out[1].data_ptr()
    return lam.cpu().double(), Y.cpu().double(), sweeps.cpu(), (lam, Y, sweeps)


def _check_exact(cases, lam, Y, sweeps, p, uppest, dtype, tag, scale_exp=0):
    """per member: every bound of the module docstring against the exact spectrum; records the worst ratios"""
    for b, c in enumerate(cases):
        t = tag + (b,)
        k = c.T.shape[0]
        assert torch.isfinite(lam[b]).all() and torch.isfinite(Y[b]).all(), t     # a sentinel left = an unwritten entry
        assert 0 <= int(sweeps[b]) < 16, (t, int(sweeps[b]))
        assert bool((lam[b, 1:] >= lam[b, :-1]).all()), t
        lb = torch.ldexp(lam[b], torch.tensor(-scale_exp))                        # exact: back to the unscaled case
        r = jc.ratios(c.T, lb, Y[b], c, p, uppest, dtype)
        for q, v in r.items():
            if v is None:
                continue
            key = (str(dtype).replace("torch.", ""), q)
            WORST[key] = max(WORST.get(key, 0.0), v)
            assert v <= jc.bound_factor(q, dtype), (t, q, v, jc.bound_factor(q, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", jc.ORDERS)
def test_exact_spectra(dev, k, dtype):
    """the four Hadamard families and the trivial matrices, as the batch of one launch, for every wanted count and
    both ends of the spectrum"""
    cases = [jc.case(f, k, dtype) for f in jc.FAMILIES]
    for p in jc.wanted_counts(k):
        for uppest in (False, True):
            lam, Y, sweeps, _ = _run([c.T for c in cases], k, p, uppest, dtype, dev)
            _check_exact(cases, lam, Y, sweeps, p, uppest, dtype, (k, p, uppest))


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_spectra_batch_of_70(dev, dtype):
    """70 distinct members in one launch: more workgroups than one per family, every batch pitch"""
    k = jc.BATCH70_ORDER
    cases = jc.batch70(k, dtype)
    for p, uppest in ((6, False), (16, True)):
        lam, Y, sweeps, _ = _run([c.T for c in cases], k, p, uppest, dtype, dev)
        _check_exact(cases, lam, Y, sweeps, p, uppest, dtype, (k, p, uppest))


@pytest.mark.parametrize("dtype", DTYPES)
def test_early_exit_waits_for_its_certificate(dev, dtype):
    """jacobi_cases.hidden: after the first sweep the p extreme diagonal entries sit on rows without any off-diagonal
    mass, while the extreme eigenvalue is still inside the unconverged block — the early exit may only be taken once
    the Gershgorin bounds of the unwanted rows exclude that"""
    p = jc.HIDDEN_P
    for nb in jc.HIDDEN_BLOCKS:
        for uppest in (False, True):
            c = jc.hidden(nb, dtype, uppest)
            lam, Y, sweeps, _ = _run([c.T], p + nb, p, uppest, dtype, dev)
            _check_exact([c], lam, Y, sweeps, p, uppest, dtype, ("hidden", nb, uppest))
            assert int(sweeps[0]) > 1, (nb, uppest, int(sweeps[0]))       # nothing is resolved after one sweep


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", jc.ORDERS)
def test_generic_dense(dev, k, dtype):
    """(R + R^T) / 2 without a diagonal shift against float64 LAPACK on the rounded matrix, with the constants of
    test_gpu_k1.py::test_small_eigh_vs_oracle"""
    B = 3
    T = jc.generic(B, k, dtype, seed=1000 + k)
    lam_ref = torch.linalg.eigvalsh(T)
    tol = 1e-12 if dtype == F64 else 2e-5
    scale = lam_ref.abs().max().item()
    for p in jc.wanted_counts(k):
        for uppest in (False, True):
            tag = (k, p, uppest)
            sl = slice(k - p, k) if uppest else slice(0, p)
            lam, Y, sweeps, _ = _run(list(T), k, p, uppest, dtype, dev)
            assert torch.isfinite(lam).all() and torch.isfinite(Y).all(), tag
            assert (lam - lam_ref[:, sl]).abs().max().item() < tol * scale * 10, tag
            assert bool((lam[:, 1:] >= lam[:, :-1]).all()), tag
            Yc = Y.transpose(-2, -1)
            res = torch.matmul(T, Yc) - Yc * lam.unsqueeze(-2)
            assert res.abs().max().item() < tol * scale * 50, tag
            G = torch.matmul(Y, Yc)
            assert (G - torch.eye(p, dtype=F64)).abs().max().item() < tol * 100, tag
            assert 0 <= int(sweeps.min()) and int(sweeps.max()) < 16, tag


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", jc.SCALE_ORDERS)
def test_scale(dev, k, dtype):
    """T 2^e with e up to where the squares of the entries (the kernel's norms and thresholds) underflow to zero or
    overflow: the same relative bounds as at e = 0 — no unflagged wrong answer at any scale"""
    fams = ("spread", "cluster")
    cases = [jc.case(f, k, dtype) for f in fams]
    p = min(k, 6)
    for e in jc.SCALE_EXPONENTS[dtype]:
        Ts = [torch.ldexp(c.T, torch.tensor(e)) for c in cases]
        for uppest in (False, True):
            lam, Y, sweeps, _ = _run(Ts, k, p, uppest, dtype, dev)
            _check_exact(cases, lam, Y, sweeps, p, uppest, dtype, ("scale", e, k, p, uppest), scale_exp=e)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [33, 128])
def test_truncated_run(dev, k, dtype):
    """max_sweeps = 2, far from converged: the replayed rotation log must still be the similarity the rotated diagonal
    came from — Y orthonormal, lam[c] = y_c^T T y_c, sweeps = 2"""
    B, p = 3, min(k, 16)
    T = jc.generic(B, k, dtype, seed=2000 + k)
    ku = k * jc.unit_roundoff(dtype)
    nrm = max(torch.linalg.eigvalsh(T).abs().max().item(), 1.0)
    for uppest in (False, True):
        lam, Y, sweeps, _ = _run(list(T), k, p, uppest, dtype, dev, max_sweeps=2)
        assert sweeps.tolist() == [2] * B, sweeps
        assert torch.isfinite(lam).all() and torch.isfinite(Y).all()
        assert bool((lam[:, 1:] >= lam[:, :-1]).all())
        G = torch.matmul(Y, Y.transpose(-2, -1))
        orth = (G - torch.eye(p, dtype=F64)).abs().max().item() / ku
        rq = torch.einsum("bci,bij,bcj->bc", Y, T, Y)
        ray = (lam - rq).abs().max().item() / (ku * nrm)
        for q, v in (("orth", orth), ("lam", ray)):
            key = (str(dtype).replace("torch.", ""), "truncated " + q)
            WORST[key] = max(WORST.get(key, 0.0), v)
            assert v <= jc.bound_factor(q, dtype), (k, uppest, q, v)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [5, 45, 128])
def test_two_calls_give_equal_bits(dev, k, dtype):
    cases = [jc.case(f, k, dtype) for f in jc.FAMILIES] + [jc.Case(T, None, None, None) for T in jc.generic(2, k, dtype, 3000 + k)]
    p = min(k, 6)
    a = _run([c.T for c in cases], k, p, False, dtype, dev)[3]
    b = _run([c.T for c in cases], k, p, False, dtype, dev)[3]
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_zz_worst_ratios():
    """the kernel's worst error per (dtype, quantity) of this run, in the units of jacobi_cases.ratios, next to its
    bound; written as JSON where XK_JACOBI_WORST_JSON points"""
    rep = {"%s/%s" % k: v for k, v in sorted(WORST.items())}
    print("jacobi kernel worst ratios:", json.dumps(rep))
    print("bounds:", json.dumps({"%s/%s" % (str(d).replace("torch.", ""), q): jc.bound_factor(q, d)
                                 for q in jc.LAPACK_RATIO for d in DTYPES}))
    path = os.environ.get("XK_JACOBI_WORST_JSON")
    if path:
        with open(path, "w") as f:
            json.dump(rep, f, indent=1)
    for (dt, q), v in WORST.items():
        assert v <= jc.bound_factor(q.split()[-1], getattr(torch, dt)), (dt, q, v)
