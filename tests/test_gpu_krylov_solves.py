"""-m gpu: native cg / bicgstab in the dtypes and sizes the golden cases do not reach.

* float32 / complex64 (Hermitian and not, with and without E / M, a resid_calc_every refresh) against a
  float64 / complex128 dense solve, and against the oracle run in the SAME dtype: same convergence flag, iteration
  count within a small slack.
* all four dtypes on dense operators of order 5000, where kry_blocks() picks 2..63 blocks per system, and on an
  implicit tridiagonal operator of order 300 000, beyond the 64-block cap, against a known float64 / complex128
  solution.

Error bounds: a solve stopped at |r| < rtol |b| is within cond(A) * |r| / |b| of the exact solution in the relative
2-norm; on top of that the recurrence residual may drift from the true one by a few hundred roundings of |A||x| over
the iterations, hence |x - x*| <= cond * (2 rtol + 200 u) |x*| per column."""
import math
import warnings
import pytest
import torch
import xitorch_amd as xa
from oracle import ops as oops, solve as osolve
from tests import krylov_ref as kref
from xitorch_amd.linalg import native_krylov as nk

pytestmark = pytest.mark.gpu

HP = kref.HP_OF
U = kref.unit_roundoff
ITER_SLACK = lambda n: 2 + n // 10      # native vs oracle iteration counts in the same dtype (different roundings)


def _crand(g, shape, dtype):
    x = torch.randn(shape, dtype=torch.float64, generator=g)
    if dtype.is_complex:
        x = torch.complex(x, torch.randn(shape, dtype=torch.float64, generator=g)) / math.sqrt(2)
    return x


def _crand_dev(g, shape, dtype, dev):
    x = torch.randn(shape, dtype=torch.float64, device=dev, generator=g)
    if dtype.is_complex:
        x = torch.complex(x, torch.randn(shape, dtype=torch.float64, device=dev, generator=g)) / math.sqrt(2)
    return x


def _col_err_bound(Ahp, Mhp, E, Xref, rtol, dtype):
    """cond(A - e_c M) * (2 rtol + 200 u) * |x*_c| per column (dense, small orders)"""
    out = []
    for c in range(Xref.shape[-1]):
        Ac = Ahp if E is None else Ahp - (Mhp if Mhp is not None else torch.eye(Ahp.shape[-1], dtype=Ahp.dtype)) \
            * E[..., c].unsqueeze(-1).unsqueeze(-1)
        cond = torch.linalg.cond(Ac)
        out.append(cond * (2 * rtol + 200 * U(dtype)) * Xref[..., c].norm(dim=-1))
    return torch.stack(out, -1)


SMALL = [  # method, Hermitian A, E, M, resid_calc_every
    ("cg", True, False, False, 10), ("cg", True, True, True, 10), ("cg", True, True, False, 3),
    ("bicgstab", False, False, False, 10), ("bicgstab", False, True, False, 10), ("bicgstab", False, True, True, 3),
    ("bicgstab", True, False, False, 10),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.complex64], ids=["f32", "c64"])
@pytest.mark.parametrize("method,herm,withE,withM,rce", SMALL,
                         ids=["%s-%s%s%s-rce%d" % (m, "H" if h else "G", "E" if e else "", "M" if mm else "", r)
                              for m, h, e, mm, r in SMALL])
def test_single_precision_solve_vs_dense_and_same_dtype_oracle(dev, dtype, method, herm, withE, withM, rce):
    g = torch.Generator().manual_seed(7 * SMALL.index((method, herm, withE, withM, rce)) + int(dtype.is_complex))
    n, batch, nc = 200, 2, 3
    W = _crand(g, (batch, n, n), dtype) / math.sqrt(n)
    if herm:
        W = (W + W.transpose(-2, -1).conj()) / 2
    A = 2 * torch.eye(n, dtype=W.dtype) + 0.3 * W
    B = _crand(g, (batch, n, nc), dtype)
    M = E = None
    if withM:
        V = _crand(g, (n, n), dtype) / math.sqrt(n)
        M = torch.eye(n, dtype=V.dtype) + 0.05 * (V + V.transpose(-2, -1).conj())
    if withE:
        # CG: real, negative shifts keep A - E M Hermitian positive definite; BiCGStab: complex shifts when complex
        E = -(0.1 + 0.4 * torch.rand(nc, dtype=torch.float64, generator=g))
        if dtype.is_complex and method == "bicgstab":
            E = E * torch.polar(torch.ones(nc, dtype=torch.float64), torch.rand(nc, dtype=torch.float64, generator=g))
        E = E.to(HP[dtype])
    rtol, atol = 1e-5, 1e-8
    lo = lambda t: None if t is None else t.to(dtype)
    Al, Bl, El, Ml = lo(A), lo(B), lo(E), lo(M)
    opts = dict(posdef=True, rtol=rtol, atol=atol, resid_calc_every=rce)
    tr = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        X = getattr(nk, method)(xa.LinearOperator.m(Al.to(dev), is_hermitian=herm), Bl.to(dev),
                                El.to(dev) if El is not None else None,
                                xa.LinearOperator.m(Ml.to(dev), is_hermitian=True) if Ml is not None else None,
                                trace=tr, **opts)
    assert X.dtype == dtype and X.shape == (batch, n, nc)
    # the dense solution of the problem as stored in the kernel dtype, in float64 / complex128
    h = lambda t: None if t is None else t.to(HP[dtype])
    Ah, Bh, Eh, Mh = h(Al), h(Bl), h(El), h(Ml)
    Xref = osolve.exactsolve(oops.DenseOp(Ah, herm), Bh, Eh, oops.DenseOp(Mh, True) if Mh is not None else None)
    err = (X.cpu().to(HP[dtype]) - Xref).norm(dim=-2)
    bound = _col_err_bound(Ah, Mh, Eh, Xref, rtol, dtype)
    assert bool((err <= bound).all()), (err / bound).max().item()
    # the oracle in the same dtype: same convergence, about the same number of iterations
    tro = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        getattr(osolve, method)(oops.DenseOp(Al, herm), Bl, El, oops.DenseOp(Ml, True) if Ml is not None else None,
                                trace=tro, **opts)
    assert tr["converged"] and tro["converged"]
    assert abs(tr["niter"] - tro["niter"]) <= ITER_SLACK(tro["niter"]), (tr["niter"], tro["niter"])


DTYPES = [torch.float64, torch.float32, torch.complex128, torch.complex64]
IDS = ["f64", "f32", "c128", "c64"]
RTOL = {torch.float64: 1e-10, torch.float32: 1e-5, torch.complex128: 1e-10, torch.complex64: 1e-5}


def _nblk(N, dtype):
    return max(1, min(64, -(-N // (1024 * kref.VEC_ELEMS[dtype]))))


def _check_known(X, Xs, cond, rtol, dtype):
    err = (X.to(HP[dtype]) - Xs).norm(dim=-2)
    bound = cond * (2 * rtol + 200 * U(dtype)) * Xs.norm(dim=-2)
    assert bool((err <= bound).all()), (err / bound).max().item()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_multi_block_dense_solve(dev, dtype, method):
    """order 5000: 2..63 blocks per system (f64 3, f32 2, c128 5, c64 3).  A = 2 I + 0.3 W with W = G / sqrt(n)
    (Hermitian part of it for cg): |W| < 2.5 with overwhelming probability, so cond(A) <= 2.75 / 1.25 = 2.2."""
    n, nc = 5000, 2
    assert 2 <= _nblk(n, dtype) <= 63
    g = torch.Generator(device=dev).manual_seed(5000 + DTYPES.index(dtype))
    hd = HP[dtype]
    W = _crand_dev(g, (n, n), dtype, dev) / math.sqrt(n)
    if method == "cg":
        W = (W + W.transpose(-2, -1).conj()) / 2
    A = (2 * torch.eye(n, dtype=hd, device=dev) + 0.3 * W).to(dtype)
    Xs = _crand_dev(g, (n, nc), dtype, dev)
    # B from the STORED matrix: the exact solution of the stored problem differs from Xs by B's rounding only,
    # |dx| <= cond * u |x|, well inside the bound
    B = (A.to(hd) @ Xs).to(dtype)
    del W
    rtol = RTOL[dtype]
    tr = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        X = getattr(nk, method)(xa.LinearOperator.m(A, is_hermitian=(method == "cg")), B, posdef=True, rtol=rtol,
                                atol=1e-30, trace=tr)
    assert tr["converged"]
    _check_known(X, Xs, 2.2, rtol, dtype)


class _Tridiag(xa.LinearOperator):
    """implicit tridiagonal operator in torch ops: (A x)_i = lo x_{i-1} + d x_i + up x_{i+1}"""

    def __init__(self, n, d, up, lo, dtype, device, hermitian):
        super().__init__((n, n), is_hermitian=hermitian, dtype=dtype, device=device)
        self.d, self.up, self.lo = d, up, lo

    def _mv(self, x):
        y = self.d * x
        y[..., :-1] += self.up * x[..., 1:]
        y[..., 1:] += self.lo * x[..., :-1]
        return y

    def _getparamnames(self, prefix=""):
        return []


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_above_the_block_cap_tridiagonal_solve(dev, dtype, method):
    """order 300 000: more than 64 * 1024 vectors per system in every dtype, so nblk is capped at 64 and one block
    covers more than 1024 vectors.  d = 4, |up| + |lo| = o < 2: cond <= (4 + o) / (4 - o) (|A - 4 I|_2 <= o)."""
    n, nc = 300000, 2
    assert _nblk(n, dtype) == 64 and -(-n // kref.VEC_ELEMS[dtype]) > 64 * 1024
    if dtype.is_complex:
        up = -1.0 * complex(math.cos(0.7), math.sin(0.7))
        lo = up.conjugate() if method == "cg" else complex(-0.5, 0.3)
    else:
        up, lo = -1.0, (-1.0 if method == "cg" else -0.5)
    o = abs(up) + abs(lo)
    cond = (4 + o) / (4 - o)
    g = torch.Generator(device=dev).manual_seed(300000 + DTYPES.index(dtype))
    hd = HP[dtype]
    Xs = _crand_dev(g, (n, nc), dtype, dev)
    Ahp = _Tridiag(n, 4.0, up, lo, hd, dev, method == "cg")
    B = Ahp.mm(Xs).to(dtype)
    A = _Tridiag(n, 4.0, up, lo, dtype, dev, method == "cg")
    rtol = RTOL[dtype]
    tr = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        X = getattr(nk, method)(A, B, posdef=True, rtol=rtol, atol=1e-30, trace=tr)
    assert tr["converged"]
    # the exact solution of the stored problem differs from Xs by B's rounding: |dx| <= cond * u |x|, inside the bound
    _check_known(X, Xs, cond, rtol, dtype)
    r = (Ahp.mm(X.to(hd)) - B.to(hd)).norm(dim=-2)
    assert bool((r <= (2 * rtol + 200 * U(dtype)) * B.to(hd).norm(dim=-2)).all())
