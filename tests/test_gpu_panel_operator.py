"""-m gpu: the shared rectangular panel operator (linalg/_panel.py::RectPanelOperator), forward and adjoint, on every
storage kind it classifies, against the operator's `.mm` / `.rmm` evaluated in float64 / complex128 on the host.

Shapes 7x5, 5x7 (swapped in / out lengths) and 6x6; two batch members with one shared or two own operators; 1 and 3
columns.  No length is a multiple of 8, so every panel row has pad elements: they must stay zero.  Every entry is held
to the standard dot-product bound |fl(sum a_j x_j) - sum a_j x_j| <= (n + 2) eps (|A| |x|)_i with n the contraction
length and eps that of the operator's dtype (derived, e.g. Higham, Accuracy and Stability, section 3.1; eps = 2 u leaves
the factor the complex products need), the right-hand side computed in float64."""
import pytest
import torch
from xitorch_amd import LinearOperator
from xitorch_amd.linop import SparseLinearOperator, BandedLinearOperator
from xitorch_amd.linalg._panel import RectPanelOperator, PanelOperator, pad_len

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = [torch.float64, torch.float32, torch.complex128, torch.complex64]
IDS = ["f64", "f32", "c128", "c64"]
SHAPES = [(7, 5), (5, 7), (6, 6)]
BT = 2
HB = 2                                      # half bandwidth of the banded case
# storage -> (kind, flip, cj) the classifier must report
STORAGES = {"dense": ("dense", False, False), "dense_T": ("dense", True, False), "dense_conj": ("dense", False, True),
            "dense_H": ("dense", True, True), "dense_2d": ("dense", False, False), "banded": ("banded", False, False),
            "csr": ("csr", False, False), "generic": ("generic", False, False)}


def _hp(dtype):
    return torch.complex128 if dtype.is_complex else torch.float64


def _randn(g, dtype, *shape):
    """random numbers of the working precision (host)"""
    return torch.randn(*shape, dtype=_hp(dtype), generator=g).to(dtype)


class _Generic(LinearOperator):
    """a user operator with only _mv / _rmv"""

    def __init__(self, mat):
        super().__init__(shape=mat.shape, dtype=mat.dtype, device=mat.device)
        self.mat = mat

    def _mv(self, x):
        return torch.matmul(self.mat, x.unsqueeze(-1)).squeeze(-1)

    def _rmv(self, x):
        return torch.matmul(self.mat.transpose(-2, -1).conj(), x.unsqueeze(-1)).squeeze(-1)

    def _getparamnames(self, prefix=""):
        return [prefix + "mat"]


def _build(storage, g, dtype, nA, m, n):
    """-> (operator on the device, its matrices (nA, m, n) in float64 / complex128 on the host)"""
    if storage == "dense":
        A = _randn(g, dtype, nA, m, n)
        return LinearOperator.m(A.to(DEV)), A.to(_hp(dtype))
    if storage == "dense_2d":
        A = _randn(g, dtype, m, n)
        return LinearOperator.m(A.to(DEV)), A.to(_hp(dtype)).unsqueeze(0)
    if storage in ("dense_T", "dense_conj", "dense_H"):
        base = _randn(g, dtype, nA, n, m) if storage != "dense_conj" else _randn(g, dtype, nA, m, n)
        view = {"dense_T": lambda t: t.transpose(-2, -1), "dense_conj": lambda t: t.conj(),
                "dense_H": lambda t: t.transpose(-2, -1).conj()}[storage]
        mat = view(base.to(DEV))
        assert not mat.is_contiguous() or mat.is_conj()
        return LinearOperator.m(mat), view(base).resolve_conj().to(_hp(dtype))
    if storage == "banded":
        band = _randn(g, dtype, nA, 2 * HB + 1, n)
        A = torch.zeros(nA, n, n, dtype=_hp(dtype))
        for i in range(n):
            for j in range(max(0, i - HB), min(n, i + HB + 1)):
                A[:, i, j] = band[:, j - i + HB, i]
        return BandedLinearOperator(band.to(DEV)), A
    if storage == "csr":
        mask = torch.rand(m, n, generator=g) < 0.5
        mask[0, :] = False                                      # an empty row, a full row
        mask[1, :] = True
        A = _randn(g, dtype, nA, m, n) * mask
        crow = torch.cat([torch.zeros(1, dtype=torch.int64), mask.sum(-1).cumsum(0)])
        cols = torch.nonzero(mask)[:, 1]
        vals = A[:, mask]                                        # (nA, nnz), row-major like the pattern
        if nA == 1:
            op = SparseLinearOperator(crow.to(DEV), cols.to(DEV), vals[0].to(DEV), (m, n))
        else:
            op = SparseLinearOperator(crow.to(DEV), cols.to(DEV), vals.to(DEV), (nA, m, n))
        return op, A.to(_hp(dtype))
    A = _randn(g, dtype, nA, m, n)
    return _Generic(A.to(DEV)), A.to(_hp(dtype))


def _cases():
    out = []
    for storage in STORAGES:
        for (m, n) in SHAPES:
            for dtype, did in zip(DTYPES, IDS):
                for nA in (1, 2):
                    if storage in ("dense_conj", "dense_H") and not dtype.is_complex:
                        continue
                    if storage == "banded" and (m != n or dtype.is_complex):
                        continue                                # (banded operators are square; the kernel is real)
                    if storage == "dense_2d" and nA != 1:
                        continue
                    out.append(pytest.param(storage, m, n, dtype, nA, id="%s-%dx%d-%s-nA%d" % (storage, m, n, did, nA)))
    return out


@pytest.mark.parametrize("storage,m,n,dtype,nA", _cases())
def test_rect_panel_apply(storage, m, n, dtype, nA):
    g = torch.Generator().manual_seed(1000 * m + 10 * n + nA + len(storage))
    A, Ahp = _build(storage, g, dtype, nA, m, n)
    kind, flip, cj = STORAGES[storage]
    op = RectPanelOperator(A, [BT], BT)
    assert (op.kind, op.m, op.n) == (kind, m, n)
    if kind == "dense":
        assert (op.flip, op.cj) == (flip, cj)
    assert PanelOperator(A, [BT], BT, n).kind == kind              # the square operator classifies alike
    ref_op = LinearOperator.m(Ahp.expand(BT, m, n).contiguous(), is_hermitian=False)      # host, float64 / complex128
    eps = torch.finfo(dtype).eps
    applies = 0
    for p in (1, 3):
        for trans in (False, True):
            nin, nout = (m, n) if trans else (n, m)
            x = _randn(g, dtype, BT, nin, p)
            X = torch.zeros(BT, p, pad_len(nin), dtype=dtype, device=DEV)
            X[:, :, :nin] = x.transpose(-2, -1).to(DEV)
            out = torch.zeros(BT, p, pad_len(nout), dtype=dtype, device=DEV)
            out[:, :, :nout] = 7.0                                  # the apply overwrites, it does not accumulate
            assert op.apply(X, out, trans) is out
            applies += 1
            xh = x.to(_hp(dtype))
            ref = ref_op.rmm(xh) if trans else ref_op.mm(xh)       # (BT, nout, p)
            absA = Ahp.abs().expand(BT, m, n)
            scale = torch.matmul(absA.transpose(-2, -1) if trans else absA, xh.abs())
            got = out.cpu()
            assert bool((got[:, :, nout:] == 0).all()), "pad columns of out written"
            assert bool((X.cpu()[:, :, nin:] == 0).all())
            err = (got[:, :, :nout].transpose(-2, -1).to(_hp(dtype)) - ref).abs()
            bound = (nin + 2) * eps * scale
            worst = float((err - bound).max())
            print("%s p=%d trans=%s: max err %.3e, max bound %.3e" % (storage, p, trans, float(err.max()),
                                                                     float(bound.max())))
            assert bool((err <= bound).all()), (p, trans, worst)
    assert op.napply == applies and op.torch_applies == (applies if kind == "generic" else 0)
