"""-m gpu: xk_gkl_sweep_{f64,f32,c128,c64}, xk_gkl_finish and xk_gkl_bsvd per entry against tests/gkl_ref.py.

sweep: the basis and the vector live in NaN-filled buffers with NaN pads [N, ld) and NaN margins — what the kernel must
not read would poison the result, what it must not write is compared bit for bit.  N below / at / above the chunk of
every dtype (64 .. 256 elements) and the 16 B vector, several chunks (4099), j = 0, 1, 5, 63 (both register tilings and
the row cap), Bt = 1 and 3, the aligned pitch (vector form) and a base one element into its buffer (scalar form), the
null-coefficient pass, a scale, dst apart from w, a repeat call (bit-identical).  The bounds are gkl_ref's, in units of
the sum lengths.  bsvd: orders 2, 3, 17, 64; arrow + bidiagonal, graded, zero and repeated-value matrices; Bt = 1 and 5;
both sort orders; residual estimates, status word and the restart matrix."""
import numpy as np
import pytest
import torch
from tests import gkl_ref as gref
from xitorch_amd import kernels as K
from xitorch_amd.linalg._panel import pad_len

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.float64, torch.float32, torch.complex128, torch.complex64]
IDS = ["f64", "f32", "c128", "c64"]
NPDT = {torch.float64: np.float64, torch.float32: np.float32, torch.complex128: np.complex128,
        torch.complex64: np.complex64}
NS = [1, 7, 255, 256, 257, 1027, 4099]
JS = [0, 1, 5, 63]
MARGIN = 64
XK_ERR_ARG = -1


def _bits(t):
    t = t.detach().cpu().contiguous()
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _randn(rng, shape, dtype):
    x = rng.standard_normal(shape)
    if dtype.is_complex:
        x = x + 1j * rng.standard_normal(shape)
    return torch.from_numpy(np.asarray(x).astype(NPDT[dtype]))


class _Buf:
    """a (Bt, rows, ld) view `off` elements past MARGIN into a NaN-filled flat buffer; [:N] of every row = host"""

    def __init__(self, host, ld, off=0):
        Bt, rows, N = host.shape
        self.N = N
        n = Bt * rows * ld
        self.buf = torch.full((2 * MARGIN + off + n,), float("nan"), dtype=host.dtype, device=DEV)
        self.view = self.buf[MARGIN + off:MARGIN + off + n].view(Bt, rows, ld)
        self.view[:, :, :N] = host.to(DEV)
        self.before = self.buf.clone()

    def unchanged(self):
        return torch.equal(_bits(self.buf), _bits(self.before))

    def outside_unchanged(self, row):
        """everything but [:N] of `row` of every member is bit-identical to what it was"""
        now, was = self.buf.clone(), self.before.clone()
        for t in (now, was):
            v = t[self.view.storage_offset():self.view.storage_offset() + self.view.numel()].view(self.view.shape)
            v[:, row, :self.N] = 0
        return torch.equal(_bits(now), _bits(was))


def _check_sweep(dtype, Bt, N, j, off=0, with_coef=True, scale=False, inplace=True, seed=0):
    rng = np.random.default_rng(1000 * seed + 17 * N + j + Bt)
    ld = pad_len(N)
    cap = j + 1
    Qh = _randn(rng, (Bt, cap, N), dtype)                       # row j is the new vector when in place
    Qb = _Buf(Qh, ld, off)
    if inplace:
        w = dst = Qb.view[:, j]
        wb = None
    else:
        wb = _Buf(Qh[:, j:j + 1].clone(), ld, off)
        db = _Buf(torch.zeros_like(Qh[:, j:j + 1]), ld, off)
        w, dst = wb.view[:, 0], db.view[:, 0]
    ncf = 2 * j if dtype.is_complex else j
    coef = None
    if with_coef and j > 0:
        coef = torch.from_numpy(rng.standard_normal((Bt, max(ncf, 1)))).to(DEV)
    sc = torch.from_numpy(rng.uniform(0.5, 2.0, (Bt,))).to(DEV) if scale else None
    nchunk, nval = K.gkl_chunks(N, dtype), K.gkl_nval(j, dtype)
    assert nchunk == (N + gref.chunk_elems(NPDT[dtype]) - 1) // gref.chunk_elems(NPDT[dtype])
    part = torch.full((Bt * nval * nchunk + 5,), float("nan"), dtype=torch.float64, device=DEV)
    K.gkl_sweep(Qb.view, j, w, dst, coef, sc, part, N)
    torch.cuda.synchronize()
    got = dst[:, :N].cpu().numpy()
    gpart = part[:Bt * nval * nchunk].cpu().numpy().reshape(Bt, nval, nchunk)
    assert torch.isnan(part[Bt * nval * nchunk:]).all()           # nothing beyond the partials of this call
    Qn = Qh.numpy()
    for b in range(Bt):
        cf = None
        if coef is not None:
            c = coef[b].cpu().numpy()
            cf = c[0:2 * j:2] + 1j * c[1:2 * j:2] if dtype.is_complex else c[:j]
        ref, bound, rpart, pbound = gref.sweep(Qn[b], Qn[b, j], cf, None if sc is None else float(sc[b]), j, N,
                                               NPDT[dtype])
        err = np.abs(got[b].astype(ref.dtype) - ref)
        # (a stored value may sit one rounding away from the restated one: both are within `bound` of the exact one)
        assert (err <= 2 * bound + 1e-300).all(), (b, float((err / (bound + 1e-300)).max()))
        perr = np.abs(gpart[b] - rpart)
        assert (perr <= 2 * pbound + 1e-300).all(), (b, float((perr / (pbound + 1e-300)).max()))
    if inplace:
        assert Qb.outside_unchanged(j)
    else:
        assert Qb.unchanged() and wb.unchanged() and db.outside_unchanged(0)
    return Qb, dst, part


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", NS)
def test_sweep_lengths(dtype, N):
    """every N at j = 5, Bt = 3, with coefficients, in place (the driver's call)"""
    _check_sweep(dtype, 3, N, 5)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("j", JS)
@pytest.mark.parametrize("Bt", [1, 3])
def test_sweep_rows_and_batch(dtype, j, Bt):
    _check_sweep(dtype, Bt, 1027, j, seed=1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", [7, 257, 1027])
def test_sweep_scalar_form(dtype, N):
    """a base pointer one element into its buffer breaks the 16 B rule: element-by-element form, same contract"""
    _check_sweep(dtype, 3, N, 5, off=1, seed=2)
    _check_sweep(dtype, 1, N, 63, off=1, seed=3)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_sweep_null_coefficients_scale_and_separate_dst(dtype):
    _check_sweep(dtype, 3, 1027, 5, with_coef=False, seed=4)                 # first pass of CGS2: accumulate only
    _check_sweep(dtype, 3, 1027, 0, with_coef=False, scale=True, seed=5)     # the normalising store
    _check_sweep(dtype, 3, 257, 17, scale=True, inplace=False, seed=6)       # dst apart from w


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_sweep_repeat_is_bit_identical(dtype):
    rng = np.random.default_rng(5)
    Bt, N, j = 3, 4099, 21
    ld = pad_len(N)
    Q = torch.zeros((Bt, j, ld), dtype=dtype, device=DEV)
    Q[:, :, :N] = _randn(rng, (Bt, j, N), dtype).to(DEV)
    w = torch.zeros((Bt, ld), dtype=dtype, device=DEV)
    w[:, :N] = _randn(rng, (Bt, N), dtype).to(DEV)
    coef = torch.from_numpy(rng.standard_normal((Bt, 2 * j))).to(DEV)
    outs = []
    for _ in range(2):
        dst = torch.zeros_like(w)
        part = torch.zeros((Bt * K.gkl_nval(j, dtype) * K.gkl_chunks(N, dtype),), dtype=torch.float64, device=DEV)
        K.gkl_sweep(Q, j, w, dst, coef, None, part, N)
        outs.append((dst.clone(), part.clone()))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))


def test_finish_sums_flags_and_stores():
    rng = np.random.default_rng(9)
    Bt, nval, nchunk = 3, 11, 133
    part = rng.standard_normal((Bt, nval, nchunk))
    part[:, -1] = np.abs(part[:, -1])
    part[1, -1] = 1e-40                                                   # member 1 breaks down against smax = 1
    dpart = torch.from_numpy(part).to(DEV)
    coef = torch.full((Bt, 16), float("nan"), dtype=torch.float64, device=DEV)
    nrm = torch.zeros((Bt,), dtype=torch.float64, device=DEV)
    rnrm = torch.zeros_like(nrm)
    Bm = torch.full((Bt, 4, 4), 7.0, dtype=torch.float64, device=DEV)
    smax = torch.ones((Bt,), dtype=torch.float64, device=DEV)
    brk = torch.tensor([-1, -1, 5], dtype=torch.int32, device=DEV)
    K.gkl_finish(dpart.reshape(-1), Bt, nval, nchunk, coef, nrm, rnrm, dst=Bm[:, 2, 3], smax=smax, u=2.0 ** -53,
                 brk=brk, code=9)
    ref_sum = part.sum(axis=-1)
    bound = (nchunk + 8) * gref.U64 * np.abs(part).sum(axis=-1)
    assert (np.abs(coef[:, :nval - 1].cpu().numpy() - ref_sum[:, :-1]) <= bound[:, :-1]).all()
    assert torch.isnan(coef[:, nval - 1:]).all()
    norm = np.sqrt(ref_sum[:, -1])
    got = nrm.cpu().numpy()
    assert abs(got[0] - norm[0]) <= 4 * gref.U64 * norm[0] + bound[0, -1] and got[1] == 0.0
    assert abs(got[2] - norm[2]) <= 4 * gref.U64 * norm[2] + bound[2, -1]
    assert rnrm[1].item() == 0.0 and abs(rnrm[0].item() * got[0] - 1.0) <= 4 * gref.U64
    assert brk.tolist() == [-1, 9, 5]                                     # first breakdown only; others untouched
    ref_B = torch.full((Bt, 4, 4), 7.0, dtype=torch.float64)
    ref_B[:, 2, 3] = torch.from_numpy(got)
    assert torch.equal(Bm.cpu(), ref_B)
    assert smax.tolist() == [max(1.0, got[0]), 1.0, max(1.0, got[2])]


CASES = gref.projected_cases()


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("Bt", [1, 5])
@pytest.mark.parametrize("descending", [True, False], ids=["uppest", "lowest"])
def test_bsvd(name, Bt, descending):
    B0 = CASES[name]
    n = B0.shape[0]
    scales = np.array([1.0, 0.5, 2.0, 1e-3, 7.0])[:Bt]
    Bs = np.stack([B0 * s for s in scales])
    beta = np.linspace(0.3, 1.1, Bt)
    k, keep = max(1, n // 4), max(1, n // 2) if n > 2 else 1
    Bm = torch.from_numpy(Bs).to(DEV).contiguous()
    Bnext = torch.full_like(Bm, float("nan"))
    brk = torch.arange(-1, Bt - 1, dtype=torch.int32, device=DEV)
    tol = 1e-3
    sigma, P, Q, res, status = K.gkl_bsvd(Bm, torch.from_numpy(beta).to(DEV), None, brk, k=k, keep=keep,
                                          descending=descending, tol=tol, Bnext=Bnext)
    sigma, P, Q, res, status, Bnext = (t.cpu().numpy() for t in (sigma, P, Q, res, status, Bnext))
    eye = np.eye(n)
    for b in range(Bt):
        ref = np.linalg.svd(Bs[b], compute_uv=False)
        if not descending:
            ref = ref[::-1]
        sweeps = int(status[b, 1])
        bound = gref.jacobi_bound(Bs[b], sweeps) + 4 * n * gref.U64 * ref.max()      # (+ the library's own error)
        assert status[b, 2] == 0 and 1 <= sweeps <= 40 and status[b, 3] == b - 1
        assert (np.abs(sigma[b] - ref) <= bound).all(), (name, b, float(np.abs(sigma[b] - ref).max() / bound))
        order = np.diff(sigma[b])
        assert (order <= 0).all() if descending else (order >= 0).all()
        obound = gref.jacobi_bound(np.eye(n), sweeps) * 4
        assert np.abs(P[b].T @ P[b] - eye).max() <= obound and np.abs(Q[b].T @ Q[b] - eye).max() <= obound
        assert np.abs((P[b] * sigma[b]) @ Q[b].T - Bs[b]).max() <= 2 * bound
        rho = beta[b] * P[b, n - 1, :]
        assert np.array_equal(res[b], np.abs(rho))
        assert status[b, 0] == int((res[b, :k] <= tol * sigma[b].max()).sum())
        nxt = np.zeros((n, n))
        nxt[np.arange(keep), np.arange(keep)] = sigma[b, :keep]
        nxt[:keep, keep] = rho[:keep]
        assert np.array_equal(Bnext[b], nxt)


def test_argument_refusals_launch_nothing():
    w = torch.zeros((2, 64), dtype=torch.float64, device=DEV)
    Q = torch.zeros((2, 4, 64), dtype=torch.float64, device=DEV)
    part = torch.full((2 * 5 * 1,), float("nan"), dtype=torch.float64, device=DEV)
    assert K.gkl_sweep(Q, 4, w, w, None, None, part[:3], 64, raw=True) == XK_ERR_ARG          # short partials
    assert K.gkl_sweep(Q, 3, w, Q[:, 1], None, None, part, 64, raw=True) == XK_ERR_ARG         # dst inside rows [0, j)
    assert K.gkl_sweep(Q, 4, w, w[:, 8:], None, None, part, 56, raw=True) == XK_ERR_ARG        # dst overlaps w
    assert torch.isnan(part).all()
    Bm = torch.zeros((1, 4, 4), dtype=torch.float64, device=DEV)
    assert K.gkl_bsvd(Bm, k=5, raw=True) == XK_ERR_ARG
    assert K.gkl_bsvd(Bm, k=1, keep=4, Bnext=torch.zeros_like(Bm), raw=True) == XK_ERR_ARG
