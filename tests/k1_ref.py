"""Float64 / complex128 reference of the K1 operator-panel products, exact and graded inputs, driver-like strided
layouts and a per-entry checker, for tests/test_gpu_k1_contract.py (the kernels) and tests/test_k1_ref.py (the proof,
on the CPU, that the checker rejects plausible kernel faults).

    Y[b, c, :] = A_b X[b, c, :]        (trans = False)        Y[b, c, :] = A_b^T X[b, c, :]      (trans = True)

Panels are panel-major (B, P, n), like everywhere in xitorch_amd.kernels.

Input families (`make_inputs`)
  integer    entries uniform in -8 .. 8.  Every product and partial sum is an integer below 64 * n, exactly
             representable in fp32 for 64 n < 2^24 (asserted: `assert_exact`) and in fp64 always, whatever the summation
             order, FMA or MFMA: the result must equal the reference BIT FOR BIT.
  onehot     X[b, c, :] is a unit vector at index e_c (`edge_indices`: tile, slab and split edges) and A[i, j] holds the
             code i * W + j (W = 4096, or the row length where that is longer; the largest code is asserted below 2^24).
             The output NAMES the element that was read.  Exact.
  graded     randn with rows and / or columns scaled by logspace(-6, 6): only a per-entry bound sees the small rows.
  cancelling panel columns projected so that the true product is about 1e-6 of mag = |A| |X| (needs a contraction longer
             than the output: skinny Gram shapes for A X, tall operators for A^T X).  The bound is in terms of mag.
  symmetric  `symm=True` with any family: exactly symmetric (the upper triangle mirrored).

Per-entry bound (`check`):  |Y - ref| <= C_TOL * u * (terms + levels) * mag, u the unit roundoff of the kernel dtype.
C_TOL = 8 is the constant of tests/krylov_ref.py and tests/davidson_ref.py, with their justification: a sum of n
products accumulated in any order has |err| <= gamma_n sum|terms| (Higham, Accuracy and Stability, 3.1), a reduction
tree or a fixed-order fold of d partials adds d to n, and for the fp64 kernels the fp64 reference carries its own
rounding of the same order, which at most doubles the first-order error: 8 leaves a factor of two above both.  It is
not tuned to what the kernels give.  For complex results the modulus of the error of the two real sums is bounded by
sqrt(2) times the real bound (|Re a||Re x| + |Im a||Im x| <= |a||x|).

`form_terms` gives (terms, levels) per kernel form, read off the sources:
  rows         dense_mm_rows: lane l accumulates VN elements per step of 64 VN columns in one register:
               VN * ceil(n / (64 VN)) terms; wave_reduce_scatter 6 levels; fold_splits adds nsplit partials
               (choose_nsplit, the largest over the row counts R = 4 .. 16)
  rows_scalar  dense_mm_rows_scalar: one element per lane per step of 64: ceil(n / 64) terms, 6 levels
  cols         dense_rmm_cols: one register walks the rows of a slab: rows_per_slab terms, fold_slabs adds nslab
               partials.  The slab count shrinks to what the workspace holds, so the bound takes the rows of the
               fewest slabs (the workspace's count) and the levels of the most (the dtype's count).
  cols_scalar  dense_rmm_cols_scalar: the whole column in one register: n terms
  every other form (K1w, K1wr, K1s, K1sw, the complex wrapper): the full contraction length n (2 n real terms + 2 for
               the complex wrapper), valid for any summation order (gamma_n) at the price of tightness.
"""
import math
import torch

from tests.davidson_ref import C_TOL, _choose_nsplit

VEC_ELEMS = {torch.float64: 2, torch.float32: 4, torch.complex128: 2, torch.complex64: 4}   # of the REAL kernels
REAL_OF = {torch.float64: torch.float64, torch.float32: torch.float32,
           torch.complex128: torch.float64, torch.complex64: torch.float32}
CODE_W = 4096
FAMILIES = ("integer", "onehot", "graded", "cancelling")

# worst |kernel - reference| / bound seen by check(), per (kernel dtype, form) (reported by the GPU runs)
WORST = {}


def unit_roundoff(dtype):
    return torch.finfo(REAL_OF[dtype]).eps / 2


def hp(t):
    t = t.detach().cpu()
    return t.to(torch.complex128 if t.is_complex() else torch.float64)


def pad_len(n):
    """the drivers' padded panel length (xitorch_amd.linalg._panel.pad_len)"""
    return (n + 7) // 8 * 8


def assert_exact(dtype, contraction, amax=8):
    """refuse an `integer` case whose partial sums could leave the exactly representable integers"""
    if REAL_OF[dtype] == torch.float32:
        assert amax * amax * contraction < 2 ** 24, "integer family: %d n = %d is not exact in fp32" % (amax * amax,
                                                                                                      contraction)


# ------------------------------------------------------------------------------------------------ reference
def _op3(A):
    A = hp(A)
    return A if A.dim() == 3 else A.unsqueeze(0)


def mirror_upper(A):
    """the exactly symmetric matrix whose upper triangle (diagonal included) is that of A; the rest of A is never read"""
    up = torch.ones(A.shape[-2:], dtype=torch.bool).triu()
    U = torch.where(up, A, torch.zeros_like(A))
    return U + torch.where(up.triu(1), A, torch.zeros_like(A)).transpose(-2, -1)


def ref_mm(A, X, trans, symm=False):
    """(ref, mag): ref[b, c, :] = op(A_b) X[b, c, :] in float64 / complex128 from plain torch.matmul on the logical
    arrays, op = A or A^T (no conjugation: see `ref_mm_complex`), and mag = |A| |X| per entry.  `symm`: only the upper
    triangle of A is read and mirrored, so a poisoned lower triangle cannot reach the reference."""
    A3, Xh = _op3(A), hp(X)
    if symm:
        A3 = mirror_upper(A3)
    op = A3.transpose(-2, -1) if trans else A3
    ref = torch.matmul(Xh, op.transpose(-2, -1))
    mag = torch.matmul(Xh.abs(), op.abs().transpose(-2, -1))
    return ref, mag


def ref_mm_complex(A, X, adjoint, conj_io):
    """kernels.dense_mm_complex: op = A^H (adjoint) or A, conjugated when conj_io (conj(op conj x) = conj(op) x)"""
    A3, Xh = _op3(A), hp(X)
    op = A3.transpose(-2, -1).conj() if adjoint else A3
    if conj_io:
        op = op.conj()
    op = op.resolve_conj()
    return torch.matmul(Xh, op.transpose(-2, -1)), torch.matmul(Xh.abs(), op.abs().transpose(-2, -1))


# ------------------------------------------------------------------------------------------------ term counts
def cols_slabs(dtype, B, M, N):
    """replica of the slab choice of xk_dense.hip rmm_cols_p / xk_dense_mm_workspace_elems for an (M, N) operator:
    (fewest slabs = the workspace's count, most slabs = the dtype's own count)"""
    vn = VEC_ELEMS[dtype]
    out = []
    for tile in (512, 256 * vn):
        ct = (N + tile - 1) // tile
        out.append(max(1, min((2048 + B * ct - 1) // (B * ct), (M + 63) // 64)))
    return min(out), max(out)


def form_terms(form, dtype, B, M, N, trans):
    """(terms, levels) of the bound for `form` on a (B, M, N) operator (the module docstring says where each comes
    from).  Unknown forms get the full contraction length."""
    vn = VEC_ELEMS[dtype]
    n = M if trans else N
    if form == "rows":
        ns = max(_choose_nsplit(B, M, N, R, vn) for R in (4, 8, 12, 16))
        return vn * ((N + 64 * vn - 1) // (64 * vn)), 6 + ns
    if form == "rows_scalar":
        return (N + 63) // 64, 6
    if form == "cols":
        lo, hi = cols_slabs(dtype, B, M, N)
        return (M + lo - 1) // lo, hi
    if dtype.is_complex:
        return 2 * n + 2, 0
    return n, 0


# ------------------------------------------------------------------------------------------------ checking
def check(Y, ref, mag, dtype, terms, levels=0, exact=False, what="", form=None):
    """Compare a kernel result with the reference.  exact (integer / onehot inputs): `torch.equal` with the reference
    cast to the dtype, no bound at all.  Otherwise per entry |Y - ref| <= C_TOL u (terms + levels) mag (times sqrt 2 for
    complex results); a non-finite kernel value is out of bounds.  Raises AssertionError naming the first entry;
    returns the worst error / bound ratio (0 for exact) and records it in WORST[(dtype, form)]."""
    Yc = Y.detach().cpu()
    assert Yc.shape == ref.shape, "%s: shape %s, want %s" % (what, tuple(Yc.shape), tuple(ref.shape))
    if exact:
        want = ref.to(dtype)
        assert torch.equal(want.to(ref.dtype), ref), "%s: the reference is not representable in %s" % (what, dtype)
        if not torch.equal(Yc, want):
            bad = (Yc != want) | torch.isnan(Yc.real if Yc.is_complex() else Yc)
            idx = bad.nonzero()[0].tolist()
            raise AssertionError("%s: not exact at %s: got %r, want %r (%d entries differ)"
                                 % (what, idx, Yc[tuple(idx)].item(), want[tuple(idx)].item(), int(bad.sum())))
        worst = 0.0
    else:
        bnd = C_TOL * unit_roundoff(dtype) * (terms + levels) * mag * (math.sqrt(2.0) if dtype.is_complex else 1.0)
        err = (hp(Yc) - ref).abs()
        err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
        ok = err <= bnd
        if not bool(ok.all()):
            idx = (~ok).nonzero()[0].tolist()
            raise AssertionError("%s: out of bounds at %s: got %r, want %r, |err| %.3e > bound %.3e (%d entries)"
                                 % (what, idx, Yc[tuple(idx)].item(), ref[tuple(idx)].item(), err[tuple(idx)].item(),
                                    bnd[tuple(idx)].item(), int((~ok).sum())))
        nz = bnd > 0
        worst = float((err[nz] / bnd[nz]).max()) if bool(nz.any()) else 0.0
    key = (str(dtype).replace("torch.", ""), form or what.split(" ")[0])
    WORST[key] = max(WORST.get(key, 0.0), worst)
    return worst


def normwise_ok(Y, ref, dtype, n):
    """the criterion of tests/test_gpu_k1.py: max|Y - ref| / max|ref| < tol sqrt(n), tol = 1e-13 (fp64) / 3e-6 (fp32)"""
    tol = 1e-13 if REAL_OF[dtype] == torch.float64 else 3e-6
    e = (hp(Y) - ref).abs().max().item()
    return e == e and e / (ref.abs().max().item() + 1e-300) < tol * max(1.0, float(n) ** 0.5)


# ------------------------------------------------------------------------------------------------ inputs
def edge_indices(n, dtype):
    """indices of a contraction / output range of length n that sit on tile, slab and split edges of the K1 kernels"""
    vn = VEC_ELEMS[dtype]
    c = {0, 1, vn - 1, vn, 63, 64, 65, 64 * vn - 1, 64 * vn, 255, 256, 256 * vn - 1, 256 * vn, 511, 512, 1023, 1024, 2047,
         2048, 4095, 4096, 8 * 64 * vn - 1, 8 * 64 * vn, n // 2, n - vn - 1, n - vn, n - 2, n - 1,
         (n - 1) // (64 * vn) * (64 * vn), (n - 1) // 64 * 64, (n - 1) // 4 * 4}
    return sorted(i for i in c if 0 <= i < n)


def _randint(g, *shape):
    return torch.randint(-8, 9, shape, generator=g).to(torch.float64)


def _randn(g, dtype, *shape):
    if dtype.is_complex:
        return torch.complex(torch.randn(*shape, dtype=torch.float64, generator=g),
                             torch.randn(*shape, dtype=torch.float64, generator=g))
    return torch.randn(*shape, dtype=torch.float64, generator=g)


def make_inputs(family, g, dtype, Ba, B, M, N, P, trans, symm=False, seed_edge=0):
    """logical (A, X) of `family` in the kernel dtype on the CPU: A (Ba, M, N) (Ba = B or 1), X (B, P, n_in).
    symm: M == N and A exactly symmetric.  Values are generated in float64 and rounded to dtype once."""
    nin = M if trans else N
    cplx = dtype.is_complex
    if family == "integer":
        assert_exact(dtype, (2 if cplx else 1) * nin)
        A, X = _randint(g, Ba, M, N), _randint(g, B, P, nin)
        if cplx:
            A, X = torch.complex(A, _randint(g, Ba, M, N)), torch.complex(X, _randint(g, B, P, nin))
    elif family == "onehot":
        W = max(CODE_W, N)
        assert (M - 1) * W + N - 1 < 2 ** 24, "onehot code of a %d x %d operator is not exact in fp32" % (M, N)
        i, j = torch.arange(M, dtype=torch.float64).view(M, 1), torch.arange(N, dtype=torch.float64).view(1, N)
        A = (i * W + j + 1).expand(Ba, M, N).clone()                         # + 1: element (0, 0) is not a zero
        A = A + torch.arange(Ba, dtype=torch.float64).view(Ba, 1, 1) * 0     # (members differ through X's indices)
        X = torch.zeros(B, P, nin, dtype=torch.float64)
        e = edge_indices(nin, dtype)
        for b in range(B):
            for c in range(P):
                X[b, c, e[(seed_edge + b * P + c) % len(e)]] = 1.0
        if cplx:
            A, X = torch.complex(A, -A), torch.complex(X, torch.zeros_like(X))
    elif family in ("graded", "cancelling"):
        A, X = _randn(g, dtype, Ba, M, N), _randn(g, dtype, B, P, nin)
        if family == "graded":
            lo, hi = (-3, 3) if symm else (-6, 6)
            A = A * torch.logspace(lo, hi, M, dtype=torch.float64).view(1, M, 1)
            if symm or seed_edge % 2:
                A = A * torch.logspace(hi, lo, N, dtype=torch.float64)[torch.randperm(N, generator=g)].view(1, 1, N)
        else:
            op = A.transpose(-2, -1) if trans else A                          # (Ba, n_out, n_in)
            assert op.shape[-2] < op.shape[-1], "cancelling needs a contraction longer than the output"
            Xr = X.to(dtype).to(A.dtype)
            opr = op.to(dtype).to(A.dtype).expand(B, *op.shape[-2:])
            y = torch.matmul(opr, Xr.transpose(-2, -1))                       # (B, n_out, P)
            corr = torch.linalg.lstsq(opr, y).solution                         # minimum-norm x with op x = y
            X = Xr - (1.0 - 1e-6) * corr.transpose(-2, -1)
    else:
        raise ValueError(family)
    if symm:
        assert M == N
        A = mirror_upper(A)
        assert torch.equal(A, A.transpose(-2, -1))
    A, X = A.to(dtype), X.to(dtype)
    if symm:
        assert torch.equal(A, A.transpose(-2, -1))
    return A, X


def is_exact(family):
    return family in ("integer", "onehot")


# ------------------------------------------------------------------------------------------------ layouts
class Placed:
    """a logical array inside a larger sentinel-filled buffer: `.view` (what the kernel gets), `.buf` (the whole flat
    allocation) and the geometry of the view inside it"""

    def __init__(self, buf, shape, strides, offset, squeeze):
        self.buf, self.shape, self.strides, self.offset, self.squeeze = buf, tuple(shape), tuple(strides), offset, squeeze

    def of(self, buf):
        v = torch.as_strided(buf, self.shape, self.strides, self.offset)
        return v[0] if self.squeeze else v

    @property
    def view(self):
        return self.of(self.buf)

    def outside_untouched(self, before):
        """every byte of the buffer outside the logical array equals what `before` (a clone taken before the call) held"""
        a = self.buf.clone()
        self.of(a).copy_(self.of(before))
        ra = torch.view_as_real(a) if a.is_complex() else a
        rb = torch.view_as_real(before) if before.is_complex() else before
        it = torch.int64 if ra.element_size() == 8 else torch.int32
        return torch.equal(ra.view(it), rb.view(it))


# name -> (row pitch, batch pitch, leading rows r0, element offset of the base pointer)
#   row pitch:   "n" compact, "pad" n + 3 (odd: no 16 B rows), "ld" the drivers' pad_len(n) + 8 (a panel of a wider basis)
#   batch pitch: "compact", "padded" (+ 5 rows of sentinel between members), "2d" (a 2-D operator), "b1" (shape[0] == 1)
LAYOUTS = {
    "contig":   ("n", "compact", 0, 0),
    "driver":   ("ld", "compact", 0, 0),        # X[:, :, :N] / out[:, :, :N] of ld-padded panels (PanelOperator._native)
    "basis":    ("ld", "padded", 2, 0),         # Q[:, r0:r0 + rows, :N]: a row pitch of ld, a batch pitch of cap * ld
    "padrow":   ("pad", "padded", 1, 0),        # odd row pitch: no 16 B alignment of the rows
    "op2d":     ("ld", "2d", 0, 0),
    "opb1":     ("ld", "b1", 1, 0),
    "offset1":  ("ld", "compact", 0, 1),        # base pointer one element into the buffer
}


def place(t, layout, device=None, fill=math.nan, tail_rows=3):
    """Place the logical (B, R, n) array `t` (CPU) by LAYOUTS[layout] inside a `fill`-filled buffer on `device`."""
    pitch, batch, r0, off = LAYOUTS[layout]
    B, R, n = t.shape
    ld = {"n": n, "pad": n + 3, "ld": pad_len(n) + 8}[pitch]
    rows = r0 + R + (tail_rows if (batch == "padded" or r0) else 0)
    sB = rows * ld
    squeeze = batch == "2d"
    if batch in ("2d", "b1"):
        assert B == 1
    buf = torch.full((off + B * sB + 8,), fill, dtype=t.dtype)
    p = Placed(buf, (B, R, n), (sB, ld, 1), off + r0 * ld, squeeze)
    torch.as_strided(buf, p.shape, p.strides, p.offset).copy_(t)
    if device is not None:
        p.buf = buf.to(device)
    return p


def place_out(shape, dtype, layout, device=None, fill=math.nan):
    return place(torch.full(shape, fill, dtype=dtype), layout, device, fill)
