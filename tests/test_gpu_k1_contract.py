"""-m gpu: every K1 form (xk_dense.hip row / column sweeps with their scalar fallbacks, split contraction and slabs;
K1w; K1wr; K1s; K1sw; the two-stream variants; the complex wrapper; PanelOperator) on the inputs and layouts of
tests/k1_ref.py: integer and one-hot inputs must come back BIT FOR BIT, graded and cancelling ones within the per-entry
bound, on the strided views the drivers really pass (ld-padded panels in and out, a basis used as the matrix with a
row offset, 2-D and shape[0] == 1 operators, a base pointer one element into its buffer), inside NaN-filled buffers.

CASES is one table.  Each row names the entry, the layout and the form that must serve it.  The `form` column is
written from DESIGN.md §3.0 ("K1 forms and the layouts they require") and the wrappers' docstrings by `documented_form`
below — a restatement of the document, not a call into the code under test (`_wide_ok`, `_rows_wide_ok` and
`symm_wide_ok` are never consulted).  "refuse" rows assert the documented refusal (NativeLibraryError, nothing
written); no row is ever skipped.

Per case: values (exact or bounded); every byte of the `out` buffer outside the logical result untouched; inputs
unchanged; NaN padding of the inputs does not reach the result; a second call is bit-identical; a NaN and a +inf
planted at one A[b, i, j] make exactly the dependent outputs non-finite (row i for A X, column j for A^T X, rows i and j
for the symmetric kernels) and leave every other output bit-identical.  Nothing here is meant to fault and nothing
probes memory outside buffers this file allocated.
"""
import json
import math
import os
import time
import pytest
import torch
from tests import k1_ref as R
from xitorch_amd import kernels as K, _capi
from xitorch_amd import LinearOperator

pytestmark = pytest.mark.gpu

F64, F32, C128, C64 = torch.float64, torch.float32, torch.complex128, torch.complex64
NAME = {F64: "f64", F32: "f32", C128: "c128", C64: "c64"}
ALIGNED_LAYOUTS = ("contig", "driver", "basis", "op2d", "opb1")      # 16 B rows and base pointer (contig: if n % VN == 0)
OP_ONLY = ("op2d", "opb1")                                           # broadcast operators: the panels take "driver"
PANEL_LAYOUTS = ("contig", "driver", "basis", "padrow", "offset1")
ALL_LAYOUTS = PANEL_LAYOUTS + OP_ONLY
P_EDGES = list(range(1, 18)) + [19, 20, 27, 28, 31, 32, 33, 50]
TIMES = {}


def _vec(layout, n, dtype):
    """rows of length n in `layout` start on 16 B boundaries and the base pointer is 16 B aligned"""
    vn = R.VEC_ELEMS[dtype]
    return layout in ALIGNED_LAYOUTS and n % vn == 0


def documented_form(entry, dtype, M, N, P, trans, layout, wide=True, rows_hint=0):
    """DESIGN.md §3.0, restated.  (M, N) is the operator; the panel and `out` share the alignment class of the layout."""
    vn = R.VEC_ELEMS[dtype]
    if entry == "mm" and not trans:
        if rows_hint == 16 and P > 4 and not (wide and P >= 12 and _vec(layout, N, dtype)):
            return "refuse"                                   # 16 rows per wave hold at most 4 columns of accumulators
        if not _vec(layout, N, dtype):
            return "rows_scalar"
        return "K1wr" if (wide and P >= 12) else "rows"
    if entry == "mm" and trans:
        if not _vec(layout, N, dtype):
            return "cols_scalar"
        wcols = 32 if dtype == F64 else 128
        return "K1w" if (wide and P >= 12 and N % wcols == 0) else "cols"
    if entry == "wide":                                       # K1w: up to 32 columns, whole 16 x VN column tiles
        wcols = 128 if (dtype == F32 and P > 16) else 16 * vn          # fp32 beyond 16 columns: 32-wide MFMA tiles
        return "K1w" if (P <= 32 and N % wcols == 0 and _vec(layout, N, dtype)) else "refuse"
    if entry == "rows_wide":                                  # K1wr: 16 B loads of the operator AND the panel
        return "K1wr" if _vec(layout, N, dtype) else "refuse"
    if entry in ("symm", "symm_split"):                       # K1s: 16 B loads of both; split: one 6-column chunk
        if entry == "symm_split" and P > 6:
            return "refuse"
        return "K1s" if _vec(layout, N, dtype) else "refuse"
    if entry in ("symm_wide", "symm_wide_split"):             # K1sw: fp32, whole 64-row bands, at most 16 columns
        ok = dtype == F32 and N % 64 == 0 and 1 <= P <= 16 and _vec(layout, N, dtype)
        return "K1sw" if ok else "refuse"
    raise ValueError(entry)


CASES = []


def _c(entry, dtype, B, M, N, P, trans=False, layout="contig", family="integer", form=None, **kw):
    if form is None:
        form = documented_form(entry, dtype, M, N, P, trans, layout, kw.get("wide", True), kw.get("rows_hint", 0))
    d = dict(entry=entry, dtype=dtype, B=B, M=M, N=N, P=P, trans=trans, layout=layout, family=family, form=form, kw=kw)
    CASES.append(d)
    return d


def _case_id(c):
    kw = ",".join("%s=%s" % (k, v) for k, v in sorted(c["kw"].items()))
    return "%s-%s-B%dM%dN%dP%d-%s-%s-%s-%s%s" % (c["entry"], NAME[c["dtype"]], c["B"], c["M"], c["N"], c["P"],
                                                 "T" if c["trans"] else "N", c["layout"], c["family"], c["form"],
                                                 "-" + kw if kw else "")


def _build_cases():
    fam3 = ("integer", "onehot", "graded")
    # ---- dense_mm: every panel width at which the column-block logic changes, both orientations, all layouts
    shapes = [(2, 77, 200), (1, 130, 96), (3, 33, 516)]
    k = 0
    for dtype in (F64, F32):
        for trans in (False, True):
            for P in P_EDGES:
                B, M, N = shapes[k % 3]
                if trans and dtype == F32 and k % 2:
                    N = 256                                                  # a K1w-eligible row length (N % 128 == 0)
                _c("mm", dtype, B, M, N, P, trans, ALL_LAYOUTS[k % 7], "integer", wide=(k % 3 != 0))
                k += 1
    # ---- dense_mm: M and N at vector, wave, tile and slab edges
    for dtype in (F64, F32):
        vn = R.VEC_ELEMS[dtype]
        edges = [1, vn - 1, vn, vn + 1, 63, 64, 65, 255, 256, 257, 511, 513, 1023, 1025, 2049, 3001]
        for trans in (False, True):
            for which in ("M", "N"):
                for e in edges:
                    M, N = (e, 200) if which == "M" else (37, e)
                    _c("mm", dtype, 2 if e < 1000 else 1, M, N, (3, 6, 8, 11)[k % 4], trans, ALL_LAYOUTS[k % 7],
                       fam3[k % 3])
                    k += 1
        # row-group edges of the row sweep: 4 R rows per workgroup, R = 4 / 8 / 12 / 16 (rows_hint, or RowsFor<P>)
        for hint, P, Rr in ((4, 6, 4), (8, 6, 8), (16, 3, 16), (0, 3, 12), (0, 9, 4), (0, 2, 16), (0, 7, 8)):
            for M in (4 * Rr - 1, 4 * Rr, 4 * Rr + 1):
                _c("mm", dtype, 2, M, 136, P, False, ("driver", "basis", "padrow")[k % 3], fam3[k % 2], wide=False,
                   rows_hint=hint)
                k += 1
        _c("mm", dtype, 2, 40, 136, 5, False, "driver", "integer", wide=False, rows_hint=16)        # must raise
        _c("mm", dtype, 2, 40, 136, 12, False, "driver", "integer", wide=False, rows_hint=16)       # must raise
        # ---- skinny and long: the split contraction (fold_splits), with a short last split (83 steps in 10 splits
        #      of 9: the last has 2), column blocks over the split workspace (P = 12, wide off), K1wr's own split
        for (B, M, N, P, lay, fam, wide) in (
                (1, 7, 32768, 1, "contig", "integer", True), (2, 54, 16384, 6, "basis", "integer", True),
                (3, 20, 8192, 6, "driver", "onehot", True), (1, 20, 64 * vn * 83, 6, "basis", "onehot", True),
                (2, 33, 64 * vn * 83, 5, "driver", "integer", True), (1, 64, 64 * vn * 83 + vn, 12, "basis", "integer", False),
                (2, 13, 8192, 12, "driver", "onehot", False), (1, 54, 16384, 6, "opb1", "cancelling", True),
                (2, 20, 8192, 3, "driver", "cancelling", True), (1, 20, 8192, 6, "op2d", "graded", True),
                (2, 48, 8192, 16, "driver", "integer", True), (1, 64, 12288, 17, "basis", "graded", True),
                (1, 20, 8195, 6, "padrow", "integer", True), (1, 9, 8192, 4, "offset1", "onehot", True)):
            _c("mm", dtype, B, M, N, P, False, lay, fam, wide=wide)
        # ---- tall: the column sweep over several slabs with M % rows_per_slab and (M % rows_per_slab) % 4 non-zero
        #      (tests/test_k1_ref.py checks these shapes against the slab arithmetic)
        for (B, M, N, P, lay, fam, wide) in (
                (1, 1000, 512, 6, "driver", "integer", True), (1, 1000, 1024, 6, "basis", "onehot", True),
                (2, 2049, 64, 7, "driver", "onehot", True), (1, 1000, 512, 12, "basis", "integer", False),
                (1, 1000, 516, 16, "driver", "integer", False), (2, 2049, 64, 17, "contig", "integer", False),
                (1, 1000, 512, 3, "opb1", "cancelling", True), (2, 2049, 64, 5, "driver", "cancelling", True),
                (1, 1000, 512, 8, "op2d", "graded", True), (1, 1000, 512, 33, "driver", "integer", False),
                (1, 1000, 513, 6, "contig", "integer", True), (1, 1000, 512, 6, "offset1", "onehot", True)):
            _c("mm", dtype, B, M, N, P, True, lay, fam, wide=wide)
        # ---- K1w (dense_wide) and K1wr (dense_rows_wide) called directly
        wc = 16 * vn
        for (B, M, N, P, lay, fam) in (
                (2, 130, 4 * wc, 1, "contig", "integer"), (1, 1, wc, 9, "driver", "integer"), (2, 3, 2 * wc, 12, "basis", "onehot"),
                (1, 127, 8 * wc, 16, "op2d", "integer"), (2, 129, 4 * wc, 17, "driver", "integer"),
                (1, 300, 4 * wc, 32, "basis", "onehot"), (1, 513, 6 * wc, 31, "opb1", "graded"),
                (2, 1025, 4 * wc, 16, "driver", "graded"), (1, 300, 4 * wc, 33, "driver", "integer"),      # > 32: refuse
                (1, 300, 4 * wc + vn, 16, "driver", "integer"), (1, 300, 4 * wc, 16, "offset1", "integer"),
                (1, 300, 4 * wc, 16, "padrow", "integer")):
            _c("wide", dtype, B, M, N, P, True, lay, fam)
        for (B, M, N, P, lay, fam) in (
                (2, 63, 128, 12, "contig", "integer"), (1, 64, vn, 16, "driver", "integer"), (2, 65, 14 * 2, 17, "basis", "onehot"),
                (1, 255, 128 // (8 // vn) + vn, 32, "op2d", "integer"), (2, 257, 4100, 13, "driver", "onehot"),
                (1, 1, 256, 50, "basis", "integer"), (1, 1025, 96, 33, "opb1", "graded"), (2, 130, 1026 + 2 * (vn - 1), 1, "driver", "graded"),
                (1, 300, 128 + 1, 16, "contig", "integer"), (1, 300, 128, 16, "offset1", "integer"),
                (1, 300, 128, 16, "padrow", "integer")):
            _c("rows_wide", dtype, B, M, N, P, False, lay, fam)
        # ---- K1s: the opts grid of tests/test_gpu_k1.py (runs of 1 / 2 / 3 slabs x tile heights), the resident and
        #      the 8-wave forms, orders at the slab / tile edges and ragged last runs; refusals for odd orders
        grid = [dict(run=1, tile=1024), dict(run=2, tile=1024), dict(run=3, tile=1024), dict(run=1, tile=512),
                dict(run=2, tile=512), dict(run=3, tile=0), dict(run=1, tile=1024, persist=1), dict(run=2, tile=512, persist=3),
                dict(run=3, tile=0, persist=8), dict(run=1, tile=2048), dict(run=2, tile=2048, persist=1), dict()]
        orders = [vn, 64, 64 + vn, 256, 256 + vn, 512, 512 + vn, 1024 - vn, 1024, 1024 + vn, 2048, 2048 + vn, 3072 + 6 * vn,
                  4096 + vn]
        for i, n in enumerate(orders):
            for j in range(3):
                o = grid[(i * 3 + j) % len(grid)]
                lay = ("contig", "driver", "basis", "op2d", "opb1")[(i + j) % 5]
                _c("symm", dtype, 1 if n > 2048 else 2, n, n, (1, 2, 3, 4, 5, 6, 7, 11, 13)[(i * 3 + j) % 9], False, lay,
                   ("integer", "graded", "onehot")[j] if n <= 4096 else ("integer", "graded", "integer")[j], **o)
        for (n, lay) in ((2047, "driver"), (4097, "driver"), (2048, "offset1"), (1024, "padrow")):
            _c("symm", dtype, 1, n, n, 6, False, lay, "integer")
        for (B, n, P, lay, fam) in ((2, 1024 + vn, 6, "driver", "integer"), (1, 2048, 4, "basis", "graded"),
                                    (2, 512, 1, "contig", "onehot"), (1, 1024, 7, "driver", "integer"),
                                    (1, 1024, 6, "offset1", "integer")):
            _c("symm_split", dtype, B, n, n, P, False, lay, fam)
    # ---- K1sw (fp32): forms 0 / 1 / 3 / 9 and the resident launch, orders on its N % 64 == 0 grid
    forms = (0, 1, 3, 9, "resident")
    k = 0
    for (B, n, P, lay, fam) in (
            (2, 1152, 9, "contig", "integer"), (1, 1216, 16, "driver", "onehot"), (2, 960, 12, "basis", "integer"),
            (2, 1024, 16, "driver", "integer"), (1, 1024, 9, "op2d", "onehot"), (3, 1088, 12, "basis", "graded"),
            (1, 2304, 13, "opb1", "integer"), (2, 1472, 16, "driver", "onehot"), (1, 2048, 1, "contig", "integer"),
            (1, 1024, 8, "driver", "graded"), (1, 4096, 16, "driver", "integer")):
        for f in (forms if n in (1024, 1088, 2304) else (forms[k % 5], forms[(k + 2) % 5])):
            _c("symm_wide", F32, B, n, n, P, False, lay, fam, sw=f)
        k += 1
    for (B, n, P, lay) in ((1, 1000, 12, "driver"), (1, 1024, 17, "driver"), (1, 1024, 12, "offset1"),
                           (1, 1024, 12, "padrow")):
        _c("symm_wide", F32, B, n, n, P, False, lay, "integer", sw=9)
    _c("symm_wide", F64, 1, 1024, 1024, 12, False, "driver", "integer", sw=9)                      # fp64: refuse
    for (B, n, P, lay, fam, f) in ((2, 1024, 16, "driver", "integer", 9), (1, 1088, 9, "basis", "graded", 3),
                                   (1, 2304, 12, "driver", "onehot", 1), (1, 1024, 12, "offset1", "integer", 9)):
        _c("symm_wide_split", F32, B, n, n, P, False, lay, fam, sw=f)
    # ---- the complex wrapper: all four (adjoint, conj_io), both types; 2 P >= 12 reaches K1wr / K1w underneath
    k = 0
    for dtype in (C128, C64):
        for adjoint in (False, True):
            for conj_io in (False, True):
                for (B, M, N, P) in ((2, 33, 20, 3), (1, 64, 130, 6), (2, 100, 64, 7)):
                    _c("complex", dtype, B, M, N, P, adjoint, ("contig", "driver", "basis")[k % 3],
                       ("integer", "graded", "onehot")[k % 3], form="complex", conj_io=conj_io)
                    k += 1
    # ---- PanelOperator.apply / apply_on on dense operators: which kernel serves (`last_kernel`, written by hand)
    for (dtype, B, N, P, herm, trans, on, kern, fam, extra) in (
            (F64, 2, 200, 6, False, False, False, "K1", "integer", {}), (F64, 2, 200, 6, False, True, False, "K1", "onehot", {}),
            (F64, 1, 256, 16, False, False, False, "K1wr", "integer", {}), (F64, 1, 256, 16, False, True, False, "K1w", "integer", {}),
            (F64, 1, 250, 16, False, True, False, "K1", "integer", {}), (F32, 2, 256, 12, False, False, True, "K1wr", "graded", {}),
            (F64, 2, 256, 6, True, False, False, "K1", "integer", {}), (F64, 2, 256, 12, True, False, False, "K1w", "graded", {}),
            (F32, 1, 1024, 12, True, False, False, "K1sw", "integer", {}), (F32, 2, 1088, 16, True, False, True, "K1sw", "graded", {}),
            (F32, 1, 1000, 12, True, False, False, "K1", "integer", {}),
            (F64, 2, 1026, 6, True, False, False, "K1s", "integer", dict(k1s=True)),
            (F64, 1, 2048, 4, True, False, True, "K1s", "graded", dict(k1s=True)),
            (F32, 2, 1028, 7, True, False, True, "K1s", "integer", dict(k1s=True)),
            (F64, 1, 1026, 12, True, False, False, "K1", "integer", dict(k1s=True)),
            (F64, 1, 1001, 6, True, False, False, "K1", "integer", dict(k1s=True))):
        _c("panel", dtype, B, N, N, P, trans, "driver", fam, form=kern, herm=herm, on=on, **extra)


_build_cases()


# ------------------------------------------------------------------------------------------------ running one case
def _poison_lower(A, entry):
    """NaN where the symmetric kernels must never read: strictly below the diagonal (K1sw: and outside the 64 x 64
    diagonal blocks, which it reads whole)"""
    n = A.shape[-1]
    i = torch.arange(n)
    low = i[:, None] > i[None, :]
    if entry.startswith("symm_wide"):
        low = low & ((i[:, None] // 64) != (i[None, :] // 64))
    return torch.where(low, torch.full_like(A, math.nan), A)


def _k1s_opts(kw):
    if "run" not in kw:
        return None
    o = (int(kw["run"]) << 8) | {0: 0, 512: 4, 1024: 8, 2048: 32}[kw["tile"]]
    if "persist" in kw:
        o |= K.K1S_PERSIST | (int(kw["persist"]) << 16)
    return o


class _Runner:
    def __init__(self, c, dev, monkeypatch):
        self.c, self.dev, self.mp = c, dev, monkeypatch
        self.symm = c["entry"].startswith("symm") or (c["entry"] == "panel" and c["kw"]["herm"])
        self.op = None

    def place_inputs(self, A, X):
        c = self.c
        lay = c["layout"]
        if c["entry"] == "complex":
            return R.place(A, "contig" if lay != "basis" else "basis", self.dev), R.place(X, lay, self.dev)
        if c["entry"] == "panel":
            Xp = torch.full((X.shape[0], X.shape[1], R.pad_len(X.shape[2])), math.nan, dtype=X.dtype)
            Xp[:, :, :X.shape[2]] = X
            return R.place(A, "contig", self.dev), R.place(Xp, "contig", self.dev)
        return R.place(A, lay, self.dev), R.place(X, "driver" if lay in OP_ONLY else lay, self.dev)

    def place_out(self, nout):
        c = self.c
        lay = "driver" if c["layout"] in OP_ONLY else c["layout"]
        if c["entry"] == "panel":
            return R.place_out((c["B"], c["P"], R.pad_len(nout)), c["dtype"], "contig", self.dev)
        return R.place_out((c["B"], c["P"], nout), c["dtype"], lay, self.dev)

    def call(self, pa, px, po):
        c, kw = self.c, self.c["kw"]
        A, X, out = pa.view, px.view, po.view
        e = c["entry"]
        if e == "mm":
            K.dense_mm(A, X, out=out, trans=c["trans"], rows_hint=kw.get("rows_hint", 0), wide=kw.get("wide", True))
        elif e == "wide":
            K.dense_wide(A, X, out=out)
        elif e == "rows_wide":
            K.dense_rows_wide(A, X, out=out)
        elif e == "symm":
            K.dense_symm(A, X, out=out, opts=_k1s_opts(kw))
        elif e in ("symm_wide", "symm_wide_split"):
            f = kw["sw"]
            self.mp.setattr(K, "K1SW_OPTS", 3 if f == "resident" else f)
            self.mp.setattr(K, "K1SW_RESIDENT", f == "resident")
            if e == "symm_wide":
                K.dense_symm_wide(A, X, out=out)
            else:
                K.dense_symm_wide_split(A, X, out, torch.cuda.Stream(device=self.dev))
        elif e == "symm_split":
            K.dense_symm_split(A, X, out, torch.cuda.Stream(device=self.dev))
        elif e == "complex":
            K.dense_mm_complex(A, X, adjoint=c["trans"], conj_io=kw["conj_io"], out=out)
        elif e == "panel":
            from xitorch_amd.linalg import _panel
            if kw.get("k1s"):
                self.mp.setattr(_panel, "K1S_MIN_BYTES", 0.0)       # the crossover is a tuning constant, not a contract
            lo = LinearOperator.m(A, is_hermitian=True) if kw["herm"] else LinearOperator.m(A, is_hermitian=False)
            self.op = _panel.PanelOperator(lo, [c["B"]], c["B"], c["N"])
            if kw["on"]:
                self.op.apply_on(X, out, torch.cuda.Stream(device=self.dev))
            else:
                self.op.apply(X, out, trans=c["trans"])
        else:
            raise ValueError(e)
        torch.cuda.synchronize()

    def logical(self, po, nout):
        y = po.view.cpu()
        return y[:, :, :nout] if self.c["entry"] == "panel" else y


def _bits_equal(a, b):
    ra = torch.view_as_real(a) if a.is_complex() else a
    rb = torch.view_as_real(b) if b.is_complex() else b
    it = torch.int64 if ra.element_size() == 8 else torch.int32
    return ra.shape == rb.shape and torch.equal(ra.contiguous().view(it), rb.contiguous().view(it))


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[_case_id(c) for c in CASES])
def test_k1_contract(dev, ci, monkeypatch):
    t_start = time.perf_counter()
    c = CASES[ci]
    dtype, B, M, N, P, trans, kw = c["dtype"], c["B"], c["M"], c["N"], c["P"], c["trans"], c["kw"]
    entry, family, form = c["entry"], c["family"], c["form"]
    what = _case_id(c)
    run = _Runner(c, dev, monkeypatch)
    symm = run.symm
    g = torch.Generator().manual_seed(1000 + ci)
    Ba = 1 if c["layout"] in OP_ONLY else B
    A, X = R.make_inputs(family, g, dtype, Ba, B, M, N, P, trans, symm=symm, seed_edge=ci)
    poison = entry.startswith("symm")            # (PanelOperator verifies the symmetry of what it is given: no NaN there)
    Ain = _poison_lower(A, entry) if poison else A
    if entry == "complex":
        ref, mag = R.ref_mm_complex(A, X, trans, kw["conj_io"])
    else:
        ref, mag = R.ref_mm(Ain, X, trans, symm=symm)
    nout = ref.shape[-1]
    pa, px = run.place_inputs(Ain, X)
    po = run.place_out(nout)
    a0, x0, o0 = pa.buf.clone(), px.buf.clone(), po.buf.clone()

    if form == "refuse":
        with pytest.raises(_capi.NativeLibraryError):
            run.call(pa, px, po)
        torch.cuda.synchronize()
        assert _bits_equal(po.buf, o0), what + ": a refused call wrote to `out`"
        assert _bits_equal(pa.buf, a0) and _bits_equal(px.buf, x0)
        TIMES[what] = time.perf_counter() - t_start
        return

    run.call(pa, px, po)
    if entry == "panel":
        assert run.op.last_kernel == form, "%s: served by %s" % (what, run.op.last_kernel)
        tform = {"K1": "cols" if (trans or kw["herm"]) else "rows"}.get(form, form)
    else:
        tform = form
    Y = run.logical(po, nout)
    terms, levels = R.form_terms(tform, dtype, B, M, N, trans)
    R.check(Y, ref, mag, dtype, terms, levels, exact=R.is_exact(family), what=what, form=tform)
    # nothing outside the logical result was written; the inputs (their NaN padding included) are unchanged
    if entry == "panel":
        full = po.view.cpu()
        assert bool(torch.isnan(full[:, :, nout:]).all()), what + ": the panel's padding was written"
    assert po.outside_untouched(o0), what + ": bytes of `out` outside the logical result changed"
    assert _bits_equal(pa.buf, a0) and _bits_equal(px.buf, x0), what + ": an input was modified"

    # the dispatcher's documented choice is the kernel that ran: same bits as the named form called directly
    if entry == "mm" and not R.is_exact(family) and form in ("K1wr", "K1w", "rows", "cols") and not kw.get("rows_hint"):
        p2 = run.place_out(nout)
        if form == "K1wr":
            K.dense_rows_wide(pa.view, px.view, out=p2.view)
        elif form == "K1w":
            for c0 in range(0, P, 32):
                K.dense_wide(pa.view, px.view[:, c0:c0 + 32], out=p2.view[:, c0:c0 + 32])
        else:
            K.dense_mm(pa.view, px.view, out=p2.view, trans=trans, wide=False)
        torch.cuda.synchronize()
        assert _bits_equal(p2.view.cpu(), po.view.cpu()), what + ": not the bits of the documented form"

    # a second identical call is bit-identical
    p2 = run.place_out(nout)
    run.call(pa, px, p2)
    assert _bits_equal(p2.buf, po.buf), what + ": a second call differs"

    # a NaN / +inf at one operator entry reaches exactly the outputs that depend on it
    i = (M - 1) // 64 * 64 - 1 if M > 130 else M // 2               # the row before the last 64-row block
    j = N - 1
    if symm and i == j:
        i = 0
    bsel = Ba - 1
    for val in (() if (entry == "panel" and kw["herm"]) else (math.nan, math.inf)):
        A2 = A.clone()
        A2[bsel, i, j] = val
        if symm:
            A2[bsel, j, i] = val
            A2 = _poison_lower(A2, entry) if poison else A2
        pa2, _ = run.place_inputs(A2, X)
        p3 = run.place_out(nout)
        run.call(pa2, px, p3)
        Y3 = run.logical(p3, nout)
        dep = torch.zeros(B, P, nout, dtype=torch.bool)
        bs = slice(None) if Ba == 1 and B > 1 else bsel
        if symm:
            dep[bs, :, i] = True
            dep[bs, :, j] = True
        elif trans:
            dep[bs, :, j] = True
        else:
            dep[bs, :, i] = True
        fin = torch.isfinite(Y3)
        assert bool((~fin[dep]).all()), "%s: %r at A[%d, %d, %d] did not reach every dependent output" % (what, val, bsel, i, j)
        assert bool(fin[~dep].all()), "%s: %r at A[%d, %d, %d] reached an independent output" % (what, val, bsel, i, j)
        keep = ~dep
        assert _bits_equal(Y3[keep], Y[keep]), "%s: independent outputs changed with %r planted" % (what, val)
    TIMES[what] = time.perf_counter() - t_start


@pytest.mark.parametrize("dtype,N,P", [(F32, 1024, 12), (F32, 1088, 16), (F64, 1024, 6), (F32, 2048, 9), (F64, 256, 16)])
def test_all_forms_of_one_product_agree_bit_for_bit(dev, dtype, N, P, monkeypatch):
    """One integer symmetric operator, one panel: every K1 form that can serve the product returns the same bits (they
    all equal the exact integer result)."""
    g = torch.Generator().manual_seed(N + P)
    A, X = R.make_inputs("integer", g, dtype, 2, 2, N, N, P, False, symm=True)
    ref, _ = R.ref_mm(A, X, False, symm=True)
    want = ref.to(dtype)
    Ad, Xd = A.to(dev), X.to(dev)
    got = {"rows": K.dense_mm(Ad, Xd, wide=False), "cols": K.dense_mm(Ad, Xd, trans=True, wide=False),
           "mm": K.dense_mm(Ad, Xd), "mmT": K.dense_mm(Ad, Xd, trans=True), "K1wr": K.dense_rows_wide(Ad, Xd),
           "K1s": K.dense_symm(Ad, Xd), "K1s-run2-512": K.dense_symm(Ad, Xd, opts=(2 << 8) | 4),
           "K1s-resident": K.dense_symm(Ad, Xd, opts=(1 << 8) | 8 | K.K1S_PERSIST | (3 << 16))}
    if P <= 32:
        got["K1w"] = K.dense_wide(Ad, Xd)
    if dtype == F64:
        got["K1s-8wave"] = K.dense_symm(Ad, Xd, opts=(1 << 8) | 32)
    if dtype == F32 and P <= 16:
        for f in (0, 1, 3, 9):
            monkeypatch.setattr(K, "K1SW_OPTS", f)
            got["K1sw-%d" % f] = K.dense_symm_wide(Ad, Xd).clone()
    torch.cuda.synchronize()
    for name, Y in got.items():
        assert torch.equal(Y.cpu(), want), name


def test_zz_report_worst_ratios_and_time(dev):
    """not a check of the kernels: prints the worst error / bound per (dtype, form) and the wall time of the cases above,
    and writes both to $K1_CONTRACT_REPORT when that is set (the figures a commit message quotes)"""
    rep = {"worst": {"%s %s" % k: v for k, v in sorted(R.WORST.items())}, "cases": len(TIMES),
           "seconds": sum(TIMES.values()), "slowest": sorted(TIMES.items(), key=lambda kv: -kv[1])[:10]}
    print(json.dumps(rep, indent=1))
    path = os.environ.get("K1_CONTRACT_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(rep, f, indent=1)
    assert all(v <= 1.0 for v in R.WORST.values())
