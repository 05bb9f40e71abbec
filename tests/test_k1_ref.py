"""CPU: the K1 checker of tests/k1_ref.py accepts the correct product rounded to the kernel dtype and rejects plausible
kernel faults, each at the shape, family and layout of a case that tests/test_gpu_k1_contract.py really runs (`_case`
looks the case up in its table and fails when it is gone, so a GPU case cannot be dropped without this file noticing).
Where the point is that the normwise criterion of tests/test_gpu_k1.py is blind, the fault is also shown to pass it."""
import math
import pytest
import torch
from tests import k1_ref as R
from tests import test_gpu_k1_contract as G

F64, F32 = torch.float64, torch.float32
ROWS = ("rows", "rows_scalar")


def _case(pred, what):
    for ci, c in enumerate(G.CASES):
        if c["form"] != "refuse" and c["entry"] != "panel" and max(c["M"], c["N"]) <= 4100 and pred(c):
            return ci, c
    raise AssertionError("tests/test_gpu_k1_contract.py has no case that would catch: " + what)


def _long(pred, what):
    for ci, c in enumerate(G.CASES):
        if c["form"] != "refuse" and pred(c):
            return ci, c
    raise AssertionError("tests/test_gpu_k1_contract.py has no case that would catch: " + what)


def _setup(ci, c):
    """what the GPU test feeds the kernel, in float64: (A as the kernel may read it, X, op (Ba, n_out, n_in), ref, mag)"""
    symm = c["entry"].startswith("symm")
    g = torch.Generator().manual_seed(1000 + ci)
    Ba = 1 if c["layout"] in G.OP_ONLY else c["B"]
    A, X = R.make_inputs(c["family"], g, c["dtype"], Ba, c["B"], c["M"], c["N"], c["P"], c["trans"], symm=symm, seed_edge=ci)
    Ain = G._poison_lower(A, c["entry"]) if symm else A
    ref, mag = R.ref_mm(Ain, X, c["trans"], symm=symm)
    A64 = R.mirror_upper(R.hp(A)) if symm else R.hp(A)
    op = A64.transpose(-2, -1) if c["trans"] else A64
    return Ain, R.hp(X), op, ref, mag


def _verdict(c, Y64, ref, mag):
    """the GPU test's value assertion on a float64 emulation rounded to the kernel dtype"""
    form = c["form"]
    terms, levels = R.form_terms(form, c["dtype"], c["B"], c["M"], c["N"], c["trans"])
    return R.check(Y64.to(c["dtype"]), ref, mag, c["dtype"], terms, levels, exact=R.is_exact(c["family"]), what=form)


def _accept_then_reject(c, ref, mag, bad, blind=False):
    assert _verdict(c, ref, ref, mag) <= 1.0
    n = c["M"] if c["trans"] else c["N"]
    with pytest.raises(AssertionError):
        _verdict(c, bad, ref, mag)
    if blind:
        assert R.normwise_ok(bad.to(c["dtype"]), ref, c["dtype"], n), "the old criterion was expected to be blind here"


def _part(op, X, terms, rows=None):
    """contribution of the contraction indices `terms` to the outputs `rows` (all when None), zero elsewhere"""
    y = torch.matmul(X[..., terms], op[..., terms].transpose(-2, -1))
    if rows is None:
        return y
    out = torch.zeros_like(y)
    out[..., rows] = y[..., rows]
    return out


# ------------------------------------------------------------------------------------------------ contraction tails
@pytest.mark.parametrize("dtype", [F64, F32])
def test_dropped_and_doubled_contraction_tail_of_the_row_sweep(dtype):
    step = 64 * R.VEC_ELEMS[dtype]
    ci, c = _case(lambda c: c["entry"] == "mm" and not c["trans"] and c["form"] == "rows" and c["dtype"] == dtype
                  and c["family"] == "integer" and c["N"] % step and c["N"] > step, "a dropped N % (64 VN) tail")
    _, X, op, ref, mag = _setup(ci, c)
    tail = slice(c["N"] - c["N"] % step, c["N"])
    _accept_then_reject(c, ref, mag, ref - _part(op, X, tail))
    _accept_then_reject(c, ref, mag, ref + _part(op, X, tail))                     # the tail taken twice


def test_tail_dropped_from_small_rows_only_is_invisible_to_the_normwise_criterion():
    ci, c = _case(lambda c: c["entry"] == "mm" and not c["trans"] and c["form"] in ROWS and c["dtype"] == F32
                  and c["family"] == "graded" and c["M"] >= 64 and c["N"] >= 64, "a tail dropped from the small rows")
    _, X, op, ref, mag = _setup(ci, c)
    bad = ref - _part(op, X, slice(c["N"] - 2, c["N"]), rows=slice(0, 16))         # the first workgroup's rows
    _accept_then_reject(c, ref, mag, bad, blind=True)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_dropped_slab_tails_and_last_slab_of_the_column_sweep(dtype):
    ci, c = _case(lambda c: c["entry"] == "mm" and c["trans"] and c["form"] == "cols" and c["dtype"] == dtype
                  and c["family"] == "integer" and c["M"] in (1000, 2049) and c["N"] <= 1024, "a dropped slab tail")
    _, X, op, ref, mag = _setup(ci, c)
    for nslab in set(R.cols_slabs(dtype, c["B"], c["M"], c["N"])):
        rps = (c["M"] + nslab - 1) // nslab
        # the shape really has ragged slabs: a short last slab, and 4-row steps that leave a remainder
        assert nslab > 1 and c["M"] % rps and (c["M"] % rps) % 4 and rps % 4
        tails = []
        for s in range(nslab):
            i0, i1 = s * rps, min((s + 1) * rps, c["M"])
            tails += list(range(i1 - (i1 - i0) % 4, i1))
        _accept_then_reject(c, ref, mag, ref - _part(op, X, torch.tensor(tails)))
        _accept_then_reject(c, ref, mag, ref - _part(op, X, slice((nslab - 1) * rps, c["M"])))


def test_every_tall_case_of_the_gpu_table_has_ragged_slabs():
    seen = 0
    for c in G.CASES:
        if c["entry"] == "mm" and c["trans"] and c["form"] == "cols" and c["M"] in (1000, 2049) and c["N"] <= 1024:
            for nslab in set(R.cols_slabs(c["dtype"], c["B"], c["M"], c["N"])):
                rps = (c["M"] + nslab - 1) // nslab
                assert nslab > 1 and c["M"] % rps and (c["M"] % rps) % 4, G._case_id(c)
            seen += 1
    assert seen >= 8


@pytest.mark.parametrize("dtype", [F64, F32])
def test_dropped_last_split(dtype):
    vn = R.VEC_ELEMS[dtype]
    ci, c = _long(lambda c: c["entry"] == "mm" and not c["trans"] and c["form"] == "rows" and c["dtype"] == dtype
                  and c["family"] == "integer" and c["N"] == 64 * vn * 83, "a dropped last split")
    _, X, op, ref, mag = _setup(ci, c)
    from tests.davidson_ref import _choose_nsplit
    ns = _choose_nsplit(c["B"], c["M"], c["N"], 8, vn)
    sps = (83 + ns - 1) // ns
    nsplit = (83 + sps - 1) // sps
    assert nsplit > 1 and 83 - (nsplit - 1) * sps < sps, "the case was meant to have a short last split"
    _accept_then_reject(c, ref, mag, ref - _part(op, X, slice((nsplit - 1) * sps * 64 * vn, c["N"])))


# ------------------------------------------------------------------------------------------------ addressing
@pytest.mark.parametrize("P", [9, 13, 17, 33])
def test_column_block_offset_faults(P):
    ci, c = _case(lambda c: c["entry"] == "mm" and c["P"] == P and c["family"] == "integer"
                  and c["form"] in ("rows", "cols", "rows_scalar", "cols_scalar"), "a column-block offset at P = %d" % P)
    _, X, op, ref, mag = _setup(ci, c)
    bad = ref.clone()
    bad[:, 8:] = math.nan                       # c0 * ldx used for c0 * ldy: the block lands elsewhere, the sentinel stays
    _accept_then_reject(c, ref, mag, bad)
    bad = ref.clone()
    bad[:, 8:] = ref[:, torch.arange(8, P) % 8]
    _accept_then_reject(c, ref, mag, bad)       # the first block written twice
    # and the misplaced block is seen by the sentinel check whenever the pitches of X and out differ
    ci, c = _case(lambda c: c["entry"] == "mm" and c["P"] >= 9 and c["layout"] in ("driver", "basis")
                  and c["form"] in ("rows", "cols") and R.pad_len(c["M"]) != R.pad_len(c["N"]), "c0 * ldx for c0 * ldy")
    _, X, op, ref, mag = _setup(ci, c)
    px = R.place(X.to(c["dtype"]), c["layout"])
    po = R.place_out(tuple(ref.shape), c["dtype"], c["layout"])
    before = po.buf.clone()
    po.view.copy_(ref.to(c["dtype"]))
    assert po.outside_untouched(before)
    off = po.offset + 8 * px.strides[1]
    if off + 4 <= po.buf.numel():
        po.buf[off:off + 4] = 1.0
        inside = torch.zeros(po.buf.numel(), dtype=torch.bool)
        po.of(inside).fill_(True)
        assert bool(inside[off:off + 4].all()) or not po.outside_untouched(before)


def test_ldy_taken_as_compact_on_a_padded_out_and_clamped_row_stored():
    ci, c = _case(lambda c: c["entry"] == "mm" and not c["trans"] and c["layout"] in ("driver", "basis") and c["P"] >= 2
                  and c["form"] == "rows" and c["M"] % 16, "ldy = M on a padded out")
    _, X, op, ref, mag = _setup(ci, c)
    B, P, nout = ref.shape
    po = R.place_out((B, P, nout), c["dtype"], c["layout"])
    before = po.buf.clone()
    torch.as_strided(po.buf, (B, P, nout), (po.strides[0], nout, 1), po.offset).copy_(ref.to(c["dtype"]))
    with pytest.raises(AssertionError):
        _verdict(c, R.hp(po.view), ref, mag)
    # a clamped duplicate of the last row stored at row M: the values are right, the padding is not
    po = R.place_out((B, P, nout), c["dtype"], c["layout"])
    po.view.copy_(ref.to(c["dtype"]))
    assert _verdict(c, R.hp(po.view), ref, mag) <= 1.0 and po.outside_untouched(before)
    torch.as_strided(po.buf, (B, P, 1), po.strides, po.offset + nout).copy_(ref[:, :, -1:].to(c["dtype"]))
    assert not po.outside_untouched(before)


def test_batch_pitch_of_a_broadcast_operator_not_zeroed():
    for lay in G.OP_ONLY:
        ci, c = _case(lambda c: c["layout"] == lay and c["B"] >= 2 and c["family"] == "integer" and c["M"] > 2,
                      "sA != 0 for a %s operator" % lay)
        A, X, op, ref, mag = _setup(ci, c)
        # member b reads b * M * lda further on: the sentinel rows that follow the operator in its buffer
        pa = R.place(A, lay)
        M, N = A.shape[-2:]
        ld = pa.strides[1]
        want = pa.offset + M * ld + N
        buf = torch.cat([pa.buf, torch.full((max(0, want + M * ld - pa.buf.numel()),), math.nan, dtype=A.dtype)])
        A1 = torch.as_strided(buf, (1, M, N), (0, ld, 1), pa.offset + M * ld)
        bad = ref.clone()
        bad[1:] = R.ref_mm(A1, X[1:], c["trans"])[0]
        _accept_then_reject(c, ref, mag, bad)


def test_padding_read_reaches_the_result():
    for lay, which in (("driver", "X"), ("basis", "A")):
        ci, c = _case(lambda c: c["entry"] == "mm" and not c["trans"] and c["layout"] == lay and c["form"] in ROWS,
                      "a read of the %s padding" % which)
        A, X, op, ref, mag = _setup(ci, c)
        px, pa = R.place(X.to(c["dtype"]), lay), R.place(A, lay)
        n = c["N"]
        Xe = torch.as_strided(px.buf, (c["B"], c["P"], n + 1), px.strides, px.offset)
        Ae = torch.as_strided(pa.buf, (A.shape[0], c["M"], n + 1), pa.strides, pa.offset)
        assert bool(torch.isnan(Xe[..., n]).all()) and bool(torch.isnan(Ae[..., n]).all())       # the layouts poison both
        if which == "X":
            bad = torch.matmul(R.hp(Xe), torch.cat([op, torch.zeros_like(op[..., :1])], -1).transpose(-2, -1))
        else:
            bad = torch.matmul(torch.cat([X, torch.zeros_like(X[..., :1])], -1), R.hp(Ae).transpose(-2, -1))
        _accept_then_reject(c, ref, mag, bad)


# ------------------------------------------------------------------------------------------------ tiles and fragments
def test_transposed_sub_tile():
    for trans in (False, True):
        ci, c = _case(lambda c: c["entry"] in ("mm", "wide", "rows_wide") and c["trans"] == trans and c["M"] >= 64
                      and c["N"] >= 64 and c["family"] == "integer", "A for A^T in one 64 x 64 sub-tile")
        _, X, op, ref, mag = _setup(ci, c)
        op2 = op.clone()
        op2[..., :64, :64] = op[..., :64, :64].transpose(-2, -1)
        _accept_then_reject(c, ref, mag, torch.matmul(X, op2.transpose(-2, -1)))


@pytest.mark.parametrize("entry", ["symm", "symm_wide", "symm_split", "symm_wide_split"])
def test_symmetric_tile_faults(entry):
    ci, c = _case(lambda c: c["entry"] == entry and c["N"] >= 256 and c["family"] == "integer" and c["N"] <= 1100,
                  "a symmetric tile fault of " + entry)
    Ain, X, op, ref, mag = _setup(ci, c)
    assert bool(torch.isnan(Ain[..., 128:192, 0:64]).all()), "the GPU test poisons the lower triangle"
    # the lower triangle read for one tile: y[128:192] += A[128:192, 0:64] x[0:64] taken from the stored lower block
    low = R.hp(Ain)[..., 128:192, 0:64]
    bad = ref.clone()
    bad[..., 128:192] += torch.matmul(X[..., 0:64], low.transpose(-2, -1)) - torch.matmul(X[..., 0:64], op[..., 128:192, 0:64].transpose(-2, -1))
    _accept_then_reject(c, ref, mag, bad)
    # a diagonal tile counted twice
    bad = ref.clone()
    bad[..., 0:64] += torch.matmul(X[..., 0:64], op[..., 0:64, 0:64].transpose(-2, -1))
    _accept_then_reject(c, ref, mag, bad)
    # an off-diagonal tile not mirrored: y[64:128] misses A[0:64, 64:128]^T x[0:64]
    bad = ref.clone()
    bad[..., 64:128] -= torch.matmul(X[..., 0:64], op[..., 64:128, 0:64].transpose(-2, -1))
    _accept_then_reject(c, ref, mag, bad)


@pytest.mark.parametrize("form", ["K1w", "K1wr", "K1sw"])
def test_permuted_mfma_fragment_rows(form):
    ci, c = _case(lambda c: c["form"] == form and c["family"] in ("integer", "onehot") and min(c["M"], c["N"]) >= 32,
                  "permuted rows of one MFMA fragment of " + form)
    _, X, op, ref, mag = _setup(ci, c)
    bad = ref.clone()
    bad[..., 16:32] = ref[..., 16:32][..., torch.arange(16) ^ 1]        # neighbouring rows of one 16-row fragment swapped
    if torch.equal(bad, ref):                                             # (one-hot outputs may coincide in that fragment)
        bad[..., 16:32] = ref[..., 16:32].flip(-1)
    _accept_then_reject(c, ref, mag, bad)


def test_shared_exponent_accumulation_fails_the_graded_bound_and_passes_the_normwise_one():
    """an fp32 product accumulated in a lower precision: partial sums kept on the grid 2^-20 max|y| of the whole member
    (a block-floating-point accumulator).  Normwise that is 1e-6, far under 3e-6 sqrt(N); the small rows of a graded
    operator are lost."""
    ci, c = _case(lambda c: c["entry"] == "mm" and not c["trans"] and c["dtype"] == F32 and c["family"] == "graded"
                  and c["M"] >= 64 and c["N"] >= 64, "a lower-precision accumulator")
    _, X, op, ref, mag = _setup(ci, c)
    q = ref.abs().amax(dim=(1, 2), keepdim=True) * 2.0 ** -20
    bad = torch.round(ref / q) * q
    _accept_then_reject(c, ref, mag, bad, blind=True)


# ------------------------------------------------------------------------------------------------ the module itself
def test_integer_family_is_exact_in_any_order_and_refuses_beyond_its_limit():
    g = torch.Generator().manual_seed(3)
    for N in (8192, 16384):
        A, X = R.make_inputs("integer", g, F32, 1, 1, 4, N, 3, False)
        ref, _ = R.ref_mm(A, X, False)
        fwd = torch.matmul(X, A.transpose(-2, -1))
        rev = torch.matmul(X.flip(-1), A.flip(-1).transpose(-2, -1))
        assert torch.equal(fwd.double(), ref) and torch.equal(rev.double(), ref) and float(ref.abs().max()) < 2 ** 24
    with pytest.raises(AssertionError):
        R.make_inputs("integer", g, F32, 1, 1, 2, 2 ** 18, 1, False)
    with pytest.raises(AssertionError):
        R.make_inputs("onehot", g, F32, 1, 1, 4097, 4096, 1, False)


def test_symmetric_reference_never_reads_the_lower_triangle():
    g = torch.Generator().manual_seed(4)
    A, X = R.make_inputs("graded", g, F64, 2, 2, 96, 96, 3, False, symm=True)
    ref, mag = R.ref_mm(A, X, False)
    ref2, mag2 = R.ref_mm(G._poison_lower(A, "symm"), X, False, symm=True)
    assert torch.equal(ref, ref2) and torch.equal(mag, mag2)


def test_cancelling_family_cancels_and_layouts_round_trip():
    g = torch.Generator().manual_seed(5)
    A, X = R.make_inputs("cancelling", g, F64, 1, 2, 20, 4096, 3, False)
    ref, mag = R.ref_mm(A, X, False)
    assert float((ref.abs() / mag).max()) < 1e-5
    for lay in R.LAYOUTS:
        t = torch.randn(1, 5, 12, dtype=F32, generator=g)
        p = R.place(t, lay)
        assert torch.equal(p.view.reshape(1, 5, 12), t)
        before = p.buf.clone()
        p.view.fill_(2.0)
        assert p.outside_untouched(before)
        assert int(torch.isnan(p.buf).sum()) == p.buf.numel() - 60
        vn = 4
        aligned = (p.offset % vn == 0) and (p.strides[1] % vn == 0) and (p.strides[0] % vn == 0)
        assert aligned == (lay in G.ALIGNED_LAYOUTS), lay


def test_gpu_table_covers_every_edge_value_and_layout():
    mm = [c for c in G.CASES if c["entry"] == "mm"]
    for P in G.P_EDGES:
        assert any(c["P"] == P and c["trans"] == t and c["dtype"] == d for c in mm for t in (False,) for d in (F64,)), P
        assert {(c["trans"], c["dtype"]) for c in mm if c["P"] == P} >= {(False, F64), (True, F64), (False, F32), (True, F32)}
    for lay in G.ALL_LAYOUTS:
        assert {c["dtype"] for c in mm if c["layout"] == lay} >= {F64, F32}, lay
    for e in (1, 63, 64, 65, 255, 256, 257, 511, 513, 1023, 1025, 2049):
        assert any(c["M"] == e for c in mm) and any(c["N"] == e for c in mm), e
    entries = {c["entry"] for c in G.CASES}
    assert entries == {"mm", "wide", "rows_wide", "symm", "symm_wide", "symm_split", "symm_wide_split", "complex", "panel"}
    assert {c["kw"].get("sw") for c in G.CASES if c["entry"] == "symm_wide" and c["form"] != "refuse"} == {0, 1, 3, 9, "resident"}
    assert {(c["trans"], c["kw"]["conj_io"], c["dtype"]) for c in G.CASES if c["entry"] == "complex"} == \
        {(a, b, d) for a in (False, True) for b in (False, True) for d in (torch.complex128, torch.complex64)}
    assert any(c["form"] == "refuse" for c in G.CASES)
