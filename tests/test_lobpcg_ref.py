"""CPU: the reference of the LOBPCG rotation kernel (tests/lobpcg_ref.py) accepts a plain evaluation in the storage
precision — in any summation order — and rejects every planted fault."""
import pytest
import torch
from tests import lobpcg_ref as lr

DTYPES = [torch.float64, torch.float32, torch.complex128, torch.complex64]
IDS = ["f64", "f32", "c128", "c64"]
SHAPES = [(1, 1, 1), (3, 2, 1), (9, 6, 3), (13, 10, 5), (24, 16, 8)]


def _plain(S, AS, MS, C, lam, k, q, w, dtype, reverse=False):
    """the rotation in the storage precision by torch ops (a summation order of the library's choosing; reversed rows:
    yet another one): (S', AS', MS', Pnorm, Pmax)"""
    order = list(range(k))[::-1] if reverse else list(range(k))
    Ck = C[:, order, :q]

    def comb(t):
        return torch.einsum("bac,ban->bcn", Ck, t[:, order])
    rd = lr.REAL_OF[dtype]
    lamr = lam[:, :w].to(rd).to(dtype)
    outs = {}
    for name, t in (("S", S), ("AS", AS), ("MS", MS)):
        outs[name] = None if t is None else comb(t)
    R = outs["AS"][:, :w] - lamr[:, :, None] * (outs["MS"] if MS is not None else outs["S"])[:, :w]
    res = []
    for name, t in (("S", S), ("AS", AS), ("MS", MS)):
        if t is None:
            res.append(None)
            continue
        n = t.clone()
        n[:, :q] = outs[name]
        if name == "S":
            n[:, q:q + w] = R
        res.append(n)
    N = S.shape[2]
    ch = lr.chunk_elems(dtype)
    nblk = -(-N // ch)
    a2 = (R.abs().to(torch.float64)) ** 2
    Pn = torch.stack([a2[:, :, j * ch:(j + 1) * ch].sum(-1) for j in range(nblk)], dim=-1)
    Pm = torch.stack([R.abs().to(torch.float64)[:, :, j * ch:(j + 1) * ch].amax(dim=(1, 2)) for j in range(nblk)], dim=-1)
    return res[0], res[1], res[2], Pn, Pm


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["randn", "graded", "cancel", "integer"])
@pytest.mark.parametrize("with_m", [True, False], ids=["M", "noM"])
def test_reference_accepts_a_plain_evaluation(dtype, kind, with_m):
    worst = 0.0
    for i, (k, q, w) in enumerate(SHAPES):
        N = (65, 257, 7, 600, 1030)[i]
        rows = max(k, q + w) + 1
        S, AS, MS, C, lam = lr.make_inputs(dtype, 2, rows, N, k, q, w, 10 + i, kind, with_m)
        ref = lr.rotate(S, AS, MS, C, lam, k, q, w, dtype)
        for reverse in (False, True):
            S1, AS1, MS1, Pn, Pm = _plain(S, AS, MS, C, lam, k, q, w, dtype, reverse)
            worst = max(worst, lr.check_all(ref, S1, AS1, MS1, Pn, Pm, q, w, what="%s %s" % (kind, (k, q, w))))
        if kind == "integer":
            for name, t in (("S", S1), ("AS", AS1), ("MS", MS1)):
                if t is not None:
                    assert torch.equal(lr.as_real64(t[:, :q]), ref.stacks[name][0])
            assert torch.equal(lr.as_real64(S1[:, q:q + w]), ref.resid[0])
        assert ref.nblk == -(-N // lr.chunk_elems(dtype))
    print("worst |err| / bound: %.3g" % worst)
    assert worst <= 1.0


# (conjugation is void for real coefficients: that fault is planted in the complex forms only)
FAULT_CASES = [(d, f) for d in DTYPES for f in lr.FAULTS if d.is_complex or f != "C_conjugated"]


@pytest.mark.parametrize("dtype,fault", FAULT_CASES, ids=["%s-%s" % (IDS[DTYPES.index(d)], f) for d, f in FAULT_CASES])
@pytest.mark.parametrize("with_m", [True, False], ids=["M", "noM"])
def test_planted_faults_are_rejected(dtype, fault, with_m):
    k, q, w, N = 9, 6, 3, 130
    S, AS, MS, C, lam = lr.make_inputs(dtype, 2, 10, N, k, q, w, 3, "randn", with_m)
    ref = lr.rotate(S, AS, MS, C, lam, k, q, w, dtype)
    good = lr.emulate(S, AS, MS, C, lam, k, q, w, dtype)
    lr.check_all(ref, *good, q, w, what="fault-free")
    S1, AS1, MS1, Pn, Pm = lr.emulate(S, AS, MS, C, lam, k, q, w, dtype, fault=fault)
    nbad_rows = lr.violates(S1[:, :q], *ref.stacks["S"]) + lr.violates(AS1[:, :q], *ref.stacks["AS"])
    nbad_res = lr.violates(S1[:, q:q + w], *ref.resid)
    if fault in ("C_transposed", "C_conjugated", "P_overwritten"):
        assert nbad_rows > 0 and nbad_res > 0 or fault == "P_overwritten" and nbad_rows > 0
    else:
        assert nbad_rows == 0 and nbad_res > 0            # the rotation is right, only the residual is not
    with pytest.raises(AssertionError):
        lr.check_all(ref, S1, AS1, MS1, Pn, Pm, q, w, what=fault)
    if fault in ("resid_old_X", "lam_wrong_column", "C_transposed", "C_conjugated"):
        assert lr.violates(Pn, *ref.pnorm) > 0            # and the partial sums of the wrong residual are caught too


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_chunks_are_the_library_s(dtype):
    """the reference cuts N into the chunks xk_lobpcg_blocks reports, and accepts no order beyond xk_lobpcg_max_rows"""
    from xitorch_amd import _capi
    esize = torch.empty((), dtype=dtype).element_size()
    for N in (1, 255, 256, 257, 1000, 1024, 1025, 4099):
        assert -(-N // lr.chunk_elems(dtype)) == _capi.fn("xk_lobpcg_blocks")(N, esize), N
    assert max(k for k, _, _ in SHAPES) <= _capi.fn("xk_lobpcg_max_rows")()


def test_nan_rows_beyond_k_are_not_read():
    dtype = torch.float64
    k, q, w, N = 6, 4, 2, 40
    S, AS, MS, C, lam = lr.make_inputs(dtype, 1, 9, N, k, q, w, 5)
    S[:, 7:] = float("nan")
    AS[:, 6:] = float("nan")
    ref = lr.rotate(S, AS, MS, C, lam, k, q, w, dtype)
    for v, b in list(ref.stacks.values()) + [ref.resid, ref.pnorm]:
        assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(b).all())
