"""CPU: the Hermitian-kernel checker of tests/herm_ref.py agrees with independent torch expressions, accepts a correct
output rounded to the kernel dtype, and rejects every fault of herm_ref.FAULTS at the shapes and with the inputs of
tests/test_gpu_herm_kernels.py -- the evidence that the GPU tests would fail on a subtly wrong kernel.  It also asserts
the conditioning premise of the per-entry CholeskyQR family: kappa_2(G) <= KAPPA2_MAX for every one of its cases, so that
no per-entry comparison is silently left out on the GPU."""
import math
import pytest
import torch
from tests import herm_ref as hr

c128, c64 = hr.c128, hr.c64
DTYPES = [c128, c64]
IDS = ["c128", "c64"]

RITZ_FAULTS = ("chunk_y", "chunk_lam", "chunk_out", "y_transposed", "lam_x", "tn_sign", "conj_y", "drop_last_block",
               "status_nan_dropped", "status_wrong_member")
APPLY_FAULTS = ("mw_not_transformed", "rinv_transposed")
GRAM_FAULTS = ("gram_no_conj", "no_shift", "gram_drop_256", "gram_drop_512", "drop_tail_chunk")
EIGH_FAULTS = ("upper_read", "imag_diag_used", "uppest_lowest", "y_conj")
OUTER_FAULTS = ("outer_no_conj",)


def test_every_fault_has_a_rejection_test():
    assert set(RITZ_FAULTS + APPLY_FAULTS + GRAM_FAULTS + EIGH_FAULTS + OUTER_FAULTS) == set(hr.FAULTS)
    assert len(set(hr.FAULTS)) == len(hr.FAULTS)


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------ Ritz
def _ritz_applies(fault, B, k, p, N, with_m):
    return {"chunk_y": p > hr.RITZ_PC, "chunk_lam": p > hr.RITZ_PC, "chunk_out": p > hr.RITZ_PC,
            "y_transposed": min(k, p) > 1, "lam_x": with_m, "drop_last_block": N % 256 != 0,
            "status_wrong_member": B > 1}.get(fault, True)


_plant = hr.ritz_plant


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ritz_restatement_vs_einsum_and_accepted(dtype):
    for k in (5, 40):
        for (B, k, p, N, with_m, _) in hr.ritz_configs(k):
            c = hr.ritz_case(dtype, B, k, p, N, with_m)
            ref = hr.ritz(c["V"], c["AV"], c["MV"], c["Y"], c["lam"], dtype)
            Yt = c["Y"].transpose(1, 2)
            X = torch.matmul(Yt, c["V"])
            R = torch.matmul(Yt, c["AV"]) - c["lam"].unsqueeze(-1) * torch.matmul(Yt, c["MV"] if with_m else c["V"])
            scale = k * 1e-14
            assert (ref["X"][0] - X).abs().max().item() <= scale * 10
            assert (ref["Tn"][0] + R).abs().max().item() <= scale * 100
            rm = R.abs().flatten(1).max(1).values
            assert (ref["status"][0][1:] - rm).abs().max().item() <= scale * 100
            assert hr.status_consistent(ref["status"][0])
            assert hr.check(hr.values(ref, dtype), ref, dtype, what="accept") <= 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fault", RITZ_FAULTS)
def test_ritz_fault_rejected(dtype, fault):
    seen = 0
    for k in (5,):
        for (B, k, p, N, with_m, _) in hr.ritz_configs(k):
            if not _ritz_applies(fault, B, k, p, N, with_m):
                continue
            c = hr.ritz_case(dtype, B, k, p, N, with_m)
            if fault == "status_nan_dropped":
                c = _plant(c, math.nan)
            args = (c["V"], c["AV"], c["MV"], c["Y"], c["lam"], dtype)
            ref = hr.ritz(*args)
            bad = hr.values(hr.ritz(*args, fault=fault), dtype)
            what = "%s %s" % (fault, (B, k, p, N, with_m))
            assert _rejected(lambda: hr.check(bad, ref, dtype, what=what)), what
            seen += 1
    assert seen >= 10


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("value", [math.nan, math.inf])
def test_ritz_non_finite_status(dtype, value):
    B, k, p, N = 3, 5, 17, 257
    c = _plant(hr.ritz_case(dtype, B, k, p, N, True), value)
    st = hr.ritz(c["V"], c["AV"], c["MV"], c["Y"], c["lam"], dtype)["status"][0]
    same = torch.isnan if math.isnan(value) else torch.isinf
    assert bool(same(st[0])) and bool(same(st[B])) and bool(torch.isfinite(st[1:B]).all())
    assert hr.status_consistent(st)
    wrong = st.clone()
    wrong[0] = st[1:B].max()
    assert not hr.status_consistent(wrong)


# ------------------------------------------------------------------------------------------------ CholeskyQR
def _chol_inputs(dtype, q, N, with_m, shifted, kind="gauss"):
    c = hr.cholqr_case(dtype, q, N, with_m, kind)
    sh = hr.cast(hr.shift_rel(N, q, dtype), dtype) if shifted else 0.0
    return c["W"], c["MW"], sh


@pytest.mark.parametrize("N", hr.CHOL_N + (33,))
def test_cholqr_per_entry_family_is_well_conditioned(N):
    """the premise of the per-entry comparison, for EVERY case of it and both dtypes"""
    worst = 0.0
    for dtype in DTYPES:
        for (q, N, with_m, shifted) in hr.cholqr_entry_configs(N):
            W, MW, sh = _chol_inputs(dtype, q, N, with_m, shifted)
            k2 = hr.kappa2(hr.cholqr_gram(W, MW, sh, dtype)).max().item()
            assert k2 <= hr.KAPPA2_MAX[hr.REAL[dtype]], (hr.DNAME[dtype], q, N, with_m, shifted, k2)
            worst = max(worst, k2)
    print("N = %d: worst kappa_2(G) %.1f" % (N, worst))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", [64, 257, 777])
def test_cholqr_restatement_vs_torch_and_accepted(dtype, N):
    for (q, N, with_m, shifted) in hr.cholqr_entry_configs(N):
        W, MW, sh = _chol_inputs(dtype, q, N, with_m, shifted)
        ref = hr.cholqr_factor(W, MW, sh, dtype)
        G = ref["_meta"]["G"]
        Gt = torch.einsum("bin,bjn->bij", W.conj(), W if MW is None else MW)
        Gt = Gt + sh * torch.diagonal(Gt, dim1=1, dim2=2).real.sum(-1).view(-1, 1, 1) * torch.eye(q, dtype=c128)
        assert (G - Gt).abs().max().item() <= 1e-5 * N           # (MW is M W only to the rounding of the kernel dtype)
        R, bad = hr.herm_chol(G)
        assert int(bad.max()) == 0
        Lt = torch.linalg.cholesky(G)
        assert (R - Lt.transpose(1, 2).conj()).abs().max().item() <= 1e-10 * N ** 0.5
        Rinv = ref["Rinv"][0]
        E = torch.matmul(Rinv.transpose(1, 2).conj(), torch.matmul(G, Rinv)) - torch.eye(q, dtype=c128)
        assert E.abs().max().item() <= 1e-11
        got = hr.rnd(Rinv, dtype)
        assert hr.check({"Rinv": got}, ref, dtype, what="accept") <= 1.0
        hr.cholqr_properties(got, G, N, dtype, kernel="accept")
        ap = hr.cholqr_apply(W, MW, got, dtype)
        Q = torch.matmul(torch.triu(got).transpose(1, 2), W)
        assert (ap["W"][0] - Q).abs().max().item() <= 1e-12 * q
        assert hr.check(hr.values(ap, dtype), ap, dtype, what="accept") <= 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fault", APPLY_FAULTS)
def test_cholqr_apply_fault_rejected(dtype, fault):
    for N in (64, 257, 777):
        for (q, N, with_m, shifted) in hr.cholqr_entry_configs(N):
            if q < 2 or (fault == "mw_not_transformed" and not with_m):
                continue
            W, MW, sh = _chol_inputs(dtype, q, N, with_m, shifted)
            Rinv = hr.rnd(hr.cholqr_factor(W, MW, sh, dtype)["Rinv"][0], dtype)
            ref = hr.cholqr_apply(W, MW, Rinv, dtype)
            bad = hr.values(hr.cholqr_apply(W, MW, Rinv, dtype, fault=fault), dtype)
            what = "%s %s" % (fault, (q, N, with_m, shifted))
            assert _rejected(lambda: hr.check(bad, ref, dtype, what=what)), what


def _gram_applies(fault, q, N, shifted):
    ne = q * (q + 1) // 2
    return {"no_shift": shifted, "gram_drop_256": ne > 256, "gram_drop_512": ne > 512,
            "drop_tail_chunk": N % hr.CHOL_CH != 0, "gram_no_conj": q >= 1}[fault]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fault", GRAM_FAULTS)
def test_cholqr_gram_fault_rejected(dtype, fault):
    """by the per-entry comparison of Rinv or by the properties, as the GPU test applies them"""
    seen = 0
    for N in (64, 255, 257, 777):
        for (q, N, with_m, shifted) in hr.cholqr_entry_configs(N):
            if not _gram_applies(fault, q, N, shifted):
                continue
            if fault == "no_shift" and q < 17:
                continue          # the driver's shift of a narrow block is below the bound: not detectable, nor harmful
            W, MW, sh = _chol_inputs(dtype, q, N, with_m, shifted)
            ref = hr.cholqr_factor(W, MW, sh, dtype)
            bad = hr.rnd(hr.cholqr_factor(W, MW, sh, dtype, fault=fault)["Rinv"][0], dtype)
            what = "%s %s" % (fault, (q, N, with_m, shifted))

            def both():
                hr.check({"Rinv": bad}, ref, dtype, what=what)
                hr.cholqr_properties(bad, ref["_meta"]["G"], N, dtype, what=what, kernel="fault")
            assert _rejected(both), what
            seen += 1
    assert seen >= 4


# ------------------------------------------------------------------------------------------------ eigh
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [1, 2, 7, 33, 64])
def test_eigh_model_accepted(dtype, n):
    for kind in hr.EIGH_KINDS:
        T = hr.eigh_case(dtype, kind, n)
        if T is None:
            continue
        A = hr.contracted(T)
        assert bool(torch.isfinite(torch.view_as_real(A)).all())
        assert (A - A.transpose(-2, -1).conj()).abs().max().item() == 0
        assert bool((torch.diagonal(A, dim1=-2, dim2=-1).imag == 0).all())
        for p in hr.EIGH_P:
            for uppest in (False, True):
                if p > n:
                    continue
                lam, Y = hr.eigh_model(T, p, uppest)
                ev = torch.linalg.eigvalsh(A)
                assert (lam - (ev[:, n - p:] if uppest else ev[:, :p])).abs().max().item() <= 1e-12 * ev.abs().max().item()
                hr.eigh_check(T, hr.rnd(lam, dtype), hr.rnd(Y, dtype), p, uppest, dtype, what="accept")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fault", EIGH_FAULTS)
def test_eigh_fault_rejected(dtype, fault):
    for n in (7, 33, 64):
        for kind in ("generic", "cluster", "imaginary"):
            T = hr.eigh_case(dtype, kind, n, garbage="finite" if fault == "upper_read" else "nan")
            for p in (1, 6):
                for uppest in (False, True):
                    if fault == "uppest_lowest" and not uppest:
                        continue
                    lam, Y = hr.eigh_model(T, p, uppest, fault=fault)
                    what = "%s %s" % (fault, (kind, n, p, uppest))
                    assert _rejected(lambda: hr.eigh_check(T, hr.rnd(lam, dtype), hr.rnd(Y, dtype), p, uppest, dtype,
                                                           what=what)), what


# ------------------------------------------------------------------------------------------------ dense_outer_complex
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_outer_restatement_and_fault(dtype):
    for B in hr.OUTER_B:
        for C in hr.OUTER_C:
            for (M, N) in hr.OUTER_MN:
                U, W = hr.outer_case(dtype, B, C, M, N)
                ref = hr.dense_outer_complex(U, W, dtype)
                G = torch.einsum("bci,bcj->bij", U, W.conj())
                val = torch.view_as_complex(ref["G"][0].reshape(B, M, N, 2).contiguous())
                assert (val - G).abs().max().item() <= 1e-13 * C
                assert hr.check(hr.values(ref, dtype), ref, dtype, what="accept") <= 1.0
                bad = hr.values(hr.dense_outer_complex(U, W, dtype, fault="outer_no_conj"), dtype)
                assert _rejected(lambda: hr.check(bad, ref, dtype, what="outer_no_conj"))
