"""The exact-spectrum cases of ritz_cases.py are what they claim to be at every order of every form, LAPACK's ?syevx
in the test dtype stays inside the EVX_RATIO the GPU bounds of test_gpu_ritz_kernels.py are multiples of, the
batch-crossing wanted counts cross, and the scale exponents lie on the side of the kernels' range that they claim
(host only)."""
import json
import pytest
import torch
from tests import jacobi_cases as jc
from tests import ritz_cases as rc
from xitorch_amd._capi import fn

F64 = torch.float64
DTYPES = [torch.float64, torch.float32]


@pytest.mark.parametrize("dtype", DTYPES)
def test_cases_are_exact(dtype):
    """T == T^T bitwise and T survives the rounding to the test dtype, for every (family, order) of every form, the
    70-member batches and the scaled cases; up to order 257 also H^T T H / n == diag(d) bitwise (beyond that the
    generator's argument stands: every partial sum of the product is exact)"""
    for k in rc.all_orders(dtype):
        for fam in rc.FAMILIES:
            c = rc.case(fam, k, dtype)
            tag = (fam, k)
            rc.assert_exact(c, dtype, tag)
            assert c.d.shape == (k,) and c.H.shape == (k, k) and c.n.shape == (k,), tag
            if fam in rc.HADAMARD and k <= 257:
                assert torch.equal((c.H.T @ c.T @ c.H) / c.n, torch.diag(c.d)), tag
                assert torch.equal(c.H.T @ c.H, torch.diag(c.n)), tag
            if fam in jc.HADAMARD and k <= 128:                    # the Jacobi cases themselves up to their orders
                assert torch.equal(c.T, jc.case(fam, k, dtype).T), tag
    for k in sorted(set(rc.BATCH70_ORDER.values())):
        for i, c in enumerate(jc.batch70(k, dtype)):
            rc.assert_exact(c, dtype, ("batch70", k, i))
    for form in rc.FORMS:
        for k in rc.scale_orders(form, dtype):
            for fam in rc.SCALE_FAMILIES:
                c = rc.case(fam, k, dtype)
                for e in rc.SCALE_EXPONENTS[dtype]["in"] + rc.SCALE_EXPONENTS[dtype]["out"]:
                    Ts = torch.ldexp(c.T, torch.tensor(e))
                    assert torch.isfinite(Ts).all(), (fam, k, e)
                    assert torch.equal(torch.ldexp(Ts.to(dtype).double(), torch.tensor(-e)), c.T), (fam, k, e)


def test_families_hold_what_they_promise():
    for dtype in DTYPES:
        for k in (129, 257, 1025):
            h = 2.0 ** -rc.cluster_bits(k, dtype)
            assert h <= 2.0 ** -6
            assert jc.wanted(rc.spectrum("cluster", k, dtype), 1, False)[2] == h
            assert jc.wanted(rc.spectrum("cluster", k, dtype), 4, False)[2] > 0.5
            assert jc.wanted(rc.spectrum("edgegap", k, dtype), 6, False)[2] == h
            d = rc.spectrum("multiple64", k, dtype)
            assert jc.wanted(d, 6, False)[2] == 0.0 and jc.wanted(d, 64, False)[2] == 1.0
            assert int((d == 0).sum()) == 64 and int((d == d.max()).sum()) == (k - 1) % 64 + 1
        # 2^a + 1: the last block of the decomposition is a decoupled 1 x 1
        assert jc.blocks(1025) == [1024, 1]
        c = rc.case("spread", 1025, dtype)
        lone = (c.T - torch.diag(torch.diagonal(c.T))).abs().sum(1) == 0
        assert int(lone.sum()) >= 1
    assert len(rc.FAMILIES) == 9 and set(rc.XFLAG) <= {(f, d) for f in rc.FORMS for d in ("float64", "float32")}


@pytest.mark.parametrize("dtype", DTYPES)
def test_orders_and_wanted_counts(dtype):
    """the table of the forms' orders, and per order: p = 1, p = 6, a batch-crossing p picked with the library's host
    function (pb < p, ragged tail where more than one shift fits), min(k, 256) at two orders per K3g form, min(k, 16)
    for tri — each accepted by the library's own predicate"""
    big_batch = fn("xk_small_eigh_big_batch")
    es = 8 if dtype == F64 else 4
    assert set(rc.handover_orders(dtype)) <= set(rc.orders("persist", dtype))
    assert (1025 in rc.orders("step", dtype)) and max(rc.orders("step", dtype)) == (1536 if dtype == F64 else 1500)
    crossing = 0
    for form in rc.FORMS:
        for k in rc.orders(form, dtype):
            ps = rc.wanted_counts(form, k, dtype)
            assert ps and ps[0] == 1, (form, k)
            if form == "tri":
                assert all(rc.tri_ok(k, p, dtype) for p in ps)
                assert min(k, 16) in ps or not rc.tri_ok(k, min(k, 16), dtype)
                continue
            assert all(rc.big_ok(k, p, dtype) for p in ps), (form, k)
            assert 6 in ps or k < 6
            pc = rc.cross_p(k, dtype)
            if pc is None:                                   # every p fits one batch at this order
                assert big_batch(k, min(k, 256), es) == min(k, 256), (form, k)
                continue
            pb = big_batch(k, pc, es)
            assert pc in ps and 0 < pb < pc, (form, k, pc, pb)
            assert pc % pb != 0 or pb == 1, (form, k, pc, pb)         # ragged, unless one shift per batch is all that fits
            crossing += 1
        if form != "tri":
            assert len(rc.WIDE_ORDERS[form]) == 2
            for k in rc.WIDE_ORDERS[form]:
                assert min(k, 256) in rc.wanted_counts(form, k, dtype), (form, k)
    assert crossing >= 20
    if dtype == F64:
        assert big_batch(1536, 2, 8) == 1 and rc.cross_p(1536, dtype) > 1       # any p > 1 crosses there


@pytest.mark.parametrize("dtype", DTYPES)
def test_scale_exponents_lie_on_their_side(dtype):
    """the kernels' tnorm is the Gershgorin bound of the tridiagonal, in [|T|, 3 |T|]: an in-range exponent keeps even
    3 |d| 2^e inside the limit (and |d| 2^e inside the lower one), an out-of-range exponent puts |d| 2^e beyond it"""
    lim = rc.SCALE_LIMIT[dtype]
    for form in rc.FORMS:
        for k in rc.scale_orders(form, dtype):
            assert k in rc.orders(form, dtype) and rc.scale_p(form, k, dtype) >= 1
            for fam in rc.SCALE_FAMILIES:
                nd = float(rc.case(fam, k, dtype).d.abs().max())
                for e in rc.SCALE_EXPONENTS[dtype]["in"]:
                    assert rc.exponent(3 * nd) + e <= lim and rc.exponent(nd) + e >= -lim, (form, k, fam, e)
                for e in rc.SCALE_EXPONENTS[dtype]["out"]:
                    assert abs(rc.exponent(nd) + e) > lim, (form, k, fam, e)


@pytest.mark.parametrize("dtype", DTYPES)
def test_syevx_ratios_in_the_test_dtype(dtype):
    """?syevx in the test dtype against the exact spectra on ritz_cases.calibration_plan, in the units of
    jacobi_cases.ratios: the worst ratios per band of orders are printed and must not exceed EVX_RATIO"""
    scipy_linalg = pytest.importorskip("scipy.linalg")
    worst, where, outliers = {}, {}, 0
    for k, fams, todo in rc.calibration_plan(dtype):
        for fam in fams:
            c = rc.case(fam, k, dtype)
            A = c.T.to(dtype).numpy()
            for p, uppest in todo:
                lo = k - p if uppest else 0
                w, v = scipy_linalg.eigh(A, lower=True, driver="evx", subset_by_index=(lo, lo + p - 1),
                                         check_finite=False)
                lam = torch.from_numpy(w).double()
                Y = torch.from_numpy(v).double().T.contiguous()
                r = rc.ratios(c.T, lam, Y, c, p, uppest, dtype)
                if (str(dtype).replace("torch.", ""), fam, k, p, uppest) in rc.EVX_OUTLIERS:
                    print("left out of the yardstick:", fam, k, p, uppest, r)
                    outliers += 1
                    continue
                for q, val in r.items():
                    key = (q, rc.band(k))
                    if val is not None and val > worst.get(key, -1.0):
                        worst[key], where[key] = val, (fam, k, p, uppest)
    print("?syevx %s worst ratios: %s" % (dtype, json.dumps({"%s/band%d" % key: round(v, 4) for key, v in sorted(worst.items())})))
    print("at:", {"%s/band%d" % key: v for key, v in sorted(where.items())})
    assert {b for _, b in worst} == {0, 1, 2}
    assert outliers == sum(1 for o in rc.EVX_OUTLIERS if o[0] == str(dtype).replace("torch.", ""))
    for (q, b), v in worst.items():
        assert v <= rc.EVX_RATIO[q][dtype][b], (q, b, v, where[(q, b)])
