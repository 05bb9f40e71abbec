"""The exact-spectrum matrices of jacobi_cases.py are what they claim to be, and CPU LAPACK in the test dtype, measured
against them, stays inside the ratios the GPU bounds of test_gpu_jacobi_kernel.py are multiples of (host only)."""
import json
import pytest
import torch
from tests import jacobi_cases as jc

F64 = torch.float64
DTYPES = [torch.float64, torch.float32]


def _all_cases(dtype):
    for fam in jc.FAMILIES:
        for k in jc.ORDERS:
            yield (fam, k, 0), jc.case(fam, k, dtype)
    for i, c in enumerate(jc.batch70(jc.BATCH70_ORDER, dtype)):
        yield (jc.FAMILIES[i % len(jc.FAMILIES)], jc.BATCH70_ORDER, "member %d of 70" % i), c
    for nb in jc.HIDDEN_BLOCKS:
        for uppest in (False, True):
            yield ("hidden", jc.HIDDEN_P + nb, uppest), jc.hidden(nb, dtype, uppest)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cases_are_exact(dtype):
    """T == T^T bitwise, T survives the rounding to the test dtype, and H^T T H / n == diag(d) bitwise — for every
    (family, order) the GPU test uses, the 70-member batch and the scaled cases included"""
    for tag, c in _all_cases(dtype):
        k = c.T.shape[0]
        assert torch.equal(c.T, c.T.T), tag
        assert torch.equal(c.T.to(dtype).double(), c.T), tag
        assert c.d.shape == (k,) and c.H.shape == (k, k) and c.n.shape == (k,), tag
        if tag[0] != "tridiagonal":
            D = (c.H.T @ c.T @ c.H) / c.n
            assert torch.equal(D, torch.diag(c.d)), tag
            assert torch.equal(c.H.T @ c.H, torch.diag(c.n)), tag
        else:
            # closed-form vectors in float64: the similarity holds to a few units of roundoff, not bitwise
            D = c.H.T @ c.T @ c.H
            assert (D - torch.diag(c.d)).abs().max().item() <= 64 * k * jc.unit_roundoff(F64), tag
    for fam in ("spread", "cluster"):
        for k in jc.SCALE_ORDERS:
            c = jc.case(fam, k, dtype)
            for e in jc.SCALE_EXPONENTS[dtype]:
                Ts = torch.ldexp(c.T, torch.tensor(e))
                assert torch.isfinite(Ts).all(), (fam, k, e)
                assert torch.equal(Ts.to(dtype).double(), Ts), (fam, k, e)
                assert torch.equal(torch.ldexp(Ts.to(dtype).double(), torch.tensor(-e)), c.T), (fam, k, e)


def test_families_hold_what_they_promise():
    """the multiplicities, the cluster and the edge gap are where the GPU test expects them"""
    for dtype in DTYPES:
        h = 2.0 ** -jc.cluster_bits(dtype)
        d = jc.case("multiple", 45, dtype).d
        assert jc.wanted(d, 6, False)[2] == 1.0 and jc.wanted(d, 1, False)[2] == 0.0      # p % 3 != 0 straddles a triple
        d = jc.case("edgegap", 45, dtype).d
        assert jc.wanted(d, 6, False)[2] == h
        d = jc.case("cluster", 45, dtype).d
        assert jc.wanted(d, 1, False)[2] == h and jc.wanted(d, 6, False)[2] == 1.0
        d = jc.case("diagonal", 45, dtype).d
        assert not torch.equal(torch.sort(d).values, d) and torch.unique(d).numel() < d.numel()
        for nb in jc.HIDDEN_BLOCKS:
            for uppest in (False, True):
                c = jc.hidden(nb, dtype, uppest)
                sgn = -1.0 if uppest else 1.0
                diag = torch.diagonal(c.T) * sgn
                lone = (c.T - torch.diag(torch.diagonal(c.T))).abs().sum(1) == 0       # rows without off-diagonals
                assert int(lone.sum()) == jc.HIDDEN_P and bool((diag[lone] == 1).all()) and bool((diag[~lone] > 1).all())
                assert float((c.d * sgn).min()) == 1 - h and jc.wanted(c.d, jc.HIDDEN_P, uppest)[2] == 0.0
    assert jc.blocks(45) == [32, 8, 4, 1] and jc.blocks(128) == [128] and jc.blocks(1) == [1]
    for k in jc.ORDERS:
        assert sorted(jc.interleave(k).tolist()) == list(range(k))
    assert len({(float(c.d[0]), float(c.d[-1]), float(c.T[0, -1])) for c in jc.batch70(jc.BATCH70_ORDER, F64)}) == 70


@pytest.mark.parametrize("dtype", DTYPES)
def test_lapack_ratios_in_the_test_dtype(dtype):
    """torch.linalg.eigh in the test dtype against the exact spectra, in the units of jacobi_cases.ratios: the worst
    ratios are printed and must not exceed LAPACK_RATIO, the measurement the kernel's bounds rest on"""
    worst, where = {}, {}
    todo = [((fam, k), jc.case(fam, k, dtype), jc.wanted_counts(k), (False, True))
            for fam in jc.FAMILIES for k in jc.ORDERS]
    todo += [(("hidden", jc.HIDDEN_P + nb), jc.hidden(nb, dtype, uppest), [jc.HIDDEN_P], (uppest,))
             for nb in jc.HIDDEN_BLOCKS for uppest in (False, True)]
    for tag, c, counts, ends in todo:
        k = c.T.shape[0]
        lam, V = torch.linalg.eigh(c.T.to(dtype))
        lam, V = lam.double(), V.double()
        for p in counts:
            for uppest in ends:
                sl = slice(k - p, k) if uppest else slice(0, p)
                r = jc.ratios(c.T, lam[sl], V[:, sl].T.contiguous(), c, p, uppest, dtype)
                for q, v in r.items():
                    if v is not None and v > worst.get(q, -1.0):
                        worst[q], where[q] = v, tag + (p, uppest)
    print("LAPACK %s worst ratios: %s at %s" % (dtype, json.dumps(worst), where))
    for q, v in worst.items():
        assert v <= jc.LAPACK_RATIO[q][dtype], (q, v, where[q])
