"""CPU: the band-pass filter of symeig(mode="nearest") — the driver's coefficient table (host_eig.chebwin_coefficients)
run through the driver's Clenshaw loop against the closed form, the degree rule against its plain statement, and the
planted faults of tests/chebwin_ref.py against its own bound.

Grid of the closed-form comparison.  The recurrence sees t = (lambda - c) / e, the closed form theta = acos t; a
rounding u of t moves T_k(t) by k u / sin(theta), which near the ends of the interval (sin theta -> 0, slope k^2) is a
property of the polynomial and not an error of either evaluation.  So the eigenvalues are placed at lambda = c + e cos
(theta) for angles 0.1 <= theta <= pi - 0.1 plus the two ends themselves (t = +-1 exactly, where nothing is rounded),
on intervals whose c, 1 / e and c / e are exact in binary.  The centres theta_s in {0, 0.3, pi / 2, pi} are the issue's.
"""
import math
import pytest
import torch
from tests import chebwin_ref as wref
from xitorch_amd.linalg import host_eig

DEGREES = [1, 2, 8, 20, 317, 1000]
CENTRES = [0.0, 0.3, math.pi / 2, math.pi]
INTERVALS = [(-1.0, 1.0), (-3.0, 5.0)]


def _grid():
    th = torch.linspace(0.1, math.pi - 0.1, 301, dtype=torch.float64)
    return torch.cat((torch.tensor([0.0], dtype=torch.float64), th, torch.tensor([math.pi], dtype=torch.float64)))


def _table(lo, hi, theta_s, m):
    """the driver's table for one operator and the centre angle it actually uses (sigma_c is rounded once)"""
    c, e = 0.5 * (hi + lo), 0.5 * (hi - lo)
    sigma_c = torch.tensor(c + e * math.cos(theta_s), dtype=torch.float64)
    tab = host_eig.chebwin_coefficients(torch.tensor(lo, dtype=torch.float64), torch.tensor(hi, dtype=torch.float64),
                                        sigma_c, m)
    used = float(torch.acos(torch.clamp((sigma_c - c) / e, -1.0, 1.0)))
    return tab, used, float(sigma_c), c, e


@pytest.mark.parametrize("m", DEGREES)
@pytest.mark.parametrize("theta_s", CENTRES)
def test_clenshaw_with_the_drivers_table_is_the_closed_form(m, theta_s):
    for lo, hi in INTERVALS:
        tab, used, sigma_c, c, e = _table(lo, hi, theta_s, m)
        assert tab.shape == (m + 1, 4) and tab.dtype == torch.float64
        th = _grid()
        lam = c + e * torch.cos(th)
        lam[0], lam[-1] = hi, lo
        got = wref.clenshaw(tab, lambda v: lam * v, torch.ones_like(lam))
        want = wref.filter_closed_form(th, used, m)
        err = float((got - want).abs().max())
        print("m=%d theta_s=%.3f [%g, %g]: max |clenshaw - closed form| = %.3e (bound %.3e)"
              % (m, theta_s, lo, hi, err, wref.chebyshev_bound(m)))
        assert err <= wref.chebyshev_bound(m) * float(want.abs().max())
        # p(t(sigma_c)) = 1
        one = wref.clenshaw(tab, lambda v: sigma_c * v, torch.ones((1,), dtype=torch.float64))
        assert abs(float(one) - 1.0) <= wref.chebyshev_bound(m)


def test_table_layout():
    """row 0 = (0, c_m, 0, 0); row 1 has gamma = 0 (b_{m+1} = 0 is not read); the last row carries 1 / e, the others
    2 / e; delta of row j is c_{m-j}"""
    m, lo, hi, th = 8, -3.0, 5.0, 0.3
    tab, used, _, c, e = _table(lo, hi, th, m)
    g = wref.jackson(m)
    mu = [(1.0 if k == 0 else 2.0) * math.cos(k * used) for k in range(m + 1)]
    norm = sum(g[k] * mu[k] * math.cos(k * used) for k in range(m + 1))
    ck = [g[k] * mu[k] / norm for k in range(m + 1)]
    assert tab[0].tolist() == pytest.approx([0.0, ck[m], 0.0, 0.0], rel=1e-13, abs=1e-15)
    for j in range(1, m + 1):
        s = (1.0 if j == m else 2.0) / e
        assert tab[j].tolist() == pytest.approx([s, -s * c, 0.0 if j == 1 else -1.0, ck[m - j]], rel=1e-13, abs=1e-15)
    assert float(tab[1, 2]) == 0.0


def test_flat_spectrum_gets_the_identity_and_batches_are_independent():
    lo = torch.tensor([2.0, -1.0], dtype=torch.float64)
    hi = torch.tensor([2.0, 1.0], dtype=torch.float64)
    sc = torch.tensor([2.0, 0.25], dtype=torch.float64)
    tab = host_eig.chebwin_coefficients(lo, hi, sc, 5)
    assert tab.shape == (6, 2, 4)
    X = torch.tensor([0.7, -1.3], dtype=torch.float64)
    assert torch.equal(wref.clenshaw(tab[:, 0], lambda v: 2.0 * v, X), X)
    single = host_eig.chebwin_coefficients(lo[1], hi[1], sc[1], 5)
    assert torch.allclose(tab[:, 1], single, rtol=1e-13, atol=1e-15)     # (vectorised cos may differ in the last bit)


@pytest.mark.parametrize("m", DEGREES)
def test_filter_is_non_negative(m):
    th = torch.linspace(0.0, math.pi, 2001, dtype=torch.float64)
    lam = torch.cos(th)
    for theta_s in CENTRES + [1.1, 2.9]:
        tab, _, _, _, _ = _table(-1.0, 1.0, theta_s, m)
        p = wref.clenshaw(tab, lambda v: lam * v, torch.ones_like(lam))
        assert float(p.min()) >= -1e-12, (m, theta_s, float(p.min()))


def test_jackson_coefficients():
    for m in (1, 8, 317):
        assert host_eig.chebwin_jackson(m).tolist() == pytest.approx(wref.jackson(m), rel=1e-14, abs=1e-16)
        assert wref.jackson(m)[0] == pytest.approx(1.0, abs=1e-15)


def test_ladder():
    assert wref.ladder(1000)[:6] == [8, 11, 14, 18, 23, 29] and wref.ladder(1000)[-1] == 1000
    for md in (1000, 50, 8, 5, 12):
        assert host_eig.chebwin_ladder(md) == wref.ladder(md)
        assert max(host_eig.chebwin_ladder(md)) == md


@pytest.mark.parametrize("theta_s", [0.0, 0.3, 1.2, math.pi / 2, 3.0, math.pi])
def test_degree_rule_takes_the_smallest_admissible_degree(theta_s):
    for d in (1.0, 0.4, 0.12, 0.03, 0.011):
        for tail in (0.1, 0.03):
            want = wref.degree_rule(theta_s, d, tail, 1000)
            got = host_eig.chebwin_degree(torch.tensor([theta_s], dtype=torch.float64),
                                          torch.tensor([d], dtype=torch.float64), tail, 1000)
            assert got == want, (theta_s, d, tail, got, want)
            m, capped = got
            if not capped:
                lad = wref.ladder(1000)
                assert m in lad
                if m > lad[0]:                 # the degree below it on the ladder is not admissible
                    below = lad[lad.index(m) - 1]
                    p = wref.filter_closed_form(torch.tensor([theta_s + d, theta_s - d]), theta_s, below)
                    assert float(p.abs().max()) > tail


def test_degree_rule_respects_max_degree_and_batches_take_the_largest():
    ts = torch.tensor([1.0], dtype=torch.float64)
    assert host_eig.chebwin_degree(ts, torch.tensor([1e-4], dtype=torch.float64), 0.1, 1000) == (1000, True)
    assert host_eig.chebwin_degree(ts, torch.tensor([0.03], dtype=torch.float64), 0.1, 50) == (50, True)
    assert host_eig.chebwin_degree(ts, torch.tensor([1.0], dtype=torch.float64), 0.1, 50) == (8, False)
    assert host_eig.chebwin_degree(ts, torch.tensor([1.0], dtype=torch.float64), 0.1, 5) == (5, True)
    d = torch.tensor([1.0, 0.12, 0.4], dtype=torch.float64)
    each = [host_eig.chebwin_degree(ts, d[i:i + 1], 0.1, 1000)[0] for i in range(3)]
    assert host_eig.chebwin_degree(ts.expand(3), d, 0.1, 1000) == (max(each), False)
    assert each[1] > each[2] >= each[0]


DTYPES = [torch.float64, torch.float32, torch.complex128, torch.complex64]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32", "c128", "c64"])
def test_reference_accepts_itself_and_rejects_every_planted_fault(dtype):
    AY, Y, Yp, X0, coef = wref.make_inputs(dtype, 3, 5, 65, seed=3)
    value, bound = wref.step(AY, Y, Yp, X0, coef, dtype)
    rd = wref.REAL_OF[dtype]
    # the straightforward evaluation in the kernel's own arithmetic passes
    c = wref.rounded_coef(coef, dtype).to(rd)
    al, be, ga, de = (c[:, i].reshape(-1, 1, 1) for i in range(4))
    plain = ((al * AY + be * Y) + ga * Yp) + de * X0
    wref.check(plain, value, bound, "plain evaluation")
    for fault in wref.FAULTS:
        wrong, _ = wref.step(AY, Y, Yp, X0, coef, dtype, fault=fault)
        got = wrong.to(rd)
        if dtype.is_complex:
            got = torch.view_as_complex(got.reshape(3, 5, 65, 2).contiguous())
        assert wref.violates(got, value, bound) > 0.9 * value.numel(), fault


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32", "c128", "c64"])
def test_gamma_zero_leaves_yprev_unread_and_integers_are_exact(dtype):
    AY, Y, Yp, X0, coef = wref.make_inputs(dtype, 2, 3, 17, seed=5, kind="integer")
    coef[0, 2], coef[1, 2] = 0.0, -0.0
    Yp = torch.full_like(Yp, wref.nan_of(dtype))
    value, bound = wref.step(AY, Y, Yp, X0, coef, dtype)
    assert bool(torch.isfinite(value).all()) and bool(torch.isfinite(bound).all())
    al, be, de = (coef[:, i].reshape(-1, 1, 1) for i in (0, 1, 3))
    exact = wref.as_real64(AY) * al + wref.as_real64(Y) * be + wref.as_real64(X0) * de
    assert torch.equal(value, exact) and float(value.lo.abs().max()) == 0.0
