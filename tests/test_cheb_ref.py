"""CPU: tests/cheb_ref.py states what xk_cheb_step computes, its bound rejects planted faults, and the coefficient table
of the driver (`host_eig.cheb_coefficients`) reproduces the scaled Chebyshev polynomial."""
import pytest
import torch
from tests import cheb_ref as cref
from xitorch_amd.linalg.host_eig import cheb_coefficients

DTYPES = [torch.float64, torch.float32, torch.complex128, torch.complex64]
IDS = ["f64", "f32", "c128", "c64"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["randn", "graded", "cancel", "integer"])
def test_restatement_against_plain_float64(dtype, kind):
    """the restatement is the formula: against plain torch in float64 / complex128 with the rounded coefficients it
    agrees to float64 rounding (far inside its own bound for the 32-bit forms)"""
    AY, Y, Yp, coef = cref.make_inputs(dtype, 3, 5, 67, seed=11, kind=kind)
    value, bound = cref.step(AY, Y, Yp, coef, dtype)
    c = cref.rounded_coef(coef, dtype)
    wide = torch.complex128 if dtype.is_complex else torch.float64
    plain = c[:, 0].reshape(-1, 1, 1) * AY.to(wide) + c[:, 1].reshape(-1, 1, 1) * Y.to(wide) \
        + c[:, 2].reshape(-1, 1, 1) * Yp.to(wide)
    terms = cref.as_real64((c[:, 0].abs().reshape(-1, 1, 1) * AY.to(wide).abs()
                            + c[:, 1].abs().reshape(-1, 1, 1) * Y.to(wide).abs()
                            + c[:, 2].abs().reshape(-1, 1, 1) * Yp.to(wide).abs()).to(wide))
    # (|re|, |im| <= modulus: the modulus of the term sum bounds both components; complex -> interleaved with zeros)
    if dtype.is_complex:
        terms = terms.reshape(*terms.shape[:-1], -1, 2)[..., 0].repeat_interleave(2, dim=-1)
    err = (cref.as_real64(plain.to(wide)) - value).abs()
    assert bool((err <= 4 * 2.0 ** -53 * terms + 1e-300).all())
    # the error-free low part is a rounding-sized correction of the high part (three product errors and two sum errors of
    # at most u each: 5 u of the term sum; 6 u allows for its own evaluation)
    assert bool((value.lo.abs() <= 6 * 2.0 ** -53 * terms + 1e-300).all())
    nround = 5.0 if cref.REAL_OF[dtype] == torch.float32 else 4.0
    comp = cref.as_real64(AY).abs() * c[:, 0].abs().reshape(-1, 1, 1) + cref.as_real64(Y).abs() * \
        c[:, 1].abs().reshape(-1, 1, 1) + cref.as_real64(Yp).abs() * c[:, 2].abs().reshape(-1, 1, 1)
    tiny = torch.finfo(cref.REAL_OF[dtype]).tiny
    assert bool(((bound - tiny) <= nround * cref.unit_roundoff(dtype) * comp * (1 + 1e-12)).all())
    assert bool(((bound - tiny) >= nround * cref.unit_roundoff(dtype) * comp * (1 - 1e-12)).all())
    if kind == "integer":
        # integers times integers: the exact result is an integer, nothing is left for the low part, and it equals
        # plain integer arithmetic
        assert bool((value == value.round()).all()) and bool((value.lo == 0).all())
        ci = c.to(torch.int64)
        exact = sum(ci[:, i].reshape(-1, 1, 1) * cref.as_real64(t).to(torch.int64) for i, t in enumerate((AY, Y, Yp)))
        assert torch.equal(value.to(torch.int64), exact)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gamma_zero_does_not_read_yprev(dtype):
    AY, Y, Yp, coef = cref.make_inputs(dtype, 2, 3, 33, seed=5)
    coef[0, 2] = 0.0
    coef[1, 2] = -0.0
    Yp.fill_(cref.nan_of(dtype))
    value, bound = cref.step(AY, Y, Yp, coef, dtype)
    assert bool(torch.isfinite(value).all()) and bool(torch.isfinite(bound).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fault", cref.FAULTS)
@pytest.mark.parametrize("kind", ["randn", "integer"])
def test_bound_rejects_planted_faults(dtype, fault, kind):
    """a result computed with a wrong coefficient, a dropped term or a swapped panel — and rounded to the kernel's
    storage type like a real kernel's output — lies outside the bound; the faultless one inside"""
    AY, Y, Yp, coef = cref.make_inputs(dtype, 2, 4, 65, seed=3, kind=kind)
    if kind == "integer":
        coef[:, 0], coef[:, 1], coef[:, 2] = 3.0, -5.0, 2.0          # (distinct and nonzero: every fault changes the result)
    value, bound = cref.step(AY, Y, Yp, coef, dtype)
    wrong, _ = cref.step(AY, Y, Yp, coef, dtype, fault=fault)

    def stored(v):
        r = v.to(cref.REAL_OF[dtype])
        return torch.view_as_complex(r.reshape(2, 4, 65, 2).contiguous()) if dtype.is_complex else r
    assert cref.check(stored(value), value, bound, "faultless") <= 1.0
    assert cref.violates(stored(wrong), value, bound) > 0.5 * value.numel()
    with pytest.raises(AssertionError):
        cref.check(stored(wrong), value, bound, fault)


@pytest.mark.parametrize("m", [1, 2, 3, 7, 12, 20])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_coefficient_table_is_the_scaled_chebyshev_polynomial(m, sign):
    """the degree-m table applied to a diagonal operator (float64 recurrence, exactly the kernel's formula) against
    T_m((t - c) / e) / T_m((a0 - c) / e) by the cosh / cos formula: relative error <= m * 64 * eps at the points outside
    the damped interval and at its ends (|T_m| >= 1 there); inside the interval, where T_m has its zeros, the same
    bound relative to the envelope 1 / |T_m((a0 - c) / e)|."""
    a = torch.tensor([30.0, 41.5], dtype=torch.float64)
    b = torch.tensor([200.0, 333.0], dtype=torch.float64)
    a0 = torch.tensor([-1.0, 2.25], dtype=torch.float64)
    table = cheb_coefficients(a, b, a0, m, sign)                      # (m, 2, 3)
    assert table.shape == (m, 2, 3) and table.dtype == torch.float64
    assert bool((table[0, :, 2] == 0).all())                         # first step: gamma = 0 exactly
    for s in range(2):
        lo, hi, z = float(a[s]), float(b[s]), float(a0[s])
        tB = torch.cat((torch.linspace(z - 5.0, lo - 0.02 * (hi - lo), 40, dtype=torch.float64),
                        torch.tensor([lo, hi], dtype=torch.float64),
                        torch.linspace(lo, hi, 31, dtype=torch.float64)))
        d = sign * tB                                                # the operator A = sign * B, diagonal
        yp, y = None, torch.ones_like(d)
        for i in range(m):
            al, be, ga = (float(v) for v in table[i, s])
            yn = al * (d * y) + be * y + (ga * yp if i > 0 else 0.0)
            yp, y = y, yn
        want = cref.scaled_chebyshev(tB, lo, hi, z, m)
        env = abs(float(cref.scaled_chebyshev(torch.tensor([lo], dtype=torch.float64), lo, hi, z, m)[0]))      # 1 / |T_m(x0)|
        outside = torch.arange(tB.numel()) < 42
        rel = (y - want).abs() / torch.where(outside, want.abs(), torch.full_like(want, env))
        assert float(rel.max()) <= cref.chebyshev_bound(m), (m, sign, s, float(rel.max()))
        assert abs(float(cref.scaled_chebyshev(torch.tensor([z], dtype=torch.float64), lo, hi, z, m)[0]) - 1.0) < 1e-12


def test_coefficients_of_an_interval_without_width_are_the_identity_filter():
    zero = torch.zeros(2, dtype=torch.float64)
    t = cheb_coefficients(zero, zero, zero, 4)
    assert bool((t[..., 0] == 0).all()) and bool((t[..., 1] == 1).all()) and bool((t[..., 2] == 0).all())
    five = torch.full((1,), 5.0, dtype=torch.float64)
    t = cheb_coefficients(five, five, five, 3, -1.0)
    assert bool((t[..., 0] == 0).all()) and bool((t[..., 1] == 1).all()) and bool((t[..., 2] == 0).all())
