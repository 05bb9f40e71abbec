"""Float64 / complex128 restatement of xk_cheb_clenshaw (xk_cheb_clenshaw.hip) with a per-entry error bound, and a
plain statement of the band-pass filter of symeig(mode="nearest"): its coefficients, its closed form, the driver's
Clenshaw loop and the degree rule.

    out[b,c,n] = ((alpha[b] * AY[b,c,n] + beta[b] * Y[b,c,n]) + gamma[b] * Yprev[b,c,n]) + delta[b] * X0[b,c,n]

In the manner of tests/cheb_ref.py, whose helpers it uses: `step()` takes the very inputs the kernel is given (tensors
of the kernel's dtype, the coefficients as the float64 table the kernel reads), rounds them as the kernel rounds them —
the f32 / c64 forms round each coefficient ONCE to float and evaluate in float; the f64 / c128 forms evaluate in double —
and returns (value, bound) per entry.  The coefficients are real for every dtype, so complex panels are handled as real
ones on their interleaved (re, im) storage, exactly like the kernel.  Where gamma[b] == 0 exactly (either sign)
Yprev[b] is not read: the term is absent whatever Yprev holds (NaN included).

Bound.  Four products and three sums, evaluated left to right in the accumulation type with unit round-off u: each term
passes through at most four roundings (its product and the three sums), so to first order |err| <= 4 u (|alpha ay| +
|beta y| + |gamma yp| + |delta x|); the fifth u covers the second-order terms, and a contraction into FMAs only removes
roundings.  The f32 / c64 forms get one more u for the rounded coefficient (6 u), as cheb_ref's 5 against its 4.  The
bound is against the EXACT value: the value is computed by error-free transformations (two-product, two-sum) as an
unevaluated pair hi + lo; `value` is hi and carries lo as the attribute `value.lo`, which `check()` / `violates()` of
cheb_ref subtract.  `tiny` (the smallest normal number) is added once for subnormal results.

`fault=` plants plausible bugs (FAULTS); tests/test_chebwin_ref.py shows that `check()` rejects each of them.
"""
import math
import torch
from tests.cheb_ref import (REAL_OF, unit_roundoff, nan_of, as_real64, _two_sum, _two_prod, check, violates,
                            chebyshev_bound)

FAULTS = ("slot_swap", "drop_delta", "swap_panel", "x0_for_y")


def rounded_coef(coef, dtype):
    """the (Bt, 4) float64 table as the kernel uses it: rounded once to float by the 32-bit forms"""
    coef = coef.detach().cpu().to(torch.float64)
    if REAL_OF[dtype] == torch.float32:
        return coef.to(torch.float32).to(torch.float64)
    return coef


def step(AY, Y, Yp, X0, coef, dtype, fault=None):
    """what xk_cheb_clenshaw must write into out[:, :, :N]: (value, bound), both float64 (Bt, p, n) with n = N (real)
    or 2N (complex, interleaved).  AY, Y, Yp, X0: (Bt, p, N) tensors of `dtype`; coef: (Bt, 4) float64."""
    c = rounded_coef(coef, dtype)
    ay, y, yp, x = as_real64(AY), as_real64(Y), as_real64(Yp), as_real64(X0)
    al, be, ga, de = (c[:, i].reshape(-1, 1, 1) for i in range(4))
    if fault == "slot_swap":
        ga, de = de, ga                                  # gamma and delta taken from each other's slot
    if fault == "swap_panel":
        y, yp = yp, y                                    # Y and Yprev swapped (the ring rotated the wrong way)
    if fault == "x0_for_y":
        y = x                                            # X0 taken for Y
    has = (ga != 0).expand_as(yp)
    yp = torch.where(has, yp, torch.zeros_like(yp))      # gamma == 0: the term is absent whatever Yprev holds
    if fault == "drop_delta":
        x = torch.zeros_like(x)                          # the delta term left out (a three-term step)
    (t1, e1), (t2, e2), (t3, e3), (t4, e4) = (_two_prod(al.expand_as(ay), ay), _two_prod(be.expand_as(y), y),
                                              _two_prod(ga.expand_as(yp), yp), _two_prod(de.expand_as(x), x))
    s1, f1 = _two_sum(t1, t2)
    s2, f2 = _two_sum(s1, t3)
    value, f3 = _two_sum(s2, t4)
    value.lo = (((e1 + e2) + e3) + e4) + ((f1 + f2) + f3)    # value + value.lo: the exact sum to O(u64^2)
    u = unit_roundoff(dtype)
    nround = 6.0 if REAL_OF[dtype] == torch.float32 else 5.0
    bound = nround * u * (t1.abs() + t2.abs() + t3.abs() + t4.abs()) + torch.finfo(REAL_OF[dtype]).tiny
    return value, bound


def make_inputs(dtype, Bt, p, N, seed, kind="randn"):
    """(AY, Y, Yp, X0, coef) on the host.  kinds: randn; graded (magnitudes spanning 1e+-30 in 64-bit, 1e+-15 in 32-bit
    forms); integer (integer-valued panels and coefficients: the result is exact).  Distinct coefficients per member."""
    g = torch.Generator().manual_seed(seed)
    rd = REAL_OF[dtype]

    def rnd():
        t = torch.randn((Bt, p, N), dtype=rd, generator=g)
        if dtype.is_complex:
            t = torch.complex(t, torch.randn((Bt, p, N), dtype=rd, generator=g))
        return t
    panels = [rnd() for _ in range(4)]
    coef = torch.randn((Bt, 4), dtype=torch.float64, generator=g) * 2.0
    if kind == "graded":
        span = 30.0 if rd == torch.float64 else 15.0
        for t in panels:
            e = (torch.rand((Bt, p, N), dtype=torch.float64, generator=g) * 2.0 - 1.0) * span
            t.mul_((10.0 ** e).to(rd))
    elif kind == "integer":
        def ints():
            t = torch.randint(-64, 65, (Bt, p, N), generator=g).to(rd)
            if dtype.is_complex:
                t = torch.complex(t, torch.randint(-64, 65, (Bt, p, N), generator=g).to(rd))
            return t
        panels = [ints() for _ in range(4)]
        coef = torch.randint(-8, 9, (Bt, 4), generator=g).to(torch.float64)
    return (*(t.to(dtype) for t in panels), coef)


# ---- the filter, stated plainly (float64, Python loops) -------------------------------------------------------------
def jackson(m):
    """g_k^m, k = 0 .. m"""
    a = math.pi / (m + 2)
    return [math.sin((k + 1) * a) / ((m + 2) * math.sin(a)) + (1.0 - (k + 1) / (m + 2)) * math.cos(k * a)
            for k in range(m + 1)]


def filter_closed_form(theta, theta_s, m):
    """p_m at the angles `theta` (float64 tensor), normalised to 1 at theta_s:
    sum_k g_k mu_k cos(k theta) / sum_k g_k mu_k cos(k theta_s), mu_k = (2 - delta_k0) cos(k theta_s)"""
    theta = torch.as_tensor(theta, dtype=torch.float64)
    g = jackson(m)
    num, den = torch.zeros_like(theta), 0.0
    for k in range(m + 1):
        mu = (1.0 if k == 0 else 2.0) * math.cos(k * theta_s)
        num = num + g[k] * mu * torch.cos(k * theta)
        den += g[k] * mu * math.cos(k * theta_s)
    return num / den


def clenshaw(table, matvec, X):
    """the driver's loop on a (m + 1, 4) table (one operator): b_m = table[0][1] X, then m steps
    b <- alpha (A b) + beta b + gamma b_prev + delta X; returns p(A) X"""
    Bp, Bk = None, table[0][1] * X
    for j in range(1, table.shape[0]):
        al, be, ga, de = (table[j][i] for i in range(4))
        Bn = al * matvec(Bk) + be * Bk
        if float(ga) != 0.0:
            Bn = Bn + ga * Bp
        Bn = Bn + de * X
        Bp, Bk = Bk, Bn
    return Bk


def ladder(max_degree, floor=8):
    out, m = [], floor
    while m < max_degree:
        out.append(m)
        m = (5 * m) // 4 + 1
    out.append(max_degree)
    return out


def degree_rule(theta_s, d_ref, filter_tail, max_degree):
    """(degree, capped): the ladder's smallest degree with max |p_m(theta_s +- d_ref)| <= filter_tail; max_degree
    (capped) when none below it is admissible"""
    lad = ladder(max_degree)
    for m in lad[:-1]:
        p = filter_closed_form(torch.tensor([theta_s + d_ref, theta_s - d_ref]), theta_s, m)
        if float(p.abs().max()) <= filter_tail:
            return m, False
    return lad[-1], True


__all__ = ["FAULTS", "step", "check", "violates", "make_inputs", "nan_of", "as_real64", "rounded_coef", "REAL_OF",
           "jackson", "filter_closed_form", "clenshaw", "ladder", "degree_rule", "chebyshev_bound", "unit_roundoff"]
