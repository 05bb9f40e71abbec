"""Float64 / complex128 restatement of xk_cheb_step (xk_cheb.hip) with a per-entry error bound, and the closed form of
the scaled Chebyshev polynomial the driver's coefficient table must reproduce.

    out[b,c,n] = alpha[b] * AY[b,c,n] + beta[b] * Y[b,c,n] + gamma[b] * Yprev[b,c,n]

In the manner of tests/minres_ref.py: `step()` takes the very inputs the kernel is given (tensors of the kernel's
dtype, the coefficients as the float64 table the kernel reads), rounds them as the kernel rounds them — the f32 / c64
forms round each coefficient ONCE to float and evaluate in float; the f64 / c128 forms evaluate in double — and returns
(value, bound) per entry.  The coefficients are real for every dtype, so complex panels are handled as real ones on
their interleaved (re, im) storage, exactly like the kernel.  Where gamma[b] == 0 exactly (either sign) Yprev[b] is
not read: the term is absent whatever Yprev holds (NaN included).

Bound.  Three products and two sums, evaluated (alpha*ay + beta*y) + gamma*yp in the accumulation type with unit
round-off u: each term passes through at most three roundings (its product and the two sums), so to first order
|err| <= 3 u (|alpha ay| + |beta y| + |gamma yp|); 4 u covers the second-order terms, and a contraction into FMAs only
removes roundings.  That bound is against the EXACT value, so the reference must not carry a float64 rounding error of
its own next to a float64 kernel: the value is computed by error-free transformations (Veltkamp / Dekker two-product,
Knuth two-sum) as an unevaluated pair hi + lo, exact to O(u^2) of the term sum; `value` is hi and carries lo as the
attribute `value.lo`, which `check()` / `violates()` subtract.  The f32 / c64 forms get one more u for the rounding of each coefficient (5 u): the restatement uses
the rounded coefficients already, so this is slack the issue's statement of the bound grants and nothing relies on.
Results so small that they are subnormal carry an absolute error of up to the smallest normal number times u per
operation: `tiny` is added once.

`fault=` plants plausible bugs (FAULTS); tests/test_cheb_ref.py shows that `check()` rejects each of them.
"""
import torch

FAULTS = ("wrong_coef", "drop_term", "swap_panel")
REAL_OF = {torch.float64: torch.float64, torch.float32: torch.float32,
           torch.complex128: torch.float64, torch.complex64: torch.float32}


def unit_roundoff(dtype):
    return 2.0 ** -53 if REAL_OF[dtype] == torch.float64 else 2.0 ** -24


def nan_of(dtype):
    return complex(float("nan"), float("nan")) if dtype.is_complex else float("nan")


def as_real64(t):
    """(.., n) tensor of a kernel dtype -> float64 (.., n) or, complex, the interleaved (.., 2n)"""
    t = t.detach().cpu()
    if t.is_complex():
        return torch.view_as_real(t.to(torch.complex128).contiguous()).reshape(*t.shape[:-1], 2 * t.shape[-1]).clone()
    return t.to(torch.float64)


def rounded_coef(coef, dtype):
    """the (Bt, 3) float64 table as the kernel uses it: rounded once to float by the 32-bit forms"""
    coef = coef.detach().cpu().to(torch.float64)
    if REAL_OF[dtype] == torch.float32:
        return coef.to(torch.float32).to(torch.float64)
    return coef


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a                                  # 2^27 + 1 (the inputs here stay far below 2^996)
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def step(AY, Y, Yp, coef, dtype, fault=None):
    """what xk_cheb_step must write into out[:, :, :N]: (value, bound), both float64 (Bt, p, n) with n = N (real) or 2N
    (complex, interleaved).  AY, Y, Yp: (Bt, p, N) tensors of `dtype`; coef: (Bt, 3) float64."""
    c = rounded_coef(coef, dtype)
    ay, y, yp = as_real64(AY), as_real64(Y), as_real64(Yp)
    al, be, ga = (c[:, i].reshape(-1, 1, 1) for i in range(3))
    if fault == "wrong_coef":
        al, be = be, al                                  # alpha and beta taken from each other's slot
    if fault == "swap_panel":
        y, yp = yp, y                                    # Y and Yprev swapped (the ring rotated the wrong way)
    has = (ga != 0).expand_as(yp)
    yp = torch.where(has, yp, torch.zeros_like(yp))      # gamma == 0: the term is absent whatever Yprev holds
    if fault == "drop_term":
        yp = torch.zeros_like(yp)                        # the gamma term left out (every step taken as a first step)
    (t1, e1), (t2, e2), (t3, e3) = _two_prod(al.expand_as(ay), ay), _two_prod(be.expand_as(y), y), \
        _two_prod(ga.expand_as(yp), yp)
    s1, f1 = _two_sum(t1, t2)
    value, f2 = _two_sum(s1, t3)
    value.lo = ((e1 + e2) + e3) + (f1 + f2)              # value + value.lo: the exact sum to O(u64^2)
    u = unit_roundoff(dtype)
    nround = 5.0 if REAL_OF[dtype] == torch.float32 else 4.0
    bound = nround * u * (t1.abs() + t2.abs() + t3.abs()) + torch.finfo(REAL_OF[dtype]).tiny
    return value, bound


def check(got, value, bound, what=""):
    """every entry of `got` (a tensor of the kernel dtype, (Bt, p, N)) within `bound` of `value`; returns the largest
    |err| / bound.  A NaN / Inf where the reference is finite fails."""
    g = as_real64(got)
    assert g.shape == value.shape, "%s: shape %s vs %s" % (what, tuple(g.shape), tuple(value.shape))
    err = ((g - value) - getattr(value, "lo", 0.0)).abs()
    bad = ~(err <= bound)
    ratio = float((err / bound).nan_to_num(nan=float("inf")).max()) if err.numel() else 0.0
    assert not bool(bad.any()), "%s: %d entries outside the bound, worst |err| / bound = %.3g at %s" % (
        what, int(bad.sum()), ratio, tuple(torch.nonzero(bad)[0].tolist()))
    return ratio


def violates(got, value, bound):
    """number of entries of `got` outside the bound (for the planted faults)"""
    err = ((as_real64(got) - value) - getattr(value, "lo", 0.0)).abs()
    return int((~(err <= bound)).sum())


def make_inputs(dtype, Bt, p, N, seed, kind="randn"):
    """(AY, Y, Yp, coef) on the host.  kinds: randn; graded (magnitudes spanning 1e+-30 in 64-bit, 1e+-15 in 32-bit
    forms); cancel (alpha*ay ~ -beta*y); integer (integer-valued panels and coefficients: the result is exact)"""
    g = torch.Generator().manual_seed(seed)
    rd = REAL_OF[dtype]

    def rnd():
        t = torch.randn((Bt, p, N), dtype=rd, generator=g)
        if dtype.is_complex:
            t = torch.complex(t, torch.randn((Bt, p, N), dtype=rd, generator=g))
        return t
    AY, Y, Yp = rnd(), rnd(), rnd()
    coef = torch.randn((Bt, 3), dtype=torch.float64, generator=g) * 2.0
    if kind == "graded":
        span = 30.0 if rd == torch.float64 else 15.0
        for t in (AY, Y, Yp):
            e = (torch.rand((Bt, p, N), dtype=torch.float64, generator=g) * 2.0 - 1.0) * span
            t.mul_((10.0 ** e).to(rd))
    elif kind == "cancel":
        # alpha ay + beta y cancels to rounding level: y = -(alpha / beta) ay, rounded to the storage type
        coef[:, 1] = coef[:, 1].abs() + 0.5
        ratio = -(rounded_coef(coef, dtype)[:, 0] / rounded_coef(coef, dtype)[:, 1]).reshape(-1, 1, 1)
        Y = (AY.to(torch.complex128 if dtype.is_complex else torch.float64) * ratio).to(dtype)
        Yp = Yp * 1e-6
    elif kind == "integer":
        def ints():
            t = torch.randint(-64, 65, (Bt, p, N), generator=g).to(rd)
            if dtype.is_complex:
                t = torch.complex(t, torch.randint(-64, 65, (Bt, p, N), generator=g).to(rd))
            return t
        AY, Y, Yp = ints(), ints(), ints()
        coef = torch.randint(-8, 9, (Bt, 3), generator=g).to(torch.float64)
    return AY.to(dtype), Y.to(dtype), Yp.to(dtype), coef


def scaled_chebyshev(t, a, b, a0, m):
    """T_m((t - c) / e) / T_m((a0 - c) / e), c = (a + b) / 2, e = (b - a) / 2, in float64 by the cosh / cos formula"""
    c, e = 0.5 * (a + b), 0.5 * (b - a)

    def T(x):
        x = torch.as_tensor(x, dtype=torch.float64)
        inside = x.abs() <= 1.0
        xi = torch.where(inside, x, torch.zeros_like(x))
        xo = torch.where(inside, torch.full_like(x, 2.0), x)
        sgn = torch.where((xo < 0) & (m % 2 == 1), -torch.ones_like(x), torch.ones_like(x))
        return torch.where(inside, torch.cos(m * torch.acos(xi)), sgn * torch.cosh(m * torch.acosh(xo.abs())))
    return T((t - c) / e) / T(torch.tensor((a0 - c) / e, dtype=torch.float64))


def chebyshev_bound(m):
    """relative error allowed between the recurrence and the closed form: m * 64 * eps (the recurrence IS the
    polynomial; m steps of a few roundings each, amplified by at most the polynomial's own growth)"""
    return m * 64 * 2.0 ** -52


__all__ = ["FAULTS", "step", "check", "violates", "make_inputs", "scaled_chebyshev", "chebyshev_bound", "nan_of",
           "unit_roundoff", "as_real64", "rounded_coef", "REAL_OF"]
