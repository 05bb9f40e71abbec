"""Float64 / complex128 restatement of the fused Krylov step kernels of xk_krylov.hip, with error bounds.

For every kernel (xk_kry_dots, xk_bicg_p, xk_bicg_s, xk_bicg_final, xk_kry_resid, xk_cg_update, xk_cg_p,
xk_kry_status) a function computes, from the very inputs the kernel is given, what the kernel must write: its
vector outputs on [0, N), the per-system scalars it stores, and its block partials summed over the used slots
[0, nblk).  The formulas are those of the oracle (oracle/solve.py: `_dot` = sum conj(r) z, `_safedenom` = exact
zeros become eps) and of the update lines cited in the header of xk_krylov.hip.

Each function returns {name: (value, bound)}: `value` in float64 / complex128, `bound` a per-entry absolute bound
on |kernel - value| derived from the unit roundoff u of the KERNEL dtype and from the magnitudes involved.
`check()` compares a kernel's outputs with that and raises AssertionError naming the first output out of bounds.

The `fault=` argument of the functions produces plausible kernel bugs (a dropped tail, a dropped block partial,
a missing conjugation, a misplaced eps substitution, ...).  tests/test_krylov_ref.py feeds those outputs to
`check()` and asserts that every one of them is rejected: the evidence that the GPU tests would catch them.
"""
import math
import torch

# C_TOL: every bound below is C_TOL * u * (sum of the magnitudes of the terms of the computation) plus the
# propagated error of the scalars the kernel derives from partial sums.  The longest elementwise chain is the
# complex p = r + beta (p - omega v): two complex products (each normwise <= sqrt(5) u, Brent-Percival-Zimmermann)
# and two additions, about 6.5 u to first order; a real chain is at most 4 roundings.  For the float64 kernels the
# float64 reference carries its own rounding of the same order, at most doubling the first-order error of the
# simpler chains.  C_TOL = 8 covers both with a small margin while staying tight enough that every fault of
# FAULTS moves an output by many bounds (tests/test_krylov_ref.py).
C_TOL = 8.0

# reduction depth added to the per-thread term count k in the dot bound |d^ - d| <= C u (k + DOT_TREE) sum|x||y|:
# wave_sum over 64 lanes (6 levels) + 4-wave combine (2) + the consumer's 64-lane re-reduction of the partials (6)
# + the rounding of each complex product (2)
DOT_TREE = 16

# complex elements (real ones for real dtypes) per 16 B vector: the kernels' VN (real) / CV (complex)
VEC_ELEMS = {torch.float64: 2, torch.float32: 4, torch.complex128: 1, torch.complex64: 2}
REAL_OF = {torch.float64: torch.float64, torch.float32: torch.float32,
           torch.complex128: torch.float64, torch.complex64: torch.float32}
HP_OF = {torch.float64: torch.float64, torch.float32: torch.float64,
         torch.complex128: torch.complex128, torch.complex64: torch.complex128}

FAULTS = ("drop_tail", "drop_block", "noconj", "conj1_ignored", "eps_all", "eps_none", "first_ignored", "rho_swap")

# worst |kernel - reference| / bound seen by check(), per kernel dtype (reported by the GPU runs)
WORST = {}


def unit_roundoff(dtype):
    return torch.finfo(REAL_OF[dtype]).eps / 2


def hp(t):
    """float64 / complex128 copy on the CPU (complex partials (..., 2) stay real: see `partial_value`)."""
    t = t.detach().cpu()
    return t.to(torch.complex128 if t.is_complex() else torch.float64)


def rounded_eps(eps, dtype):
    """the eps the kernel really substitutes: the C entry points cast the double argument to the element type"""
    return float(torch.tensor(eps, dtype=torch.float64).to(REAL_OF[dtype]).item())


# ------------------------------------------------------------------------------------------------ block layout
def block_range(N, nblk, blk, vn):
    """replica of block_range (xk_kry_layout.h): element range [lo, hi) of block `blk` (in vn-element vectors)"""
    chunks = (N + vn - 1) // vn
    per = (chunks + nblk - 1) // nblk
    lo, hi = blk * per * vn, (blk * per + per) * vn
    npad = chunks * vn
    return min(lo, npad), min(hi, npad)


def terms_per_thread(N, nblk, vn):
    """k of the dot bound: products one thread accumulates (256 threads per block, vn per 16 B vector)"""
    chunks = (N + vn - 1) // vn
    per = (chunks + nblk - 1) // nblk
    return vn * max(1, (per + 255) // 256)


class Ctx:
    """shape / type facts shared by a kernel launch and its reference"""

    def __init__(self, dtype, S, N, nblk, eps=1e-12):
        self.dtype, self.S, self.N, self.nblk = dtype, S, N, nblk
        self.cplx = dtype.is_complex
        self.vn = VEC_ELEMS[dtype]
        self.u = unit_roundoff(dtype)
        self.cu = C_TOL * self.u
        self.eps = rounded_eps(eps, dtype)
        self.k = terms_per_thread(N, nblk, self.vn)

    def vec(self, t):
        """the [0, N) part of an (S, ld) vector array, in high precision"""
        return hp(t)[:, :self.N]

    def scal(self, t):
        """a per-system scalar array (S,) in high precision"""
        return hp(t).reshape(self.S)


def partial_value(P, ctx):
    """(S, 64) real / (S, 64, 2) interleaved complex partials -> (S, 64) float64 / complex128"""
    P = hp(P)
    if ctx.cplx and P.dim() == 3:
        return torch.complex(P[..., 0], P[..., 1])
    return P


# ------------------------------------------------------------------------------------------------ building blocks
def _dot(x, y, cplx, conj=True):
    return ((x.conj() if (cplx and conj) else x) * y).sum(-1)


def _dot_bound(ctx, x, y, ex=None, ey=None):
    """|computed <x,y> - exact <x,y>| for inputs carrying elementwise errors ex, ey (absolute)"""
    b = ctx.cu * (ctx.k + DOT_TREE) * (x.abs() * y.abs()).sum(-1)
    if ex is not None:
        b = b + (ex * y.abs()).sum(-1)
    if ey is not None:
        b = b + (x.abs() * ey).sum(-1)
    return b


def _block_dots(ctx, x, y, conj=True):
    """(S, nblk) per-block partials of <x, y> over the kernel's block ranges"""
    out = []
    for blk in range(ctx.nblk):
        lo, hi = block_range(ctx.N, ctx.nblk, blk, ctx.vn)
        hi = min(hi, ctx.N)                     # [N, npad) is zero by contract
        lo = min(lo, hi)
        out.append(_dot(x[:, lo:hi], y[:, lo:hi], ctx.cplx, conj))
    return torch.stack(out, -1)


def _dot_total(ctx, x, y, fault=None, conj=True):
    """<x, y> as the sum of the block partials; faults: drop_tail / drop_block / noconj"""
    if fault == "drop_tail":
        keep = ctx.N - ctx.N % ctx.vn
        x, y = x.clone(), y.clone()
        x[:, keep:] = 0
        y[:, keep:] = 0
    parts = _block_dots(ctx, x, y, conj=conj and fault != "noconj")
    if fault == "drop_block":
        nonempty = [b for b in range(ctx.nblk) if block_range(ctx.N, ctx.nblk, b, ctx.vn)[0] < ctx.N]
        parts[:, nonempty[-1]] = 0
    return parts.sum(-1)


def _psum(ctx, P):
    """the kernel's sum of the used partial slots [0, nblk): value and bound (a 64-lane tree in reduce_partials, a
    sequential loop of <= 63 additions in kry_status: both <= 64 u sum|p| to first order)"""
    p = partial_value(P, ctx)[:, :ctx.nblk]
    return p.sum(-1), ctx.cu * 8 * p.abs().sum(-1)


def _safe(ctx, v, fault):
    """_safedenom (oracle/solve.py:15-18): exact zeros become eps (complex: eps + 0i)"""
    if fault == "eps_none":
        return v
    if fault == "eps_all":
        return torch.full_like(v, ctx.eps)
    return torch.where(v == 0, torch.full_like(v, ctx.eps), v)


def _div(ctx, a, ea, b, eb, fault=None):
    """a / safe(b) with first-order error (ea + |q| eb) / |b| + C u |q|; a substituted eps is exact"""
    zero = b == 0
    bs = _safe(ctx, b, fault)
    q = a / bs
    eb = torch.where(zero, torch.zeros_like(eb), eb)
    return q, (ea + q.abs() * eb) / bs.abs() + ctx.cu * q.abs()


def _mul(ctx, a, ea, b, eb):
    q = a * b
    return q, ea * b.abs() + a.abs() * eb + ctx.cu * q.abs()


def _z(x):
    return torch.zeros(x.shape, dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ the kernels
def kry_dots(ctx, x1, y1, x2=None, y2=None, shiftz=None, E=None, conj1=False, x1_is_y1=False, x2_is_y1=False,
             y2_is_y1=False, fault=None):
    """xk_kry_dots: y1 -= E_s z (when E is given, written back), then P1 = <x1, y1> (<y1, x1> with conj1) and
    P2 = <x2, y2>; an operand aliased to y1 is read AFTER the shift.  Inputs are the [0, N) parts in high
    precision; E is (S,)."""
    out = {}
    ey = None
    if E is not None:
        ez = E.unsqueeze(-1) * shiftz
        y1 = y1 - ez
        ey = ctx.cu * (y1.abs() + ez.abs())
        out["y1"] = (y1, ey)
    a1 = y1 if x1_is_y1 else x1
    ea1 = ey if x1_is_y1 else None
    if ctx.cplx and conj1 and fault != "conj1_ignored":
        out["P1"] = (_dot_total(ctx, y1, a1, fault), _dot_bound(ctx, y1, a1, ey, ea1))
    else:
        out["P1"] = (_dot_total(ctx, a1, y1, fault), _dot_bound(ctx, a1, y1, ea1, ey))
    if x2 is not None or x2_is_y1:
        a2 = y1 if x2_is_y1 else x2
        b2 = y1 if y2_is_y1 else y2
        out["P2"] = (_dot_total(ctx, a2, b2, fault),
                     _dot_bound(ctx, a2, b2, ey if x2_is_y1 else None, ey if y2_is_y1 else None))
    return out


def bicg_p(ctx, r, p, v, Prho_new, rho_old, alpha, omega, first, fault=None):
    """xk_bicg_p (solve.py:273-276): beta = rho_new / safe(rho_old) * (alpha / safe(omega));
    p = r + beta (p - safe(omega) v) (the reference patches omega in place before using it);  first: p = r"""
    rho_new, e_rn = _psum(ctx, Prho_new)
    out = {"rho_store": (rho_new, e_rn)}
    if first and fault != "first_ignored":
        out["p"] = (r, _z(r))
        return out
    if first:                                   # the reference's first pass: rho_old = rho_new, alpha = omega = 1
        rho_old = rho_new.clone()
        alpha, omega = torch.ones_like(rho_new), torch.ones_like(rho_new)
    num, den = (rho_old, rho_new) if fault == "rho_swap" else (rho_new, rho_old)
    e_num, e_den = (_z(rho_old), e_rn) if fault == "rho_swap" else (e_rn, _z(rho_old))
    q1, e1 = _div(ctx, num, e_num, den, e_den, fault)
    om = _safe(ctx, omega, fault)
    q2, e2 = _div(ctx, alpha, _z(alpha), omega, _z(omega), fault)
    beta, eb = _mul(ctx, q1, e1, q2, e2)
    d = p - om.unsqueeze(-1) * v
    mag_d = p.abs() + om.abs().unsqueeze(-1) * v.abs()
    val = r + beta.unsqueeze(-1) * d
    bnd = ctx.cu * (r.abs() + beta.abs().unsqueeze(-1) * mag_d) + eb.unsqueeze(-1) * mag_d
    out["p"] = (val, bnd)
    return out


def bicg_s(ctx, r, v, rho, Pr0v, fault=None):
    """xk_bicg_s (solve.py:279, 282): alpha = rho / safe(<r0, v>);  s = r - alpha v"""
    r0v, e = _psum(ctx, Pr0v)
    al, eal = _div(ctx, rho, _z(rho), r0v, e, fault)
    s = r - al.unsqueeze(-1) * v
    bnd = ctx.cu * (r.abs() + al.abs().unsqueeze(-1) * v.abs()) + eal.unsqueeze(-1) * v.abs()
    return {"alpha_store": (al, eal), "s": (s, bnd)}


def bicg_final(ctx, x, yd, zd, sv, t, r0, alpha, Pts, Ptt, skip_r, fault=None):
    """xk_bicg_final (solve.py:286-297): omega = <t,s> / safe(<t,t>) (from partials);  x' = x + alpha yd + omega zd;
    unless skip_r: r = s - omega t and the partials |r|^2, <r0, r>"""
    ts, ets = _psum(ctx, Pts)
    tt, ett = _psum(ctx, Ptt)
    om, eom = _div(ctx, ts, ets, tt, ett, fault)
    out = {"omega_store": (om, eom)}
    a, w = alpha.unsqueeze(-1), om.unsqueeze(-1)
    xo = x + a * yd + w * zd
    out["xout"] = (xo, ctx.cu * (x.abs() + a.abs() * yd.abs() + w.abs() * zd.abs()) + eom.unsqueeze(-1) * zd.abs())
    if not skip_r:
        rn = sv - w * t
        er = ctx.cu * (sv.abs() + w.abs() * t.abs()) + eom.unsqueeze(-1) * t.abs()
        out["r"] = (rn, er)
        out["Prr"] = (_dot_total(ctx, rn, rn, fault).real, _dot_bound(ctx, rn, rn, er, er))
        out["Prho"] = (_dot_total(ctx, r0, rn, fault), _dot_bound(ctx, r0, rn, None, er))
    return out


def kry_resid(ctx, b, y, r0, with_prho, fault=None):
    """xk_kry_resid (solve.py:148-149, 290-291): r = b - y; partials |r|^2 and, when a Prho buffer is given,
    <r0, r> -- or |r|^2 again (as a complex pair with zero imaginary part) when r0 is NULL"""
    rn = b - y
    er = ctx.cu * (b.abs() + y.abs())
    out = {"r": (rn, er)}
    rr = (_dot_total(ctx, rn, rn, fault).real, _dot_bound(ctx, rn, rn, er, er))
    out["Prr"] = rr
    if with_prho:
        if r0 is None:
            out["Prho"] = (rr[0].to(HP_OF[ctx.dtype]), rr[1])
        else:
            out["Prho"] = (_dot_total(ctx, r0, rn, fault), _dot_bound(ctx, r0, rn, None, er))
    return out


def cg_update(ctx, x, p, Ap, r, Prz, PpAp, skip_r, fault=None):
    """xk_cg_update (solve.py:144-155): alpha = <r,z> / safe(<p,Ap>);  x' = x + alpha p;
    unless skip_r: r -= alpha Ap and the partials |r|^2"""
    rz, erz = _psum(ctx, Prz)
    pap, epap = _psum(ctx, PpAp)
    al, eal = _div(ctx, rz, erz, pap, epap, fault)
    a = al.unsqueeze(-1)
    out = {"xout": (x + a * p, ctx.cu * (x.abs() + a.abs() * p.abs()) + eal.unsqueeze(-1) * p.abs())}
    if not skip_r:
        rn = r - a * Ap
        er = ctx.cu * (r.abs() + a.abs() * Ap.abs()) + eal.unsqueeze(-1) * Ap.abs()
        out["r"] = (rn, er)
        out["Prr"] = (_dot_total(ctx, rn, rn, fault).real, _dot_bound(ctx, rn, rn, er, er))
    return out


def cg_p(ctx, z, p, Prz_new, Prz_old, fault=None):
    """xk_cg_p (solve.py:171-173): beta = <r,z>_new / safe(<r,z>_old);  p = z + beta p"""
    rzn, en = _psum(ctx, Prz_new)
    rzo, eo = _psum(ctx, Prz_old)
    if fault == "rho_swap":
        rzn, en, rzo, eo = rzo, eo, rzn, en
    beta, eb = _div(ctx, rzn, en, rzo, eo, fault)
    b = beta.unsqueeze(-1)
    return {"p": (z + b * p, ctx.cu * (z.abs() + b.abs() * p.abs()) + eb.unsqueeze(-1) * p.abs())}


def kry_status(ctx, Prr, stop):
    """xk_kry_status: rnorm_s = sqrt(sum of the used partials); status = (max_s rnorm_s, #{s : !(rnorm_s < stop_s)});
    a NaN system counts as unconverged and makes the max +inf.  Returns rnorm (value, bound) and the exact status
    computed from the KERNEL's own rnorm (`status_of`)."""
    ss, e = _psum(ctx, Prr)
    rn = ss.clamp(min=0).sqrt()
    # d sqrt(a) = da / (2 sqrt a), plus the rounding of the sqrt itself
    bnd = torch.where(rn > 0, e / (2 * rn), e.sqrt()) + ctx.cu * rn
    return {"rnorm": (torch.where(torch.isnan(ss), ss, rn), bnd)}


def status_of(rnorm, stop):
    """(max, count) exactly as the kernel must derive them from its own rnorm and stop (both in the kernel dtype)"""
    nan = torch.isnan(rnorm)
    mx = float("inf") if bool(nan.any()) else (float(rnorm.double().max()) if rnorm.numel() else 0.0)
    cnt = int((nan | ~(rnorm < stop)).sum())
    return mx, cnt


# ------------------------------------------------------------------------------------------------ checking
def check(got, ref, dtype, what=""):
    """Compare kernel outputs (`got`: name -> tensor, any dtype, same shape as the reference value) with the
    reference (`ref`: name -> (value, bound)).  Raises AssertionError on the first output out of bounds (NaN and
    inf count as out of bounds); returns the worst error / bound ratio and records it in WORST[dtype]."""
    worst = 0.0
    for name, (val, bnd) in ref.items():
        assert name in got, "%s: no kernel output %r" % (what, name)
        assert bool(torch.isfinite(val).all()), "%s: reference %s is not finite" % (what, name)
        g = hp(got[name]).reshape(val.shape)
        err = (g - val).abs()
        ok = err <= bnd
        if not bool(ok.all()):
            idx = (~ok).nonzero()[0].tolist()
            raise AssertionError("%s: %s out of bounds at %s: got %r, want %r, |err| %.3e > bound %.3e (%d entries)"
                                 % (what, name, idx, g[tuple(idx)].item(), val[tuple(idx)].item(),
                                    err[tuple(idx)].item(), bnd[tuple(idx)].item(), int((~ok).sum())))
        nz = bnd > 0
        if bool(nz.any()):
            worst = max(worst, float((err[nz] / bnd[nz]).max()))
    WORST[dtype] = max(WORST.get(dtype, 0.0), worst)
    return worst


def values(ref, dtype=None):
    """the reference values alone (rounded to the kernel dtype when given): what a kernel would write"""
    out = {}
    for name, (val, _) in ref.items():
        if dtype is not None:
            val = val.to(dtype if val.is_complex() else REAL_OF[dtype])
        out[name] = val
    return out


# ------------------------------------------------------------------------------------------------ inputs
def nan_of(dtype):
    return complex(math.nan, math.nan) if dtype.is_complex else math.nan


def rand_vecs(g, dtype, S, N, ld, count=1, scale=1.0):
    """`count` (S, ld) arrays of the kernel dtype: random on [0, N), exact zeros on [N, npad) (npad = N rounded up
    to whole 16 B vectors), NaN on [npad, ld) -- the panel contract of the Krylov kernels"""
    vn = VEC_ELEMS[dtype]
    npad = (N + vn - 1) // vn * vn
    out = []
    for _ in range(count):
        if dtype.is_complex:
            re = torch.randn(S, N, dtype=torch.float64, generator=g)
            im = torch.randn(S, N, dtype=torch.float64, generator=g)
            val = torch.complex(re, im) * scale
        else:
            val = torch.randn(S, N, dtype=torch.float64, generator=g) * scale
        a = torch.full((S, ld), nan_of(dtype), dtype=dtype)
        a[:, :N] = val.to(dtype)
        a[:, N:npad] = 0
        out.append(a)
    return out


def rand_scalars(g, dtype, S, lo=0.5, hi=1.5):
    """(S,) per-system scalars of magnitude in [lo, hi) with random signs / phases"""
    mag = lo + (hi - lo) * torch.rand(S, dtype=torch.float64, generator=g)
    if dtype.is_complex:
        ph = 2 * math.pi * torch.rand(S, dtype=torch.float64, generator=g)
        return torch.polar(mag, ph).to(dtype)
    sgn = torch.where(torch.rand(S, dtype=torch.float64, generator=g) < 0.5, -1.0, 1.0)
    return (mag * sgn).to(dtype)


def rand_partials(g, dtype, S, nblk, zero_systems=(), lo=0.5, hi=1.5, positive=False):
    """(S, 64) real / (S, 64, 2) complex partials: slots [0, nblk) random (exactly zero for `zero_systems`), slots
    [nblk, 64) NaN-poisoned (consumers must ignore them)"""
    shape = (S, 64, 2) if dtype.is_complex else (S, 64)
    rd = REAL_OF[dtype]
    P = torch.full(shape, math.nan, dtype=rd)
    mag = lo + (hi - lo) * torch.rand((S, nblk) + shape[2:], dtype=torch.float64, generator=g)
    if not positive:
        mag = mag * torch.where(torch.rand(mag.shape, dtype=torch.float64, generator=g) < 0.5, -1.0, 1.0)
    mag = mag / nblk                        # the sum stays O(1) whatever nblk
    P[:, :nblk] = mag.to(rd)
    for s in zero_systems:
        P[s, :nblk] = 0
    return P


def poisoned_partials(dtype, S, real=False):
    shape = (S, 64, 2) if (dtype.is_complex and not real) else (S, 64)
    return torch.full(shape, math.nan, dtype=REAL_OF[dtype])
