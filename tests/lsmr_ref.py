"""Float64 restatement of the LSMR step kernels of xk_lsmr.hip and of the whole iteration, with error bounds.

In the manner of tests/minres_ref.py (whose `Env`, block layout, partial-sum helpers, `check()` and input generators
are reused): for every kernel (xk_lsmr_init, xk_lsmr_bidiag, xk_lsmr_update) a function computes, from the very inputs
the kernel is given, what the kernel must write, and returns {name: (value, bound)}.

The recurrences are those of Fong & Saunders (2011), Algorithm LSMR with the damping rotation of section 7 and the
estimates of section 5, on the UN-normalised Golub-Kahan vectors uh_k = beta_k u_k, vh_k = alpha_k v_k:
    uh <- A vh / alpha_k - (alpha_k / beta_k) uh            (|uh| = beta_{k+1})
    vh <- A^H uh / beta_{k+1} - (beta_{k+1} / alpha_k) vh   (|vh| = alpha_{k+1})
    alphahat = sqrt(alphabar^2 + damp^2), chat = alphabar / alphahat, shat = damp / alphahat
    rho = sqrt(alphahat^2 + beta^2), c = alphahat / rho, s = beta / rho, thetanew = s alpha, alphabar' = c alpha
    thetabar = sbar rho, rhotemp = cbar rho, rhobar = sqrt(rhotemp^2 + thetanew^2), cbar' = rhotemp / rhobar,
    sbar' = thetanew / rhobar, zeta = cbar' zetabar, zetabar' = -sbar' zetabar
    hbar <- h - (thetabar rho / (rho_old rhobar_old)) hbar,  x <- x + (zeta / (rho rhobar)) hbar,
    h <- vh / alpha - (thetanew / rho) h
(start: alphabar = alpha_1, zetabar = alpha_1 beta_1, rho = rhobar = cbar = 1, sbar = 0, h = v_1, hbar = x = 0), and
the |rbar|, |A|, cond(Abar) recurrences written out in `_scalars` (|A|: the Frobenius norm of the bidiagonal capped by
an estimate of |A|_2, see there).  |x| of the S1 test is the norm of the PREVIOUS
iterate (the kernel sums |x|^2 while it writes x; the next step reads the partials).

Complex systems: every scalar above is real, so the kernels run on the interleaved (re, im) storage as real vectors of
length 2N; so do the functions here (`Env.vec` returns that view).

Bounds.  u is the unit roundoff of the kernel dtype, U_D = 2^-53 that of the double scalar state.
  * vectors: C_LS * u * sum|terms| plus the first-order propagation of the scalar errors.  The longest chain is x:
    hbar' = h - c1 hbar (the cast of c1 to the vector type, the product, the subtraction: 3 roundings), then
    x' = x + c2 hbar' (cast, product, addition: 3 more): 6 roundings on the longest path to first order; the float64
    reference carries the same chain for the float64 kernels, doubling that: C_LS = 12 (MINRES: 9 roundings, C_MR = 20).
    h' = vh (1/alpha) - c3 h is 5 roundings, the bidiagonalisation pass y' = Op (1/nu_x) - (nu_x/nu_y) y 5 as well.
  * scalar state: a running first-order error analysis (`E`): every operation adds its propagated input errors and
    C_ST * U_D * |result| for its own rounding (C_ST = 4 covers the reference's own rounding and fused multiply-adds);
    the double sums of the partials enter with 8 U_D sum|p| (64-lane tree).
`fault=` produces plausible bugs: FAULTS.  tests/test_lsmr_ref.py shows that `check()` rejects each of them."""
import math
import torch
from tests import krylov_ref as kref
from tests import minres_ref as mref

NST = 27
(ALPHA, BETA, ALPHABAR, ZETABAR, RHO, RHOBAR, CBAR, SBAR, ZETA, BETADD, BETAD, RHODOLD, TAUTILDEOLD, THETATILDE, D,
 NORMA2, MAXRBAR, MINRBAR, ITN, FLAG, NORMB, NORMR, NORMAR, NORMA, CONDA, NORMX, ALPHA1) = range(NST)
U_D = 2.0 ** -53
C_LS = 12.0
C_ST = 4.0
assert C_LS <= mref.C_MR

FAULTS = ("drop_tail", "drop_block", "wrong_slot", "no_damp", "hbar_after_x", "u_len_n")

check = kref.check
_c = lambda t: t.unsqueeze(-1)


class Env(mref.Env):
    def __init__(self, dtype, S, N, nblk):
        super().__init__(dtype, S, N, nblk)
        self.cu = C_LS * self.u


# ------------------------------------------------------------------------------------------------ running error analysis
class E:
    """a float64 tensor with a first-order absolute error bound"""

    def __init__(self, v, e=None):
        self.v = v if isinstance(v, torch.Tensor) else torch.tensor(float(v), dtype=torch.float64)
        self.e = torch.zeros_like(self.v) if e is None else e

    @staticmethod
    def of(x):
        return x if isinstance(x, E) else E(x)

    def _r(self, v, e):
        return E(v, e + C_ST * U_D * v.abs())

    def __add__(self, o):
        o = E.of(o)
        return self._r(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = E.of(o)
        return self._r(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = E.of(o)
        return self._r(self.v * o.v, self.e * o.v.abs() + self.v.abs() * o.e)

    __radd__, __rmul__ = __add__, __mul__

    def __neg__(self):
        return E(-self.v, self.e)

    def abs(self):
        return E(self.v.abs(), self.e)

    def sqrt(self):
        r = self.v.clamp(min=0).sqrt()
        pos = r > 0
        e = torch.where(pos, self.e / (2 * torch.where(pos, r, torch.ones_like(r))), self.e.sqrt())
        return self._r(r, e)


def ediv(a, b, ifzero=0.0):
    """a / b, `ifzero` where b is exactly 0 (the kernels' ls_div and their `r == 0 ? 1` selections)"""
    a, b = E.of(a), E.of(b)
    z = b.v == 0
    bs = torch.where(z, torch.ones_like(b.v), b.v)
    q = a.v / bs
    e = (a.e + q.abs() * b.e) / bs.abs() + C_ST * U_D * q.abs()
    fill = torch.full_like(q, ifzero)
    return E(torch.where(z, fill, q), torch.where(z, torch.zeros_like(e), e))


def emax(a, b):
    a, b = E.of(a), E.of(b)
    return E(torch.maximum(a.v, b.v), torch.maximum(a.e, b.e))


def emin(a, b):
    a, b = E.of(a), E.of(b)
    return E(torch.minimum(a.v, b.v), torch.maximum(a.e, b.e))


def psum(P, nblk, drop=False):
    """the kernels' double sum of the used partial slots as an E"""
    p = P.detach().cpu().to(torch.float64)[:, :nblk].clone()
    if drop:
        p[:, nblk - 1] = 0
    return E(p.sum(-1), 8 * U_D * p.abs().sum(-1))


def _slot(state, k, fault):
    kk = k + 1 if fault == "wrong_slot" else k
    return state[kk & 1].detach().cpu().to(torch.float64)


_keep_mask = mref._keep_mask


def _scalars(st, alpha, beta, normx, damp, atol, btol, conlim):
    """one step of the scalar recurrences of xk_lsmr_update.  st: {index: E} of the slot read; alpha, beta, normx: E.
    Returns ({index: E} of the slot written, the vector coefficients (c1, c2, c3) as E, the stop code tensor)."""
    g = lambda i: st[i]
    dmp = E(torch.full_like(alpha.v, float(damp)))
    alphabar, zetabar, rhoold, rhobarold = g(ALPHABAR), g(ZETABAR), g(RHO), g(RHOBAR)
    cbar, sbar, zetaold = g(CBAR), g(SBAR), g(ZETA)
    alphahat = (alphabar * alphabar + dmp * dmp).sqrt()
    chat, shat = ediv(alphabar, alphahat, 1.0), ediv(dmp, alphahat)
    rho = (alphahat * alphahat + beta * beta).sqrt()
    c, s = ediv(alphahat, rho, 1.0), ediv(beta, rho)
    thetanew, alphabar_n = s * alpha, c * alpha
    thetabar, rhotemp = sbar * rho, cbar * rho
    rhobar = (rhotemp * rhotemp + thetanew * thetanew).sqrt()
    cbar_n, sbar_n = ediv(rhotemp, rhobar, 1.0), ediv(thetanew, rhobar)
    zeta, zetabar_n = cbar_n * zetabar, -(sbar_n * zetabar)
    c1 = ediv(thetabar * rho, rhoold * rhobarold)
    c2 = ediv(zeta, rho * rhobar)
    c3 = ediv(thetanew, rho)
    betadd, betad, rhodold, tautildeold, thetatildeold = g(BETADD), g(BETAD), g(RHODOLD), g(TAUTILDEOLD), g(THETATILDE)
    betaacute, betacheck = chat * betadd, -(shat * betadd)
    betahat, betadd_n = c * betaacute, -(s * betaacute)
    rhotildeold = (rhodold * rhodold + thetabar * thetabar).sqrt()
    ctildeold, stildeold = ediv(rhodold, rhotildeold, 1.0), ediv(thetabar, rhotildeold)
    thetatilde, rhodold_n = stildeold * rhobar, ctildeold * rhobar
    betad_n = -(stildeold * betad) + ctildeold * betahat
    tautildeold_n = ediv(zetaold - thetatildeold * tautildeold, rhotildeold)
    taud = ediv(zeta - thetatilde * tautildeold_n, rhodold_n)
    d_n = g(D) + betacheck * betacheck
    dt = betad_n - taud
    normr = (d_n + dt * dt + betadd_n * betadd_n).sqrt()
    na2 = g(NORMA2) + beta * beta
    itn = g(ITN)
    maxrbar = emax(g(MAXRBAR), rhobarold)
    # |A| of the stopping rules: the Frobenius norm of the bidiagonal capped by sqrt(maxrbar^2 - damp^2) >= alpha_1
    # (an estimate of |A|_2 that ghost singular values do not inflate)
    two = emax(maxrbar * maxrbar - dmp * dmp, 0.0).sqrt()
    normA = emin(na2.sqrt(), emax(two, g(ALPHA1)))
    mn = emin(g(MINRBAR), rhobarold)
    later = itn.v >= 1
    minrbar = E(torch.where(later, mn.v, g(MINRBAR).v), torch.where(later, mn.e, g(MINRBAR).e))
    condA = ediv(emax(maxrbar, rhotemp), emin(minrbar, rhotemp))
    normar = zetabar_n.abs()
    normb = g(NORMB)
    code = torch.zeros_like(alpha.v)
    code = torch.where(condA.v >= conlim, 3.0, code)
    code = torch.where(normar.v <= atol * normA.v * normr.v, 2.0, code)
    code = torch.where(normr.v <= btol * normb.v + atol * normA.v * normx.v, 1.0, code)
    code = torch.where(alpha.v == 0, 4.0, code)
    code = torch.where(beta.v == 0, 5.0, code)
    out = {ALPHA: alpha, BETA: beta, ALPHABAR: alphabar_n, ZETABAR: zetabar_n, RHO: rho, RHOBAR: rhobar, CBAR: cbar_n,
           SBAR: sbar_n, ZETA: zeta, BETADD: betadd_n, BETAD: betad_n, RHODOLD: rhodold_n, TAUTILDEOLD: tautildeold_n,
           THETATILDE: thetatilde, D: d_n, NORMA2: na2 + alpha * alpha, MAXRBAR: maxrbar, MINRBAR: minrbar,
           ITN: E(itn.v + 1), FLAG: E(code), NORMB: normb, NORMR: normr, NORMAR: normar, NORMA: normA, CONDA: condA,
           NORMX: normx, ALPHA1: g(ALPHA1)}
    return out, (c1, c2, c3), code


def _start_scalars(alpha, beta0, normb):
    z, one = E(torch.zeros_like(alpha.v)), E(torch.ones_like(alpha.v))
    out = {i: z for i in range(NST)}
    ab = alpha * beta0
    out.update({ALPHA: alpha, BETA: beta0, ALPHABAR: alpha, ZETABAR: ab, RHO: one, RHOBAR: one, CBAR: one,
                BETADD: beta0, RHODOLD: one, NORMA2: alpha * alpha, MINRBAR: E(torch.full_like(alpha.v, 1e100)),
                FLAG: E(torch.where(alpha.v == 0, 4.0, 0.0).to(torch.float64)), NORMB: normb, NORMR: beta0, NORMAR: ab,
                NORMA: alpha, CONDA: one, ALPHA1: alpha})
    return out


# ------------------------------------------------------------------------------------------------ the kernels
def init(env, b, Pb, k, fault=None):
    """xk_lsmr_init: beta = sqrt(sum Pb), uh = b (a copy: bound 0), the start state in slot k & 1 (all zero but beta,
    normb, normr = beta and the flag: 1 when beta = 0), run = 1 / 0."""
    beta = psum(Pb, env.nblk, drop=fault == "drop_block").sqrt()
    uh = b.clone()
    keep = _keep_mask(env, fault)
    uh[:, keep] = 0.0                                  # never written
    st = torch.zeros(env.S, NST, dtype=torch.float64)
    est = torch.zeros_like(st)
    flag = (beta.v == 0).to(torch.float64)
    for i in (BETA, NORMB, NORMR):
        st[:, i], est[:, i] = beta.v, beta.e
    st[:, FLAG] = flag
    return {"uh": (uh, torch.zeros_like(uh)), "state": (st, est), "run": (1.0 - flag, torch.zeros_like(flag)),
            "flag": flag}


def bidiag(env, Op, y, Pin, nblk_in, state, half, k, fault=None, wrong_n=None):
    """xk_lsmr_bidiag: nu_x = sqrt(sum Pin) (nblk_in partials), nu_y = beta (half 0) / alpha (half 1; 0: y not read);
    y' = Op (1 / nu_x) - (nu_x / nu_y) y (2 casts, 2 products, 1 subtraction); Pout = |y'|^2.  Frozen systems: nothing
    is written (`frozen`); nu_x = 0 (`zero`): y stays, Pout = 0.  fault u_len_n: run over wrong_n < N elements."""
    st = _slot(state, k, fault)
    frozen = st[:, FLAG] != 0
    nux = psum(Pin, nblk_in, drop=fault == "drop_block").sqrt()
    nuy = st[:, BETA if half == 0 else ALPHA]
    zero = (nux.v == 0) & ~frozen
    c0 = ediv(1.0, nux)
    c1 = ediv(nux, E(nuy))
    yz = torch.where(_c(nuy != 0), y, torch.zeros_like(y))
    t0, t1 = Op * _c(c0.v), _c(c1.v) * yz
    yn = t0 - t1
    ey = env.cu * (t0.abs() + t1.abs()) + _c(c0.e) * Op.abs() + _c(c1.e) * yz.abs()
    keepm = _keep_mask(env, fault)
    if fault == "u_len_n" and wrong_n is not None:
        keepm = keepm.clone()
        keepm[wrong_n * env.mul:] = True
    ctx = env.rctx
    ydot = torch.where(keepm, torch.zeros_like(yn), yn) if fault == "u_len_n" else yn
    dfault = fault if fault in ("drop_tail", "drop_block") else None
    pv, pb = kref._dot_total(ctx, ydot, ydot, dfault), kref._dot_bound(ctx, yn, yn, ey, ey)
    skip = frozen | zero
    out_y = torch.where(_c(skip), y, yn)
    ey = torch.where(_c(skip), torch.zeros_like(ey), ey)
    out_y = out_y.clone()
    out_y[:, keepm] = y[:, keepm]                      # a faulty kernel leaves these alone
    pv = torch.where(zero, torch.zeros_like(pv), pv)
    pb = torch.where(zero, torch.zeros_like(pb), pb)
    return {"y": (out_y, ey), "Pout": (pv, pb), "frozen": frozen, "zero": zero}


def update(env, vh, h, hbar, x, Pu, nblk_u, Pv, Pxin, state, k, damp, atol, btol, conlim, fault=None):
    """xk_lsmr_update (formulas in the module docstring and in `_scalars`).  Frozen systems: the state is carried over,
    nothing else is written.  Start systems (alpha = 0 in the slot read): h = vh / alpha_1 and the start state only.
    alpha_{k+1} = 0 / beta_{k+1} = 0: the step is taken (x is final), h = 0, flag 4 / 5."""
    st = _slot(state, k, fault)
    frozen = st[:, FLAG] != 0
    start = (st[:, ALPHA] == 0) & ~frozen
    reg = ~(frozen | start)
    alpha = psum(Pv, env.nblk, drop=fault == "drop_block").sqrt()
    beta = psum(Pu, nblk_u).sqrt()
    normx = psum(Pxin, env.nblk).sqrt()
    sd = {i: E(st[:, i]) for i in range(NST)}
    new, (c1, c2, c3), code = _scalars(sd, alpha, beta, normx, 0.0 if fault == "no_damp" else damp, atol, btol, conlim)
    snew = _start_scalars(alpha, sd[BETA], sd[NORMB])
    ia = ediv(1.0, alpha)
    # regular step
    t1 = _c(c1.v) * hbar
    hb = h - t1
    ehb = env.cu * (h.abs() + t1.abs()) + _c(c1.e) * hbar.abs()
    hx, ehx = (hbar, torch.zeros_like(ehb)) if fault == "hbar_after_x" else (hb, ehb)
    t2 = _c(c2.v) * hx
    xn = x + t2
    ex = env.cu * (x.abs() + t2.abs()) + _c(c2.v.abs()) * ehx + _c(c2.e) * hx.abs()
    ta, tb = vh * _c(ia.v), _c(c3.v) * h
    hn = ta - tb
    ehn = env.cu * (ta.abs() + tb.abs()) + _c(ia.e) * vh.abs() + _c(c3.e) * h.abs()
    # start step
    hs, ehs = ta, env.cu * ta.abs() + _c(ia.e) * vh.abs()
    R, St = _c(reg), _c(start)
    zero = torch.zeros_like(ehb)
    out_h = torch.where(R, hn, torch.where(St, hs, h))
    e_h = torch.where(R, ehn, torch.where(St, ehs, zero))
    out_hb, e_hb = torch.where(R, hb, hbar), torch.where(R, ehb, zero)
    out_x, e_x = torch.where(R, xn, x), torch.where(R, ex, zero)
    keep = _keep_mask(env, fault)
    if bool(keep.any()):
        out_h, out_hb, out_x = out_h.clone(), out_hb.clone(), out_x.clone()
        out_h[:, keep], out_hb[:, keep], out_x[:, keep] = h[:, keep], hbar[:, keep], x[:, keep]
    ctx = env.rctx
    dfault = fault if fault in ("drop_tail", "drop_block") else None
    so, eso = st.clone(), torch.zeros_like(st)
    for i in range(NST):
        so[:, i] = torch.where(reg, new[i].v, torch.where(start, snew[i].v, st[:, i]))
        eso[:, i] = torch.where(reg, new[i].e, torch.where(start, snew[i].e, torch.zeros_like(new[i].e)))
    run = (so[:, FLAG] == 0).to(torch.float64)
    return {"h": (out_h, e_h), "hbar": (out_hb, e_hb), "x": (out_x, e_x),
            "Pxout": (kref._dot_total(ctx, xn, xn, dfault), kref._dot_bound(ctx, xn, xn, ex, ex)),
            "state": (so, eso), "run": (run, torch.zeros_like(run)), "frozen": frozen, "start": start, "reg": reg}


# ------------------------------------------------------------------------------------------------ whole iteration
def iterate(fwd, adj, B, n, damp=0.0, atol=1e-6, btol=1e-6, conlim=1e8, max_niter=100, fault=None):
    """LSMR from x = 0 on the systems B (S, m) float64 / complex128 with `fwd(V) -> A V` ((S, n) -> (S, m)) and
    `adj(U) -> A^H U`: the recurrences of the kernels chained as the driver chains them (un-normalised vectors, the
    lagged |x|), scalars in float64, no confirmation and no resumption.  Returns x, niter, the stop codes (0: still
    running after max_niter) and the estimates of the last step."""
    S = B.shape[0]
    f64 = torch.float64
    nrm = lambda t: (t.conj() * t).sum(-1).real.to(f64).sqrt()
    one = torch.ones(S, dtype=f64)
    inv = lambda d: torch.where(d == 0, torch.zeros_like(d), 1.0 / torch.where(d == 0, one, d))
    uh = B.clone()
    beta = nrm(uh)
    vh = adj(uh) * _c(inv(beta))
    alpha = nrm(vh)
    st = _start_scalars(E(alpha), E(beta), E(beta))
    code = torch.where(beta == 0, 1.0, torch.where(alpha == 0, 4.0, 0.0)).to(f64)
    h = vh * _c(inv(alpha))
    hbar, x = torch.zeros_like(h), torch.zeros_like(h)
    normx = torch.zeros(S, dtype=f64)
    k = 0
    m = B.shape[-1]
    while k < max_niter and bool((code == 0).any()):
        live = code == 0
        L = _c(live)
        Av = fwd(vh)
        if fault == "u_len_n" and n < m:
            Av = Av.clone()
            Av[:, n:] = 0
        un = Av * _c(inv(alpha)) - _c(alpha * inv(beta)) * uh
        if fault == "u_len_n" and n < m:
            un[:, n:] = uh[:, n:]
        uh = torch.where(L, un, uh)
        bnew = nrm(uh)
        vn = adj(uh) * _c(inv(bnew)) - _c(bnew * inv(alpha)) * vh
        vnew = torch.where(_c(live & (bnew != 0)), vn, vh)
        anew = torch.where(bnew == 0, torch.zeros_like(bnew), nrm(vnew))
        new, (c1, c2, c3), ncode = _scalars(st, E(anew), E(bnew), E(normx), 0.0 if fault == "no_damp" else damp,
                                            atol, btol, conlim)
        hb = h - _c(c1.v) * hbar
        xn = x + _c(c2.v) * (hbar if fault == "hbar_after_x" else hb)
        hn = vnew * _c(inv(anew)) - _c(c3.v) * h
        normx = torch.where(live, nrm(xn), normx)
        h, hbar, x, vh = torch.where(L, hn, h), torch.where(L, hb, hbar), torch.where(L, xn, x), torch.where(L, vnew, vh)
        st = {i: E(torch.where(live, new[i].v, st[i].v)) for i in range(NST)}
        code = torch.where(live, ncode, code)
        alpha, beta = torch.where(live, anew, alpha), torch.where(live, bnew, beta)
        k += 1
    return {"x": x, "niter": k, "code": code, "normr": st[NORMR].v, "normar": st[NORMAR].v, "normA": st[NORMA].v,
            "condA": st[CONDA].v}


# ------------------------------------------------------------------------------------------------ inputs
def rand_state(g, S, k, frozen=(), first=(), other="nan"):
    """(2, S, NST) float64 state: slot k & 1 a plausible mid-iteration state, the other slot NaN-poisoned (other="nan")
    or another plausible state (other="rand": what a kernel reading the wrong slot would see); `frozen` systems carry
    flag 2, `first` systems a start slot (alpha = 0)"""
    st = torch.full((2, S, NST), math.nan, dtype=torch.float64)
    r = lambda: 0.5 + torch.rand(S, dtype=torch.float64, generator=g)
    for slot in ((k & 1,) if other == "nan" else (k & 1, (k + 1) & 1)):
        s = st[slot]
        th = 0.2 + 1.1 * torch.rand(S, dtype=torch.float64, generator=g)
        s[:, ALPHA], s[:, BETA], s[:, ALPHABAR], s[:, ZETABAR], s[:, RHO], s[:, RHOBAR] = r(), r(), r(), r() - 1.0, r(), r()
        s[:, CBAR], s[:, SBAR], s[:, ZETA] = torch.cos(th), torch.sin(th), r() - 1.0
        s[:, BETADD], s[:, BETAD], s[:, RHODOLD], s[:, TAUTILDEOLD], s[:, THETATILDE] = r(), r() - 1.0, r(), r() - 1.0, r() - 1.0
        s[:, D], s[:, NORMA2], s[:, MAXRBAR], s[:, MINRBAR], s[:, ITN], s[:, FLAG] = r(), 4 * r(), 1.5 * r(), 0.3 * r(), 3.0, 0.0
        s[:, NORMB], s[:, NORMR], s[:, NORMAR], s[:, NORMA], s[:, CONDA], s[:, NORMX] = 2 * r(), r(), r(), r(), r(), r()
        s[:, ALPHA1] = 0.6 * r()
        for i in first:
            beta0, nb = s[i, BETA].item(), s[i, NORMB].item()
            s[i] = 0.0
            s[i, BETA], s[i, NORMB], s[i, NORMR] = beta0, nb, beta0
        for i in frozen:
            s[i, FLAG] = 2.0
    return st


def spectrum_matrix(g, dtype, m, n, kappa, rank=None):
    """(m, n) float64 / complex128 matrix with singular values log-spaced in [1 / kappa, 1] (the last min(m, n) - rank
    of them zero), random singular vectors; returns (A, singular values)"""
    hp = torch.complex128 if dtype.is_complex else torch.float64
    r = min(m, n)

    def orth(k):
        Z = torch.randn(k, k, dtype=torch.float64, generator=g)
        if dtype.is_complex:
            Z = torch.complex(Z, torch.randn(k, k, dtype=torch.float64, generator=g))
        return torch.linalg.qr(Z)[0]
    sv = torch.logspace(0, -math.log10(kappa), r, dtype=torch.float64)
    if rank is not None:
        sv[rank:] = 0
    U, V = orth(m), orth(n)
    return (U[:, :r] * sv.to(hp)) @ V[:, :r].conj().T, sv


DTYPES, IDS = mref.DTYPES, mref.IDS
configs = mref.configs
CASES, CASE_IDS = mref.CASES, mref.CASE_IDS
TOLS = dict(damp=0.37, atol=0.05, btol=0.05, conlim=1e8)


def applicable(env, fault, kernel):
    """whether `fault` changes an output of `kernel` at this configuration"""
    if fault == "drop_tail":
        return env.n % env.rctx.vn != 0
    if fault == "drop_block":
        return True
    if fault == "wrong_slot":
        return kernel in ("bidiag", "update")
    if fault in ("no_damp", "hbar_after_x"):
        return kernel == "update"
    if fault == "u_len_n":
        return kernel == "bidiag" and env.N >= 4
    return False


class Case:
    """Host-side inputs of one configuration, in the kernel dtype and the panel contract of the Krylov kernels
    ([N, npad) zero, [npad, ld) NaN, partial slots [nblk, 64) NaN), and the references on them.  Systems with
    s % 5 == 1 are frozen, s % 5 == 2 take a first step (a start slot), s % 5 == 3 meet a zero norm (bidiag: nu_x = 0;
    update: beta_{k+1} = 0 for s % 10 == 3, alpha_{k+1} = 0 for s % 10 == 8); s % 5 == 4 are plain running systems
    (every system sees the damping rotation: the update runs with damp = TOLS["damp"]); S = 1 is a running system.
    The other side of the bidiagonalisation has length N2 = N + 3 (nblk2 blocks): m != n for both halves."""

    def __init__(self, dtype, N, S, extra, nblk, seed=0, k=3, other="nan"):
        self.dtype, self.N, self.S, self.nblk, self.k = dtype, N, S, nblk, k
        self.env = Env(dtype, S, N, nblk)
        vn = kref.VEC_ELEMS[dtype]
        self.npad = (N + vn - 1) // vn * vn
        self.ld = (N + 15) // 16 * 16 + extra
        self.N2 = N + 3
        self.nblk2 = max(1, min(64, nblk + 1))
        self.g = g = torch.Generator().manual_seed(seed)
        cls = lambda r: [s for s in range(S) if S > 1 and s % 5 == r]
        self.frozen, self.first, self.zero = cls(1), cls(2), cls(3)
        self.zero_b = [s for s in self.zero if s % 10 == 3]
        self.zero_a = [s for s in self.zero if s % 10 == 8]
        (self.Op, self.y, self.vh, self.h, self.hbar, self.x, self.b) = kref.rand_vecs(g, dtype, S, N, self.ld, 7)
        self.state = rand_state(g, S, k, frozen=self.frozen, first=self.first, other=other)
        rd = kref.REAL_OF[dtype]
        P = lambda nb, z: kref.rand_partials(g, rd, S, nb, zero_systems=z, positive=True)
        self.Pin = P(self.nblk2, self.zero)            # bidiag: partials of the other side
        self.Pb = P(nblk, self.zero)                   # init: |b|^2
        self.Pu = P(self.nblk2, self.zero_b)           # update: |uh|^2 of the other side
        self.Pv = P(nblk, self.zero)                   # update: |vh|^2 (beta = 0 implies alpha = 0)
        self.Pxin = P(nblk, ())

    def ref_init(self, fault=None):
        return init(self.env, self.env.vec(self.b), self.Pb, self.k, fault)

    def ref_bidiag(self, half, fault=None):
        e = self.env
        return bidiag(e, e.vec(self.Op), e.vec(self.y), self.Pin, self.nblk2, self.state, half, self.k, fault,
                      wrong_n=max(1, self.N - 3))

    def ref_update(self, fault=None):
        e = self.env
        return update(e, e.vec(self.vh), e.vec(self.h), e.vec(self.hbar), e.vec(self.x), self.Pu, self.nblk2, self.Pv,
                      self.Pxin, self.state, self.k, fault=fault, **TOLS)


comparable = mref.comparable
