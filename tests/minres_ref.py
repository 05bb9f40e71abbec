"""Float64 restatement of the MINRES step kernels of xk_minres.hip and of the whole iteration, with error bounds.

In the manner of tests/krylov_ref.py (whose block layout, partial-sum helpers, `check()` and input generators are
reused): for every kernel (xk_minres_init, xk_minres_lanczos, xk_minres_update) a function computes, from the very
inputs the kernel is given, what the kernel must write, and returns {name: (value, bound)}.

The recurrences are those of Paige & Saunders (1975): Lanczos on the (preconditioned) operator,
    beta_{k+1} v_{k+1} = A v_k - alpha_k v_k - beta_k v_{k-1},
carried on the UN-normalised vectors r1 = beta_k v_{k-1}-like and r2 = beta_k v_k-like (so that a preconditioner only
enters through y = P r2 and beta^2 = <r2, y>); one Givens rotation per step,
    delta = cs dbar + sn alpha,  gbar = sn dbar - cs alpha,  gamma = sqrt(gbar^2 + beta_new^2),
    cs' = gbar / gamma,  sn' = beta_new / gamma,  epsln' = sn beta_new,  dbar' = -cs beta_new,
and from W R = V the direction  w = (v - epsln w_{k-2} - delta w_{k-1}) / gamma,  x += phi w,  phi = cs' phibar,
phibar' = sn' phibar  (start: cs = -1, sn = 0, dbar = epsln = 0, phibar = beta_1).

Complex systems: every scalar above is real for a Hermitian operator, so the kernels run on the interleaved (re, im)
storage as real vectors of length 2N; so do the functions here (`Env.vec` returns that view).  The only complex
arithmetic is the conjugated inner product of xk_kry_dots (`alpha_dot`), of which the real part is used.

Bounds.  u is the unit roundoff of the kernel dtype, U_D = 2^-53 that of the double scalar state.
  * vectors: C_MR * u * sum|terms| plus the propagated error of the scalars.  The longest chain is x = x + phi w with
    w = ((v - e w1) - d w2) g: three casts of a double to the vector type, three products, two subtractions, the
    product with g, the product with phi and the final addition: 9 roundings on the longest path to first order; the
    float64 reference carries the same chain for the float64 kernels, at most doubling that: C_MR = 20.
  * scalar state: first-order propagation of the error of the double sums (64-lane tree, <= 8 U_D sum|p|), written out
    next to each formula below with the number of roundings of that formula, times C_ST = 4 for the reference's own
    rounding and fused multiply-adds.
`fault=` produces plausible bugs: FAULTS.  tests/test_minres_ref.py shows that `check()` rejects each of them."""
import math
import torch
from tests import krylov_ref as kref

NST = 12
BETA, OLDB, CS, SN, DBAR, EPSLN, PHIBAR, FLAG, ALPHA, GAMMA, DELTA, PHI = range(12)
U_D = 2.0 ** -53
C_MR = 20.0
C_ST = 4.0

FAULTS = ("drop_tail", "drop_block", "noconj", "wrong_slot", "no_rotate", "w_off_by_one")

check = kref.check


class Env:
    """shape / type facts of a launch; vectors are handled as REAL arrays of length n = N (real) or 2N (complex)"""

    def __init__(self, dtype, S, N, nblk):
        self.dtype, self.S, self.N, self.nblk = dtype, S, N, nblk
        self.cplx = dtype.is_complex
        self.mul = 2 if self.cplx else 1
        self.pstride = self.mul
        self.rdtype = kref.REAL_OF[dtype]
        self.n = N * self.mul
        self.rctx = kref.Ctx(self.rdtype, S, self.n, nblk)       # block layout of the real view: same blocks
        self.cctx = kref.Ctx(dtype, S, N, nblk)
        self.u = kref.unit_roundoff(dtype)
        self.cu = C_MR * self.u

    def vec(self, t):
        """[0, N) of an (S, ld) array as float64 (S, n); complex arrays as interleaved (re, im)"""
        t = t.detach().cpu()[:, :self.N]
        if t.is_complex():
            return torch.view_as_real(t.to(torch.complex128).contiguous()).reshape(self.S, self.n).clone()
        return t.to(torch.float64)

    def unvec(self, r):
        """inverse of `vec`: (S, n) float64 -> (S, N) float64 / complex128"""
        if self.cplx:
            return torch.view_as_complex(r.reshape(self.S, self.N, 2).contiguous())
        return r


def psum_real(env, P, stride=None, fault=None):
    """the kernels' double sum of the real parts of the used partial slots: (value, bound)"""
    P = P.detach().cpu().to(torch.float64)
    if P.dim() == 3:
        P = P[..., 0]
    p = P[:, :env.nblk].clone()
    if fault == "drop_block":
        p[:, env.nblk - 1] = 0
    return p.sum(-1), 8 * U_D * p.abs().sum(-1)


def _slot(state, k, fault):
    kk = k + 1 if fault == "wrong_slot" else k
    return state[kk & 1].detach().cpu().to(torch.float64)


def _keep_mask(env, fault):
    """elements of [0, n) a faulty kernel fails to write (drop_tail: the last partial 16 B vector; drop_block: the
    last non-empty block)"""
    m = torch.zeros(env.n, dtype=torch.bool)
    vn = env.rctx.vn
    if fault == "drop_tail":
        m[env.n - env.n % vn:] = True
    if fault == "drop_block":
        ne = [b for b in range(env.nblk) if kref.block_range(env.n, env.nblk, b, vn)[0] < env.n]
        lo, hi = kref.block_range(env.n, env.nblk, ne[-1], vn)
        m[lo:hi] = True
    return m


def _c(t):
    return t.unsqueeze(-1)


def alpha_dot(env, v, Av, fault=None):
    """what xk_kry_dots must leave in Palpha for MINRES: the partials of <v, Av> = sum conj(v) Av, of which the
    kernels take the REAL part.  v, Av: (S, N) float64 / complex128.  Returns {"alpha": (value, bound)}."""
    ctx = env.cctx
    val = kref._dot_total(ctx, v, Av, fault)
    bnd = kref._dot_bound(ctx, v, Av)
    return {"alpha": (val.real if val.is_complex() else val, bnd)}


def init(env, y0, Pb, k, fault=None):
    """xk_minres_init: beta = sqrt(sum Pb) (1 rounding + the sum), v = y0 * (1 / beta) (cast + product),
    the start state in slot k & 1, phi2 = beta^2.  Systems with sum Pb = 0 are frozen (flag 1, v = 0), with
    sum Pb < 0 flagged 2 (v = 0, phi2 = +inf: not compared here)."""
    bb, ebb = psum_real(env, Pb, fault=fault)
    flag = torch.where(bb < 0, 2.0, torch.where(bb == 0, 1.0, 0.0)).to(torch.float64)
    beta = bb.clamp(min=0).sqrt()
    live = flag == 0
    sb = torch.where(live, beta, torch.ones_like(beta))
    ebeta = torch.where(live, C_ST * (ebb / (2 * sb) + 2 * U_D * beta), torch.zeros_like(beta))
    v = torch.where(_c(live), y0 / _c(sb), torch.zeros_like(y0))
    ev = env.cu * v.abs() + _c(ebeta / sb) * v.abs()
    keep = _keep_mask(env, fault)
    if bool(keep.any()):
        v = v.clone()
        v[:, keep] = 0.0                               # never written
    st = torch.zeros(env.S, NST, dtype=torch.float64)
    est = torch.zeros(env.S, NST, dtype=torch.float64)
    st[:, BETA], st[:, PHIBAR], st[:, CS], st[:, FLAG] = beta, beta, -1.0, flag
    est[:, BETA], est[:, PHIBAR] = ebeta, ebeta
    phi2 = beta * beta
    return {"v": (v, ev), "state": (st, est), "phi2": (phi2, env.cu * phi2 + 2 * beta * ebeta), "flag": flag}


def lanczos(env, Av, r2, r1, Palpha, state, k, fault=None):
    """xk_minres_lanczos: c2 = alpha / beta, c1 = beta / oldb (0 on a first step: r1 is then not read);
    y = (Av - c2 r2) - c1 r1 (2 casts, 2 products, 2 subtractions) written over r1; Pbeta = |y|^2.
    Frozen systems (flag != 0): r1 and Pbeta are left alone (`frozen` lists them)."""
    st = _slot(state, k, fault)
    frozen = st[:, FLAG] != 0
    alpha, ea = psum_real(env, Palpha, fault=fault if fault == "drop_block" else None)
    beta, oldb = st[:, BETA], st[:, OLDB]
    sb = torch.where(beta == 0, torch.ones_like(beta), beta)
    c2 = alpha / sb
    ec2 = C_ST * (ea / sb.abs() + 2 * U_D * c2.abs())
    has1 = oldb != 0
    c1 = torch.where(has1, beta / torch.where(has1, oldb, torch.ones_like(oldb)), torch.zeros_like(beta))
    r1z = torch.where(_c(has1), r1, torch.zeros_like(r1))
    a, b = (r1z, r2) if fault == "no_rotate" else (r2, r1z)
    y = (Av - _c(c2) * a) - _c(c1) * b
    ey = env.cu * (Av.abs() + _c(c2.abs()) * a.abs() + _c(c1.abs()) * b.abs()) + _c(ec2) * a.abs()
    ctx = env.rctx
    dfault = fault if fault in ("drop_tail", "drop_block") else None
    out = {"Pbeta": (kref._dot_total(ctx, y, y, dfault), kref._dot_bound(ctx, y, y, ey, ey)), "frozen": frozen}
    yv, eyv = y.clone(), ey.clone()
    yv[frozen], eyv[frozen] = r1[frozen], 0.0
    keep = _keep_mask(env, fault)
    yv[:, keep] = r1[:, keep]                          # a faulty kernel leaves these alone
    out["r1"] = (yv, eyv)
    return out


def update(env, v, y, w1, w2, x, Palpha, Pbeta, state, k, fault=None):
    """xk_minres_update: the rotation (formulas in the module docstring), w over w1, x += phi w, v <- y / beta_new,
    state slot (k + 1) & 1, phi2 = phibar'^2.  Frozen systems: the state is carried over, nothing else is written;
    sum Pbeta < 0: flag 2 (phi2 = +inf, not compared); gamma = 0: flag 3; beta_new = 0: flag 1 after the update, v = 0."""
    st = _slot(state, k, fault)
    frozen = st[:, FLAG] != 0
    alpha, ea = psum_real(env, Palpha)
    bb, ebb = psum_real(env, Pbeta, fault=fault if fault == "drop_block" else None)
    beta, cs, sn, dbar, phibar, oldeps = st[:, BETA], st[:, CS], st[:, SN], st[:, DBAR], st[:, PHIBAR], st[:, EPSLN]
    negb = (bb < 0) & ~frozen
    bnew = bb.clamp(min=0).sqrt()
    one = torch.ones_like(bnew)
    sbn = torch.where(bnew == 0, one, bnew)
    ebn = torch.where(bnew == 0, ebb.sqrt(), C_ST * (ebb / (2 * sbn) + 2 * U_D * bnew))        # sqrt: 1 rounding
    delta = cs * dbar + sn * alpha                                                               # 3 roundings
    edelta = C_ST * (sn.abs() * ea + 3 * U_D * ((cs * dbar).abs() + (sn * alpha).abs()))
    gbar = sn * dbar - cs * alpha
    egbar = C_ST * (cs.abs() * ea + 3 * U_D * ((sn * dbar).abs() + (cs * alpha).abs()))
    gamma = torch.sqrt(gbar * gbar + bnew * bnew)                                                # 4 roundings
    stuck = (gamma == 0) & ~frozen & ~negb
    sg = torch.where(gamma == 0, one, gamma)
    egamma = (gbar.abs() * egbar + bnew * ebn) / sg + C_ST * 4 * U_D * gamma
    csn, snn = gbar / sg, bnew / sg
    ecsn = (egbar + csn.abs() * egamma) / sg + C_ST * U_D * csn.abs()
    esnn = (ebn + snn.abs() * egamma) / sg + C_ST * U_D * snn.abs()
    phi, phibar_n = csn * phibar, snn * phibar
    ephi = ecsn * phibar.abs() + C_ST * U_D * phi.abs()
    ephibar = esnn * phibar.abs() + C_ST * U_D * phibar_n.abs()
    done = (bnew == 0) & ~frozen & ~negb & ~stuck
    live = ~(frozen | negb | stuck)

    a, b = (w2, w1) if fault == "w_off_by_one" else (w1, w2)
    ig = 1.0 / sg
    mag = (v.abs() + _c(oldeps.abs()) * a.abs() + _c(delta.abs()) * b.abs()) * _c(ig)
    w = ((v - _c(oldeps) * a) - _c(delta) * b) * _c(ig)
    ew = env.cu * mag + _c(edelta * ig) * b.abs() + _c(egamma * ig) * w.abs()
    xn = x + _c(phi) * w
    ex = env.cu * (x.abs() + _c(phi.abs()) * w.abs()) + _c(phi.abs()) * ew + _c(ephi) * w.abs()
    vn = torch.where(_c(done), torch.zeros_like(y), y / _c(sbn))
    evn = env.cu * vn.abs() + _c(ebn / sbn) * vn.abs()

    L = _c(live)
    out_w, out_x, out_v = torch.where(L, w, w1), torch.where(L, xn, x), torch.where(L, vn, v)
    zero = torch.zeros_like(ew)
    ew, ex, evn = torch.where(L, ew, zero), torch.where(L, ex, zero), torch.where(L, evn, zero)
    keep = _keep_mask(env, fault)
    if bool(keep.any()):
        out_w, out_x, out_v = out_w.clone(), out_x.clone(), out_v.clone()
        out_w[:, keep], out_x[:, keep], out_v[:, keep] = w1[:, keep], x[:, keep], v[:, keep]

    so = st.clone()
    eso = torch.zeros_like(so)
    new = {BETA: (bnew, ebn), OLDB: (beta, 0 * beta), CS: (csn, ecsn), SN: (snn, esnn),
           DBAR: (-cs * bnew, cs.abs() * ebn + C_ST * U_D * (cs * bnew).abs()),
           EPSLN: (sn * bnew, sn.abs() * ebn + C_ST * U_D * (sn * bnew).abs()),
           PHIBAR: (phibar_n, ephibar), FLAG: (done.to(torch.float64), 0 * beta), ALPHA: (alpha, ea),
           GAMMA: (gamma, egamma), DELTA: (delta, edelta), PHI: (phi, ephi)}
    for i, (val, err) in new.items():
        so[:, i] = torch.where(live, val, st[:, i])
        eso[:, i] = torch.where(live, err, torch.zeros_like(err))
    so[:, FLAG] = torch.where(negb, 2.0, torch.where(stuck, 3.0, so[:, FLAG]))
    phi2 = phibar_n * phibar_n
    return {"w": (out_w, ew), "x": (out_x, ex), "v": (out_v, evn), "state": (so, eso),
            "phi2": (phi2, env.cu * phi2 + 2 * phibar_n.abs() * ephibar),
            "live": live, "frozen": frozen, "negb": negb}


# ------------------------------------------------------------------------------------------------ whole iteration
def iterate(apply, B, stop, max_niter, pre=None, steps=None, fault=None):
    """MINRES from x0 = 0 on the systems B (S, N) float64 / complex128 with `apply(V) -> A V` (and `pre(R) -> P R`):
    the recurrences of the kernels chained as the driver chains them, scalars in float64, no true-residual
    confirmation.  Stops when every phibar_s <= ... passes the driver's test !(phibar < stop) nowhere, or after
    `max_niter` iterations; `steps=k` runs exactly k iterations.  Returns x, niter, hist (max phibar per iteration),
    phibar."""
    S = B.shape[0]
    f64 = torch.float64
    dot = lambda a, b: (a.conj() * b).sum(-1).real.to(f64)
    r2 = B.clone()
    y = pre(r2) if pre is not None else r2
    bb = dot(r2, y)
    assert bool((bb >= 0).all()), "preconditioner not positive definite"
    beta = bb.sqrt()
    frozen = beta == 0
    one = torch.ones(S, dtype=f64)
    safe = lambda d: torch.where(d == 0, one, d)
    v = torch.where(_c(frozen), torch.zeros_like(y), y / _c(safe(beta)))
    oldb, cs, sn = torch.zeros(S, dtype=f64), -one.clone(), torch.zeros(S, dtype=f64)
    dbar, epsln, phibar = torch.zeros(S, dtype=f64), torch.zeros(S, dtype=f64), beta.clone()
    x, w1, w2, r1 = (torch.zeros_like(B) for _ in range(4))
    hist, k = [], 0
    nit = steps if steps is not None else max_niter
    if steps is None and bool((phibar < stop).all()):
        nit = 0
    while k < nit:
        Av = apply(v)
        alpha = dot(v, Av)
        c1 = torch.where(oldb != 0, beta / safe(oldb), torch.zeros_like(beta))
        a, b = (r1, r2) if fault == "no_rotate" else (r2, r1)
        ynew = (Av - _c(alpha / safe(beta)) * a) - _c(c1) * b
        r1, r2 = r2, ynew
        y = pre(r2) if pre is not None else r2
        bb = dot(r2, y)
        assert bool(((bb >= 0) | frozen).all()), "preconditioner not positive definite"
        bnew = bb.clamp(min=0).sqrt()
        delta = cs * dbar + sn * alpha
        gbar = sn * dbar - cs * alpha
        gamma = torch.sqrt(gbar * gbar + bnew * bnew)
        stuck = (gamma == 0) & ~frozen
        live = ~(frozen | stuck)
        csn, snn = gbar / safe(gamma), bnew / safe(gamma)
        phi = csn * phibar
        wa, wb = (w2, w1) if fault == "w_off_by_one" else (w1, w2)
        w = ((v - _c(epsln) * wa) - _c(delta) * wb) / _c(safe(gamma))
        x = torch.where(_c(live), x + _c(phi) * w, x)
        phibar = torch.where(live, snn * phibar, phibar)
        w1, w2 = w2, torch.where(_c(live), w, w2)
        done = live & (bnew == 0)
        frozen = frozen | stuck | done
        v = torch.where(_c(frozen), torch.zeros_like(y), y / _c(safe(bnew)))
        epsln, dbar, oldb, beta, cs, sn = sn * bnew, -cs * bnew, beta, bnew, csn, snn
        k += 1
        hist.append(float(phibar.max()))
        if steps is None and bool((phibar < stop).all()):
            break
    return {"x": x, "niter": k, "hist": hist, "phibar": phibar}


# ------------------------------------------------------------------------------------------------ inputs
def rand_state(g, S, k, frozen=(), first=(), negative_cs=True):
    """(2, S, NST) float64 state: slot k & 1 plausible (cs^2 + sn^2 = 1, beta, oldb in [0.5, 1.5)), the other slot
    NaN-poisoned; `frozen` systems carry flag 1, `first` systems oldb = 0 (a first step)"""
    st = torch.full((2, S, NST), math.nan, dtype=torch.float64)
    r = lambda: 0.5 + torch.rand(S, dtype=torch.float64, generator=g)
    th = 2 * math.pi * torch.rand(S, dtype=torch.float64, generator=g)
    s = st[k & 1]
    s[:, BETA], s[:, OLDB], s[:, CS], s[:, SN] = r(), r(), torch.cos(th), torch.sin(th)
    s[:, DBAR], s[:, EPSLN], s[:, PHIBAR], s[:, FLAG] = r() - 1.0, r() - 1.0, r(), 0.0
    s[:, ALPHA], s[:, GAMMA], s[:, DELTA], s[:, PHI] = r(), r(), r(), r()
    for i in first:
        s[i, OLDB], s[i, CS], s[i, SN], s[i, DBAR], s[i, EPSLN] = 0.0, -1.0, 0.0, 0.0, 0.0
    for i in frozen:
        s[i, FLAG] = 1.0
    return st


def hermitian(g, dtype, n, evals):
    """dense Hermitian float64 / complex128 matrix with the given eigenvalues and a random unitary basis"""
    hp = torch.complex128 if dtype.is_complex else torch.float64
    if dtype.is_complex:
        Z = torch.complex(torch.randn(n, n, dtype=torch.float64, generator=g),
                          torch.randn(n, n, dtype=torch.float64, generator=g))
    else:
        Z = torch.randn(n, n, dtype=torch.float64, generator=g)
    Q, _ = torch.linalg.qr(Z)
    A = (Q * evals.to(hp)) @ Q.conj().T
    return (A + A.conj().T) / 2, Q


# ------------------------------------------------------------------------------------------------ shared cases
DTYPES = [torch.float64, torch.float32, torch.complex128, torch.complex64]
IDS = ["f64", "f32", "c128", "c64"]


def default_nblk(dtype, N):
    """the driver's sizing rule (linalg._panel.kry_blocks), restated"""
    vn = kref.VEC_ELEMS[dtype]
    return max(1, min(64, (N + 256 * vn * 4 - 1) // (256 * vn * 4)))


def configs(dtype):
    """(N, S, extra pitch, nblk): N below / at / off the 16 B vector width, one block and many blocks (more blocks
    than vectors, the 64-block cap, the driver's own choice), S = 1 and many"""
    vn = kref.VEC_ELEMS[dtype]
    one = 1024 * vn
    cfg = [(1, 3, 0, 1), (vn + 1, 5, 8, 1), (5, 1, 0, 7), (1000, 5, 0, 1), (1000, 257, 8, 2), (1000, 1, 8, 64),
           (one + 1, 5, 8, default_nblk(dtype, one + 1)), (5 * one + 37, 5, 0, default_nblk(dtype, 5 * one + 37)),
           (5 * one + 37, 1, 8, 7)]
    if vn > 1:
        cfg.insert(1, (vn - 1, 5, 8, 1))
    return cfg


CASES = [(d, c) for d in DTYPES for c in configs(d)]
CASE_IDS = ["%s-N%d-S%d-ld+%d-nb%d" % (IDS[DTYPES.index(d)], c[0], c[1], c[2], c[3]) for d, c in CASES]


def applicable(env, fault, kernel):
    """whether `fault` changes an output of `kernel` at this configuration"""
    if fault == "drop_tail":
        # (a dot product of many terms hides one dropped term inside its own rounding bound: the vector outputs show it)
        return env.n % env.rctx.vn != 0 and (kernel != "alpha_dot" or env.N <= 8)
    if fault == "drop_block":
        return True
    if fault == "noconj":
        return kernel == "alpha_dot" and env.cplx
    if fault == "wrong_slot":
        return kernel in ("lanczos", "update")
    if fault == "no_rotate":
        return kernel == "lanczos"
    if fault == "w_off_by_one":
        return kernel == "update"
    return False


class Case:
    """Host-side inputs of one configuration, in the kernel dtype and the panel contract of the Krylov kernels
    ([N, npad) zero, [npad, ld) NaN, partial slots [nblk, 64) NaN), and the references on them.  Systems with
    s % 5 == 1 are frozen, s % 5 == 2 take a first step (oldb = 0), s % 5 == 3 get beta_new = 0 and s % 5 == 4 a
    negative <r2, P r2> (update) / <b, P b> (init); S = 1 is a plain running system."""

    def __init__(self, dtype, N, S, extra, nblk, seed=0, k=3):
        self.dtype, self.N, self.S, self.nblk, self.k = dtype, N, S, nblk, k
        self.env = Env(dtype, S, N, nblk)
        vn = kref.VEC_ELEMS[dtype]
        self.npad = (N + vn - 1) // vn * vn
        self.ld = (N + 15) // 16 * 16 + extra
        self.g = g = torch.Generator().manual_seed(seed)
        cls = lambda r: [s for s in range(S) if S > 1 and s % 5 == r]
        self.frozen, self.first, self.zero_b, self.neg_b = cls(1), cls(2), cls(3), cls(4)
        (self.v, self.Av, self.r1, self.r2, self.y, self.w1, self.w2, self.x) = kref.rand_vecs(g, dtype, S, N, self.ld, 8)
        self.state = rand_state(g, S, k, frozen=self.frozen, first=self.first)
        self.Palpha = kref.rand_partials(g, dtype, S, nblk)
        rd = kref.REAL_OF[dtype]
        self.Pbeta = kref.rand_partials(g, rd, S, nblk, zero_systems=self.zero_b, positive=True)
        self.Pdot = kref.rand_partials(g, dtype, S, nblk, zero_systems=self.zero_b, positive=True)
        for s in self.neg_b:
            self.Pbeta[s, :nblk] *= -1
            self.Pdot[s, :nblk] *= -1

    def ref_alpha_dot(self, fault=None):
        X = lambda t: kref.hp(t)[:, :self.N]
        return alpha_dot(self.env, X(self.v), X(self.Av), fault)

    def ref_init(self, fault=None):
        return init(self.env, self.env.vec(self.y), self.Pdot, self.k, fault)

    def ref_lanczos(self, fault=None):
        e = self.env
        return lanczos(e, e.vec(self.Av), e.vec(self.r2), e.vec(self.r1), self.Palpha, self.state, self.k, fault)

    def ref_update(self, fault=None, dot=False):
        e = self.env
        return update(e, e.vec(self.v), e.vec(self.y), e.vec(self.w1), e.vec(self.w2), e.vec(self.x), self.Palpha,
                      self.Pdot if dot else self.Pbeta, self.state, self.k, fault)


def comparable(ref, names, mask=None):
    """the (value, bound) entries `names` of a reference, restricted to the systems of `mask`"""
    out = {}
    for n in names:
        val, bnd = ref[n]
        out[n] = (val, bnd) if mask is None else (val[mask], bnd[mask])
    return out
