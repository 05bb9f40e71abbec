"""Float64 (and extended precision) restatement of the solver-side kernels that had no reference yet, with error
bounds: xk_gmres_step / xk_gmres_finish / xk_gmres_solve (xk_gmres.hip), xk_vec_dots / xk_broyden_axpy
(xk_broyden.hip) and xk_dense_outer / xk_banded_grad (xk_grad.hip).

Every function computes, from the very inputs the kernel is given, what the kernel must write, and returns
{name: (value, bound)}: `value` in float64, `bound` a per-entry absolute bound on |kernel - value| of the form
C * u * (sum of the magnitudes of the terms), u the unit roundoff of the arithmetic the kernel uses for that output
(the GMRES state is double whatever the vector type), C the length of the rounding chain (derived next to each
function).  Where the magnitudes vanish the bound is 0: such entries are checked exactly.  `check()` compares a
kernel's outputs with that, raises AssertionError naming the first entry out of bounds and records the largest
|kernel - value| / bound per (kernel, dtype) in WORST.

The `fault=` argument of the functions produces plausible kernel bugs (FAULTS).  tests/test_solver_ref.py feeds those
outputs to `check()` at every configuration of the GPU test (the *_CONFIGS lists and *_case builders below are shared
by both) and asserts that every fault is rejected wherever VISIBLE says it can be seen.

The small per-system GMRES recurrences run in numpy.longdouble (u = 2^-64 where the platform has an extended type), so
the reference's own rounding does not eat into a float64 bound; the factor REF = 2 in the bounds keeps them valid where
longdouble is plain double, and covers the float64 reference sums of the streaming kernels.
"""
import functools
import math
import numpy as np
import torch
from tests.krylov_ref import unit_roundoff, hp, VEC_ELEMS

U64 = 2.0 ** -53
LD = np.longdouble
REF = 2.0                       # the reference's own rounding, at most that of the kernel (see the module docstring)
DNAME = {torch.float64: "f64", torch.float32: "f32"}
DTYPES = [torch.float64, torch.float32]

# One Givens step on an entry is two products and an addition (2 roundings on either term), the new rotation a
# square root of a two-term sum and a division (4 roundings), R[k,k] = c a + t b on top of those (3 more): the longest
# chain of xk_gmres_step is 7 roundings.  C_ST = 8.
C_ST = 8.0
# xk_vec_dots folds after the per-lane sums: wave_sum over 64 lanes (6 levels) + the 4-wave combine (2) + the finish
# kernel's sequential loop over <= 1024 / 64 = 16 block partials per lane + its 64-lane wave_sum (6) + the rounding
# of each product (1)
VD_TREE = 6 + 2 + 16 + 6 + 1
VD_MAX_BLOCKS = 1024

FAULTS_GMRES_STEP = ("rot_sign", "rot_skip_last", "hn_no_sub", "abs_a", "g_not_rotated", "est_not_squared")
FAULTS_GMRES_FINISH = ("finish_drop_tail", "finish_no_scale", "finish_c1")
FAULTS_GMRES_SOLVE = ("solve_lane_wrap", "solve_pivot_nan")
FAULTS_VEC_DOTS = ("drop_tail", "drop_block")
FAULTS_AXPY = ("scale_ignored", "gamma_on_u", "unroll_tail")
FAULTS_OUTER = ("second_pass_overwrites", "accumulate_ignored")
FAULTS_BANDED = ("second_pass_overwrites", "halo_shift", "accumulate_ignored")

# worst |kernel - reference| / bound seen by check(), per (kernel, dtype name) (reported by the GPU runs)
WORST = {}


def _ld(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().double().numpy()
    return np.asarray(x, dtype=LD)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64)))


def npad_of(N, dtype):
    vn = VEC_ELEMS[dtype]
    return (N + vn - 1) // vn * vn


def cast(x, dtype):
    """the (T) cast the C entry points apply to their double arguments"""
    return float(torch.tensor(float(x), dtype=torch.float64).to(dtype).item())


# ------------------------------------------------------------------------------------------------ checking
def check(got, ref, kernel, dtype, what=""):
    """Compare kernel outputs (`got`: name -> tensor of the reference value's shape) with `ref`
    (name -> (value, bound)).  NaN and inf count as out of bounds; a zero bound demands equality."""
    worst = 0.0
    for name, (val, bnd) in ref.items():
        assert name in got, "%s: no kernel output %r" % (what, name)
        assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(bnd).all()), \
            "%s: reference %s is not finite" % (what, name)
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
    key = (kernel, DNAME[dtype])
    WORST[key] = max(WORST.get(key, 0.0), worst)
    return worst


def values(ref, dtype=None, keep64=()):
    """the reference values alone, rounded to the kernel dtype (names in `keep64` stay double: the GMRES state)"""
    out = {}
    for name, (val, _) in ref.items():
        out[name] = val if (dtype is None or name in keep64) else val.to(dtype)
    return out


# ================================================================================================ xk_gmres_step
STEP_STATE = ("Rcol", "cs_k", "sn_k", "g_k", "g_k1")          # double outputs; inv_hn and est2 are in T


def _step(dtype, a1, a2, k, cs, sn, e_cs, e_sn, gk, e_gk, fault=None):
    """one xk_gmres_step in longdouble with running first-order error bounds.  a1 = c1, a2 = c2n (S, >= k + 2),
    cs / sn (S, >= k) with absolute errors e_cs / e_sn, gk = g[k] with error e_gk."""
    uT = unit_roundoff(dtype)
    cu = C_ST * U64
    ab = np.abs
    c2 = a2[:, :k + 1]
    ss = (c2 * c2).sum(1)
    top = a2[:, k + 1]
    # n2 = |w1|^2 - |c2|^2 is a (k + 2)-term sum: error <= u (k + 3) (|c2n[k+1]| + sum c2^2);  d sqrt(x) = dx / (2 sqrt x)
    n2 = top if fault == "hn_no_sub" else top - ss
    e_n2 = U64 * (k + 3) * (ab(top) + ss)
    assert bool(((ab(top - ss) > 16 * e_n2) | (e_n2 == 0)).all()), "n2 within rounding of zero: hn is undetermined"
    pos = n2 > 0
    hn = np.sqrt(np.where(pos, n2, 0))
    e_hn = np.where(pos, e_n2 / (2 * np.where(pos, hn, 1)) + cu * hn, 0)
    h = a1[:, :k + 1] + a2[:, :k + 1]
    e_h = U64 * (ab(a1[:, :k + 1]) + ab(a2[:, :k + 1]))
    S = a1.shape[0]
    Rcol, e_R = np.zeros((S, k + 1), LD), np.zeros((S, k + 1), LD)
    prev, e_prev = h[:, 0], e_h[:, 0]
    nrot = max(k - 1, 0) if fault == "rot_skip_last" else k
    for j in range(nrot):
        nxt, e_nxt = h[:, j + 1], e_h[:, j + 1]
        c, t, ec, et = cs[:, j], sn[:, j], e_cs[:, j], e_sn[:, j]
        Rcol[:, j] = c * prev + t * nxt
        e_R[:, j] = ab(c) * e_prev + ab(t) * e_nxt + ec * ab(prev) + et * ab(nxt) + cu * (ab(c * prev) + ab(t * nxt))
        new = (t if fault == "rot_sign" else -t) * prev + c * nxt
        e_prev = ab(t) * e_prev + ab(c) * e_nxt + et * ab(prev) + ec * ab(nxt) + cu * (ab(t * prev) + ab(c * nxt))
        prev = new
    if fault == "rot_skip_last" and k >= 1:
        Rcol[:, k - 1] = prev
        prev = h[:, k]
    a, e_a = prev, e_prev
    den = np.sqrt(a * a + hn * hn)
    nz = den > 0
    ds = np.where(nz, den, 1)
    c = np.where(nz, (ab(a) if fault == "abs_a" else a) / ds, 1)
    t = np.where(nz, hn / ds, 0)
    # |dc/da| = b^2 / den^3, |dc/db| = |a b| / den^3, both <= 1 / den (likewise for t)
    e_c = np.where(nz, (e_a + e_hn) / ds + cu, 0)
    e_t = np.where(nz & (hn > 0), e_c, 0)                   # hn = 0 exactly: t = 0 / den = 0 exactly
    Rcol[:, k] = c * a + t * hn
    e_R[:, k] = e_a + e_hn + cu * den
    g_k = gk if fault == "g_not_rotated" else c * gk
    e_g_k = e_c * ab(gk) + ab(c) * e_gk + cu * ab(c * gk)
    gn = -t * gk
    e_gn = e_t * ab(gk) + ab(t) * e_gk + cu * ab(gn)
    hs = np.where(hn > 0, hn, 1)
    inv = np.where(hn > 0, 1 / hs, 0)
    e_inv = np.where(hn > 0, e_hn / (hs * hs) + (cu + uT) / hs, 0)
    est = ab(gn) if fault == "est_not_squared" else gn * gn
    e_est = 2 * ab(gn) * e_gn + (cu + uT) * gn * gn
    return dict(Rcol=(Rcol, e_R), cs_k=(c, e_c), sn_k=(t, e_t), g_k=(g_k, e_g_k), g_k1=(gn, e_gn),
                inv_hn=(inv, e_inv), est2=(est, e_est), a=(a, e_a), hn=(hn, e_hn))


def gmres_step(dtype, c1, c2n, k, cs, sn, g, fault=None):
    """xk_gmres_step on exact state: c1 (S, >= k + 1) and c2n (S, >= k + 2) in T, cs / sn (S, >= k) and g (S, >= k + 1)
    double.  Outputs: Rcol = R[0..k, k], cs_k, sn_k, g_k, g_k1, inv_hn, est2."""
    a1, a2, cs, sn, g = _ld(c1), _ld(c2n), _ld(cs), _ld(sn), _ld(g)
    z = np.zeros_like(cs)
    out = _step(dtype, a1, a2, k, cs, sn, z, z, g[:, k], np.zeros(a1.shape[0], LD), fault)
    return {n: (_t(v), _t(REF * e)) for n, (v, e) in out.items() if n not in ("a", "hn")}


def gmres_chain(dtype, c1s, c2ns, beta, state=None, fault=None):
    """m steps of xk_gmres_step from zeroed state with g[0] = beta: c1s[k], c2ns[k] the (S, >= k + 2) inputs of step
    k.  Returns the final state R (S, m + 1, m) (zero where the kernel never writes), cs, sn (S, m), g (S, m + 1).

    A worst-case bound on the whole recurrence grows exponentially (the error of every rotation feeds all later
    ones), so the state is checked in two ways.  (1) Step by step: with `state` = the cs / sn the kernel left behind
    (they are exactly what its later steps read), column k of R, cs[k], sn[k] and g are recomputed from those; the
    bound of an entry then grows linearly with the rotations applied to it (g[k] = c_k beta prod_{j<k} (-t_j):
    2 k + 1 roundings).  (2) R_global: R of the free-running extended-precision recurrence, within the first-order
    perturbation bound of the QR factorisation, |dR|_F <= sqrt(2) cond_2(H) |dH|_F (Sun 1991), under the columnwise
    backward error |dH_k| <= C_ST (k + 1) u |H_k| of k + 1 Givens rotations (Higham, Accuracy and Stability, 19.10)."""
    m = len(c1s)
    S = c1s[0].shape[0]
    R, eR = np.zeros((S, m + 1, m), LD), np.zeros((S, m + 1, m), LD)
    cs, sn, ecs, esn = (np.zeros((S, m), LD) for _ in range(4))
    g, eg = np.zeros((S, m + 1), LD), np.zeros((S, m + 1), LD)
    zero = np.zeros((S, m), LD)
    gin, egin = _ld(beta), np.zeros(S, LD)
    if state is not None:
        cs_in, sn_in = _ld(state["cs"])[:, :m], _ld(state["sn"])[:, :m]
    for k in range(m):
        use_cs, use_sn = (cs, sn) if state is None else (cs_in, sn_in)
        o = _step(dtype, _ld(c1s[k]), _ld(c2ns[k]), k, use_cs, use_sn, zero, zero, gin, egin, fault)
        R[:, :k + 1, k], eR[:, :k + 1, k] = o["Rcol"]
        cs[:, k], ecs[:, k] = o["cs_k"]
        sn[:, k], esn[:, k] = o["sn_k"]
        if state is None:
            g[:, k], g[:, k + 1] = o["g_k"][0], o["g_k1"][0]
            gin = g[:, k + 1]
        else:
            # the rotation the kernel stored is the one it applied to g
            ck, tk = cs_in[:, k], sn_in[:, k]
            g[:, k] = gin if fault == "g_not_rotated" else ck * gin
            eg[:, k] = np.abs(ck) * egin + C_ST * U64 * np.abs(ck * gin)
            gin = -tk * gin
            egin = np.abs(tk) * egin + C_ST * U64 * np.abs(gin)
            g[:, k + 1], eg[:, k + 1] = gin, egin
    out = dict(R=(R, eR), cs=(cs, ecs), sn=(sn, esn), g=(g, eg))
    if state is not None and fault is None:
        free = gmres_chain(dtype, c1s, c2ns, beta)["R"][0]
        H = np.asarray(hessenberg_of(c1s, c2ns), dtype=np.float64)
        sv = np.linalg.svd(H, compute_uv=False)
        E = C_ST * math.sqrt(2.0) * m * U64 * (sv[:, 0] / sv[:, -1]) * np.sqrt((H * H).sum((1, 2)))
        keep = np.triu(np.ones((m + 1, m)))
        out["R_global"] = (free.numpy(), E[:, None, None] * keep[None])
    return {n: (_t(v), _t(REF * e)) for n, (v, e) in out.items()}


def hessenberg_of(c1s, c2ns):
    """the (S, m + 1, m) Hessenberg matrix the step inputs stand for: h[j,k] = c1[j] + c2[j], h[k+1,k] =
    sqrt(c2n[k+1] - sum c2^2), in longdouble"""
    m, S = len(c1s), c1s[0].shape[0]
    H = np.zeros((S, m + 1, m), LD)
    for k in range(m):
        a1, a2 = _ld(c1s[k]), _ld(c2ns[k])
        H[:, :k + 1, k] = a1[:, :k + 1] + a2[:, :k + 1]
        H[:, k + 1, k] = np.sqrt(a2[:, k + 1] - (a2[:, :k + 1] ** 2).sum(1))
    return H


# ================================================================================================ xk_gmres_solve
def gmres_solve(dtype, R, g, kd, fault=None):
    """xk_gmres_solve: back substitution of the kd x kd upper triangle of R (S, >= kd, >= kd) against g (S, >= kd); a
    zero pivot gives y_i = 0.  Bound: the standard one for back substitution in any summation order,
    |dy| <= gamma_kd |R^-1| |R| |y| (gamma_kd = kd u / (1 - kd u), u of double), evaluated on the effective system
    (a zero-pivot row is the equation y_i = 0, which holds exactly), plus one rounding of T for the cast."""
    Rt = torch.triu(torch.nan_to_num(hp(R)[:, :kd, :kd], nan=0.0))
    Rl, gl = _ld(Rt), _ld(hp(g)[:, :kd])
    S = Rl.shape[0]
    y = np.zeros((S, kd), LD)
    with np.errstate(all="ignore"):
        for i in range(kd - 1, -1, -1):
            hi = min(kd, i + 65) if fault == "solve_lane_wrap" else kd
            tot = (Rl[:, i, i + 1:hi] * y[:, i + 1:hi]).sum(1)
            d = Rl[:, i, i]
            if fault == "solve_pivot_nan":
                y[:, i] = (gl[:, i] - tot) / d
            else:
                y[:, i] = np.where(d != 0, (gl[:, i] - tot) / np.where(d != 0, d, 1), 0)
    yt = _t(y)
    if fault is not None:
        return {"y": (yt, torch.zeros_like(yt))}
    dz = torch.diagonal(Rt, dim1=1, dim2=2) == 0
    Re = Rt.clone()
    Re[dz.unsqueeze(-1).expand_as(Re)] = 0                    # zero-pivot rows become e_i
    Re = Re + torch.diag_embed(dz.double())
    eye = torch.eye(kd, dtype=torch.float64).expand(S, kd, kd)
    Rinv = torch.linalg.solve_triangular(Re, eye, upper=True)
    gam = kd * U64 / (1 - kd * U64)
    amp = (Rinv.abs() @ (Re.abs() @ yt.abs().unsqueeze(-1))).squeeze(-1)
    bnd = REF * gam * amp + unit_roundoff(dtype) * yt.abs()
    bnd[dz] = 0
    return {"y": (yt, bnd)}


# ================================================================================================ xk_gmres_finish
def gmres_finish(dtype, Q, c2n, inv_hn, N, k, c1=None, fault=None):
    """xk_gmres_finish: row k + 1 of Q (S, >= k + 2, >= npad) becomes (w - sum_{j<=k} c2n[j] q_j) * inv_hn on
    [0, npad).  Chain in T: k + 1 products and k + 1 additions into the accumulator, one subtraction, one product:
    C = k + 4 roundings at most on any term."""
    npad = npad_of(N, dtype)
    Qh = hp(Q)
    q, w = Qh[:, :k + 1, :npad], Qh[:, k + 1, :npad]
    cc = hp(c1 if fault == "finish_c1" else c2n)[:, :k + 1]
    kk = (k + 1) // 4 * 4 if fault == "finish_drop_tail" else k + 1
    acc = torch.einsum("sj,sjn->sn", cc[:, :kk], q[:, :kk])
    mag = w.abs() + torch.einsum("sj,sjn->sn", hp(c2n)[:, :k + 1].abs(), q.abs())
    sc = hp(inv_hn).reshape(-1, 1)
    val = (w - acc) * (torch.ones_like(sc) if fault == "finish_no_scale" else sc)
    return {"row": (val, REF * (k + 4) * unit_roundoff(dtype) * mag * sc.abs())}


# ================================================================================================ xk_vec_dots
def vd_layout(L):
    """replica of the block sizing of vec_dots (xk_broyden.hip): elements per block, blocks"""
    per = max((L + VD_MAX_BLOCKS - 1) // VD_MAX_BLOCKS, 8192)
    per = (per + 255) // 256 * 256
    return per, max((L + per - 1) // per, 1)


def vec_dots(dtype, pairs, fault=None):
    """xk_vec_dots: out[i] = <a_i, b_i>.  A lane sums ceil(per / 256) products in T (per the block length), the folds
    run in double (VD_TREE levels): |err| <= u (terms per lane + VD_TREE) sum |a||b|."""
    vn = VEC_ELEMS[dtype]
    L = pairs[0][0].numel()
    per, nblk = vd_layout(L)
    klane = (min(per, L) + 255) // 256
    val, bnd = [], []
    for a, b in pairs:
        a, b = hp(a), hp(b)
        mag = (a.abs() * b.abs()).sum()
        hi = L
        if fault == "drop_tail":
            hi = L - L % vn
        if fault == "drop_block":
            hi = (nblk - 1) * per
        val.append((a[:hi] * b[:hi]).sum())
        bnd.append(REF * unit_roundoff(dtype) * (klane + VD_TREE) * mag)
    return {"out": (torch.stack(val), torch.stack(bnd))}


# ================================================================================================ xk_broyden_axpy
def broyden_axpy(dtype, L, u0, g0, u1, g1, V, coef, scale, k, gamma, fault=None):
    """xk_broyden_axpy: out = g0 u0 + g1 u1 + gamma sum_{n<k} (coef[n] scale[n]) V[n] on [0, L).  Chain in T: the
    product coef * scale (1), k products and k additions into the accumulator, the product with gamma (1), one
    multiply-add per u term (2): C = k + 4 roundings at most on any term."""
    g0, g1, gamma = cast(g0, dtype), cast(g1, dtype), cast(gamma, dtype)
    val, mag = torch.zeros(L, dtype=torch.float64), torch.zeros(L, dtype=torch.float64)
    if k > 0:
        cf = hp(coef)[:k]
        if scale is not None and fault != "scale_ignored":
            cf = (cf * hp(scale)[:k]).to(dtype).double()       # the kernel rounds c0 *= scale[n] to T
        Vh = hp(V)[:k, :L]
        kk = k // 4 * 4 if fault == "unroll_tail" else k
        val = gamma * (cf[:kk] @ Vh[:kk])
        mag = abs(gamma) * (cf.abs() @ Vh.abs())
    for u, gu in ((u0, g0), (u1, g1)):
        if u is not None:
            val = val + (gamma * gu if fault == "gamma_on_u" else gu) * hp(u)[:L]
            mag = mag + abs(gu) * hp(u)[:L].abs()
    return {"out": (val, REF * (k + 4) * unit_roundoff(dtype) * mag)}


# ================================================================================================ xk_grad.hip
def _grad_terms(C):
    """C products and C additions spread over ceil(C / 8) passes, each later pass (and accumulate) one more
    read-modify-write addition"""
    return C + (C + 7) // 8 + 1


def _last_pass(C, fault):
    return (C - 1) // 8 * 8 if (fault == "second_pass_overwrites" and C > 8) else 0


def _with_out0(dtype, C, val, mag, out0, fault, overwritten):
    """(+)= semantics: where no product term exists the kernel adds an exact zero, so out0 comes back unchanged"""
    if out0 is not None:
        o = hp(out0)
        if fault != "accumulate_ignored" and not overwritten:
            val = val + o
        mag = mag + torch.where(mag > 0, o.abs(), torch.zeros_like(o))
    return val, REF * unit_roundoff(dtype) * _grad_terms(C) * mag


def dense_outer(dtype, U, W, out0=None, fault=None):
    """xk_dense_outer: G[b,i,j] (+)= sum_c U[b,c,i] W[b,c,j]; U (B, C, M), W (B, C, N) the logical panels"""
    Uh, Wh = hp(U), hp(W)
    C = Uh.shape[1]
    c0 = _last_pass(C, fault)
    val = torch.einsum("bci,bcj->bij", Uh[:, c0:], Wh[:, c0:])
    mag = torch.einsum("bci,bcj->bij", Uh.abs(), Wh.abs())
    val, bnd = _with_out0(dtype, C, val, mag, out0, fault, c0 > 0)
    return {"G": (val, bnd)}


def banded_grad(dtype, U, W, hb, out0=None, fault=None):
    """xk_banded_grad: G[b,d,i] (+)= sum_c U[b,c,i] W[b,c,i+d-hb]; entries whose column i + d - hb falls outside
    [0, N) get no term (exactly 0, or exactly out0 when accumulating)"""
    Uh, Wh = hp(U), hp(W)
    B, C, N = Uh.shape
    nd = 2 * hb + 1
    c0 = _last_pass(C, fault)
    val = torch.zeros((B, nd, N), dtype=torch.float64)
    mag = torch.zeros((B, nd, N), dtype=torch.float64)
    for d in range(nd):
        for shift, dst, lo_c in ((1 if fault == "halo_shift" else 0, val, c0), (0, mag, 0)):
            off = d - hb + shift
            lo, hi = max(0, -off), min(N, N - off)
            if lo < hi:
                u, w = Uh[:, lo_c:, lo:hi], Wh[:, lo_c:, lo + off:hi + off]
                dst[:, d, lo:hi] = (u * w).sum(1) if dst is val else (u.abs() * w.abs()).sum(1)
    val, bnd = _with_out0(dtype, C, val, mag, out0, fault, c0 > 0)
    return {"G": (val, bnd)}


# ================================================================================================ configurations
# The GPU test (tests/test_gpu_solver_kernels.py) and the CPU fault test (tests/test_solver_ref.py) both iterate
# these lists and build their inputs with the *_case functions, so the fault test sees every GPU configuration.
def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


def _randn(g, *shape):
    return torch.randn(*shape, dtype=torch.float64, generator=g)


def _rand(g, *shape):
    return torch.rand(*shape, dtype=torch.float64, generator=g)


def _signs(g, *shape):
    return torch.where(_rand(g, *shape) < 0.5, -1.0, 1.0).double()


def _nan(shape, dtype=torch.float64):
    return torch.full(shape, math.nan, dtype=dtype)


# ---- xk_gmres_step
STEP_CAP = 80
STEP_KS = (0, 1, 2, 31, 63, 64, STEP_CAP - 1)
STEP_SS = (1, 63, 64, 65, 257)
STEP_EDGES = (("n2_neg", 0), ("n2_neg", 3), ("a0_hn0", 0), ("a0_hn0", 3), ("a0_hnpos", 0), ("a0_hnpos", 3),
              ("a_neg", 0))
STEP_CONFIGS = [(k, S, None) for k in STEP_KS for S in STEP_SS] + [(k, 5, e) for e, k in STEP_EDGES]
STEP_EXTRA_SYSTEMS = 2          # the state is over-allocated by this many systems, which must stay untouched


def _step_inputs(g, dtype, S, k, sc1, sc2, hn=None):
    """generic inputs of step k: c1 O(1); c2 rounding-sized next to w1 (sum c2^2 <= 1e-4 <= 1e-3 c2n[k+1], the
    promise of the comment in the kernel) yet far above u, so that a dropped subtraction shows; c2n[k+1] = hn^2 +
    sum c2^2 with hn in [0.5, 1.5)"""
    c1 = _nan((S, sc1), dtype)
    c2n = _nan((S, sc2), dtype)
    c1[:, :k + 1] = _randn(g, S, k + 1).to(dtype)
    c2n[:, :k + 1] = ((2 * _rand(g, S, k + 1) - 1) * 0.01 / math.sqrt(k + 1)).to(dtype)
    if hn is None:
        hn = 0.5 + _rand(g, S)
    c2n[:, k + 1] = (hn ** 2 + (c2n[:, :k + 1].double() ** 2).sum(1)).to(dtype)
    return c1, c2n


def step_case(dtype, k, S, edge):
    """host inputs of one xk_gmres_step launch: dict(c1, c2n in T with NaN beyond what step k reads; R, cs, sn, g
    double of S + STEP_EXTRA_SYSTEMS systems: NaN except the earlier rotations cs / sn [:k] and g[k])"""
    g = _gen(1, k, S, DTYPES.index(dtype), len(edge or ""))
    cap, Sa = STEP_CAP, S + STEP_EXTRA_SYSTEMS
    c1, c2n = _step_inputs(g, dtype, S, k, k + 2 + 3, k + 2 + 5)
    R, cs, sn, gg = _nan((Sa, cap + 1, cap)), _nan((Sa, cap)), _nan((Sa, cap)), _nan((Sa, cap + 1))
    th = 2 * math.pi * _rand(g, S, k)
    cs[:S, :k], sn[:S, :k] = torch.cos(th), torch.sin(th)
    gg[:S, k] = (0.5 + _rand(g, S)) * _signs(g, S)
    if edge == "n2_neg":                     # c2n[k+1] < sum c2^2: hn = 0, inv_hn = 0, sn[k] = 0
        c2n[:, :k + 1] = 0.3
        c2n[:, k + 1] = 0.5 * (c2n[:, :k + 1].double() ** 2).sum(1).to(dtype)
    elif edge in ("a0_hn0", "a0_hnpos"):     # a zero column: a = 0 exactly through every replayed rotation
        c1[:, :k + 1] = 0
        c2n[:, :k + 1] = 0
        c2n[:, k + 1] = 0 if edge == "a0_hn0" else (0.5 + _rand(g, S)).to(dtype)
    elif edge == "a_neg":
        c1[:, 0] = (-(0.5 + _rand(g, S))).to(dtype)
    return dict(c1=c1, c2n=c2n, R=R, cs=cs, sn=sn, g=gg, k=k, S=S, cap=cap)


def step_ref(dtype, case, fault=None):
    S, k = case["S"], case["k"]
    return gmres_step(dtype, case["c1"], case["c2n"], k, case["cs"][:S, :k], case["sn"][:S, :k],
                      case["g"][:S, :k + 1].nan_to_num(0.0), fault)


# ---- chained xk_gmres_step
CHAIN_MS = (1, 5, 31, 64, 65, 200)
CHAIN_S = 3


def chain_case(dtype, m):
    """m columns of a random upper Hessenberg matrix (diagonal shifted by 2, sub-diagonal in [0.5, 1.5)) split at
    random into c1 + c2 with c2 small; beta in [0.5, 1.5)"""
    g = _gen(2, m, DTYPES.index(dtype))
    S = CHAIN_S
    H = torch.triu(_randn(g, S, m, m) * 0.3) + 2 * torch.eye(m, dtype=torch.float64)
    sub = 0.5 + _rand(g, S, m)
    c1s, c2ns = [], []
    for k in range(m):
        c1, c2n = _step_inputs(g, dtype, S, k, m + 3, m + 4, hn=sub[:, k])
        c1[:, :k + 1] = (H[:, :k + 1, k] - c2n[:, :k + 1].double()).to(dtype)
        c1s.append(c1)
        c2ns.append(c2n)
    beta = 0.5 + _rand(g, S)
    return dict(c1s=c1s, c2ns=c2ns, beta=beta, m=m, S=S, cap=m + 1)


def chain_ref(dtype, case, state=None, fault=None):
    return gmres_chain(dtype, case["c1s"], case["c2ns"], case["beta"], state, fault)


# ---- xk_gmres_solve
SOLVE_KDS = (1, 2, 63, 64, 65, 129, 1000)
SOLVE_SS = (1, 3, 70)
# (kd = 1000 with S = 70 is left out: its |R^-1| on the host alone took a quarter of the GPU test's run time)
SOLVE_CONFIGS = [(kd, S, None) for kd in SOLVE_KDS for S in SOLVE_SS if (kd, S) != (1000, 70)] + \
                [(kd, 3, z) for kd in (1, 65, 129) for z in ("last", "first", "mid")]


def solve_case(dtype, kd, S, zero):
    """R (S, cap + 1, cap) double, cap = kd + 3: NaN except the kd x kd upper triangle (diagonal in +-[1, 2),
    off-diagonal N(0, 1) / (2 sqrt kd)); g NaN beyond kd.  zero: a zero pivot in the last / first / middle row"""
    g = _gen(3, kd, S, DTYPES.index(dtype), len(zero or ""))
    cap = kd + 3
    R = _nan((S, cap + 1, cap))
    tri = torch.triu(_randn(g, S, kd, kd) * (0.5 / math.sqrt(kd)), 1) + torch.diag_embed((1 + _rand(g, S, kd)) * _signs(g, S, kd))
    keep = torch.triu(torch.ones(kd, kd, dtype=torch.bool))
    R[:, :kd, :kd] = torch.where(keep, tri, _nan((kd, kd)))
    if zero is not None:
        i = {"last": kd - 1, "first": 0, "mid": kd // 2}[zero]
        R[:, i, i] = 0
    gg = _nan((S, cap + 1))
    gg[:, :kd] = _randn(g, S, kd)
    return dict(R=R, g=gg, kd=kd, S=S, cap=cap, sy=kd + 5)


def solve_ref(dtype, case, fault=None):
    return gmres_solve(dtype, case["R"], case["g"], case["kd"], fault)


# ---- xk_gmres_finish
FINISH_KS = (0, 1, 2, 3, 4, 5, 7, 8, 33)


def finish_ns(dtype):
    vn = VEC_ELEMS[dtype]
    return (1, vn - 1, vn, vn + 1, 255 * vn, 256 * vn, 256 * vn + 1, 100003)


def finish_configs(dtype):
    """(N, k, extra pitch in vectors, S): every N with every k; the pitch and S alternate so that each value meets
    each N and each k"""
    combos = ((0, 1), (3, 3), (0, 3), (3, 1))
    return [(N, k, *combos[(3 * i + j) % 4]) for i, N in enumerate(finish_ns(dtype)) for j, k in enumerate(FINISH_KS)]


def finish_case(dtype, N, k, wide, S):
    """Q: S systems of k + 3 rows at pitch ldq inside one NaN-poisoned flat buffer, system stride sQ > rows * ldq.
    Rows 0 .. k + 1 random on [0, N), zero on [N, npad); row k + 2 and columns [npad, ldq) stay NaN.  With S = 3
    system 1 has inv_hn = 0 (breakdown)."""
    g = _gen(4, N, k, wide, S, DTYPES.index(dtype))
    vn = VEC_ELEMS[dtype]
    npad = npad_of(N, dtype)
    ldq = npad + wide * vn
    rows = k + 3
    sQ = rows * ldq + 4 * vn
    flat = _nan((S * sQ,), dtype)
    Q = flat.as_strided((S, rows, ldq), (sQ, ldq, 1))
    Q[:, :k + 2, :N] = _randn(g, S, k + 2, N).to(dtype)
    Q[:, :k + 2, N:npad] = 0
    c2n, c1 = _nan((S, k + 2 + 3), dtype), _nan((S, k + 2 + 3), dtype)
    c2n[:, :k + 2] = (0.3 * _randn(g, S, k + 2)).to(dtype)
    c1[:, :k + 2] = _randn(g, S, k + 2).to(dtype)
    inv = ((0.5 + 1.5 * _rand(g, S)) * _signs(g, S)).to(dtype)
    if S == 3:
        inv[1] = 0
    return dict(flat=flat, Q=Q, c2n=c2n, c1=c1, inv_hn=inv, N=N, k=k, S=S, ldq=ldq, sQ=sQ, npad=npad, rows=rows)


def finish_ref(dtype, case, fault=None):
    return gmres_finish(dtype, case["Q"], case["c2n"], case["inv_hn"], case["N"], case["k"], c1=case["c1"], fault=fault)


# ---- xk_vec_dots
VD_BIG = 8192 * 1024
HUGE = 1000.0                   # the planted last entry: its product 1e6 is many bounds whatever L is tested


def vd_lengths(dtype):
    vn = VEC_ELEMS[dtype]
    return (0, 1, vn - 1, vn, 8191, 8192, 8193, 100003, VD_BIG, VD_BIG + 256 * vn, VD_BIG + 1)


def vd_configs(dtype):
    """(L, pairs, kind).  plain: pairs (X0, X1), (X1, X2), (X2, X0), (X0, X0): the last has `a is b`; equal: X1 holds
    a copy of X0; offset: pair 2 reads X2 from element 1 on (not 16-byte aligned: every pair takes the scalar
    kernel).  The three lengths above 8192 * 1024 run 4 pairs and the offset form only."""
    vn = VEC_ELEMS[dtype]
    cfg = []
    for L in vd_lengths(dtype):
        cfg += [(L, np_, "plain") for np_ in ((1, 2, 3, 4) if L < VD_BIG else (4,))]
    cfg += [(100003, 2, "equal"), (8192, 2, "equal")]
    cfg += [(L, 3, "offset") for L in (vn, 8192, 100000, VD_BIG, VD_BIG + 256 * vn)]
    return cfg


@functools.lru_cache(maxsize=2)
def _vd_bufs(dtype, L, equal):
    g = _gen(5, L, DTYPES.index(dtype), equal)
    bufs = [_randn(g, L + 1).to(dtype) for _ in range(3)]
    if equal:
        bufs[1] = bufs[0].clone()
    return bufs


def vd_case(dtype, L, np_, kind):
    """three buffers of L + 1 elements and, per pair, ((buffer, offset), (buffer, offset)).  Every operand ends in
    +-HUGE: the last block, the last lane and the last slot of its vector (or the ragged tail) carry the result."""
    bufs = _vd_bufs(dtype, L, kind == "equal")
    spec = [((0, 0), (1, 0)), ((1, 0), (2, 0)), ((2, 0), (0, 0)), ((0, 0), (0, 0))][:np_]
    if kind == "offset":
        spec = [((0, 0), (1, 0)), ((1, 0), (1, 0)), ((2, 1), (0, 0))]
    if L > 0:
        for b in bufs:
            b[L - 1:] = HUGE
        if kind != "equal":
            bufs[1][L - 1:] = -HUGE
    return dict(bufs=bufs, spec=spec, L=L)


def vd_pairs(case, bufs=None):
    bufs, L = bufs or case["bufs"], case["L"]
    return [(bufs[ia][oa:oa + L], bufs[ib][ob:ob + L]) for (ia, oa), (ib, ob) in case["spec"]]


def vd_ref(dtype, case, fault=None):
    return vec_dots(dtype, vd_pairs(case), fault)


# ---- xk_broyden_axpy
AX_KS = (0, 1, 2, 3, 4, 5, 7, 8, 9)
AX_G0 = (0.7, 0.0, -1.3)
AX_G1 = (-1.3, 1.0, 0.0)
AX_GAMMA = (1.0, -0.5, 0.0, 2.5)


def ax_lengths(dtype):
    vn = VEC_ELEMS[dtype]
    return (1, vn - 1, vn, 4096, 100003)


def ax_configs(dtype):
    """(k, mask, L, extra pitch, mode, variant).  mask bit 0 / 1 / 2: u0 / u1 / scale present.  Every k with every
    mask; L, the pitch and the scalars (variant indexes AX_G0 / AX_G1 / AX_GAMMA) rotate through their lists.  Modes:
    plain; alias_u0 (out is u0); row_k (out is row k of V, the driver's in-place update); offset (out starts one
    element into its buffer: scalar kernel although L % VN == 0)."""
    Ls = ax_lengths(dtype)
    cfg, n = [], 0
    for k in AX_KS:
        for mask in range(8):
            cfg.append((k, mask, Ls[n % len(Ls)], (0, 8)[(n // len(Ls)) % 2], "plain", n))
            n += 1
    for k in AX_KS:
        cfg.append((k, 7, 4096, 8, "row_k", n))
        cfg.append((k, 5, 100003, 0, "row_k", n + 1))
        cfg.append((k, 7, 4096, 0, "alias_u0", n + 2))
        cfg.append((k, 3 + 4 * (k % 2), 4096, 8, "offset", n + 3))
        n += 4
    return cfg


def ax_case(dtype, k, mask, L, extra, mode, variant):
    """V: k + 2 rows at pitch ldv >= L (a multiple of the vector width), columns [L, ldv) and rows > k NaN"""
    g = _gen(6, k, mask, L, extra, variant, DTYPES.index(dtype))
    vn = VEC_ELEMS[dtype]
    ldv = (L + vn - 1) // vn * vn + extra
    V = _nan((k + 2, ldv), dtype)
    V[:k, :L] = _randn(g, k, L).to(dtype)
    u0 = _randn(g, L).to(dtype) if mask & 1 else None
    u1 = _randn(g, L).to(dtype) if mask & 2 else None
    scale = (0.5 + _rand(g, k + 2)).to(dtype) if mask & 4 else None
    coef = _randn(g, k + 2).to(dtype)
    return dict(V=V, u0=u0, u1=u1, scale=scale, coef=coef, k=k, L=L, ldv=ldv, mode=mode,
                g0=AX_G0[variant % 3], g1=AX_G1[(variant // 3) % 3], gamma=AX_GAMMA[variant % 4])


def ax_ref(dtype, c, fault=None):
    return broyden_axpy(dtype, c["L"], c["u0"], c["g0"], c["u1"], c["g1"], c["V"], c["coef"], c["scale"], c["k"],
                        c["gamma"], fault)


# ---- xk_dense_outer / xk_banded_grad
OUTER_CS = (1, 7, 8, 9, 16, 17)
BANDED_HBS = (0, 1, 5, 63)
BANDED_CS = (0, 1, 8, 9, 17)


def outer_configs(dtype):
    vn = VEC_ELEMS[dtype]
    mns = ((1, 1), (63, vn - 1), (64, 256 * vn), (65, 256 * vn + 1), (130, 1026))
    return [(C, M, N, B, acc) for C in OUTER_CS for (M, N) in mns for B in (1, 3) for acc in (False, True)]


def banded_configs(dtype):
    vn = VEC_ELEMS[dtype]
    cfg = []
    for hb in BANDED_HBS:
        for N in sorted({1, hb, hb + 1, 256 * vn, 256 * vn + 1, 1537}):        # (hb = 0: N = 0, an empty launch)
            cfg += [(hb, N, C, acc) for C in BANDED_CS for acc in (False, True)]
    return cfg


def _panel(g, dtype, B, C, n, extra):
    """(B, C, n) panel inside a NaN-poisoned (B, C + 1, n + extra) allocation"""
    full = _nan((B, C + 1, n + extra), dtype)
    full[:, :C, :n] = _randn(g, B, C, n).to(dtype)
    return full


def outer_case(dtype, C, M, N, B, acc):
    """U (B, C, M), W (B, C, N) with pitches M + 3 / N + 5 and a spare row; out0: the (B, M, N) view at pitch
    ldg = N rounded up to whole vectors + 2 vectors, batch stride M * ldg + 4 vectors, of a flat buffer that is NaN
    outside the view and, inside it, O(1) random when accumulating / NaN otherwise"""
    g = _gen(7, C, M, N, B, acc, DTYPES.index(dtype))
    vn = VEC_ELEMS[dtype]
    ldg = npad_of(N, dtype) + 2 * vn
    sG = M * ldg + 4 * vn
    flat = _nan((B * sG + 2 * vn,), dtype)
    G = flat[2 * vn:].as_strided((B, M, N), (sG, ldg, 1))
    if acc:
        G.copy_(_randn(g, B, M, N).to(dtype))
    return dict(U=_panel(g, dtype, B, C, M, 3), W=_panel(g, dtype, B, C, N, 5), flat=flat, G=G, C=C, M=M, N=N, B=B,
                acc=acc, ldg=ldg, sG=sG, off=2 * vn)


def outer_ref(dtype, c, fault=None):
    C, M, N = c["C"], c["M"], c["N"]
    return dense_outer(dtype, c["U"][:, :C, :M], c["W"][:, :C, :N], c["G"].clone() if c["acc"] else None, fault)


BANDED_B = 2


def banded_case(dtype, hb, N, C, acc):
    """U, W (B, C, N) with pitch N + 3 and a spare row; out0: the contiguous (B, nd, N) array the wrapper demands,
    between two NaN guard zones of one flat buffer"""
    g = _gen(8, hb, N, C, acc, DTYPES.index(dtype))
    vn = VEC_ELEMS[dtype]
    B, nd = BANDED_B, 2 * hb + 1
    flat = _nan((B * nd * N + 4 * vn,), dtype)
    G = flat[2 * vn:2 * vn + B * nd * N].view(B, nd, N)
    if acc:
        G.copy_(_randn(g, B, nd, N).to(dtype))
    return dict(U=_panel(g, dtype, B, C, N, 3), W=_panel(g, dtype, B, C, N, 3), flat=flat, G=G, C=C, N=N, B=B, hb=hb,
                acc=acc, off=2 * vn)


def banded_ref(dtype, c, fault=None):
    C, N = c["C"], c["N"]
    return banded_grad(dtype, c["U"][:, :C, :N], c["W"][:, :C, :N], c["hb"], c["G"].clone() if c["acc"] else None,
                       fault)


# ================================================================================================ where a fault shows
# VISIBLE[fault](config) -> bool: can this fault change an output at this configuration at all?  The CPU test
# demands a rejection wherever this is true, and at least one such configuration per fault.
VISIBLE = {
    # xk_gmres_step: (k, S, edge); xk_gmres_step chained: (m,)
    ("step", "rot_sign"): lambda k, S, e: k >= 1 and e not in ("a0_hn0", "a0_hnpos"),
    ("step", "rot_skip_last"): lambda k, S, e: k >= 1 and e not in ("a0_hn0", "a0_hnpos"),
    ("step", "hn_no_sub"): lambda k, S, e: e not in ("a0_hn0", "a0_hnpos"),
    ("step", "abs_a"): lambda k, S, e: e == "a_neg" or (e is None and S >= 63),     # some a < 0 among >= 63 systems
    ("step", "g_not_rotated"): lambda k, S, e: e != "n2_neg" and e != "a0_hn0",     # |c| = 1 there: g[k] keeps |g|
    ("step", "est_not_squared"): lambda k, S, e: e not in ("n2_neg", "a0_hn0"),     # g[k+1] = 0 there
    ("chain", "rot_sign"): lambda m: m >= 2,
    ("chain", "rot_skip_last"): lambda m: m >= 2,
    ("chain", "hn_no_sub"): lambda m: True,
    ("chain", "g_not_rotated"): lambda m: True,
    # xk_gmres_solve: (kd, S, zero)
    ("solve", "solve_lane_wrap"): lambda kd, S, z: kd >= 66,
    ("solve", "solve_pivot_nan"): lambda kd, S, z: z is not None,
    # xk_gmres_finish: (N, k, wide, S)
    ("finish", "finish_drop_tail"): lambda N, k, w, S: (k + 1) % 4 != 0,
    ("finish", "finish_no_scale"): lambda N, k, w, S: True,
    ("finish", "finish_c1"): lambda N, k, w, S: True,
    # xk_vec_dots: (L, pairs, kind) + the vector width
    ("vec_dots", "drop_tail"): lambda L, np_, kind, vn: L % vn != 0,
    ("vec_dots", "drop_block"): lambda L, np_, kind, vn: L > 0,
    # xk_broyden_axpy: the case dict
    ("axpy", "scale_ignored"): lambda c: c["k"] > 0 and c["scale"] is not None and c["gamma"] != 0,
    ("axpy", "gamma_on_u"): lambda c: c["gamma"] != 1 and ((c["u0"] is not None and c["g0"] != 0) or
                                                           (c["u1"] is not None and c["g1"] != 0)),
    ("axpy", "unroll_tail"): lambda c: c["k"] % 4 != 0 and c["gamma"] != 0,
    # xk_dense_outer: (C, M, N, B, acc); xk_banded_grad: (hb, N, C, acc)
    ("outer", "second_pass_overwrites"): lambda C, M, N, B, acc: C > 8,
    ("outer", "accumulate_ignored"): lambda C, M, N, B, acc: acc,
    ("banded", "second_pass_overwrites"): lambda hb, N, C, acc: C > 8 and N > 0,
    ("banded", "halo_shift"): lambda hb, N, C, acc: C > 0 and N > 0,
    ("banded", "accumulate_ignored"): lambda hb, N, C, acc: acc and C > 0 and N > 0,
}


# ================================================================================================ CPU Arnoldi
def arnoldi(A, b, m, order="mgs2"):
    """float64 Arnoldi of A (N, N) from b: Q (m + 1, N) rows, H (m + 1, m).  order: "mgs2" (modified Gram-Schmidt,
    twice) or "cgs2" (classical, twice)"""
    N = A.shape[0]
    Q = torch.zeros((m + 1, N), dtype=torch.float64)
    H = torch.zeros((m + 1, m), dtype=torch.float64)
    Q[0] = b / b.norm()
    for k in range(m):
        w = A @ Q[k]
        for _ in range(2):
            if order == "cgs2":
                c = Q[:k + 1] @ w
                w = w - c @ Q[:k + 1]
                H[:k + 1, k] += c
            else:
                for j in range(k + 1):
                    c = torch.dot(Q[j], w)
                    w = w - c * Q[j]
                    H[j, k] += c
        H[k + 1, k] = w.norm()
        Q[k + 1] = w / H[k + 1, k]
    return Q, H


def lstsq_y(H, beta):
    """argmin |beta e1 - H y| (numpy.linalg.lstsq)"""
    H = np.asarray(H, dtype=np.float64)
    rhs = np.zeros(H.shape[0])
    rhs[0] = beta
    return np.linalg.lstsq(H, rhs, rcond=None)[0]
