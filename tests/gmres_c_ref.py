"""Complex128 (and extended precision) restatement of the five kernels of xk_gmres_c.hip — xk_gmres_gram_c*,
xk_lincomb_c*, xk_gmres_step_c*, xk_gmres_finish_c*, xk_gmres_solve_c* — with per-entry error bounds, in the manner of
tests/solver_ref.py.

Every function computes, from the very inputs the kernel is given, what the kernel must write, and returns
{name: (value, bound)}: `value` complex128 (float64 for the real outputs), `bound` a per-entry absolute bound on
|kernel - value| (the modulus of the complex difference) of the form SQ2 * C * u * (sum of the magnitudes of the terms).
u is the unit roundoff of the arithmetic that produces that output (the GMRES state is double whatever the vector type),
C the length of the longest rounding chain on any real term, derived next to each function.  A real term of a complex
product a b is one of ar br, ai bi, ar bi, ai br: every component of the product is 2 real products and 1 addition, and
the magnitude used for both components is (|ar| + |ai|) (|br| + |bi|), which bounds either component's term sum; the
modulus of a complex error is at most sqrt(2) = SQ2 times its larger component.  Where the magnitudes vanish the bound is
0: such entries are checked exactly (the imaginary part of the norm entry of the Gram kernel always is).

`check()` compares kernel outputs with that, raises AssertionError naming the first entry out of bounds and records the
largest |kernel - value| / bound per (kernel, dtype) in WORST.  The `fault=` argument produces plausible kernel bugs;
tests/test_gmres_c_ref.py feeds them to `check()` at every configuration of the GPU test (the *_CONFIGS lists and *_case
builders are shared by both) and asserts that each is rejected wherever `visible()` says it can be seen.

The per-system recurrence of xk_gmres_step_c runs in numpy.longdouble / clongdouble (u = 2^-64 where the platform has an
extended type); REF = 2 keeps the bounds valid where it is plain double and covers the complex128 sums of the others.
"""
import math
import numpy as np
import torch
from tests.krylov_ref import unit_roundoff, hp

U64 = 2.0 ** -53
LD, CLD = np.longdouble, np.clongdouble
REF = 2.0
SQ2 = math.sqrt(2.0)
DTYPES = [torch.complex128, torch.complex64]
DNAME = {torch.complex128: "c128", torch.complex64: "c64"}
CV = {torch.complex128: 1, torch.complex64: 2}            # complex elements per 16 B vector
RDT = {torch.complex128: torch.float64, torch.complex64: torch.float32}
GRAM_U = 4                                                # 16 B vectors of w per lane (xk_gmres_c.hip)

FAULTS_GRAM = ("noconj", "conj_w", "drop_tail", "nrm_im")
FAULTS_LINCOMB = ("drop_tail_rows", "coef_conj")
FAULTS_STEP = ("sn_noconj", "cs_no_abs")
FAULTS_FINISH = ("drop_tail_rows", "coef_conj")
FAULTS_SOLVE = ("pivot_nan", "lane_wrap")

WORST = {}


KEEP64 = ("Rcol", "cs_k", "sn_k", "g_k", "g_k1", "nrm_im")      # double outputs (the state); the others are in T


def values(ref, dtype):
    """the reference values alone, rounded to the kernel dtype where the kernel writes T"""
    out = {}
    for name, (val, _) in ref.items():
        if name in KEEP64:
            out[name] = val
        else:
            out[name] = val.to(dtype if val.is_complex() else RDT[dtype])
    return out


def npad_of(N, dtype):
    return (N + CV[dtype] - 1) // CV[dtype] * CV[dtype]


def gram_tiles(N, dtype):
    tile = 256 * GRAM_U * CV[dtype]
    return (N + tile - 1) // tile


def mag1(z):
    """|re| + |im|: bounds the magnitude of either component's terms in a product"""
    return z.real.abs() + z.imag.abs()


def check(got, ref, kernel, dtype, what=""):
    worst = 0.0
    for name, (val, bnd) in ref.items():
        assert name in got, "%s: no kernel output %r" % (what, name)
        assert bool(torch.isfinite(torch.view_as_real(val) if val.is_complex() else val).all()) and \
            bool(torch.isfinite(bnd).all()), "%s: reference %s is not finite" % (what, name)
        g = hp(got[name]).reshape(val.shape)
        err = (g - val).abs()
        err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
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


# ================================================================================================ xk_gmres_gram_c
def gram_chain(N, dtype):
    """Longest rounding chain on a real term of one component of c[i]: its product (1); the lane's sequential sum of
    2 * GRAM_U * CV terms (<= 16 additions); wave_sum (6 levels) — all in T; then in double (u64 <= u): the 4-wave
    combine (2), the fold kernel's per-lane loop over ceil(nblk / 64) tile partials and its wave_sum (6); the cast of
    the result to T (1)."""
    return 1 + 2 * GRAM_U * CV[dtype] + 6 + 2 + (gram_tiles(N, dtype) + 63) // 64 + 6 + 1


def gram(dtype, Q, w, N, kq, fault=None):
    """c[s, i] = sum_n conj(Q[s, i, n]) w[s, n] (i < kq); nrm[s] = sum |w|^2 with nrm_im[s] = 0 exactly."""
    npad = npad_of(N, dtype)
    Qh, wh = hp(Q)[:, :kq, :npad], hp(w)[:, :npad]
    S = wh.shape[0]
    Qe, we = Qh, wh
    if fault == "drop_tail":
        keep = npad - CV[dtype]
        Qe, we = Qh[:, :, :keep], wh[:, :keep]
    if fault == "noconj":
        c = torch.einsum("sin,sn->si", Qe, we)
    elif fault == "conj_w":
        c = torch.einsum("sin,sn->si", Qe, we.conj())
    else:
        c = torch.einsum("sin,sn->si", Qe.conj(), we)
    nrm = (we.real ** 2 + we.imag ** 2).sum(-1)
    u = unit_roundoff(dtype)
    C = gram_chain(N, dtype)
    bc = REF * SQ2 * C * u * torch.einsum("sin,sn->si", mag1(Qh), mag1(wh))
    bn = REF * C * u * (wh.real ** 2 + wh.imag ** 2).sum(-1)
    nim = torch.zeros(S, dtype=torch.float64)
    if fault == "nrm_im":
        nim = 2.0 ** -60 * nrm                        # an imaginary part that was summed, not zeroed
    return {"c": (c, bc), "nrm": (nrm, bn), "nrm_im": (nim, torch.zeros(S, dtype=torch.float64))}


# ================================================================================================ xk_lincomb_c
def lincomb(dtype, V, C, out0, N, k, P, alpha, beta, fault=None):
    """out[s, c, :npad] = beta out0 + alpha sum_{a<k} C[s, c, a] V[s, a, :].  Chain in T on a term of the sum: its
    product (1), the sequential accumulation of the 2 k real terms of a component (2 k), alpha * acc (1), the final
    addition (1): 2 k + 3; on beta * out0: product and addition (2)."""
    npad = npad_of(N, dtype)
    Vh, Ch, oh = hp(V)[:, :k, :npad], hp(C)[:, :P, :k], hp(out0)[:, :P, :npad]
    kk = k // 4 * 4 if fault == "drop_tail_rows" else k
    Ce = Ch.conj() if fault == "coef_conj" else Ch
    acc = torch.einsum("sca,san->scn", Ce[:, :, :kk], Vh[:, :kk])
    val = alpha * acc + (beta * oh if beta != 0 else 0)
    u = unit_roundoff(dtype)
    mag = abs(alpha) * torch.einsum("sca,san->scn", mag1(Ch), mag1(Vh)) + (abs(beta) * oh.abs() if beta != 0 else 0)
    return {"out": (val, REF * SQ2 * (2 * k + 3) * u * mag)}


# ================================================================================================ xk_gmres_finish_c
def finish(dtype, Q, c2n, inv_hn, N, k, fault=None):
    """row k + 1 of Q <- (w - sum_{j<=k} c2n[j] q_j) * inv_hn on [0, npad).  Chain in T: product (1), accumulation of
    the 2 (k + 1) real terms of a component, the subtraction (1), the scaling (1): 2 k + 5."""
    npad = npad_of(N, dtype)
    Qh = hp(Q)
    q, w = Qh[:, :k + 1, :npad], Qh[:, k + 1, :npad]
    cc = hp(c2n)[:, :k + 1]
    kk = (k + 1) // 4 * 4 if fault == "drop_tail_rows" else k + 1
    ce = cc.conj() if fault == "coef_conj" else cc
    acc = torch.einsum("sj,sjn->sn", ce[:, :kk], q[:, :kk])
    sc = hp(inv_hn).reshape(-1, 1)
    mag = w.abs() + torch.einsum("sj,sjn->sn", mag1(cc), mag1(q))
    return {"row": ((w - acc) * sc, REF * SQ2 * (2 * k + 5) * unit_roundoff(dtype) * mag * sc.abs())}


# ================================================================================================ xk_gmres_step_c
# Longest chain of xk_gmres_step_c in double: |a| = sqrt(pr^2 + pi^2) is two products, an addition and a root (4),
# den = sqrt(|a|^2 + b^2) four more (8), a / |a| one division (9), sn = (a/|a|) b / den a product and a division (11);
# R[k,k] = (a/|a|) den is 10.  A replayed entry c prev + t nxt is a real-complex product (1), a complex product (2) and
# an addition (1).  C_STC = 12.
C_STC = 12.0


def _ldc(x):
    return np.asarray(hp(x).numpy(), dtype=CLD)


def _t(x):
    x = np.asarray(x)
    if np.iscomplexobj(x):
        return torch.from_numpy(np.ascontiguousarray(x.astype(np.complex128)))
    return torch.from_numpy(np.ascontiguousarray(x.astype(np.float64)))


def step(dtype, c1, c2n, k, cs, sn, g, fault=None):
    """xk_gmres_step_c on exact state: c1 (S, >= k+1), c2n (S, >= k+2) complex in T (c2n[k+1] = |w1|^2 + 0i); cs (S, >= k)
    real double, sn (S, >= k) and g (S, >= k+1) complex double.  Outputs: Rcol = R[0..k, k], cs_k, sn_k, g_k, g_k1
    (double state), inv_hn, est2 (real, in T).  First-order error propagation as in solver_ref._step: the phase a / |a|
    moves by at most 2 e_a / |a| when a moves by e_a."""
    uT = unit_roundoff(dtype)
    cu = SQ2 * C_STC * U64
    ab = np.abs
    a1, a2 = _ldc(c1), _ldc(c2n)
    csl, snl, gl = np.asarray(hp(cs).numpy(), dtype=LD), _ldc(sn), _ldc(g)
    S = a1.shape[0]
    c2 = a2[:, :k + 1]
    ss = (c2.real ** 2 + c2.imag ** 2).sum(1)
    top = a2[:, k + 1].real
    n2 = top - ss
    e_n2 = U64 * (k + 4) * (ab(top) + ss)               # (k + 2)-term sum of two-product terms
    assert bool(((ab(n2) > 16 * e_n2) | (e_n2 == 0)).all()), "n2 within rounding of zero: hn is undetermined"
    pos = n2 > 0
    hn = np.sqrt(np.where(pos, n2, 0))
    e_hn = np.where(pos, e_n2 / (2 * np.where(pos, hn, 1)) + cu * hn, 0)
    h = a1[:, :k + 1] + a2[:, :k + 1]
    e_h = SQ2 * U64 * (ab(a1[:, :k + 1]) + ab(a2[:, :k + 1]))
    Rcol, e_R = np.zeros((S, k + 1), CLD), np.zeros((S, k + 1), LD)
    prev, e_prev = h[:, 0], e_h[:, 0]
    for j in range(k):
        nxt, e_nxt = h[:, j + 1], e_h[:, j + 1]
        c, t = csl[:, j], snl[:, j]
        Rcol[:, j] = c * prev + t * nxt
        e_R[:, j] = ab(c) * e_prev + ab(t) * e_nxt + cu * (ab(c * prev) + ab(t) * ab(nxt))
        t2 = t if fault == "sn_noconj" else np.conj(t)
        new = -t2 * prev + c * nxt
        e_prev = ab(t) * e_prev + ab(c) * e_nxt + cu * (ab(t) * ab(prev) + ab(c * nxt))
        prev = new
    a, e_a = prev, e_prev
    ma = ab(a)
    den = np.sqrt(ma * ma + hn * hn)
    nz = ma > 0
    mas, ds = np.where(nz, ma, 1), np.where(nz, den, 1)
    ph = np.where(nz, a / mas, 1)
    c = np.where(nz, (a.real if fault == "cs_no_abs" else ma) / ds, 0)
    t = np.where(nz, ph * hn / ds, 1)
    e_ph = np.where(nz, 2 * e_a / mas, 0)
    e_c = np.where(nz, (e_a + e_hn) / ds + cu, 0)
    e_t = np.where(nz, e_ph * hn / ds + (e_a + e_hn) / ds + cu * ab(t), 0)
    Rcol[:, k] = np.where(nz, ph * den, hn)
    e_R[:, k] = np.where(nz, e_ph * den + e_a + e_hn + cu * den, e_hn)
    gk = gl[:, k]
    g_k, e_g_k = c * gk, e_c * ab(gk) + cu * ab(c * gk)
    t2 = t if fault == "sn_noconj" else np.conj(t)
    gn = -t2 * gk
    e_gn = e_t * ab(gk) + cu * ab(gn)
    hs = np.where(hn > 0, hn, 1)
    inv = np.where(hn > 0, 1 / hs, 0)
    e_inv = np.where(hn > 0, e_hn / (hs * hs) + (cu + uT) / hs, 0)
    est = ab(gn) ** 2
    e_est = 2 * ab(gn) * e_gn + (cu + uT) * est
    out = dict(Rcol=(Rcol, e_R), cs_k=(c, e_c), sn_k=(t, e_t), g_k=(g_k, e_g_k), g_k1=(gn, e_gn),
               inv_hn=(inv, e_inv), est2=(est, e_est))
    return {n: (_t(v), _t(REF * np.asarray(e, dtype=LD))) for n, (v, e) in out.items()}


# ================================================================================================ xk_gmres_solve_c
def solve(dtype, R, g, kd, fault=None):
    """back substitution of the kd x kd upper triangle of R (complex double) against g; a zero pivot gives y_i = 0.
    Bound: |dy| <= gamma |R^-1| |R| |y| on the effective system (solver_ref.gmres_solve), where a complex multiply-add
    into a component is at most 4 real roundings on a term and the closing division (n conj(d)) / |d|^2 at most 7:
    gamma = SQ2 (4 kd + 7) u64; plus one rounding of T for the cast of either component."""
    Rt = torch.triu(torch.nan_to_num(hp(R)[:, :kd, :kd], nan=0.0))
    Rl, gl = _ldc(Rt), _ldc(hp(g)[:, :kd])
    S = Rl.shape[0]
    y = np.zeros((S, kd), CLD)
    with np.errstate(all="ignore"):
        for i in range(kd - 1, -1, -1):
            hi = min(kd, i + 65) if fault == "lane_wrap" else kd
            tot = (Rl[:, i, i + 1:hi] * y[:, i + 1:hi]).sum(1)
            d = Rl[:, i, i]
            if fault == "pivot_nan":
                y[:, i] = (gl[:, i] - tot) / d
            else:
                y[:, i] = np.where(d != 0, (gl[:, i] - tot) / np.where(d != 0, d, 1), 0)
    if fault is not None:
        yt = torch.from_numpy(np.ascontiguousarray(y.astype(np.complex128)))
        return {"y": (yt, torch.zeros(yt.shape, dtype=torch.float64))}
    yt = _t(y)
    dz = torch.diagonal(Rt, dim1=1, dim2=2) == 0
    Re = Rt.clone()
    Re[dz.unsqueeze(-1).expand_as(Re)] = 0
    Re = Re + torch.diag_embed(dz.to(torch.complex128))
    eye = torch.eye(kd, dtype=torch.complex128).expand(S, kd, kd)
    Rinv = torch.linalg.solve_triangular(Re, eye, upper=True)
    gam = SQ2 * (4 * kd + 7) * U64
    amp = (Rinv.abs() @ (Re.abs() @ yt.abs().unsqueeze(-1))).squeeze(-1)
    bnd = REF * gam * amp + SQ2 * unit_roundoff(dtype) * yt.abs()
    bnd[dz] = 0
    return {"y": (yt, bnd)}


# ================================================================================================ cases
def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(x) for x in key))) % (2 ** 31))


def _crandn(g, *shape):
    return torch.complex(torch.randn(shape, dtype=torch.float64, generator=g),
                         torch.randn(shape, dtype=torch.float64, generator=g))


def nan_like(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype) if not dtype.is_complex else \
        torch.full(shape, complex(float("nan"), float("nan")), dtype=dtype)


def ld_of(N):
    return (N + 7) // 8 * 8 + 8          # always a pad [npad, ld) for the poison


def _vectors(g, dtype, lead, N):
    """(*lead, ld) vectors: random on [0, N), zero on [N, npad), NaN on [npad, ld)"""
    ld, npad = ld_of(N), npad_of(N, dtype)
    v = nan_like((*lead, ld), dtype)
    v[..., :npad] = 0
    v[..., :N] = _crandn(g, *lead, N).to(dtype)
    return v


# (N, kq, S): N below (1), at (2, 1024, 2048) and off (5, 1027, 2051) the 16 B width and the tile; kq = 0, 1, not a
# multiple of 4, beyond one 64-row group; S = 1 and many.  The basis always has CAP_EXTRA poisoned rows beyond kq.
CAP_EXTRA = 3
GRAM_CONFIGS = [(1, 0, 1), (1, 1, 2), (2, 3, 1), (5, 1, 3), (5, 6, 1), (1024, 2, 2), (1027, 7, 3), (2048, 5, 1),
                (2051, 70, 2), (4100, 9, 1), (333, 130, 1), (2500, 0, 2)]


def gram_case(dtype, N, kq, S):
    g = _gen(1, N, kq, S, CV[dtype])
    Q = nan_like((S, kq + CAP_EXTRA, ld_of(N)), dtype)
    if kq:
        Q[:, :kq] = _vectors(g, dtype, (S, kq), N)
    return dict(N=N, kq=kq, S=S, Q=Q, w=_vectors(g, dtype, (S,), N), nblk=gram_tiles(N, dtype))


def gram_ref(dtype, case, fault=None):
    return gram(dtype, case["Q"], case["w"], case["N"], case["kq"], fault)


# (N, k, S, P, alpha, beta)
LINCOMB_CONFIGS = [(1, 0, 1, 1, 1.0, 0.0), (1, 1, 2, 1, -1.0, 1.0), (2, 3, 1, 1, -1.0, 1.0), (5, 6, 3, 2, 1.0, 0.0),
                   (513, 7, 2, 1, -1.0, 1.0), (512, 4, 1, 3, 0.5, -2.0), (1027, 33, 2, 1, 1.0, 0.0),
                   (300, 0, 2, 1, 1.0, 1.0)]


def lincomb_case(dtype, N, k, S, P, alpha, beta):
    g = _gen(2, N, k, S, P, CV[dtype])
    V = nan_like((S, k + CAP_EXTRA, ld_of(N)), dtype)
    if k:
        V[:, :k] = _vectors(g, dtype, (S, k), N)
    C = nan_like((S, P, k + CAP_EXTRA), dtype)
    C[:, :, :k] = _crandn(g, S, P, k).to(dtype)
    out = nan_like((S, P + 1, ld_of(N)), dtype)
    out[:, :P] = _vectors(g, dtype, (S, P), N)
    return dict(N=N, k=k, S=S, P=P, alpha=alpha, beta=beta, V=V, C=C, out0=out)


def lincomb_ref(dtype, case, fault=None):
    return lincomb(dtype, case["V"], case["C"], case["out0"], case["N"], case["k"], case["P"], case["alpha"],
                   case["beta"], fault)


# (N, k, S)
FINISH_CONFIGS = [(1, 0, 1), (2, 1, 2), (5, 2, 3), (5, 3, 1), (513, 4, 2), (1024, 6, 1), (1027, 33, 2)]


def finish_case(dtype, N, k, S):
    g = _gen(3, N, k, S, CV[dtype])
    Q = nan_like((S, k + 2 + CAP_EXTRA, ld_of(N)), dtype)
    Q[:, :k + 2] = _vectors(g, dtype, (S, k + 2), N)
    c2n = nan_like((S, k + 2 + CAP_EXTRA), dtype)
    c2n[:, :k + 2] = (1e-3 * _crandn(g, S, k + 2)).to(dtype)
    inv_hn = (0.5 + torch.rand(S, dtype=torch.float64, generator=g)).to(RDT[dtype])
    return dict(N=N, k=k, S=S, Q=Q, c2n=c2n, inv_hn=inv_hn)


def finish_ref(dtype, case, fault=None):
    return finish(dtype, case["Q"], case["c2n"], case["inv_hn"], case["N"], case["k"], fault)


# (k, S, edge): cap = STEP_CAP > k always; edges: a = 0 with hn > 0 (cs = 0, sn = 1), a = 0 and hn = 0, n2 < 0
STEP_CAP = 40
STEP_CONFIGS = [(k, S, None) for k in (0, 1, 2, 7, 31, STEP_CAP - 1) for S in (1, 65)] + \
               [(0, 5, "a0"), (3, 5, "a0"), (0, 5, "a0_hn0"), (2, 5, "n2_neg")]
STEP_EXTRA_SYSTEMS = 2


def step_case(dtype, k, S, edge):
    g = _gen(4, k, S, CV[dtype], 0 if edge is None else len(edge))
    St = S + STEP_EXTRA_SYSTEMS
    c1 = nan_like((S, STEP_CAP + 2), dtype)
    c2n = nan_like((S, STEP_CAP + 2), dtype)
    c1[:, :k + 1] = _crandn(g, S, k + 1).to(dtype)
    c2 = (1e-4 * _crandn(g, S, k + 1)).to(dtype)
    hn = 0.5 + torch.rand(S, dtype=torch.float64, generator=g)
    if edge in ("a0", "a0_hn0"):
        # zero Hessenberg column: every replayed entry and the final a are exactly 0
        c1[:, :k + 1] = 0
        c2 = torch.zeros_like(c2)
    c2n[:, :k + 1] = c2
    top = hn ** 2 + (hp(c2).abs() ** 2).sum(1)
    if edge == "a0_hn0":
        top = torch.zeros(S, dtype=torch.float64)
    if edge == "n2_neg":
        top = 0.25 * (hp(c2).abs() ** 2).sum(1)
    c2n[:, k + 1] = top.to(RDT[dtype]).to(dtype)
    # a unitary history: cs = cos, sn = sin * phase
    th = torch.rand(S, STEP_CAP, dtype=torch.float64, generator=g) * math.pi / 2
    ph = torch.rand(S, STEP_CAP, dtype=torch.float64, generator=g) * 2 * math.pi
    cs = nan_like((St, STEP_CAP), torch.float64)
    sn = nan_like((St, STEP_CAP), torch.complex128)
    gv = nan_like((St, STEP_CAP + 1), torch.complex128)
    R = nan_like((St, STEP_CAP + 1, STEP_CAP), torch.complex128)
    cs[:S, :k], sn[:S, :k] = torch.cos(th)[:, :k], (torch.sin(th) * torch.polar(torch.ones_like(ph), ph))[:, :k]
    gv[:S, :k + 1] = _crandn(g, S, k + 1)
    return dict(k=k, S=S, c1=c1, c2n=c2n, cs=cs, sn=sn, g=gv, R=R)


def step_ref(dtype, case, fault=None):
    S = case["S"]
    return step(dtype, case["c1"], case["c2n"], case["k"], case["cs"][:S], case["sn"][:S], case["g"][:S], fault)


# (kd, S, zero pivot row or None); cap = kd + 2
SOLVE_CONFIGS = [(1, 1, None), (2, 3, None), (5, 2, None), (63, 1, None), (64, 2, None), (65, 1, None), (130, 3, None),
                 (700, 1, None), (5, 2, 2), (130, 1, 70), (1, 2, 0)]


def solve_case(dtype, kd, S, zero):
    g = _gen(5, kd, S, CV[dtype], -1 if zero is None else zero)
    cap = kd + 2
    R = nan_like((S, cap + 1, cap), torch.complex128)
    # a well-conditioned triangle: dominant diagonal of modulus ~ 2, off-diagonal ~ 1 / kd
    T = _crandn(g, S, kd, kd) / max(kd, 1)
    d = torch.polar(1.5 + torch.rand(S, kd, dtype=torch.float64, generator=g),
                    torch.rand(S, kd, dtype=torch.float64, generator=g) * 2 * math.pi)
    T = torch.triu(T, diagonal=1) + torch.diag_embed(d)
    if zero is not None:
        T[:, zero, zero] = 0
    low = torch.tril(torch.ones(kd, kd, dtype=torch.bool), diagonal=-1)
    Rk = R[:, :kd, :kd]
    Rk[:, ~low] = T[:, ~low]                                   # below the diagonal stays NaN: never read
    gv = nan_like((S, cap + 1), torch.complex128)
    gv[:, :kd] = _crandn(g, S, kd)
    return dict(kd=kd, S=S, cap=cap, R=R, g=gv, zero=zero)


def solve_ref(dtype, case, fault=None):
    return solve(dtype, case["R"], case["g"], case["kd"], fault)


def visible(kernel, fault, cfg, dtype):
    """whether a planted fault changes any output at this configuration"""
    if kernel == "gram":
        N, kq, S = cfg
        if fault == "nrm_im":
            return True
        if fault == "drop_tail":
            return True                                        # the last vector always holds a non-zero element
        return kq > 0
    if kernel == "lincomb":
        N, k, S, P, alpha, beta = cfg
        return k % 4 != 0 if fault == "drop_tail_rows" else k > 0
    if kernel == "finish":
        N, k, S = cfg
        return (k + 1) % 4 != 0 if fault == "drop_tail_rows" else True
    if kernel == "step":
        k, S, edge = cfg
        return edge not in ("a0", "a0_hn0")                    # generic a and g are not real
    if kernel == "solve":
        kd, S, zero = cfg
        return zero is not None if fault == "pivot_nan" else kd > 65
    raise KeyError(kernel)
