"""Block Davidson for operators that live in HOST memory.

Device dispatch, not a fallback (see host_krylov.py): the reference's `davidson` runs on whatever device the operator is
on (xitorch/_impls/linalg/symeig.py:100-227, :149); an operator on a HIP device is served by native_eig.py's HIP kernels
and nothing else, an operator whose tensors are in host memory by this file.  The iteration is native_eig.py's — start
block from the reference's seed, Rayleigh-Ritz on the whole basis, ONE global stopping test `max|A X - M X diag(lam)| <
min_eps`, best block returned, expansion by the negated residual block, the basis grows until it spans the space — and so
is the restructuring: only the NEW block is orthonormalised (two passes of block Gram-Schmidt against the basis + a QR of
the block; the reference re-factorises the whole basis by CholeskyQR every iteration, `tallqr([V, t])`, which yields the
same Q in exact arithmetic), and `T = V^H A V` is extended by its new rows instead of being recomputed.  Each HIP kernel
call of the native driver is the torch expression it computes.  Nothing here imports `oracle/`.
"""
import math
import torch
from xitorch_amd._capi import NativeLibraryError
from xitorch_amd._util import bcast_shape
from xitorch_amd.dist import allreduce_max_
from xitorch_amd.linalg._block import _initial_block, _shard_of_global_batch, _shift_rel, GUARD_BAD, GUARD_MAX_REDO

__all__ = ["davidson", "chebfsi", "cheb_coefficients", "cheb_default_nguard", "gkl", "gkl_default_ncv", "lobpcg",
           "lobpcg_default_nguard", "chebwin_coefficients", "chebwin_jackson", "chebwin_ladder", "chebwin_degree",
           "chebwin_tail", "chebwin_select"]

calls = {"davidson": 0, "chebfsi": 0, "gkl": 0, "lobpcg": 0}


def _H(x):
    return x.transpose(-2, -1).conj()


def _orthonormalise(W, V, MV, M):
    """W (.., N, q) -> an (M-)orthonormal block, (M-)orthogonal to the basis V (V is None: the start block).
    Two rounds of [project out the basis, Householder QR of the block, and — with an overlap operator — a CholeskyQR of
    the now well-conditioned block in the M inner product].  A rank-deficient START block raises, like the native
    kernels; an expansion block whose residual columns are rounding noise (pairs that converged long ago) gets whatever
    orthonormal completion the QR supplies, which is harmless."""
    for _ in range(2):
        if V is not None:
            W = W - torch.matmul(V, torch.matmul(_H(MV), W))          # V (V^H M W): MV = M V, M Hermitian
        W, R = torch.linalg.qr(W)
        if V is None:
            d = torch.diagonal(R, dim1=-2, dim2=-1).abs()
            if bool((d.min(dim=-1)[0] <= 1e-13 * d.max(dim=-1)[0]).any()):
                raise RuntimeError("davidson: the start block is rank deficient (linearly dependent start vectors)")
        if M is not None:
            G = torch.matmul(_H(W), M.mm(W))
            L, info = torch.linalg.cholesky_ex((G + _H(G)) * 0.5)
            if bool((info != 0).any()):
                raise RuntimeError("davidson: the overlap operator M is not positive definite on the new block")
            W = torch.linalg.solve_triangular(_H(L), W, upper=True, left=False)
    return W


def davidson(A, neig, mode, M=None, max_niter=1000, nguess=None, v_init="randn", max_addition=None, min_eps=1e-6,
             verbose=False, V0=None, process_group=None, trace=None, rng_device="cpu", precond=None, restart=None,
             **unused):
    """Options as the reference's `davidson` plus `V0` (start block), `process_group` (batch-sharded ranks decide on
    the all-reduced residual) and `trace`, as in `native_eig.davidson`; the HIP driver's scheduling knobs are accepted
    and have no meaning here; `precond=` / `restart=` (extensions of the HIP driver) are not available."""
    calls["davidson"] += 1
    refuse_nearest("davidson", mode)
    dev = torch.device(A.device)
    if dev.type != "cpu":
        raise NativeLibraryError("host_eig serves operators in host memory only (operator is on %s): device operators "
                                 "run on the HIP kernels" % dev)
    if precond is not None or restart is not None:
        raise NativeLibraryError("precond= / restart= are extensions of the HIP davidson; not available for an "
                                 "operator in host memory")
    N = A.shape[-1]
    if nguess is None:
        nguess = neig
    bdims = list(A.shape[:-2]) if M is None else list(bcast_shape(A.shape[:-2], M.shape[:-2]))
    dtype = A.dtype
    B = 1
    for d in bdims:
        B *= d
    distributed = process_group is not None and torch.distributed.get_world_size(process_group) > 1
    shard = None
    if distributed and V0 is None and v_init.lower() in ("randn", "rand", "random"):
        shard = _shard_of_global_batch(B, dev, process_group)
    V = _initial_block(v_init, V0, bdims, B, N, nguess, dtype, dev, "cpu", shard)      # (B, nguess, N), panel-major
    V = V.transpose(-2, -1).reshape(*bdims, N, V.shape[-2])
    V = _orthonormalise(V, None, None, M)
    MV = M.mm(V) if M is not None else V
    AV = A.mm(V)
    T = torch.matmul(_H(V), AV)
    napply = 1
    best_resid, best = float("inf"), None
    history = []
    niter = 0
    for it in range(max_niter):
        niter = it + 1
        k = V.shape[-1]
        lam, Y = torch.linalg.eigh((T + _H(T)) * 0.5)
        if mode == "lowest":
            lam, Y = lam[..., :neig], Y[..., :neig]
        else:
            lam, Y = lam[..., -neig:], Y[..., -neig:]
        X = torch.matmul(V, Y)
        R = torch.matmul(AV, Y) - torch.matmul(MV, Y) * lam.unsqueeze(-2)
        mx = R.abs().max().double().reshape(1)
        max_resid = float(allreduce_max_(mx, process_group if distributed else None).item())
        history.append(max_resid)
        if verbose:
            print("Iter %3d (guess size: %d): resid: %.3e" % (it + 1, k, max_resid))
        if max_resid < best_resid:
            best_resid, best = max_resid, (lam, X)
        if max_resid < min_eps or k == N:
            break
        nadd = min(R.shape[-1], N - k)
        W = _orthonormalise(-R[..., :nadd], V, MV, M)
        AW = A.mm(W)
        napply += 1
        Tcol = torch.matmul(_H(V), AW)                                 # (.., k, nadd)
        Tnew = torch.matmul(_H(W), AW)                                 # (.., nadd, nadd)
        T = torch.cat((torch.cat((T, Tcol), dim=-1), torch.cat((_H(Tcol), Tnew), dim=-1)), dim=-2)
        V = torch.cat((V, W), dim=-1)
        AV = torch.cat((AV, AW), dim=-1)
        MV = torch.cat((MV, M.mm(W)), dim=-1) if M is not None else V
    if trace is not None:
        trace.update(niter=niter, napply=napply, resid_history=history, basis_size=int(V.shape[-1]),
                     best_resid=float(best_resid), groups=1, panel_kernel="host")
    return best


# ---------------------------------------------------------------------------------------------------------------------
# Chebyshev-filtered subspace iteration (extension; Zhou, Saad, Tiago, Chelikowsky, J. Comput. Phys. 219 (2006) 172)
# ---------------------------------------------------------------------------------------------------------------------
def cheb_default_nguard(neig, N):
    """guard vectors of the filtered block: max(8, ceil(neig / 4)), capped so that neig + nguard <= N"""
    return max(0, min(max(8, -(-neig // 4)), N - neig))


def cheb_coefficients(a, b, a0, degree, sign=1.0):
    """Coefficient table of one scaled Chebyshev filter: (degree, *S, 3) float64 from the float64 tensors a, b, a0 of
    shape S (any device; a handful of elementwise ops, no host synchronisation).  The filter is for B = sign * A with
    the unwanted part of B's spectrum in [a, b] and the scaling point a0 < a; step i computes
        Y_i = alpha_i (A Y_{i-1}) + beta_i Y_{i-1} + gamma_i Y_{i-2},     (alpha, beta, gamma) = table[i - 1]
    so that Y_m = p_m(B) Y_0 with p_m(t) = T_m((t - c) / e) / T_m((a0 - c) / e), c = (a + b) / 2, e = (b - a) / 2:
    sigma_1 = e / (a0 - c), Y_1 = (sigma_1 / e)(B - c) Y_0, then sigma' = 1 / (2 / sigma_1 - sigma),
    Y_i = (2 sigma' / e)(B - c) Y_{i-1} - sigma sigma' Y_{i-2}.  `sign` enters alpha only (B Y = sign * A Y).
    An interval without width (a zero operator, a multiple of the identity) gets the identity filter (0, 1, 0)."""
    a, b, a0 = a.to(torch.float64), b.to(torch.float64), a0.to(torch.float64)
    width = b - a0
    flat = ~(width > 1e-14 * torch.maximum(b.abs(), a0.abs()))          # (also NaN)
    safe_w = torch.where(flat, torch.ones_like(width), width)
    # keep the cut strictly inside (a0, b): a block whose Ritz values coincide must not collapse the interval
    a = torch.minimum(torch.maximum(a, a0 + 1e-3 * safe_w), b - 1e-3 * safe_w)
    a = torch.where(flat, a0 - 1.0, a)
    b = torch.where(flat, a0 + 1.0, b)
    e = (b - a) * 0.5
    c = (b + a) * 0.5
    sigma1 = e / (a0 - c)
    sigma = sigma1
    one, zero = torch.ones_like(e), torch.zeros_like(e)
    rows = []
    for i in range(degree):
        if i == 0:
            al, be, ga = sigma1 / e, -c * sigma1 / e, zero
        else:
            sn = 1.0 / (2.0 / sigma1 - sigma)
            al, be, ga = 2.0 * sn / e, -2.0 * sn * c / e, -sigma * sn
            sigma = sn
        al, be, ga = torch.where(flat, zero, al * sign), torch.where(flat, one, be), torch.where(flat, zero, ga)
        rows.append(torch.stack((al, be, ga), dim=-1))
    return torch.stack(rows, dim=0)


# ---- mode="nearest": the Jackson-damped Chebyshev delta filter (Li, Xi, Vecharynski, Yang, Saad, SIAM J. Sci. Comput.
# 38 (2016) A2512), evaluated by Clenshaw's recurrence; shared by this file's twin and native_chebfsi
CHEBWIN_FIRST_DEGREE = 20    # degree of the first filter of a run
CHEBWIN_LADDER_FLOOR = 8     # the ladder of the degree rule: 8, then m <- floor(1.25 m) + 1, ..., max_degree
_chebwin_tables = {}


def refuse_nearest(name, mode):
    """davidson and lobpcg find an END of the spectrum: asked for interior pairs they would return the uppermost"""
    if isinstance(mode, str) and mode.lower() == "nearest":
        raise NotImplementedError("%s: mode='nearest' (interior eigenpairs) is not supported by this method; use "
                                  "method='chebfsi' (or 'exacteig')" % name)


def chebwin_sigma(sigma, bdims, device):
    """the target of mode="nearest" as a float64 tensor of the batch shape on `device` (no gradient flows to it)"""
    if sigma is None:
        raise ValueError("mode='nearest' needs the target: pass sigma= (a number, or a real tensor broadcastable to "
                         "the batch dimensions)")
    s = sigma.detach() if isinstance(sigma, torch.Tensor) else torch.as_tensor(sigma)
    if s.is_complex():
        raise ValueError("mode='nearest': sigma must be real (the spectrum of a Hermitian operator is)")
    return s.to(device=device, dtype=torch.float64).expand(tuple(bdims)).contiguous()


def chebwin_select(lam, sigma):
    """(.., w) indices that order the Ritz values lam (.., w) by |lam - sigma| ascending (sigma (..,): the true
    target, not the clipped centre); torch ops on the values' device, no host read"""
    return torch.argsort((lam.to(torch.float64) - sigma.unsqueeze(-1)).abs(), dim=-1, stable=True)


def chebwin_jackson(m, device=None):
    """Jackson damping coefficients g_k^m, k = 0 .. m, float64: with a = pi / (m + 2),
    g_k = sin((k + 1) a) / ((m + 2) sin a) + (1 - (k + 1) / (m + 2)) cos(k a); g_0 = 1"""
    k = torch.arange(m + 1, dtype=torch.float64, device=device)
    a = math.pi / (m + 2)
    return torch.sin((k + 1) * a) / ((m + 2) * math.sin(a)) + (1.0 - (k + 1) / (m + 2)) * torch.cos(k * a)


def chebwin_interval(lo, hi):
    """(c, e, flat) of the interval [lo, hi] (float64 tensors): centre, half width, and the members whose spectrum has
    no width (a zero operator, a multiple of the identity; also NaN), which get c = lo, e = 1 and the identity filter"""
    lo, hi = lo.to(torch.float64), hi.to(torch.float64)
    width = hi - lo
    flat = ~(width > 1e-14 * torch.maximum(hi.abs(), lo.abs()))
    c = torch.where(flat, lo, (hi + lo) * 0.5)
    e = torch.where(flat, torch.ones_like(width), width * 0.5)
    return c, e, flat


def chebwin_angle(x, c, e):
    """theta = acos((x - c) / e), the argument clipped to [-1, 1]"""
    return torch.acos(torch.clamp((x.to(torch.float64) - c) / e, -1.0, 1.0))


def chebwin_coefficients(lo, hi, sigma_c, m):
    """Coefficient table of one band-pass filter of degree m >= 1 in Clenshaw form: (m + 1, *S, 4) float64 from the
    float64 tensors lo, hi, sigma_c of shape S (any device; elementwise ops, no host synchronisation).  With
    c = (hi + lo) / 2, e = (hi - lo) / 2, t = (lambda - c) / e and theta_s = acos(t(sigma_c)) the filter is
        p(t) = sum_{k=0..m} c_k T_k(t),   c_k = g_k^m mu_k / norm,   mu_k = (2 - delta_k0) cos(k theta_s),
    the Jackson-damped Chebyshev expansion of a delta function at sigma_c, normalised to p(t(sigma_c)) = 1.  Row 0 is
    (0, c_m, 0, 0): b_m = c_m X, one `cheb_step` on its first three entries.  Row j = 1 .. m is the Clenshaw step
        b_k = alpha (A b_{k+1}) + beta b_{k+1} + gamma b_{k+2} + delta X,   k = m - j,
    (alpha, beta, gamma, delta) = (2 / e, -2 c / e, -1, c_k) for k >= 1 and (1 / e, -c / e, -1, c_0) for the last one,
    whose result is p(A) X; gamma = 0 in row 1 (b_{m+1} = 0: the panel is not read).  That is m applies.  A member
    without spectral width gets the identity: (0, 1, 0, 0), then (0, 0, 0, 1)."""
    m = int(m)
    if m < 1:
        raise ValueError("chebwin_coefficients: the degree must be >= 1, got %d" % m)
    c, e, flat = chebwin_interval(lo, hi)
    th = chebwin_angle(sigma_c, c, e)
    dev = th.device
    shape = (m + 1,) + (1,) * th.dim()
    k = torch.arange(m + 1, dtype=torch.float64, device=dev).reshape(shape)
    cosk = torch.cos(k * th.unsqueeze(0))                               # (m + 1, *S)
    mu = cosk * 2.0
    mu[0] = cosk[0]
    gm = chebwin_jackson(m, dev).reshape(shape) * mu
    ck = gm / (gm * cosk).sum(dim=0, keepdim=True)                      # p(theta_s) = 1 (the Jackson kernel is > 0)
    ck = ck.flip(0)                                                     # row j holds c_{m-j}
    one, zero = torch.ones_like(ck), torch.zeros_like(ck)
    last = torch.zeros(shape, dtype=torch.bool, device=dev)
    last[m] = True
    first = torch.zeros(shape, dtype=torch.bool, device=dev)
    first[0] = True
    second = torch.zeros(shape, dtype=torch.bool, device=dev)
    second[1] = True
    scale = torch.where(last, one, 2.0 * one) / e.unsqueeze(0)          # 2 / e, the last row 1 / e
    al = torch.where(first, zero, scale)
    be = torch.where(first, ck, -scale * c.unsqueeze(0))
    ga = torch.where(first | second, zero, -one)
    de = torch.where(first, zero, ck)
    fl = flat.unsqueeze(0)
    al = torch.where(fl, zero, al)
    be = torch.where(fl, torch.where(first, one, zero), be)
    ga = torch.where(fl, zero, ga)
    de = torch.where(fl, torch.where(first, zero, one), de)
    return torch.stack((al, be, ga, de), dim=-1)


def chebwin_ladder(max_degree):
    """the degrees the rule chooses from: 8, then m <- floor(1.25 m) + 1 while below max_degree, then max_degree"""
    max_degree = int(max_degree)
    out, m = [], CHEBWIN_LADDER_FLOOR
    while m < max_degree:
        out.append(m)
        m = (5 * m) // 4 + 1
    out.append(max(1, max_degree))
    return out


def _chebwin_table(max_degree):
    """(ladder, G) with G (L, K + 1) float64 on the host: row l holds the Jackson coefficients of degree ladder[l],
    zero beyond it (built once per max_degree)"""
    key = int(max_degree)
    if key not in _chebwin_tables:
        ladder = chebwin_ladder(key)
        G = torch.zeros((len(ladder), ladder[-1] + 1), dtype=torch.float64)
        for i, m in enumerate(ladder):
            G[i, :m + 1] = chebwin_jackson(m)
        _chebwin_tables[key] = (ladder, G)
    return _chebwin_tables[key]


def chebwin_tail(theta_s, d_ref, max_degree):
    """(L, *S) float64: max |p_m(theta_s +- d_ref)| of the normalised filter of every ladder degree, by the closed form
    p_m(theta) = sum_k g_k^m mu_k cos(k theta) / sum_k g_k^m mu_k cos(k theta_s); torch ops on the angles' device"""
    ladder, G = _chebwin_table(max_degree)
    G = G.to(theta_s.device)
    S = theta_s.shape
    ts, d = theta_s.reshape(1, -1).to(torch.float64), d_ref.reshape(1, -1).to(torch.float64)
    k = torch.arange(G.shape[1], dtype=torch.float64, device=G.device).reshape(-1, 1)
    cs = torch.cos(k * ts)
    mu = cs * 2.0
    mu[0] = cs[0]
    peak = torch.matmul(G, mu * cs)
    up = torch.matmul(G, mu * torch.cos(k * (ts + d))).abs()
    dn = torch.matmul(G, mu * torch.cos(k * (ts - d))).abs()
    return (torch.maximum(up, dn) / peak).reshape(len(ladder), *S)


def chebwin_degree(theta_s, d_ref, filter_tail, max_degree):
    """The degree rule: the smallest degree of the ladder whose filter, centred at the angle theta_s, has fallen to
    `filter_tail` of its peak at the angular distance d_ref on both sides; a batch takes the largest degree any member
    asks for.  Returns (degree, capped): capped = no degree below max_degree satisfies it (max_degree is then used).
    ONE host read (the index into the ladder)."""
    ladder, _G = _chebwin_table(max_degree)
    ok = chebwin_tail(theta_s, d_ref, max_degree) <= filter_tail
    ok = ok.reshape(len(ladder), -1)
    ok[-1] = True
    idx = int(torch.argmax(ok.to(torch.int32), dim=0).max().item())
    return ladder[idx], idx == len(ladder) - 1


def chebwin_dref(lam_sel, theta_s, c, e, neig, w):
    """angular distance |theta - theta_s| of the (neig + ceil(nguard / 2))-th nearest block Ritz value (lam_sel (.., w)
    in the order of `chebwin_select`; the index is clipped to the block)"""
    idx = min(neig + -(-(w - neig) // 2), w) - 1
    return (chebwin_angle(lam_sel[..., idx], c, e) - theta_s).abs()


def _cheb_check_args(name, M, process_group):
    if M is not None:
        raise NotImplementedError("%s: an overlap operator M is not supported: the Chebyshev filter of A X = M X E acts "
                                  "on M^-1 A, and no M^-1 is available here; use method='davidson'" % name)
    if process_group is not None:
        raise NotImplementedError("%s: batch sharding over a process group is not supported by the filtered subspace "
                                  "iteration; use method='davidson'" % name)


def _cheb_lanczos_vector(bdims, N, dtype):
    """the one start vector of the bound-estimating Lanczos run: drawn on the host from a generator of its own (the
    global generators are left alone), the same numbers for the host twin and the device driver"""
    g = torch.Generator().manual_seed(12421 + 1)
    rd = torch.float64 if dtype in (torch.float64, torch.complex128) else torch.float32
    v = torch.randn((*bdims, N, 1), dtype=rd, generator=g)
    return v.to(dtype)


def _cheb_start_block(v_init, V0, bdims, B, N, w, dtype, dev, rng_device):
    """(B, w, N) panel-major start block: `_initial_block`'s, a caller's V0 completed by random columns when it has
    fewer than w"""
    if V0 is None:
        return _initial_block(v_init, None, bdims, B, N, w, dtype, dev, rng_device)
    V = _initial_block(v_init, V0, bdims, B, N, w, dtype, dev, rng_device)
    k = V.shape[1]
    if k >= w:
        return V[:, :w]
    extra = _initial_block("randn", None, bdims, B, N, w - k, dtype, dev, rng_device)
    return torch.cat((V, extra), dim=1)


def _cheb_host_lanczos(apply, bdims, N, dtype, rdt, lanczos_steps):
    """Ritz values (*bdims, ks) of A, ascending, and the residual norm |f_k| (*bdims,) of a short Lanczos run from the
    one start vector of `_cheb_lanczos_vector`, float64"""
    ks = max(2, min(int(lanczos_steps), N - 1))
    v = _cheb_lanczos_vector(bdims, N, dtype)
    v = v / torch.linalg.vector_norm(v, dim=-2, keepdim=True)
    vprev = torch.zeros_like(v)
    Tl = torch.zeros((*bdims, ks, ks), dtype=torch.float64)
    beta = torch.zeros((*bdims,), dtype=torch.float64)
    for j in range(ks):
        f = apply(v)
        al = (v.conj() * f).sum(dim=(-2, -1)).real.to(torch.float64)
        f = f - al.to(rdt)[..., None, None] * v - beta.to(rdt)[..., None, None] * vprev
        Tl[..., j, j] = al
        beta = torch.linalg.vector_norm(f, dim=(-2, -1)).to(torch.float64)
        if j + 1 < ks:
            Tl[..., j, j + 1] = beta
            Tl[..., j + 1, j] = beta
            inv = torch.where(beta > 0, 1.0 / beta, torch.zeros_like(beta))
            vprev, v = v, f * inv.to(rdt)[..., None, None]
    return torch.linalg.eigvalsh(Tl), beta


def chebwin_first_degree(filter_degree, max_degree):
    """(degree of the first filter, fixed): filter_degree=None is the adaptive rule, which starts at
    CHEBWIN_FIRST_DEGREE; an int fixes the degree of every filter.  max_degree caps both."""
    max_degree = int(max_degree)
    if max_degree < 1:
        raise ValueError("chebfsi: max_degree must be >= 1, got %d" % max_degree)
    if filter_degree is None:
        return min(CHEBWIN_FIRST_DEGREE, max_degree), False
    if int(filter_degree) < 1:
        raise ValueError("chebfsi: filter_degree must be None or an int >= 1, got %r" % (filter_degree,))
    return min(int(filter_degree), max_degree), True


def _chebfsi_nearest(apply, orth, X, sigma, neig, w, bdims, N, dtype, rdt, max_niter, min_eps, filter_degree,
                     max_degree, filter_tail, lanczos_steps, verbose, trace, napply):
    """mode="nearest" of the host twin: filtered subspace iteration with the band-pass filter of
    `chebwin_coefficients`, centred on sigma clipped to the Ritz extremes seen so far and evaluated by Clenshaw's
    recurrence (m applies); the Ritz pairs are ordered by |lambda - sigma| and the first neig are the wanted ones;
    after every Rayleigh-Ritz the degree rule `chebwin_degree` picks the next filter's degree.  Everything else —
    orthonormalisation passes, guard redo, stopping rule, best-block return — is chebfsi's."""
    import warnings
    from xitorch_amd._util import ConvergenceWarning
    theta, beta = _cheb_host_lanczos(apply, bdims, N, dtype, rdt, lanczos_steps)
    emin, emax = theta.min(dim=-1)[0], theta.max(dim=-1)[0]
    lo, hi = emin - beta, emax + beta
    deg_now, fixed = chebwin_first_degree(filter_degree, max_degree)
    capped = (not fixed) and deg_now == int(max_degree) and deg_now < CHEBWIN_FIRST_DEGREE
    gbad = GUARD_BAD[rdt]
    best_resid, best = float("inf"), None
    history, redo, degrees = [], [], []
    niter, passes, halved = 0, 2, False
    eye = torch.eye(w, dtype=dtype)
    for it in range(max_niter):
        niter = it + 1
        sigma_c = torch.minimum(torch.maximum(sigma, emin), emax)
        while True:
            coef = chebwin_coefficients(lo, hi, sigma_c, deg_now).to(rdt)              # (deg + 1, *bdims, 4)
            Bp, Bk = None, coef[0][..., None, None, 1] * X                             # b_m = c_m X
            for j in range(1, deg_now + 1):
                AB = apply(Bk)
                c4 = coef[j][..., None, None, :]
                Bn = c4[..., 0] * AB + c4[..., 1] * Bk
                if j > 1:
                    Bn = Bn + c4[..., 2] * Bp
                Bn = Bn + c4[..., 3] * X
                Bp, Bk = Bk, Bn
            Q = orth(Bk, passes)
            AQ = apply(Q)
            T = torch.matmul(_H(Q), AQ)
            mu, Yr = torch.linalg.eigh((T + _H(T)) * 0.5)
            sel = chebwin_select(mu, sigma)
            lam = torch.gather(mu, -1, sel)
            Yr = torch.gather(Yr, -1, sel.unsqueeze(-2).expand_as(Yr))
            Xn = torch.matmul(Q, Yr)
            R = torch.matmul(AQ, Yr[..., :neig]) - Xn[..., :neig] * lam[..., None, :neig]
            guard = float((torch.matmul(_H(Xn), Xn) - eye).abs().max())
            max_resid = float(R.abs().max())
            if guard <= gbad:
                break
            redo.append({"iter": niter, "guard": guard, "passes": passes + 1, "degree": max(1, deg_now // 2)})
            if len(redo) > 1:
                raise RuntimeError("xitorch_amd chebfsi: the filtered block lost its orthonormality twice (max|X^H X - "
                                   "I| = %.2e at iteration %d)" % (guard, niter))
            passes, deg_now, halved = 3, max(1, deg_now // 2), True
        X = Xn
        degrees.append(deg_now)
        if max_resid != max_resid:
            max_resid = float("inf")
        history.append(max_resid)
        if verbose:
            print("Iter %3d (block of %d, degree %d): resid: %.3e" % (niter, w, deg_now, max_resid))
        if max_resid < best_resid:
            best_resid, best = max_resid, (lam[..., :neig], Xn[..., :neig])
        if max_resid < min_eps:
            break
        mu = mu.to(torch.float64)
        emin, emax = torch.minimum(emin, mu.min(dim=-1)[0]), torch.maximum(emax, mu.max(dim=-1)[0])
        lo, hi = torch.minimum(lo, emin), torch.maximum(hi, emax)
        if not fixed:
            c, e, _flat = chebwin_interval(lo, hi)
            theta_s = chebwin_angle(torch.minimum(torch.maximum(sigma, emin), emax), c, e)
            deg_now, capped = chebwin_degree(theta_s, chebwin_dref(lam, theta_s, c, e, neig, w), filter_tail,
                                             max_degree)
            if halved:
                deg_now = max(1, deg_now // 2)
    if best is None:
        raise RuntimeError("xitorch_amd chebfsi: no finite residual was produced")
    if not best_resid < min_eps:
        warnings.warn(ConvergenceWarning("chebfsi: convergence is not achieved after %d iterations (max |resid| = %.3e "
                                         ">= min_eps = %.3e); the best block is returned" % (niter, best_resid, min_eps)))
    if trace is not None:
        trace.update(niter=niter, napply=napply(), degree=degrees[-1], degrees=degrees, w=w, resid_history=history,
                     best_resid=best_resid, sigma_centre=sigma_c.tolist(), degree_capped=bool(capped),
                     bounds={"lo": lo.tolist(), "hi": hi.tolist(), "emin": emin.tolist(), "emax": emax.tolist()},
                     small_eigh="library", guard_redo=redo, panel_kernel="host")
    evals, evecs = best
    order = torch.argsort(evals, dim=-1)                                              # ascending, like every mode
    return torch.gather(evals, -1, order), torch.gather(evecs, -1, order.unsqueeze(-2).expand_as(evecs))


def chebfsi(A, neig, mode, M=None, max_niter=100, min_eps=1e-6, degree=12, nguard=None, V0=None, v_init="randn",
            rng_device="cpu", lanczos_steps=12, verbose=False, trace=None, process_group=None, sigma=None,
            filter_degree=None, max_degree=1000, filter_tail=0.1, **unused):
    """Chebyshev-filtered subspace iteration in torch ops for a Hermitian operator in HOST memory: the statement of
    `native_chebfsi.chebfsi` (same options, same refusals, same decisions).  A block of w = neig + nguard vectors; per
    outer iteration `degree` applies through the three-term filter step, two orthonormalisation passes, one apply and a
    Rayleigh-Ritz of order w; the cut of the filter follows the block's largest Ritz value.  mode="uppest" filters -A
    through the sign of the coefficients.  A block that fails the guard is redone from the pre-filter block with a third
    pass and half the degree, which stay in force for the rest of the run; a second failure raises.  Stopping rule, best-block return and the guard thresholds are davidson's.
    mode="nearest" (with sigma=, filter_degree=, max_degree=, filter_tail=) is `_chebfsi_nearest`: the same outer
    iteration around a band-pass filter centred on sigma."""
    import warnings
    from xitorch_amd._util import ConvergenceWarning
    from xitorch_amd.linalg.native_eig import exacteig
    calls["chebfsi"] += 1
    _cheb_check_args("chebfsi", M, process_group)
    dev = torch.device(A.device)
    if dev.type != "cpu":
        raise NativeLibraryError("host_eig serves operators in host memory only (operator is on %s): device operators "
                                 "run on the HIP kernels" % dev)
    N, dtype = A.shape[-1], A.dtype
    bdims = list(A.shape[:-2])
    B = 1
    for d in bdims:
        B *= d
    if nguard is None:
        nguard = cheb_default_nguard(neig, N)
    w = min(N, neig + int(nguard))
    if V0 is not None and w < V0.shape[-1]:
        w = min(N, V0.shape[-1])
    nearest = mode == "nearest"
    if nearest:
        sigma = chebwin_sigma(sigma, bdims, dev)
    if N <= max(2 * w, 16):
        if trace is not None:
            trace.update(niter=0, napply=0, degree=degree, w=w, handed_to="exacteig")
        return exacteig(A, neig, mode, None, sigma=sigma) if nearest else exacteig(A, neig, mode, None)
    sign = 1.0 if mode == "lowest" else -1.0
    rdt = torch.float64 if dtype in (torch.float64, torch.complex128) else torch.float32
    napply = 0

    def apply(X):
        nonlocal napply
        napply += 1
        return A.mm(X)

    def orth(Y, passes):
        for _ in range(passes):
            Y, _R = torch.linalg.qr(Y)
        return Y

    X = _cheb_start_block(v_init, V0, bdims, B, N, w, dtype, dev, rng_device)          # (B, w, N)
    X = orth(X.transpose(-2, -1).reshape(*bdims, N, w), 2)
    if nearest:
        return _chebfsi_nearest(apply, orth, X, sigma, neig, w, bdims, N, dtype, rdt, max_niter, min_eps,
                                filter_degree, max_degree, filter_tail, lanczos_steps, verbose, trace,
                                lambda: napply)

    # spectral bounds of B = sign * A from a short Lanczos run (Zhou & Li's safeguarded upper bound)
    theta, beta = _cheb_host_lanczos(apply, bdims, N, dtype, rdt, lanczos_steps)
    theta = theta * sign                                                               # Ritz values of B
    th_min, th_max = theta.min(dim=-1)[0], theta.max(dim=-1)[0]
    b_sup = th_max + beta
    a0 = th_min
    a = theta.median(dim=-1)[0]

    gbad = GUARD_BAD[rdt]
    best_resid, best = float("inf"), None
    history, redo = [], []
    niter, deg_now, passes = 0, int(degree), 2
    eye = torch.eye(w, dtype=dtype)
    for it in range(max_niter):
        niter = it + 1
        while True:
            coef = cheb_coefficients(a, b_sup, a0, deg_now, sign).to(rdt)              # (deg, *bdims, 3)
            Yp, Y = None, X
            for i in range(deg_now):
                AY = apply(Y)
                c3 = coef[i][..., None, None, :]
                Yn = c3[..., 0] * AY + c3[..., 1] * Y
                if i > 0:
                    Yn = Yn + c3[..., 2] * Yp
                Yp, Y = Y, Yn
            Q = orth(Y, passes)
            AQ = apply(Q)
            T = torch.matmul(_H(Q), AQ)
            mu, Yr = torch.linalg.eigh((T + _H(T)) * (0.5 * sign))
            Xn = torch.matmul(Q, Yr)
            lam = mu * sign
            R = torch.matmul(AQ, Yr[..., :neig]) - Xn[..., :neig] * lam[..., None, :neig]
            guard = float((torch.matmul(_H(Xn), Xn) - eye).abs().max())
            max_resid = float(R.abs().max())
            if guard <= gbad:
                break
            redo.append({"iter": niter, "guard": guard, "passes": passes + 1, "degree": max(1, deg_now // 2)})
            if len(redo) > 1:
                raise RuntimeError("xitorch_amd chebfsi: the filtered block lost its orthonormality twice (max|X^H X - "
                                   "I| = %.2e at iteration %d)" % (guard, niter))
            passes, deg_now = 3, max(1, deg_now // 2)
        X = Xn
        if max_resid != max_resid:
            max_resid = float("inf")
        history.append(max_resid)
        if verbose:
            print("Iter %3d (block of %d, degree %d): resid: %.3e" % (niter, w, deg_now, max_resid))
        if max_resid < best_resid:
            best_resid, best = max_resid, (lam[..., :neig], Xn[..., :neig])
        if max_resid < min_eps:
            break
        a, a0 = mu.max(dim=-1)[0].to(torch.float64), mu.min(dim=-1)[0].to(torch.float64)
    if best is None:
        raise RuntimeError("xitorch_amd chebfsi: no finite residual was produced")
    if not best_resid < min_eps:
        warnings.warn(ConvergenceWarning("chebfsi: convergence is not achieved after %d iterations (max |resid| = %.3e "
                                         ">= min_eps = %.3e); the best block is returned" % (niter, best_resid, min_eps)))
    if trace is not None:
        trace.update(niter=niter, napply=napply, degree=deg_now, w=w, resid_history=history, best_resid=best_resid,
                     bounds={"a": a.tolist(), "b_sup": b_sup.tolist(), "a0": a0.tolist()}, small_eigh="library",
                     guard_redo=redo, panel_kernel="host")
    evals, evecs = best
    if mode != "lowest":
        evals, evecs = evals.flip(-1), evecs.flip(-1)
    return evals, evecs


# ---------------------------------------------------------------------------------------------------------------------
# Golub-Kahan-Lanczos bidiagonalisation with thick restart (extension; Baglama & Reichel, SIAM J. Sci. Comput. 27 (2005)
# 19; full reorthogonalisation as in Larsen's PROPACK): svd(method="gkl")
# ---------------------------------------------------------------------------------------------------------------------
GKL_MAX_NCV = 64             # order of the projected matrix the native small SVD serves (xk_gkl_bsvd)


def gkl_default_ncv(k, short):
    """basis size: min(max(2k + 8, 20), short side)"""
    return min(max(2 * k + 8, 20), short)


def _gkl_setup(A, k, mode, ncv, process_group):
    """argument checks and sizes shared by the host twin and the device driver: (m, n, tall, mm, nn, k, ncv, keep,
    dense) with mm >= nn the sides of the operator the iteration runs on (A, or A^H when m < n) and dense = the
    problem is handed to the dense SVD (short side <= max(2k, 16))."""
    if process_group is not None:
        raise NotImplementedError("gkl: batch sharding over a process group is not supported by the Golub-Kahan-"
                                  "Lanczos iteration; use method='davidson'")
    if mode not in ("lowest", "uppest"):
        raise ValueError("gkl: mode must be 'lowest' or 'uppest'/'uppermost', got %r" % (mode,))
    m, n = A.shape[-2], A.shape[-1]
    tall = m >= n
    mm, nn = (m, n) if tall else (n, m)
    if k is None:
        k = nn
    if k < 1 or k > nn:
        raise ValueError("gkl: k = %d singular triplets asked of an operator whose short side is %d" % (k, nn))
    dense = nn <= max(2 * k, 16)
    if ncv is None:
        ncv = gkl_default_ncv(k, nn)
        if not dense and ncv > GKL_MAX_NCV:
            raise ValueError("gkl: k = %d needs a basis of %d > %d vectors, beyond the native small SVD; pass a "
                             "smaller ncv (> k) or use method='davidson'" % (k, ncv, GKL_MAX_NCV))
    ncv = int(ncv)
    if ncv > GKL_MAX_NCV:
        raise ValueError("gkl: ncv = %d is beyond the native small SVD (ncv <= %d)" % (ncv, GKL_MAX_NCV))
    if not dense and k > ncv - 1:
        raise ValueError("gkl: k = %d needs ncv >= k + 1 (got ncv = %d)" % (k, ncv))
    if not dense and ncv > nn:
        raise ValueError("gkl: ncv = %d exceeds the short side %d of the operator" % (ncv, nn))
    keep = k + (ncv - k) // 2
    return m, n, tall, mm, nn, k, ncv, keep, dense


def _gkl_dense(A, k, mode):
    """the hand-off of small problems: the library SVD of the full matrix, k triplets, sigma ascending"""
    Uf, S, Vh = torch.linalg.svd(A.fullmatrix(), full_matrices=False)               # sigma descending
    if mode == "lowest":
        idx = torch.arange(S.shape[-1] - 1, S.shape[-1] - 1 - k, -1, device=S.device)      # smallest first
    else:
        idx = torch.arange(k - 1, -1, -1, device=S.device)                           # the k largest, ascending
    return Uf.index_select(-1, idx), S.index_select(-1, idx), _H(Vh).index_select(-1, idx)


def _gkl_start_vector(A, V0, v_init, bdims, B, nn, tall, dtype, dev, rng_device):
    """(B, nn) start vector on the SHORT side.  V0 (*batch, n, k0) holds guesses of right singular vectors of A: their
    sum starts the iteration (through A when the short side is the left one)."""
    if V0 is not None:
        if V0.shape[-2] != A.shape[-1]:
            raise RuntimeError("V0 must have shape (*batch, %d, k0), got %s" % (A.shape[-1], tuple(V0.shape)))
        v = V0.to(device=dev, dtype=dtype).sum(dim=-1, keepdim=True)
        if not tall:
            v = A.mm(v)
        return v.expand(*bdims, nn, 1).reshape(B, nn)
    return _initial_block(v_init, None, bdims, B, nn, 1, dtype, dev, rng_device).reshape(B, nn)


def _gkl_random(gen, B, N, dtype):
    """(B, N) replacement vectors after a breakdown: drawn on the host from the run's own generator"""
    rd = torch.float64 if dtype in (torch.float64, torch.complex128) else torch.float32
    return torch.randn((B, N), dtype=rd, generator=gen).to(dtype)


def gkl(A, k, mode, max_niter=100, min_eps=1e-6, ncv=None, V0=None, v_init="randn", rng_device="cpu", verbose=False,
        trace=None, process_group=None, **unused):
    """Golub-Kahan-Lanczos bidiagonalisation with thick restart in torch ops for an operator in HOST memory: the
    statement of `native_gkl.gkl` (same options, same refusals, same decisions).  Works on A itself — never on A^H A —
    always in the tall orientation (A^H when m < n).  Per Lanczos step one apply of A and one of A^H, each new vector
    orthogonalised against its whole basis by two classical Gram-Schmidt passes; alpha and beta are the norms.  A cycle
    fills the basis to ncv vectors, takes the SVD of the projected matrix (upper bidiagonal plus the restart arrow),
    and keeps k + (ncv - k) // 2 plain Ritz triplets.  Returns (u (*B, m, k), s (*B, k) ASCENDING like svd's other
    route, v (*B, n, k))."""
    import warnings
    from xitorch_amd._util import ConvergenceWarning
    calls["gkl"] += 1
    dev = torch.device(A.device)
    if dev.type != "cpu":
        raise NativeLibraryError("host_eig serves operators in host memory only (operator is on %s): device operators "
                                 "run on the HIP kernels" % dev)
    m, n, tall, mm, nn, k, ncv, keep, dense = _gkl_setup(A, k, mode, ncv, process_group)
    if dense:
        if trace is not None:
            trace.update(niter=0, napply=0, ncv=ncv, handed_to="dense_svd")
        return _gkl_dense(A, k, mode)
    dtype = A.dtype
    bdims = list(A.shape[:-2])
    B = 1
    for d in bdims:
        B *= d
    rdt = torch.float64 if dtype in (torch.float64, torch.complex128) else torch.float32
    u_round = torch.finfo(rdt).eps
    napply = 0

    def apply(x, adjoint):
        # x (B, len) -> (B, len'); the iteration's operator is A (tall) or A^H
        nonlocal napply
        napply += 1
        X = x.reshape(*bdims, x.shape[-1], 1)
        Y = A.rmm(X) if (adjoint == tall) else A.mm(X)
        return Y.expand(*bdims, Y.shape[-2], 1).reshape(B, Y.shape[-2])

    U = torch.zeros((B, mm, ncv), dtype=dtype)
    V = torch.zeros((B, nn, ncv + 1), dtype=dtype)
    Bm = torch.zeros((B, ncv, ncv), dtype=torch.float64)
    beta = torch.zeros((B,), dtype=torch.float64)
    smax = torch.zeros((B,), dtype=torch.float64)
    gen = torch.Generator().manual_seed(12421 + 7)
    breakdowns = []

    def orth(w, Q, code):
        """two classical Gram-Schmidt passes of w (B, len) against Q (B, len, j); (unit vector, norm (B,) float64);
        a member whose norm is <= u * (largest norm so far) breaks down: norm 0, a fresh random unit vector orthogonal
        to Q takes its place"""
        nonlocal smax
        for _ in range(2):
            if Q.shape[-1]:
                w = w - torch.matmul(Q, torch.matmul(_H(Q), w.unsqueeze(-1))).squeeze(-1)
        nrm = torch.linalg.vector_norm(w, dim=-1).to(torch.float64)
        bad = ~(nrm > u_round * smax) | ~torch.isfinite(nrm)
        if bool(bad.any()):
            breakdowns.append((code, bad.nonzero().flatten().tolist()))
            r = _gkl_random(gen, B, w.shape[-1], dtype)
            for _ in range(2):
                if Q.shape[-1]:
                    r = r - torch.matmul(Q, torch.matmul(_H(Q), r.unsqueeze(-1))).squeeze(-1)
            r = r / torch.linalg.vector_norm(r, dim=-1, keepdim=True)
            w = torch.where(bad.unsqueeze(-1), r, w / torch.where(bad, torch.ones_like(nrm), nrm).to(rdt).unsqueeze(-1))
            nrm = torch.where(bad, torch.zeros_like(nrm), nrm)
        else:
            w = w / nrm.to(rdt).unsqueeze(-1)
        smax = torch.maximum(smax, nrm)
        return w, nrm

    v0 = _gkl_start_vector(A, V0, v_init, bdims, B, nn, tall, dtype, dev, rng_device)
    nv0 = torch.linalg.vector_norm(v0, dim=-1, keepdim=True)
    if bool((nv0 == 0).any()):
        raise RuntimeError("gkl: the start vector is zero")
    V[:, :, 0] = v0 / nv0
    start, niter, history, conv_history, done = 0, 0, [], [], False
    descending = mode != "lowest"
    for cycle in range(max_niter):
        niter = cycle + 1
        for j in range(start, ncv):
            w, al = orth(apply(V[:, :, j], False), U[:, :, :j], 2 * j)
            U[:, :, j] = w
            Bm[:, j, j] = al
            w, be = orth(apply(U[:, :, j], True), V[:, :, :j + 1], 2 * j + 1)
            V[:, :, j + 1] = w
            if j + 1 < ncv:
                Bm[:, j, j + 1] = be
            else:
                beta = be
        P, S, Qh = torch.linalg.svd(Bm)
        Q = Qh.transpose(-2, -1)
        if not descending:
            P, S, Q = P.flip(-1), S.flip(-1), Q.flip(-1)
        rho = beta.unsqueeze(-1) * P[:, -1, :]
        res = rho.abs()
        scale = torch.maximum(S.max(dim=-1)[0], smax)
        nconv = (res[:, :k] <= min_eps * scale.unsqueeze(-1)).sum(dim=-1)
        history.append(float((res[:, :k] / scale.unsqueeze(-1)).max()))
        conv_history.append(nconv.tolist())
        if verbose:
            print("Cycle %3d (basis of %d): max |beta P[last, i]| / sigma_max = %.3e, converged %s"
                  % (niter, ncv, history[-1], nconv.tolist()))
        if bool((nconv >= k).all()):
            done = True
            break
        if cycle + 1 == max_niter:
            break
        Pc, Qc = P[:, :, :keep].to(dtype), Q[:, :, :keep].to(dtype)
        Vn = torch.zeros_like(V)
        Vn[:, :, :keep] = torch.matmul(V[:, :, :ncv], Qc)
        Vn[:, :, keep] = V[:, :, ncv]
        Un = torch.zeros_like(U)
        Un[:, :, :keep] = torch.matmul(U, Pc)
        U, V = Un, Vn
        Bm = torch.zeros_like(Bm)
        idx = torch.arange(keep)
        Bm[:, idx, idx] = S[:, :keep]
        Bm[:, idx, keep] = rho[:, :keep]
        start = keep
    if not done:
        warnings.warn(ConvergenceWarning("gkl: convergence is not achieved after %d restart cycles (max |beta P[last, i]| "
                                         "/ sigma_max = %.3e > min_eps = %.3e); the last Ritz block is returned"
                                         % (niter, history[-1], min_eps)))
    uu = torch.matmul(U, P[:, :, :k].to(dtype))
    vv = torch.matmul(V[:, :, :ncv], Q[:, :, :k].to(dtype))
    ss = S[:, :k].to(rdt)
    if descending:
        uu, vv, ss = uu.flip(-1), vv.flip(-1), ss.flip(-1)
    if not tall:
        uu, vv = vv, uu
    if trace is not None:
        trace.update(niter=niter, restarts=niter - 1, napply=napply, ncv=ncv, keep=keep, resid_history=history,
                     converged_history=conv_history, breakdowns=breakdowns, host_reads=None, panel_kernel="host", tall=tall, converged=done)
    return uu.reshape(*bdims, m, k), ss.reshape(*bdims, k), vv.reshape(*bdims, n, k)


# ---------------------------------------------------------------------------------------------------------------------
# LOBPCG in its basis-orthonormal form (extension; Knyazev, SIAM J. Sci. Comput. 23 (2001) 517; Duersch, Shao, Yang, Gu,
# SIAM J. Sci. Comput. 40 (2018) C655): symeig(method="lobpcg")
# ---------------------------------------------------------------------------------------------------------------------
LOBPCG_MAX_ROWS = 96         # order 3 w of the Rayleigh-Ritz problem the rotation kernel serves (xk_lobpcg_max_rows)


def lobpcg_default_nguard(neig, N):
    """guard vectors of the LOBPCG block: max(2, ceil(neig / 4)), capped so that neig + nguard <= N"""
    return max(0, min(max(2, -(-neig // 4)), N - neig))


def _lob_setup(A, neig, M, nguard, V0, process_group):
    """argument checks and sizes shared by the host twin and the device driver: (N, bdims, B, w, hand_over)"""
    if process_group is not None:
        raise NotImplementedError("lobpcg: batch sharding over a process group is not supported; use method='davidson'")
    N = A.shape[-1]
    bdims = list(A.shape[:-2]) if M is None else list(bcast_shape(A.shape[:-2], M.shape[:-2]))
    B = 1
    for d in bdims:
        B *= d
    if nguard is None:
        nguard = lobpcg_default_nguard(neig, N)
    w = min(N, neig + int(nguard))
    if V0 is not None and w < V0.shape[-1]:
        w = min(N, V0.shape[-1])
    hand_over = N <= max(5 * w, 16)
    if not hand_over and 3 * w > LOBPCG_MAX_ROWS:
        raise NotImplementedError("lobpcg: a block of %d vectors needs a Rayleigh-Ritz problem of order %d, beyond the "
                                  "%d rows of the rotation kernel; use method='chebfsi' (many pairs, M=None) or "
                                  "method='davidson'" % (w, 3 * w, LOBPCG_MAX_ROWS))
    return N, bdims, B, w, hand_over


def _lob_check_precond(precond):
    """the strings LOBPCG takes: "diag" / "jacobi", both T = |diag A|^-1.  davidson's third spelling "davidson" names
    its shifted form (diag A - lam diag M)^-1, which LOBPCG does not use: refused rather than reinterpreted"""
    if isinstance(precond, str) and precond.lower() not in ("diag", "jacobi"):
        raise RuntimeError("Unknown lobpcg preconditioner: %s (\"diag\" / \"jacobi\", a diagonal tensor or a "
                           "LinearOperator)" % precond)


def _lob_random(bdims, B, N, w, dtype, dev, rng_device, draw):
    """(B, w, N) panel-major random block number `draw` of a run, from a generator of its own (the global ones are left
    alone): the replacement of residual columns without a direction, and the redrawn W"""
    rdev = torch.device("cpu") if rng_device == "cpu" else dev
    g = torch.Generator(device=rdev).manual_seed(12421 + 2 + draw)
    return torch.randn((B, w, N), dtype=dtype, device=rdev, generator=g).to(dev)


def lob_dependent_columns(G, rdtype):
    """(B, w) bool, on the host: the columns of a block whose Gram matrix G = X^H M X (B, w, w) a Cholesky
    factorisation without pivoting finds dependent on the columns before them (pivot <= sqrt(u) G_jj, or not finite).
    Runs only after a failed orthonormalisation of the START block."""
    Gh = G.detach().cpu().to(torch.complex128 if G.is_complex() else torch.float64)
    B, w = Gh.shape[0], Gh.shape[-1]
    tol = float(torch.finfo(rdtype).eps) ** 0.5
    bad = torch.zeros((B, w), dtype=torch.bool)
    for b in range(B):
        L = torch.zeros_like(Gh[b])
        for j in range(w):
            gjj = float(Gh[b, j, j].real)
            piv = gjj - float((L[j, :j].abs() ** 2).sum())
            if not (piv > tol * gjj) or not (gjj > 0) or piv != piv:
                bad[b, j] = True
                continue
            L[j, j] = piv ** 0.5
            if j + 1 < w:
                L[j + 1:, j] = (Gh[b, j + 1:, j] - torch.matmul(L[j + 1:, :j], L[j, :j].conj())) / L[j, j]
                L[j + 1:, j][bad[b, j + 1:]] = 0
    return bad


def lob_cp(Cx, w):
    """The coefficient columns of the implicit search directions (Duersch et al., section 4.2): C_x (.., k, w) with
    its X rows (the first w) zeroed, projected against C_x and orthonormalised — twice, so that columns the first QR
    had to complete (directions that have converged away) end up orthogonal to C_x as well.  [C_x, C_p] then has
    orthonormal columns, and with an M-orthonormal S so have X' = S C_x and P' = S C_p.  Torch ops on small tensors of
    the operator's device, no host read."""
    Cp = Cx.clone()
    Cp[..., :w, :] = 0
    for _ in range(2):
        Cp = Cp - torch.matmul(Cx, torch.matmul(_H(Cx), Cp))
        Cp, _R = torch.linalg.qr(Cp)
    return Cp


def _lob_host_precond(precond, A, M, bdims, N, dtype):
    """davidson's grammar for operators in host memory: None, ("diag", d, None) with the (.., N) diagonal of A or the
    caller's, or ("op", LinearOperator)"""
    if precond is None:
        return None
    from xitorch_amd.linop import LinearOperator as _LinOp, MatrixLinearOperator

    def diag_of(op):
        if isinstance(op, MatrixLinearOperator):
            return op.mat.diagonal(dim1=-2, dim2=-1)
        return op.fullmatrix().diagonal(dim1=-2, dim2=-1)

    _lob_check_precond(precond)
    if isinstance(precond, str):
        return ("diag", diag_of(A).expand(*bdims, N), None)
    if isinstance(precond, torch.Tensor):
        if precond.shape[-1] != N:
            raise RuntimeError("precond diagonal must have shape (*batch, %d), got %s" % (N, tuple(precond.shape)))
        return ("diag", precond.to(dtype).expand(*bdims, N), None)
    if isinstance(precond, _LinOp):
        return ("op", precond)
    raise TypeError("precond must be None, 'diag', a tensor or a LinearOperator, got %s" % type(precond))


def lobpcg(A, neig, mode, M=None, max_niter=200, min_eps=1e-6, nguard=None, precond=None, V0=None, v_init="randn",
           rng_device="cpu", verbose=False, trace=None, process_group=None, **unused):
    """LOBPCG in torch ops for a Hermitian operator in HOST memory: the statement of `native_lobpcg.lobpcg` (same
    options, same refusals, same decisions; see there).  Three blocks S = [X | P | W] of w = neig + nguard vectors
    kept M-orthonormal, one operator product and one preconditioner product per iteration, a Rayleigh-Ritz problem of
    order 3 w recomputed from the blocks, P formed from orthonormal coefficient columns (`lob_cp`)."""
    import warnings
    from xitorch_amd._util import ConvergenceWarning
    from xitorch_amd.linalg.native_eig import exacteig
    calls["lobpcg"] += 1
    refuse_nearest("lobpcg", mode)
    dev = torch.device(A.device)
    if dev.type != "cpu":
        raise NativeLibraryError("host_eig serves operators in host memory only (operator is on %s): device operators "
                                 "run on the HIP kernels" % dev)
    N, bdims, B, w, hand_over = _lob_setup(A, neig, M, nguard, V0, process_group)
    _lob_check_precond(precond)
    dtype = A.dtype
    if hand_over:
        if trace is not None:
            trace.update(niter=0, napply=0, w=w, handed_to="exacteig")
        return exacteig(A, neig, mode, M)
    sign = 1.0 if mode == "lowest" else -1.0
    rdt = torch.float64 if dtype in (torch.float64, torch.complex128) else torch.float32
    gbad = GUARD_BAD[rdt]
    pc = _lob_host_precond(precond, A, M, bdims, N, dtype)
    napply, ndraw, redraws, restarts = 0, 0, 0, 0
    eye = torch.eye(w, dtype=dtype)

    def apply(X):
        nonlocal napply
        napply += 1
        return A.mm(X)

    def Mmm(X):
        return M.mm(X) if M is not None else X

    def random_block():
        nonlocal ndraw
        ndraw += 1
        return _lob_random(bdims, B, N, w, dtype, dev, rng_device, ndraw).transpose(-2, -1).reshape(*bdims, N, w)

    def orth(W, Q, MQ, passes):
        """W M-orthonormal and M-orthogonal to Q: `passes` x [projection, CholeskyQR], the first CholeskyQR shifted;
        M is applied once and M W transformed alongside.  Returns (W, M W, largest Cholesky flag)."""
        MW = Mmm(W)
        flag = 0
        for r in range(passes):
            if Q is not None:
                c = torch.matmul(_H(MQ), W)
                W = W - torch.matmul(Q, c)
                MW = MW - torch.matmul(MQ, c) if M is not None else W
            G = torch.matmul(_H(W), MW)
            G = (G + _H(G)) * 0.5
            if r == 0 and passes > 1:
                tr = torch.diagonal(G, dim1=-2, dim2=-1).sum(-1).real
                G = G + (_shift_rel(N, w, rdt) * tr)[..., None, None] * eye
            L, info = torch.linalg.cholesky_ex(G)
            flag = max(flag, int(info.max()))
            ok = (info == 0)[..., None, None]
            L = torch.where(ok, L, eye.expand_as(L))
            W = torch.linalg.solve_triangular(_H(L), W, upper=True, left=False)
            MW = torch.linalg.solve_triangular(_H(L), MW, upper=True, left=False) if M is not None else W
        return W, MW, flag

    def ritz_on_x(X, AX, MX):
        """Rayleigh-Ritz on span(X) alone: (X, AX, MX rotated, lam (.., w), residual block)"""
        T = torch.matmul(_H(X), AX)
        mu, Y = torch.linalg.eigh((T + _H(T)) * (0.5 * sign))
        lam = mu * sign
        X, AX = torch.matmul(X, Y), torch.matmul(AX, Y)
        MX = torch.matmul(MX, Y) if M is not None else X
        return X, AX, MX, lam, AX - MX * lam.unsqueeze(-2).to(dtype)

    def guard_of(X, MX):
        g = float((torch.matmul(_H(X), MX) - eye).abs().max())
        return g if g == g else float("inf")

    # ---- start: M-orthonormal block, Rayleigh-Ritz on it alone
    spare = random_block()          # random directions, drawn once: what replaces a column without a direction
    X = _cheb_start_block(v_init, V0, bdims, B, N, w, dtype, dev, rng_device)          # (B, w, N)
    X = X.transpose(-2, -1).reshape(*bdims, N, w)
    X1, MX, flag = orth(X, None, None, 2)
    if flag != 0 or guard_of(X1, MX) > gbad:
        # dependent start vectors (the shifted first pass hides them from the Cholesky flag; the guard sees them): the
        # columns a Cholesky factorisation of the Gram matrix finds dependent are drawn afresh, and the block gets
        # three passes; a second failure raises
        G = torch.matmul(_H(X), Mmm(X)).reshape(B, w, w)
        bad = lob_dependent_columns(G, rdt).reshape(*bdims, 1, w)
        redraws += int(bad.sum())
        X1, MX, flag = orth(torch.where(bad, spare, X), None, None, 3)
        if flag != 0:
            raise RuntimeError("lobpcg: the start block is rank deficient (linearly dependent start vectors)")
    X = X1
    AX = apply(X)
    X, AX, MX, lam, R = ritz_on_x(X, AX, MX)
    P = AP = MP = None
    guard = guard_of(X, MX)
    if guard > gbad:
        raise RuntimeError("lobpcg: the start block is not orthonormal (max|X^H M X - I| = %.2e)" % guard)

    best_resid, best = float("inf"), None
    history = []
    niter, nfail = 0, 0
    while True:
        max_resid = float(R[..., :neig].abs().max())
        if max_resid != max_resid:
            max_resid = float("inf")
        history.append(max_resid)
        if verbose:
            print("Iter %3d (block of %d): resid: %.3e" % (niter, w, max_resid))
        if max_resid < best_resid:
            best_resid, best = max_resid, (lam[..., :neig], X[..., :neig])
        if max_resid < min_eps or niter >= max_niter:
            break
        niter += 1
        # W = T R, columns scaled to unit norm; a column without a direction is replaced, never divided by
        if pc is None:
            W = R
        elif pc[0] == "diag":
            # Jacobi: T = |diag|^-1, positive definite as LOBPCG needs it.  (Davidson's denominator diag A - lam diag M
            # is indefinite for every column but the first: 142 iterations with it on the diagonally dominant test
            # matrix, 13 with this one, 72 without a preconditioner.)
            W = R / pc[1].abs().clamp(min=float(torch.finfo(rdt).eps) ** 0.5).unsqueeze(-1).to(dtype)
        else:
            W = pc[1].mm(R)
        nrm = torch.linalg.vector_norm(W, dim=-2, keepdim=True)
        bad = ~(torch.isfinite(nrm) & (nrm > 0))
        if bool(bad.any()):
            redraws += int(bad.sum())
            W = torch.where(bad, spare, W)
            nrm = torch.where(bad, torch.ones_like(nrm), nrm)
        W = W / nrm
        Q = X if P is None else torch.cat((X, P), dim=-1)
        AQ = AX if P is None else torch.cat((AX, AP), dim=-1)
        MQ = Q if M is None else (MX if P is None else torch.cat((MX, MP), dim=-1))
        W1, MW, flag = orth(W, Q, MQ, 2)
        if flag != 0:
            redraws += w
            W1, MW, flag = orth(random_block(), Q, MQ, 3)
            if flag != 0:
                raise RuntimeError("xitorch_amd lobpcg: the new directions could not be orthonormalised against the "
                                   "block (Cholesky flag %d at iteration %d)" % (flag, niter))
        W = W1
        AW = apply(W)
        S, AS = torch.cat((Q, W), dim=-1), torch.cat((AQ, AW), dim=-1)
        MS = S if M is None else torch.cat((MQ, MW), dim=-1)
        T = torch.matmul(_H(S), AS)                                   # recomputed from the blocks every iteration
        mu, Y = torch.linalg.eigh((T + _H(T)) * (0.5 * sign))
        Cx = Y[..., :w]
        lam = mu[..., :w] * sign
        Cp = lob_cp(Cx, w)
        X, P = torch.matmul(S, Cx), torch.matmul(S, Cp)
        AX, AP = torch.matmul(AS, Cx), torch.matmul(AS, Cp)
        MX, MP = (torch.matmul(MS, Cx), torch.matmul(MS, Cp)) if M is not None else (X, P)
        R = AX - MX * lam.unsqueeze(-2).to(dtype)
        guard = guard_of(X, MX)
        if guard > gbad:
            # never returned or kept: re-orthonormalise X, drop P (the next problem has order 2 w), go on
            restarts += 1
            nfail += 1
            if nfail > GUARD_MAX_REDO:
                raise RuntimeError("xitorch_amd lobpcg: the block lost its orthonormality %d times (max|X^H M X - I| = "
                                   "%.2e at iteration %d)" % (nfail, guard, niter))
            X, MX, flag = orth(X, None, None, 3)
            if flag != 0:
                raise RuntimeError("xitorch_amd lobpcg: the block is rank deficient after a guard failure")
            AX = apply(X)
            X, AX, MX, lam, R = ritz_on_x(X, AX, MX)
            P = AP = MP = None
            if guard_of(X, MX) > gbad:
                R = torch.full_like(R, float("inf"))
    if best is None:
        raise RuntimeError("xitorch_amd lobpcg: no finite residual was produced")
    if not best_resid < min_eps:
        warnings.warn(ConvergenceWarning("lobpcg: convergence is not achieved after %d iterations (max |resid| = %.3e "
                                         ">= min_eps = %.3e); the best block is returned" % (niter, best_resid, min_eps)))
    if trace is not None:
        trace.update(niter=niter, napply=napply, w=w, resid_history=history, best_resid=best_resid, restarts=restarts,
                     redraws=redraws, small_eigh="library", panel_kernel="host")
    evals, evecs = best
    if mode != "lowest":
        evals, evecs = evals.flip(-1), evecs.flip(-1)
    return evals, evecs


# ---------------------------------------------------------------------------------------------------------------------
# Krylov-Schur Arnoldi for non-Hermitian eigenpairs (extension; Stewart, SIAM J. Matrix Anal. Appl. 23 (2001) 601):
# eigs(method="arnoldi")
# ---------------------------------------------------------------------------------------------------------------------
__all__ += ["arnoldi", "arn_default_ncv"]
calls.setdefault("arnoldi", 0)
ARN_MAX_NCV = 48             # order of the projected matrix the native small Schur kernel serves (xk_arn_schur)
ARN_WHICH = ("LM", "LR", "SR", "LI", "SI")
ARN_PAIR_RTOL = 1e-6         # two eigenvalues of a real matrix are conjugate partners within this relative distance
ARN_CLOSED_TOL = 1e-8        # a column of [Re Z | Im Z] longer than this outside the real basis: the pairing misjudged


def arn_default_ncv(neig, n):
    """basis size: min(max(2 neig + 8, 20), n)"""
    return min(max(2 * neig + 8, 20), n)


def _arn_check(A, neig, which, M, process_group):
    """the refusals every route of eigs shares (the dense one included); returns (n, neig)"""
    if M is not None:
        raise NotImplementedError("eigs: the generalised problem (M=) is not supported")
    if process_group is not None:
        raise NotImplementedError("eigs: batch sharding over a process group is not supported")
    if A.shape[-1] != A.shape[-2]:
        raise RuntimeError("eigs: the operator must be square, got %s" % (tuple(A.shape),))
    if which == "SM":
        raise ValueError("eigs: which='SM' needs shift-and-invert, which is not built; for the eigenvalues nearest 0 "
                         "run eigs on an operator that applies the inverse and take 1 / lambda")
    if which not in ARN_WHICH:
        raise ValueError("eigs: which must be one of %s, got %r" % (", ".join(ARN_WHICH), which))
    if which in ("LI", "SI") and not A.dtype.is_complex:
        raise ValueError("eigs: which=%r is for complex operators; the spectrum of a real operator is symmetric about "
                         "the real axis" % which)
    n = A.shape[-1]
    if neig is None or neig < 1 or neig > n:
        raise ValueError("eigs: neig = %r eigenpairs asked of an operator of order %d" % (neig, n))
    return n, int(neig)


def _arn_setup(A, neig, which, ncv, M, process_group):
    """argument checks and sizes shared by the host twin and the device driver: (n, neig, ncv, keep, dense) with dense
    = the problem is handed to the dense eigensolver (n <= max(2 neig, 16))."""
    n, neig = _arn_check(A, neig, which, M, process_group)
    dense = n <= max(2 * neig, 16)
    if ncv is None:
        ncv = arn_default_ncv(neig, n)
        if not dense and ncv > ARN_MAX_NCV:
            raise ValueError("eigs: neig = %d needs a basis of %d > %d vectors, beyond the native small Schur kernel; "
                             "pass a smaller ncv (>= neig + 2)" % (neig, ncv, ARN_MAX_NCV))
    ncv = int(ncv)
    if not dense:
        if ncv > ARN_MAX_NCV:
            raise ValueError("eigs: ncv = %d is beyond the native small Schur kernel (ncv <= %d)" % (ncv, ARN_MAX_NCV))
        if neig > ncv - 2:
            raise ValueError("eigs: neig = %d needs ncv >= neig + 2 (got ncv = %d)" % (neig, ncv))
        if ncv > n:
            raise ValueError("eigs: ncv = %d exceeds the order %d of the operator" % (ncv, n))
    keep = neig + (ncv - neig) // 2
    return n, neig, ncv, keep, dense


def _arn_key(lam, which):
    if which == "LM":
        return lam.abs()
    if which in ("LR", "SR"):
        return lam.real if which == "LR" else -lam.real
    return lam.imag if which == "LI" else -lam.imag


def _arn_order(lam, which, real_op):
    """The ranking of xk_arn_schur on one member's eigenvalues lam (m,) complex128 (host): (order, partner) with order
    the indices best first by `which`.  For a real operator an eigenvalue and the nearest one of opposite imaginary
    part, if it is its conjugate to ARN_PAIR_RTOL, are partners: they share the larger key and stay adjacent, positive
    imaginary part first."""
    m = lam.shape[0]
    key = _arn_key(lam, which).tolist()
    re, im = lam.real.tolist(), lam.imag.tolist()
    partner = [-1] * m
    if real_op:
        for i in range(m):
            if partner[i] >= 0 or im[i] == 0.0:
                continue
            best, bd = -1, 0.0
            for j in range(m):
                if j == i or partner[j] >= 0 or not im[j] * im[i] < 0.0:
                    continue
                d = math.hypot(re[j] - re[i], im[j] + im[i])
                if best < 0 or d < bd:
                    best, bd = j, d
            if best >= 0 and bd <= ARN_PAIR_RTOL * max(math.hypot(re[i], im[i]), math.hypot(re[best], im[best])):
                partner[i], partner[best] = best, i
    skey = [max(key[i], key[partner[i]]) if partner[i] >= 0 else key[i] for i in range(m)]
    lead = [min(i, partner[i]) if partner[i] >= 0 else i for i in range(m)]
    order = sorted(range(m), key=lambda i: (-skey[i], lead[i], -im[i], i))
    return order, partner


def _arn_cut(order, partner, keep, m):
    """keep' of xk_arn_schur: keep, moved by one when the cut separates partners, never above m - 1"""
    kp = min(keep, m - 1)
    if partner[order[kp - 1]] == order[kp]:
        kp += 1
    if kp > m - 1:
        kp = m - 1
        if partner[order[kp - 1]] == order[kp]:
            kp -= 1
    return kp


def _arn_complex_dtype(dtype):
    return torch.complex128 if dtype in (torch.float64, torch.complex128) else torch.complex64


def _arn_select(evals, evecs, neig, which, real_op, out_dtype):
    """the first neig eigenpairs of every member in the order of `which`; evals (B, m), evecs (B, n, m) complex"""
    ev, vec = evals.to("cpu", torch.complex128), evecs
    idx = torch.tensor([_arn_order(ev[b], which, real_op)[0][:neig] for b in range(ev.shape[0])], dtype=torch.int64)
    idx = idx.to(evals.device)
    lam = torch.gather(evals, 1, idx)
    X = torch.gather(vec, 2, idx.unsqueeze(1).expand(-1, vec.shape[1], -1))
    X = X / torch.linalg.vector_norm(X, dim=1, keepdim=True)
    return lam.to(out_dtype), X.to(out_dtype)


def _arn_dense(A, neig, which):
    """the dense route (method="exacteig" and the hand-over of small problems): the library eigensolver on the full
    matrix, in host memory (the general eigenproblem has no device route here), and the same selection"""
    full = A.fullmatrix()
    bdims, n = list(full.shape[:-2]), full.shape[-1]
    cdt = _arn_complex_dtype(A.dtype)
    ev, vec = torch.linalg.eig(full.reshape(-1, n, n).to("cpu"))
    lam, X = _arn_select(ev, vec, neig, which, not A.dtype.is_complex, cdt)
    return lam.reshape(*bdims, neig).to(full.device), X.reshape(*bdims, n, neig).to(full.device)


def _arn_start_vector(A, V0, v_init, bdims, B, n, dtype, dev, rng_device):
    """(B, n) start vector; V0 (*batch, n, k0) holds guesses of eigenvectors: their sum starts the iteration (the real
    part of the sum for a real operator)"""
    if V0 is not None:
        if V0.shape[-2] != n:
            raise RuntimeError("V0 must have shape (*batch, %d, k0), got %s" % (n, tuple(V0.shape)))
        v = V0.sum(dim=-1, keepdim=True)
        if v.is_complex() and not dtype.is_complex:
            v = v.real
        v = v.to(device=dev, dtype=dtype)
        return v.expand(*bdims, n, 1).reshape(B, n)
    return _initial_block(v_init, None, bdims, B, n, 1, dtype, dev, rng_device).reshape(B, n)


def _arn_true_residuals(apply_cols, X, lam, real_op):
    """|A x_i - theta_i x_i| per pair in the output precision; X (B, n, k) complex, apply_cols maps (B, n, p) of the
    OPERATOR's dtype to A times it"""
    if real_op:
        k = X.shape[-1]
        AX = apply_cols(torch.cat([X.real, X.imag], dim=-1).contiguous())
        AX = torch.complex(AX[..., :k], AX[..., k:])
    else:
        AX = apply_cols(X)
    return torch.linalg.vector_norm(AX - X * lam.unsqueeze(-2), dim=-2)


def _arn_finish_report(resid, lam, hfro, u_round, min_eps, niter, done):
    """the one ConvergenceWarning of a call: pairs whose true residual misses the bound by more than a factor 2"""
    import warnings
    from xitorch_amd._util import ConvergenceWarning
    bound = min_eps * torch.maximum(lam.abs().to(torch.float64), (u_round * hfro).unsqueeze(-1))
    nmiss = int((~(resid.to(torch.float64) <= 2.0 * bound)).sum())
    if nmiss or not done:
        worst = float((resid.to(torch.float64) / torch.clamp(bound, min=1e-300)).max())
        warnings.warn(ConvergenceWarning("eigs: %d of %d eigenpairs miss |A x - theta x| <= min_eps max(|theta|, u |H|_F) "
                                         "by more than a factor 2 after %d restart cycles (worst ratio %.3e, min_eps = "
                                         "%.3e); the last Ritz block is returned"
                                         % (nmiss, resid.numel(), niter, worst, min_eps)))
    return nmiss


def arnoldi(A, neig, which="LM", max_niter=100, min_eps=1e-6, ncv=None, V0=None, v_init="randn", rng_device="cpu",
            verbose=False, trace=None, M=None, process_group=None, **unused):
    """Krylov-Schur Arnoldi in torch ops for an operator in HOST memory: the statement of `native_arnoldi.arnoldi`
    (same options, same refusals, same decisions).  One Arnoldi vector per member and step, orthogonalised against the
    whole basis by two classical Gram-Schmidt passes, the column of H the sum of their coefficients.  A cycle fills
    the basis to ncv vectors; the small problem goes through the library's eig: the wanted eigenvectors' span is that
    of the reordered Schur vectors the device kernel keeps, and an orthonormal basis of it (QR; for a real operator a
    real basis of [Re | Im] by SVD) restarts the iteration with H = Q^H B Q and the spike beta Q[m-1, :].  Returns
    (evals (*B, neig), evecs (*B, n, neig)), complex."""
    calls["arnoldi"] += 1
    dev = torch.device(A.device)
    if dev.type != "cpu":
        raise NativeLibraryError("host_eig serves operators in host memory only (operator is on %s): device operators "
                                 "run on the HIP kernels" % dev)
    n, neig, ncv, keep, dense = _arn_setup(A, neig, which, ncv, M, process_group)
    if dense:
        if trace is not None:
            trace.update(niter=0, napply=0, ncv=ncv, handed_to="dense_eig")
        return _arn_dense(A, neig, which)
    dtype = A.dtype
    real_op = not dtype.is_complex
    cdt = _arn_complex_dtype(dtype)
    hdt = torch.float64 if real_op else torch.complex128
    bdims = list(A.shape[:-2])
    B = 1
    for d in bdims:
        B *= d
    rdt = torch.float64 if dtype in (torch.float64, torch.complex128) else torch.float32
    u_round = torch.finfo(rdt).eps
    napply = 0
    m = ncv

    def apply_cols(X):
        # (B, n, p) -> A X
        nonlocal napply
        napply += 1
        Y = A.mm(X.reshape(*bdims, n, X.shape[-1]))
        return Y.expand(*bdims, n, X.shape[-1]).reshape(B, n, X.shape[-1])

    V = torch.zeros((B, n, m + 1), dtype=dtype)
    H = torch.zeros((B, m + 1, m), dtype=hdt)
    smax = torch.zeros((B,), dtype=torch.float64)
    gen = torch.Generator().manual_seed(12421 + 11)
    breakdowns = []

    def project(w, Q):
        c = torch.matmul(_H(Q), w.unsqueeze(-1))
        return w - torch.matmul(Q, c).squeeze(-1), c.squeeze(-1)

    def step(j, kps):
        # members whose restart kept more than j vectors (kps[b] > j) hold column j already: the step leaves them alone
        nonlocal smax
        live = torch.tensor([kp <= j for kp in kps])
        Q = V[:, :, :j + 1]
        w = apply_cols(V[:, :, j:j + 1]).squeeze(-1)
        w, c1 = project(w, Q)
        w, c2 = project(w, Q)
        nrm = torch.linalg.vector_norm(w, dim=-1).to(torch.float64)
        bad = (~(nrm > u_round * smax) | ~torch.isfinite(nrm)) & live
        if bool(bad.any()):
            breakdowns.append((j, bad.nonzero().flatten().tolist()))
            r = _gkl_random(gen, B, n, dtype)
            r, _ = project(r, Q)
            r, _ = project(r, Q)
            r = r / torch.linalg.vector_norm(r, dim=-1, keepdim=True)
            w = torch.where(bad.unsqueeze(-1), r, w / torch.where(bad, torch.ones_like(nrm), nrm).to(rdt).unsqueeze(-1))
            nrm = torch.where(bad, torch.zeros_like(nrm), nrm)
        else:
            w = w / nrm.to(rdt).unsqueeze(-1)
        smax = torch.where(live, torch.maximum(smax, nrm), smax)
        col = H[:, :, j].clone()
        col[:, :j + 1] = (c1 + c2).to(hdt)
        col[:, j + 1] = nrm.to(hdt)
        H[:, :, j] = torch.where(live.unsqueeze(-1), col, H[:, :, j])
        V[:, :, j + 1] = torch.where(live.unsqueeze(-1), w, V[:, :, j + 1])

    v0 = _arn_start_vector(A, V0, v_init, bdims, B, n, dtype, dev, rng_device)
    nv0 = torch.linalg.vector_norm(v0, dim=-1, keepdim=True)
    if bool((nv0 == 0).any()):
        raise RuntimeError("eigs: the start vector is zero")
    V[:, :, 0] = v0 / nv0
    niter, history, kept, done = 0, [], [], False
    kps = [0] * B                                   # vectors every member kept at its last restart
    for cycle in range(max_niter):
        niter = cycle + 1
        for j in range(min(kps), m):
            step(j, kps)
        Bm, beta = H[:, :m, :m], H[:, m, m - 1]
        theta, Yv = torch.linalg.eig(Bm)
        hfro = torch.linalg.matrix_norm(Bm).to(torch.float64)
        orders = [_arn_order(theta[b].to(torch.complex128), which, real_op) for b in range(B)]
        sel = torch.tensor([o[:neig] for o, _ in orders], dtype=torch.int64)
        th = torch.gather(theta, 1, sel)
        Ys = torch.gather(Yv, 2, sel.unsqueeze(1).expand(-1, m, -1))
        res = beta.abs().unsqueeze(-1) * Ys[:, m - 1, :].abs()
        bound = min_eps * torch.maximum(th.abs(), (u_round * hfro).unsqueeze(-1))
        nconv = (res <= bound).sum(dim=-1)
        history.append(nconv.tolist())
        if verbose:
            print("Cycle %3d (basis of %d): converged pairs per member %s" % (niter, m, nconv.tolist()))
        if bool((nconv >= neig).all()):
            done = True
            break
        if cycle + 1 == max_niter:
            break
        # restart: member b keeps its own keep' vectors (a conjugate pair of a real operator is never cut) and
        # continues from step keep'; `step` leaves the members that are ahead alone
        Vn = torch.zeros_like(V)
        Hn = torch.zeros_like(H)
        kps = []
        for b in range(B):
            order, partner = orders[b]
            kp = _arn_cut(order, partner, keep, m) if real_op else min(keep, m - 1)
            X = Yv[b][:, order[:kp]]
            if real_op:
                while True:
                    Uu, S_, _ = torch.linalg.svd(torch.cat([X.real, X.imag], dim=-1), full_matrices=False)
                    if kp >= m - 1 or not (S_.shape[0] > kp and float(S_[kp]) > ARN_CLOSED_TOL):
                        break
                    kp += 1                                        # the pairing misjudged: one more vector
                    X = Yv[b][:, order[:kp]]
                Qb = Uu[:, :kp].to(hdt)
            else:
                Qb, _ = torch.linalg.qr(X)
            kps.append(kp)
            Vn[b, :, :kp] = torch.matmul(V[b, :, :m], Qb.to(dtype))
            Vn[b, :, kp] = V[b, :, m]
            Hn[b, :kp, :kp] = _H(Qb) @ Bm[b] @ Qb
            Hn[b, kp, :kp] = beta[b] * Qb[m - 1, :]
        V, H = Vn, Hn
        kept.append(list(kps))
    # Ritz vectors, normalised, and the true residuals from one more apply
    X = torch.matmul(V[:, :, :m].to(cdt), Ys.to(cdt))
    X = X / torch.linalg.vector_norm(X, dim=-2, keepdim=True)
    lam = th.to(cdt)
    resid = _arn_true_residuals(apply_cols, X, lam, real_op)
    _arn_finish_report(resid, lam, hfro, u_round, min_eps, niter, done)
    if trace is not None:
        trace.update(niter=niter, restarts=niter - 1, napply=napply, ncv=ncv, keep=keep, converged_history=history,
                     breakdowns=breakdowns, host_reads=None, torch_applies=napply, converged=done,
                     resid=resid.reshape(*bdims, neig), panel_kernel="host", kept_history=kept)
    return lam.reshape(*bdims, neig), X.reshape(*bdims, n, neig)
