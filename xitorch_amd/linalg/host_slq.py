"""Stochastic Lanczos quadrature in host memory: the iteration of `native_slq.forms` in torch ops, for operators whose
tensors live on the CPU.  Device operators never reach `forms` (`calls` counts the entries; the GPU tests assert that
it stays 0).

The recurrence is the kernels' (xk_slq.hip): Lanczos on the un-normalised vectors r2 = beta_k v_k, all scalars float64
`(*batch, 1, p)`, no reorthogonalisation, a system frozen by masks when its new beta falls to `BREAK * eps * tnorm`
(tnorm: the running maximum row sum of the Jacobi matrix).  The quadrature is `torch.linalg.eigh` of the small matrix.

Shared with the native driver and the public functions: the argument checks (`check_options`), the probes
(`draw_probes`: drawn on the host from a generator of their own, the same numbers for a host and a device run) and the
sum over the nodes for a Python callable (`sum_nodes`, any device).

`funm` is the host twin of `native_fnm.funm`: f(A) B by two-pass Lanczos.  Pass 1 is `lanczos`; the coefficients of
f(A) b in the Lanczos basis come from `torch.linalg.eigh` of the small matrix (`eigvecs`, `coefficients`); `replay` runs
the recurrence again from the recorded scalars, by the expressions of `lanczos`, and accumulates X.
"""
import torch
from xitorch_amd._util import bcast_shape

__all__ = ["forms", "funm", "check_options", "draw_probes", "sum_nodes", "node_values", "calls", "FN_NAMES",
           "NEEDS_POSITIVE", "MAX_STEPS", "BREAK"]

calls = {"forms": 0, "funm": 0}
MAX_STEPS = 128                        # the projected matrix of xk_slq_quad lives on chip
BREAK = 64.0                           # SQ_BREAK of xk_slq.hip
FN_NAMES = ("log", "inv", "sqrt", "invsqrt", "exp", "identity")
NEEDS_POSITIVE = ("log", "inv", "sqrt", "invsqrt")


def _real_dtype(dtype):
    return {torch.complex128: torch.float64, torch.complex64: torch.float32}.get(dtype, dtype)


def check_options(who, A, fn, nsteps, options):
    """argument checks shared by quadform / trace_fn / logdet and both drivers; returns the options with their
    defaults: fn (a name of FN_NAMES or a callable), t, nsteps, dist, trace, verbose"""
    if not A.is_hermitian:
        raise RuntimeError("The linear operator A must be Hermitian")
    if A.shape[-1] != A.shape[-2]:
        raise RuntimeError("%s: the operator must be square, got %s" % (who, tuple(A.shape)))
    for name, what in (("M", "a metric M="), ("process_group", "batch sharding (process_group=)"),
                       ("precond", "a preconditioner (precond=)"), ("E", "a shift E=")):
        if options.get(name) is not None:
            raise NotImplementedError("%s: %s is not supported by the Lanczos quadrature" % (who, what))
    known = ("t", "dist", "trace", "verbose", "M", "process_group", "precond", "E")
    unknown = [k for k in options if k not in known]
    if unknown:
        raise TypeError("%s: unknown option(s) %s" % (who, ", ".join(sorted(unknown))))
    if not callable(fn) and fn not in FN_NAMES:
        raise ValueError("%s: fn must be one of %s or a callable, got %r" % (who, ", ".join(FN_NAMES), fn))
    n = A.shape[-1]
    if nsteps is None:
        nsteps = min(n, 50)
    if isinstance(nsteps, bool) or not isinstance(nsteps, int) or nsteps < 1:
        raise ValueError("%s: nsteps must be a positive int, got %r" % (who, nsteps))
    if nsteps > MAX_STEPS:
        raise ValueError("%s: nsteps = %d is beyond the %d steps whose projected matrix the quadrature kernel keeps on "
                         "chip" % (who, nsteps, MAX_STEPS))
    dist = options.get("dist") or "rademacher"
    if dist not in ("rademacher", "gaussian"):
        raise ValueError("%s: dist must be 'rademacher' or 'gaussian', got %r" % (who, dist))
    t = options.get("t")
    if t is not None and fn != "exp":
        raise TypeError("%s: the option t belongs to fn='exp'" % who)
    return dict(fn=fn, t=1.0 if t is None else float(t), nsteps=nsteps, dist=dist, trace=options.get("trace"),
                verbose=bool(options.get("verbose", False)))


def draw_probes(n, p, dtype, seed=0, dist="rademacher"):
    """(n, p) probes on the HOST from a generator of their own, seeded by `seed` (the global generators are left alone):
    the same numbers for a host run and a device run of one call.  Real entries also for a complex operator."""
    g = torch.Generator().manual_seed(int(seed))
    rd = _real_dtype(dtype)
    if dist == "rademacher":
        z = (torch.randint(0, 2, (n, p), generator=g, dtype=torch.int64) * 2 - 1).to(rd)
    else:
        z = torch.randn((n, p), dtype=rd, generator=g)
    return z.to(dtype)


def named_fn(name, t=1.0):
    """the torch expression of a named function (what xk_slq_quad sums inside the kernel)"""
    return {"log": torch.log, "inv": torch.reciprocal, "sqrt": torch.sqrt, "invsqrt": torch.rsqrt,
            "exp": lambda x: torch.exp(t * x), "identity": lambda x: x}[name]


def sum_nodes(theta, weight, m, zz, fn):
    """|z|^2 sum_k weight_k fn(theta_k) over the first m_s nodes of every system, in torch on the arrays' device.
    theta, weight: (S, nsteps); m, zz: (S,).  `fn` sees an (S, nsteps) array whose unused entries repeat the system's
    first node (1 for a system without nodes), so that it is evaluated on numbers of its domain only."""
    ns = theta.shape[-1]
    used = torch.arange(ns, device=theta.device)[None, :] < m[:, None]
    first = torch.where(m[:, None] > 0, theta[:, :1], torch.ones_like(theta[:, :1]))
    f = fn(torch.where(used, theta, first))
    if not isinstance(f, torch.Tensor) or f.shape != theta.shape:
        raise RuntimeError("trace_fn: a callable fn must map an (S, m) tensor to a tensor of the same shape")
    return zz * torch.where(used, weight * f.to(torch.float64), torch.zeros_like(weight)).sum(-1)


def lanczos(A, Z, nsteps, bdims):
    """nsteps Lanczos steps on every column of Z (*bdims, n, p).  Returns Tal, Tbe (*bdims, p, nsteps) float64, the step
    counts m and |z|^2 (*bdims, p) and the number of operator applies."""
    f64 = torch.float64
    rdt = _real_dtype(Z.dtype)
    eps = torch.finfo(rdt).eps
    sc = lambda s: s.to(rdt)
    dot = lambda x, y: (x.conj() * y).sum(-2, keepdim=True).real.to(f64)
    r2, r1 = Z.clone(), torch.zeros_like(Z)
    zz = dot(Z, Z)
    beta = torch.sqrt(zz)
    oldb = torch.zeros_like(beta)
    frozen = zz == 0
    m = torch.zeros_like(beta)
    tnorm, rowp = torch.zeros_like(beta), torch.zeros_like(beta)
    p = Z.shape[-1]
    Tal = torch.zeros((*bdims, p, nsteps), dtype=f64, device=Z.device)
    Tbe = torch.zeros_like(Tal)
    one = torch.ones_like(beta)
    napply = 0
    for k in range(nsteps):
        if bool(frozen.all()):
            break
        W = A.mm(r2)
        napply += 1
        first = k == 0
        if not first:
            oldb = torch.where(frozen, oldb, beta)
            bnew = torch.sqrt(dot(r2, r2))
            tn = torch.maximum(tnorm, rowp + bnew)
            brk = ~frozen & (bnew <= BREAK * eps * tn)
            tnorm = torch.where(frozen, tnorm, tn)
            frozen = frozen | brk
            beta = torch.where(frozen, beta, bnew)
        live = ~frozen
        sb = torch.where(live, beta, one)
        alpha = dot(r2, W) / (sb * sb)
        y = W * sc(1.0 / sb) - sc(alpha / sb) * r2
        if not first:
            y = y - sc(sb / torch.where(live, oldb, one)) * r1
        r1, r2 = torch.where(live, r2, r1), torch.where(live, y, r2)           # y over r1 and the swap, running systems
        lv = live.squeeze(-2)
        Tal[..., k] = torch.where(lv, alpha.squeeze(-2), Tal[..., k])
        Tbe[..., k] = torch.where(lv, beta.squeeze(-2), Tbe[..., k])
        rowp = torch.where(live, alpha.abs() + (0.0 if first else 1.0) * beta, rowp)
        m = torch.where(live, m + 1, m)
    return Tal, Tbe, m.squeeze(-2), zz.squeeze(-2), napply


def quadrature(Tal, Tbe, m):
    """nodes and weights of every system's m_s x m_s Jacobi matrix by torch.linalg.eigh.  Tal, Tbe: (S, nsteps), m: (S,)
    -> theta, weight (S, nsteps), entries [m_s, nsteps) zero."""
    theta, weight = torch.zeros_like(Tal), torch.zeros_like(Tal)
    for mv in torch.unique(m).tolist():
        mv = int(mv)
        if mv == 0:
            continue
        idx = (m == mv).nonzero().squeeze(-1)
        T = torch.diag_embed(Tal[idx, :mv])
        if mv > 1:
            off = Tbe[idx, 1:mv]
            T = T + torch.diag_embed(off, offset=1) + torch.diag_embed(off, offset=-1)
        ev, V = torch.linalg.eigh(T)
        theta[idx, :mv] = ev
        weight[idx, :mv] = V[:, 0, :] ** 2
    return theta, weight


def forms(A, Z, opt):
    """z_j^H f(A) z_j for every column of Z (*BZ, n, p) in host memory.  Returns the forms (*BAZ, p) in float64, a bool
    array of the same shape (a node <= 0 under a function that needs positivity: the form is NaN), the step counts
    and the number of operator applies."""
    calls["forms"] += 1
    if torch.device(A.device).type != "cpu":
        raise RuntimeError("host_slq serves operators in host memory only (operator is on %s)" % (A.device,))
    n = A.shape[-1]
    bdims = list(bcast_shape(A.shape[:-2], Z.shape[:-2]))
    p = Z.shape[-1]
    Zb = Z.to(A.dtype).expand(*bdims, n, p)
    Tal, Tbe, m, zz, napply = lanczos(A, Zb, opt["nsteps"], bdims)
    ns = Tal.shape[-1]
    theta, weight = quadrature(Tal.reshape(-1, ns), Tbe.reshape(-1, ns), m.reshape(-1))
    mf, zf = m.reshape(-1), zz.reshape(-1)
    fn = opt["fn"]
    bad = torch.zeros_like(mf, dtype=torch.bool)
    if callable(fn):
        q = sum_nodes(theta, weight, mf, zf, fn)
    else:
        if fn in NEEDS_POSITIVE:
            used = torch.arange(ns)[None, :] < mf[:, None]
            bad = (used & ~(theta > 0)).any(-1)
            theta = torch.where(used & (theta > 0), theta, torch.ones_like(theta))
        q = sum_nodes(theta, weight, mf, zf, named_fn(fn, opt["t"]))
        q = torch.where(bad, torch.full_like(q, float("nan")), q)
    return q.reshape(*bdims, p), bad.reshape(*bdims, p), m.to(torch.int64), napply


# ------------------------------------------------------------------------------------------------ f(A) B, two passes
def node_values(theta, m, fn, cplx, who="funm_multiply"):
    """a callable `fn` on the nodes, in torch on the arrays' device: (S, nsteps) float64, or complex128 with `cplx`,
    zero beyond m_s.  As in `sum_nodes`, the unused entries `fn` sees repeat the system's first node (1 for a system
    without nodes).  A complex result on a real operator is refused."""
    ns = theta.shape[-1]
    used = torch.arange(ns, device=theta.device)[None, :] < m[:, None]
    first = torch.where(m[:, None] > 0, theta[:, :1], torch.ones_like(theta[:, :1]))
    f = fn(torch.where(used, theta, first))
    if not isinstance(f, torch.Tensor) or f.shape != theta.shape:
        raise RuntimeError("%s: a callable fn must map an (S, m) tensor to a tensor of the same shape" % who)
    if f.is_complex() and not cplx:
        raise RuntimeError("%s: fn returned complex values on a real operator; cast A to a complex dtype to apply a "
                           "complex function" % who)
    f = f.to(torch.complex128 if cplx else torch.float64)
    return torch.where(used, f, torch.zeros_like(f))


def eigvecs(Tal, Tbe, m):
    """eigenvalues theta (S, nsteps) and eigenvectors Q (S, nsteps, nsteps), Q[s, j, k] = component j of eigenvector k,
    of every system's m_s x m_s Jacobi matrix by torch.linalg.eigh; entries at and beyond m_s are zero"""
    S, ns = Tal.shape
    theta = torch.zeros_like(Tal)
    Q = torch.zeros((S, ns, ns), dtype=Tal.dtype, device=Tal.device)
    for mv in torch.unique(m).tolist():
        mv = int(mv)
        if mv == 0:
            continue
        idx = (m == mv).nonzero().squeeze(-1)
        T = torch.diag_embed(Tal[idx, :mv])
        if mv > 1:
            off = Tbe[idx, 1:mv]
            T = T + torch.diag_embed(off, offset=1) + torch.diag_embed(off, offset=-1)
        ev, V = torch.linalg.eigh(T)
        theta[idx, :mv] = ev
        Q[idx[:, None, None], torch.arange(mv)[None, :, None], torch.arange(mv)[None, None, :]] = V
    return theta, Q


def coefficients(Q, f, m, zz):
    """C[s, j] = |b_s| sum_k Q[s, j, k] f[s, k] Q[s, 0, k] and tail[s] = |C[s, m-4:m]| / |C[s, :m]| (0 when m <= 4)"""
    C = torch.sqrt(zz)[:, None] * torch.einsum("sjk,sk->sj", Q.to(f.dtype), f * Q[:, 0, :])
    ar = torch.arange(C.shape[-1], device=C.device)[None, :]
    a2 = C.abs() ** 2
    last4 = torch.where((ar >= m[:, None] - 4) & (ar < m[:, None]), a2, torch.zeros_like(a2)).sum(-1)
    tail = torch.where(m > 4, torch.sqrt(last4 / a2.sum(-1)), torch.zeros_like(last4))
    return C, tail


def replay(A, Z, Tal, Tbe, m, zz, C):
    """pass 2: the recurrence of `lanczos` once more from the recorded Tal, Tbe (*bdims, p, nsteps), accumulating
    X = sum_k (C[..., k] / beta_k) r2_k.  Every expression that forms a vector is the one of `lanczos`, so the vectors
    are the same bits.  Returns X and the number of operator applies."""
    rdt = _real_dtype(Z.dtype)
    sc = lambda s: s.to(rdt)
    r2, r1 = Z.clone(), torch.zeros_like(Z)
    X = torch.zeros_like(Z)
    mk, nz = m.unsqueeze(-2), (zz != 0).unsqueeze(-2)
    one = torch.ones_like(zz).unsqueeze(-2)
    kmax = int(m.max()) if m.numel() else 0
    napply = 0
    for k in range(kmax):
        live = nz & (mk > k)
        alpha, beta = Tal[..., k].unsqueeze(-2), Tbe[..., k].unsqueeze(-2)
        sb = torch.where(live, beta, one)
        X = torch.where(live, X + (C[..., k].unsqueeze(-2) / sb).to(Z.dtype) * r2, X)
        if k + 1 == kmax:                                                      # the last step needs no product
            break
        W = A.mm(r2)
        napply += 1
        y = W * sc(1.0 / sb) - sc(alpha / sb) * r2
        if k > 0:
            y = y - sc(sb / torch.where(live, Tbe[..., k - 1].unsqueeze(-2), one)) * r1
        r1, r2 = torch.where(live, r2, r1), torch.where(live, y, r2)
    return X, napply


def funm(A, B, opt):
    """f(A) b_j for every column of B (*BB, n, p) in host memory.  Returns X (*BAB, n, p), the flags (*BAB, p) of
    native_fnm.funm (int64; here only bit 0: a node <= 0 under a function that needs positivity, the column is NaN; eigh
    has no non-convergence flag), the step counts, the tails (*BAB, p) and the
    number of operator applies."""
    calls["funm"] += 1
    if torch.device(A.device).type != "cpu":
        raise RuntimeError("host_slq serves operators in host memory only (operator is on %s)" % (A.device,))
    n, p = A.shape[-1], B.shape[-1]
    bdims = list(bcast_shape(A.shape[:-2], B.shape[:-2]))
    Bb = B.to(A.dtype).expand(*bdims, n, p)
    Tal, Tbe, m, zz, napply = lanczos(A, Bb, opt["nsteps"], bdims)
    ns = Tal.shape[-1]
    mf, zf = m.reshape(-1), zz.reshape(-1)
    theta, Q = eigvecs(Tal.reshape(-1, ns), Tbe.reshape(-1, ns), mf)
    fn, cplx = opt["fn"], A.dtype.is_complex
    bad = torch.zeros_like(mf, dtype=torch.bool)
    if callable(fn):
        f = node_values(theta, mf, fn, cplx)
    else:
        if fn in NEEDS_POSITIVE:
            used = torch.arange(ns)[None, :] < mf[:, None]
            bad = (used & ~(theta > 0)).any(-1)
            theta = torch.where(used & (theta > 0), theta, torch.ones_like(theta))
        f = node_values(theta, mf, named_fn(fn, opt["t"]), cplx)
    C, tail = coefficients(Q, f, mf, zf)
    C = torch.where(bad[:, None], torch.full_like(C, float("nan")), C)
    X, nap2 = replay(A, Bb, Tal, Tbe, m, zz, C.reshape(*bdims, p, ns))
    return X, bad.to(torch.int64).reshape(*bdims, p), m.to(torch.int64), tail.reshape(*bdims, p), napply + nap2
