"""Float64 / complex128 restatement of xk_lobpcg_rotate (xk_lobpcg.hip) with a per-entry error bound.

    stack[b,c,n] <- sum_{a<k} C[b,a,c] * stack[b,a,n]                   c < q,  stack = S, MS, AS
    S[b,q+c,n]   <- AS'[b,c,n] - lam[b,c] * (MS ? MS' : S')[b,c,n]      c < w
    Pnorm[b,c,blk] = sum over column chunk blk of |S[b,q+c,n]|^2,   Pmax[b,blk] = max over the chunk and c of |S[b,q+c,n]|

In the manner of tests/cheb_ref.py: `rotate()` takes the very inputs the kernel is given (stacks and C of the kernel's
dtype, lam as the float64 table the kernel reads, rounded once to float by the 32-bit forms) and returns (value, bound)
per entry.  Complex data are handled through their real products on interleaved (re, im) storage.

Value.  Every sum is accumulated as an unevaluated pair hi + lo by error-free transformations (Veltkamp / Dekker
two-product, Knuth two-sum), exact to O(k u64^2) of the term sum: the reference carries no rounding error of its own
next to a float64 kernel.  `value` is hi and carries lo as the attribute `value.lo`, which `check()` subtracts.

Bound of a rotated entry: (n + 2) u sum_a |C_ac| |s_an| — the dot-product bound gamma_n (Higham, Accuracy and
Stability of Numerical Algorithms, section 3.1), valid for any summation order and for FMA contraction — with n = k
real terms (real dtypes) or 2 k (complex: moduli per real product), one more u in the 32-bit forms, and `tiny` once.
Bound of a residual entry: bound(AX') + |lam| bound(MX') + 3 u (|AX'| + |lam| |MX'|): it covers forming the residual
from the accumulators or from the stored values.  Pnorm: relative (N + 4) u64 plus the propagated entry bounds
sum (2 |r| b + b^2).  Pmax: between max(|r| - b) and max(|r| + b), a few u64 of slack for the modulus.

`fault=` plants plausible bugs (FAULTS); tests/test_lobpcg_ref.py shows that `check()` rejects each of them.
"""
from types import SimpleNamespace
import torch
from tests.cheb_ref import REAL_OF, unit_roundoff, as_real64, nan_of, _two_sum, _two_prod

FAULTS = ("C_transposed", "C_conjugated", "resid_old_X", "P_overwritten", "lam_wrong_column")
U64 = 2.0 ** -53


def chunk_elems(dtype):
    """elements of one column chunk = 256 vectors of 16 B (xk_lobpcg_blocks)"""
    return 256 * 16 // torch.empty((), dtype=dtype).element_size()


def rounded_lam(lam, dtype):
    lam = lam.detach().cpu().to(torch.float64)
    if REAL_OF[dtype] == torch.float32:
        return lam.to(torch.float32).to(torch.float64)
    return lam


def _planes(t):
    """(re, im or None) float64 planes of a host tensor of a kernel dtype"""
    t = t.detach().cpu()
    if t.is_complex():
        t = t.to(torch.complex128)
        return t.real.clone(), t.imag.clone()
    return t.to(torch.float64), None


class _DD:
    """an unevaluated sum hi + lo and the running sum of the terms' moduli"""

    def __init__(self, shape):
        self.hi, self.lo, self.mag = (torch.zeros(shape, dtype=torch.float64) for _ in range(3))

    def add_prod(self, a, b):
        p, e = _two_prod(a, b)
        self.hi, f = _two_sum(self.hi, p)
        self.lo = self.lo + (e + f)
        self.mag = self.mag + p.abs()


def _combine(Cre, Cim, sre, sim, k, q, single=False):
    """sum_{a<k} C[b,a,c] s[b,a,n] for c < q: ((re _DD, im _DD or None)); C planes (Bt, k, q), s planes (Bt, k, N).
    single: the data are floats — their products are exact in double, and a plain double sum of the <= 2 k of them is
    off by at most 2 k u64 of the moduli, 2^-29 of the float bound (which `rotate` widens by just that)."""
    Bt, N = sre.shape[0], sre.shape[2]
    if single:
        mm = lambda c, t: torch.einsum("bac,ban->bcn", c[:, :k, :q], t[:, :k])
        re = _DD((0,))
        re.hi, re.mag = mm(Cre, sre), mm(Cre.abs(), sre.abs())
        im = None
        if sim is not None:
            im = _DD((0,))
            re.hi, re.mag = re.hi - mm(Cim, sim), re.mag + mm(Cim.abs(), sim.abs())
            im.hi, im.mag = mm(Cre, sim) + mm(Cim, sre), mm(Cre.abs(), sim.abs()) + mm(Cim.abs(), sre.abs())
            im.lo = torch.zeros_like(im.hi)
        re.lo = torch.zeros_like(re.hi)
        return re, im
    re = _DD((Bt, q, N))
    im = _DD((Bt, q, N)) if sim is not None else None
    for a in range(k):
        cr = Cre[:, a, :q, None].expand(Bt, q, N)
        sr = sre[:, a, None, :].expand(Bt, q, N)
        re.add_prod(cr, sr)
        if sim is not None:
            ci = Cim[:, a, :q, None].expand(Bt, q, N)
            si = sim[:, a, None, :].expand(Bt, q, N)
            re.add_prod(-ci, si)
            im.add_prod(cr, si)
            im.add_prod(ci, sr)
    return re, im


def _interleave(re, im):
    if im is None:
        return re
    return torch.stack((re, im), dim=-1).reshape(*re.shape[:-1], 2 * re.shape[-1])


def rotate(S, AS, MS, C, lam, k, q, w, dtype, fault=None):
    """what xk_lobpcg_rotate must leave behind.  S, AS, MS (or None): (Bt, rows, N) host tensors of `dtype` (the
    first N elements of every row, no pads); C (Bt, >= k, >= q) of `dtype`; lam (Bt, >= w) float64.  Returns a namespace
    with, as float64 tensors on interleaved storage (n = N or 2 N):
      stacks: {"S" | "AS" | "MS": (value, bound)} of rows [0, q): (Bt, q, n)
      resid:  (value, bound) of rows [q, q + w) of S: (Bt, w, n)
      pnorm:  (value, bound) (Bt, w, nblk);   pmax: (lower, upper) (Bt, nblk)"""
    cplx = dtype.is_complex
    u = unit_roundoff(dtype)
    tiny = torch.finfo(REAL_OF[dtype]).tiny
    single = REAL_OF[dtype] == torch.float32
    nterm = (2 * k if cplx else k) + 2 + (1 if single else 0)
    Cre, Cim = _planes(C[:, :k, :q])
    if fault == "C_transposed":
        m = min(k, q)
        Cre = Cre.clone()
        Cre[:, :m, :m] = Cre[:, :m, :m].transpose(1, 2).clone()
        if cplx:
            Cim = Cim.clone()
            Cim[:, :m, :m] = Cim[:, :m, :m].transpose(1, 2).clone()
    if fault == "C_conjugated" and cplx:
        Cim = -Cim
    lamr = rounded_lam(lam, dtype)[:, :w]
    if fault == "lam_wrong_column":
        lamr = torch.roll(lamr, 1, dims=1)
    out = {}
    acc = {}
    for name, stack in (("S", S), ("MS", MS), ("AS", AS)):
        if stack is None:
            continue
        sre, sim = _planes(stack[:, :k])
        if fault == "P_overwritten" and q > w:
            # the X' rows are stored before the P' rows are formed: P' sees rows [0, w) already replaced
            re0, im0 = _combine(Cre, Cim, sre, sim, k, w, single)
            sre = sre.clone()
            sre[:, :w] = (re0.hi + re0.lo).to(REAL_OF[dtype]).to(torch.float64)
            if cplx:
                sim = sim.clone()
                sim[:, :w] = (im0.hi + im0.lo).to(REAL_OF[dtype]).to(torch.float64)
            re1, im1 = _combine(Cre, Cim, sre, sim, k, q, single)
            for d0, d1 in ((re0, re1), (im0, im1)):
                if d0 is not None:
                    d1.hi[:, :w], d1.lo[:, :w], d1.mag[:, :w] = d0.hi, d0.lo, d0.mag
            re, im = re1, im1
        else:
            re, im = _combine(Cre, Cim, sre, sim, k, q, single)
        value = _interleave(re.hi, im.hi if cplx else None)
        value.lo = _interleave(re.lo, im.lo if cplx else None)
        bound = (nterm * u + (4 * k * U64 if single else 0.0)) * _interleave(re.mag, im.mag if cplx else None) + tiny
        out[name] = (value, bound)
        acc[name] = (value, bound)
    # residual: AX' - lam * (MX' or X'), c < w
    kname = "MS" if MS is not None else "S"
    ax, bax = acc["AS"]
    mx, bmx = acc[kname]
    E = 2 if cplx else 1
    if fault == "resid_old_X":
        old = as_real64((MS if MS is not None else S)[:, :w])
        mx = old.clone()
        mx.lo = torch.zeros_like(old)
    lam_e = lamr[:, :, None]
    axh, axl = ax[:, :w], ax.lo[:, :w]
    mxh, mxl = mx[:, :w], mx.lo[:, :w]
    p, e = _two_prod(-lam_e.expand_as(mxh), mxh)
    r, f = _two_sum(axh, p)
    r.lo = (e + f) + (axl - lam_e * mxl)
    rb = bax[:, :w] + lam_e.abs() * bmx[:, :w] + 3.0 * u * (axh.abs() + lam_e.abs() * mxh.abs()) + tiny
    # partial sums and maxima per column chunk
    Bt, n = r.shape[0], r.shape[2]
    N = n // E
    ch = chunk_elems(dtype)
    nblk = -(-N // ch)
    rr = (r + r.lo).reshape(Bt, w, N, E)
    bb = rb.reshape(Bt, w, N, E)
    m2 = (rr * rr).sum(-1)                                               # |r|^2 per element
    mod = torch.sqrt(m2)
    bmod = bb.sum(-1)
    pn = torch.zeros((Bt, w, nblk), dtype=torch.float64)
    pnb = torch.zeros((Bt, w, nblk), dtype=torch.float64)
    plo = torch.zeros((Bt, nblk), dtype=torch.float64)
    phi = torch.zeros((Bt, nblk), dtype=torch.float64)
    for j in range(nblk):
        sl = slice(j * ch, min(N, (j + 1) * ch))
        pn[:, :, j] = m2[:, :, sl].sum(-1)
        prop = (2.0 * rr[:, :, sl].abs() * bb[:, :, sl] + bb[:, :, sl] ** 2).sum(dim=(-1, -2))
        pnb[:, :, j] = (N + 4) * U64 * pn[:, :, j] + prop + torch.finfo(torch.float64).tiny
        plo[:, j] = ((mod[:, :, sl] - bmod[:, :, sl]) * (1 - 8 * U64)).amax(dim=(1, 2)).clamp(min=0.0)
        phi[:, j] = ((mod[:, :, sl] + bmod[:, :, sl]) * (1 + 8 * U64)).amax(dim=(1, 2))
    return SimpleNamespace(stacks=out, resid=(r, rb), pnorm=(pn, pnb), pmax=(plo, phi), nblk=nblk)


def errors(got, value, bound):
    return ((as_real64(got) - value) - getattr(value, "lo", 0.0)).abs()


def check(got, value, bound, what=""):
    """every entry of `got` (a tensor of the kernel dtype, or float64 for the partial sums) within `bound` of `value`;
    returns the largest |err| / bound.  A NaN / Inf where the reference is finite fails."""
    err = errors(got, value, bound)
    assert err.shape == value.shape, "%s: shape %s vs %s" % (what, tuple(err.shape), tuple(value.shape))
    bad = ~(err <= bound)
    ratio = float((err / bound).nan_to_num(nan=float("inf")).max()) if err.numel() else 0.0
    assert not bool(bad.any()), "%s: %d entries outside the bound, worst |err| / bound = %.3g at %s" % (
        what, int(bad.sum()), ratio, tuple(torch.nonzero(bad)[0].tolist()))
    return ratio


def violates(got, value, bound):
    """number of entries of `got` outside the bound (for the planted faults)"""
    return int((~(errors(got, value, bound) <= bound)).sum())


def check_all(ref, S, AS, MS, Pnorm, Pmax, q, w, what=""):
    """the kernel's outputs (stacks after the call: host tensors (Bt, rows, N); Pnorm (Bt, w, nblk), Pmax (Bt, nblk)
    float64) against `ref`; returns the largest |err| / bound over everything"""
    worst = 0.0
    for name, stack in (("S", S), ("AS", AS), ("MS", MS)):
        if stack is not None:
            worst = max(worst, check(stack[:, :q], *ref.stacks[name], what="%s %s rows [0, q)" % (what, name)))
    worst = max(worst, check(S[:, q:q + w], *ref.resid, what="%s residual rows" % what))
    worst = max(worst, check(Pnorm.detach().cpu(), *ref.pnorm, what="%s Pnorm" % what))
    pm = Pmax.detach().cpu()
    lo, hi = ref.pmax
    assert bool(((pm >= lo) & (pm <= hi)).all()), "%s Pmax: %s outside [%s, %s]" % (what, pm, lo, hi)
    return worst


def emulate(S, AS, MS, C, lam, k, q, w, dtype, fault=None):
    """a stand-in for the kernel on the host: the reference (with `fault` planted) rounded to the storage type.
    Returns (S', AS', MS' of `dtype` with rows [0, q) replaced and the residual in rows [q, q + w) of S', Pnorm, Pmax)"""
    ref = rotate(S, AS, MS, C, lam, k, q, w, dtype, fault=fault)

    def back(v):
        v = (v + getattr(v, "lo", 0.0)).to(REAL_OF[dtype])
        if dtype.is_complex:
            return torch.view_as_complex(v.reshape(*v.shape[:-1], v.shape[-1] // 2, 2).contiguous())
        return v
    outs = []
    for name, stack in (("S", S), ("AS", AS), ("MS", MS)):
        if stack is None:
            outs.append(None)
            continue
        t = stack.clone()
        t[:, :q] = back(ref.stacks[name][0])
        if name == "S":
            t[:, q:q + w] = back(ref.resid[0])
        outs.append(t)
    lo, hi = ref.pmax
    return outs[0], outs[1], outs[2], ref.pnorm[0], 0.5 * (lo + hi)


def make_inputs(dtype, Bt, rows, N, k, q, w, seed, kind="randn", with_m=True):
    """(S, AS, MS or None, C, lam) on the host.  kinds as tests/cheb_ref.make_inputs: randn; graded (magnitudes of the
    stack rows spanning 1e+-30 in 64-bit, 1e+-15 in 32-bit forms); cancel (A S = lam M S up to 1e-6: the residual
    cancels); integer (integer-valued stacks, coefficients and lam: every result is exact).  C differs per member."""
    g = torch.Generator().manual_seed(seed)
    rd = REAL_OF[dtype]

    def rnd(*shape):
        t = torch.randn(shape, dtype=rd, generator=g)
        if dtype.is_complex:
            t = torch.complex(t, torch.randn(shape, dtype=rd, generator=g))
        return t

    def ints(lim, *shape):
        t = torch.randint(-lim, lim + 1, shape, generator=g).to(rd)
        if dtype.is_complex:
            t = torch.complex(t, torch.randint(-lim, lim + 1, shape, generator=g).to(rd))
        return t
    if kind == "integer":
        # |sum| <= 2 k 8 8 < 2^24 / 64: exact in every dtype, also after the product with lam
        S, AS, MS = ints(8, Bt, rows, N), ints(8, Bt, rows, N), ints(8, Bt, rows, N)
        C = ints(8, Bt, k, q)
        lam = torch.randint(-4, 5, (Bt, w), generator=g).to(torch.float64)
    else:
        S, AS, MS = rnd(Bt, rows, N), rnd(Bt, rows, N), rnd(Bt, rows, N)
        C = rnd(Bt, k, q) / max(1.0, k ** 0.5)
        lam = torch.randn((Bt, w), dtype=torch.float64, generator=g) * 3.0
        if kind == "graded":
            span = 30.0 if rd == torch.float64 else 15.0
            for t in (S, AS, MS):
                e = (torch.rand((Bt, rows, 1), dtype=torch.float64, generator=g) * 2.0 - 1.0) * span
                t.mul_((10.0 ** e).to(rd))
        elif kind == "cancel":
            lam = lam.abs() + 0.5
            lam[:] = lam[:, :1]                                   # one value per member: A S = lam M S row by row
            base = MS if with_m else S
            AS = (base * lam[:, :1, None].to(rd) * (1.0 + 1e-6 * rnd(Bt, rows, N).real)).to(dtype)
    return S.to(dtype), AS.to(dtype), (MS.to(dtype) if with_m else None), C.to(dtype), lam


__all__ = ["FAULTS", "rotate", "check", "check_all", "violates", "emulate", "make_inputs", "chunk_elems", "nan_of",
           "REAL_OF"]
