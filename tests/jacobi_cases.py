"""Test matrices for the Jacobi eigensolver (K3) whose spectrum is known exactly (host, torch CPU only).

Sylvester-Hadamard similarity: for n = 2^j, T = H diag(d) H / n has the eigenvalues d and the eigenvectors H / sqrt(n).
With d made of dyadic rationals of few bits every entry of T is an exact float, so T is bitwise symmetric, survives
the rounding to the test dtype unchanged, and the reference spectrum carries no error at all.  Other orders: a
block-diagonal of Hadamard blocks over the binary decomposition of k (45 = 32 + 8 + 4 + 1) on consecutive slices of
d, under one fixed symmetric permutation that interleaves the blocks.

A case is (T, d, H, n), all float64: the matrix, its eigenvalues in construction order, and the eigenvectors as the
columns of H / sqrt(n) (H holds +-1 / 0 for the Hadamard kinds, n the block order of each column), so that the
projector on a set S of them, (H_S / n_S) H_S^T, is exact too.  Besides the families: the trivial matrices (zero, 3 I,
an unsorted repeated diagonal, the second-difference tridiagonal), `generic` dense ones for a LAPACK reference, and
`hidden`, where the early exit of the kernel meets an extreme eigenvalue that no diagonal entry shows yet.
"""
import collections
import decimal
import math
import torch

F64 = torch.float64
Case = collections.namedtuple("Case", "T d H n")

HADAMARD = ("spread", "multiple", "cluster", "edgegap")
TRIVIAL = ("zero", "identity3", "diagonal", "tridiagonal")
FAMILIES = HADAMARD + TRIVIAL

# every workgroup-size (256 / 512 / 768 / 1024 threads) and blocks-per-thread (1 .. 4) boundary of the kernel with its
# odd neighbour (odd orders get a dummy player), the smallest orders, the largest
ORDERS = (1, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33, 44, 45, 54, 55, 64, 65, 90, 91, 110, 111, 127, 128)
SCALE_ORDERS = (5, 40, 128)
SCALE_EXPONENTS = {torch.float32: (40, -40, 100, -100), F64: (400, -400, 520, -520, 900, -900)}
BATCH70_ORDER = 91

# Worst error of CPU LAPACK (eigh in the test dtype) on these very matrices, in the units below, as measured by
# test_jacobi_cases.py (which asserts that they still hold): the yardstick the kernel's bounds are multiples of.
# Measured, float64 / float32: lam 0.625 / 0.601, res 0.75 / 0.619, orth 2.667 / 1.694, proj 0.667 / 0.5.  Another
# LAPACK build rounds differently, so each figure is taken up to the next quarter above it.
LAPACK_RATIO = {
    "lam": {F64: 0.75, torch.float32: 0.75},
    "res": {F64: 1.0, torch.float32: 0.75},
    "orth": {F64: 2.75, torch.float32: 1.75},
    "proj": {F64: 0.75, torch.float32: 0.75},
}
# K3 applies about one orthogonal similarity per sweep, typically 8 sweeps, where LAPACK applies one reduction
KERNEL_FACTOR = 8.0


def bound_factor(what, dtype):
    """c of the kernel's bounds  c * k * u * ...  for the quantity `what`"""
    return KERNEL_FACTOR * LAPACK_RATIO[what][dtype]


def unit_roundoff(dtype):
    return torch.finfo(dtype).eps / 2


def cluster_bits(dtype):
    """cluster spacing 2^-bits at which T stays exact up to order 128 (2^-12 already fails in float32)"""
    return 30 if dtype == F64 else 8


def wanted_counts(k):
    """the numbers of wanted pairs tried at order k: 1, 6, min(k, 16) (which is k itself up to order 16)"""
    return sorted({p for p in (1, 6, min(k, 16)) if p <= k})


def hadamard(n):
    H = torch.ones(1, 1, dtype=F64)
    while H.shape[0] < n:
        H = torch.cat([torch.cat([H, H], 1), torch.cat([H, -H], 1)], 0)
    assert H.shape[0] == n, "order %d is no power of two" % n
    return H


def blocks(k):
    """binary decomposition of k, largest first: 45 -> [32, 8, 4, 1]"""
    return [1 << j for j in range(k.bit_length() - 1, -1, -1) if k >> j & 1]


def interleave(k):
    """one fixed permutation of 0 .. k-1 that spreads every block over the whole index range: i -> i * s mod k with
    s the first integer from 0.618 k on that is coprime to k"""
    s = max(1, int(0.618 * k))
    while math.gcd(s, k) != 1:
        s += 1
    return (torch.arange(k) * s) % k


_PI = decimal.Decimal("3.14159265358979323846264338327950288419716939937510582097494")


def _sin_dec(x):
    """sin of a Decimal in [0, pi/2] by its Taylor series, 50 digits"""
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        term, total, n = x, x, 1
        while abs(term) > decimal.Decimal(10) ** -45:
            term = -term * x * x / ((n + 1) * (n + 2))
            total += term
            n += 2
        return total


def spectrum(family, k, dtype):
    j = torch.arange(k, dtype=F64)
    h = 2.0 ** -cluster_bits(dtype)
    if family == "spread":
        return j - k // 2
    if family == "multiple":                    # exact triple eigenvalues; one straddles the boundary for p % 3 != 0
        return torch.floor(j / 3)
    if family == "cluster":
        return torch.where(j < 4, 1 + j * h, 2 + j)
    if family == "edgegap":                     # p = 6: the first unwanted eigenvalue sits h above the wanted ones
        return torch.where(j < 6, torch.ones_like(j), torch.where(j == 6, torch.full_like(j, 1 + h), 3 + j))
    raise ValueError(family)


def case(family, k, dtype, shift=0.0):
    """Case of the family at order k, exact in `dtype`; `shift` is added to every eigenvalue (T + shift I)"""
    eye = torch.eye(k, dtype=F64)
    if family == "zero":
        d = torch.zeros(k, dtype=F64) + shift
        return Case(torch.diag(d), d, eye, torch.ones(k, dtype=F64))
    if family == "identity3":
        d = torch.full((k,), 3.0, dtype=F64) + shift
        return Case(torch.diag(d), d, eye, torch.ones(k, dtype=F64))
    if family == "diagonal":                    # repeated entries, not sorted
        d = ((torch.arange(k) * 5) % 7).to(F64) - 3 + shift
        return Case(torch.diag(d), d, eye, torch.ones(k, dtype=F64))
    if family == "tridiagonal":
        # second-difference matrix: lambda_j = 2 - 2 cos(j pi / (k+1)) = 4 sin^2(j pi / (2k+2)), vectors sin(i j pi / (k+1)).
        # The eigenvalues are evaluated in 50-digit decimal arithmetic and rounded once (error <= u |lambda|, 1/k of the
        # unit they are compared in); the vectors, which only the projector check reads, in float64.
        T = 2 * eye - torch.diag(torch.ones(k - 1, dtype=F64), 1) - torch.diag(torch.ones(k - 1, dtype=F64), -1)
        j = torch.arange(1, k + 1, dtype=F64)
        d = torch.tensor([float(4 * _sin_dec(_PI * i / (2 * k + 2)) ** 2 + decimal.Decimal(shift))
                          for i in range(1, k + 1)], dtype=F64)
        H = torch.sin(j[:, None] * j[None, :] * math.pi / (k + 1)) * math.sqrt(2.0 / (k + 1))
        return Case(T + shift * eye, d, H, torch.ones(k, dtype=F64))
    d = spectrum(family, k, dtype) + shift
    T = torch.zeros(k, k, dtype=F64)
    H = torch.zeros(k, k, dtype=F64)
    n = torch.ones(k, dtype=F64)
    at = 0
    for nb in blocks(k):
        Hb = hadamard(nb)
        sl = slice(at, at + nb)
        T[sl, sl] = (Hb * d[sl]) @ Hb / nb
        H[sl, sl] = Hb
        n[sl] = nb
        at += nb
    perm = interleave(k)
    return Case(T[perm][:, perm], d, H[perm], n)


HIDDEN_BLOCKS = (8, 32, 64)
HIDDEN_P = 6


def hidden(nb, dtype, uppest=False):
    """Order 6 + nb: six decoupled rows holding the eigenvalue 1 exactly, beside one dense Hadamard block of order nb
    with the spectrum {1 - h, 34, 35, ...}, interleaved.  Every diagonal entry of the block is a Rayleigh quotient
    >= 1 - h, and exceeds 1 until the block's lowest vector is resolved to sqrt(h / 33): after the first sweeps the
    six lowest diagonal entries are the decoupled 1s, their rows carry no off-diagonal mass at all, and the lowest
    eigenvalue is still hidden in the block.  With p = 6 only the Gershgorin certificate of the unwanted rows keeps the
    early exit from returning six 1s (an error of h, against a bound of order k u).  uppest: the negated matrix."""
    h = 2.0 ** -cluster_bits(dtype)
    k = HIDDEN_P + nb
    d = torch.cat([torch.ones(HIDDEN_P, dtype=F64), torch.tensor([1 - h], dtype=F64),
                   33 + torch.arange(1, nb, dtype=F64)])
    if uppest:
        d = -d
    Hb = hadamard(nb)
    T = torch.diag(d)
    T[HIDDEN_P:, HIDDEN_P:] = (Hb * d[HIDDEN_P:]) @ Hb / nb
    H = torch.eye(k, dtype=F64)
    H[HIDDEN_P:, HIDDEN_P:] = Hb
    n = torch.cat([torch.ones(HIDDEN_P, dtype=F64), torch.full((nb,), float(nb), dtype=F64)])
    perm = interleave(k)
    return Case(T[perm][:, perm], d, H[perm], n)


def wanted(d, p, uppest):
    """indices (into d) of the p lowest / uppermost eigenvalues, ascending (ties by index), the sorted spectrum, and
    the gap between the wanted and the unwanted ones (inf when p == k)"""
    k = d.numel()
    ds, order = torch.sort(d, stable=True)
    sl = slice(k - p, k) if uppest else slice(0, p)
    if p == k:
        gap = math.inf
    else:
        gap = float(ds[k - p] - ds[k - p - 1]) if uppest else float(ds[p] - ds[p - 1])
    return order[sl], ds[sl], gap


def projector(c, idx):
    """exact orthogonal projector on the eigenvectors idx of the case"""
    Hs = c.H[:, idx]
    return (Hs / c.n[idx]) @ Hs.T


def generic(B, k, dtype, seed):
    """(R + R^T) / 2 without a diagonal shift, rounded to `dtype` (float64 values): reference = float64 LAPACK on it"""
    g = torch.Generator().manual_seed(seed)
    R = torch.randn(B, k, k, dtype=F64, generator=g)
    return ((R + R.transpose(-2, -1)) * 0.5).to(dtype).double()


def batch70(k, dtype):
    """70 distinct members: the eight families under nine shifts of the spectrum (0, 4, .. 32)"""
    return [case(FAMILIES[i % len(FAMILIES)], k, dtype, shift=4.0 * (i // len(FAMILIES))) for i in range(70)]


def ratios(T, lam, Y, c, p, uppest, dtype):
    """Errors of p computed eigenpairs (lam (p,), Y (p, k) rows, float64 copies) of the case c, whose matrix was handed
    over as T (float64), each in its unit:
      lam   max |lam - d_sorted|                     / (k u max(|d|_inf, 1))
      res   max |T y - lam y|                        / (k u max(|d|_inf, 1))
      orth  max |Y Y^T - I|                          / (k u)
      proj  max |Y^T Y - exact projector|            / (k u max(|d|_inf, 1) / gap)   (None without a gap, or for p = k)
    """
    k = T.shape[-1]
    ku = k * unit_roundoff(dtype)
    idx, dw, gap = wanted(c.d, p, uppest)
    nd = max(float(c.d.abs().max()), 1.0)
    out = {"lam": float((lam - dw).abs().max()) / (ku * nd),
           "res": float((Y @ T - lam[:, None] * Y).abs().max()) / (ku * nd),
           "orth": float((Y @ Y.T - torch.eye(p, dtype=F64)).abs().max()) / ku,
           "proj": None}
    if p < k and gap > 0:
        out["proj"] = float((Y.T @ Y - projector(c, idx)).abs().max()) / (ku * nd / gap)
    return out
