"""Exact-spectrum cases for the Ritz eigensolvers K3t (xk_small_eigh_tri_*) and K3g (xk_small_eigh_big_*, every
form): the families of jacobi_cases.py carried to order 1536, plus `multiple64` (host, torch CPU only; the wanted
counts and the batch-crossing p come from the library's own host functions).

The construction is that of jacobi_cases.py (Sylvester-Hadamard similarity, block-diagonal over the binary
decomposition of k, one interleaving permutation).  An entry of H diag(d) H / n is a multiple of 2^-bits / n of
magnitude <= max|d|, so it needs log2(n max|d|) + bits mantissa bits: float64 holds the 30-bit clusters of the Jacobi
cases up to order 1536 (10 + 11 + 30 = 51 bits), float32 does not beyond order 128.  There `cluster` and `edgegap`
get a spectrum of bounded magnitude for the unwanted part (64 distinct dyadic values in [2, 6) / [3, 7), repeated) and
a spacing 2^-cluster_bits(k, dtype) of 2^-12 .. 2^-11.  The generator proves exactness instead of trusting it: every
partial sum of the product is an integer multiple of one power of two below 2^53, and the result must be bitwise
symmetric and survive the rounding to the test dtype.

Yardstick: LAPACK's ?syevx in the test dtype on these very matrices (the same algorithm the kernels implement:
Householder tridiagonalisation, bisection, inverse iteration), measured by test_ritz_cases.py in the units of
jacobi_cases.ratios, per dtype and per band of orders.  The kernels' bounds are FACTOR[form] x EVX_RATIO.
"""
import functools
import math
import torch
from tests import jacobi_cases as jc

F64 = torch.float64
F32 = torch.float32
Case = jc.Case

FAMILIES = jc.FAMILIES + ("multiple64",)
HADAMARD = jc.HADAMARD + ("multiple64",)
FORMS = ("tri", "step", "persist", "two_stage", "auto")
ALGO = {"step": 1, "two_stage": 2, "persist": 3, "auto": 0}        # the `algo` argument of xk_small_eigh_big_*

# One orthogonal reduction like LAPACK's: the margin of 4 covers the other summation order (wave tree reductions) and
# the Newton-refined reciprocal / rsqrt in place of divisions.  The two-stage form applies two reductions and two
# back-transformations (8); `auto` may pick it.
FACTOR = {"tri": 4.0, "step": 4.0, "persist": 4.0, "two_stage": 8.0, "auto": 8.0}

# Worst error of ?syevx (scipy.linalg.eigh(driver="evx") in the test dtype) on the calibration cases below, per band
# of orders (<= 128, 129 .. 512, 513 .. 1536), each measured figure taken up to the next quarter.  Asserted by
# test_ritz_cases.py::test_syevx_ratios_in_the_test_dtype.  Measured:
#   float64  lam 1.0 / 0.0454 / 0.0145   res 1.0 / 0.0454 / 0.0102   orth 2.823 / 0.9341 / 0.1543   proj 1.0 / 0.0008 / 0.0035
#   float32  lam 1.0 / 0.0358 / 0.0145   res 0.7071 / 0.0354 / 0.0061   orth 2.9398 / 0.718 / 0.2431   proj 0.3034 / 0.0008 / 0.0007
# (the figures of 1.0 are one unit in the last place at order 2, where k u is one such unit)
EVX_RATIO = {
    "lam": {F64: (1.0, 0.25, 0.25), F32: (1.0, 0.25, 0.25)},
    "res": {F64: (1.0, 0.25, 0.25), F32: (0.75, 0.25, 0.25)},
    "orth": {F64: (3.0, 1.0, 0.25), F32: (3.0, 0.75, 0.25)},
    "proj": {F64: (1.0, 0.25, 0.25), F32: (0.5, 0.25, 0.25)},
}

# One call of the yardstick is left out of it: on `multiple` at order 15 (blocks 8 + 4 + 2 + 1, a triple eigenvalue
# inside the block of 8), p = 6 lowest, dsyevx returns vectors that are orthogonal to 616 k u only (res 12.5, proj 52):
# dstein reorthogonalises within clusters of the computed eigenvalues only.  Taking that figure in would put every
# float64 bound up to order 128 at thousands of k u; leaving it out holds the kernels, which orthogonalise against all
# earlier vectors, to the stricter bound of the other 1119 calls.  The next-worst orth of that band is 2.82.
EVX_OUTLIERS = {("float64", "multiple", 15, 6, False)}

# (form, dtype name) -> reason, for forms whose self-check flags `multiple64` by design.  multiple64 only.
XFLAG = {}

PROJ_UNIT_MAX = 0.125       # proj is not asserted where its unit k u |d| / gap reaches this: the bound would be vacuous


def band(k):
    return 0 if k <= 128 else (1 if k <= 512 else 2)


def bound(form, what, dtype, k):
    """c of the kernel's bound  c k u ...  for the quantity `what` at order k"""
    return FACTOR[form] * EVX_RATIO[what][dtype][band(k)]


def _esize(dtype):
    return 8 if dtype == F64 else 4


def _fn(name):
    from xitorch_amd._capi import fn
    return fn(name)


def tri_ok(k, p, dtype):
    from xitorch_amd import kernels as K
    return K.small_eigh_tri_ok(k, p, dtype)


def big_ok(k, p, dtype):
    from xitorch_amd import kernels as K
    return K.small_eigh_big_ok(k, p, dtype)


# ---------------------------------------------------------------------------------------------------- orders
# Every boundary the form has, read from its code:
#   tri        one workgroup, lanes l and l + 64 (65), the LDS pitch n | 1, the largest order
#   step       column slots 2 / 4 / 8 / 12 / 16 / 24 of the step kernel (trailing order 128 / 256 / 512 / 768 / 1024) and
#              2 / 4 / 6 / 8 / 12 / 16 / 24 of the final kernel; 1025 = 2^10 + 1 leaves a decoupled 1 x 1 block
#   persist    register limit 256 (float64) / 384 (float32): one beyond it and 128 beyond it are hand-over orders, which
#              start with step launches
#   two_stage  35 is the smallest order; the 16-column panel (47 .. 49, 63 .. 65) and the 64-row strip (191 .. 193, 257);
#              614 is the largest float64 order whose band fits the LDS
#   auto       the choice between the forms: 192 (two-stage from here), persistent limit + 64 (B > 8) / + 128 (B <= 8)
_TWO_STAGE_MAX = {F64: 614, F32: 1024}
TWO_STAGE_REFUSED = (615, F64)


def orders(form, dtype):
    if form == "tri":
        return (1, 2, 3, 7, 15, 16, 17, 33, 64, 65, 108, 127, 128)
    if form == "step":
        return (8, 9, 63, 64, 65, 128, 129, 256, 257, 512, 513, 768, 769, 1024, 1025) + ((1536,) if dtype == F64 else (1500,))
    if form == "persist":
        return (8, 64, 129, 255, 256, 257, 384) + (() if dtype == F64 else (385, 512))
    if form == "two_stage":
        ks = (35, 36, 47, 48, 49, 63, 64, 65, 191, 192, 193, 257, 614, 1000, 1024)
        return tuple(k for k in ks if k <= _TWO_STAGE_MAX[dtype] and (k != 614 or dtype == F64))
    if form == "auto":
        return (191, 192, 193, 320, 321, 385)
    raise ValueError(form)


def handover_orders(dtype):
    """orders of `persist` beyond the register limit: the first steps are step launches (wg matters there)"""
    return (257, 384) if dtype == F64 else (385, 512)


HANDOVER_WG = (0, 3, 8)
WIDE_ORDERS = {"step": (64, 513), "persist": (64, 257), "two_stage": (48, 257), "auto": (192, 321)}   # p = min(k, 256)
BATCH70_ORDER = {"tri": 91, "step": 150, "persist": 150, "two_stage": 150, "auto": 150}
GENERIC_ORDERS = {"tri": (17, 65, 128), "step": (129, 513, 1025), "persist": (129, 257, 384),
                  "two_stage": (49, 193, 614), "auto": (193, 321, 385)}
EQUAL_BITS_ORDERS = {"tri": {F64: (17, 128), F32: (17, 128)}, "step": {F64: (65, 257), F32: (65, 257)},
                     "persist": {F64: (64, 257), F32: (64, 385)}, "two_stage": {F64: (49, 193), F32: (49, 193)},
                     "auto": {F64: (192, 385), F32: (192, 385)}}


def all_orders(dtype):
    return sorted({k for f in FORMS for k in orders(f, dtype)})


def cross_p(k, dtype):
    """a wanted count whose inverse iteration runs in more than one LU batch (xk_small_eigh_big_batch(k, p) < p) with
    a ragged last batch, or None where every p <= min(k, 256) fits one batch.  Where only one shift fits (float64
    beyond order 1024) every batch is full: 3 there."""
    big_batch = _fn("xk_small_eigh_big_batch")
    pmax = min(k, 256)
    pb = big_batch(k, pmax, _esize(dtype))
    if pb <= 0 or pb >= pmax:
        return None
    p = pb + 1 if pb > 1 else 3
    assert p <= pmax and big_batch(k, p, _esize(dtype)) == pb
    return p


def wanted_counts(form, k, dtype):
    if form == "tri":
        return sorted({p for p in (1, 6, min(k, 16)) if p <= k and tri_ok(k, p, dtype)})
    ps = {p for p in (1, 6) if p <= k}
    pc = cross_p(k, dtype)
    if pc is not None:
        ps.add(pc)
    if k in WIDE_ORDERS[form]:
        ps.add(min(k, 256))
    return sorted(p for p in ps if big_ok(k, p, dtype))


# ---------------------------------------------------------------------------------------------------- cases
def cluster_bits(k, dtype):
    """cluster spacing 2^-bits at which T of order k stays exact in `dtype` (with the spectra below)"""
    if dtype == F64 or k <= 128:
        return jc.cluster_bits(dtype)
    return min(12, 21 - (k.bit_length() - 1))          # |d| < 8: log2(n) + 3 + bits <= 24


def spectrum(family, k, dtype):
    j = torch.arange(k, dtype=F64)
    if family == "multiple64":                  # 64-fold eigenvalues at the wanted end (and everywhere else)
        return torch.floor(j / 64)
    if dtype == F64 or k <= 128 or family in ("spread", "multiple"):
        assert family in ("spread", "multiple") or cluster_bits(k, dtype) == jc.cluster_bits(dtype)
        return jc.spectrum(family, k, dtype)
    h = 2.0 ** -cluster_bits(k, dtype)
    rest = torch.remainder(j, 64) / 16          # bounded magnitude: 64 distinct values in [0, 4)
    if family == "cluster":
        return torch.where(j < 4, 1 + j * h, 2 + rest)
    if family == "edgegap":
        return torch.where(j < 6, torch.ones_like(j), torch.where(j == 6, torch.full_like(j, 1 + h), 3 + rest))
    raise ValueError(family)


def _hadamard_case(d, k):
    T = torch.zeros(k, k, dtype=F64)
    H = torch.zeros(k, k, dtype=F64)
    n = torch.ones(k, dtype=F64)
    at = 0
    for nb in jc.blocks(k):
        Hb = jc.hadamard(nb)
        sl = slice(at, at + nb)
        T[sl, sl] = (Hb * d[sl]) @ Hb / nb
        H[sl, sl] = Hb
        n[sl] = nb
        at += nb
    perm = jc.interleave(k)
    return Case(T[perm][:, perm], d, H[perm], n)


def assert_exact(c, dtype, tag):
    assert torch.equal(c.T, c.T.T), tag
    assert torch.equal(c.T.to(dtype).double(), c.T), tag


@functools.lru_cache(maxsize=12)
def case(family, k, dtype):
    """Case of the family at order k, exact in `dtype` (asserted)"""
    if family in jc.TRIVIAL:
        c = jc.case(family, k, dtype)
    else:
        d = spectrum(family, k, dtype)
        # every partial sum of (H d) H is an integer multiple of 2^-bits below 2^53 2^-bits: the product is exact
        bits = 0
        while not torch.equal(torch.floor(d * 2.0 ** bits), d * 2.0 ** bits):
            bits += 1
            assert bits <= 40, (family, k)
        assert jc.blocks(k)[0] * float(d.abs().max()) * 2.0 ** bits <= 2.0 ** 53, (family, k, bits)
        c = _hadamard_case(d, k)
    assert_exact(c, dtype, (family, k, dtype))
    return c


def cases(k, dtype):
    return [case(f, k, dtype) for f in FAMILIES]


def ratios(T, lam, Y, c, p, uppest, dtype):
    """jacobi_cases.ratios, with proj dropped where its unit k u |d| / gap is PROJ_UNIT_MAX or more"""
    r = jc.ratios(T, lam, Y, c, p, uppest, dtype)
    if r["proj"] is not None:
        k = T.shape[-1]
        gap = jc.wanted(c.d, p, uppest)[2]
        nd = max(float(c.d.abs().max()), 1.0)
        if k * jc.unit_roundoff(dtype) * nd / gap >= PROJ_UNIT_MAX:
            r["proj"] = None
    return r


def ratios_generic(T, lam, Y, lam_ref, dtype):
    """the same quantities against a float64 reference spectrum of a generic matrix (lam_ref: the wanted slice): no
    exact projector, so no proj"""
    k, p = T.shape[-1], lam.numel()
    ku = k * jc.unit_roundoff(dtype)
    nd = max(float(lam_ref.abs().max()), 1.0)
    return {"lam": float((lam - lam_ref).abs().max()) / (ku * nd),
            "res": float((Y @ T - lam[:, None] * Y).abs().max()) / (ku * nd),
            "orth": float((Y @ Y.T - torch.eye(p, dtype=F64)).abs().max()) / ku}


# ---------------------------------------------------------------------------------------------------- scale
# tri_scale_in_range (xk_tridiag.h): the frexp exponent of the tridiagonal's Gershgorin bound, which lies in
# [|T|, 3 |T|], must be within +-450 (float64) / +-50 (float32); outside it the result is flagged
SCALE_LIMIT = {F64: 450, F32: 50}
SCALE_EXPONENTS = {F64: {"in": (400, -400), "out": (500, -500)}, F32: {"in": (40, -40), "out": (60, -60)}}
SCALE_FAMILIES = ("spread", "cluster")


def scale_orders(form, dtype):
    """the member of orders(form) nearest 128 (the larger of two equally near), and for `persist` one hand-over order"""
    k0 = min(orders(form, dtype), key=lambda k: (abs(k - 128), -k))
    return (k0,) + ((handover_orders(dtype)[0],) if form == "persist" else ())


def scale_p(form, k, dtype):
    return max(p for p in wanted_counts(form, k, dtype) if p <= 6)


def exponent(x):
    return math.frexp(x)[1]


# ---------------------------------------------------------------------------------------------------- calibration
def calibration_plan(dtype):
    """(k, families, [(p, uppest), ...]) on which ?syevx is measured: every order up to 128 of every form with every
    wanted count and both ends; a sample of the orders beyond; the largest order once"""
    plan = []
    for k in all_orders(dtype):
        if k > 128:
            continue
        ps = {p for f in FORMS if k in orders(f, dtype) for p in wanted_counts(f, k, dtype)}
        plan.append((k, FAMILIES, [(p, up) for p in sorted(ps) for up in (False, True)]))
    for k in (129, 193, 257, 385, 512):
        pc = cross_p(k, dtype)
        todo = [(1, False), (6, True), (pc, False)] + ([(256, True)] if k == 257 else [])
        plan.append((k, FAMILIES, todo))
    plan.append((614, FAMILIES, [(6, False), (cross_p(614, dtype), True)]))
    plan.append((1025, ("cluster", "multiple64", "tridiagonal"), [(6, False)]))
    plan.append((1536 if dtype == F64 else 1500, ("cluster",), [(6, True)]))
    return plan
