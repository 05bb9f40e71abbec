"""CPU: the reference of tests/banded_ref.py (the banded operator apply xk_banded_mm) agrees with independent
formulations (the oracle's dense matrix, linop.banded_apply_torch, a numpy.longdouble dense product), its checker
accepts a correct output rounded to the kernel dtype at EVERY configuration of tests/test_gpu_banded_kernel.py and
rejects every fault of banded_ref.FAULTS wherever banded_ref.VISIBLE says the fault can show -- and every fault shows
in at least one configuration per dtype, so the configuration list cannot shrink into blindness."""
import numpy as np
import pytest
import torch
from oracle import ops as oops
from tests import banded_ref as br
from tests import solver_ref as sr
from xitorch_amd.linop import banded_apply_torch

DTYPES = br.DTYPES
IDS = [br.DNAME[d] for d in DTYPES]
LD = np.longdouble

# (N, hb, C, B, bcast): hb = 0, hb >= N, a band per member and a broadcast one, more than one chunk of columns
SMALL = [(1, 0, 1, 1, False), (7, 0, 3, 3, False), (50, 63, 3, 3, False), (50, 5, 17, 1, False), (40, 5, 9, 3, True),
         (130, 63, 2, 2, False)]


def _small_cases(dtype):
    return [br.case(dtype, br.Cfg(*s, trans, False)) for s in SMALL for trans in (False, True)]


def _rejected(got, ref, dtype):
    try:
        br.check(got, ref, br.KERNEL, dtype)
    except AssertionError:
        return True
    return False


# ================================================================================================ (a) independent forms
def test_reference_is_the_dense_matrix_and_the_torch_apply():
    """the reference value equals the oracle's BandedOp(...).fullmatrix() (out-of-matrix storage zeroed: the oracle
    multiplies by it) applied densely, and linop.banded_apply_torch fed the NaN-holding band itself; both in float64,
    each within the reference's share (1 / REF) of the float64 bound"""
    dtype = torch.float64
    for c in _small_cases(dtype):
        cfg = c["cfg"]
        val, bnd = br.ref(dtype, c)["Y"]
        band, x = c["band"].double(), c["X"].double().transpose(1, 2)              # x (B, N, C)
        A = oops.BandedOp(torch.nan_to_num(band, nan=0.0)).fullmatrix()            # (1 or B, N, N)
        dense = ((A.transpose(1, 2) if cfg.trans else A) @ x).transpose(1, 2)
        assert bool(((val - dense).abs() <= bnd / br.REF).all()), cfg
        torchy = banded_apply_torch(band, x, cfg.trans).transpose(1, 2)
        assert bool(torch.isfinite(torchy).all()) and bool(((val - torchy).abs() <= bnd / br.REF).all()), cfg


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_reference_rounding_stays_within_its_share_of_the_bound(dtype):
    """against the dense product in numpy.longdouble: the float64 reference is off by at most (t + 1) 2^-53 sum |band
    x|, i.e. 1 / REF of the float64 bound (and a 2^-29-th of that of the float32 one)"""
    for c in _small_cases(dtype):
        cfg = c["cfg"]
        val, bnd = br.ref(dtype, c)["Y"]
        band = torch.nan_to_num(c["band"].double(), nan=0.0) * br.in_matrix(cfg.hb, cfg.N)
        nb, N = band.shape[0], cfg.N
        A = np.zeros((nb, N, N), LD)
        for d in range(2 * cfg.hb + 1):
            for i in range(N):
                if 0 <= i + d - cfg.hb < N:
                    A[:, i, i + d - cfg.hb] = band[:, d, i].numpy()
        if cfg.trans:
            A = A.transpose(0, 2, 1)
        x = c["X"].double().numpy().astype(LD)                                     # (B, C, N)
        want = np.einsum("bij,bcj->bci", np.broadcast_to(A, (cfg.B, N, N)), x)
        err = np.abs(val.numpy().astype(LD) - want)
        share = bnd.numpy().astype(LD) / br.REF * LD(sr.U64 / br.unit_roundoff(dtype))
        assert bool((err <= share).all()), (cfg, float(err.max()))


def test_out_of_matrix_storage_is_never_read():
    """the stored NaN may become anything: the reference does not move by a bit"""
    dtype = torch.float64
    for c in _small_cases(dtype):
        cfg = c["cfg"]
        other = torch.where(br.in_matrix(cfg.hb, cfg.N), c["band"], torch.full_like(c["band"], 1e300))
        a, b = br.ref(dtype, c)["Y"], br.banded_mm(dtype, other, c["X"], cfg.hb, cfg.trans)["Y"]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_operator_reference_broadcasts_like_the_torch_apply():
    g = br._gen(12)
    for BA, BX in (((), (4,)), ((3,), (3,)), ((3,), (2, 3)), ((2, 1), (2, 3))):
        band = br._randn(g, *BA, 7, 20)
        x = br._randn(g, *BX, 20, 3)
        for trans in (False, True):
            val, bnd = br.operator_ref(torch.float64, band, x, trans)["Y"]
            want = banded_apply_torch(band, x, trans)
            assert val.shape == want.shape and bool(((val - want).abs() <= bnd / br.REF).all())


# ================================================================================================ (b) faults
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_banded_mm_faults_rejected_everywhere(dtype):
    """at every configuration of the GPU test: the reference rounded to the kernel dtype is accepted, every visible
    fault's output rounded to the kernel dtype rejected; every fault is visible somewhere"""
    seen = {f: 0 for f in br.FAULTS}
    for cfg in br.configs(dtype):
        c = br.case(dtype, cfg)
        ref = br.ref(dtype, c)
        assert br.check(sr.values(ref, dtype), ref, br.KERNEL, dtype, what=str(cfg)) <= 1.0
        for f in br.FAULTS:
            if br.VISIBLE[f](cfg, dtype):
                seen[f] += 1
                assert _rejected(sr.values(br.ref(dtype, c, f), dtype), ref, dtype), \
                    "%s: fault %s not rejected at %s" % (br.DNAME[dtype], f, cfg)
    for f in br.FAULTS:
        assert seen[f] >= 1, "fault %s shows at no configuration" % f


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_configurations_cover_every_listed_value(dtype):
    """every N, hb, C and batch form the kernel has a path for appears with both `trans`, and so do the misaligned
    band and a tile of 8 columns above 64 KiB on both the vector and the scalar path"""
    R, vn = br.rows_of(dtype), br.VEC_ELEMS[dtype]
    cfgs = br.configs(dtype)
    for trans in (False, True):
        sub = [c for c in cfgs if c.trans == trans]
        assert {0, 1, 2, 3, 50, R - 1, R, R + 1, 2 * R + vn + 1} <= {c.N for c in sub}
        assert any(c.N > 2 * R and c.N % vn == 0 for c in sub) and any(c.N > 2 * R and c.N % vn for c in sub)
        assert {0, 1, 5, 63, 600} <= {c.hb for c in sub} and any(c.hb >= c.N > 0 for c in sub)
        assert {0, 1, 3, 8, 9, 17} <= {c.C for c in sub}
        assert {(1, False), (3, False), (3, True)} <= {(c.B, c.bcast) for c in sub}
        assert any(c.offset and c.N % vn == 0 for c in sub)
        for vec in (True, False):
            assert any(min(c.C, 8) * (R + 2 * c.hb) * (16 // vn) > 64 * 1024 and (c.N % vn == 0) == vec for c in sub)
    assert set(br.VISIBLE) == set(br.FAULTS)
    for c in cfgs:
        if c.hb == 600:
            assert c.N <= 2 * R + vn + 1 and c.B <= 2
