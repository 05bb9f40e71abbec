"""CPU: the Krylov step-kernel checker of tests/krylov_ref.py accepts a correct output rounded to the kernel dtype
and rejects plausible kernel bugs (tests/krylov_ref.py FAULTS) at shapes where they matter -- the evidence that
tests/test_gpu_krylov_kernels.py would fail on a subtly wrong kernel."""
import pytest
import torch
from tests import krylov_ref as kref

DTYPES = [torch.float64, torch.float32, torch.complex128, torch.complex64]
IDS = ["f64", "f32", "c128", "c64"]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _expect_rejected(mut, ref, dtype, fault):
    with pytest.raises(AssertionError):
        kref.check(kref.values(mut, dtype), ref, dtype, what=fault)


def _expect_accepted(ref, dtype):
    assert kref.check(kref.values(ref, dtype), ref, dtype) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_checker_accepts_reference_rounded_to_kernel_dtype(dtype):
    g = _gen(1)
    S, N, nblk = 3, 5 * 1024 * kref.VEC_ELEMS[dtype] + 37, 7
    ctx = kref.Ctx(dtype, S, N, nblk)
    x, y, z, w = (ctx.vec(t) for t in kref.rand_vecs(g, dtype, S, N, N + 8, count=4))
    E = ctx.scal(kref.rand_scalars(g, dtype, S))
    _expect_accepted(kref.kry_dots(ctx, x, y, None, None, z, E, conj1=True, x2_is_y1=True, y2_is_y1=True), dtype)
    P = [kref.rand_partials(g, dtype, S, nblk, zero_systems=(1,)) for _ in range(2)]
    sc = [ctx.scal(kref.rand_scalars(g, dtype, S)) for _ in range(3)]
    _expect_accepted(kref.bicg_p(ctx, x, y, z, P[0], sc[0], sc[1], sc[2], first=False), dtype)
    _expect_accepted(kref.bicg_s(ctx, x, y, sc[0], P[0]), dtype)
    _expect_accepted(kref.bicg_final(ctx, x, y, z, z, w, x, sc[0], P[0], P[1], skip_r=False), dtype)
    _expect_accepted(kref.kry_resid(ctx, x, y, z, True), dtype)
    _expect_accepted(kref.cg_update(ctx, x, y, z, w, P[0], P[1], skip_r=False), dtype)
    _expect_accepted(kref.cg_p(ctx, x, y, P[0], P[1]), dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.complex64], ids=["f64", "f32", "c64"])
@pytest.mark.parametrize("nblk", [1, 2])
def test_rejects_dot_that_drops_the_ragged_tail(dtype, nblk):
    """the last N mod VN elements dropped (a kernel looping over whole vectors of N // VN only)"""
    g = _gen(2)
    vn = kref.VEC_ELEMS[dtype]
    S, N = 3, 250 * vn + vn - 1
    ctx = kref.Ctx(dtype, S, N, nblk)
    x1, y1 = (ctx.vec(t) for t in kref.rand_vecs(g, dtype, S, N, N + 8, count=2))
    x1[:, N - N % vn:] = 1                  # an O(1) tail: what goes missing is well above the dot bound
    y1[:, N - N % vn:] = 1
    ref = kref.kry_dots(ctx, x1, y1)
    _expect_rejected(kref.kry_dots(ctx, x1, y1, fault="drop_tail"), ref, dtype, "drop_tail")
    ref = kref.kry_resid(ctx, x1, y1 * 0, None, True)
    _expect_rejected(kref.kry_resid(ctx, x1, y1 * 0, None, True, fault="drop_tail"), ref, dtype, "drop_tail")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N_blocks,nblk", [((5, 37), 7), ((64, 1), 64), ((0, 5), 2)])
def test_rejects_a_dropped_block_partial(dtype, N_blocks, nblk):
    """one block's partial missing from the two-stage sum (a consumer reading nblk - 1 slots, a producer block that
    never stores): |r|^2-type partials cannot cancel, so the loss is a whole block's share"""
    g = _gen(3)
    vn = kref.VEC_ELEMS[dtype]
    S, N = 3, N_blocks[0] * 1024 * vn + N_blocks[1]
    ctx = kref.Ctx(dtype, S, N, nblk)
    b, y, r0 = (ctx.vec(t) for t in kref.rand_vecs(g, dtype, S, N, N, count=3))
    ref = kref.kry_resid(ctx, b, y, r0, True)
    _expect_rejected(kref.kry_resid(ctx, b, y, r0, True, fault="drop_block"), ref, dtype, "drop_block")
    ref = kref.kry_dots(ctx, b, b, x1_is_y1=True)
    _expect_rejected(kref.kry_dots(ctx, b, b, x1_is_y1=True, fault="drop_block"), ref, dtype, "drop_block")


@pytest.mark.parametrize("dtype", [torch.complex128, torch.complex64], ids=["c128", "c64"])
def test_rejects_unconjugated_and_conj1_ignored_complex_dots(dtype):
    g = _gen(4)
    S, N, nblk = 3, 1000, 1
    ctx = kref.Ctx(dtype, S, N, nblk)
    x1, y1, z = (ctx.vec(t) for t in kref.rand_vecs(g, dtype, S, N, N + 8, count=3))
    E = ctx.scal(kref.rand_scalars(g, dtype, S))
    ref = kref.kry_dots(ctx, x1, y1)
    _expect_rejected(kref.kry_dots(ctx, x1, y1, fault="noconj"), ref, dtype, "noconj")
    Pts, Ptt = kref.rand_partials(g, dtype, S, nblk), kref.rand_partials(g, dtype, S, nblk)
    ref = kref.bicg_final(ctx, x1, y1, z, z, y1, x1, E, Pts, Ptt, skip_r=False)
    mut = kref.bicg_final(ctx, x1, y1, z, z, y1, x1, E, Pts, Ptt, skip_r=False, fault="noconj")
    _expect_rejected(mut, ref, dtype, "noconj")
    # the BiCGStab form: <t, s> with t = y1 shifted, <t, t>
    kw = dict(shiftz=z, E=E, conj1=True, x2_is_y1=True, y2_is_y1=True)
    ref = kref.kry_dots(ctx, x1, y1, **kw)
    _expect_rejected(kref.kry_dots(ctx, x1, y1, fault="conj1_ignored", **kw), ref, dtype, "conj1_ignored")


def _consumers(ctx, g, dtype, first=False):
    """every consumer of partials / per-system scalars on one input set; systems 1 (and 4, ...) have exactly zero
    denominators, system 2 (and 6, ...) a zero omega"""
    S, N, nblk = ctx.S, ctx.N, ctx.nblk
    zs = [s for s in range(S) if s % 3 == 1]
    x, y, z, w = (ctx.vec(t) for t in kref.rand_vecs(g, dtype, S, N, N, count=4))
    Pnum = kref.rand_partials(g, dtype, S, nblk)
    Pden = kref.rand_partials(g, dtype, S, nblk, zero_systems=zs)
    rho_old = ctx.scal(kref.rand_scalars(g, dtype, S))
    omega = ctx.scal(kref.rand_scalars(g, dtype, S))
    alpha = ctx.scal(kref.rand_scalars(g, dtype, S))
    rho_old[zs] = 0
    omega[[s for s in range(S) if s % 4 == 2]] = 0
    return {
        "bicg_p": lambda f: kref.bicg_p(ctx, x, y, z, Pnum, rho_old, alpha, omega, first=first, fault=f),
        "bicg_s": lambda f: kref.bicg_s(ctx, x, y, alpha, Pden, fault=f),
        "bicg_final": lambda f: kref.bicg_final(ctx, x, y, z, z, w, x, alpha, Pnum, Pden, skip_r=False, fault=f),
        "cg_update": lambda f: kref.cg_update(ctx, x, y, z, w, Pnum, Pden, skip_r=False, fault=f),
        "cg_p": lambda f: kref.cg_p(ctx, x, y, Pnum, Pden, fault=f),
    }


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fault", ["eps_all", "eps_none"])
def test_rejects_misplaced_eps_substitution(dtype, fault):
    """eps must replace an exactly-zero denominator of THAT system only (oracle/solve.py:15-18)"""
    ctx = kref.Ctx(dtype, 7, 1000, 2)
    for name, run in _consumers(ctx, _gen(5), dtype).items():
        _expect_rejected(run(fault), run(None), dtype, "%s %s" % (name, fault))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rejects_bicg_p_first_ignored_and_swapped_rho(dtype):
    ctx = kref.Ctx(dtype, 3, 1000, 2)
    run = _consumers(ctx, _gen(6), dtype, first=True)["bicg_p"]
    _expect_rejected(run("first_ignored"), run(None), dtype, "first_ignored")
    for name, run in _consumers(ctx, _gen(7), dtype).items():
        if name in ("bicg_p", "cg_p"):
            _expect_rejected(run("rho_swap"), run(None), dtype, "%s rho_swap" % name)


def test_block_range_tiles_the_padded_range():
    """the replica of block_range: blocks tile [0, npad) in order, empty blocks when nblk exceeds the chunks"""
    for vn in (1, 2, 4):
        for N in (1, 5, vn + 1, 1000, 1024 * vn + 1, 300001):
            for nblk in (1, 2, 7, 64):
                rs = [kref.block_range(N, nblk, b, vn) for b in range(nblk)]
                npad = (N + vn - 1) // vn * vn
                assert rs[0][0] == 0 and rs[-1][1] == npad
                assert all(rs[i][1] == rs[i + 1][0] for i in range(nblk - 1))
                assert all(lo <= hi for lo, hi in rs)
    assert kref.block_range(5, 7, 6, 2) == (6, 6)      # N = 5, nblk = 7: blocks 3..6 are empty
