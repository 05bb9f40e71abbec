"""-m gpu: the entry points of xk_fnm.hip against tests/fnm_ref.py within its bounds.

xk_fnm_step, all four dtypes, N below, at and off the 16 B vector width and beyond one block's stride, nblk = 1, 3 and
64, S = 3, nsteps = 8: a first step (r1 NaN-filled: it must not be read), a middle step and a `last` one, each with two
casts of the three systems: (running, past its m_s, b = 0) and (running, on its own last vector: X only, running).  Every
buffer is NaN-poisoned where the kernel has no business: [npad, ld) of the vectors, the entries of Tal, Tbe and C other
than the ones of this step, the other state slot; X and r1 of a system that is not to be written must come back
bit-identical, [N, npad) must be zero, inputs must not change and a second run must give identical bits.

Replay: 8 steps of xk_slq_step (with xk_kry_dots) on a random Hermitian matrix, then 8 steps of xk_fnm_step from the
recorded Tal, Tbe on the same products: every replayed vector must equal pass 1's bit for bit.

xk_fnm_eig + xk_fnm_coeff against numpy.linalg.eigh of the same Jacobi matrices under the bound of fnm_ref (C_K = 4):
nsteps in {1, 2, 3, 17, 64, 128}, S = 1 and 70 (systems of different m_s in one launch), every fn code, the fvals path
real and complex, a decoupled matrix, a matrix with a node <= 0; Q orthonormal to 64 m EPS64; tail; flags."""
import math
import numpy as np
import pytest
import torch
from tests import krylov_ref as kref
from tests import slq_ref as sref
from tests import fnm_ref as fref
from tests.test_gpu_slq_kernels import _lanczos_T, _bits, _same
from xitorch_amd import kernels as K
from xitorch_amd.linalg._panel import pad_len
from xitorch_amd.linalg.native_krylov import _Kry
from xitorch_amd.linalg.native_slq import _Geom

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.float64, torch.float32, torch.complex128, torch.complex64]
IDS = ["f64", "f32", "c128", "c64"]
NS = [1, 2, 3, 40, 257, 1031]
NSTEPS = 8
S3 = 3
WORST_C = {}


def _step_inputs(dtype, N, nblk, k, kstate, ms, flags, seed):
    g = torch.Generator().manual_seed(seed)
    ld = (N + 15) // 16 * 16 + (16 if N % 2 else 0)
    W, r2, r1, X = kref.rand_vecs(g, dtype, S3, N, ld, 4)
    if k == 0:
        r1[:] = kref.nan_of(dtype)                               # a first step must not read r1
    rnd = lambda *shape: 0.5 + torch.rand(*shape, dtype=torch.float64, generator=g)
    sgn = lambda t: t * torch.where(torch.rand(t.shape, dtype=torch.float64, generator=g) < 0.5, -1.0, 1.0)
    Tal = torch.full((S3, NSTEPS), math.nan, dtype=torch.float64)
    Tbe = torch.full((S3, NSTEPS), math.nan, dtype=torch.float64)
    cshape = (S3, NSTEPS, 2) if dtype.is_complex else (S3, NSTEPS)
    C = torch.full(cshape, math.nan, dtype=torch.float64)
    Tal[:, k], Tbe[:, k], C[:, k] = sgn(rnd(S3)), rnd(S3), sgn(rnd(*((S3,) + cshape[2:])))
    if k > 0:
        Tbe[:, k - 1] = rnd(S3)
    state = sref.rand_state(g, S3, kstate)
    state[kstate & 1, :, sref.M] = torch.tensor(ms, dtype=torch.float64)
    state[kstate & 1, :, sref.FLAG] = torch.tensor(flags, dtype=torch.float64)
    return ld, W, r2, r1, X, C, Tal, Tbe, state


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_step(dtype, N):
    env_of = {}
    vn = kref.VEC_ELEMS[dtype]
    npad = (N + vn - 1) // vn * vn
    for nblk in (1, 3, 64):
        env = env_of.setdefault(nblk, sref.Env(dtype, S3, N, nblk))
        for k, last in ((0, False), (3, False), (5, True)):
            casts = (((NSTEPS, k, NSTEPS), (0, 1, 2)),               # running; past its m_s (a breakdown); b = 0
                     ((NSTEPS, k + 1, k + 2), (0, 1, 0)))            # running; its own last vector; running
            for ci, (ms, flags) in enumerate(casts):
                kstate = 4 - ci                                      # both slots
                what = "[%s N=%d nblk=%d k=%d last=%d cast %d]" % (dtype, N, nblk, k, last, ci)
                ld, W, r2, r1, X, C, Tal, Tbe, state = _step_inputs(dtype, N, nblk, k, kstate, ms, flags,
                                                                    1000 * N + 10 * nblk + k + ci)
                dW, dr2, dC, dTal, dTbe, dst = (t.to(DEV) for t in (W, r2, C, Tal, Tbe, state))
                outs = []
                for _ in range(2):
                    dr1, dX = r1.to(DEV), X.to(DEV)
                    K.fnm_step(dW, dr2, dr1, dX, dC, dTal, dTbe, dst, S3, N, ld, nblk, NSTEPS, k, kstate, last=last)
                    outs.append((dr1.cpu(), dX.cpu()))
                _same(outs[0][0], outs[1][0], "r1 of the second run " + what)
                _same(outs[0][1], outs[1][1], "X of the second run " + what)
                gr1, gX = outs[0]
                ref = fref.step(env, env.vec(W), env.vec(r2), env.vec(r1), env.vec(X), C, Tal, Tbe, state, k, kstate,
                                last)
                live, moved = ref["live"], ref["moved"]
                assert live.tolist() == [m > k and f != 2 for m, f in zip(ms, flags)]
                assert moved.tolist() == [bool(l) and not last and m > k + 1 for l, m in zip(live.tolist(), ms)]
                if bool((~live).any()):
                    _same(gX[~live], X[~live], "X of a system that is not to be written " + what)
                if bool((~moved).any()):
                    _same(gr1[~moved], r1[~moved], "r1 of a system that is not to be moved " + what)
                for got, src, mask, name in ((gX, X, live, "X"), (gr1, r1, moved, "r1")):
                    if bool(mask.any()):
                        assert bool((got[mask][:, N:npad] == 0).all()), "%s %s: [N, npad) not zero" % (name, what)
                        tail = got[mask][:, npad:]
                        tail = torch.view_as_real(tail) if tail.is_complex() else tail
                        assert bool(torch.isnan(tail).all()), "%s %s: [npad, ld) written" % (name, what)
                kref.check({"X": env.vec(gX)[live]}, {"X": (ref["X"][0][live], ref["X"][1][live])}, dtype,
                           what="fnm_step X " + what)
                if bool(moved.any()):
                    kref.check({"y": env.vec(gr1)[moved]}, {"y": (ref["y"][0][moved], ref["y"][1][moved])}, dtype,
                               what="fnm_step r1 " + what)
                for t, h, n in ((dW, W, "W"), (dr2, r2, "r2"), (dC, C, "C"), (dTal, Tal, "Tal"), (dTbe, Tbe, "Tbe"),
                                (dst, state, "state")):
                    _same(t, h, n + " " + what)


@pytest.mark.parametrize("last_by_null", [False, True], ids=["last-flag", "W-null"])
def test_last_needs_no_product(last_by_null):
    """`last` (or W == NULL) updates X only; W and r1 may then be absent"""
    dtype, N, k = torch.float64, 40, 5
    ld, W, r2, r1, X, C, Tal, Tbe, state = _step_inputs(dtype, N, 1, k, 0, (8, 8, 8), (0, 0, 0), 7)
    dX = X.to(DEV)
    rc = K.fnm_step(None, r2.to(DEV), None if last_by_null else r1.to(DEV), dX, C.to(DEV), Tal.to(DEV), Tbe.to(DEV),
                    state.to(DEV), S3, N, ld, 1, NSTEPS, k, 0, last=not last_by_null, raw=True)
    assert rc == 0
    env = sref.Env(dtype, S3, N, 1)
    ref = fref.step(env, env.vec(W), env.vec(r2), env.vec(r1), env.vec(X), C, Tal, Tbe, state, k, 0, True)
    kref.check({"X": env.vec(dX.cpu())}, {"X": ref["X"]}, dtype, what="fnm_step last")


@pytest.mark.parametrize("n", [40, 257])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_replay_is_bit_identical(dtype, n):
    g = torch.Generator().manual_seed(n)
    S = 2
    hp = torch.complex128 if dtype.is_complex else torch.float64
    M = torch.randn(n, n, dtype=torch.float64, generator=g)
    if dtype.is_complex:
        M = torch.complex(M, torch.randn(n, n, dtype=torch.float64, generator=g))
    A = ((M + M.conj().T) / 2).to(dtype).to(DEV)
    geom = _Geom(n, 1, S, dtype, DEV)
    kr = _Kry(geom)
    N, ld, nblk = n, geom.ld, kr.nblk
    b = geom.new()
    b[0, :, :n] = kref.rand_vecs(g, dtype, S, n, n)[0].to(DEV)
    apply = lambda r2, W: W[0, :, :n].copy_((A @ r2[0, :, :n].T).T)
    # pass 1, keeping every vector and every product
    r1, r2, W = geom.new(), geom.new(), geom.new()
    Pa, Pn = kr.partial(), (kr.partial_real(), kr.partial_real())
    state = K.slq_state(S, DEV)
    Tal = torch.zeros((S, NSTEPS), dtype=torch.float64, device=DEV)
    Tbe = torch.zeros_like(Tal)
    kr.dots(b, b, Pa)
    K.slq_init(b, r2, Pa, state, S, N, ld, nblk, 0)
    vecs, prods = [], []
    for k in range(NSTEPS):
        vecs.append(r2.clone())
        apply(r2, W)
        prods.append(W.clone())
        kr.dots(r2, W, Pa)
        K.slq_step(W, r2, r1, Pa, Pn[k & 1], Pn[(k + 1) & 1], state, Tal, Tbe, S, N, ld, nblk, NSTEPS, k)
        r1, r2 = r2, r1
    ks = NSTEPS & 1
    assert state[ks, :, sref.M].tolist() == [NSTEPS] * S and state[ks, :, sref.FLAG].tolist() == [0.0] * S
    # pass 2 from the recorded scalars, on the same products
    cshape = (S, NSTEPS, 2) if dtype.is_complex else (S, NSTEPS)
    C = torch.ones(cshape, dtype=torch.float64, device=DEV)
    X = geom.new()
    q2, q1 = b.clone(), torch.full_like(b, kref.nan_of(dtype))
    for k in range(NSTEPS):
        _same(q2[:, :, :n], vecs[k][:, :, :n], "replayed vector %d" % k)     # (the pads of q1 keep their NaN)
        last = k == NSTEPS - 1
        K.fnm_step(None if last else prods[k], q2, q1, X, C, Tal, Tbe, state, S, N, ld, nblk, NSTEPS, k, ks, last=last)
        q1, q2 = q2, q1
    # and X is the sum it should be: sum_k ((1 [+ i]) / beta_k) r2_k
    c = complex(1, 1) if dtype.is_complex else 1.0
    want = sum((c / Tbe[:, k].to(hp))[None, :, None] * vecs[k].to(hp) for k in range(NSTEPS))
    mag = sum((abs(c) / Tbe[:, k])[None, :, None] * vecs[k].abs().to(torch.float64) for k in range(NSTEPS))
    assert bool(((X.to(hp) - want).abs() <= fref.C_X * NSTEPS * sref.eps_of(dtype) * mag).all())


# ------------------------------------------------------------------------------------------------ eig + coeff
@pytest.mark.parametrize("S", [1, 70])
@pytest.mark.parametrize("nsteps", [1, 2, 3, 17, 64, 128])
def test_eig_coeff(nsteps, S):
    INDEFINITE = fref.INDEFINITE
    Tal, Tbe, state, k, ms, zzs = fref.eig_cases(_lanczos_T, nsteps, S)
    dTal, dTbe, dst = (torch.from_numpy(a).to(DEV) for a in (Tal, Tbe, state))
    theta, Qt, flag = K.fnm_eig(dTal, dTbe, dst, k)
    theta2, Qt2, flag2 = K.fnm_eig(dTal, dTbe, dst, k)
    for a, b in ((theta, theta2), (Qt, Qt2), (flag, flag2)):
        _same(a, b, "second run of xk_fnm_eig")
    th_h, Q_h, fl_h = theta.cpu().numpy(), Qt.cpu().numpy(), flag.cpu().numpy()
    assert not fl_h.any()
    truth = []
    for s in range(S):
        m = ms[s]
        what = "xk_fnm_eig nsteps=%d s=%d m=%d" % (nsteps, s, m)
        assert np.all(th_h[s, m:] == 0) and np.all(Q_h[s, m:, :] == 0) and np.all(Q_h[s, :, m:] == 0), what
        if m == 0:
            truth.append(None)
            continue
        T = sref.jacobi(Tal[s], Tbe[s], m)
        tn = np.abs(T).sum(1).max()
        ev, U = np.linalg.eigh(T)
        truth.append((T, tn, ev, U))
        Z = Q_h[s, :m, :m].T                                     # Z[j, i]: component j of eigenvector i
        assert np.all(np.abs(np.sort(th_h[s, :m]) - ev) <= sref.C_Q * m * sref.EPS64 * tn), what
        assert np.abs(Z.T @ Z - np.eye(m)).max() <= fref.C_QORTH * m * fref.EPS64, what
        assert np.abs((Z * th_h[s, :m]) @ Z.T - T).max() <= fref.C_QORTH * m * fref.EPS64 * tn, what
    worst = 0.0

    def judge(Cd, taild, s, want, bound, what):
        nonlocal worst
        m = ms[s]
        got = Cd[s, :m]
        assert np.all(Cd[s, m:] == 0), what
        err = float(np.linalg.norm(got - want))
        assert err <= bound, "%s: |error| %.3e, bound %.3e" % (what, err, bound)
        if bound > 0:
            worst = max(worst, err / bound)
        if m <= 4:
            assert taild[s] == 0, what
        elif np.linalg.norm(want) > 0:
            assert abs(taild[s] - fref.tail_of(want)) <= 2 * bound / np.linalg.norm(want), what

    t = -0.01
    for name, code in sref.FN_CODES.items():
        fl = flag.clone()
        C, tail = K.fnm_coeff(Qt, theta, dst, fl, k, code, t)
        fl2 = flag.clone()
        C2, tail2 = K.fnm_coeff(Qt, theta, dst, fl2, k, code, t)
        for a, b in ((C, C2), (tail, tail2), (fl, fl2)):
            _same(a, b, "second run of xk_fnm_coeff")
        Ch, th, fh = C.cpu().numpy(), tail.cpu().numpy(), fl.cpu().numpy()
        for s in range(S):
            m = ms[s]
            what = "xk_fnm_coeff %s nsteps=%d s=%d m=%d" % (name, nsteps, s, m)
            if m == 0:
                assert fh[s] == 0 and th[s] == 0 and not Ch[s].any(), what
                continue
            if name in sref.NEEDS_POSITIVE and truth[s][2].min() <= 0:
                assert s == INDEFINITE and fh[s] == 1 and np.isnan(Ch[s, :m]).all() and np.all(Ch[s, m:] == 0), what
                continue
            assert fh[s] == 0, what
            want, bound = fref.coeff_truth(Tal[s], Tbe[s], m, zzs[s], name, t)
            judge(Ch, th, s, want, bound, what)
        if S > INDEFINITE and name in sref.NEEDS_POSITIVE:
            assert fh[INDEFINITE] == 1 and np.count_nonzero(fh) == 1, "bit 0 for the indefinite system only"
    # the caller's values: real (sqrt of |theta|), then complex (exp(-i tau theta)) with C as (re, im) pairs
    fl = flag.clone()
    fv = torch.sqrt(theta.abs())
    C, tail = K.fnm_coeff(Qt, theta, dst, fl, k, -1, 0.0, fvals=fv.contiguous())
    Ch, th = C.cpu().numpy(), tail.cpu().numpy()
    assert not fl.cpu().numpy().any()                             # no positivity is asked of the caller's values
    tau = 0.3
    fvc = torch.view_as_real(torch.exp(-1j * tau * theta)).contiguous()
    Cc, tailc = K.fnm_coeff(Qt, theta, dst, fl, k, -1, 0.0, fvals=fvc, cplx=True)
    Cch, tch = torch.view_as_complex(Cc).cpu().numpy(), tailc.cpu().numpy()
    for s in range(S):
        m = ms[s]
        if m == 0:
            assert not Ch[s].any() and not Cch[s].any()
            continue
        T, tn, ev, U = truth[s]
        bn = math.sqrt(zzs[s])
        f = np.sqrt(np.abs(ev))
        with np.errstate(all="ignore"):
            df = 0.5 / np.sqrt(np.abs(ev))
        if np.abs(ev).min() > 1e-3:                               # (sqrt |x| is not smooth at 0)
            judge(Ch, th, s, bn * (U @ (f * U[0])), fref.C_K * m * fref.EPS64 * bn * (f.max() + tn * df.max()),
                  "fvals real s=%d" % s)
        judge(Cch, tch, s, bn * (U @ (np.exp(-1j * tau * ev) * U[0])), fref.C_K * m * fref.EPS64 * bn * (1 + tn * tau),
              "fvals complex s=%d" % s)
    # a named function on a complex system: imaginary parts zero, real parts those of the real call
    fl = flag.clone()
    Cr, _ = K.fnm_coeff(Qt, theta, dst, fl, k, sref.FN_CODES["exp"], t)
    fl = flag.clone()
    Cp, _ = K.fnm_coeff(Qt, theta, dst, fl, k, sref.FN_CODES["exp"], t, cplx=True)
    _same(Cp[..., 0].contiguous(), Cr, "real parts of a named function")
    assert not bool(Cp[..., 1].any())
    _same(dTal, torch.from_numpy(Tal), "Tal")
    _same(dTbe, torch.from_numpy(Tbe), "Tbe")
    _same(dst, torch.from_numpy(state), "state")
    WORST_C[(nsteps, S)] = worst
    print("xk_fnm_eig + xk_fnm_coeff nsteps = %d S = %d: worst error / bound %.3f" % (nsteps, S, worst))


def test_worst_ratio_report():
    """(runs last in this file) the largest |kernel - reference| / bound seen"""
    for d, w in sorted(kref.WORST.items(), key=lambda kv: str(kv[0])):
        print("fnm_step: worst error / bound for %s: %.3f" % (d, w))
    for key, w in sorted(WORST_C.items()):
        print("fnm_eig + fnm_coeff: worst error / bound at nsteps = %d, S = %d: %.3f" % (key + (w,)))
