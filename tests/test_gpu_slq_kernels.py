"""-m gpu: the entry points of xk_slq.hip in all four dtypes against tests/slq_ref.py within its bounds.

xk_slq_init and xk_slq_step are fed the partial arrays the restatement is fed.  N below, at and off the 16 B vector
width and beyond one block's stride, nblk = 1, 3 and 64, S = 1 and 5, both state slots.  With S = 5 the systems are: 0 and
4 running, 1 frozen, 2 on its first step (no previous beta: r1 is NaN-filled and must not be read), 3 meeting a breakdown
in this step.  Every buffer is NaN-poisoned where the kernel has no business: [npad, ld) of the vectors, partial slots
[nblk, 64), the T entries other than the one written, everything of a frozen system; all of it must come back
bit-identical, [N, npad) must be zero, inputs must not change, flags and step counts must be exactly equal and a second
run must give identical bits.

xk_slq_quad against numpy.linalg.eigh of the same Jacobi matrices under the bound of slq_ref: m in {1, 2, 3, 17, 64,
128}, S = 1 and 70 (more than one wave of lanes, systems of different m_s in one launch), every fn code, a decoupled
matrix (some beta = 0), a matrix with a node <= 0."""
import math
import numpy as np
import pytest
import torch
from tests import krylov_ref as kref
from tests import slq_ref as sref
from xitorch_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.float64, torch.float32, torch.complex128, torch.complex64]
IDS = ["f64", "f32", "c128", "c64"]
NS = [1, 2, 3, 40, 257, 1031]
NSTEPS = 8


def _bits(t):
    t = t.detach().cpu().contiguous()
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.view({torch.float64: torch.int64, torch.float32: torch.int32}.get(t.dtype, t.dtype))


def _same(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), "%s changed" % what


class _Case:
    def __init__(self, dtype, N, S, nblk, k):
        self.dtype, self.N, self.S, self.nblk, self.k = dtype, N, S, nblk, k
        self.env = sref.Env(dtype, S, N, nblk)
        vn = kref.VEC_ELEMS[dtype]
        self.npad = (N + vn - 1) // vn * vn
        self.ld = (N + 15) // 16 * 16 + (16 if N % 2 else 0)
        self.g = g = torch.Generator().manual_seed(1000 * N + 10 * nblk + S + k)
        if S > 1:
            self.frozen, self.first, self.brk = [1], [2], [3]
        else:
            self.frozen, self.first, self.brk = [], ([0] if N % 2 else []), []
        self.W, self.r2, self.r1 = kref.rand_vecs(g, dtype, S, N, self.ld, 3)
        rd = kref.REAL_OF[dtype]
        self.Pa = kref.rand_partials(g, dtype, S, nblk)
        self.Pb = kref.rand_partials(g, dtype, S, nblk, zero_systems=self.frozen, positive=True)
        self.Pin = kref.rand_partials(g, rd, S, nblk, positive=True)
        for s in self.brk:
            self.Pin[s, :nblk] = 1e-30 / nblk
        self.state = sref.rand_state(g, S, k, frozen=self.frozen, first=self.first)
        self.what = "[%s N=%d S=%d ld=%d nblk=%d k=%d]" % (dtype, N, S, self.ld, nblk, k)

    def poison_vec(self):
        return torch.full((self.S, self.ld), kref.nan_of(self.dtype), dtype=self.dtype, device=DEV)

    def vec(self, t, name):
        """contract of a written vector: [N, npad) zero, [npad, ld) untouched; returns the [0, N) part"""
        t = t.cpu()
        assert bool((t[:, self.N:self.npad] == 0).all()), "%s %s: [N, npad) not zero" % (name, self.what)
        assert bool(torch.isnan(torch.view_as_real(t) if t.is_complex() else t)[:, self.npad:].all()), \
            "%s %s: [npad, ld) written" % (name, self.what)
        return self.env.vec(t)


def _configs(N):
    k = 3
    for nblk in (1, 3, 64):
        for S in (1, 5):
            k = 7 - k                                   # slots alternate: k = 4 reads slot 0, k = 3 reads slot 1
            yield nblk, S, k


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_init(dtype, N):
    for nblk, S, k in _configs(N):
        c = _Case(dtype, N, S, nblk, k)
        z, Pb = c.W.to(DEV), c.Pb.to(DEV)
        outs = []
        for _ in range(2):
            r2 = c.poison_vec()
            state = torch.full((2, S, sref.NST), math.nan, dtype=torch.float64, device=DEV)
            K.slq_init(z, r2, Pb, state, S, N, c.ld, nblk, k)
            outs.append((r2, state))
        (r2, state) = outs[0]
        _same(outs[1][0], r2, "r2 of the second run")
        _same(outs[1][1], state, "state of the second run")
        _same(c.vec(r2, "r2"), c.env.vec(c.W), "r2 against z " + c.what)            # a bit copy
        st = state.cpu()
        assert bool(torch.isnan(st[(k + 1) & 1]).all()), "the other state slot was written"
        ref = sref.init(c.env, c.Pb)
        kref.check({"state": st[k & 1]}, {"state": ref["state"]}, dtype, what="slq_init " + c.what)
        assert torch.equal(st[k & 1][:, sref.FLAG], ref["state"][0][:, sref.FLAG])
        assert bool((st[k & 1][c.frozen, sref.FLAG] == 2).all())                    # z = 0
        _same(z, c.W, "z")
        _same(Pb, c.Pb, "Pb")


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_step(dtype, N):
    eps = sref.eps_of(dtype)
    for nblk, S, k in _configs(N):
        c = _Case(dtype, N, S, nblk, k)
        W, r2, Pa, Pin = c.W.to(DEV), c.r2.to(DEV), c.Pa.to(DEV), c.Pin.to(DEV)
        r1h = c.r1.clone()
        if c.first:
            r1h[c.first] = kref.nan_of(dtype)                    # a first step must not read r1
        outs = []
        for _ in range(2):
            r1, state = r1h.to(DEV), c.state.to(DEV)
            Pout = kref.poisoned_partials(dtype, S, real=True).to(DEV)
            Tal = torch.full((S, NSTEPS), math.nan, dtype=torch.float64, device=DEV)
            Tbe = torch.full((S, NSTEPS), math.nan, dtype=torch.float64, device=DEV)
            K.slq_step(W, r2, r1, Pa, Pin, Pout, state, Tal, Tbe, S, N, c.ld, nblk, NSTEPS, k)
            outs.append((r1, state, Pout, Tal, Tbe))
        for a, b, n in zip(outs[0], outs[1], ("r1", "state", "Pout", "Tal", "Tbe")):
            _same(a, b, n + " of the second run " + c.what)
        r1, state, Pout, Tal, Tbe = outs[0]
        e = c.env
        ref = sref.step(e, e.vec(c.W), e.vec(c.r2), e.vec(c.r1), c.Pa, c.Pin, c.state, k, NSTEPS)
        live, frozen, broke = ref["live"], ref["frozen"], ref["broke"]
        assert frozen.tolist() == [s in c.frozen for s in range(S)] and broke.tolist() == [s in c.brk for s in range(S)]
        # the vectors
        r1c = r1.cpu()
        still = ~live
        if bool(still.any()):
            _same(r1c[still], r1h[still], "r1 of a frozen system " + c.what)
        yk = c.vec(r1c, "r1")
        yref, ey = ref["y"]
        kref.check({"y": yk[live]}, {"y": (yref[live], ey[live])}, dtype, what="slq_step " + c.what)
        # the block partials of |y|^2 against the sums of the kernel's own y
        P = Pout.cpu()
        assert bool(torch.isnan(P[:, nblk:]).all()) and bool(torch.isnan(P[still]).all()), "Pout written out of place"
        sums, cnt = sref.block_sums(e, yk)
        kref.check({"Pout": P[live][:, :nblk]}, {"Pout": (sums[live], (cnt + 4) * eps * sums[live])}, dtype,
                   what="slq_step Pout " + c.what)
        # T and the state
        Ta, Tb, col = Tal.cpu(), Tbe.cpu(), ref["col"]
        written = torch.zeros((S, NSTEPS), dtype=torch.bool)
        for s in range(S):
            if live[s]:
                written[s, col[s]] = True
        assert bool(torch.isnan(Ta[~written]).all()) and bool(torch.isnan(Tb[~written]).all()), "T written out of place"
        got = {"alpha": Ta[written], "beta": Tb[written]}
        want = {n: (ref[n][0][live], ref[n][1][live]) for n in ("alpha", "beta")}
        kref.check(got, want, dtype, what="slq_step T " + c.what)
        st = state.cpu()
        _same(st[k & 1], c.state[k & 1], "the state slot read")
        kref.check({"state": st[(k + 1) & 1]}, {"state": ref["state"]}, dtype, what="slq_step state " + c.what)
        for i in (sref.FLAG, sref.M):
            assert torch.equal(st[(k + 1) & 1][:, i], ref["state"][0][:, i]), "flags / step counts must be exactly equal"
        for t, h, n in ((W, c.W, "W"), (r2, c.r2, "r2"), (Pa, c.Pa, "Pa"), (Pin, c.Pin, "Pin")):
            _same(t, h, n)


# ------------------------------------------------------------------------------------------------ xk_slq_quad
def _lanczos_T(rng, m, kappa):
    """alpha (m,), beta (m,) (beta[0] = |z|) of m Lanczos steps on diag(geomspace(1, kappa, 4 m)), and |z|^2"""
    n = 4 * m
    lam = np.geomspace(1.0, kappa, n)
    z = rng.standard_normal(n)
    zz = float(z @ z)
    v, vp, b = z / math.sqrt(zz), np.zeros(n), 0.0
    al, be = np.zeros(m), np.zeros(m)
    be[0] = math.sqrt(zz)
    for j in range(m):
        w = lam * v
        al[j] = v @ w
        w = w - al[j] * v - b * vp
        b = float(np.linalg.norm(w))
        if j + 1 < m:
            be[j + 1] = b
        vp, v = v, w / b
    return al, be, zz


@pytest.mark.parametrize("S", [1, 70])
@pytest.mark.parametrize("nsteps", [1, 2, 3, 17, 64, 128])
def test_quad(nsteps, S):
    rng = np.random.default_rng(nsteps * 100 + S)
    k = nsteps & 1
    Tal = np.full((S, nsteps), math.nan)
    Tbe = np.full((S, nsteps), math.nan)
    state = np.full((2, S, sref.NST), math.nan)
    ms, zzs = [], []
    DECOUPLED, INDEFINITE = 5, 9
    for s in range(S):
        m = nsteps if s == 0 else 1 + (7 * s) % nsteps          # different m_s in one launch (s = 0: the full count)
        al, be, zz = _lanczos_T(rng, m, 1e2 if s % 2 else 1e6)
        if s == DECOUPLED and m >= 3:
            be[m // 2] = 0.0
        if s == INDEFINITE:
            al = al - (np.linalg.eigvalsh(sref.jacobi(al, be, m)).min() + 0.5)      # the smallest node is now -0.5
        Tal[s, :m], Tbe[s, :m] = al, be
        state[k, s] = 0.0
        state[k, s, sref.M], state[k, s, sref.ZNORM2] = m, zz
        ms.append(m)
        zzs.append(zz)
    dTal, dTbe, dst = (torch.from_numpy(a).to(DEV) for a in (Tal, Tbe, state))
    worst = 0.0
    for name, code in sref.FN_CODES.items():
        t = -0.01
        theta, weight, out, flag = K.slq_quad(dTal, dTbe, dst, k, code, t)
        theta2, weight2, out2, flag2 = K.slq_quad(dTal, dTbe, dst, k, code, t)
        for a, b in ((theta, theta2), (weight, weight2), (out, out2), (flag, flag2)):
            _same(a, b, "second run of xk_slq_quad")
        theta, weight, out, flag = theta.cpu().numpy(), weight.cpu().numpy(), out.cpu().numpy(), flag.cpu().numpy()
        for s in range(S):
            m, zz = ms[s], zzs[s]
            th, w2, ex, bound = sref.quad_truth(Tal[s], Tbe[s], m, zz, name, t)
            what = "xk_slq_quad %s nsteps=%d s=%d m=%d" % (name, nsteps, s, m)
            assert np.all(theta[s, m:] == 0) and np.all(weight[s, m:] == 0), what
            tn = np.abs(sref.jacobi(Tal[s], Tbe[s], m)).sum(1).max()
            order = np.argsort(theta[s, :m])
            assert np.all(np.abs(theta[s, :m][order] - th) <= sref.C_Q * m * sref.EPS64 * tn), what
            assert abs(weight[s, :m].sum() - 1.0) <= sref.C_Q * m * sref.EPS64, what
            if name in sref.NEEDS_POSITIVE and th.min() <= 0:
                assert s == INDEFINITE and flag[s] == 1 and math.isnan(out[s]), what
                continue
            assert flag[s] == 0, what
            assert abs(out[s] - ex) <= bound, "%s: got %r, want %r, bound %.3e" % (what, out[s], ex, bound)
            if bound > 0:
                worst = max(worst, abs(out[s] - ex) / bound)
        if S > INDEFINITE and name in sref.NEEDS_POSITIVE:
            assert flag[INDEFINITE] == 1 and np.count_nonzero(flag) == 1, "bit 0 for the indefinite system only"
    _same(dTal, torch.from_numpy(Tal), "Tal")
    _same(dTbe, torch.from_numpy(Tbe), "Tbe")
    _same(dst, torch.from_numpy(state), "state")
    print("xk_slq_quad nsteps = %d S = %d: worst error / bound %.3f" % (nsteps, S, worst))


def test_worst_ratio_report():
    """(runs last in this file) the largest |kernel - reference| / bound seen, per dtype"""
    for d, w in sorted(kref.WORST.items(), key=lambda kv: str(kv[0])):
        print("slq kernels: worst error / bound for %s: %.3f" % (d, w))
