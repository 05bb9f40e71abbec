"""-m gpu: xk_lobpcg_rotate_{f64,f32,c128,c64} per entry against tests/lobpcg_ref.py, inside NaN-filled buffers.

Every stack lives in a NaN-filled buffer with NaN margins on both sides, NaN pads [N, ld) and NaN rows from k on:
whatever the kernel must not read would poison the result, whatever it must not write is compared bit for bit
afterwards.  Shapes: N below, at and off the 16 B vector, below / at / above one wave, one and several column chunks
(4099 > 4 x 1024 floats); (k, q, w) from a single vector to the largest order, the first-iteration shape k = q and a
ragged one; one and three members with coefficients of their own; pitch pad_len(N) and pad_len(N) + 8 (vector form), a
base one element into its buffer and an odd pitch (scalar form); with and without the overlap stack; C with unit and
non-unit strides."""
import pytest
import torch
from tests import lobpcg_ref as lr
from xitorch_amd import kernels as K
from xitorch_amd.linalg._panel import pad_len

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.float64, torch.float32, torch.complex128, torch.complex64]
IDS = ["f64", "f32", "c128", "c64"]
NS = [1, 7, 8, 63, 64, 65, 257, 1000, 4099]
SHAPES = [(1, 1, 1), (2, 2, 1), (3, 2, 1), (6, 4, 2), (9, 6, 3), (13, 10, 5), (24, 16, 8), (48, 32, 16), (96, 64, 32)]
MARGIN = 64
XK_ERR_ARG = -1


def _bits(t):
    t = t.detach().cpu().contiguous()
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


class _Stack:
    """a (Bt, rows, ld) view `off` elements past MARGIN into a NaN-filled flat buffer; [:N] of rows [0, k) = `host`"""

    def __init__(self, host, rows, ld, off=0):
        Bt, k, N = host.shape
        self.N = N
        self.buf = torch.full((2 * MARGIN + off + Bt * rows * ld,), lr.nan_of(host.dtype), dtype=host.dtype, device=DEV)
        self.view = self.buf[MARGIN + off:MARGIN + off + Bt * rows * ld].view(Bt, rows, ld)
        self.view[:, :k, :N] = host.to(DEV)
        self.before = self.buf.clone()

    def only_rows_written(self, nrows):
        """everything but [:N] of rows [0, nrows) is bit-identical to what it was"""
        now, was = self.buf.clone(), self.before.clone()
        for t in (now, was):
            v = t[self.view.storage_offset():self.view.storage_offset() + self.view.numel()].view(self.view.shape)
            v[:, :nrows, :self.N] = 0
        return torch.equal(_bits(now), _bits(was))

    def host(self):
        return self.view[:, :, :self.N].cpu()


def _run(dtype, Bt, N, k, q, w, ld, with_m=True, cstrided=False, off=0, kind="randn", seed=0, twice=True):
    S, AS, MS, C, lam = lr.make_inputs(dtype, Bt, k, N, k, q, w, seed + N + 7 * k + Bt, kind, with_m)
    ref = lr.rotate(S, AS, MS, C, lam, k, q, w, dtype)
    rows = max(k, q + w) + 2
    what = "[%s Bt=%d N=%d (k,q,w)=(%d,%d,%d) ld=%d off=%d %s %s %s]" % (
        dtype, Bt, N, k, q, w, ld, off, kind, "M" if with_m else "noM", "Cstrided" if cstrided else "C")

    def once():
        ps, pa = _Stack(S, rows, ld, off), _Stack(AS, rows, ld, off)
        pm = _Stack(MS, rows, ld, off) if with_m else None
        if cstrided:
            Cbuf = torch.full((Bt, q + 1, k + 2), lr.nan_of(dtype), dtype=dtype, device=DEV)
            Cd = Cbuf.transpose(1, 2)[:, :k, :q]                     # strides (.., 1, k + 2)
        else:
            Cbuf = torch.full((Bt, k, q), lr.nan_of(dtype), dtype=dtype, device=DEV)
            Cd = Cbuf
        Cd.copy_(C.to(DEV))
        Cbefore = Cbuf.clone()
        lamd = torch.full((Bt, w + 1), float("nan"), dtype=torch.float64, device=DEV)
        lamd[:, :w] = lam.to(DEV)
        lam_before = lamd.clone()
        Pn, Pm = K.lobpcg_rotate(ps.view, pa.view, pm.view if with_m else None, Cd, lamd, k, q, w, N=N)
        torch.cuda.synchronize()
        assert Pn.shape == (Bt, w, ref.nblk) and Pm.shape == (Bt, ref.nblk), what
        assert ps.only_rows_written(q + w), "S: pads, margins or rows >= q + w written " + what
        assert pa.only_rows_written(q), "AS: pads, margins or rows >= q written " + what
        assert pm is None or pm.only_rows_written(q), "MS: pads, margins or rows >= q written " + what
        assert torch.equal(_bits(Cbuf), _bits(Cbefore)) and torch.equal(_bits(lamd), _bits(lam_before)), what
        return ps.host(), pa.host(), pm.host() if with_m else None, Pn.cpu(), Pm.cpu()

    S1, AS1, MS1, Pn, Pm = once()
    ratio = lr.check_all(ref, S1, AS1, MS1, Pn, Pm, q, w, what)
    if twice:
        again = once()
        for a, b in zip((S1[:, :q + w], AS1[:, :q], Pn, Pm), (again[0][:, :q + w], again[1][:, :q], again[3], again[4])):
            assert torch.equal(_bits(a), _bits(b)), "two runs differ " + what
    return ratio, (S1, AS1, MS1), ref


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("shape", SHAPES, ids=["%d-%d-%d" % s for s in SHAPES])
def test_rotate_per_entry(dtype, N, shape):
    """all shapes; members, pitch, overlap stack and coefficient strides alternate over the grid so that each option meets
    every N and every (k, q, w), and a second run with every option flipped follows where the case is small"""
    k, q, w = shape
    i = NS.index(N) * len(SHAPES) + SHAPES.index(shape)
    opts = dict(Bt=3 if i % 2 else 1, ld=pad_len(N) + 8 * ((i // 2) % 2), with_m=(i // 4) % 2 == 0,
                cstrided=(i // 8) % 2 == 1)
    small = k * q * N <= 24 * 16 * 4099
    worst, _, _ = _run(dtype, opts["Bt"] if small or N < 1000 else 1, N, k, q, w, opts["ld"], opts["with_m"],
                       opts["cstrided"])
    if small:
        flip = dict(Bt=4 - opts["Bt"], ld=2 * pad_len(N) + 8 - opts["ld"], with_m=not opts["with_m"],
                    cstrided=not opts["cstrided"])
        r, _, _ = _run(dtype, flip["Bt"], N, k, q, w, flip["ld"], flip["with_m"], flip["cstrided"], twice=False)
        worst = max(worst, r)
    print("worst |err| / bound %s N=%d (k,q,w)=%s: %.3f" % (dtype, N, shape, worst))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", [7, 65, 1000, 4099])
def test_unaligned_base_and_odd_pitch_take_the_scalar_form(dtype, N):
    worst = 0.0
    for (k, q, w), with_m in (((3, 2, 1), True), ((9, 6, 3), False), ((24, 16, 8), True), ((48, 32, 16), False)):
        r1, _, _ = _run(dtype, 2, N, k, q, w, pad_len(N), with_m, off=1, twice=False)
        r2, _, _ = _run(dtype, 3, N, k, q, w, N + 1 if N % 2 == 0 else N, with_m, cstrided=True, twice=False)
        worst = max(worst, r1, r2)
    r3, _, _ = _run(dtype, 1, N, 96, 64, 32, pad_len(N), True, off=1, twice=False)
    print("worst |err| / bound (scalar form) %s N=%d: %.3f" % (dtype, N, max(worst, r3)))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["graded", "cancel"])
def test_graded_and_cancelling_inputs(dtype, kind):
    for N in (65, 1000):
        for (k, q, w) in ((9, 6, 3), (24, 16, 8), (48, 32, 16)):
            _run(dtype, 2, N, k, q, w, pad_len(N), with_m=(k != 24), kind=kind, twice=False)
            _run(dtype, 2, N, k, q, w, pad_len(N), with_m=(k == 24), kind=kind, off=1, twice=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_integer_inputs_come_back_exact(dtype):
    for N in (63, 1000):
        for (k, q, w), off in (((9, 6, 3), 0), ((24, 16, 8), 1), ((96, 64, 32), 0)):
            for with_m in (True, False):
                _, (S1, AS1, MS1), ref = _run(dtype, 2, N, k, q, w, pad_len(N), with_m, kind="integer", off=off,
                                              twice=False)
                for name, t in (("S", S1), ("AS", AS1), ("MS", MS1)):
                    if t is not None:
                        assert torch.equal(lr.as_real64(t[:, :q]), ref.stacks[name][0]), name
                assert torch.equal(lr.as_real64(S1[:, q:q + w]), ref.resid[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_refusals_launch_nothing(dtype):
    N, ld, (k, q, w) = 65, pad_len(65), (9, 6, 3)
    S, AS, MS, C, lam = lr.make_inputs(dtype, 2, k, N, k, q, w, 1)
    ps, pa, pm = _Stack(S, 11, ld), _Stack(AS, 11, ld), _Stack(MS, 11, ld)
    Cd, lamd = C.to(DEV), lam.to(DEV)
    Pn = torch.zeros((2, 3, 1), dtype=torch.float64, device=DEV)
    Pm = torch.zeros((2, 1), dtype=torch.float64, device=DEV)

    def rc(S_=ps.view, A_=pa.view, M_=pm.view, k_=k, q_=q, w_=w, N_=N):
        return K.lobpcg_rotate(S_, A_, M_, Cd, lamd, k_, q_, w_, N=N_, Pnorm=Pn, Pmax=Pm, raw=True)

    assert rc(q_=2) == XK_ERR_ARG and rc(q_=10) == XK_ERR_ARG
    assert rc(k_=K.lobpcg_max_rows() + 1) == XK_ERR_ARG
    assert rc(w_=0) == XK_ERR_ARG and rc(w_=-1) == XK_ERR_ARG
    assert rc(N_=0) == XK_ERR_ARG and rc(N_=-5) == XK_ERR_ARG
    assert rc(N_=ld + 1) == XK_ERR_ARG                                     # a pitch below N
    short = ps.buf[MARGIN:MARGIN + 2 * 8 * ld].view(2, 8, ld)              # a stack stride below (q + w) * pitch
    assert rc(S_=short) == XK_ERR_ARG and rc(A_=short) == XK_ERR_ARG and rc(M_=short) == XK_ERR_ARG
    torch.cuda.synchronize()
    for p in (ps, pa, pm):
        assert torch.equal(_bits(p.buf), _bits(p.before))
    # and the same call, legal, goes through
    assert rc() == 0
    torch.cuda.synchronize()
    ref = lr.rotate(S, AS, MS, C, lam, k, q, w, dtype)
    lr.check_all(ref, ps.host(), pa.host(), pm.host(), Pn.cpu(), Pm.cpu(), q, w, "after the refusals")
