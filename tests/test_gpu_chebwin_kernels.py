"""-m gpu: xk_cheb_clenshaw_{f64,f32,c128,c64} per entry against tests/chebwin_ref.py, inside NaN-filled buffers.

The pattern of tests/test_gpu_cheb_kernels.py.  Every panel lives in a NaN-filled buffer with NaN margins on both sides
and NaN pads [N, ld): whatever the kernel must not read would poison the result, whatever it must not write is compared
bit for bit afterwards.  Shapes: N below, at and off the 16 B vector, below / at / above one 64-lane wave, several chunks
of a row (4099 > 4 x 256 x 4 floats), p and Bt so that the grid has many rows; pitch pad_len(N) and pad_len(N) + 8
(vector form), and a base pointer one element into its buffer / an odd pitch (scalar form).  (On the parent commit
the entry point does not exist.)"""
import pytest
import torch
from tests import chebwin_ref as wref
from xitorch_amd import kernels as K
from xitorch_amd.linalg._panel import pad_len

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.float64, torch.float32, torch.complex128, torch.complex64]
IDS = ["f64", "f32", "c128", "c64"]
NS = [1, 7, 8, 63, 64, 65, 257, 1000, 4099]
MARGIN = 64
XK_ERR_ARG = -1


def _bits(t):
    t = t.detach().cpu().contiguous()
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


class _Panel:
    """a (Bt, p, ld) view `off` elements past MARGIN into a NaN-filled flat buffer; [:N] of every row = `host`"""

    def __init__(self, host, ld, off=0):
        Bt, p, N = host.shape
        self.N = N
        self.buf = torch.full((2 * MARGIN + off + Bt * p * ld,), wref.nan_of(host.dtype), dtype=host.dtype, device=DEV)
        self.view = self.buf[MARGIN + off:MARGIN + off + Bt * p * ld].view(Bt, p, ld)
        self.view[:, :, :N] = host.to(DEV)
        self.before = self.buf.clone()

    def unchanged(self):
        return torch.equal(_bits(self.buf), _bits(self.before))

    def only_rows_written(self):
        """everything but [:N] of the rows is bit-identical to what it was (NaN)"""
        now, was = self.buf.clone(), self.before.clone()
        for t in (now, was):
            v = t[self.view.storage_offset():self.view.storage_offset() + self.view.numel()].view(self.view.shape)
            v[:, :, :self.N] = 0
        return torch.equal(_bits(now), _bits(was))


def _run(dtype, Bt, p, N, ld, kind="randn", alias=True, off=0, coef_edit=None, seed=0, yprev_nan=False):
    AY, Y, Yp, X0, coef = wref.make_inputs(dtype, Bt, p, N, seed=seed + N + 7 * p + Bt, kind=kind)
    if coef_edit is not None:
        coef_edit(coef)
    if yprev_nan:
        Yp.fill_(wref.nan_of(dtype))
    value, bound = wref.step(AY, Y, Yp, X0, coef, dtype)
    pa, py, pp, px = _Panel(AY, ld, off), _Panel(Y, ld, off), _Panel(Yp, ld, off), _Panel(X0, ld, off)
    po = pp if alias else _Panel(torch.full_like(AY, wref.nan_of(dtype)), ld, off)
    cd = coef.to(DEV)
    K.cheb_clenshaw(pa.view, py.view, pp.view, px.view, cd, out=None if alias else po.view, N=N)
    torch.cuda.synchronize()
    what = "[%s Bt=%d p=%d N=%d ld=%d off=%d %s %s]" % (dtype, Bt, p, N, ld, off, kind, "alias" if alias else "apart")
    ratio = wref.check(po.view[:, :, :N], value, bound, what)
    assert po.only_rows_written(), "pads / neighbours of out written " + what
    assert pa.unchanged() and py.unchanged() and px.unchanged(), "an input changed " + what
    if not alias:
        assert pp.unchanged(), "Yprev changed " + what
    assert torch.equal(cd.cpu(), coef), "coef changed " + what
    return ratio, po.view[:, :, :N].cpu(), value


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", NS)
def test_step_per_entry(dtype, N):
    """all shapes, both pitches, out over Yprev and apart, distinct coefficients per operator"""
    worst = 0.0
    for p in (1, 3, 16, 33):
        for Bt in (1, 3):
            for k, ld in enumerate((pad_len(N), pad_len(N) + 8)):
                r, _, _ = _run(dtype, Bt, p, N, ld, alias=(p + Bt + k) % 2 == 0)
                worst = max(worst, r)
    print("worst |err| / bound %s N=%d: %.3f" % (dtype, N, worst))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", [7, 65, 1000, 4099])
def test_unaligned_base_takes_the_scalar_form(dtype, N):
    """a base pointer one element into its buffer, and an odd pitch: same result contract"""
    for alias in (True, False):
        _run(dtype, 3, 3, N, pad_len(N), alias=alias, off=1)
        _run(dtype, 2, 5, N, N + 1 if N % 2 == 0 else N, alias=alias, off=0)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", [8, 65, 4099])
def test_gamma_zero_does_not_read_yprev(dtype, N):
    """gamma == 0 (+0 and -0) with Yprev all NaN: the result stays finite, in both forms"""
    def edit(c):
        c[:, 2] = 0.0
        c[-1, 2] = -0.0
    for alias in (True, False):
        _, got, _ = _run(dtype, 3, 3, N, pad_len(N), alias=alias, coef_edit=edit, yprev_nan=True)
        assert bool(torch.isfinite(torch.view_as_real(got) if got.is_complex() else got).all())
        _, got, _ = _run(dtype, 2, 2, N, pad_len(N), alias=alias, off=1, coef_edit=edit, yprev_nan=True)
        assert bool(torch.isfinite(torch.view_as_real(got) if got.is_complex() else got).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_zero_coefficients_and_mixed_members(dtype):
    """one member with gamma = 0 beside members that read Yprev; alpha, beta, delta = +-0 get no special treatment"""
    def edit(c):
        c[0, 2] = 0.0
        c[1, 0], c[1, 3] = 0.0, -0.0
        c[2, 1] = -0.0
    for N in (7, 257, 4099):
        _run(dtype, 3, 3, N, pad_len(N), coef_edit=edit)
        _run(dtype, 3, 3, N, pad_len(N), coef_edit=edit, alias=False, off=1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_graded_inputs(dtype):
    for N in (65, 1000):
        for alias in (True, False):
            _run(dtype, 3, 3, N, pad_len(N), kind="graded", alias=alias)
            _run(dtype, 2, 3, N, pad_len(N), kind="graded", alias=alias, off=1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_integer_inputs_come_back_exact(dtype):
    for N in (63, 1000):
        for off in (0, 1):
            _, got, value = _run(dtype, 3, 16, N, pad_len(N), kind="integer", off=off)
            assert torch.equal(wref.as_real64(got), value)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_runs_are_bit_identical(dtype):
    for N, off in ((4099, 0), (1000, 1)):
        _, a, _ = _run(dtype, 3, 16, N, pad_len(N), off=off, seed=5)
        _, b, _ = _run(dtype, 3, 16, N, pad_len(N), off=off, seed=5)
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_refusals_launch_nothing(dtype):
    """out over AY, Y or X0 (whole or partly), over a Yprev it is not, rows of out that overlap, N <= 0: XK_ERR_ARG, no
    buffer changes"""
    N, ld = 65, pad_len(65)
    AY, Y, Yp, X0, coef = wref.make_inputs(dtype, 2, 3, N, seed=1)
    pa, py, pp, px = _Panel(AY, ld), _Panel(Y, ld), _Panel(Yp, ld), _Panel(X0, ld)
    cd = coef.to(DEV)
    args = (pa.view, py.view, pp.view, px.view, cd)
    for src in (pa, py, px):
        assert K.cheb_clenshaw(*args, out=src.view, N=N, raw=True) == XK_ERR_ARG
        # a shifted view: not the same pointer, overlapping all the same
        shifted = src.buf[MARGIN + 8:MARGIN + 8 + 2 * 3 * ld].view(2, 3, ld)
        assert K.cheb_clenshaw(*args, out=shifted, N=N, raw=True) == XK_ERR_ARG
    # out overlapping Yprev without being it
    shifted_p = pp.buf[MARGIN + 8:MARGIN + 8 + 2 * 3 * ld].view(2, 3, ld)
    assert K.cheb_clenshaw(*args, out=shifted_p, N=N, raw=True) == XK_ERR_ARG
    # rows of out that overlap each other: every member of the batch at one address, a batch stride inside a member
    po = _Panel(torch.full_like(AY, wref.nan_of(dtype)), ld)
    assert K.cheb_clenshaw(*args, out=po.view[:1].expand(2, 3, ld), N=N, raw=True) == XK_ERR_ARG
    assert K.cheb_clenshaw(*args, out=po.buf[MARGIN:MARGIN + 4 * ld].as_strided((2, 3, ld), (ld, ld, 1)), N=N,
                           raw=True) == XK_ERR_ARG
    assert K.cheb_clenshaw(*args, N=0, raw=True) == XK_ERR_ARG
    assert K.cheb_clenshaw(*args, N=-3, raw=True) == XK_ERR_ARG
    torch.cuda.synchronize()
    assert pa.unchanged() and py.unchanged() and pp.unchanged() and px.unchanged() and po.unchanged()
    # and the same call, legal, goes through
    assert K.cheb_clenshaw(*args, N=N, raw=True) == 0
    torch.cuda.synchronize()
    value, bound = wref.step(AY, Y, Yp, X0, coef, dtype)
    wref.check(pp.view[:, :, :N], value, bound, "after the refusals")
