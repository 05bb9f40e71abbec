"""-m gpu: the banded operator apply xk_banded_mm (xk_krylov.hip) in float64 and float32 against the reference of
tests/banded_ref.py, entry by entry with the dtype-derived bound (shared configurations with the CPU fault test
tests/test_banded_ref.py).

The kernel is driven through `K.banded_mm(..., out=Y)` on strided views of NaN-filled buffers with NaN in every
out-of-matrix band entry, through the C entry points with a padded band batch stride, at the LDS limit, and through
BandedLinearOperator.  Every case also checks what must NOT change: the output buffer outside Y's (B, C, N) entries
and the operands come back bit-identical."""
import pytest
import torch
import xitorch_amd as xa
from tests import banded_ref as br
from xitorch_amd import kernels as K
from xitorch_amd._capi import NativeLibraryError, ptr, stream_ptr, suffix
from xitorch_amd.linop import banded_apply_torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = br.DTYPES
IDS = [br.DNAME[d] for d in DTYPES]
XK_OK = 0


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _run(dtype, c, what, launch=None):
    """one launch on device copies of the buffers of case `c` (default: K.banded_mm(band, X, out=Y)): Y against the
    reference, the rest of its buffer and the operands bit-identical.  Returns the output buffer on the host."""
    cfg = c["cfg"]
    bbuf, xbuf, ybuf = c["bbuf"].to(DEV), c["xbuf"].to(DEV), c["ybuf"].to(DEV)
    band = br.view_like(bbuf, c["band"])
    X, Y = br.view_like(xbuf, c["X"]), br.view_like(ybuf, c["Y"])
    if launch is None:
        assert K.banded_mm(band, X, out=Y, trans=cfg.trans) is Y
    else:
        launch(band, X, Y)
    torch.cuda.synchronize()
    yh = ybuf.cpu()
    got = br.view_like(yh, c["Y"]).clone()
    br.check({"Y": got}, br.ref(dtype, c), br.KERNEL, dtype, what)
    want = c["ybuf"].clone()
    br.view_like(want, c["Y"]).copy_(got)
    assert _same_bits(yh, want), what + ": written outside Y"
    assert _same_bits(xbuf, c["xbuf"]) and _same_bits(bbuf, c["bbuf"]), what + ": an operand changed"
    return yh


# ================================================================================================ reference check
CASES = [(d, cfg) for d in DTYPES for cfg in br.configs(d)]


@pytest.mark.parametrize("dtype,cfg", CASES, ids=["%s-%s" % (br.DNAME[d], "-".join(str(int(v)) for v in c))
                                                  for d, c in CASES])
def test_banded_mm_vs_reference(dev, dtype, cfg):
    """Y entry by entry, its buffer untouched elsewhere (wholly so for C = 0 and N = 0), and a second call with the
    same arguments bit-identical"""
    c = br.case(dtype, cfg)
    what = "banded_mm %s %s" % (br.DNAME[dtype], cfg)
    if cfg.offset:
        band = br.view_like(c["bbuf"].to(DEV), c["band"])
        assert band.data_ptr() % 16 != 0 and cfg.N % br.VEC_ELEMS[dtype] == 0
    yh = _run(dtype, c, what)
    if cfg.C == 0 or cfg.N == 0:
        assert _same_bits(yh, c["ybuf"]), what + ": an empty apply wrote something"
    assert _same_bits(_run(dtype, c, what), yh), what + ": not deterministic"


# ================================================================================================ C entry points
@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("pad", ["scalar", "vector"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_banded_mm_padded_band_stride(dev, dtype, pad, trans):
    """xk_banded_mm_f64 / _f32 with a band batch stride beyond nd N: nd N + 1 (scalar band loads) and nd N + VN
    (vector loads), the gap NaN; two row tiles"""
    vn = br.VEC_ELEMS[dtype]
    cfg = br.Cfg(br.rows_of(dtype) + vn, 5, 3, 3, False, trans, False)
    c = br.case(dtype, cfg)
    N, nd, B, C = cfg.N, 2 * cfg.hb + 1, cfg.B, cfg.C
    sBand = nd * N + (1 if pad == "scalar" else vn)
    wide = br._nan((B * sBand,), dtype)
    wide.as_strided((B, nd, N), (sBand, N, 1)).copy_(c["band"])
    wide = wide.to(DEV)

    def launch(band, X, Y):
        rc = K.fn("xk_banded_mm_" + suffix(dtype))(ptr(wide), ptr(X), ptr(Y), B, N, cfg.hb, C, sBand, X.stride(1),
                                                   X.stride(0), Y.stride(1), Y.stride(0), 1 if trans else 0,
                                                   stream_ptr())
        assert rc == XK_OK
    assert wide.data_ptr() % 16 == 0 and N % vn == 0 and (sBand % vn == 0) == (pad == "vector")
    _run(dtype, c, "xk_banded_mm_%s sBand = nd N + %d trans=%s" % (suffix(dtype), sBand - nd * N, trans), launch)


# ================================================================================================ LDS limit
WIDE_HB = {torch.float64: 1100, torch.float32: 2100}        # 7 columns of ROWS + 2 hb elements fit 160 KiB, 8 do not
TOO_WIDE_HB = {torch.float64: 10000, torch.float32: 20000}  # one column does not fit


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("C", [7, 8, 9])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_banded_mm_wide_band_any_column_count(dev, dtype, C, trans):
    """a band whose halo leaves room for 7 columns in the LDS is applied to 7, 8 and 9 columns alike: the column
    chunk shrinks to what fits instead of the launch being refused"""
    hb, R, es = WIDE_HB[dtype], br.rows_of(dtype), 16 // br.VEC_ELEMS[dtype]
    assert 7 * (R + 2 * hb) * es <= br.LDS_LIMIT < 8 * (R + 2 * hb) * es
    cfg = br.Cfg(300, hb, C, 1, False, trans, False)
    _run(dtype, br.case(dtype, cfg), "banded_mm %s %s" % (br.DNAME[dtype], cfg))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_banded_mm_too_wide_band_is_refused(dev, dtype):
    """(ROWS + 2 hb) sizeof(T) > 160 KiB: not even one column fits; NativeLibraryError and `out` left alone"""
    hb, N = TOO_WIDE_HB[dtype], 64
    assert (br.rows_of(dtype) + 2 * hb) * (16 // br.VEC_ELEMS[dtype]) > br.LDS_LIMIT
    band = torch.ones((1, 2 * hb + 1, N), dtype=dtype, device=DEV)
    X = torch.ones((1, 1, N), dtype=dtype, device=DEV)
    for C in (1, 9):
        out = br._nan((1, C, N), dtype).to(DEV)
        with pytest.raises(NativeLibraryError):
            K.banded_mm(band, X.expand(1, C, N).contiguous(), out=out)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())


# ================================================================================================ wrapper validation
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_banded_mm_wrapper_refuses_bad_arguments(dev, dtype):
    """each refused on the host, before anything is launched: `out` keeps its NaN"""
    B, C, N, hb = 3, 2, 40, 2
    nd = 2 * hb + 1
    other = torch.float32 if dtype == torch.float64 else torch.float64
    z = lambda *shape, dt=dtype: torch.zeros(shape, dtype=dt, device=DEV)
    band, X = z(B, nd, N), z(B, C, N)
    flat = br._nan((B * C * N + 8,), dtype).to(DEV)
    good = flat[:B * C * N].view(B, C, N)
    bad = {
        "band batch neither 1 nor B": dict(band=z(2, nd, N)),
        "band batch above B": dict(band=z(4, nd, N)),
        "band dtype": dict(band=z(B, nd, N, dt=other)),
        "band of 4 dims": dict(band=z(1, B, nd, N)),
        "out shape (N)": dict(out=flat[:B * C * (N - 1)].view(B, C, N - 1)),
        "out shape (C)": dict(out=flat[:B * (C - 1) * N].view(B, C - 1, N)),
        "out shape (B)": dict(out=flat[:(B - 1) * C * N].view(B - 1, C, N)),
        "out dtype": dict(out=z(B, C, N, dt=other)),
        "out device": dict(out=torch.zeros((B, C, N), dtype=dtype)),
        "out row pitch < N": dict(out=flat.as_strided((B, C, N), (C * N, N - 1, 1))),
        "out batch members overlap": dict(out=flat.as_strided((B, C, N), (N, N, 1))),
        "out batch stride 0": dict(out=good[:1].expand(B, C, N)),
    }
    for name, kw in bad.items():
        args = dict(band=band, out=good)
        args.update(kw)
        try:
            K.banded_mm(args["band"], X, out=args["out"])
        except NativeLibraryError:
            continue
        pytest.fail("banded_mm accepted: " + name)
    torch.cuda.synchronize()
    assert bool(torch.isnan(flat).all())
    # what must stay accepted: a batch-1 band with B = 1, a broadcast band (3-D of batch 1, or 2-D), `out` whose batch
    # index is the faster one
    ones = torch.ones((1, nd, N), dtype=dtype, device=DEV)
    x = torch.ones((B, C, N), dtype=dtype, device=DEV)
    want = K.banded_mm(ones.expand(B, nd, N).contiguous(), x)
    assert torch.equal(K.banded_mm(ones, x), want) and torch.equal(K.banded_mm(ones[0], x), want)
    assert torch.equal(K.banded_mm(ones, x[:1]), want[:1])
    inter = torch.zeros((C, B, N), dtype=dtype, device=DEV).transpose(0, 1)
    assert torch.equal(K.banded_mm(ones, x, out=inter), want)


# ================================================================================================ operator level
# (band batch, x batch): () x (4,) folds the whole x batch into columns; (3,) x (2, 3) and (2, 1) x (2, 3) keep one
# batch index and fold the other (the keep / fold permutation of linop._banded_native)
OP_BATCHES = [((), (4,)), ((3,), (3,)), ((3,), (2, 3)), ((2, 1), (2, 3))]


@pytest.mark.parametrize("layout", ["contiguous", "sliced", "transposed"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_banded_operator_vs_torch_apply(dev, dtype, layout):
    """BandedLinearOperator.mm / mv / rmm / rmv against linop.banded_apply_torch on the host in float64, entry by
    entry with the bound of the broadcast operands; the band also as a non-contiguous view (every other column of a
    wider array / stored diagonal-fastest)"""
    N, hb, r = 131, 5, 3
    nd = 2 * hb + 1
    for BA, BX in OP_BATCHES:
        g = br._gen(13, len(BA), len(BX), DTYPES.index(dtype))
        nb = 1
        for n in BA:
            nb *= n
        band = br.make_band(g, dtype, nb, hb, N)[2].reshape(*BA, nd, N)
        x = br._randn(g, *BX, N, r).to(dtype)
        bd = band.to(DEV)
        if layout == "sliced":
            wide = torch.full((*BA, nd, 2 * N), 7.0, dtype=dtype, device=DEV)
            wide[..., ::2] = bd
            bd = wide[..., ::2]
        if layout == "transposed":
            bd = bd.transpose(-2, -1).contiguous().transpose(-2, -1)
        assert torch.equal(bd.cpu().nan_to_num(nan=3.0), band.nan_to_num(nan=3.0))
        assert bd.is_contiguous() == (layout == "contiguous")
        op = xa.BandedLinearOperator(bd, is_hermitian=False)
        for trans in (False, True):
            what = "BandedLinearOperator %s band %s x %s %s trans=%s" % (br.DNAME[dtype], BA, BX, layout, trans)
            ref = br.operator_ref(dtype, band, x, trans)
            want = banded_apply_torch(band.double(), x.double(), trans)
            ref = {"Y": (want, ref["Y"][1])}
            got = (op.rmm if trans else op.mm)(x.to(DEV))
            assert got.shape == want.shape and got.dtype == dtype
            br.check({"Y": got}, ref, "banded_operator", dtype, what + " mm")
            gv = (op.rmv if trans else op.mv)(x[..., 0].to(DEV))
            refv = {"Y": (want[..., 0], ref["Y"][1][..., 0])}
            assert gv.shape == want.shape[:-1]
            br.check({"Y": gv}, refv, "banded_operator", dtype, what + " mv")


def test_report_worst_ratios(dev):
    """the largest |kernel - reference| / bound per kernel and dtype seen by this module's checks (run last)"""
    mine = {k: v for k, v in br.WORST.items() if k[0] in (br.KERNEL, "banded_operator")}
    for key in sorted(mine):
        print("WORST %s %s: %.3f" % (key[0], key[1], mine[key]))
    assert all(v <= 1.0 for v in mine.values())
