"""Float64 restatement of the banded operator apply xk_banded_mm (xk_krylov.hip), with a per-entry error bound.

It follows the contract of tests/solver_ref.py and uses its `check`, `WORST`, `REF` and generators: `banded_mm`
computes, from the very operands the kernel is given, what the kernel must write and returns {"Y": (value, bound)}.
The value is written from the definition in the kernel's header comment,

    not transposed:  y[b,c,i] = sum_d band[b,d,i] x[b,c,i+d-hb]
    transposed:      y[b,c,j] = sum_d band[b,d,j-(d-hb)] x[b,c,j-(d-hb)]

where an entry band[b,d,i] = A_b[i, i+d-hb] whose column i + d - hb falls outside [0, N) is no entry of the matrix
and contributes nothing, whatever is stored there (the cases below store NaN there).

The `fault=` argument produces plausible kernel bugs (FAULTS); tests/test_banded_ref.py feeds those outputs to
`check()` at every configuration of the GPU test tests/test_gpu_banded_kernel.py (`configs` and `case` below are
shared by both) and asserts that each is rejected wherever VISIBLE says it can be seen."""
import collections
import math
import torch
from tests.krylov_ref import unit_roundoff, hp, VEC_ELEMS
from tests.solver_ref import check, WORST, REF, DNAME, DTYPES, _gen, _randn, _nan     # noqa: F401 (re-exported)

KERNEL = "banded_mm"
FAULTS = ("mask_dropped", "halo_shift", "tile_halo_zero", "trans_ignored", "tail_rows_dropped",
          "second_chunk_dropped", "band_batch_ignored", "pitch_ignored")
CHUNK = 8                       # columns per launch of banded_mm (fewer only where 8 do not fit the LDS)
LDS_LIMIT = 160 * 1024          # bytes of LDS a workgroup can get on gfx950


def rows_of(dtype):
    """rows per block: 256 threads, one 16-byte vector of consecutive rows each"""
    return 256 * VEC_ELEMS[dtype]


def in_matrix(hb, N):
    """(nd, N) mask: is band[d, i] = A[i, i + d - hb] an entry of the N x N matrix?"""
    col = torch.arange(N).unsqueeze(0) + torch.arange(2 * hb + 1).unsqueeze(1) - hb
    return (col >= 0) & (col < N)


def _apply(band, x, hb, trans, magnitudes=False, shift=0, tile=None):
    """sum over the in-matrix entries of every diagonal; band (1 or B, nd, N), x (B, C, N), float64.  magnitudes: the
    sum of |band x| and the number of terms t (N,) instead.  shift / tile model the faults halo_shift (x read one
    element further on, zero past the end) and tile_halo_zero (x outside the output row's tile of `tile` rows is 0)."""
    B, C, N = x.shape
    y = torch.zeros((B, C, N), dtype=torch.float64)
    t = torch.zeros(N, dtype=torch.float64)
    if shift:
        x = torch.cat([x[:, :, shift:], torch.zeros((B, C, min(shift, N)), dtype=torch.float64)], dim=2)
    if magnitudes:
        band, x = band.abs(), x.abs()
    for d in range(max(0, hb - N + 1), min(2 * hb + 1, hb + N)):         # the diagonals that cross the matrix
        off = d - hb
        lo, hi = max(0, -off), min(N, N - off)                            # rows i with 0 <= i + off < N
        coef = band[:, d, lo:hi].unsqueeze(1)
        # not transposed: row i takes x[i + off]; transposed: row j = i + off takes x[i]
        src, dst = ((lo + off, hi + off), (lo, hi)) if not trans else ((lo, hi), (lo + off, hi + off))
        term = coef * x[:, :, src[0]:src[1]]
        if tile is not None:
            same = (torch.arange(*src) // tile) == (torch.arange(*dst) // tile)
            term = term * same
        y[:, :, dst[0]:dst[1]] += term
        t[dst[0]:dst[1]] += 1
    return (y, t) if magnitudes else y


# The kernel forms the t in-matrix terms of an entry in order of d and adds each to one accumulator that starts at an
# exact zero: one rounding per product and one per addition (none where the compiler contracts them into a fused
# multiply-add, none for the terms it masks: those add an exact zero).  A term therefore carries at most t roundings,
# |err| <= ((1 + u)^t - 1) sum |band x|, below (t + 1) u sum |band x| for every t u < 0.1 (t <= 4201, u <= 2^-24
# here).  REF doubles it for the float64 reference's own sum of the same length.
def banded_mm(dtype, band, X, hb, trans, fault=None):
    """xk_banded_mm: band (1 or B, 2 hb + 1, N) and the logical panel X (B, C, N) in the kernel dtype (X may be a
    strided view: the fault pitch_ignored re-reads its storage at pitch N).  Returns {"Y": (value, bound)}, (B, C, N);
    for a fault the bound is 0 (only the value is of use).  Entries the faulty kernel would not write hold NaN: the
    sentinel they keep."""
    B, C, N = X.shape
    bh = torch.nan_to_num(hp(band), nan=0.0) * in_matrix(hb, N)           # what is stored outside is never used
    if fault == "pitch_ignored" and B * C * N > 0:
        X = X.as_strided((B, C, N), (X.stride(0), N, 1))
    xh = hp(X)
    if fault == "band_batch_ignored":
        bh = bh[:1]
    kw = {}
    if fault == "halo_shift":
        kw["shift"] = 1
    if fault == "tile_halo_zero":
        kw["tile"] = rows_of(dtype)
    val = _apply(bh, xh, hb, trans and fault != "trans_ignored", **kw)
    if fault == "mask_dropped" and hb > 0:
        # rows with an out-of-matrix entry on some diagonal: NaN (stored) times the zero-filled halo
        r = torch.arange(N)
        val[:, :, (r < hb) | (r >= N - hb)] = math.nan
    if fault == "tail_rows_dropped":
        vn, rows = VEC_ELEMS[dtype], rows_of(dtype)
        val[:, :, (N // vn * vn if N % vn else N // rows * rows):] = math.nan
    if fault == "second_chunk_dropped":
        val[:, CHUNK:] = math.nan
    if fault is not None:
        return {"Y": (val, torch.zeros_like(val))}
    mag, t = _apply(bh, xh, hb, trans, magnitudes=True)
    return {"Y": (val, REF * (t + 1) * unit_roundoff(dtype) * mag)}


# ================================================================================================ configurations
Cfg = collections.namedtuple("Cfg", "N hb C B bcast trans offset")


def configs(dtype):
    """The smallest shapes at which each path of the kernel can go wrong, each with both `trans`:
    N around one row tile (ROWS = 512 / 1024) and beyond two, a multiple of the vector width VN (vector band loads)
    or not (scalar), tiny N below hb; hb = 0 up to 600 (8 columns of ROWS + 2 hb elements then exceed 64 KiB: the
    launch has to ask for them; there B <= 2 so that the band stays below 20 MB); C = 0, one chunk, exactly 8, a
    second chunk, a third; B = 1 or 3 with a band per member or one broadcast (bcast); offset: the band starts one
    element into its allocation (not 16-byte aligned: scalar loads although N % VN = 0)."""
    R, vn = rows_of(dtype), VEC_ELEMS[dtype]
    big, mult = 2 * R + vn + 1, 2 * R + vn
    base = [(0, 1, 3, 1, False), (1, 0, 1, 1, False), (1, 5, 3, 3, True), (2, 1, 8, 3, False), (2, 5, 1, 3, False),
            (3, 1, 9, 1, False), (3, 0, 17, 3, True), (50, 63, 3, 3, False), (50, 5, 0, 3, False),
            (50, 5, 17, 1, False), (50, 1, 9, 3, False), (R - 1, 5, 3, 3, False), (R - 1, 63, 9, 1, False),
            (R, 1, 1, 3, True), (R, 63, 8, 3, False), (R, 600, 17, 2, False), (R + 1, 1, 3, 3, False),
            (R + 1, 63, 17, 1, False), (R + 1, 0, 8, 3, True), (big, 5, 9, 3, False), (big, 63, 1, 3, True),
            (big, 600, 8, 1, False), (mult, 5, 8, 3, False), (mult, 63, 17, 3, True), (mult, 600, 8, 2, True),
            (mult, 0, 3, 1, False), (2 * R + 3, 1, 3, 1, False)]
    cfg = [Cfg(*b, trans, False) for b in base for trans in (False, True)]
    cfg += [Cfg(R, 5, 3, 1, False, trans, True) for trans in (False, True)]
    return cfg


def make_band(g, dtype, nb, hb, N, offset=False):
    """contiguous (nb, 2 hb + 1, N) band, every diagonal of every member at its own scale 10^-3 .. 10^3, NaN in every
    out-of-matrix entry; offset: placed one element into a NaN buffer.  Returns (buffer, element offset, band view)."""
    nd = 2 * hb + 1
    scale = 10.0 ** torch.randint(-3, 4, (nb, nd, 1), generator=g).double()
    vals = torch.where(in_matrix(hb, N), _randn(g, nb, nd, N) * scale, _nan((nb, nd, N)))
    off = 1 if offset else 0
    buf = _nan((nb * nd * N + off,), dtype)
    band = buf[off:].view(nb, nd, N)
    band.copy_(vals.to(dtype))
    return buf, off, band


def strided_panel(dtype, B, C, N, extra, pad, off, fill=None):
    """(B, C, N) view at row pitch N + extra and batch pitch C (N + extra) + pad, `off` elements into a NaN buffer;
    filled with `fill` (B, C, N) if given.  Returns (buffer, view)."""
    ld = N + extra
    sB = C * ld + pad
    buf = _nan((B * sB + off + 8,), dtype)
    view = buf.as_strided((B, C, N), (sB, ld, 1), off)
    if fill is not None:
        view.copy_(fill.to(dtype))
    return buf, view


def case(dtype, cfg):
    """host operands of one launch: band (see make_band); X a strided view (row pitch N + 3, batch pitch padded by
    5) of the NaN buffer xbuf, every column at its own scale 0.1 .. 10; Y likewise (row pitch N + 11, batch pitch
    padded by 7) of ybuf, all NaN: the output the caller hands in"""
    N, hb, C, B = cfg.N, cfg.hb, cfg.C, cfg.B
    g = _gen(9, N, hb, C, B, cfg.bcast, cfg.trans, cfg.offset, DTYPES.index(dtype))
    bbuf, boff, band = make_band(g, dtype, 1 if cfg.bcast else B, hb, N, cfg.offset)
    x = _randn(g, B, C, N) * 10.0 ** torch.randint(-1, 2, (B, C, 1), generator=g).double()
    xbuf, X = strided_panel(dtype, B, C, N, 3, 5, 3, x)
    ybuf, Y = strided_panel(dtype, B, C, N, 11, 7, 5)
    return dict(cfg=cfg, bbuf=bbuf, boff=boff, band=band, xbuf=xbuf, X=X, ybuf=ybuf, Y=Y)


def view_like(buf, view):
    """the view of `buf` (a copy of the host buffer, e.g. on the device) that `view` is of the host buffer"""
    return buf.as_strided(view.shape, view.stride(), view.storage_offset())


def ref(dtype, c, fault=None):
    return banded_mm(dtype, c["band"], c["X"], c["cfg"].hb, c["cfg"].trans, fault)


def operator_ref(dtype, band, x, trans):
    """BandedLinearOperator level: band (*BA, nd, N), x (*BX, N, R) in the kernel dtype on the host, batches
    broadcast against each other.  {"Y": (value, bound)} of shape (*batch, N, R), from the broadcast operands."""
    nd, N = band.shape[-2:]
    FB = torch.broadcast_shapes(band.shape[:-2], x.shape[:-2])
    bf = band.expand(*FB, nd, N).reshape(-1, nd, N)
    xf = x.expand(*FB, N, x.shape[-1]).reshape(-1, N, x.shape[-1]).transpose(1, 2)
    val, bnd = banded_mm(dtype, bf, xf, nd // 2, trans)["Y"]
    back = lambda t: t.transpose(1, 2).reshape(*FB, N, x.shape[-1])
    return {"Y": (back(val), back(bnd))}


# ================================================================================================ where a fault shows
# VISIBLE[fault](cfg, dtype) -> bool: can this fault change an output at this configuration at all?
def _some(cfg):
    return cfg.N > 0 and cfg.C > 0


VISIBLE = {
    "mask_dropped": lambda cfg, dtype: _some(cfg) and cfg.hb > 0,
    "halo_shift": lambda cfg, dtype: _some(cfg),
    "tile_halo_zero": lambda cfg, dtype: _some(cfg) and cfg.N > rows_of(dtype) and cfg.hb > 0,
    "trans_ignored": lambda cfg, dtype: _some(cfg) and cfg.trans and cfg.hb > 0 and cfg.N > 1,
    "tail_rows_dropped": lambda cfg, dtype: _some(cfg) and cfg.N % rows_of(dtype) != 0,
    "second_chunk_dropped": lambda cfg, dtype: cfg.N > 0 and cfg.C > CHUNK,
    "band_batch_ignored": lambda cfg, dtype: _some(cfg) and cfg.B > 1 and not cfg.bcast,
    "pitch_ignored": lambda cfg, dtype: cfg.N > 0 and cfg.C > 1,        # the case builder's pitch is N + 3, never N
}
