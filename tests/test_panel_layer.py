"""not-gpu: the geometry rules every native driver takes from linalg/_panel.py -- the Krylov block count, the real type
of a dtype, the batch count and the device / dtype guard."""
import pytest
import torch
import xitorch_amd as xa
from xitorch_amd import _capi
from xitorch_amd.linalg._panel import batch_count, real_dtype, kry_blocks, require_hip

VN = {torch.float64: 2, torch.float32: 4, torch.complex128: 1, torch.complex64: 2}     # elements per 16 B vector
DTYPES = list(VN)
IDS = ["f64", "f32", "c128", "c64"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_kry_blocks_is_the_literal_formula(dtype):
    vn = VN[dtype]
    cap = _capi.fn("xk_kry_max_partials")()
    beyond = 1024 * vn * cap + 1                 # one element more than `cap` blocks hold: the cap decides
    for N in (1, 1024 * vn, 1024 * vn + 1, beyond, 3 * beyond):
        assert kry_blocks(N, dtype) == max(1, min(cap, (N + 256 * vn * 4 - 1) // (256 * vn * 4))), N
    assert kry_blocks(1, dtype) == 1 and kry_blocks(1024 * vn, dtype) == 1 and kry_blocks(1024 * vn + 1, dtype) == 2
    assert kry_blocks(beyond, dtype) == cap and kry_blocks(3 * beyond, dtype) == cap
    assert kry_blocks(beyond - 1, dtype) == cap and kry_blocks(1024 * vn * (cap - 1), dtype) == cap - 1


def test_real_dtype():
    assert [real_dtype(d) for d in DTYPES] == [torch.float64, torch.float32, torch.float64, torch.float32]


def test_batch_count():
    assert batch_count(()) == 1 and batch_count([]) == 1
    assert batch_count((3,)) == 3
    assert batch_count((2, 0, 4)) == 0
    assert batch_count(torch.Size([2, 3, 4])) == 24


def test_require_hip_refuses_host_operators_and_half_precision():
    with pytest.raises(_capi.NativeLibraryError, match="HIP device only"):
        require_hip(xa.LinearOperator.m(torch.eye(4, dtype=torch.float64)), "solver")

    class _HalfOnDevice:
        device, dtype = torch.device("cuda:0"), torch.float16

    with pytest.raises(_capi.NativeLibraryError, match="float16"):
        require_hip(_HalfOnDevice(), "solver")
    for dtype in DTYPES:
        _HalfOnDevice.dtype = dtype
        require_hip(_HalfOnDevice(), "solver")
