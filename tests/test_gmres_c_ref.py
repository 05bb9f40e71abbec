"""The per-kernel reference of the complex GMRES kernels (tests/gmres_c_ref.py) on the CPU: at every configuration the
GPU test runs, the reference accepts its own values rounded to the kernel dtype, and rejects every planted fault
wherever `visible()` says the fault changes an output."""
import pytest
import torch
from tests import gmres_c_ref as R

KERNELS = {
    "gram": (R.GRAM_CONFIGS, R.gram_case, R.gram_ref, R.FAULTS_GRAM),
    "lincomb": (R.LINCOMB_CONFIGS, R.lincomb_case, R.lincomb_ref, R.FAULTS_LINCOMB),
    "finish": (R.FINISH_CONFIGS, R.finish_case, R.finish_ref, R.FAULTS_FINISH),
    "step": (R.STEP_CONFIGS, R.step_case, R.step_ref, R.FAULTS_STEP),
    "solve": (R.SOLVE_CONFIGS, R.solve_case, R.solve_ref, R.FAULTS_SOLVE),
}
PARAMS = [(k, d, cfg) for k in KERNELS for d in R.DTYPES for cfg in KERNELS[k][0]]
IDS = ["%s-%s-%s" % (k, R.DNAME[d], "_".join(str(x) for x in cfg)) for k, d, cfg in PARAMS]


@pytest.mark.parametrize("kernel,dtype,cfg", PARAMS, ids=IDS)
def test_reference_accepts_itself_and_rejects_faults(kernel, dtype, cfg):
    _, mk, ref_of, faults = KERNELS[kernel]
    case = mk(dtype, *cfg)
    ref = ref_of(dtype, case)
    R.check(R.values(ref, dtype), ref, kernel, dtype, what="clean %s %s" % (kernel, cfg))
    seen = 0
    for f in faults:
        bad = ref_of(dtype, case, fault=f)
        if R.visible(kernel, f, cfg, dtype):
            with pytest.raises(AssertionError):
                R.check(R.values(bad, dtype), ref, kernel, dtype, what="%s %s %s" % (kernel, f, cfg))
            seen += 1
        else:
            R.check(R.values(bad, dtype), ref, kernel, dtype, what="%s %s %s (invisible)" % (kernel, f, cfg))
    assert seen or not any(R.visible(kernel, f, cfg, dtype) for f in faults)


def test_every_fault_is_visible_somewhere():
    for kernel, (cfgs, _, _, faults) in KERNELS.items():
        for f in faults:
            assert any(R.visible(kernel, f, cfg, d) for cfg in cfgs for d in R.DTYPES), (kernel, f)


def test_norm_entry_imaginary_part_is_checked_exactly():
    case = R.gram_case(torch.complex128, 5, 1, 3)
    ref = R.gram_ref(torch.complex128, case)
    assert bool((ref["nrm_im"][1] == 0).all()) and bool((ref["nrm_im"][0] == 0).all())
