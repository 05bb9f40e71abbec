from xitorch_amd.linalg.solve import solve
from xitorch_amd.linalg.symeig import symeig, lsymeig, usymeig, svd
from xitorch_amd.linalg.precond import fsai, FSAIOperator, fsai_lu, FSAILUOperator
from xitorch_amd.linalg.lstsq import lstsq
from xitorch_amd.linalg.slq import quadform, trace_fn, logdet
from xitorch_amd.linalg.fnm import funm_multiply, expm_multiply
from xitorch_amd.linalg.eigs import eigs

__all__ = ["solve", "symeig", "lsymeig", "usymeig", "svd", "fsai", "FSAIOperator", "fsai_lu", "FSAILUOperator", "lstsq",
           "quadform", "trace_fn", "logdet", "funm_multiply", "expm_multiply", "eigs"]
