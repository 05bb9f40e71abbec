from xitorch_amd.linalg.solve import solve
from xitorch_amd.linalg.symeig import symeig, lsymeig, usymeig, svd
from xitorch_amd.linalg.precond import fsai, FSAIOperator
from xitorch_amd.linalg.lstsq import lstsq

__all__ = ["solve", "symeig", "lsymeig", "usymeig", "svd", "fsai", "FSAIOperator", "lstsq"]
