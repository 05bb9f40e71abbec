"""Stochastic Lanczos quadrature on the HIP kernels of xk_slq.hip: the quadratic forms z_j^H f(A) z_j of a Hermitian
operator on a device, by Gauss quadrature on the Lanczos tridiagonal.

An extension (the reference has no logdet / trace of a matrix function).  Every (batch member, probe) pair is one
system; all S = Bt * p systems advance in lock step on (Bt, p, ld) panels.  One step:

  apply A on r2            -> W          (`PanelOperator`: dense, CSR, banded natively; the operator's own .mm otherwise)
  xk_kry_dots              -> partials of <r2, W>
  xk_slq_step              -> alpha, beta into the device arrays Tal, Tbe (S, nsteps); the next un-normalised Lanczos
                              vector over r1; partials of its squared norm; breakdown freezes the system

Three vectors per system whatever the step count (the probe panel becomes r1 after xk_slq_init has copied it), no
stored basis, no reorthogonalisation.  The host reads NOTHING inside the run: after nsteps steps xk_slq_quad turns every
(Tal, Tbe) into nodes, weights and the sum on the device, and the caller reads the results once.

Not built: reorthogonalisation (f(A) B itself is native_fnm.py), preconditioned or M-weighted quadrature, batch sharding.
"""
import torch
from xitorch_amd import kernels as K
from xitorch_amd._util import bcast_shape
from xitorch_amd.linalg._panel import PanelOperator, pad_len, batch_count, require_hip, to_panel
from xitorch_amd.linalg.native_krylov import _Kry
from xitorch_amd.linalg import host_slq

__all__ = ["forms"]

ST_M, ST_ZNORM2 = 3, 6


class _Geom:
    """geometry of the panels: what `_Kry` asks for"""

    def __init__(self, N, Bt, p, dtype, device):
        self.N, self.ld, self.S = N, pad_len(N), Bt * p
        self.shape = (Bt, p, self.ld)
        self.dtype, self.device = dtype, device

    def new(self):
        return torch.zeros(self.shape, dtype=self.dtype, device=self.device)


def forms(A, Z, opt):
    """z_j^H f(A) z_j for every column of Z (*BZ, n, p) on the HIP kernels.  Returns the forms (*BAZ, p) in float64, a
    bool array of the same shape (a node <= 0 under a function that needs positivity, or a quadrature that did not
    converge: the form is NaN), the step counts (*BAZ, p) and the number of operator applies -- all device tensors:
    nothing is read by the host here."""
    require_hip(A, "slq")                       # (operators in host memory are dispatched to host_slq by slq._forms)
    device = torch.device(A.device)
    dtype, n = A.dtype, A.shape[-1]
    bdims = list(bcast_shape(A.shape[:-2], Z.shape[:-2]))
    Bt, p = batch_count(bdims), Z.shape[-1]
    nsteps = opt["nsteps"]
    op = PanelOperator(A, bdims, Bt, n)
    g = _Geom(n, Bt, p, dtype, device)
    kr = _Kry(g)
    S, N, ld, nblk = g.S, g.N, g.ld, kr.nblk
    z = to_panel(Z.to(device=device, dtype=dtype), bdims, Bt, n)
    r2, W = g.new(), g.new()
    Pa, Pn = kr.partial(), (kr.partial_real(), kr.partial_real())
    state = K.slq_state(S, device)
    Tal = torch.zeros((S, nsteps), dtype=torch.float64, device=device)
    Tbe = torch.zeros_like(Tal)
    kr.dots(z, z, Pa)                                                 # |z|^2
    K.slq_init(z, r2, Pa, state, S, N, ld, nblk, 0)
    r1 = z                                                            # the first step does not read r1
    for k in range(nsteps):
        op.apply(r2, W)
        kr.dots(r2, W, Pa)                                            # <r2, A r2> = beta^2 alpha
        K.slq_step(W, r2, r1, Pa, Pn[k & 1], Pn[(k + 1) & 1], state, Tal, Tbe, S, N, ld, nblk, nsteps, k)
        r1, r2 = r2, r1
    fn = opt["fn"]
    named = not callable(fn)
    theta, weight, out, flag = K.slq_quad(Tal, Tbe, state, nsteps, K.SLQ_FN[fn] if named else K.SLQ_FN["identity"],
                                          opt["t"])
    m = state[nsteps & 1, :, ST_M]
    if named:
        q, bad = out, flag != 0
    else:
        bad = (flag & 2) != 0
        q = host_slq.sum_nodes(theta, weight, m, state[nsteps & 1, :, ST_ZNORM2], fn)
        q = torch.where(bad, torch.full_like(q, float("nan")), q)
    return q.reshape(*bdims, p), bad.reshape(*bdims, p), m.to(torch.int64).reshape(*bdims, p), op.napply
