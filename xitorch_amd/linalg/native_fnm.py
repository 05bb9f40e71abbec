"""f(A) B for a Hermitian operator on a device, by two-pass Lanczos on the HIP kernels of xk_slq.hip and xk_fnm.hip.

An extension (the reference has no matrix function of an operator).  Every (batch member, column) pair is one system;
all S = Bt * p systems advance in lock step on (Bt, p, ld) panels, five of them: b, r1, r2, W, X.

  pass 1   the run of `native_slq.forms` on b (apply, xk_kry_dots, xk_slq_step): Tal, Tbe (S, nsteps) and the step
           counts on the device.  b survives: r1 is a panel of its own here.
  small    xk_fnm_eig: nodes theta and the whole eigenvector matrix of every Jacobi matrix; a callable is applied in
           torch, on the device, to theta; xk_fnm_coeff: the coefficients C of f(A) b in the Lanczos basis, and `tail`.
  pass 2   the same recurrence replayed from Tal, Tbe (apply, xk_fnm_step): X += (C_k / beta_k) r2_k.  No inner
           products; the last step needs no apply.  b is the first r2 and is overwritten from the second step on.

No stored basis, no reorthogonalisation: pass 2 must reproduce pass 1's vectors bit for bit, which holds because the
operator applies and the step kernels are deterministic and xk_fnm_step forms its scalars as xk_slq_step does.  The host
reads NOTHING here; the caller reads flags, step counts and tails once.

Not built: the gradient with respect to the operator, restarts, rational or shift-and-invert Krylov spaces,
reorthogonalisation, batch sharding.
"""
import torch
from xitorch_amd import kernels as K
from xitorch_amd._util import bcast_shape
from xitorch_amd.linalg._panel import PanelOperator, batch_count, require_hip, to_panel, from_panel
from xitorch_amd.linalg.native_krylov import _Kry
from xitorch_amd.linalg.native_slq import _Geom, ST_M
from xitorch_amd.linalg import host_slq

__all__ = ["funm"]


def funm(A, B, opt):
    """f(A) b_j for every column of B (*BB, n, p) on the HIP kernels.  Returns X (*BAB, n, p), the flags (*BAB, p)
    (int64; bit 0: a node <= 0 under a function that needs positivity, bit 1: the QL iteration did not converge; the
    column of a flagged system is NaN), the step counts and the tails (*BAB, p) and the number of operator applies -- device tensors: nothing is read by the
    host here."""
    require_hip(A, "funm_multiply")             # (operators in host memory are dispatched to host_slq by fnm._funm)
    device = torch.device(A.device)
    dtype, n = A.dtype, A.shape[-1]
    bdims = list(bcast_shape(A.shape[:-2], B.shape[:-2]))
    Bt, p = batch_count(bdims), B.shape[-1]
    nsteps = opt["nsteps"]
    op = PanelOperator(A, bdims, Bt, n)
    g = _Geom(n, Bt, p, dtype, device)
    kr = _Kry(g)
    S, N, ld, nblk = g.S, g.N, g.ld, kr.nblk
    b = to_panel(B.to(device=device, dtype=dtype), bdims, Bt, n)
    r1, r2, W, X = g.new(), g.new(), g.new(), g.new()
    Pa, Pn = kr.partial(), (kr.partial_real(), kr.partial_real())
    state = K.slq_state(S, device)
    Tal = torch.zeros((S, nsteps), dtype=torch.float64, device=device)
    Tbe = torch.zeros_like(Tal)
    # pass 1
    kr.dots(b, b, Pa)                                                 # |b|^2
    K.slq_init(b, r2, Pa, state, S, N, ld, nblk, 0)
    for k in range(nsteps):
        op.apply(r2, W)
        kr.dots(r2, W, Pa)
        K.slq_step(W, r2, r1, Pa, Pn[k & 1], Pn[(k + 1) & 1], state, Tal, Tbe, S, N, ld, nblk, nsteps, k)
        r1, r2 = r2, r1
    # the small problem
    ks = nsteps & 1
    theta, Qt, flag = K.fnm_eig(Tal, Tbe, state, ks)
    m = state[ks, :, ST_M]
    fn, cplx = opt["fn"], dtype.is_complex
    if callable(fn):
        f = host_slq.node_values(theta, m, fn, cplx)
        fvals = torch.view_as_real(f).contiguous() if cplx else f.contiguous()
        C, tail = K.fnm_coeff(Qt, theta, state, flag, ks, -1, 0.0, fvals=fvals, cplx=cplx)
    else:
        C, tail = K.fnm_coeff(Qt, theta, state, flag, ks, K.SLQ_FN[fn], opt["t"], cplx=cplx)
    # pass 2: b is the first r2; the vector of step k + 1 goes over r1
    r2 = b
    for k in range(nsteps):
        last = k == nsteps - 1
        if not last:
            op.apply(r2, W)
        K.fnm_step(None if last else W, r2, r1, X, C, Tal, Tbe, state, S, N, ld, nblk, nsteps, k, ks, last=last)
        r1, r2 = r2, r1
    return (from_panel(X, bdims, n), flag.to(torch.int64).reshape(*bdims, p), m.to(torch.int64).reshape(*bdims, p),
            tail.reshape(*bdims, p), op.napply)
