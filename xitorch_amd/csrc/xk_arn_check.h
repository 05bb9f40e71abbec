// xitorch_amd :: the host-side argument checks of the Krylov-Schur Arnoldi entry points (xk_arn.hip).  Plain C++ with
// no HIP in sight: xk_arn.hip calls them before any launch, and tests/sanitize/arn_check_main.cpp compiles them alone
// (address + undefined-behaviour sanitizers on the host, nothing that touches a device linked in).
#pragma once
#include "xitorch_amd.h"

namespace xk {

constexpr int ARN_MAX_ROWS = 48;                   // order of the projected matrix xk_arn_schur serves
constexpr int ARN_WHICH_MAX = 4;                   // which: 0 LM, 1 LR, 2 SR, 3 LI, 4 SI
constexpr int ARN_FINISH_MAX_NVAL = 2 * 64 + 1;    // the partial sums of one xk_gkl_sweep over 64 rows (complex)

inline int arn_finish_check(const double* part, int Bt, int nval, int nchunk, const double* coef, long sC,
                            const double* nrm, const double* rnrm, const double* hcol, long sHb, long sHr, int cplx,
                            int accumulate, long sdst, double u) {
  if (Bt <= 0 || nval <= 0 || nchunk <= 0 || !part || !nrm || !rnrm || sC < 0 || sdst < 0 || !(u >= 0.0))
    return XK_ERR_ARG;
  if (nval > ARN_FINISH_MAX_NVAL || (Bt > 1 && coef && sC < nval - 1)) return XK_ERR_ARG;
  if ((cplx != 0 && cplx != 1) || (accumulate != 0 && accumulate != 1)) return XK_ERR_ARG;
  if (cplx && (nval - 1) % 2 != 0) return XK_ERR_ARG;
  if (hcol) {
    const long rows = cplx ? (nval - 1) / 2 : nval - 1;          // entries of the column
    if (sHr < (cplx ? 2 : 1) || sHb < 0) return XK_ERR_ARG;
    if (Bt > 1 && rows > 0 && sHb < (rows - 1) * sHr + (cplx ? 2 : 1)) return XK_ERR_ARG;
  }
  return XK_OK;
}

inline int arn_schur_check(const double* H, int Bt, int m, int neig, int keep, int which, int cplx, double tol,
                           double u, const double* theta, const double* Y, const double* res, const double* Q,
                           const double* Hnext, const int* status) {
  if (Bt <= 0 || Bt > 65535 || m < 2 || m > ARN_MAX_ROWS) return XK_ERR_ARG;
  if (neig < 1 || keep < neig || keep > m - 1) return XK_ERR_ARG;
  if (which < 0 || which > ARN_WHICH_MAX || (cplx != 0 && cplx != 1)) return XK_ERR_ARG;
  if (!cplx && which >= 3) return XK_ERR_ARG;                    // LI / SI: complex operators only
  if (!(tol >= 0.0) || !(u >= 0.0)) return XK_ERR_ARG;
  if (!H || !theta || !Y || !res || !Q || !Hnext || !status) return XK_ERR_ARG;
  if (Hnext == H) return XK_ERR_ARG;
  return XK_OK;
}

}  // namespace xk
