// Stand-alone host program for the sanitizers: the argument checks of the Krylov-Schur Arnoldi entry points
// (xitorch_amd/csrc/xk_arn_check.h: what xk_arn_finish / xk_arn_schur run before any launch) and, with the lanes as a
// loop (XK_ARN_HOST), the member algorithm of xk_arn_schur on exact-size heap buffers.  Nothing that touches a device
// is compiled or linked.
//
//   hipcc -x c++ -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all -O1 -g -std=c++17 \
//         -I xitorch_amd/csrc -I include scripts/micro/arn_check_asan.cpp -o /tmp/arn_check_asan && /tmp/arn_check_asan
//   (any host C++17 compiler does: g++ -fsanitize=address,undefined ... the same line without -x c++ -Xarch_host)
#define XK_ARN_HOST
#include "xk_arn.hip"
#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);       \
      ++failures;                                                 \
    }                                                             \
  } while (0)

static void refusals() {
  std::vector<double> buf(64, 0.0);
  std::vector<int> ib(8, 0);
  double* p = buf.data();
  int* ip = ib.data();
  using xk::arn_finish_check;
  using xk::arn_schur_check;
  // part, Bt, nval, nchunk, coef, sC, nrm, rnrm, hcol, sHb, sHr, cplx, accumulate, sdst, u
  EXPECT(arn_finish_check(p, 1, 3, 1, p, 0, p, p, p, 0, 4, 0, 0, 0, 0.0) == XK_OK);
  EXPECT(arn_finish_check(nullptr, 1, 3, 1, p, 0, p, p, p, 0, 4, 0, 0, 0, 0.0) == XK_ERR_ARG);
  EXPECT(arn_finish_check(p, 0, 3, 1, p, 0, p, p, p, 0, 4, 0, 0, 0, 0.0) == XK_ERR_ARG);
  EXPECT(arn_finish_check(p, 1, 0, 1, p, 0, p, p, p, 0, 4, 0, 0, 0, 0.0) == XK_ERR_ARG);
  EXPECT(arn_finish_check(p, 1, 200, 1, p, 0, p, p, p, 0, 4, 0, 0, 0, 0.0) == XK_ERR_ARG);
  EXPECT(arn_finish_check(p, 1, 3, 0, p, 0, p, p, p, 0, 4, 0, 0, 0, 0.0) == XK_ERR_ARG);
  EXPECT(arn_finish_check(p, 1, 3, 1, p, 0, nullptr, p, p, 0, 4, 0, 0, 0, 0.0) == XK_ERR_ARG);
  EXPECT(arn_finish_check(p, 1, 3, 1, p, 0, p, nullptr, p, 0, 4, 0, 0, 0, 0.0) == XK_ERR_ARG);
  EXPECT(arn_finish_check(p, 1, 3, 1, p, -1, p, p, p, 0, 4, 0, 0, 0, 0.0) == XK_ERR_ARG);
  EXPECT(arn_finish_check(p, 1, 3, 1, p, 0, p, p, p, 0, 4, 0, 0, -1, 0.0) == XK_ERR_ARG);
  EXPECT(arn_finish_check(p, 1, 3, 1, p, 0, p, p, p, 0, 4, 0, 0, 0, -1.0) == XK_ERR_ARG);
  EXPECT(arn_finish_check(p, 1, 3, 1, p, 0, p, p, p, 0, 4, 2, 0, 0, 0.0) == XK_ERR_ARG);
  EXPECT(arn_finish_check(p, 1, 3, 1, p, 0, p, p, p, 0, 4, 0, 2, 0, 0.0) == XK_ERR_ARG);
  EXPECT(arn_finish_check(p, 1, 4, 1, p, 0, p, p, p, 0, 4, 1, 0, 0, 0.0) == XK_ERR_ARG);
  EXPECT(arn_finish_check(p, 1, 3, 1, p, 0, p, p, p, 0, 0, 0, 0, 0, 0.0) == XK_ERR_ARG);
  EXPECT(arn_finish_check(p, 1, 3, 1, p, 0, p, p, p, 0, 1, 1, 0, 0, 0.0) == XK_ERR_ARG);
  EXPECT(arn_finish_check(p, 2, 3, 1, p, 2, p, p, p, 4, 4, 0, 0, 0, 0.0) == XK_ERR_ARG);
  EXPECT(arn_finish_check(p, 2, 3, 1, p, 1, p, p, p, 8, 4, 0, 0, 0, 0.0) == XK_ERR_ARG);
  EXPECT(arn_finish_check(p, 2, 3, 1, p, 2, p, p, nullptr, 0, 0, 0, 0, 0, 0.0) == XK_OK);
  // H, Bt, m, neig, keep, which, cplx, tol, u, theta, Y, res, Q, Hnext, status
  double* q = p + 32;
  EXPECT(arn_schur_check(p, 1, 8, 2, 5, 0, 0, 1e-6, 1e-16, q, q, q, q, q, ip) == XK_OK);
  EXPECT(arn_schur_check(p, 0, 8, 2, 5, 0, 0, 1e-6, 1e-16, q, q, q, q, q, ip) == XK_ERR_ARG);
  EXPECT(arn_schur_check(p, 70000, 8, 2, 5, 0, 0, 1e-6, 1e-16, q, q, q, q, q, ip) == XK_ERR_ARG);
  EXPECT(arn_schur_check(p, 1, 1, 1, 1, 0, 0, 1e-6, 1e-16, q, q, q, q, q, ip) == XK_ERR_ARG);
  EXPECT(arn_schur_check(p, 1, xk::ARN_MAX_ROWS + 1, 2, 5, 0, 0, 1e-6, 1e-16, q, q, q, q, q, ip) == XK_ERR_ARG);
  EXPECT(arn_schur_check(p, 1, 8, 0, 5, 0, 0, 1e-6, 1e-16, q, q, q, q, q, ip) == XK_ERR_ARG);
  EXPECT(arn_schur_check(p, 1, 8, 6, 5, 0, 0, 1e-6, 1e-16, q, q, q, q, q, ip) == XK_ERR_ARG);
  EXPECT(arn_schur_check(p, 1, 8, 2, 8, 0, 0, 1e-6, 1e-16, q, q, q, q, q, ip) == XK_ERR_ARG);
  EXPECT(arn_schur_check(p, 1, 8, 2, 5, -1, 0, 1e-6, 1e-16, q, q, q, q, q, ip) == XK_ERR_ARG);
  EXPECT(arn_schur_check(p, 1, 8, 2, 5, 5, 1, 1e-6, 1e-16, q, q, q, q, q, ip) == XK_ERR_ARG);
  EXPECT(arn_schur_check(p, 1, 8, 2, 5, 3, 0, 1e-6, 1e-16, q, q, q, q, q, ip) == XK_ERR_ARG);
  EXPECT(arn_schur_check(p, 1, 8, 2, 5, 3, 1, 1e-6, 1e-16, q, q, q, q, q, ip) == XK_OK);
  EXPECT(arn_schur_check(p, 1, 8, 2, 5, 0, 2, 1e-6, 1e-16, q, q, q, q, q, ip) == XK_ERR_ARG);
  EXPECT(arn_schur_check(p, 1, 8, 2, 5, 0, 0, -1.0, 1e-16, q, q, q, q, q, ip) == XK_ERR_ARG);
  EXPECT(arn_schur_check(p, 1, 8, 2, 5, 0, 0, 1e-6, -1.0, q, q, q, q, q, ip) == XK_ERR_ARG);
  EXPECT(arn_schur_check(nullptr, 1, 8, 2, 5, 0, 0, 1e-6, 1e-16, q, q, q, q, q, ip) == XK_ERR_ARG);
  EXPECT(arn_schur_check(p, 1, 8, 2, 5, 0, 0, 1e-6, 1e-16, nullptr, q, q, q, q, ip) == XK_ERR_ARG);
  EXPECT(arn_schur_check(p, 1, 8, 2, 5, 0, 0, 1e-6, 1e-16, q, nullptr, q, q, q, ip) == XK_ERR_ARG);
  EXPECT(arn_schur_check(p, 1, 8, 2, 5, 0, 0, 1e-6, 1e-16, q, q, nullptr, q, q, ip) == XK_ERR_ARG);
  EXPECT(arn_schur_check(p, 1, 8, 2, 5, 0, 0, 1e-6, 1e-16, q, q, q, nullptr, q, ip) == XK_ERR_ARG);
  EXPECT(arn_schur_check(p, 1, 8, 2, 5, 0, 0, 1e-6, 1e-16, q, q, q, q, nullptr, ip) == XK_ERR_ARG);
  EXPECT(arn_schur_check(p, 1, 8, 2, 5, 0, 0, 1e-6, 1e-16, q, q, q, q, q, nullptr) == XK_ERR_ARG);
  EXPECT(arn_schur_check(p, 1, 8, 2, 5, 0, 0, 1e-6, 1e-16, q, q, q, q, p, ip) == XK_ERR_ARG);
}

template <bool CPLX>
static void members(int m, int which) {
  const int EL = CPLX ? 2 : 1, Bt = 2;
  const int neig = m > 3 ? 3 : 1;
  int keep = neig + (m - neig) / 2;
  if (keep > m - 1) keep = m - 1;
  std::vector<double> H((size_t)Bt * (m + 1) * m * EL), th((size_t)Bt * m * 2), Y((size_t)Bt * m * neig * 2),
      res((size_t)Bt * neig), Q((size_t)Bt * m * m * EL), Hn((size_t)Bt * (m + 1) * m * EL);
  std::vector<int> st(Bt * xk::ARN_STATUS), add(Bt, 1);
  for (auto& v : H) v = std::rand() / (double)RAND_MAX - 0.5;
  for (int b = 0; b < Bt; ++b) {
    xk::arn_schur_member<CPLX>(H.data(), m, neig, keep, b ? add.data() : nullptr, which, 1e-6, 1e-16, nullptr, th.data(),
                               Y.data(), res.data(), Q.data(), Hn.data(), st.data(), b);
    const int* s = st.data() + b * xk::ARN_STATUS;
    EXPECT((s[2] & 7) == 0 && s[3] >= keep - 1 && s[3] <= keep + 2 && s[3] <= m - 1 && s[1] <= 30 * m);
  }
}

int main() {
  refusals();
  std::srand(1);
  for (int m : {2, 3, 5, 16, 17, 33, xk::ARN_MAX_ROWS}) {
    for (int which = 0; which < 3; ++which) members<false>(m, which);
    for (int which = 0; which < 5; ++which) members<true>(m, which);
  }
  std::printf(failures ? "%d check(s) failed\n" : "arn_check_asan: all checks passed\n", failures);
  return failures ? 1 : 0;
}
