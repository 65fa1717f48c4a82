/*
 * certify_sanitize.cpp -- TEST-ONLY: the CPU build of the certificate (tests/certify_twin/certify_twin.cpp, compiled into this
 * program) on garbage, under AddressSanitizer + UndefinedBehaviorSanitizer.  argv[1]: a config file.  Every array has exactly the
 * size the call states, so a read or write outside an instance's records, or past column B, is an error of the run.
 * Eight instances, N = 10, B = 8, ld = 9, ld_sol = 11 (ld_sol > ld); the columns from B on hold not-a-number (inputs) or a sentinel
 * (outputs).  Column: 0 a plain interior point; 1 a record full of not-a-number; 2 full of 1e300; 3 negative duals; 4 a horizon of 2;
 * 5 a horizon of N + 1; 6 an unusable model column (dt = 0); 7 the plain point again.  Two calls: with model and horizon arrays, and
 * with all of weights, model and horizon NULL (columns 4 - 6 are then plain points too).  Exit 0: the verdicts are what
 * include/mpc_amd_certify.h states, column 7 equals column 0 bit for bit, and nothing behind column B was written.
 */
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mpc_amd.h"

extern "C" int mpc_certify_twin(const MpcParams *p, int64_t B, int64_t ld, const double *state, const double *coeffs, const double *yaw_lo,
                                const double *yaw_hi, const double *weights, const double *model, const int32_t *horizon, const double *sol,
                                int64_t ld_sol, double *cert, int32_t *verdict);

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  MpcParams p;
  if (mpc_params_load_json(argv[1], &p) != MPC_OK) return 3;
  p.N = 10;
  const int N = p.N, B = 8, ld = 9, ld_sol = 11, rows = (N - 1) * MPC_WARM_REC;
  const double sentinel = -7777.25;
  const int32_t isentinel = -12345;
  std::vector<double> state((size_t)6 * ld, NAN), coeffs((size_t)MPC_NCOEF * ld, NAN), ylo((size_t)ld, NAN), yhi((size_t)ld, NAN);
  std::vector<double> model((size_t)MPC_NMODEL * ld, NAN), sol((size_t)rows * ld_sol, NAN);
  std::vector<int32_t> horizon((size_t)ld, 0);
  const double st[6] = {0.0, 0.0, 0.02, 12.0, 0.4, 0.03}, cf[MPC_NCOEF] = {0.4, 0.05, 0.002, 0.0, 0.0};
  const double own[MPC_NMODEL] = {p.dt, p.Lf, p.max_steering, p.max_acceleration, p.max_deceleration, p.max_speed};
  for (int i = 0; i < B; i++) {
    for (int q = 0; q < 6; q++) state[(size_t)q * ld + i] = st[q];
    for (int q = 0; q < MPC_NCOEF; q++) coeffs[(size_t)q * ld + i] = cf[q];
    for (int q = 0; q < MPC_NMODEL; q++) model[(size_t)q * ld + i] = own[q];
    ylo[i] = -1.0; yhi[i] = 1.0; horizon[i] = N;
    for (int k = 0; k < N - 1; k++)
      for (int f = 0; f < MPC_WARM_REC; f++) {
        /* an interior point that is no solution: the state repeated, small controls, multipliers 0.1, duals 1 */
        const double v = f < 6 ? st[f] : f < 8 ? 0.01 : f < 14 ? 0.1 : 1.0;
        sol[(size_t)(k * MPC_WARM_REC + f) * ld_sol + i] = v;
      }
  }
  for (int r = 0; r < rows; r++) { sol[(size_t)r * ld_sol + 1] = NAN; sol[(size_t)r * ld_sol + 2] = 1e300; }
  for (int k = 0; k < N - 1; k++)
    for (int f = 14; f < MPC_WARM_REC; f++) sol[(size_t)(k * MPC_WARM_REC + f) * ld_sol + 3] = -1.0;
  horizon[4] = 2; horizon[5] = N + 1;
  model[(size_t)MPC_MODEL_DT * ld + 6] = 0.0;
  const int32_t want_full[8] = {MPC_CERT_NOT_CONVERGED, MPC_CERT_NOT_A_POINT, MPC_CERT_NOT_A_POINT, MPC_CERT_NOT_A_POINT,
                                MPC_CERT_NO_PROBLEM, MPC_CERT_NO_PROBLEM, MPC_CERT_NO_PROBLEM, MPC_CERT_NOT_CONVERGED};
  const int32_t want_plain[8] = {MPC_CERT_NOT_CONVERGED, MPC_CERT_NOT_A_POINT, MPC_CERT_NOT_A_POINT, MPC_CERT_NOT_A_POINT,
                                 MPC_CERT_NOT_CONVERGED, MPC_CERT_NOT_CONVERGED, MPC_CERT_NOT_CONVERGED, MPC_CERT_NOT_CONVERGED};
  int bad = 0;
  for (int call = 0; call < 2; call++) {
    std::vector<double> cert((size_t)MPC_NCERT * ld, sentinel);
    std::vector<int32_t> verdict((size_t)ld, isentinel);
    const int rc = mpc_certify_twin(&p, B, ld, state.data(), coeffs.data(), ylo.data(), yhi.data(), nullptr, call == 0 ? model.data() : nullptr,
                                    call == 0 ? horizon.data() : nullptr, sol.data(), ld_sol, cert.data(), verdict.data());
    if (rc != MPC_OK) { printf("call %d: rc %d\n", call, rc); return 4; }
    const int32_t *want = call == 0 ? want_full : want_plain;
    printf("call %d verdicts", call);
    for (int i = 0; i < B; i++) {
      printf(" %d", verdict[i]);
      if (verdict[i] != want[i]) bad++;
      bool all_nan = true;
      for (int r = 0; r < MPC_NCERT; r++) all_nan = all_nan && std::isnan(cert[(size_t)r * ld + i]);
      if (verdict[i] == MPC_CERT_NO_PROBLEM && !all_nan) bad++;
      if (verdict[i] == MPC_CERT_NOT_CONVERGED && all_nan) bad++;
    }
    printf("\n");
    for (int r = 0; r < MPC_NCERT; r++) {
      if (memcmp(&cert[(size_t)r * ld + 7], &cert[(size_t)r * ld + 0], sizeof(double)) != 0) bad++;      /* the neighbour of the garbage */
      if (cert[(size_t)r * ld + B] != sentinel) bad++;
    }
    if (verdict[B] != isentinel) bad++;
  }
  /* the argument checks of the CPU build */
  std::vector<double> c1((size_t)MPC_NCERT * ld);
  std::vector<int32_t> v1((size_t)ld);
  if (mpc_certify_twin(&p, B, B - 1, state.data(), coeffs.data(), ylo.data(), yhi.data(), nullptr, nullptr, nullptr, sol.data(), ld_sol, c1.data(), v1.data()) != MPC_ERR_INVALID) bad++;
  if (mpc_certify_twin(&p, B, ld, state.data(), coeffs.data(), ylo.data(), yhi.data(), nullptr, nullptr, nullptr, sol.data(), B - 1, c1.data(), v1.data()) != MPC_ERR_INVALID) bad++;
  if (mpc_certify_twin(nullptr, B, ld, state.data(), coeffs.data(), ylo.data(), yhi.data(), nullptr, nullptr, nullptr, sol.data(), ld_sol, c1.data(), v1.data()) != MPC_ERR_INVALID) bad++;
  printf("bad %d\n", bad);
  return bad == 0 ? 0 : 1;
}
