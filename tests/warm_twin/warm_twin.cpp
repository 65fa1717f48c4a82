/*
 * warm_twin.cpp -- TEST-ONLY CPU build of the warm start of carnd-mpc-project_amd/csrc/mpc_core.h.
 *
 * The same Solver::warm_point / begin_warm / warm_store (through Solver::solve_warm) that the device kernels call, compiled with
 * g++ and driven with the arguments of mpc_solve_batch_host_warm (include/mpc_amd.h), so that the warm rules can be checked
 * against the oracle on a machine without a GPU (tests/test_warm_start.py).  Never linked into the product library.
 */
#include <cstdint>
#include <vector>

#include "mpc_core.h"

extern "C" int mpc_warm_twin_solve(const MpcParams *p, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                   const double *yaw_lo, const double *yaw_hi, const double *weights, const double *warm_in,
                                   const int32_t *warm_status, double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts,
                                   double *out, double *traj, int32_t *status, int32_t *iters) {
  if (!p || p->N < 3 || p->N > MPC_MAX_N || !opts || opts->size != (int32_t)sizeof(MpcWarmOpts)) return MPC_ERR_INVALID;
  if ((warm_in || warm_out) && ld_warm < B) return MPC_ERR_INVALID;
  using WS = mpc::HostWorkspace<double>;
  using SV = mpc::Solver<WS, double>;
  const int N = p->N;
  std::vector<double> wsbuf((size_t)mpc::workspace_fields_per_instance(N, false, true));
  for (int64_t i = 0; i < B; i++) {
    double st[6], cf[MPC_NCOEF], w[MPC_NW];
    for (int q = 0; q < 6; q++) st[q] = state[q * ld + i];
    for (int q = 0; q < MPC_NCOEF; q++) cf[q] = coeffs[q * ld + i];
    for (int q = 0; q < MPC_NW; q++) w[q] = weights ? weights[q * ld + i] : p->weights[q];
    SV S(*p, WS{wsbuf.data()});
    /* as in the kernels: the instance's column (and the status it came with) is read before anything of it is written */
    const bool warm = warm_in != nullptr && (warm_status == nullptr || warm_status[i] == MPC_STATUS_SUCCESS);
    int r = S.setup(st, cf, yaw_lo[i], yaw_hi[i], w, true);
    if (r == MPC_STATUS_SUCCESS) {
      const double *wi = warm_in + i;
      r = S.solve_warm(warm, [wi, ld_warm](int k, int f) { return wi[(int64_t)(k * MPC_WARM_REC + f) * ld_warm]; }, *opts);
    }
    double *o = out + i;
    double *t = traj ? traj + i : nullptr;
    S.unpack([o, ld](int q) -> double & { return o[q * ld]; }, [t, ld](int q) -> double & { return t[q * ld]; }, traj != nullptr, yaw_lo[i], yaw_hi[i]);
    if (warm_out) {
      double *wo = warm_out + i;
      S.warm_store([wo, ld_warm](int k, int f, double v) { wo[(int64_t)(k * MPC_WARM_REC + f) * ld_warm] = v; });
    }
    status[i] = r;
    if (iters) iters[i] = S.iters;
  }
  return MPC_OK;
}
