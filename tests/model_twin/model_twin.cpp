/*
 * model_twin.cpp -- TEST-ONLY CPU build of the per-instance model values of carnd-mpc-project_amd/csrc/mpc_core.h.
 *
 * The same Solver::setup_model / unpack_model that the MODEL builds of the lane kernel call, compiled with g++ and driven with the
 * arguments of mpc_solve_batch_host_model (include/mpc_amd.h), so that the rule -- which six values an instance brings along, what
 * a column that cannot be used ends as -- can be checked against the oracle on a machine without a GPU (tests/test_model.py).  The
 * solver type is the one of tests/host_twin (MpcParams.max_soc is honoured).  Never linked into the product library.
 */
#include <cstdint>
#include <vector>

#include "mpc_core.h"

extern "C" int mpc_model_twin_solve(const MpcParams *p, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                    const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                    double *out, double *traj, int32_t *status, int32_t *iters) {
  if (!p || p->N < 3 || p->N > MPC_MAX_N || !model || ld < B) return MPC_ERR_INVALID;
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
    /* as in the kernel: the column is read at set-up and again at the hand-over, nothing of it is carried in between */
    const double *mc = model + i;
    int r = S.setup_model([mc, ld](int q) { return mc[q * ld]; }, st, cf, yaw_lo[i], yaw_hi[i], w, true);
    if (r == MPC_STATUS_SUCCESS) r = S.solve();
    double *o = out + i;
    double *t = traj ? traj + i : nullptr;
    S.unpack_model([mc, ld](int q) { return mc[q * ld]; }, [o, ld](int q) -> double & { return o[q * ld]; },
                   [t, ld](int q) -> double & { return t[q * ld]; }, traj != nullptr, yaw_lo[i], yaw_hi[i]);
    status[i] = r;
    if (iters) iters[i] = S.iters;
  }
  return MPC_OK;
}

extern "C" int mpc_model_twin_nmodel(void) { return MPC_NMODEL; }
