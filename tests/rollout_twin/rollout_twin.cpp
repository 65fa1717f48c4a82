/*
 * rollout_twin.cpp -- TEST-ONLY CPU build of the fused rollout's per-car loop (mpc_rollout_batch_device_fused).
 *
 * The fused rollout keeps a car in one lane for all its steps; between two solves of a car it goes through mpc::RolloutCar
 * (carnd-mpc-project_amd/csrc/mpc_core.h) and nothing else.  This build runs the cars ONE AFTER THE OTHER, each through its whole
 * loop, with the same struct and Solver::solve_warm (warm = false is Solver::solve), so that the order "car by car" can be checked
 * against the order "step by step" of tests/warm_twin on a machine without a GPU (tests/test_rollout_fused.py).  Arguments as
 * mpc_rollout_batch_device_fused, plus every solve's status and iterations.  Never linked into the product library.
 */
#include <cstdint>
#include <vector>

#include "mpc_core.h"

extern "C" int mpc_rollout_twin(const MpcParams *p, int64_t B, int64_t ld, int steps, double *state, const double *coeffs,
                                const double *yaw_lo, const double *yaw_hi, const double *weights, int warm_start,
                                const MpcWarmOpts *opts, double *hist, int32_t *status, int32_t *iters, int32_t *step_status,
                                int32_t *step_iters) {
  if (!p || p->N < 3 || p->N > MPC_MAX_N || steps < 1 || ld < B || !opts || opts->size != (int32_t)sizeof(MpcWarmOpts)) return MPC_ERR_INVALID;
  if (!state || !coeffs || !yaw_lo || !yaw_hi || !hist || !status || !iters) return MPC_ERR_INVALID;
  using WS = mpc::HostWorkspace<double>;
  using SV = mpc::Solver<WS, double>;
  using Car = mpc::RolloutCar;
  const int N = p->N;
  std::vector<double> wsbuf((size_t)mpc::workspace_fields_per_instance(N, false, true));
  std::vector<double> column((size_t)(N - 1) * MPC_WARM_REC);       /* the car's warm column */
  for (int64_t i = 0; i < B; i++) {
    double cf[MPC_NCOEF], w[MPC_NW];
    for (int q = 0; q < MPC_NCOEF; q++) cf[q] = coeffs[q * ld + i];
    for (int q = 0; q < MPC_NW; q++) w[q] = weights ? weights[q * ld + i] : p->weights[q];
    int32_t prev = 0;
    for (int t = 0; t < steps; t++) {
      double st[6];
      for (int q = 0; q < 6; q++) st[q] = state[q * ld + i];
      SV S(*p, WS{wsbuf.data()});
      const bool warm = warm_start != 0 && Car::starts_warm(t, prev);
      int r = S.setup(st, cf, yaw_lo[i], yaw_hi[i], w, true);
      if (r == MPC_STATUS_SUCCESS) {
        const double *col = column.data();
        r = S.solve_warm(warm, [col](int k, int f) { return col[k * MPC_WARM_REC + f]; }, *opts);
      }
      double *o = hist + (int64_t)t * 9 * ld + i;
      S.unpack([o, ld](int q) -> double & { return o[q * ld]; }, [](int) -> double & { static double none; return none; }, false, yaw_lo[i], yaw_hi[i]);
      double *sp = state + i;
      Car::next_state([o, ld](int q) { return o[q * ld]; }, [sp, ld](int q, double v) { sp[q * ld] = v; });
      status[i] = Car::fold_status(t, status[i], r);
      iters[i] = Car::sum_iters(t, iters[i], S.iters);
      if (warm_start) {
        double *wo = column.data();
        S.warm_store([wo](int k, int f, double v) { wo[k * MPC_WARM_REC + f] = v; });
      }
      if (step_status) step_status[(int64_t)t * ld + i] = r;
      if (step_iters) step_iters[(int64_t)t * ld + i] = S.iters;
      prev = r;
    }
  }
  return MPC_OK;
}
