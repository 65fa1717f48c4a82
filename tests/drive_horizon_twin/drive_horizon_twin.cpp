/*
 * drive_horizon_twin.cpp -- TEST-ONLY CPU build of the track-driving loop with a per-car horizon (the mpc_drive_*_horizon and
 * mpc_telemetry_batch_*_horizon entry points of include/mpc_amd_drive.h), in its stepwise definition.
 *
 * tests/drive_latency_twin with a horizon array: the solve of car i is set up with an mpc::HorizonColumn -- horizon[i] steps, the
 * car's column of model if there is one -- and nothing else reads N: the window, the handler's two halves, the plant and the summary
 * are the latency twin's.  The warm buffer keeps the rows of the handle's N; a car reads and writes the records of its own stages.
 * model may be NULL here (the handle's own six values, as on the device); latency is always passed.  Compiled like tests/drive_twin.
 * Never linked into the product library.
 */
#include <cmath>
#include <cstdint>
#include <vector>

#include "mpc_drive_core.h"

namespace {
using WS = mpc::HostWorkspace<double>;
using SV = mpc::Solver<WS, double>;

bool bad_opts(const MpcParams *p, const MpcDriveOpts *o, const MpcWarmOpts *w, int n_track) {
  return !p || p->N < 3 || p->N > MPC_MAX_N || !o || o->size != (int32_t)sizeof(MpcDriveOpts) || o->npts < 3 || o->npts > mpc::RUN_MAX_PTS ||
         n_track < o->npts || n_track > MPC_DRIVE_MAX_TRACK || !w || w->size != (int32_t)sizeof(MpcWarmOpts) || o->sub_old < 0 || o->sub_new < 0 ||
         o->sub_old + o->sub_new < 1 || o->sub_old + o->sub_new > 1000;
}

mpc::ModelVals vals_of(const MpcParams &p, const double *model, int64_t ld, int64_t i) {
  return model ? mpc::model_vals_of(p, model, ld, i) : mpc::ModelVals::of(p);
}

/* The handler for car i on the window that starts at waypoint k, compensating for `comp` seconds, solved over n steps. */
void handler_one(const MpcParams &p, std::vector<double> &wsbuf, int64_t i, int64_t ld, const double *car, double comp, const double *tx,
                 const double *ty, int n_track, int k, int npts, const double *weights, const double *model, int n, const mpc::WarmCall &W,
                 double *ptsx, double *ptsy, double *pre, double *out9, double *cmd, int32_t *status, int32_t *iters) {
  const mpc::ModelVals mv = vals_of(p, model, ld, i);
  const mpc::HorizonColumn col{model ? model + i : nullptr, ld, n};
  mpc::drive_window_points(tx, ty, n_track, k, npts, ptsx, ptsy, ld, i);
  mpc::run_pre_instance<true>(p, mv, i, ld, npts, car, mpc::RunComp{true, comp}, ptsx, ptsy, pre, ld);
  double st[6], cf[MPC_NCOEF], w[MPC_NW];
  mpc::gather_instance(p, i, ld, pre + mpc::RUN_PRE_STATE * ld, pre + mpc::RUN_PRE_COEFFS * ld, weights, st, cf, w);
  const double ylo = pre[mpc::RUN_PRE_YAW_LO * ld + i], yhi = pre[mpc::RUN_PRE_YAW_HI * ld + i];
  SV S(p, WS{wsbuf.data()});
  const mpc::WarmStart warm = W.instance(i, ylo, yhi);
  status[i] = mpc::instance_solve(S, col, warm, st, cf, ylo, yhi, w);
  double *o = out9 + i;
  iters[i] = mpc::instance_store(S, col, warm, [o, ld](int q) -> double & { return o[q * ld]; }, [o](int) -> double & { return o[0]; }, false,
                                 ylo, yhi);
  mpc::run_post_instance(p, mv, i, pre, ld, out9, ld, nullptr, cmd, ld);
}
}  // namespace

/* the plant on car [6][ld] in place: the latency twin's, model may be NULL (the horizon is no part of the plant) */
extern "C" int mpc_drive_horizon_twin_plant(const MpcParams *p, int64_t B, int64_t ld, double *car, const double *cmd, const double *model,
                                            const double *latency, const MpcDriveOpts *opts) {
  if (!p || ld < B || !car || !cmd || !latency || !opts || opts->sub_old < 0 || opts->sub_new < 0 || opts->sub_old + opts->sub_new > 1000)
    return MPC_ERR_INVALID;
  for (int64_t i = 0; i < B; i++) {
    double c[6];
    for (int q = 0; q < 6; q++) c[q] = car[q * ld + i];
    const mpc::DriveLatency dl = mpc::drive_latency_of(*opts, latency, ld, i);
    mpc::drive_plant(*p, vals_of(*p, model, ld, i), c, cmd[i], cmd[ld + i], dl.sub_old, dl.sub_new, opts->h);
    for (int q = 0; q < 6; q++) car[q * ld + i] = c[q];
  }
  return MPC_OK;
}

/* One handler call on cars [6][ld] with the windows that start at k [ld], comp [ld] and horizon [ld]: the arguments of
 * mpc_telemetry_batch_host_horizon with the window named by its index, plus weights, iterations and the two rows cte0 / epsi0 [2][ld]. */
extern "C" int mpc_drive_horizon_twin_handler(const MpcParams *p, int64_t B, int64_t ld, const double *car, const double *comp, const int32_t *k,
                                              const double *tx, const double *ty, int n_track, const double *weights, const double *model,
                                              const int32_t *horizon, const MpcDriveOpts *opts, const double *warm_in, const int32_t *warm_status,
                                              double *warm_out, int64_t ld_warm, const MpcWarmOpts *warm_opts, double *cmd, int32_t *status,
                                              int32_t *iters, double *cte_epsi) {
  if (bad_opts(p, opts, warm_opts, n_track) || ld < B || !car || !comp || !k || !tx || !ty || !horizon || !cmd || !status || !iters ||
      ((warm_in || warm_out) && ld_warm < B))
    return MPC_ERR_INVALID;
  std::vector<double> wsbuf((size_t)mpc::workspace_fields_per_instance(p->N, false, true));
  std::vector<double> rows((size_t)(2 * mpc::RUN_MAX_PTS + mpc::RUN_PRE_ROWS + 9) * ld);
  double *ptsx = rows.data(), *ptsy = ptsx + mpc::RUN_MAX_PTS * ld, *pre = ptsy + mpc::RUN_MAX_PTS * ld, *out9 = pre + mpc::RUN_PRE_ROWS * ld;
  const mpc::WarmCall W{warm_in, warm_status, warm_out, ld_warm, *warm_opts, 1};
  for (int64_t i = 0; i < B; i++) {
    if (k[i] < 0 || k[i] >= n_track) return MPC_ERR_INVALID;
    handler_one(*p, wsbuf, i, ld, car, comp[i], tx, ty, n_track, k[i], opts->npts, weights, model, horizon[i], W, ptsx, ptsy, pre, out9, cmd, status,
                iters);
    if (cte_epsi) { cte_epsi[i] = pre[(mpc::RUN_PRE_STATE + 4) * ld + i]; cte_epsi[ld + i] = pre[(mpc::RUN_PRE_STATE + 5) * ld + i]; }
  }
  return MPC_OK;
}

/* The arguments of mpc_drive_batch_host_horizon: step by step, every car of a step before the next step (the stepwise definition). */
extern "C" int mpc_drive_horizon_twin(const MpcParams *p, int64_t B, int64_t ld, int steps, double *car, const double *tx, const double *ty,
                                      int n_track, const double *weights, const double *model, const int32_t *horizon, const double *latency,
                                      const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary, double *hist, int32_t *status,
                                      int32_t *iters) {
  if (bad_opts(p, opts, warm_opts, n_track) || B < 0 || ld < B || steps < 1 || !car || !tx || !ty || !horizon || !latency || !summary || !status)
    return MPC_ERR_INVALID;
  std::vector<double> wsbuf((size_t)mpc::workspace_fields_per_instance(p->N, false, true));
  std::vector<double> rows((size_t)(2 * mpc::RUN_MAX_PTS + mpc::RUN_PRE_ROWS + 9 + 2) * ld);
  double *ptsx = rows.data(), *ptsy = ptsx + mpc::RUN_MAX_PTS * ld, *pre = ptsy + mpc::RUN_MAX_PTS * ld, *out9 = pre + mpc::RUN_PRE_ROWS * ld, *cmd = out9 + 9 * ld;
  std::vector<double> warm(opts->warm_start ? (size_t)(p->N - 1) * MPC_WARM_REC * ld : 0);      /* (the rows of the handle's N) */
  std::vector<int32_t> st(ld, 0), it(ld, 0), kbuf(2 * ld, 0);
  for (int t = 0; t < steps; t++) {
    int32_t *k_now = kbuf.data() + (int64_t)(t & 1) * ld, *k_prev = kbuf.data() + (int64_t)((t & 1) ^ 1) * ld;
    const mpc::WarmCall W = opts->warm_start ? mpc::WarmCall{t == 0 ? nullptr : warm.data(), st.data(), warm.data(), ld, *warm_opts, 1}
                                             : mpc::WarmCall{nullptr, nullptr, nullptr, ld, *warm_opts, 1};
    for (int64_t i = 0; i < B; i++) {
      k_now[i] = mpc::drive_window(tx, ty, n_track, car[i], car[ld + i]);
      handler_one(*p, wsbuf, i, ld, car, mpc::drive_latency_of(*opts, latency, ld, i).comp, tx, ty, n_track, k_now[i], opts->npts, weights, model,
                  horizon[i], W, ptsx, ptsy, pre, out9, cmd, st.data(), it.data());
    }
    for (int64_t i = 0; i < B; i++) {
      const mpc::DriveLatency dl = mpc::drive_latency_of(*opts, latency, ld, i);
      mpc::drive_step_instance(*p, vals_of(*p, model, ld, i), *opts, dl.sub_old, dl.sub_new, i, ld, t, n_track, car, cmd, pre, ld, st[i], it[i], k_now[i],
                               k_prev[i], summary, hist ? hist + (int64_t)t * MPC_DRIVE_REC * ld : nullptr, status, iters);
    }
  }
  return MPC_OK;
}
