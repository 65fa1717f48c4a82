/*
 * drive_plant_twin.cpp -- TEST-ONLY CPU build of the track-driving loop with per-car plant values (the mpc_drive_*_plant entry points of
 * include/mpc_amd_drive.h), in its stepwise definition.
 *
 * tests/drive_latency_twin with a plant array: the handler is what it is there -- it reads nothing of the plant --, and the plant moves
 * every car with the values of its own column (mpc::drive_plant_vals_of: a column that cannot be used has become the default column
 * and a status) -- what the plant build of the plant-and-summary kernel and the lane kernel's hand-over do.  A model and a latency
 * array are always passed (tests/run_model_helpers.uniform_model and tests/drive_latency_helpers.uniform_latency give the handle's own
 * values, bitwise the builds without them).  Compiled like tests/drive_twin.  Never linked into the product library.
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

/* The handler for car i on the window that starts at waypoint k, compensating for `comp` seconds, with the car's column of model. */
void handler_one(const MpcParams &p, std::vector<double> &wsbuf, int64_t i, int64_t ld, const double *car, double comp, const double *tx,
                 const double *ty, int n, int k, int npts, const double *weights, const double *model, const mpc::WarmCall &W, double *ptsx,
                 double *ptsy, double *pre, double *out9, double *cmd, int32_t *status, int32_t *iters) {
  const mpc::ModelVals mv = mpc::model_vals_of(p, model, ld, i);
  const mpc::ModelColumn col{model + i, ld};
  mpc::drive_window_points(tx, ty, n, k, npts, ptsx, ptsy, ld, i);
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

/* the plant on car [6][ld] in place, reply cmd [2][ld], model [MPC_NMODEL][ld], plant [MPC_NPLANT][ld]: every car moved with the values
 * of its own column, sub_old and sub_new substeps of length h; ok [ld] or nullptr: whether the column could be used */
extern "C" int mpc_drive_plant_twin_plant(const MpcParams *p, int64_t B, int64_t ld, double *car, const double *cmd, const double *model,
                                          const double *plant, int sub_old, int sub_new, double h, int32_t *ok) {
  if (!p || ld < B || !car || !cmd || !model || !plant || sub_old < 0 || sub_new < 0 || sub_old + sub_new > 1000) return MPC_ERR_INVALID;
  for (int64_t i = 0; i < B; i++) {
    double c[6];
    for (int q = 0; q < 6; q++) c[q] = car[q * ld + i];
    const mpc::ModelVals mv = mpc::model_vals_of(*p, model, ld, i);
    const mpc::DrivePlantVals pv = mpc::drive_plant_vals_of(*p, mv, plant, ld, i);
    mpc::drive_plant(*p, mv, pv, c, cmd[i], cmd[ld + i], sub_old, sub_new, h);
    for (int q = 0; q < 6; q++) car[q * ld + i] = c[q];
    if (ok) ok[i] = pv.ok ? 1 : 0;
  }
  return MPC_OK;
}

/* The arguments of mpc_drive_batch_host_plant without the horizon: step by step, every car of a step before the next step (the
 * stepwise definition).  handler_status [steps][ld] or nullptr: the handler's own status of every step, which the warm rule reads. */
extern "C" int mpc_drive_plant_twin(const MpcParams *p, int64_t B, int64_t ld, int steps, double *car, const double *tx, const double *ty,
                                    int n_track, const double *weights, const double *model, const double *latency, const double *plant,
                                    const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary, double *hist, int32_t *status,
                                    int32_t *iters, int32_t *handler_status) {
  if (bad_opts(p, opts, warm_opts, n_track) || B < 0 || ld < B || steps < 1 || !car || !tx || !ty || !model || !latency || !plant || !summary || !status)
    return MPC_ERR_INVALID;
  std::vector<double> wsbuf((size_t)mpc::workspace_fields_per_instance(p->N, false, true));
  std::vector<double> rows((size_t)(2 * mpc::RUN_MAX_PTS + mpc::RUN_PRE_ROWS + 9 + 2) * ld);
  double *ptsx = rows.data(), *ptsy = ptsx + mpc::RUN_MAX_PTS * ld, *pre = ptsy + mpc::RUN_MAX_PTS * ld, *out9 = pre + mpc::RUN_PRE_ROWS * ld, *cmd = out9 + 9 * ld;
  std::vector<double> warm(opts->warm_start ? (size_t)(p->N - 1) * MPC_WARM_REC * ld : 0);
  std::vector<int32_t> st(ld, 0), it(ld, 0), kbuf(2 * ld, 0);
  for (int t = 0; t < steps; t++) {
    int32_t *k_now = kbuf.data() + (int64_t)(t & 1) * ld, *k_prev = kbuf.data() + (int64_t)((t & 1) ^ 1) * ld;
    const mpc::WarmCall W = opts->warm_start ? mpc::WarmCall{t == 0 ? nullptr : warm.data(), st.data(), warm.data(), ld, *warm_opts, 1}
                                             : mpc::WarmCall{nullptr, nullptr, nullptr, ld, *warm_opts, 1};
    for (int64_t i = 0; i < B; i++) {
      k_now[i] = mpc::drive_window(tx, ty, n_track, car[i], car[ld + i]);
      handler_one(*p, wsbuf, i, ld, car, mpc::drive_latency_of(*opts, latency, ld, i).comp, tx, ty, n_track, k_now[i], opts->npts, weights, model, W,
                  ptsx, ptsy, pre, out9, cmd, st.data(), it.data());
      if (handler_status) handler_status[(int64_t)t * ld + i] = st[i];
    }
    for (int64_t i = 0; i < B; i++) {
      const mpc::DriveLatency dl = mpc::drive_latency_of(*opts, latency, ld, i);
      const mpc::ModelVals mv = mpc::model_vals_of(*p, model, ld, i);
      mpc::drive_step_instance(*p, mv, mpc::drive_plant_vals_of(*p, mv, plant, ld, i), *opts, dl.sub_old, dl.sub_new, i, ld, t, n_track, car, cmd, pre, ld,
                               st[i], it[i], k_now[i], k_prev[i], summary, hist ? hist + (int64_t)t * MPC_DRIVE_REC * ld : nullptr, status, iters);
    }
  }
  return MPC_OK;
}
