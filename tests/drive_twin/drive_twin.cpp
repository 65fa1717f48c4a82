/*
 * drive_twin.cpp -- TEST-ONLY CPU build of the track-driving loop (include/mpc_amd_drive.h), in its stepwise definition: the one CPU
 * build of every drive entry point, with the nullable per-car arrays of the _plant / _horizon forms.
 *
 * The functions of carnd-mpc-project_amd/csrc/mpc_drive_core.h (window, plant, summary: what the two drive kernels run) around the
 * per-instance driver of mpc_run_core.h and mpc_core.h (what the handler's three launches run), with an MpcParams in the place of the
 * handle, so that the loop can be checked against numpy and the oracle on a machine without a GPU and the device against this build.
 *
 * The handler chooses its column type the way the device chooses its build: mpc::NoColumn and the MpcParams itself with neither
 * `model` nor `horizon`, mpc::ModelColumn with `model` alone, mpc::HorizonColumn with `horizon` (model may then be NULL: the handle's
 * own six values); and it compensates for the call's extra_latency under the handle's rule without `latency` / `comp`, for the car's
 * own mpc::RunComp with it.  So NULL and an array of the handle's own values take different paths, and the tests that find their bits
 * equal say something.  The plant side has one path, like mpc_drive_plant_kernel.  The warm buffer keeps the rows of the handle's N;
 * a car with a horizon reads and writes the records of its own stages.
 * Compiled like tests/certify_twin (the device code's front end and contraction rule).  Never linked into the product library.
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

/* the scratch rows of one call: ptsx / ptsy [RUN_MAX_PTS][ld], pre [RUN_PRE_ROWS][ld], out9 [9][ld], cmd [2][ld] */
struct Rows {
  std::vector<double> wsbuf, buf;
  double *ptsx, *ptsy, *pre, *out9, *cmd;
  Rows(const MpcParams &p, int64_t ld)
      : wsbuf((size_t)mpc::workspace_fields_per_instance(p.N, false, true)), buf((size_t)(2 * mpc::RUN_MAX_PTS + mpc::RUN_PRE_ROWS + 9 + 2) * ld),
        ptsx(buf.data()), ptsy(ptsx + mpc::RUN_MAX_PTS * ld), pre(ptsy + mpc::RUN_MAX_PTS * ld), out9(pre + mpc::RUN_PRE_ROWS * ld), cmd(out9 + 9 * ld) {}
};

/* The handler for car i on the window that starts at waypoint k: pre rows, the solve from them (W: the warm call, psi box of the
 * run() path), the reply.  mv / col: the car's model values and the column its solve is set up with; lc: what it compensates for. */
template <class MV, class Col, class LC>
void handler_one(const MpcParams &p, const MV &mv, const Col &col, const LC &lc, Rows &R, int64_t i, int64_t ld, const double *car, const double *tx,
                 const double *ty, int n_track, int k, int npts, const double *weights, const mpc::WarmCall &W, double *cmd, int32_t *status,
                 int32_t *iters) {
  mpc::drive_window_points(tx, ty, n_track, k, npts, R.ptsx, R.ptsy, ld, i);
  mpc::run_pre_instance<true>(p, mv, i, ld, npts, car, lc, R.ptsx, R.ptsy, R.pre, ld);
  double st[6], cf[MPC_NCOEF], w[MPC_NW];
  mpc::gather_instance(p, i, ld, R.pre + mpc::RUN_PRE_STATE * ld, R.pre + mpc::RUN_PRE_COEFFS * ld, weights, st, cf, w);
  const double ylo = R.pre[mpc::RUN_PRE_YAW_LO * ld + i], yhi = R.pre[mpc::RUN_PRE_YAW_HI * ld + i];
  SV S(p, WS{R.wsbuf.data()});
  const mpc::WarmStart warm = W.instance(i, ylo, yhi);
  status[i] = mpc::instance_solve(S, col, warm, st, cf, ylo, yhi, w);
  double *o = R.out9 + i;
  iters[i] = mpc::instance_store(S, col, warm, [o, ld](int q) -> double & { return o[q * ld]; }, [o](int) -> double & { return o[0]; }, false,
                                 ylo, yhi);
  mpc::run_post_instance(p, mv, i, R.pre, ld, R.out9, ld, nullptr, cmd, ld);
}

/* ... with the column type chosen from what the call brought */
template <class LC>
void handler_with(const MpcParams &p, const double *model, const int32_t *horizon, const LC &lc, Rows &R, int64_t i, int64_t ld, const double *car,
                const double *tx, const double *ty, int n_track, int k, int npts, const double *weights, const mpc::WarmCall &W, double *cmd,
                int32_t *status, int32_t *iters) {
  if (horizon)
    handler_one(p, vals_of(p, model, ld, i), mpc::HorizonColumn{model ? model + i : nullptr, ld, horizon[i]}, lc, R, i, ld, car, tx, ty, n_track, k, npts,
                weights, W, cmd, status, iters);
  else if (model)
    handler_one(p, mpc::model_vals_of(p, model, ld, i), mpc::ModelColumn{model + i, ld}, lc, R, i, ld, car, tx, ty, n_track, k, npts, weights, W, cmd,
                status, iters);
  else
    handler_one(p, p, mpc::NoColumn{}, lc, R, i, ld, car, tx, ty, n_track, k, npts, weights, W, cmd, status, iters);
}
/* ... and what it compensates for: comp (seconds, the car's own) or nullptr -- the call's extra_latency under the handle's rule */
void handler_of(const MpcParams &p, const double *model, const int32_t *horizon, const double *comp, const MpcDriveOpts &O, Rows &R, int64_t i,
                int64_t ld, const double *car, const double *tx, const double *ty, int n_track, int k, const double *weights, const mpc::WarmCall &W,
                double *cmd, int32_t *status, int32_t *iters) {
  if (comp) handler_with(p, model, horizon, mpc::RunComp{true, *comp}, R, i, ld, car, tx, ty, n_track, k, O.npts, weights, W, cmd, status, iters);
  else handler_with(p, model, horizon, O.extra_latency, R, i, ld, car, tx, ty, n_track, k, O.npts, weights, W, cmd, status, iters);
}

/* what mpc_drive_plant_kernel hands on for car i: its substep counts, model values and plant values, each array nullable */
struct PlantSide {
  int sub_old, sub_new;
  mpc::ModelVals mv;
  mpc::DrivePlantVals pv;
  PlantSide(const MpcParams &p, const MpcDriveOpts &O, const double *model, const double *latency, const double *plant, int64_t ld, int64_t i)
      : sub_old(O.sub_old), sub_new(O.sub_new), mv(vals_of(p, model, ld, i)), pv(mpc::drive_plant_vals_of(p, mv, plant, ld, i)) {
    if (latency) {
      const mpc::DriveLatency dl = mpc::drive_latency_of(O, latency, ld, i);
      sub_old = dl.sub_old; sub_new = dl.sub_new;
    }
  }
};
}  // namespace

/* window indices of `count` points */
extern "C" int mpc_drive_twin_window(const double *tx, const double *ty, int n, int64_t count, const double *x, const double *y, int32_t *k) {
  if (!tx || !ty || n < 3 || n > MPC_DRIVE_MAX_TRACK) return MPC_ERR_INVALID;
  for (int64_t i = 0; i < count; i++) k[i] = mpc::drive_window(tx, ty, n, x[i], y[i]);
  return MPC_OK;
}

/* the plant on car [6][ld] in place, reply cmd [2][ld]: opts->sub_old / sub_new substeps of length opts->h, or the counts of the car's
 * column of latency; model, latency and plant as for mpc_drive_batch_host_plant, each may be NULL; ok [ld] or NULL: whether the car's
 * plant column could be used */
extern "C" int mpc_drive_twin_plant(const MpcParams *p, int64_t B, int64_t ld, double *car, const double *cmd, const double *model,
                                    const double *latency, const double *plant, const MpcDriveOpts *opts, int32_t *ok) {
  if (!p || ld < B || !car || !cmd || !opts || opts->sub_old < 0 || opts->sub_new < 0 || opts->sub_old + opts->sub_new > 1000) return MPC_ERR_INVALID;
  for (int64_t i = 0; i < B; i++) {
    double c[6];
    for (int q = 0; q < 6; q++) c[q] = car[q * ld + i];
    const PlantSide s(*p, *opts, model, latency, plant, ld, i);
    mpc::drive_plant(*p, s.mv, s.pv, c, cmd[i], cmd[ld + i], s.sub_old, s.sub_new, opts->h);
    for (int q = 0; q < 6; q++) car[q * ld + i] = c[q];
    if (ok) ok[i] = s.pv.ok ? 1 : 0;
  }
  return MPC_OK;
}

/* One handler call on cars [6][ld] with the windows that start at k [ld]: the arguments of mpc_telemetry_batch_host_horizon with the
 * window named by its index, plus weights, iterations and the two rows cte0 / epsi0 [2][ld].  comp [ld] or NULL (opts->extra_latency);
 * model, horizon, warm_in / warm_out may be NULL. */
extern "C" int mpc_drive_twin_handler(const MpcParams *p, int64_t B, int64_t ld, const double *car, const double *comp, const int32_t *k,
                                      const double *tx, const double *ty, int n_track, const double *weights, const double *model,
                                      const int32_t *horizon, const MpcDriveOpts *opts, const double *warm_in, const int32_t *warm_status,
                                      double *warm_out, int64_t ld_warm, const MpcWarmOpts *warm_opts, double *cmd, int32_t *status, int32_t *iters,
                                      double *cte_epsi) {
  if (bad_opts(p, opts, warm_opts, n_track) || ld < B || !car || !k || !tx || !ty || !cmd || !status || !iters || ((warm_in || warm_out) && ld_warm < B))
    return MPC_ERR_INVALID;
  Rows R(*p, ld);
  const mpc::WarmCall W{warm_in, warm_status, warm_out, ld_warm, *warm_opts, 1};
  for (int64_t i = 0; i < B; i++) {
    if (k[i] < 0 || k[i] >= n_track) return MPC_ERR_INVALID;
    handler_of(*p, model, horizon, comp ? comp + i : nullptr, *opts, R, i, ld, car, tx, ty, n_track, k[i], weights, W, cmd, status, iters);
    if (cte_epsi) { cte_epsi[i] = R.pre[(mpc::RUN_PRE_STATE + 4) * ld + i]; cte_epsi[ld + i] = R.pre[(mpc::RUN_PRE_STATE + 5) * ld + i]; }
  }
  return MPC_OK;
}

/* The arguments of mpc_drive_batch_host_plant: step by step, every car of a step before the next step (the stepwise definition).
 * handler_status [steps][ld] or NULL: the handler's own status of every step, which the warm rule reads. */
extern "C" int mpc_drive_twin(const MpcParams *p, int64_t B, int64_t ld, int steps, double *car, const double *tx, const double *ty, int n_track,
                              const double *weights, const double *model, const int32_t *horizon, const double *latency, const double *plant,
                              const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary, double *hist, int32_t *status, int32_t *iters,
                              int32_t *handler_status) {
  if (bad_opts(p, opts, warm_opts, n_track) || B < 0 || ld < B || steps < 1 || !car || !tx || !ty || !summary || !status) return MPC_ERR_INVALID;
  Rows R(*p, ld);
  std::vector<double> warm(opts->warm_start ? (size_t)(p->N - 1) * MPC_WARM_REC * ld : 0);      /* (the rows of the handle's N) */
  std::vector<int32_t> st(ld, 0), it(ld, 0), kbuf(2 * ld, 0);
  for (int t = 0; t < steps; t++) {
    int32_t *k_now = kbuf.data() + (int64_t)(t & 1) * ld, *k_prev = kbuf.data() + (int64_t)((t & 1) ^ 1) * ld;
    const mpc::WarmCall W = opts->warm_start ? mpc::WarmCall{t == 0 ? nullptr : warm.data(), st.data(), warm.data(), ld, *warm_opts, 1}
                                             : mpc::WarmCall{nullptr, nullptr, nullptr, ld, *warm_opts, 1};
    for (int64_t i = 0; i < B; i++) {
      k_now[i] = mpc::drive_window(tx, ty, n_track, car[i], car[ld + i]);
      double comp = 0.0;
      if (latency) comp = mpc::drive_latency_of(*opts, latency, ld, i).comp;
      handler_of(*p, model, horizon, latency ? &comp : nullptr, *opts, R, i, ld, car, tx, ty, n_track, k_now[i], weights, W, R.cmd, st.data(), it.data());
      if (handler_status) handler_status[(int64_t)t * ld + i] = st[i];
    }
    for (int64_t i = 0; i < B; i++) {
      const PlantSide s(*p, *opts, model, latency, plant, ld, i);
      mpc::drive_step_instance(*p, s.mv, s.pv, *opts, s.sub_old, s.sub_new, i, ld, t, n_track, car, R.cmd, R.pre, ld, st[i], it[i], k_now[i], k_prev[i],
                               summary, hist ? hist + (int64_t)t * MPC_DRIVE_REC * ld : nullptr, status, iters);
    }
  }
  return MPC_OK;
}
