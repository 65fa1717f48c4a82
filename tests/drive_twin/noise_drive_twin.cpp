/*
 * noise_drive_twin.cpp -- TEST-ONLY CPU build of the track-driving loop under noise (include/mpc_amd_noise.h), in its stepwise
 * definition: mpc_drive_batch_host_noise with an MpcParams in the place of the handle.
 *
 * tests/drive_twin/budget_drive_twin.cpp's loop with one more nullable per-car array, `noise`, and one more nullable output, `seen`:
 * the same functions of mpc_drive_core.h (window, what the handler is told, plant, summary) around the same per-instance driver.  Per
 * message the window is chosen from the true car, mpc::drive_seen writes the car's column of the seen rows, the handler is pointed at
 * those, and mpc::drive_step_instance is handed the car's mpc::DriveNoise.  noise == NULL and seen == NULL is budget_drive_twin.cpp's
 * loop, and a test holds it to that library's bits.  Compiled into a library of its own by tests/noise_helpers.py.  Never linked
 * into the product library.
 */
#include <cmath>
#include <cstdint>
#include <vector>

#include "mpc_drive_core.h"

namespace {
struct WS : mpc::HostWorkspace<double> {
  static constexpr bool kBudget = true;
};
using SV = mpc::Solver<WS, double>;

bool bad_opts(const MpcParams *p, const MpcDriveOpts *o, const MpcWarmOpts *w, int n_track) {
  return !p || p->N < 3 || p->N > MPC_MAX_N || !o || o->size != (int32_t)sizeof(MpcDriveOpts) || o->npts < 3 || o->npts > mpc::RUN_MAX_PTS ||
         n_track < o->npts || n_track > MPC_DRIVE_MAX_TRACK || !w || w->size != (int32_t)sizeof(MpcWarmOpts) || o->sub_old < 0 || o->sub_new < 0 ||
         o->sub_old + o->sub_new < 1 || o->sub_old + o->sub_new > 1000;
}

mpc::ModelVals vals_of(const MpcParams &p, const double *model, int64_t ld, int64_t i) {
  return model ? mpc::model_vals_of(p, model, ld, i) : mpc::ModelVals::of(p);
}

/* the scratch rows of one call: ptsx / ptsy [RUN_MAX_PTS][ld], pre [RUN_PRE_ROWS][ld], out9 [9][ld], cmd [2][ld], seen6 [6][ld] */
struct Rows {
  std::vector<double> wsbuf, buf;
  double *ptsx, *ptsy, *pre, *out9, *cmd, *seen6;
  Rows(const MpcParams &p, int64_t ld)
      : wsbuf((size_t)mpc::workspace_fields_per_instance(p.N, false, true)), buf((size_t)(2 * mpc::RUN_MAX_PTS + mpc::RUN_PRE_ROWS + 9 + 2 + 6) * ld),
        ptsx(buf.data()), ptsy(ptsx + mpc::RUN_MAX_PTS * ld), pre(ptsy + mpc::RUN_MAX_PTS * ld), out9(pre + mpc::RUN_PRE_ROWS * ld), cmd(out9 + 9 * ld), seen6(cmd + 2 * ld) {}
};

/* the handler for car i on the window that starts at waypoint k (budget_drive_twin.cpp's handler_one; `car`: what the handler is told) */
template <class MV, class Col, class LC>
void handler_one(const MpcParams &p, const MV &mv, const Col &col, const LC &lc, bool budgeted, Rows &R, int64_t i, int64_t ld, const double *car,
                 const double *tx, const double *ty, int n_track, int k, int npts, const double *weights, const mpc::WarmCall &W, double *cmd,
                 int32_t *status, int32_t *iters) {
  mpc::drive_window_points(tx, ty, n_track, k, npts, R.ptsx, R.ptsy, ld, i);
  mpc::run_pre_instance<true>(p, mv, i, ld, npts, car, lc, R.ptsx, R.ptsy, R.pre, ld);
  double st[6], cf[MPC_NCOEF], w[MPC_NW];
  mpc::gather_instance(p, i, ld, R.pre + mpc::RUN_PRE_STATE * ld, R.pre + mpc::RUN_PRE_COEFFS * ld, weights, st, cf, w);
  const double ylo = R.pre[mpc::RUN_PRE_YAW_LO * ld + i], yhi = R.pre[mpc::RUN_PRE_YAW_HI * ld + i];
  WS ws;
  ws.base = R.wsbuf.data();
  SV S(p, ws);
  const mpc::WarmStart warm = W.instance(i, ylo, yhi, budgeted);
  status[i] = mpc::instance_solve(S, col, warm, st, cf, ylo, yhi, w);
  double *o = R.out9 + i;
  iters[i] = mpc::instance_store(S, col, warm, [o, ld](int q) -> double & { return o[q * ld]; }, [o](int) -> double & { return o[0]; }, false,
                                 ylo, yhi);
  mpc::run_post_instance(p, mv, i, R.pre, ld, R.out9, ld, nullptr, cmd, ld);
}

template <class LC>
void handler_with(const MpcParams &p, const double *model, const int32_t *horizon, const int32_t *budget, const LC &lc, Rows &R, int64_t i, int64_t ld,
                  const double *car, const double *tx, const double *ty, int n_track, int k, int npts, const double *weights, const mpc::WarmCall &W,
                  double *cmd, int32_t *status, int32_t *iters) {
  if (horizon || budget)
    handler_one(p, vals_of(p, model, ld, i),
                mpc::HorizonColumn{model ? model + i : nullptr, ld, horizon ? horizon[i] : p.N, budget ? budget[i] : (int)mpc::kNoBudget}, lc, budget != nullptr, R,
                i, ld, car, tx, ty, n_track, k, npts, weights, W, cmd, status, iters);
  else if (model)
    handler_one(p, mpc::model_vals_of(p, model, ld, i), mpc::ModelColumn{model + i, ld}, lc, false, R, i, ld, car, tx, ty, n_track, k, npts, weights, W, cmd,
                status, iters);
  else
    handler_one(p, p, mpc::NoColumn{}, lc, false, R, i, ld, car, tx, ty, n_track, k, npts, weights, W, cmd, status, iters);
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

/* One handler call on what it is told, car [6][ld], with the windows that start at k [ld] (budget_drive_twin.cpp's handler, as it is):
 * comp [ld] or NULL (opts->extra_latency); model, horizon, budget, warm_in / warm_out may be NULL. */
extern "C" int mpc_noise_drive_twin_handler(const MpcParams *p, int64_t B, int64_t ld, const double *car, const double *comp, const int32_t *k,
                                             const double *tx, const double *ty, int n_track, const double *weights, const double *model,
                                             const int32_t *horizon, const int32_t *budget, const MpcDriveOpts *opts, const double *warm_in,
                                             const int32_t *warm_status, double *warm_out, int64_t ld_warm, const MpcWarmOpts *warm_opts, double *cmd,
                                             int32_t *status, int32_t *iters, double *cte_epsi) {
  if (bad_opts(p, opts, warm_opts, n_track) || ld < B || !car || !k || !tx || !ty || !cmd || !status || !iters || ((warm_in || warm_out) && ld_warm < B))
    return MPC_ERR_INVALID;
  Rows R(*p, ld);
  const mpc::WarmCall W{warm_in, warm_status, warm_out, ld_warm, *warm_opts, 1};
  for (int64_t i = 0; i < B; i++) {
    if (k[i] < 0 || k[i] >= n_track) return MPC_ERR_INVALID;
    if (comp) handler_with(*p, model, horizon, budget, mpc::RunComp{true, comp[i]}, R, i, ld, car, tx, ty, n_track, k[i], opts->npts, weights, W, cmd, status, iters);
    else handler_with(*p, model, horizon, budget, opts->extra_latency, R, i, ld, car, tx, ty, n_track, k[i], opts->npts, weights, W, cmd, status, iters);
    if (cte_epsi) { cte_epsi[i] = R.pre[(mpc::RUN_PRE_STATE + 4) * ld + i]; cte_epsi[ld + i] = R.pre[(mpc::RUN_PRE_STATE + 5) * ld + i]; }
  }
  return MPC_OK;
}

/* The arguments of mpc_drive_batch_host_noise: step by step, every car of a step before the next step (the stepwise definition).
 * handler_status [steps][ld] or NULL: the handler's own status of every step, which the warm rule reads. */
extern "C" int mpc_noise_drive_twin(const MpcParams *p, int64_t B, int64_t ld, int steps, double *car, const double *tx, const double *ty, int n_track,
                                     const double *weights, const double *model, const int32_t *horizon, const int32_t *budget, const double *latency,
                                     const double *plant, const double *noise, const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary,
                                     double *hist, double *seen, int32_t *status, int32_t *iters, int32_t *handler_status) {
  if (bad_opts(p, opts, warm_opts, n_track) || B < 0 || ld < B || steps < 1 || !car || !tx || !ty || !summary || !status) return MPC_ERR_INVALID;
  Rows R(*p, ld);
  std::vector<double> warm(opts->warm_start ? (size_t)(p->N - 1) * MPC_WARM_REC * ld : 0);      /* (the rows of the handle's N) */
  std::vector<int32_t> st(ld, 0), it(ld, 0), kbuf(2 * ld, 0);
  for (int t = 0; t < steps; t++) {
    int32_t *k_now = kbuf.data() + (int64_t)(t & 1) * ld, *k_prev = kbuf.data() + (int64_t)((t & 1) ^ 1) * ld;
    const mpc::WarmCall W = opts->warm_start ? mpc::WarmCall{t == 0 ? nullptr : warm.data(), st.data(), warm.data(), ld, *warm_opts, 1}
                                             : mpc::WarmCall{nullptr, nullptr, nullptr, ld, *warm_opts, 1};
    const bool senses = noise || seen;
    const double *tel = senses ? R.seen6 : car;
    for (int64_t i = 0; i < B; i++) {
      k_now[i] = mpc::drive_window(tx, ty, n_track, car[i], car[ld + i]);
      if (senses) mpc::drive_seen(mpc::drive_noise_of(noise, ld, i), t, car, ld, i, R.seen6, ld, seen ? seen + (int64_t)t * 4 * ld : nullptr);
      if (latency)
        handler_with(*p, model, horizon, budget, mpc::RunComp{true, mpc::drive_latency_of(*opts, latency, ld, i).comp}, R, i, ld, tel, tx, ty, n_track, k_now[i],
                     opts->npts, weights, W, R.cmd, st.data(), it.data());
      else
        handler_with(*p, model, horizon, budget, opts->extra_latency, R, i, ld, tel, tx, ty, n_track, k_now[i], opts->npts, weights, W, R.cmd, st.data(), it.data());
      if (handler_status) handler_status[(int64_t)t * ld + i] = st[i];
    }
    for (int64_t i = 0; i < B; i++) {
      const PlantSide s(*p, *opts, model, latency, plant, ld, i);
      mpc::drive_step_instance(*p, s.mv, s.pv, mpc::drive_noise_of(noise, ld, i), *opts, s.sub_old, s.sub_new, i, ld, t, n_track, car, R.cmd, R.pre, ld, st[i], it[i], k_now[i], k_prev[i],
                               summary, hist ? hist + (int64_t)t * MPC_DRIVE_REC * ld : nullptr, status, iters);
    }
  }
  return MPC_OK;
}

/* mpc::drive_noise_draw and mpc::philox4x32 as this build compiles them (the product library's host evaluation is mpc_drive_noise_draw) */
extern "C" int mpc_noise_drive_twin_draw(double seed, int32_t step, double *out7) {
  if (!out7 || !mpc::drive_finite(seed) || !mpc::drive_seed_ok(seed) || step < 0) return MPC_ERR_INVALID;
  mpc::drive_noise_draw(seed, step, out7);
  return MPC_OK;
}
