/*
 * mpc_drive_core.h -- one car of the track-driving loop (include/mpc_amd_drive.h) between two calls of the telemetry handler: the
 * waypoint window at its position, the plant that moves it under the command it was sent, and what the call keeps per car.
 *
 * THE PLANT IS NOT THE UNITY SIMULATOR.  It is the reference's own model of it: Vehicle::move (src/model/Vehicle.cpp:145-168), the
 * kinematic step of the handler's latency compensation, fed the way the handler reads a telemetry message (mpc_main.cpp:129, :131,
 * :156).  One instance per lane, everything in registers; compiles for the device and, for the test-only CPU build
 * (tests/drive_twin), as plain C++.
 */
#ifndef MPC_DRIVE_CORE_H
#define MPC_DRIVE_CORE_H

#include "mpc_run_core.h"

namespace mpc {

MPC_HD bool drive_finite(double v) { return fabs(v) < HUGE_VAL; }

/* The window's first waypoint k (0 .. n-1) for a car at (x, y) on the cyclic track tx / ty [n]: j = the nearest waypoint (smallest
 * dx * dx + dy * dy; ties: the lowest index; not-a-number never wins: j = 0 for a position that is not finite), k = j if the car is
 * past it along the segment to the next one, (p - w_j) . (w_{j+1} - w_j) > 0, else the one before.  n trips, whatever the data; the
 * track is read at the loop index, the same address in every lane. */
MPC_HD int drive_window(const double *__restrict__ tx, const double *__restrict__ ty, int n, double x, double y) {
  double best = HUGE_VAL;
  int j = 0;
  MPC_STAGE_LOOP
  for (int q = 0; q < n; q++) {
    const double dx = x - tx[q], dy = y - ty[q];
    const double d = dx * dx + dy * dy;
    if (d < best) { best = d; j = q; }
  }
  const int jn = j + 1 == n ? 0 : j + 1;
  const double wx = tx[j], wy = ty[j];
  const double dot = (x - wx) * (tx[jn] - wx) + (y - wy) * (ty[jn] - wy);
  return dot > 0.0 ? j : (j == 0 ? n - 1 : j - 1);
}

/* w[k .. k + npts - 1], cyclically (npts <= n) -> ptsx / ptsy [npts][ld], column i */
MPC_HD void drive_window_points(const double *__restrict__ tx, const double *__restrict__ ty, int n, int k, int npts, double *ptsx,
                                double *ptsy, int64_t ld, int64_t i) {
  MPC_UNROLL
  for (int q = 0; q < RUN_MAX_PTS; q++) {
    if (q < npts) {
      int idx = k + q;
      if (idx >= n) idx -= n;
      ptsx[q * ld + i] = tx[idx]; ptsy[q * ld + i] = ty[idx];
    }
  }
}

/* the signed cyclic difference of two window indices: k - k_prev brought to (-n / 2, n / 2] */
MPC_HD int drive_progress(int k, int k_prev, int n) {
  int d = k - k_prev;
  if (d < 0) d += n;
  if (2 * d > n) d -= n;
  return d;
}

/* The plant's own values: what the car really turns and accelerates with, where the handler goes on believing `m`.  Lf in the heading
 * update; steer = -(steering_angle * gain + bias), bias in the simulator's sign like the angle; accel = (throttle - v / drag) * accel;
 * drift: a steady speed to the car's left [m/s].  ok: the caller's column could be used.  Every car of every entry point is moved
 * with one of these: its column of `plant` (the mpc_drive_*_plant entry points), or the default column, which is the plant of the
 * entry points without `plant` bit for bit (drive_substep). */
struct DrivePlantVals {
  double Lf, gain, bias, accel, drag, drift;
  bool ok;
};
/* Car i's column of plant [MPC_NPLANT][ld], or with plant == nullptr the default column {m.Lf, 1, 0, 6, 50, 0} (mpc_drive_plant_default
 * with the car's own Lf: the model's or the handle's).  A column that cannot be used -- a value that is not finite, Lf <= 0, drag <= 0
 * -- : the default column and ok = false, which drive_step_instance turns into a status. */
template <class MV>
MPC_HD DrivePlantVals drive_plant_vals_of(const MpcParams &P, const MV &m_, const double *plant, int64_t ld, int64_t i) {
  const MV &m = run_model_of(P, m_);
  DrivePlantVals d{m.Lf, 1.0, 0.0, 6.0, 50.0, 0.0, true};
  if (plant) {
    double c[MPC_NPLANT];
    bool ok = true;
    MPC_UNROLL
    for (int q = 0; q < MPC_NPLANT; q++) { c[q] = plant[q * ld + i]; ok = ok && drive_finite(c[q]); }
    ok = ok && c[MPC_PLANT_LF] > 0.0 && c[MPC_PLANT_DRAG_SPEED] > 0.0;
    d.ok = ok;
    if (ok) {
      d.Lf = c[MPC_PLANT_LF]; d.gain = c[MPC_PLANT_STEER_GAIN]; d.bias = c[MPC_PLANT_STEER_BIAS];
      d.accel = c[MPC_PLANT_ACCEL_GAIN]; d.drag = c[MPC_PLANT_DRAG_SPEED]; d.drift = c[MPC_PLANT_DRIFT];
    }
  }
  return d;
}

/* Where the plant reads max_steering, and the default column its Lf: `m`, the template argument of mpc_run_core.h's functions
 * (run_model_of) -- the car's mpc::ModelVals (its column of `model`; one that cannot be used has become the handle's values there,
 * model_vals_of; without `model`, ModelVals::of(P)) or the handle's MpcParams itself. */
/* One plant substep of length h on car = {x, y, psi, speed [mph], steering_angle, throttle}: the handler's reading of the message
 * (MpH2MpS mpc_main.cpp:129, the sign :131, the acceleration :156 -- from the speed of this substep), Vehicle::move(h)
 * (Vehicle.cpp:145-168; the clamp at :156 is overwritten at :167), the speed back to mph (MpS2MpH, utils.h:19-21).
 * The terms a plant column adds are statements of their own behind the expressions that stood here before there were plant columns,
 * so those contract as they did (-ffp-contract=on works within a statement) and the default column {Lf, 1, 0, 6, 50, 0} gives their
 * bits: a product with 1, a difference with 0, and a drift of 0 that adds +-0 to a coordinate. */
MPC_HD void drive_substep(const DrivePlantVals &pv, double *car, double h) {
  const double Lf = pv.Lf, drag = pv.drag, acc = pv.accel;
  const double v = car[3] * 1609.34 / 3600.0;
  double steer = -car[4];
  steer = steer * pv.gain;
  steer = steer - pv.bias;
  const double accel = (car[5] - v / drag) * acc;
  const double dist = v * h;
  double sn, cs;
  fsincos(car[2], &sn, &cs);
  double x = car[0] + dist * cs;
  double y = car[1] + dist * sn;
  const double side = pv.drift * h;
  x = x - side * sn;
  y = y + side * cs;
  car[0] = x;
  car[1] = y;
  car[2] = car[2] + steer * dist / Lf;
  car[3] = (v + accel * h) * 3600.0 / 1609.34;
}

/* The plant between two messages: sub_old substeps under the command in force (rows 4 / 5), then the reply takes effect --
 * (cmd_steer * max_steering, cmd_throttle), the controller's normalisation whatever the plant column says; a reply that is not finite
 * leaves the old command in force --, then sub_new substeps.  psi is not normalised: the handler does that. */
template <class MV>
MPC_HD void drive_plant(const MpcParams &P, const MV &m_, const DrivePlantVals &pv, double *car, double cmd_steer, double cmd_throttle, int sub_old, int sub_new, double h) {
  const MV &m = run_model_of(P, m_);
  MPC_STAGE_LOOP
  for (int s = 0; s < sub_old; s++) drive_substep(pv, car, h);
  if (drive_finite(cmd_steer) && drive_finite(cmd_throttle)) { car[4] = cmd_steer * m.max_steering; car[5] = cmd_throttle; }
  MPC_STAGE_LOOP
  for (int s = 0; s < sub_new; s++) drive_substep(pv, car, h);
}
/* The short call forms -- without plant values: the default column of `m`; without `m`: P itself.  CPU builds that include this header
 * (test builds of other commits among them) call these; they forward to the one body above and add no path of their own
 * (tests/cpp/drive_call_forms_test.cpp holds them to its bits).  The device code calls the full form only. */
template <class MV>
MPC_HD void drive_plant(const MpcParams &P, const MV &m, double *car, double cmd_steer, double cmd_throttle, int sub_old, int sub_new, double h) {
  drive_plant(P, m, drive_plant_vals_of(P, m, nullptr, 0, 0), car, cmd_steer, cmd_throttle, sub_old, sub_new, h);
}
MPC_HD void drive_plant(const MpcParams &P, double *car, double cmd_steer, double cmd_throttle, int sub_old, int sub_new, double h) {
  drive_plant(P, P, car, cmd_steer, cmd_throttle, sub_old, sub_new, h);
}

/* Car i's column of latency [MPC_NLATENCY][ld] (the mpc_drive_*_latency entry points): the seconds its handler compensates for and its
 * own substep counts, doubles holding integer values.  A column that cannot be used -- a value that is not finite, comp < 0, a count
 * that is no integer or below 0, sub_old + sub_new outside 1..1000 -- : comp is not-a-number, which the handler turns into a status
 * (mpc::run_comp_ok), and the counts are the call's.  The counts handed on are checked: 0 .. 1000, whatever the array holds. */
struct DriveLatency {
  double comp;
  int sub_old, sub_new;
};
MPC_HD DriveLatency drive_latency_of(const MpcDriveOpts &O, const double *latency, int64_t ld, int64_t i) {
  const double c = latency[MPC_LATENCY_COMP * ld + i], so = latency[MPC_LATENCY_SUB_OLD * ld + i], sn = latency[MPC_LATENCY_SUB_NEW * ld + i];
  const bool ok = run_comp_usable(c) && so >= 0.0 && sn >= 0.0 && so + sn >= 1.0 && so + sn <= 1000.0 && so == rint(so) && sn == rint(sn);
  DriveLatency L;
  L.comp = ok ? c : NAN;
  L.sub_old = ok ? (int)so : O.sub_old;
  L.sub_new = ok ? (int)sn : O.sub_new;
  return L;
}

/* The summary rows of one car (MPC_DRIVE_SUM_*), step `step` (0-based) folded in; dk = the progress of this step (0 at step 0).
 * A not-a-number never wins a maximum or the minimum. */
MPC_HD void drive_summary(int step, double *sum, double cte0, double epsi0, double speed, int dk, int status, double cte_limit) {
  const double ac = fabs(cte0), ae = fabs(epsi0);
  const bool first = step == 0;
  const double m0 = first ? 0.0 : sum[MPC_DRIVE_SUM_MAX_CTE], m2 = first ? 0.0 : sum[MPC_DRIVE_SUM_MAX_EPSI];
  const double m4 = first ? HUGE_VAL : sum[MPC_DRIVE_SUM_MIN_SPEED];
  sum[MPC_DRIVE_SUM_MAX_CTE] = ac > m0 ? ac : m0;
  sum[MPC_DRIVE_SUM_CTE2] = (first ? 0.0 : sum[MPC_DRIVE_SUM_CTE2]) + cte0 * cte0;
  sum[MPC_DRIVE_SUM_MAX_EPSI] = ae > m2 ? ae : m2;
  sum[MPC_DRIVE_SUM_SPEED] = (first ? 0.0 : sum[MPC_DRIVE_SUM_SPEED]) + speed;
  sum[MPC_DRIVE_SUM_MIN_SPEED] = speed < m4 ? speed : m4;
  sum[MPC_DRIVE_SUM_PROGRESS] = (first ? 0.0 : sum[MPC_DRIVE_SUM_PROGRESS]) + (double)dk;
  const double off = first ? -1.0 : sum[MPC_DRIVE_SUM_FIRST_OFF];
  sum[MPC_DRIVE_SUM_FIRST_OFF] = (off < 0.0 && ac > cte_limit) ? (double)step : off;
  sum[MPC_DRIVE_SUM_FAILED] = (first ? 0.0 : sum[MPC_DRIVE_SUM_FAILED]) + (status != MPC_STATUS_SUCCESS ? 1.0 : 0.0);
}

/* ---- one car of a batch between the handler's reply and the next message, as the plant-and-summary kernel and the CPU build run it:
 * car [6][ld] in / out, cmd [2][ld], pre [RUN_PRE_ROWS][ldp] (the handler's own rows: cte0, epsi0), the step's status and iterations,
 * the window index of this step and of the one before; sub_old / sub_new: the car's substep counts (its latency column's, or the
 * call's); summary [MPC_DRIVE_NSUM][ld], rec = this step's block of hist [MPC_DRIVE_REC][ld] or nullptr, status / iters (or nullptr)
 * per car: worst code, summed iterations (mpc::RolloutCar).  m: the plant's model values, as above.  pv: the plant's own values
 * (drive_plant_vals_of).  A car whose plant column could not be used carries a status at every step: a step the handler ended
 * SUCCESS or ACCEPTABLE is recorded, summed and folded as INFEASIBLE; st_step itself, which the warm rule reads, is the caller's and
 * stays. */
template <class MV>
MPC_HD void drive_step_instance(const MpcParams &P, const MV &m, const DrivePlantVals &pv, const MpcDriveOpts &O, int sub_old, int sub_new, int64_t i, int64_t ld,
                                int step, int n_track, double *car, const double *cmd, const double *pre, int64_t ldp, int32_t st_step, int32_t it_step, int k,
                                int k_prev, double *summary, double *rec, int32_t *status, int32_t *iters) {
  if (!pv.ok && (st_step == MPC_STATUS_SUCCESS || st_step == MPC_STATUS_ACCEPTABLE)) st_step = MPC_STATUS_INFEASIBLE;
  double c[6], sum[MPC_DRIVE_NSUM] = {};
  MPC_UNROLL
  for (int q = 0; q < 6; q++) c[q] = car[q * ld + i];
  const double cs = cmd[i], ct = cmd[ld + i];
  const double cte0 = pre[(RUN_PRE_STATE + 4) * ldp + i], epsi0 = pre[(RUN_PRE_STATE + 5) * ldp + i];
  if (rec) {
    MPC_UNROLL
    for (int q = 0; q < 6; q++) rec[(MPC_DRIVE_REC_CAR + q) * ld + i] = c[q];
    rec[MPC_DRIVE_REC_CMD * ld + i] = cs; rec[(MPC_DRIVE_REC_CMD + 1) * ld + i] = ct;
    rec[MPC_DRIVE_REC_CTE * ld + i] = cte0; rec[MPC_DRIVE_REC_EPSI * ld + i] = epsi0;
    rec[MPC_DRIVE_REC_STATUS * ld + i] = (double)st_step; rec[MPC_DRIVE_REC_ITERS * ld + i] = (double)it_step;
    rec[MPC_DRIVE_REC_K * ld + i] = (double)k;
  }
  if (step > 0) {
    MPC_UNROLL
    for (int q = 0; q < MPC_DRIVE_NSUM; q++) sum[q] = summary[q * ld + i];
  }
  drive_summary(step, sum, cte0, epsi0, c[3], step > 0 ? drive_progress(k, k_prev, n_track) : 0, st_step, O.cte_limit);
  MPC_UNROLL
  for (int q = 0; q < MPC_DRIVE_NSUM; q++) summary[q * ld + i] = sum[q];
  int32_t worst = 0, total = 0;
  if (step > 0) worst = status[i];
  status[i] = RolloutCar::fold_status(step, worst, st_step);
  if (iters) {
    if (step > 0) total = iters[i];
    iters[i] = RolloutCar::sum_iters(step, total, it_step);
  }
  drive_plant(P, m, pv, c, cs, ct, sub_old, sub_new, O.h);
  MPC_UNROLL
  for (int q = 0; q < 6; q++) car[q * ld + i] = c[q];
}
/* The short call forms, as for drive_plant: without plant values (the default column of `m`), without counts (the call's), without `m`
 * (P itself); each forwards to the one body above. */
template <class MV>
MPC_HD void drive_step_instance(const MpcParams &P, const MV &m, const MpcDriveOpts &O, int sub_old, int sub_new, int64_t i, int64_t ld, int step, int n_track,
                                double *car, const double *cmd, const double *pre, int64_t ldp, int32_t st_step, int32_t it_step, int k, int k_prev,
                                double *summary, double *rec, int32_t *status, int32_t *iters) {
  drive_step_instance(P, m, drive_plant_vals_of(P, m, nullptr, 0, 0), O, sub_old, sub_new, i, ld, step, n_track, car, cmd, pre, ldp, st_step, it_step, k, k_prev,
                      summary, rec, status, iters);
}
template <class MV>
MPC_HD void drive_step_instance(const MpcParams &P, const MV &m, const MpcDriveOpts &O, int64_t i, int64_t ld, int step, int n_track, double *car,
                                const double *cmd, const double *pre, int64_t ldp, int32_t st_step, int32_t it_step, int k, int k_prev,
                                double *summary, double *rec, int32_t *status, int32_t *iters) {
  drive_step_instance(P, m, O, O.sub_old, O.sub_new, i, ld, step, n_track, car, cmd, pre, ldp, st_step, it_step, k, k_prev, summary, rec, status, iters);
}
MPC_HD void drive_step_instance(const MpcParams &P, const MpcDriveOpts &O, int64_t i, int64_t ld, int step, int n_track, double *car,
                                const double *cmd, const double *pre, int64_t ldp, int32_t st_step, int32_t it_step, int k, int k_prev,
                                double *summary, double *rec, int32_t *status, int32_t *iters) {
  drive_step_instance(P, P, O, i, ld, step, n_track, car, cmd, pre, ldp, st_step, it_step, k, k_prev, summary, rec, status, iters);
}

}  // namespace mpc
#endif
