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

/* ---- noise: what a car's sensors, actuator and link add per message (include/mpc_amd_noise.h) ----------------------------------------
 * Philox4x32-10 as published (Salmon, Moraes, Dror, Shaw, SC'11): multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 /
 * 0xBB67AE85, ten rounds; counter-based, no state.  Plain C++: the high word of a product is __umulhi on the device and the upper half
 * of a 64-bit product on the host. */
MPC_HD uint32_t philox_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}
MPC_HD void philox4x32(const uint32_t *ctr, const uint32_t *key, uint32_t *out) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
  MPC_UNROLL
  for (int r = 0; r < 10; r++) {
    const uint32_t hi0 = philox_mulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = philox_mulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
/* a word as a uniform inside (0, 1): (r + 0.5) * 2^-32, exact in a double */
MPC_HD double drive_uniform(uint32_t r) { return ((double)r + 0.5) * (1.0 / 4294967296.0); }
/* a normal pair from two words (Box-Muller on the project's own flog and fsincos) */
MPC_HD void drive_normal_pair(uint32_t ra, uint32_t rb, double *za, double *zb) {
  const double ua = drive_uniform(ra), ub = drive_uniform(rb);
  const double rad = sqrt(-2.0 * flog(ua));
  double sn, cs;
  fsincos(6.283185307179586 * ub, &sn, &cs);
  *za = rad * cs;
  *zb = rad * sn;
}
/* The rows of one draw, in the order of the blocks */
enum { DRIVE_Z_X = 0, DRIVE_Z_Y, DRIVE_Z_PSI, DRIVE_Z_SPEED, DRIVE_Z_STEER, DRIVE_Z_DRIFT, DRIVE_U_DROP, DRIVE_NDRAW };
/* THE draw of a car with seed s = k1 * 2^32 + k0 at message `step` (0-based): two blocks, key (k0, k1), counter (step, block, 0, 0).
 * Block 0, pairs (r0, r1), (r2, r3): z_x, z_y, z_psi, z_speed.  Block 1: pair (r0, r1): z_steer, z_drift; r2: u_drop; r3 is not used.
 * (seed, step) only: no instance index, batch size, leading dimension, lane or launch form enters.  The only place this is spelled;
 * every kernel and every CPU build calls it.  (Inlined like everything here: behind a call it cost every DRIVE build of the lane
 * kernel 16 B of scratch for the call's own frame, more than its temporaries cost inline; profiles/drive_noise_resources.md.) */
struct DriveDraw { double v[DRIVE_NDRAW]; };
MPC_HD DriveDraw drive_noise_draw(uint32_t k0, uint32_t k1, int32_t step) {
  DriveDraw d;
  const uint32_t key[2] = {k0, k1};
  uint32_t ctr[4] = {(uint32_t)step, 0u, 0u, 0u}, r[4];
  philox4x32(ctr, key, r);
  drive_normal_pair(r[0], r[1], d.v + DRIVE_Z_X, d.v + DRIVE_Z_Y);
  drive_normal_pair(r[2], r[3], d.v + DRIVE_Z_PSI, d.v + DRIVE_Z_SPEED);
  ctr[1] = 1u;
  philox4x32(ctr, key, r);
  drive_normal_pair(r[0], r[1], d.v + DRIVE_Z_STEER, d.v + DRIVE_Z_DRIFT);
  d.v[DRIVE_U_DROP] = drive_uniform(r[2]);
  return d;
}
/* ... for a seed as a column holds it (drive_seed_ok), into out7 */
MPC_HD void drive_noise_draw(double seed, int32_t step, double *out7) {
  const uint64_t s = (uint64_t)seed;
  const DriveDraw d = drive_noise_draw((uint32_t)s, (uint32_t)(s >> 32), step);
  MPC_UNROLL
  for (int q = 0; q < DRIVE_NDRAW; q++) out7[q] = d.v[q];
}
/* a seed as the column holds it: a double holding an integer, 0 <= s < 2^53 */
MPC_HD bool drive_seed_ok(double s) { return s >= 0.0 && s < 9007199254740992.0 && s == rint(s); }

/* Car i's column of noise [MPC_NNOISE][ld] (the mpc_drive_*_noise entry points), or with noise == nullptr the zero column.  A column
 * that cannot be used -- a value that is not finite, a sigma below 0, p_drop outside [0, 1], a seed that is no integer value or is
 * outside [0, 2^53) -- : the zero column and ok = false, which drive_step_instance turns into a status (the rule of a plant column). */
struct DriveNoise {
  uint32_t k0, k1;
  double pos, psi, speed, steer, drift, drop;
  bool ok;
  MPC_HD bool senses() const { return pos != 0.0 || psi != 0.0 || speed != 0.0; }
  MPC_HD bool acts() const { return steer != 0.0 || drift != 0.0 || drop != 0.0; }
};
MPC_HD DriveNoise drive_noise_of(const double *noise, int64_t ld, int64_t i) {
  DriveNoise d{0u, 0u, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, true};
  if (noise) {
    double c[MPC_NNOISE];
    bool ok = true;
    MPC_UNROLL
    for (int q = 0; q < MPC_NNOISE; q++) { c[q] = noise[q * ld + i]; ok = ok && drive_finite(c[q]); }
    MPC_UNROLL
    for (int q = MPC_NOISE_POS; q <= MPC_NOISE_DRIFT; q++) ok = ok && c[q] >= 0.0;
    ok = ok && c[MPC_NOISE_DROP] >= 0.0 && c[MPC_NOISE_DROP] <= 1.0 && drive_seed_ok(c[MPC_NOISE_SEED]);
    d.ok = ok;
    if (ok) {
      const uint64_t s = (uint64_t)c[MPC_NOISE_SEED];
      d.k0 = (uint32_t)s; d.k1 = (uint32_t)(s >> 32);
      d.pos = c[MPC_NOISE_POS]; d.psi = c[MPC_NOISE_PSI]; d.speed = c[MPC_NOISE_SPEED];
      d.steer = c[MPC_NOISE_STEER]; d.drift = c[MPC_NOISE_DRIFT]; d.drop = c[MPC_NOISE_DROP];
    }
  }
  return d;
}

/* What the handler is told about car i at message `step`: seen6 [6][lds], column i <- the car's rows 0..3 plus sigma * z, rows 4 / 5
 * as they are; seen_out (this step's block of the caller's `seen`, [4][ld]) or nullptr gets rows 0..3.  A row whose sigma is exactly 0
 * is copied, not added to (the zero column hands the car's own bits on, and draws nothing); sigma * z is a statement of its own, so
 * the sum is the rounded sum of the rounded product.  With sigma_speed > 0 the reading is max(0, speed + sigma * z): noise does not
 * manufacture a negative speed, which the handler would call a defect.  psi is not normalised: the handler does that. */
MPC_HD void drive_seen(const DriveNoise &nz, int32_t step, const double *car, int64_t ld, int64_t i, double *seen6, int64_t lds, double *seen_out) {
  double c[6];
  MPC_UNROLL
  for (int q = 0; q < 6; q++) c[q] = car[q * ld + i];
  if (nz.senses()) {
    const DriveDraw dr = drive_noise_draw(nz.k0, nz.k1, step);
    const double *z = dr.v;
    if (nz.pos != 0.0) {
      const double dx = nz.pos * z[DRIVE_Z_X], dy = nz.pos * z[DRIVE_Z_Y];
      c[0] = c[0] + dx;
      c[1] = c[1] + dy;
    }
    if (nz.psi != 0.0) {
      const double dp = nz.psi * z[DRIVE_Z_PSI];
      c[2] = c[2] + dp;
    }
    if (nz.speed != 0.0) {
      const double dv = nz.speed * z[DRIVE_Z_SPEED];
      const double v = c[3] + dv;
      c[3] = v < 0.0 ? 0.0 : v;
    }
  }
  MPC_UNROLL
  for (int q = 0; q < 6; q++) seen6[q * lds + i] = c[q];
  if (seen_out) {
    MPC_UNROLL
    for (int q = 0; q < 4; q++) seen_out[q * ld + i] = c[q];
  }
}

/* The plant column in force between message `step` and the next: bias + sigma_steer * z_steer, drift + sigma_drift * z_drift, on top
 * of the car's column or the default column, each a statement of its own and skipped where its sigma is 0 (drive_substep's rule:
 * what stood there before contracts as it did).  *dropped: u_drop < p_drop, the reply of this message never reaches the car. */
MPC_HD DrivePlantVals drive_plant_perturbed(DrivePlantVals pv, const DriveNoise &nz, int32_t step, bool *dropped) {
  *dropped = false;
  if (nz.acts()) {
    const DriveDraw dr = drive_noise_draw(nz.k0, nz.k1, step);
    const double *z = dr.v;
    if (nz.steer != 0.0) {
      const double db = nz.steer * z[DRIVE_Z_STEER];
      pv.bias = pv.bias + db;
    }
    if (nz.drift != 0.0) {
      const double dd = nz.drift * z[DRIVE_Z_DRIFT];
      pv.drift = pv.drift + dd;
    }
    *dropped = z[DRIVE_U_DROP] < nz.drop;
  }
  return pv;
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
 * (drive_plant_vals_of).  nz: the car's noise values (drive_noise_of): what this message adds to the plant column in force, and whether
 * its reply arrives.  A car whose plant column or noise column could not be used carries a status at every step: a step the handler ended
 * SUCCESS or ACCEPTABLE is recorded, summed and folded as INFEASIBLE; st_step itself, which the warm rule reads, is the caller's and
 * stays. */
template <class MV>
MPC_HD void drive_step_instance(const MpcParams &P, const MV &m, const DrivePlantVals &pv, const DriveNoise &nz, const MpcDriveOpts &O, int sub_old, int sub_new,
                                int64_t i, int64_t ld, int step, int n_track, double *car, const double *cmd, const double *pre, int64_t ldp, int32_t st_step,
                                int32_t it_step, int k, int k_prev, double *summary, double *rec, int32_t *status, int32_t *iters) {
  if (!(pv.ok && nz.ok) && (st_step == MPC_STATUS_SUCCESS || st_step == MPC_STATUS_ACCEPTABLE)) st_step = MPC_STATUS_INFEASIBLE;
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
  /* (a reply that never arrives is a reply that is not finite to the plant: the command in force stays; the record above holds what was sent) */
  bool dropped;
  const DrivePlantVals pn = drive_plant_perturbed(pv, nz, step, &dropped);
  drive_plant(P, m, pn, c, dropped ? NAN : cs, ct, sub_old, sub_new, O.h);
  MPC_UNROLL
  for (int q = 0; q < 6; q++) car[q * ld + i] = c[q];
}
/* The short call forms, as for drive_plant: without noise values (the zero column), without plant values (the default column of `m`),
 * without counts (the call's), without `m` (P itself); each forwards to the one body above. */
template <class MV>
MPC_HD void drive_step_instance(const MpcParams &P, const MV &m, const DrivePlantVals &pv, const MpcDriveOpts &O, int sub_old, int sub_new, int64_t i, int64_t ld,
                                int step, int n_track, double *car, const double *cmd, const double *pre, int64_t ldp, int32_t st_step, int32_t it_step, int k,
                                int k_prev, double *summary, double *rec, int32_t *status, int32_t *iters) {
  drive_step_instance(P, m, pv, drive_noise_of(nullptr, 0, 0), O, sub_old, sub_new, i, ld, step, n_track, car, cmd, pre, ldp, st_step, it_step, k, k_prev, summary,
                      rec, status, iters);
}
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
