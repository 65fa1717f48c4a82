/*
 * mpc_run_core.h -- per-instance pre/post-processing of MPC::run().
 *
 * What the reference does around solve() in MPC::run (src/control/MPC.cpp:327-382), for one instance:
 *   pre:  Vehicle::globalToVehicle on the waypoints (Vehicle.cpp:105-114), RoadGeometry::fit with adaptive
 *         order 2..maxFitOrder-1 (RoadGeometry.cpp:18-34; polyfit = Vandermonde + Householder QR,
 *         utils.cpp:10-29), cte0 = f(0), epsi0 = -atan(c1), computeOrientationChange, speed tables,
 *         yaw bounds, state = (0,0,0,v,cte0,epsi0)                        (MPC.cpp:329-356)
 *   post: steering adjustment, acceleration clamp, steering normalisation   (MPC.cpp:360-381)
 * One instance per lane; everything in registers (the least-squares problem is at most 8 x 5).
 * Compiles for the device and, for the test-only host build, with g++.
 */
#ifndef MPC_RUN_CORE_H
#define MPC_RUN_CORE_H

#include <type_traits>

#include "mpc_core.h"

namespace mpc {

enum : int { RUN_MAX_PTS = 8 };
#define RUN_MAX_STEERING_ANGLE 1.57079632679489661923   /* rad: the largest |steering| of a pose / |steering_angle| of a telemetry row that is taken as one */

/* Rows of `pre` [RUN_PRE_ROWS][ld], what the pre-solve half hands to the solve and to the post-solve half (and to the caller who
 * asks for it): the solve's inputs first, in the order a solve call takes them */
enum : int {
  RUN_PRE_STATE = 0,              /* 6 rows */
  RUN_PRE_COEFFS = 6,             /* MPC_NCOEF rows */
  RUN_PRE_YAW_LO = 11,
  RUN_PRE_YAW_HI = 12,
  RUN_PRE_MAX_YAW_CHANGE = 13,
  RUN_PRE_TARGET_SPEED = 14,
  RUN_PRE_ROWS = 15
};
static_assert(RUN_PRE_COEFFS + MPC_NCOEF == RUN_PRE_YAW_LO, "the rows of pre");

/* least squares min ||A c - y|| with A[i][j] = x_i^j, i < n <= 8, j < NC, by Householder QR (the
 * factorisation Eigen's householderQr() performs in utils.cpp:24-26); everything unrolled */
template <int NC>
MPC_HD void polyfit_qr(const double *x, const double *y, int n, double *coef) {
  double A[RUN_MAX_PTS][NC], b[RUN_MAX_PTS];
  MPC_UNROLL
  for (int i = 0; i < RUN_MAX_PTS; i++) {
    const bool in = i < n;
    double pw = in ? 1.0 : 0.0;
    MPC_UNROLL
    for (int j = 0; j < NC; j++) { A[i][j] = pw; pw *= x[i]; }
    b[i] = in ? y[i] : 0.0;
  }
  MPC_UNROLL
  for (int k = 0; k < NC; k++) {
    double nrm2 = 0.0;
    MPC_UNROLL
    for (int i = k; i < RUN_MAX_PTS; i++) nrm2 += A[i][k] * A[i][k];
    const double nrm = sqrt(nrm2);
    const double alpha = A[k][k] > 0.0 ? -nrm : nrm;
    const double vk = A[k][k] - alpha;
    double vn2 = vk * vk;
    MPC_UNROLL
    for (int i = k + 1; i < RUN_MAX_PTS; i++) vn2 += A[i][k] * A[i][k];
    const double beta = vn2 > 0.0 ? 2.0 / vn2 : 0.0;
    MPC_UNROLL
    for (int j = k + 1; j < NC; j++) {
      double sdot = vk * A[k][j];
      MPC_UNROLL
      for (int i = k + 1; i < RUN_MAX_PTS; i++) sdot += A[i][k] * A[i][j];
      sdot *= beta;
      A[k][j] -= sdot * vk;
      MPC_UNROLL
      for (int i = k + 1; i < RUN_MAX_PTS; i++) A[i][j] -= sdot * A[i][k];
    }
    {
      double sdot = vk * b[k];
      MPC_UNROLL
      for (int i = k + 1; i < RUN_MAX_PTS; i++) sdot += A[i][k] * b[i];
      sdot *= beta;
      b[k] -= sdot * vk;
      MPC_UNROLL
      for (int i = k + 1; i < RUN_MAX_PTS; i++) b[i] -= sdot * A[i][k];
    }
    A[k][k] = alpha;
  }
  MPC_UNROLL
  for (int k = NC - 1; k >= 0; k--) {
    double sacc = b[k];
    MPC_UNROLL
    for (int j = k + 1; j < NC; j++) sacc -= A[k][j] * coef[j];
    coef[k] = (A[k][k] != 0.0) ? sacc / A[k][k] : 0.0;
  }
}

MPC_HD double poly5(const double *c, double x) { return (((c[4] * x + c[3]) * x + c[2]) * x + c[1]) * x + c[0]; }
MPC_HD double poly5_der(const double *c, double x) { return ((4.0 * c[4] * x + 3.0 * c[3]) * x + 2.0 * c[2]) * x + c[1]; }

/* table lookups of Vehicle::computeSpeedTarget / computeYawChangeSpeedLimit (Vehicle.cpp:34-79) */
MPC_HD double table_lookup(const double *xs, int nx, const double *ys, int ny, double key, double maxv) {
  const double a = fabs(key);
  for (int i = 0; i < nx; i++)
    if (a <= xs[i]) return fmin(ys[i < ny ? i : ny - 1], maxv);
  return fmin(ys[ny - 1], maxv);
}

/* normalizeAngle (utils.h:87-92): an angle -> [-pi, pi).  The reference subtracts 2 pi until the value fits, a loop whose trip
 * count is the caller's number: 1.6e11 turns for psi = 1e12, and no end at all for an infinity or for |psi| above ~1e17, where
 * the subtraction no longer changes the value.  Here no trip count depends on data:
 *   |a| <= MPC_NORMALIZE_SEQ_RANGE (64 pi and a little)  the reference's sequential subtraction, at most NORMALIZE_SEQ_TURNS turns: bit for bit what
 *                                         the two while loops gave (202 - 32 * 2 pi < pi, so 32 turns reach the interval from there);
 *   beyond it, |a| < 1e9 (fsincos' range) ONE reduction a - rint(a / 2 pi) * 2 pi in a single FMA, then the turns above take the
 *                                         one step that may be left.  Against the exact remainder: within 4 ulp(|a|) -- a itself is
 *                                         only known to half an ulp, and the double 2 pi is off by 3.9e-17 relative, a third of one;
 *   not finite, or |a| >= 1e9             returned as it came: fsincos flags such an angle with not-a-number and the instance ends
 *                                         with a status (there is no such heading in this model). */
enum : int { NORMALIZE_SEQ_TURNS = 32 };
#define MPC_NORMALIZE_SEQ_RANGE 202.0
static_assert(MPC_NORMALIZE_SEQ_RANGE > 64.0 * M_PI && MPC_NORMALIZE_SEQ_RANGE - NORMALIZE_SEQ_TURNS * 2.0 * M_PI < 3.0, "the turns reach [-pi, pi)");
MPC_HD double normalize_angle(double a) {
  if (!(fabs(a) < 1.0e9)) return a;
  if (fabs(a) > MPC_NORMALIZE_SEQ_RANGE) a = fma(-rint(a * 1.59154943091895345554e-01), 2.0 * M_PI, a);
  MPC_STAGE_LOOP      /* (one copy of the turn: unrolled 32 times it costs mpc_run_pre_kernel a register, 169 instead of 168, and with it a wave of occupancy) */
  for (int turn = 0; turn < NORMALIZE_SEQ_TURNS; turn++) {
    if (a >= M_PI) a -= 2.0 * M_PI;
    else if (a < -M_PI) a += 2.0 * M_PI;
    else break;
  }
  return a;
}

/* RoadGeometry::orientation (RoadGeometry.cpp:41-47) */
MPC_HD double road_orientation(const double *c, double px, double dir) {
  double psi = atan(poly5_der(c, px));
  if (dir < 0.0) psi = normalize_angle(psi + M_PI);
  return psi;
}

struct RunPre {
  double state[6], coef[MPC_NCOEF], yaw_lo, yaw_hi, max_yaw_change, target_speed;
  int ncoef;
};

/* Where the functions below read the six model values (dt, Lf and the four limits; only Lf and the limits occur here): `m`, a
 * template argument like Solver::setup_vals' -- the handle's MpcParams itself for the entry points without per-instance values
 * (their kernels pass P twice and each field is read from P where it is used, so they are instruction for instruction what they
 * were; the signatures without `m` are the same call for host code) or an instance's mpc::ModelVals (the mpc_run_*_model / mpc_telemetry_*_model entry points; a column that
 * ModelVals::column refuses has become the handle's values there).  Everything else -- the tables, max_fit_*, latency_ms,
 * lookahead, steer_adj_*, the weights -- is the handle's on every path. */
/* (MV = MpcParams: the values are read through P itself -- a second reference to the same parameter block moved a scalar load in
 * mpc_run_pre_kernel) */
template <class MV>
MPC_HD const MV &run_model_of(const MpcParams &P, const MV &m) {
  if constexpr (std::is_same<MV, MpcParams>::value) return P;
  else return m;
}

/* The pre-solve half of MPC::run.  pose = {x, y, psi, v, steering, acceleration}; px/py hold the n global
 * waypoints on entry and the vehicle-frame waypoints on return (the reference transforms them in place). */
template <class MV>
MPC_HD void run_pre(const MpcParams &P, const MV &m_, const double *pose, double *px, double *py, int n, RunPre &R) {
  const MV &m = run_model_of(P, m_);
  double sn, cs;
  fsincos(pose[2], &sn, &cs);
  MPC_UNROLL
  for (int i = 0; i < RUN_MAX_PTS; i++) {
    if (i < n) {
      const double vx = px[i] - pose[0], vy = py[i] - pose[1];                   /* Vehicle.cpp:108-112 */
      px[i] = vx * cs + vy * sn;
      py[i] = vy * cs - vx * sn;
    }
  }
  /* RoadGeometry::fit: order 2, 3, 4 while the squared error exceeds maxFitError (RoadGeometry.cpp:26-34) */
  double c[MPC_NCOEF] = {0, 0, 0, 0, 0};
  int order = 2, ncoef = 3;
  bool pending = true;
  MPC_UNROLL
  for (int pass = 0; pass < 3; pass++) {
    if (pending) {
      const int used = order++;
      double cc[MPC_NCOEF] = {0, 0, 0, 0, 0};
      if (pass == 0) polyfit_qr<3>(px, py, n, cc);
      else if (pass == 1) polyfit_qr<4>(px, py, n, cc);
      else polyfit_qr<5>(px, py, n, cc);
      double err = 0.0;
      MPC_UNROLL
      for (int i = 0; i < RUN_MAX_PTS; i++)
        if (i < n) { const double d = py[i] - poly5(cc, px[i]); err += d * d; }
      MPC_UNROLL
      for (int j = 0; j < MPC_NCOEF; j++) c[j] = cc[j];
      ncoef = used + 1;
      pending = (err > P.max_fit_error) && (order < P.max_fit_order);
    }
  }
  MPC_UNROLL
  for (int j = 0; j < MPC_NCOEF; j++) R.coef[j] = c[j];
  R.ncoef = ncoef;
  const double cte = c[0];                                                        /* f(0), MPC.cpp:334 */
  const double epsi = -atan(c[1]);                                                /* MPC.cpp:336 */
  double back = px[0], front = px[0];
  MPC_UNROLL
  for (int i = 0; i < RUN_MAX_PTS; i++) if (i == n - 1) back = px[i];
  const double dir = back - 0.0;                                                  /* computeOrientationChange(0, back) */
  /* (a road whose first and last waypoint have the same x in the car's frame -- all of them at one x, all of them at the car -- has
   * no extent along the car's axis and no fit that means anything: not-a-number here, and through the psi box a status) */
  const double span = back - front;
  R.max_yaw_change = (road_orientation(c, back, dir) - road_orientation(c, 0.0, dir)) * (span != 0.0 ? span : NAN) / back;   /* :339 */
  const double max_speed = table_lookup(P.yaw_changes, P.n_yaw_changes, P.yaw_change_speeds, P.n_yaw_change_speeds,
                                        R.max_yaw_change, m.max_speed);           /* :340 */
  R.target_speed = table_lookup(P.steers, P.n_steers, P.steer_speeds, P.n_steer_speeds, pose[4], max_speed);   /* :342 */
  if (R.max_yaw_change < 0.0) { R.yaw_lo = R.max_yaw_change; R.yaw_hi = 0.1; }   /* :345-352 */
  else { R.yaw_lo = -0.1; R.yaw_hi = R.max_yaw_change; }
  /* (a steering angle that is no angle of a wheel -- not a number, beyond a quarter turn -- only picks a row of the speed table above
   * and would pass unnoticed: the instance is handed to the solve without a speed, which ends it with a status) */
  const double v0 = fabs(pose[4]) <= RUN_MAX_STEERING_ANGLE ? pose[3] : NAN;
  R.state[0] = 0.0; R.state[1] = 0.0; R.state[2] = 0.0; R.state[3] = v0; R.state[4] = cte; R.state[5] = epsi;   /* :355-356 */
}

MPC_HD void run_pre(const MpcParams &P, const double *pose, double *px, double *py, int n, RunPre &R) { run_pre(P, P, pose, px, py, n, R); }

/* The post-solve half (MPC.cpp:360-381): result9 -> {x1,y1,psi1,v1,steer in [-1,1],accel,cte1,epsi1} */
template <class MV>
MPC_HD void run_post(const MpcParams &P, const MV &m_, double max_yaw_change, double target_speed, double v0, const double *r9, double *o8) {
  const MV &m = run_model_of(P, m_);
  double steer = r9[6];
  if (fabs(max_yaw_change) > P.steer_adj_thresh) steer += P.steer_adj_ratio * max_yaw_change;
  const double accel = fmin(r9[7], target_speed - v0);
  double sv = steer / m.max_steering;
  sv = sv < -1.0 ? -1.0 : (sv > 1.0 ? 1.0 : sv);
  o8[0] = r9[0]; o8[1] = r9[1]; o8[2] = r9[2]; o8[3] = r9[3]; o8[4] = sv; o8[5] = accel; o8[6] = r9[4]; o8[7] = r9[5];
}
MPC_HD void run_post(const MpcParams &P, double max_yaw_change, double target_speed, double v0, const double *r9, double *o8) {
  run_post(P, P, max_yaw_change, target_speed, v0, r9, o8);
}

/* ---- N2: the telemetry handler around run(), src/mpc_main.cpp:126-159 and :171-174 ------------------ */
/* tel = {x, y, psi (rad, any range: normalize_angle above says what becomes of it), speed (mph), steering_angle (simulator sign), previous throttle command};
 * extra = the handler's mean solve time added to Config::lookahead (mpc_main.cpp:158).
 * -> pose {x,y,psi,v,steering,acceleration} after latency compensation (Vehicle::update + Vehicle::move) */
/* How long the handler compensates for: `lc`, a template argument like `m` --
 *   a double          the handle's rule (every entry point without per-instance latency: they are instruction for instruction what they
 *                     were): Vehicle::move if P.latency_ms != 0, over P.lookahead + lc seconds (lc = the call's extra_latency);
 *   RunComp{own, s}   own: this instance's own `s` seconds (the mpc_telemetry_*_latency / mpc_drive_*_latency entry points): Vehicle::move if
 *                     s > 0, over s seconds -- s == 0 is the reference's `if (Config::latency)` not taken.  A value that cannot be used
 *                     (not finite, below 0) moves nothing and takes the speed away, like a speedometer reading below zero: the instance
 *                     ends with a status.  !own: the handle's rule with extra = s, decided at run time (the one-launch drive, whose
 *                     array may be NULL). */
struct RunComp {
  bool own;
  double s;
};
MPC_HD bool run_comp_usable(double s) { return s >= 0.0 && s < HUGE_VAL; }
/* the three questions telemetry_to_pose asks: can the value be used, is there a move, over how many seconds */
template <class LC>
MPC_HD bool run_comp_ok(const LC &lc) {
  if constexpr (std::is_same<LC, RunComp>::value) return !lc.own || run_comp_usable(lc.s);
  else return true;
}
template <class LC>
MPC_HD bool run_comp_on(const MpcParams &P, const LC &lc) {
  if constexpr (std::is_same<LC, RunComp>::value) return lc.own ? (run_comp_usable(lc.s) && lc.s > 0.0) : P.latency_ms != 0;
  else return P.latency_ms != 0;
}
template <class LC>
MPC_HD double run_comp_seconds(const MpcParams &P, const LC &lc) {
  if constexpr (std::is_same<LC, RunComp>::value) return lc.own ? lc.s : P.lookahead + lc.s;
  else return P.lookahead + lc;
}
template <class MV, class LC>
MPC_HD void telemetry_to_pose(const MpcParams &P, const MV &m_, const double *tel, const LC &lc, double *pose) {
  const MV &m = run_model_of(P, m_);
  const double psi = normalize_angle(tel[2]);            /* normalizeAngle, mpc_main.cpp:127 */
  /* (a speedometer reading below zero is none: the instance ends with a status -- and so does one whose compensation is no time span) */
  const double mph = (tel[3] >= 0.0 && run_comp_ok(lc)) ? tel[3] : NAN;
  const double v = mph * 1609.34 / 3600.0;               /* MpH2MpS, :129 */
  const double steer = -tel[4];                          /* :131 */
  const double acc = (tel[5] - v / 50.0) * 6.0;          /* :156 */
  pose[0] = tel[0]; pose[1] = tel[1]; pose[2] = psi; pose[3] = v; pose[4] = steer; pose[5] = acc;
  if (run_comp_on(P, lc)) {                              /* :157-159, Vehicle::move (Vehicle.cpp:145-168) */
    const double dtm = run_comp_seconds(P, lc);
    const double dist = v * dtm;
    double sn, cs;
    fsincos(psi, &sn, &cs);
    pose[0] = tel[0] + dist * cs;
    pose[1] = tel[1] + dist * sn;
    pose[2] = psi + steer * dist / m.Lf;                 /* Vehicle::length = Config::Lf, mpc_main.cpp:155 */
    pose[3] = v + acc * dtm;                             /* not clamped: Vehicle.cpp:156 is overwritten at :167 */
  }
}
MPC_HD void telemetry_to_pose(const MpcParams &P, const double *tel, double extra, double *pose) { telemetry_to_pose(P, P, tel, extra, pose); }
/* Vehicle::computeThrottle (Vehicle.cpp:81-103) */
template <class MV>
MPC_HD double compute_throttle(const MV &m, double accel, double target) {
  const double keep = target / m.max_speed;
  if (accel >= 0.0) return accel < 0.001 ? keep : fmin(1.0, keep + (1.0 - keep) * accel / m.max_acceleration);
  if (accel <= -15.0) return -1.0;
  const double base = accel < -10.0 ? 0.95 : (accel < -5.0 ? 0.9 : 0.85);
  return -base - (1.0 - base) * accel / m.max_deceleration;
}
/* mpc_main.cpp:171-174: run()'s result -> the command sent back to the simulator */
template <class MV>
MPC_HD void command_from_run(const MV &m, const double *o8, double *steer_cmd, double *throttle_cmd) {
  *steer_cmd = -o8[4];
  *throttle_cmd = compute_throttle(m, o8[5], o8[3]);
}


/* ---- one instance of a batch, as the run() kernels and the test-only CPU build (tests/host_twin) run it ----------------------
 * MV as above: the handle's MpcParams (pass P twice) or the instance's ModelVals (model_vals_of). */
/* instance i's column of model [MPC_NMODEL][ld]; a column that cannot be used: the handle's values (the solve reports it INFEASIBLE) */
MPC_HD ModelVals model_vals_of(const MpcParams &P, const double *model, int64_t ld, int64_t i) {
  bool ok;
  return ModelColumn{model + i, ld}.vals(P, ok);
}

/* pose [6][ld] (TELEMETRY: the simulator's telemetry rows, latency compensation first, mpc_main.cpp:126-159) and the waypoints
 * ptsx / ptsy [npts][ld], which become the vehicle-frame ones in place -> pre [RUN_PRE_ROWS][ldp].  Returns the fit's coefficient count.
 * extra: the call's extra_latency, or the instance's own RunComp. */
template <bool TELEMETRY, class MV, class LC>
MPC_HD int run_pre_instance(const MpcParams &P, const MV &m, int64_t i, int64_t ld, int npts, const double *pose, const LC &extra,
                            double *ptsx, double *ptsy, double *pre, int64_t ldp) {
  double po[6], px[RUN_MAX_PTS], py[RUN_MAX_PTS];
  MPC_UNROLL
  for (int q = 0; q < 6; q++) po[q] = pose[q * ld + i];
  if (TELEMETRY) {
    double t6[6];
    MPC_UNROLL
    for (int q = 0; q < 6; q++) t6[q] = po[q];
    telemetry_to_pose(P, m, t6, extra, po);
  }
  MPC_UNROLL
  for (int q = 0; q < RUN_MAX_PTS; q++) {
    /* (no load under a condition: the rows past npts read the last row that exists and count as 0.0 -- with conditional loads
     * mpc_run_pre_kernel needs 188 VGPRs instead of 168 and loses a wave of occupancy) */
    const int row = q < npts ? q : npts - 1;
    const double x = ptsx[row * ld + i], y = ptsy[row * ld + i];
    px[q] = q < npts ? x : 0.0; py[q] = q < npts ? y : 0.0;
  }
  RunPre R;
  run_pre(P, m, po, px, py, npts, R);
  MPC_UNROLL
  for (int q = 0; q < RUN_MAX_PTS; q++) if (q < npts) { ptsx[q * ld + i] = px[q]; ptsy[q * ld + i] = py[q]; }
  MPC_UNROLL
  for (int q = 0; q < 6; q++) pre[(RUN_PRE_STATE + q) * ldp + i] = R.state[q];
  MPC_UNROLL
  for (int q = 0; q < MPC_NCOEF; q++) pre[(RUN_PRE_COEFFS + q) * ldp + i] = R.coef[q];
  pre[RUN_PRE_YAW_LO * ldp + i] = R.yaw_lo; pre[RUN_PRE_YAW_HI * ldp + i] = R.yaw_hi;
  pre[RUN_PRE_MAX_YAW_CHANGE * ldp + i] = R.max_yaw_change; pre[RUN_PRE_TARGET_SPEED * ldp + i] = R.target_speed;
  return R.ncoef;
}

/* pre and solve()'s vector out9 [9][ld9] -> out8 [8][ld] and / or cmd [2][ld], the reply of the telemetry handler (either may be nullptr) */
template <class MV>
MPC_HD void run_post_instance(const MpcParams &P, const MV &m, int64_t i, const double *pre, int64_t ldp, const double *out9, int64_t ld9,
                              double *out8, double *cmd, int64_t ld) {
  double r9[9], o8[8];
  MPC_UNROLL
  for (int q = 0; q < 9; q++) r9[q] = out9[q * ld9 + i];
  run_post(P, m, pre[RUN_PRE_MAX_YAW_CHANGE * ldp + i], pre[RUN_PRE_TARGET_SPEED * ldp + i], pre[(RUN_PRE_STATE + 3) * ldp + i], r9, o8);
  if (out8) {
    MPC_UNROLL
    for (int q = 0; q < 8; q++) out8[q * ld + i] = o8[q];
  }
  if (cmd) {
    double sc, tc;
    command_from_run(run_model_of(P, m), o8, &sc, &tc);
    cmd[i] = sc; cmd[ld + i] = tc;
  }
}

}  // namespace mpc
#endif
