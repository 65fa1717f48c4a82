/*
 * drive_model_sanitize.cpp -- TEST-ONLY: the CPU build of the track-driving loop with per-car model values
 * (tests/drive_twin/drive_twin.cpp, compiled into this program) on garbage columns and garbage cars, under
 * AddressSanitizer + UndefinedBehaviorSanitizer.  argv[1]: a config file.  Every array has exactly the size the call states, so a read
 * or write outside a car's column, or past column B, is an error of the run.
 * A circular track of 40 waypoints (radius 50 m); N = 10, B = 8, ld = 9, 3 messages, cold and warm.  The columns from B on hold
 * not-a-number (inputs) or a sentinel (outputs).  Car: 0 a plain car with the handle's own values as its column; 1 x = NaN; 2 every
 * row 1e300; 3 speed -1 mph; 4 a plain car whose column is all not-a-number; 5 dt = 0; 6 Lf = -1; 7 car 0 again.
 * Exit 0: cars 4 - 6 end MPC_STATUS_INFEASIBLE at every step with finite rows, cars 1 - 3 carry a status, car 7 equals car 0 bit for
 * bit, nothing behind column B was written, and the plant and the handler behave the same way on their own.
 */
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mpc_amd.h"

extern "C" int mpc_drive_twin_plant(const MpcParams *p, int64_t B, int64_t ld, double *car, const double *cmd, const double *model,
                                    const double *latency, const double *plant, const MpcDriveOpts *opts, int32_t *ok);
extern "C" int mpc_drive_twin_handler(const MpcParams *p, int64_t B, int64_t ld, const double *car, const double *comp, const int32_t *k,
                                      const double *tx, const double *ty, int n_track, const double *weights, const double *model,
                                      const int32_t *horizon, const MpcDriveOpts *opts, const double *warm_in, const int32_t *warm_status,
                                      double *warm_out, int64_t ld_warm, const MpcWarmOpts *warm_opts, double *cmd, int32_t *status, int32_t *iters,
                                      double *cte_epsi);
extern "C" int mpc_drive_twin(const MpcParams *p, int64_t B, int64_t ld, int steps, double *car, const double *tx, const double *ty, int n_track,
                              const double *weights, const double *model, const int32_t *horizon, const double *latency, const double *plant,
                              const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary, double *hist, int32_t *status, int32_t *iters,
                              int32_t *handler_status);

/* mpc_drive_opts_default and mpc_warm_opts_default live in the product library; their values, restated for a program without it */
static MpcDriveOpts drive_opts(const MpcParams &p, int warm) {
  MpcDriveOpts o;
  memset(&o, 0, sizeof(o));
  o.size = (int32_t)sizeof(o); o.npts = 6; o.h = 0.01; o.sub_old = (p.latency_ms + 5) / 10; o.sub_new = p.latency_ms != 0 ? 2 : 10;
  o.warm_start = warm; o.extra_latency = 0.0; o.cte_limit = 3.0;
  return o;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  MpcParams p;
  if (mpc_params_load_json(argv[1], &p) != MPC_OK) return 3;
  p.N = 10;
  const int B = 8, ld = 9, steps = 3, n_track = 40;
  const double sentinel = -7777.25;
  const int32_t isentinel = -12345;
  std::vector<double> tx(n_track), ty(n_track);
  for (int q = 0; q < n_track; q++) { tx[q] = 50.0 * cos(2.0 * M_PI * q / n_track); ty[q] = 50.0 * sin(2.0 * M_PI * q / n_track); }
  const double plain[6] = {50.2, 1.0, 0.5 * M_PI + 0.02, 30.0, 0.01, 0.3};
  const double own[MPC_NMODEL] = {p.dt, p.Lf, p.max_steering, p.max_acceleration, p.max_deceleration, p.max_speed};
  std::vector<double> car0((size_t)6 * ld, NAN), model((size_t)MPC_NMODEL * ld, NAN);
  for (int i = 0; i < B; i++) {
    for (int q = 0; q < 6; q++) car0[(size_t)q * ld + i] = plain[q];
    for (int q = 0; q < MPC_NMODEL; q++) model[(size_t)q * ld + i] = own[q];
  }
  car0[(size_t)0 * ld + 1] = NAN;
  for (int q = 0; q < 6; q++) car0[(size_t)q * ld + 2] = 1e300;
  car0[(size_t)3 * ld + 3] = -1.0;
  for (int q = 0; q < MPC_NMODEL; q++) model[(size_t)q * ld + 4] = NAN;
  model[(size_t)MPC_MODEL_DT * ld + 5] = 0.0;
  model[(size_t)MPC_MODEL_LF * ld + 6] = -1.0;
  MpcWarmOpts wo;
  memset(&wo, 0, sizeof(wo));
  wo.size = (int32_t)sizeof(wo); wo.shift = 0; wo.mu_init = 1e-6; wo.bound_push = 1e-6; wo.duals = 0;
  int bad = 0;
  for (int warm = 0; warm < 2; warm++) {
    const MpcDriveOpts o = drive_opts(p, warm);
    std::vector<double> car = car0, summary((size_t)MPC_DRIVE_NSUM * ld, sentinel), hist((size_t)steps * MPC_DRIVE_REC * ld, sentinel);
    std::vector<int32_t> status((size_t)ld, isentinel), iters((size_t)ld, isentinel);
    const int rc = mpc_drive_twin(&p, B, ld, steps, car.data(), tx.data(), ty.data(), n_track, nullptr, model.data(), nullptr, nullptr, nullptr, &o, &wo,
                                  summary.data(), hist.data(), status.data(), iters.data(), nullptr);
    if (rc != MPC_OK) { printf("warm %d: rc %d\n", warm, rc); return 4; }
    printf("warm %d status", warm);
    for (int i = 0; i < B; i++) printf(" %d", status[i]);
    printf("\n");
    for (int i = 1; i <= 3; i++) if (status[i] == MPC_STATUS_SUCCESS) bad++;
    for (int i = 4; i <= 6; i++) {
      if (status[i] != MPC_STATUS_INFEASIBLE || summary[(size_t)MPC_DRIVE_SUM_FAILED * ld + i] != (double)steps) bad++;
      for (int q = 0; q < 6; q++) if (!std::isfinite(car[(size_t)q * ld + i])) bad++;
      for (int q = 0; q < MPC_DRIVE_NSUM; q++) if (!std::isfinite(summary[(size_t)q * ld + i])) bad++;
      for (int r = 0; r < steps * MPC_DRIVE_REC; r++) if (!std::isfinite(hist[(size_t)r * ld + i])) bad++;
      for (int t = 0; t < steps; t++) if (hist[(size_t)(t * MPC_DRIVE_REC + MPC_DRIVE_REC_STATUS) * ld + i] != (double)MPC_STATUS_INFEASIBLE) bad++;
    }
    /* the neighbour of the garbage, and what lies behind column B */
    for (int q = 0; q < 6; q++) if (memcmp(&car[(size_t)q * ld + 7], &car[(size_t)q * ld], sizeof(double)) != 0) bad++;
    for (int q = 0; q < MPC_DRIVE_NSUM; q++) if (memcmp(&summary[(size_t)q * ld + 7], &summary[(size_t)q * ld], sizeof(double)) != 0) bad++;
    for (int r = 0; r < steps * MPC_DRIVE_REC; r++) if (memcmp(&hist[(size_t)r * ld + 7], &hist[(size_t)r * ld], sizeof(double)) != 0) bad++;
    if (status[7] != status[0] || iters[7] != iters[0]) bad++;
    for (int q = 0; q < 6; q++) if (!std::isnan(car[(size_t)q * ld + B])) bad++;
    for (int q = 0; q < MPC_DRIVE_NSUM; q++) if (summary[(size_t)q * ld + B] != sentinel) bad++;
    for (int r = 0; r < steps * MPC_DRIVE_REC; r++) if (hist[(size_t)r * ld + B] != sentinel) bad++;
    if (status[B] != isentinel || iters[B] != isentinel) bad++;
  }
  /* the plant alone: a reply that is not finite, a garbage car, garbage columns -- the cars with an unusable column move under the handle's values */
  {
    std::vector<double> car = car0, cmd((size_t)2 * ld, NAN);
    for (int i = 0; i < B; i++) { cmd[i] = 0.1; cmd[(size_t)ld + i] = 0.5; }
    cmd[1] = NAN; cmd[(size_t)ld + 2] = INFINITY;
    MpcDriveOpts po = drive_opts(p, 0);
    po.sub_old = 10; po.sub_new = 2; po.h = 0.01;
    if (mpc_drive_twin_plant(&p, B, ld, car.data(), cmd.data(), model.data(), nullptr, nullptr, &po, nullptr) != MPC_OK) bad++;
    for (int i = 4; i <= 7; i++)
      for (int q = 0; q < 6; q++) if (memcmp(&car[(size_t)q * ld + i], &car[(size_t)q * ld], sizeof(double)) != 0) bad++;
    for (int q = 0; q < 6; q++) if (!std::isnan(car[(size_t)q * ld + B])) bad++;
    if (mpc_drive_twin_plant(&p, B, B - 1, car.data(), cmd.data(), model.data(), nullptr, nullptr, &po, nullptr) != MPC_ERR_INVALID) bad++;
    if (mpc_drive_twin_plant(&p, B, ld, car.data(), nullptr, model.data(), nullptr, nullptr, &po, nullptr) != MPC_ERR_INVALID) bad++;   /* (no reply) */
  }
  /* one handler call: every window index the track has is taken, one outside it is refused */
  {
    const MpcDriveOpts o = drive_opts(p, 0);
    std::vector<int32_t> k((size_t)ld, 0), status((size_t)ld, isentinel), iters((size_t)ld, isentinel);
    std::vector<double> cmd((size_t)2 * ld, sentinel), ce((size_t)2 * ld, sentinel);
    for (int i = 0; i < B; i++) k[i] = i == 3 ? n_track - 1 : 0;
    if (mpc_drive_twin_handler(&p, B, ld, car0.data(), nullptr, k.data(), tx.data(), ty.data(), n_track, nullptr, model.data(), nullptr, &o, nullptr, nullptr,
                               nullptr, 0, &wo, cmd.data(), status.data(), iters.data(), ce.data()) != MPC_OK) bad++;
    for (int i = 4; i <= 6; i++) if (status[i] != MPC_STATUS_INFEASIBLE || !std::isfinite(cmd[i]) || !std::isfinite(cmd[(size_t)ld + i])) bad++;
    if (memcmp(&cmd[7], &cmd[0], sizeof(double)) != 0 || memcmp(&cmd[(size_t)ld + 7], &cmd[ld], sizeof(double)) != 0 || status[7] != status[0]) bad++;
    if (cmd[B] != sentinel || cmd[(size_t)ld + B] != sentinel || status[B] != isentinel || ce[B] != sentinel) bad++;
    k[2] = n_track;
    if (mpc_drive_twin_handler(&p, B, ld, car0.data(), nullptr, k.data(), tx.data(), ty.data(), n_track, nullptr, model.data(), nullptr, &o, nullptr, nullptr,
                               nullptr, 0, &wo, cmd.data(), status.data(), iters.data(), ce.data()) != MPC_ERR_INVALID) bad++;
  }
  printf("bad %d\n", bad);
  return bad == 0 ? 0 : 1;
}
