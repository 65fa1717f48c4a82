/*
 * drive_plant_sanitize.cpp -- TEST-ONLY: the CPU build of the track-driving loop with per-car plant values
 * (tests/drive_twin/drive_twin.cpp, compiled into this program) on garbage columns and garbage cars, under
 * AddressSanitizer + UndefinedBehaviorSanitizer.  argv[1]: a config file.  Every array has exactly the size the call states, so a read
 * or write outside a car's column, or past column B, is an error of the run.
 * A circular track of 40 waypoints (radius 50 m); N = 10, B = 12, ld = 13, 3 messages, cold and warm.  The columns from B on hold
 * not-a-number (inputs) or a sentinel (outputs).  Every model column holds the handle's own values, every latency column (0.1 s, 10, 2).
 * Car: 0 a plain car with the plant column (Lf 3.1, g 1.1, b 0.01, a 5, d 60, w 0.5); 1 x = NaN; 2 a plant column that is all
 * not-a-number; 3 Lf_p = 0; 4 Lf_p = -1; 5 d = 0; 6 g = infinity; 7 b = NaN; 8 a = -infinity; 9 w = NaN; 10 every row of the car
 * 1e300; 11 car 0 again.
 * Exit 0: cars 2 - 9 are MPC_STATUS_INFEASIBLE at every step with finite rows and equal, but for the status rows, the car moved with the
 * default column; cars 1 and 10 carry a status; car 11 equals car 0 bit for bit; nothing behind column B was written; and the plant
 * behaves the same way on its own.
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

/* mpc_drive_opts_default, mpc_warm_opts_default and mpc_drive_plant_default live in the product library; their values, restated for a
 * program without it */
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
  const int B = 12, ld = 13, steps = 3, n_track = 40;
  const double sentinel = -7777.25;
  const int32_t isentinel = -12345;
  std::vector<double> tx(n_track), ty(n_track);
  for (int q = 0; q < n_track; q++) { tx[q] = 50.0 * cos(2.0 * M_PI * q / n_track); ty[q] = 50.0 * sin(2.0 * M_PI * q / n_track); }
  const double plain[6] = {50.2, 1.0, 0.5 * M_PI + 0.02, 30.0, 0.01, 0.3};
  const double own[MPC_NMODEL] = {p.dt, p.Lf, p.max_steering, p.max_acceleration, p.max_deceleration, p.max_speed};
  const double lcol[MPC_NLATENCY] = {0.1, 10.0, 2.0};
  const double pcol[MPC_NPLANT] = {3.1, 1.1, 0.01, 5.0, 60.0, 0.5};
  const double dcol[MPC_NPLANT] = {p.Lf, 1.0, 0.0, 6.0, 50.0, 0.0};
  std::vector<double> car0((size_t)6 * ld, NAN), model((size_t)MPC_NMODEL * ld, NAN), lat((size_t)MPC_NLATENCY * ld, NAN),
      plant((size_t)MPC_NPLANT * ld, NAN), dplant((size_t)MPC_NPLANT * ld, NAN);
  for (int i = 0; i < B; i++) {
    for (int q = 0; q < 6; q++) car0[(size_t)q * ld + i] = plain[q];
    for (int q = 0; q < MPC_NMODEL; q++) model[(size_t)q * ld + i] = own[q];
    for (int q = 0; q < MPC_NLATENCY; q++) lat[(size_t)q * ld + i] = lcol[q];
    for (int q = 0; q < MPC_NPLANT; q++) { plant[(size_t)q * ld + i] = (i >= 2 && i <= 9) ? dcol[q] : pcol[q]; dplant[(size_t)q * ld + i] = dcol[q]; }
  }
  car0[(size_t)0 * ld + 1] = NAN;
  for (int q = 0; q < MPC_NPLANT; q++) plant[(size_t)q * ld + 2] = NAN;
  plant[(size_t)MPC_PLANT_LF * ld + 3] = 0.0;
  plant[(size_t)MPC_PLANT_LF * ld + 4] = -1.0;
  plant[(size_t)MPC_PLANT_DRAG_SPEED * ld + 5] = 0.0;
  plant[(size_t)MPC_PLANT_STEER_GAIN * ld + 6] = INFINITY;
  plant[(size_t)MPC_PLANT_STEER_BIAS * ld + 7] = NAN;
  plant[(size_t)MPC_PLANT_ACCEL_GAIN * ld + 8] = -INFINITY;
  plant[(size_t)MPC_PLANT_DRIFT * ld + 9] = NAN;
  for (int q = 0; q < 6; q++) car0[(size_t)q * ld + 10] = 1e300;
  MpcWarmOpts wo;
  memset(&wo, 0, sizeof(wo));
  wo.size = (int32_t)sizeof(wo); wo.shift = 0; wo.mu_init = 1e-6; wo.bound_push = 1e-6; wo.duals = 0;
  int bad = 0;
  for (int warm = 0; warm < 2; warm++) {
    const MpcDriveOpts o = drive_opts(p, warm);
    std::vector<double> car = car0, summary((size_t)MPC_DRIVE_NSUM * ld, sentinel), hist((size_t)steps * MPC_DRIVE_REC * ld, sentinel);
    std::vector<int32_t> status((size_t)ld, isentinel), iters((size_t)ld, isentinel), hs((size_t)steps * ld, isentinel);
    const int rc = mpc_drive_twin(&p, B, ld, steps, car.data(), tx.data(), ty.data(), n_track, nullptr, model.data(), nullptr, lat.data(), plant.data(), &o,
                                  &wo, summary.data(), hist.data(), status.data(), iters.data(), hs.data());
    if (rc != MPC_OK) { printf("warm %d: rc %d\n", warm, rc); return 4; }
    /* the same cars under the default column everywhere: what cars 2 - 9 must equal but for their status rows */
    std::vector<double> dcar = car0, dsummary((size_t)MPC_DRIVE_NSUM * ld, sentinel), dhist((size_t)steps * MPC_DRIVE_REC * ld, sentinel);
    std::vector<int32_t> dstatus((size_t)ld, isentinel), diters((size_t)ld, isentinel);
    if (mpc_drive_twin(&p, B, ld, steps, dcar.data(), tx.data(), ty.data(), n_track, nullptr, model.data(), nullptr, lat.data(), dplant.data(), &o, &wo,
                       dsummary.data(), dhist.data(), dstatus.data(), diters.data(), nullptr) != MPC_OK) return 5;
    printf("warm %d status", warm);
    for (int i = 0; i < B; i++) printf(" %d", status[i]);
    printf("\n");
    if (status[1] == MPC_STATUS_SUCCESS || status[10] == MPC_STATUS_SUCCESS) bad++;
    for (int i = 2; i <= 9; i++) {
      if (status[i] != MPC_STATUS_INFEASIBLE || summary[(size_t)MPC_DRIVE_SUM_FAILED * ld + i] != (double)steps || dstatus[i] != MPC_STATUS_SUCCESS) bad++;
      if (iters[i] != diters[i]) bad++;
      for (int q = 0; q < 6; q++) if (!std::isfinite(car[(size_t)q * ld + i]) || memcmp(&car[(size_t)q * ld + i], &dcar[(size_t)q * ld + i], sizeof(double)) != 0) bad++;
      for (int q = 0; q < MPC_DRIVE_NSUM; q++) {
        if (!std::isfinite(summary[(size_t)q * ld + i])) bad++;
        if (q != MPC_DRIVE_SUM_FAILED && memcmp(&summary[(size_t)q * ld + i], &dsummary[(size_t)q * ld + i], sizeof(double)) != 0) bad++;
      }
      for (int t = 0; t < steps; t++) {
        for (int q = 0; q < MPC_DRIVE_REC; q++) {
          const size_t at = (size_t)(t * MPC_DRIVE_REC + q) * ld + i;
          if (!std::isfinite(hist[at])) bad++;
          if (q != MPC_DRIVE_REC_STATUS && memcmp(&hist[at], &dhist[at], sizeof(double)) != 0) bad++;
        }
        if (hist[(size_t)(t * MPC_DRIVE_REC + MPC_DRIVE_REC_STATUS) * ld + i] != (double)MPC_STATUS_INFEASIBLE) bad++;
        if (hs[(size_t)t * ld + i] != MPC_STATUS_SUCCESS) bad++;       /* the handler's own status is untouched */
      }
    }
    /* the neighbour of the garbage, and what lies behind column B */
    const int twin = B - 1;
    for (int q = 0; q < 6; q++) if (memcmp(&car[(size_t)q * ld + twin], &car[(size_t)q * ld], sizeof(double)) != 0) bad++;
    for (int q = 0; q < MPC_DRIVE_NSUM; q++) if (memcmp(&summary[(size_t)q * ld + twin], &summary[(size_t)q * ld], sizeof(double)) != 0) bad++;
    for (int r = 0; r < steps * MPC_DRIVE_REC; r++) if (memcmp(&hist[(size_t)r * ld + twin], &hist[(size_t)r * ld], sizeof(double)) != 0) bad++;
    if (status[twin] != status[0] || iters[twin] != iters[0] || status[0] != MPC_STATUS_SUCCESS) bad++;
    if (memcmp(&car[0], &dcar[0], sizeof(double)) == 0) bad++;          /* car 0's column reaches the plant */
    for (int q = 0; q < 6; q++) if (!std::isnan(car[(size_t)q * ld + B])) bad++;
    for (int q = 0; q < MPC_DRIVE_NSUM; q++) if (summary[(size_t)q * ld + B] != sentinel) bad++;
    for (int r = 0; r < steps * MPC_DRIVE_REC; r++) if (hist[(size_t)r * ld + B] != sentinel) bad++;
    if (status[B] != isentinel || iters[B] != isentinel) bad++;
    for (int t = 0; t < steps; t++) if (hs[(size_t)t * ld + B] != isentinel) bad++;
  }
  /* the plant alone: a reply that is not finite, a garbage car, the unusable columns -- those cars move as under the default column */
  {
    std::vector<double> car = car0, dcar = car0, cmd((size_t)2 * ld, NAN);
    std::vector<int32_t> ok((size_t)ld, isentinel);
    for (int i = 0; i < B; i++) { cmd[i] = 0.1; cmd[(size_t)ld + i] = 0.5; }
    cmd[1] = NAN; cmd[(size_t)ld + 10] = INFINITY;
    MpcDriveOpts po = drive_opts(p, 0);
    po.sub_old = 10; po.sub_new = 2; po.h = 0.01;
    if (mpc_drive_twin_plant(&p, B, ld, car.data(), cmd.data(), model.data(), nullptr, plant.data(), &po, ok.data()) != MPC_OK) bad++;
    if (mpc_drive_twin_plant(&p, B, ld, dcar.data(), cmd.data(), model.data(), nullptr, dplant.data(), &po, nullptr) != MPC_OK) bad++;
    for (int i = 0; i < B; i++) if (ok[i] != ((i >= 2 && i <= 9) ? 0 : 1)) bad++;
    for (int i = 2; i <= 9; i++)
      for (int q = 0; q < 6; q++) if (memcmp(&car[(size_t)q * ld + i], &dcar[(size_t)q * ld + i], sizeof(double)) != 0 || !std::isfinite(car[(size_t)q * ld + i])) bad++;
    for (int q = 0; q < 6; q++) if (memcmp(&car[(size_t)q * ld + 11], &car[(size_t)q * ld], sizeof(double)) != 0) bad++;
    for (int q = 0; q < 6; q++) if (!std::isnan(car[(size_t)q * ld + B])) bad++;
    if (ok[B] != isentinel) bad++;
    if (mpc_drive_twin_plant(&p, B, B - 1, car.data(), cmd.data(), model.data(), nullptr, plant.data(), &po, nullptr) != MPC_ERR_INVALID) bad++;
    if (mpc_drive_twin_plant(&p, B, ld, car.data(), nullptr, model.data(), nullptr, plant.data(), &po, nullptr) != MPC_ERR_INVALID) bad++;   /* (no reply) */
  }
  printf("bad %d\n", bad);
  return bad == 0 ? 0 : 1;
}
