/*
 * drive_horizon_sanitize.cpp -- TEST-ONLY: the CPU build of the track-driving loop with a per-car horizon
 * (tests/drive_twin/drive_twin.cpp, compiled into this program) under AddressSanitizer + UndefinedBehaviorSanitizer.
 * argv[1]: a config file; argv[2]: a text file of numbers -- n_track, B, track_x [n_track], track_y [n_track], car [6][B] -- that
 * tests/test_drive_horizon.py writes: the 16 cars of its mixed batch on the lake track.
 * N = 10, ld = B + 1, 8 messages, cold and warm, horizon (3, 4, 5, 7, 10)[i % 5]: the mixed batch; then the same batch with the
 * unusable horizons 2, 0, -1 and N + 1 in cars 2, 7, 11 and 14.  Every array has exactly the size the call states and the warm buffer
 * inside the twin the rows of the handle's N, so a car that reads or writes records past its own stages' rows, or a trip count taken
 * from an unchecked horizon, is an error of the run.  The columns from B on hold not-a-number, a horizon of -999 or a sentinel.
 * Exit 0: every car of the mixed batch ends SUCCESS; the four cars end MPC_STATUS_INFEASIBLE at every step with finite rows; every
 * other car is bit for bit what it is in the mixed batch; nothing behind column B was written; model == NULL is bitwise a model array
 * of the handle's own values.
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

struct Result {
  std::vector<double> car, summary, hist;
  std::vector<int32_t> status, iters;
};

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  MpcParams p;
  if (mpc_params_load_json(argv[1], &p) != MPC_OK) return 3;
  p.N = 10;
  FILE *f = fopen(argv[2], "r");
  if (!f) return 3;
  int n_track = 0, B = 0;
  if (fscanf(f, "%d %d", &n_track, &B) != 2 || n_track < 6 || n_track > MPC_DRIVE_MAX_TRACK || B < 16 || B > 64) return 3;
  const int ld = B + 1, steps = 8;
  std::vector<double> tx(n_track), ty(n_track), car0((size_t)6 * ld, NAN);
  for (int q = 0; q < n_track; q++) if (fscanf(f, "%lf", &tx[q]) != 1) return 3;
  for (int q = 0; q < n_track; q++) if (fscanf(f, "%lf", &ty[q]) != 1) return 3;
  for (int q = 0; q < 6; q++)
    for (int i = 0; i < B; i++) if (fscanf(f, "%lf", &car0[(size_t)q * ld + i]) != 1) return 3;
  fclose(f);
  const double sentinel = -7777.25;
  const int32_t isentinel = -12345;
  const int loop_n[5] = {3, 4, 5, 7, 10}, bad_cars[4] = {2, 7, 11, 14}, bad_n[4] = {2, 0, -1, p.N + 1};
  const double own[MPC_NMODEL] = {p.dt, p.Lf, p.max_steering, p.max_acceleration, p.max_deceleration, p.max_speed};
  std::vector<int32_t> hz((size_t)ld, -999), hz_bad;
  for (int i = 0; i < B; i++) hz[i] = loop_n[i % 5];
  hz_bad = hz;
  for (int j = 0; j < 4; j++) hz_bad[bad_cars[j]] = bad_n[j];
  std::vector<double> model((size_t)MPC_NMODEL * ld, NAN), lat((size_t)MPC_NLATENCY * ld, NAN);
  MpcWarmOpts wo;
  memset(&wo, 0, sizeof(wo));
  wo.size = (int32_t)sizeof(wo); wo.shift = 0; wo.mu_init = 1e-6; wo.bound_push = 1e-6; wo.duals = 0;
  int bad = 0;
  for (int warm = 0; warm < 2; warm++) {
    const MpcDriveOpts o = drive_opts(p, warm);
    for (int i = 0; i < B; i++) {
      for (int q = 0; q < MPC_NMODEL; q++) model[(size_t)q * ld + i] = own[q];
      lat[(size_t)MPC_LATENCY_COMP * ld + i] = p.latency_ms != 0 ? p.lookahead : 0.0;
      lat[(size_t)MPC_LATENCY_SUB_OLD * ld + i] = o.sub_old; lat[(size_t)MPC_LATENCY_SUB_NEW * ld + i] = o.sub_new;
    }
    const auto run = [&](const std::vector<int32_t> &n, const double *md, Result &r) {
      r.car = car0;
      r.summary.assign((size_t)MPC_DRIVE_NSUM * ld, sentinel); r.hist.assign((size_t)steps * MPC_DRIVE_REC * ld, sentinel);
      r.status.assign((size_t)ld, isentinel); r.iters.assign((size_t)ld, isentinel);
      return mpc_drive_twin(&p, B, ld, steps, r.car.data(), tx.data(), ty.data(), n_track, nullptr, md, n.data(), lat.data(), nullptr, &o, &wo,
                            r.summary.data(), r.hist.data(), r.status.data(), r.iters.data(), nullptr);
    };
    Result mixed, dirty, with_model;
    if (run(hz, nullptr, mixed) != MPC_OK || run(hz_bad, nullptr, dirty) != MPC_OK || run(hz, model.data(), with_model) != MPC_OK) { printf("warm %d: rc\n", warm); return 4; }
    printf("warm %d mixed", warm);
    for (int i = 0; i < B; i++) printf(" %d", mixed.status[i]);
    printf("\nwarm %d dirty", warm);
    for (int i = 0; i < B; i++) printf(" %d", dirty.status[i]);
    printf("\n");
    for (int i = 0; i < B; i++) if (mixed.status[i] != MPC_STATUS_SUCCESS) bad++;
    if (memcmp(mixed.car.data(), with_model.car.data(), sizeof(double) * mixed.car.size()) != 0) bad++;
    if (memcmp(mixed.hist.data(), with_model.hist.data(), sizeof(double) * mixed.hist.size()) != 0 || mixed.iters != with_model.iters) bad++;
    for (int i = 0; i < B; i++) {
      bool is_bad = false;
      for (int j = 0; j < 4; j++) is_bad = is_bad || bad_cars[j] == i;
      if (is_bad) {
        if (dirty.status[i] != MPC_STATUS_INFEASIBLE || dirty.summary[(size_t)MPC_DRIVE_SUM_FAILED * ld + i] != (double)steps) bad++;
        for (int q = 0; q < 6; q++) if (!std::isfinite(dirty.car[(size_t)q * ld + i])) bad++;
        for (int q = 0; q < MPC_DRIVE_NSUM; q++) if (!std::isfinite(dirty.summary[(size_t)q * ld + i])) bad++;
        for (int r = 0; r < steps * MPC_DRIVE_REC; r++) if (!std::isfinite(dirty.hist[(size_t)r * ld + i])) bad++;
        for (int t = 0; t < steps; t++) if (dirty.hist[(size_t)(t * MPC_DRIVE_REC + MPC_DRIVE_REC_STATUS) * ld + i] != (double)MPC_STATUS_INFEASIBLE) bad++;
      } else {
        for (int q = 0; q < 6; q++) if (memcmp(&dirty.car[(size_t)q * ld + i], &mixed.car[(size_t)q * ld + i], sizeof(double)) != 0) bad++;
        for (int q = 0; q < MPC_DRIVE_NSUM; q++) if (memcmp(&dirty.summary[(size_t)q * ld + i], &mixed.summary[(size_t)q * ld + i], sizeof(double)) != 0) bad++;
        for (int r = 0; r < steps * MPC_DRIVE_REC; r++) if (memcmp(&dirty.hist[(size_t)r * ld + i], &mixed.hist[(size_t)r * ld + i], sizeof(double)) != 0) bad++;
        if (dirty.status[i] != mixed.status[i] || dirty.iters[i] != mixed.iters[i]) bad++;
      }
    }
    for (const Result *r : {&mixed, &dirty}) {
      for (int q = 0; q < 6; q++) if (!std::isnan(r->car[(size_t)q * ld + B])) bad++;
      for (int q = 0; q < MPC_DRIVE_NSUM; q++) if (r->summary[(size_t)q * ld + B] != sentinel) bad++;
      for (int q = 0; q < steps * MPC_DRIVE_REC; q++) if (r->hist[(size_t)q * ld + B] != sentinel) bad++;
      if (r->status[B] != isentinel || r->iters[B] != isentinel) bad++;
    }
  }
  printf("bad %d\n", bad);
  return bad == 0 ? 0 : 1;
}
