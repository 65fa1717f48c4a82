/*
 * run_warm_twin.cpp -- TEST-ONLY CPU build of run() / the telemetry handler with a warm start (the mpc_run_*_warm and
 * mpc_telemetry_*_warm entry points of include/mpc_amd.h).
 *
 * What the device does for one instance, compiled with g++: run_pre / telemetry_to_pose / run_post / command_from_run of
 * csrc/mpc_run_core.h around Solver::solve_warm of csrc/mpc_core.h, the warm column read through mpc::WarmColumn -- the one place that
 * knows the rule of the run() path (psi projected into the psi box of this call).  So the rule can be checked against the oracle on
 * a machine without a GPU (tests/test_run_warm.py).  Never linked into the product library.
 */
#include <cmath>
#include <cstdint>
#include <vector>

#include "mpc_run_core.h"

namespace {
using WS = mpc::HostWorkspace<double>;
using SV = mpc::Solver<WS, double>;

/* one instance from (state, coeffs, psi box) on: column i of the warm buffers, out9 = solve()'s vector */
int solve_one(const MpcParams &p, std::vector<double> &wsbuf, const double *st, const double *cf, double yaw_lo, double yaw_hi, bool psi_box,
              int64_t i, const double *warm_in, const int32_t *warm_status, double *warm_out, int64_t ld_warm, const MpcWarmOpts &opts,
              double *out9, int32_t *iters) {
  double w[MPC_NW];
  for (int q = 0; q < MPC_NW; q++) w[q] = p.weights[q];
  SV S(p, WS{wsbuf.data()});
  /* as in the kernels: the instance's column (and the status it came with) is read before anything of it is written */
  const bool warm = warm_in != nullptr && (warm_status == nullptr || warm_status[i] == MPC_STATUS_SUCCESS);
  int r = S.setup(st, cf, yaw_lo, yaw_hi, w, true);
  if (r == MPC_STATUS_SUCCESS)
    r = S.solve_warm(warm, mpc::WarmColumn{warm_in + i, ld_warm, psi_box ? yaw_lo : -HUGE_VAL, psi_box ? yaw_hi : HUGE_VAL}, opts);
  double *t = nullptr;
  S.unpack([out9](int q) -> double & { return out9[q]; }, [t](int q) -> double & { return t[q]; }, false, yaw_lo, yaw_hi);
  if (warm_out) {
    double *wo = warm_out + i;
    S.warm_store([wo, ld_warm](int k, int f, double v) { wo[(int64_t)(k * MPC_WARM_REC + f) * ld_warm] = v; });
  }
  if (iters) *iters = S.iters;
  return r;
}

bool bad_args(const MpcParams *p, int64_t B, const double *warm_in, const double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts) {
  return !p || p->N < 3 || p->N > MPC_MAX_N || !opts || opts->size != (int32_t)sizeof(MpcWarmOpts) || ((warm_in || warm_out) && ld_warm < B);
}
}  // namespace

/* The arguments of mpc_run_batch_host_warm (tel = 0) or mpc_telemetry_batch_host_warm plus out8 (tel = 1; `pose` then holds the
 * telemetry rows, `extra` the extra latency and cmd [2][ld] the reply); host arrays, ptsx / ptsy are only read, pre [15][ld] or NULL. */
extern "C" int mpc_run_warm_twin_run(const MpcParams *p, int64_t B, int64_t ld, int npts, const double *pose, int tel, double extra,
                                     const double *ptsx, const double *ptsy, const double *warm_in, const int32_t *warm_status,
                                     double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts, double *out8, double *cmd,
                                     int32_t *status, int32_t *iters, double *pre) {
  if (bad_args(p, B, warm_in, warm_out, ld_warm, opts) || npts < 3 || npts > mpc::RUN_MAX_PTS) return MPC_ERR_INVALID;
  std::vector<double> wsbuf((size_t)mpc::workspace_fields_per_instance(p->N, false, true));
  for (int64_t i = 0; i < B; i++) {
    double po[6], px[mpc::RUN_MAX_PTS] = {}, py[mpc::RUN_MAX_PTS] = {};
    for (int q = 0; q < 6; q++) po[q] = pose[q * ld + i];
    if (tel) {
      double t6[6];
      for (int q = 0; q < 6; q++) t6[q] = po[q];
      mpc::telemetry_to_pose(*p, t6, extra, po);
    }
    for (int q = 0; q < npts; q++) { px[q] = ptsx[q * ld + i]; py[q] = ptsy[q * ld + i]; }
    mpc::RunPre R;
    mpc::run_pre(*p, po, px, py, npts, R);
    double r9[9], o8[8];
    status[i] = solve_one(*p, wsbuf, R.state, R.coef, R.yaw_lo, R.yaw_hi, true, i, warm_in, warm_status, warm_out, ld_warm, *opts, r9,
                          iters ? iters + i : nullptr);
    mpc::run_post(*p, R.max_yaw_change, R.target_speed, R.state[3], r9, o8);
    if (out8) for (int q = 0; q < 8; q++) out8[q * ld + i] = o8[q];
    if (cmd) mpc::command_from_run(*p, o8, &cmd[i], &cmd[ld + i]);
    if (pre) {
      for (int q = 0; q < 6; q++) pre[q * ld + i] = R.state[q];
      for (int q = 0; q < 5; q++) pre[(6 + q) * ld + i] = R.coef[q];
      pre[11 * ld + i] = R.yaw_lo; pre[12 * ld + i] = R.yaw_hi; pre[13 * ld + i] = R.max_yaw_change; pre[14 * ld + i] = R.target_speed;
    }
  }
  return MPC_OK;
}

/* The solve inside it on its own, the psi box posed by the caller: psi_box != 0 reads the warm column the way the run() path does,
 * psi_box = 0 the way mpc_solve_batch_host_warm does.  out [9][ld]. */
extern "C" int mpc_run_warm_twin_solve(const MpcParams *p, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                       const double *yaw_lo, const double *yaw_hi, int psi_box, const double *warm_in,
                                       const int32_t *warm_status, double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts, double *out,
                                       int32_t *status, int32_t *iters) {
  if (bad_args(p, B, warm_in, warm_out, ld_warm, opts)) return MPC_ERR_INVALID;
  std::vector<double> wsbuf((size_t)mpc::workspace_fields_per_instance(p->N, false, true));
  for (int64_t i = 0; i < B; i++) {
    double st[6], cf[MPC_NCOEF], o9[9];
    for (int q = 0; q < 6; q++) st[q] = state[q * ld + i];
    for (int q = 0; q < MPC_NCOEF; q++) cf[q] = coeffs[q * ld + i];
    status[i] = solve_one(*p, wsbuf, st, cf, yaw_lo[i], yaw_hi[i], psi_box != 0, i, warm_in, warm_status, warm_out, ld_warm, *opts, o9,
                          iters ? iters + i : nullptr);
    for (int q = 0; q < 9; q++) out[q * ld + i] = o9[q];
  }
  return MPC_OK;
}
