/*
 * run_model_twin.cpp -- TEST-ONLY CPU build of run() / the telemetry handler with per-instance model values (the mpc_run_*_model and
 * mpc_telemetry_*_model entry points of include/mpc_amd.h, cold and warm).
 *
 * What the device does for one instance, compiled with g++: the instance's column becomes an mpc::ModelVals (ModelVals::column: an
 * unusable column is replaced by the handle's values), which run_pre / telemetry_to_pose / run_post / command_from_run of
 * csrc/mpc_run_core.h read their six values from; between them Solver::setup_model, solve_warm (the warm column through
 * mpc::WarmColumn with the psi box of this call) and unpack_model of csrc/mpc_core.h.  So the five places where a model value enters the
 * run() path can be checked against the oracle with a per-car OrcConfig on a machine without a GPU (tests/test_run_model.py).  Never
 * linked into the product library.
 */
#include <cmath>
#include <cstdint>
#include <vector>

#include "mpc_run_core.h"

namespace {
using WS = mpc::HostWorkspace<double>;
using SV = mpc::Solver<WS, double>;
}  // namespace

/* The arguments of mpc_run_batch_host_warm_model (tel = 0) or mpc_telemetry_batch_host_warm_model plus out8 (tel = 1; `pose` then holds
 * the telemetry rows, `extra` the extra latency and cmd [2][ld] the reply); host arrays, ptsx / ptsy are transformed in place as in
 * mpc_run_batch_host, pre [15][ld] or NULL.  model [MPC_NMODEL][ld], not NULL. */
extern "C" int mpc_run_model_twin_run(const MpcParams *p, int64_t B, int64_t ld, int npts, const double *pose, int tel, double extra,
                                      double *ptsx, double *ptsy, const double *model, const double *warm_in, const int32_t *warm_status,
                                      double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts, double *out8, double *cmd,
                                      int32_t *status, int32_t *iters, double *pre) {
  if (!p || p->N < 3 || p->N > MPC_MAX_N || !opts || opts->size != (int32_t)sizeof(MpcWarmOpts) || ((warm_in || warm_out) && ld_warm < B) ||
      !model || ld < B || npts < 3 || npts > mpc::RUN_MAX_PTS)
    return MPC_ERR_INVALID;
  std::vector<double> wsbuf((size_t)mpc::workspace_fields_per_instance(p->N, false, true));
  for (int64_t i = 0; i < B; i++) {
    const double *mc = model + i;
    const auto col = [mc, ld](int q) { return mc[q * ld]; };
    bool ok;
    const mpc::ModelVals m = mpc::ModelVals::column(*p, col, ok);
    double po[6], px[mpc::RUN_MAX_PTS] = {}, py[mpc::RUN_MAX_PTS] = {};
    for (int q = 0; q < 6; q++) po[q] = pose[q * ld + i];
    if (tel) {
      double t6[6];
      for (int q = 0; q < 6; q++) t6[q] = po[q];
      mpc::telemetry_to_pose(*p, m, t6, extra, po);
    }
    for (int q = 0; q < npts; q++) { px[q] = ptsx[q * ld + i]; py[q] = ptsy[q * ld + i]; }
    mpc::RunPre R;
    mpc::run_pre(*p, m, po, px, py, npts, R);
    for (int q = 0; q < npts; q++) { ptsx[q * ld + i] = px[q]; ptsy[q * ld + i] = py[q]; }
    double w[MPC_NW];
    for (int q = 0; q < MPC_NW; q++) w[q] = p->weights[q];
    SV S(*p, WS{wsbuf.data()});
    /* as in the kernels: the instance's record (and the status it came with) is read before anything of it is written */
    const bool warm = warm_in != nullptr && (warm_status == nullptr || warm_status[i] == MPC_STATUS_SUCCESS);
    int r = S.setup_model(col, R.state, R.coef, R.yaw_lo, R.yaw_hi, w, true);
    if (r == MPC_STATUS_SUCCESS) r = S.solve_warm(warm, mpc::WarmColumn{warm_in + i, ld_warm, R.yaw_lo, R.yaw_hi}, *opts);
    double r9[9], o8[8], *t = nullptr;
    S.unpack_model(col, [&r9](int q) -> double & { return r9[q]; }, [t](int q) -> double & { return t[q]; }, false, R.yaw_lo, R.yaw_hi);
    if (warm_out) {
      double *wo = warm_out + i;
      S.warm_store([wo, ld_warm](int k, int f, double v) { wo[(int64_t)(k * MPC_WARM_REC + f) * ld_warm] = v; });
    }
    status[i] = r;
    if (iters) iters[i] = S.iters;
    mpc::run_post(*p, m, R.max_yaw_change, R.target_speed, R.state[3], r9, o8);
    if (out8) for (int q = 0; q < 8; q++) out8[q * ld + i] = o8[q];
    if (cmd) mpc::command_from_run(m, o8, &cmd[i], &cmd[ld + i]);
    if (pre) {
      for (int q = 0; q < 6; q++) pre[q * ld + i] = R.state[q];
      for (int q = 0; q < 5; q++) pre[(6 + q) * ld + i] = R.coef[q];
      pre[11 * ld + i] = R.yaw_lo; pre[12 * ld + i] = R.yaw_hi; pre[13 * ld + i] = R.max_yaw_change; pre[14 * ld + i] = R.target_speed;
    }
  }
  return MPC_OK;
}
