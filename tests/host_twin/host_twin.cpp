/*
 * host_twin.cpp -- TEST-ONLY CPU build of carnd-mpc-project_amd/csrc/mpc_core.h.
 *
 * The build container has no GPU, so the interior-point/Riccati logic of the
 * device solver is debugged here by compiling the very same header with g++
 * and checking it against the oracle (tests/test_host_twin.py).  This file is
 * never linked into the product library and nothing in the product path
 * loads it: the shipped path is HIP only and fails loudly without a device.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mpc_core.h"
#include "mpc_run_core.h"

template <class R>
static int twin_solve(const MpcParams *p, int64_t B, int64_t ld, const R *state, const R *coeffs, const R *yaw_lo, const R *yaw_hi,
                      const R *weights, R *out, R *traj, int32_t *status, int32_t *iters) {
  if (!p || p->N < 3 || p->N > MPC_MAX_N) return MPC_ERR_INVALID;
  const int N = p->N;
  std::vector<R> wsbuf((size_t)mpc::workspace_fields_per_instance(N, sizeof(R) == 4, true));
  for (int64_t i = 0; i < B; i++) {
    R st[6], cf[MPC_NCOEF], w[MPC_NW], o9[9];
    std::vector<R> tr(2 * N);
    mpc::gather_instance(*p, i, ld, state, coeffs, weights, st, cf, w);
    mpc::HostWorkspace<R> ws{wsbuf.data()};
    int it = 0;
    int s = mpc::solve_instance<mpc::HostWorkspace<R>, R>(*p, ws, st, cf, yaw_lo[i], yaw_hi[i], w, o9, traj ? tr.data() : nullptr, &it);
    for (int q = 0; q < 9; q++) out[q * ld + i] = o9[q];
    if (traj) for (int q = 0; q < 2 * N; q++) traj[q * ld + i] = tr[q];
    status[i] = s;
    if (iters) iters[i] = it;
  }
  return MPC_OK;
}

extern "C" int mpc_host_twin_solve(const MpcParams *p, int64_t B, int64_t ld, const double *state,
                                   const double *coeffs, const double *yaw_lo, const double *yaw_hi,
                                   const double *weights, double *out, double *traj, int32_t *status,
                                   int32_t *iters) {
  return twin_solve<double>(p, B, ld, state, coeffs, yaw_lo, yaw_hi, weights, out, traj, status, iters);
}
/* the MPC_PRECISION_F32 solver (float I/O) */
extern "C" int mpc_host_twin_solve_f32(const MpcParams *p, int64_t B, int64_t ld, const float *state,
                                       const float *coeffs, const float *yaw_lo, const float *yaw_hi,
                                       const float *weights, float *out, float *traj, int32_t *status,
                                       int32_t *iters) {
  return twin_solve<float>(p, B, ld, state, coeffs, yaw_lo, yaw_hi, weights, out, traj, status, iters);
}

extern "C" void mpc_host_twin_math(int64_t n, const double *x, double *sn, double *cs, double *rc) {
  for (int64_t i = 0; i < n; i++) { mpc::fsincos(x[i], &sn[i], &cs[i]); rc[i] = mpc::frcp(x[i]); }
}
extern "C" void mpc_host_twin_math_f32(int64_t n, const float *x, float *sn, float *cs, float *at) {
  for (int64_t i = 0; i < n; i++) { mpc::fsincos(x[i], &sn[i], &cs[i]); at[i] = mpc::fatan(x[i]); }
}
extern "C" void mpc_host_twin_math2(int64_t n, const double *x, double *at, double *lg) {
  for (int64_t i = 0; i < n; i++) { at[i] = mpc::fatan(x[i]); lg[i] = mpc::flog(fabs(x[i])); }
}
/* mpc_debug_math_all of the library on the CPU: the same rows ([MPC_DEBUG_MATH_ROWS][n]) from the same mpc:: functions */
template <class R>
static void twin_math_rows(R x, R y, double *out, int64_t n) {
  R sa, ca, sb, cb;
  mpc::fsincos2(x, y, &sa, &ca, &sb, &cb);
  out[0] = (double)sa; out[n] = (double)ca; out[2 * n] = (double)sb; out[3 * n] = (double)cb;
  out[4 * n] = (double)mpc::frcp(x); out[5 * n] = (double)mpc::frcp1(x);
  out[6 * n] = (double)mpc::fatan(x); out[7 * n] = (double)mpc::flog(x);
  out[8 * n] = (double)mpc::hpow(x, mpc::IpmConst<R>::s_theta); out[9 * n] = (double)mpc::hpow(x, mpc::IpmConst<R>::s_phi);
}
extern "C" int mpc_host_twin_math_all(int64_t n, const double *x, const double *y, double *out) {
  if (n < 0 || (n > 0 && (!x || !y || !out))) return MPC_ERR_INVALID;
  for (int64_t i = 0; i < n; i++) {
    twin_math_rows<double>(x[i], y[i], out + i, n);
    twin_math_rows<float>((float)x[i], (float)y[i], out + 10 * n + i, n);
  }
  return MPC_OK;
}

/* MPC::run pre/post-processing of the device header, one instance at a time (struct-of-arrays I/O like the ABI):
 * pose[6][ld], pts[npts][ld] in/out, pre[RUN_PRE_ROWS][ld] (the rows: mpc_run_core.h) */
extern "C" int mpc_host_twin_run_pre(const MpcParams *p, int64_t B, int64_t ld, int npts, const double *pose, double *ptsx,
                                     double *ptsy, double *pre, int32_t *ncoef) {
  if (npts < 3 || npts > mpc::RUN_MAX_PTS) return MPC_ERR_INVALID;
  for (int64_t i = 0; i < B; i++) {
    const int nc = mpc::run_pre_instance<false>(*p, *p, i, ld, npts, pose, 0.0, ptsx, ptsy, pre, ld);
    if (ncoef) ncoef[i] = nc;
  }
  return MPC_OK;
}
extern "C" void mpc_host_twin_run_post(const MpcParams *p, double max_yaw_change, double target_speed, double v0, const double *r9, double *o8) {
  mpc::run_post(*p, max_yaw_change, target_speed, v0, r9, o8);
}

/* N2: telemetry handler pieces (mpc_run_core.h) */
extern "C" void mpc_host_twin_tel_pose(const MpcParams *p, const double *tel6, double extra, double *pose6) {
  mpc::telemetry_to_pose(*p, tel6, extra, pose6);
}
extern "C" void mpc_host_twin_tel_cmd(const MpcParams *p, const double *o8, double *cmd2) {
  mpc::command_from_run(*p, o8, &cmd2[0], &cmd2[1]);
}

/* The multi-phase solve of the device kernel, replayed on the host: run the state machine, PARK the instance after
 * `pass_cut` passes (at a pass boundary in the DIR phase), then RESUME it in a different solver object on a different
 * workspace that only receives the current iterate slot -- exactly what a resume phase of mpc_solve_kernel does.  With
 * `repeat` the instance is parked again every `pass_cut` passes (the two objects take turns), as under a cut schedule. */
template <class R>
static int solve_parked_t(const MpcParams *p, int64_t B, int64_t ld, int pass_cut, int repeat, const R *state, const R *coeffs,
                          const R *yaw_lo, const R *yaw_hi, const R *weights, R *out, int32_t *status, int32_t *iters,
                          int32_t *was_parked) {
  if (!p || p->N < 3 || p->N > MPC_MAX_N) return MPC_ERR_INVALID;
  const int N = p->N, M = N - 1;
  using SV = mpc::Solver<mpc::HostWorkspace<R>, R>;
  using FD = mpc::Fields<R>;
  std::vector<R> wsA((size_t)(M + 1) * FD::STAGE_SZ), wsB((size_t)(M + 1) * FD::STAGE_SZ, R(-7.0));
  for (int64_t i = 0; i < B; i++) {
    R st[6], cf[MPC_NCOEF], w[MPC_NW];
    double park[SV::PARK_N];
    mpc::gather_instance(*p, i, ld, state, coeffs, weights, st, cf, w);
    SV A(*p, mpc::HostWorkspace<R>{wsA.data()});
    int s = A.setup(st, cf, yaw_lo[i], yaw_hi[i], w), attempt = 0, it_total = 0, passes = 0;
    SV *fin = &A;
    SV Bs(*p, mpc::HostWorkspace<R>{wsB.data()});
    was_parked[i] = 0;
    if (s == MPC_STATUS_SUCCESS) {
      A.begin(true);
      SV *cur = &A;
      std::vector<R> *wcur = &wsA, *woth = &wsB;
      for (;;) {
        const int r = cur->step();
        ++passes;
        if (r != SV::MPC_RUNNING) {
          if (cur->next_attempt(r, attempt, it_total)) continue;
          s = r; cur->iters += it_total; fin = cur;
          break;
        }
        if ((cur == &A || repeat) && pass_cut > 0 && passes >= pass_cut && cur->phase == SV::PH_DIR) {
          SV *oth = cur == &A ? &Bs : &A;
          cur->park([&park](int q) -> double & { return park[q]; }, attempt, it_total);
          std::fill(woth->begin(), woth->end(), R(-7.0));                /* nothing but the iterate slot comes along */
          oth->setup(st, cf, yaw_lo[i], yaw_hi[i], w, false);
          oth->unpark([&park](int q) -> double { return park[q]; }, attempt, it_total);
          const int I = oth->cur ? FD::IT1 : FD::IT0;
          for (int k = 0; k < M; k++)
            for (int f = 0; f < FD::IT_SZ; f++) (*woth)[(size_t)k * FD::STAGE_SZ + I + f] = (*wcur)[(size_t)k * FD::STAGE_SZ + I + f];
          cur = oth; std::swap(wcur, woth); was_parked[i] += 1; passes = 0;
        }
      }
    }
    R o9[9];
    R *o = o9;
    fin->unpack([o](int q) -> R & { return o[q]; }, [o](int) -> R & { return o[0]; }, false, yaw_lo[i], yaw_hi[i]);
    for (int q = 0; q < 9; q++) out[q * ld + i] = o9[q];
    status[i] = s; iters[i] = fin->iters;
  }
  return MPC_OK;
}
extern "C" int mpc_host_twin_solve_parked(const MpcParams *p, int64_t B, int64_t ld, int pass_cut, const double *state,
                                          const double *coeffs, const double *yaw_lo, const double *yaw_hi,
                                          const double *weights, double *out, int32_t *status, int32_t *iters,
                                          int32_t *was_parked) {
  return solve_parked_t<double>(p, B, ld, pass_cut, 0, state, coeffs, yaw_lo, yaw_hi, weights, out, status, iters, was_parked);
}
extern "C" int mpc_host_twin_solve_reparked(const MpcParams *p, int64_t B, int64_t ld, int pass_cut, const double *state,
                                            const double *coeffs, const double *yaw_lo, const double *yaw_hi,
                                            const double *weights, double *out, int32_t *status, int32_t *iters,
                                            int32_t *was_parked) {
  return solve_parked_t<double>(p, B, ld, pass_cut, 1, state, coeffs, yaw_lo, yaw_hi, weights, out, status, iters, was_parked);
}
extern "C" int mpc_host_twin_solve_reparked_f32(const MpcParams *p, int64_t B, int64_t ld, int pass_cut, const float *state,
                                                const float *coeffs, const float *yaw_lo, const float *yaw_hi,
                                                const float *weights, float *out, int32_t *status, int32_t *iters,
                                                int32_t *was_parked) {
  return solve_parked_t<float>(p, B, ld, pass_cut, 1, state, coeffs, yaw_lo, yaw_hi, weights, out, status, iters, was_parked);
}


/* Mixed precision across phases, replayed on the host exactly as the device does it (MpcParams.f32_finish on an F32 handle:
 * RIO = float; f64_f32_start on an F64 handle: RIO = double): the fp32 solver runs until it returns MPC_PROMOTE, the instance is
 * parked, an fp64 solver unparks it on its own workspace (iterate record converted field by field), re-evaluates the point and
 * finishes; an instance the fp64 phase cannot finish from there is solved again from the start point, as the single-phase solve
 * begins.  iters_f32[i]: iterations of the fp32 phase. */
template <class RIO>
static int solve_mixed_t(const MpcParams *p, int64_t B, int64_t ld, const RIO *state, const RIO *coeffs, const RIO *yaw_lo, const RIO *yaw_hi,
                         const RIO *weights, RIO *out, RIO *traj, int32_t *status, int32_t *iters, int32_t *iters_f32) {
  if (!p || p->N < 3 || p->N > MPC_MAX_N) return MPC_ERR_INVALID;
  const int N = p->N, M = N - 1;
  using SF = mpc::Solver<mpc::HostWorkspace<float>, float>;
  using SD = mpc::Solver<mpc::HostWorkspace<double>, double>;
  using FF = mpc::Fields<float>;
  using FD = mpc::Fields<double>;
  std::vector<float> wsf((size_t)(M + 1) * FF::STAGE_SZ);
  std::vector<double> wsd((size_t)(M + 1) * FD::STAGE_SZ);
  for (int64_t i = 0; i < B; i++) {
    float st[6], cf[MPC_NCOEF], w[MPC_NW];
    double std_[6], cfd[MPC_NCOEF], wd[MPC_NW], park[SF::PARK_N];
    for (int q = 0; q < 6; q++) { st[q] = (float)state[q * ld + i]; std_[q] = (double)state[q * ld + i]; }
    for (int q = 0; q < MPC_NCOEF; q++) { cf[q] = (float)coeffs[q * ld + i]; cfd[q] = (double)coeffs[q * ld + i]; }
    for (int q = 0; q < MPC_NW; q++) { w[q] = weights ? (float)weights[q * ld + i] : (float)p->weights[q]; wd[q] = weights ? (double)weights[q * ld + i] : p->weights[q]; }
    SF A(*p, mpc::HostWorkspace<float>{wsf.data()});
    SD D(*p, mpc::HostWorkspace<double>{wsd.data()});
    int s = A.setup(st, cf, (float)yaw_lo[i], (float)yaw_hi[i], w), attempt = 0, it_total = 0;
    bool in_double = false;
    if (iters_f32) iters_f32[i] = 0;
    if (s == MPC_STATUS_SUCCESS) {
      A.promote_mu = (float)p->mixed_switch_mu;
      if (const char *e = getenv("MPC_TWIN_PROMOTE_CAP")) A.promote_cap = atoi(e);     /* (analysis aid) */
      A.begin(true);
      for (;;) {
        const int r = in_double ? D.step() : A.step();
        if (r == SF::MPC_RUNNING) continue;
        if (r == SF::MPC_PROMOTE && !A.promote_clean) {   /* a hand-over out of trouble (allowance used up, line search / inertia out of single precision): from the start point in fp64 */
          if (iters_f32) iters_f32[i] = A.iter + it_total;
          (void)D.setup(std_, cfd, (double)yaw_lo[i], (double)yaw_hi[i], wd, true);
          D.begin(true); attempt = 0; it_total = A.iter; in_double = true;
          continue;
        }
        if (r == SF::MPC_PROMOTE) {
          A.park([&park](int q) -> double & { return park[q]; }, attempt, it_total);
          if (iters_f32) iters_f32[i] = A.iter + it_total;
          (void)D.setup(std_, cfd, (double)yaw_lo[i], (double)yaw_hi[i], wd, false);
          D.unpark([&park](int q) -> double { return park[q]; }, attempt, it_total);
          const int Is = A.cur ? FF::IT1 : FF::IT0, Id = D.cur ? FD::IT1 : FD::IT0;
          for (int k = 0; k < M; k++)
            mpc::convert_iterate_record<float, double>([&](int f) { return A.ws.it(k, Is, f); }, [&](int f, double v) { D.ws.it(k, Id, f) = v; });
          D.promoted();
          attempt = -1;
          in_double = true;
          continue;
        }
        if (r == MPC_STATUS_NUMERIC && !in_double) {      /* not-a-number in fp32 is not a verdict: fp64 solves it from the start point */
          (void)D.setup(std_, cfd, (double)yaw_lo[i], (double)yaw_hi[i], wd, true);
          D.begin(true); attempt = 0; it_total = A.iter + it_total; in_double = true;
          continue;
        }
        /* (attempt -1: started by fp32, not finished by fp64: solved again as the single-phase solve does it) */
        if (in_double ? D.next_attempt(r, attempt, it_total) : A.next_attempt(r, attempt, it_total)) continue;
        s = r;
        break;
      }
    }
    RIO *o = out + i;
    RIO *t = traj ? traj + i : nullptr;
    struct Ref { RIO *q; void operator=(double v) { *q = (RIO)v; } void operator=(float v) { *q = (RIO)v; } };
    if (in_double) D.unpack([o, ld](int q) { return Ref{o + q * ld}; }, [t, ld](int q) { return Ref{t + q * ld}; }, traj != nullptr, (double)yaw_lo[i], (double)yaw_hi[i]);
    else A.unpack([o, ld](int q) { return Ref{o + q * ld}; }, [t, ld](int q) { return Ref{t + q * ld}; }, traj != nullptr, (float)yaw_lo[i], (float)yaw_hi[i]);
    status[i] = s;
    if (iters) iters[i] = (in_double ? D.iters : A.iters) + it_total;
  }
  return MPC_OK;
}
extern "C" int mpc_host_twin_solve_mixed(const MpcParams *p, int64_t B, int64_t ld, const float *state, const float *coeffs,
                                         const float *yaw_lo, const float *yaw_hi, const float *weights, float *out, float *traj,
                                         int32_t *status, int32_t *iters, int32_t *iters_f32) {
  return solve_mixed_t<float>(p, B, ld, state, coeffs, yaw_lo, yaw_hi, weights, out, traj, status, iters, iters_f32);
}
extern "C" int mpc_host_twin_solve_mixed_f64(const MpcParams *p, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                             const double *yaw_lo, const double *yaw_hi, const double *weights, double *out, double *traj,
                                             int32_t *status, int32_t *iters, int32_t *iters_f32) {
  return solve_mixed_t<double>(p, B, ld, state, coeffs, yaw_lo, yaw_hi, weights, out, traj, status, iters, iters_f32);
}

/* What the device's staged workspace moves per instance: the same solver on a workspace that counts the reals its sweeps
 * ask for (stage_fetch_* = one LDS-DMA record each, store_run = the group stores) -- the bytes the ACTIVE lanes of a wave
 * request, to put beside the FETCH_SIZE / WRITE_SIZE counters of a launch (tools/traffic_model.py).  counts[i] = reals
 * fetched, reals stored, passes (Solver::step calls), iterations. */
struct TrafficCount { long long fetched = 0, stored = 0; };
template <class R>
struct CountingWorkspace : mpc::HostWorkspace<R> {
  using F = mpc::Fields<R>;
  TrafficCount *c;
  CountingWorkspace(R *b, TrafficCount *cc) : mpc::HostWorkspace<R>{b}, c(cc) {}
  template <int F0, int COUNT> void store_run(int k, int I, const R *v) const {
    c->stored += (COUNT + F::G - 1) / F::G * F::G;
    mpc::HostWorkspace<R>::template store_run<F0, COUNT>(k, I, v);
  }
  void setD(int k, int j, R v) const { c->stored += 1; mpc::HostWorkspace<R>::setD(k, j, v); }
  void stage_fetch_it(int, int, int) const { c->fetched += F::IT_SZ; }
  void stage_fetch_itf(int, int, int) const { c->fetched += 16; }
  void stage_fetch_d(int, int) const { c->fetched += F::D_N; }
  void stage_fetch_g(int, int, int) const { c->fetched += F::GAIN_SZ; }
};

template <class R>
static int traffic_t(const MpcParams *p, int64_t B, int64_t ld, const R *state, const R *coeffs, const R *yaw_lo, const R *yaw_hi,
                     const R *weights, int64_t *counts) {
  if (!p || p->N < 3 || p->N > MPC_MAX_N) return MPC_ERR_INVALID;
  using WS = CountingWorkspace<R>;
  using SV = mpc::Solver<WS, R>;
  std::vector<R> wsbuf((size_t)mpc::workspace_fields_per_instance(p->N, sizeof(R) == 4, true));
  for (int64_t i = 0; i < B; i++) {
    R st[6], cf[MPC_NCOEF], w[MPC_NW];
    mpc::gather_instance(*p, i, ld, state, coeffs, weights, st, cf, w);
    TrafficCount c;
    SV S(*p, WS(wsbuf.data(), &c));
    int s = S.setup(st, cf, yaw_lo[i], yaw_hi[i], w), attempt = 0, it_total = 0;
    long long passes = 0;
    if (s == MPC_STATUS_SUCCESS) {
      S.begin(true);
      for (;;) {
        const int r = S.step();
        ++passes;
        if (r == SV::MPC_RUNNING) continue;
        if (S.next_attempt(r, attempt, it_total)) continue;
        break;
      }
    }
    counts[4 * i + 0] = c.fetched; counts[4 * i + 1] = c.stored; counts[4 * i + 2] = passes; counts[4 * i + 3] = S.iters + it_total;
  }
  return MPC_OK;
}
extern "C" int mpc_host_twin_traffic(const MpcParams *p, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                     const double *yaw_lo, const double *yaw_hi, const double *weights, int64_t *counts) {
  return traffic_t<double>(p, B, ld, state, coeffs, yaw_lo, yaw_hi, weights, counts);
}
