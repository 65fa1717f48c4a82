/*
 * mpc_amd_budget.h -- the per-instance iteration budget of the C ABI: the reference's solve deadline, for solves and track drives.
 * Part of include/mpc_amd.h, which includes it (do not include it on its own): the five mpc_*_budget entry points and everything a
 * caller needs to know about them.
 */
#ifndef MPC_AMD_BUDGET_H
#define MPC_AMD_BUDGET_H
#ifndef MPC_AMD_H
#error "include mpc_amd.h"
#endif

/* ---- per-instance iteration budget: how much solver work a message may cost -----------------------------------------------------
 * The reference gives every solve a deadline (MPC::MPC sets max_cpu_time = Config::ipoptTimeout, MPC.cpp:176-178): when it fires,
 * solve() returns IPOPT's current iterate and run() drives the car with it.  A wall-clock limit has no deterministic meaning where
 * 64 instances share a wave, so the deadline is counted here in interior-point iterations, per instance: reproducible bit for bit
 * and comparable with a CPU build.  `budget`, [ld] int32 addressed like `horizon` (device or host like its neighbours), stands
 * directly behind `horizon` in five entry points:
 *   mpc_solve_batch_device_budget / _host_budget           the _warm_horizon forms plus `budget`
 *   mpc_drive_batch_device_budget / _device_fused_budget / _host_budget      the _plant forms plus `budget`
 * horizon, model, weights and the warm arguments may each be NULL, as in the forms they extend; a solve with all warm arguments NULL
 * is the cold solve.
 * budget == NULL: the call IS the form it extends, bitwise, with that form's dispatch, refusals and info counters.
 * budget != NULL, what budget[i] = b means:
 *   b is the number of interior-point iterations instance i may take in this call over ALL of its attempts -- the warm attempt, the
 *   cold solve that follows a refused record or a failed warm attempt, and the one restart -- counted as `iters` reports them.  The
 *   convergence test and the acceptable-level test come first, as they come before max_iter; the termination polish reads the same
 *   cap.  When the count reaches b the instance ends MPC_STATUS_MAXITER with its current iterate in out, traj and warm_out, exactly
 *   as a max_iter stop leaves them, and iters[i] == b.  An end by budget is final in every attempt: no cold solve and no restart
 *   follow it.  An attempt that ends in any other way is followed by what follows it without a budget, with what is left of the
 *   budget (at least one iteration); the handle's max_iter still bounds each attempt.
 *   Valid: b >= 1.  b < 1 ends that instance as an unusable horizon does: MPC_STATUS_INFEASIBLE, the start point, no not-a-number,
 *   and the batch goes on -- every other instance is bit for bit what it is without the defect.
 *   Warm records: a record whose warm_status is MPC_STATUS_MAXITER is a candidate like one with MPC_STATUS_SUCCESS -- it is an interior
 *   iterate of the same NLP, and handing it on is what makes warm start meaningful under a deadline (the real-time-iteration scheme).
 *   The box test and every other warm rule apply unchanged.
 * The drive: each car's handler call of every step is solved under budget[i].  From step 2 on, with warm_start, a car whose previous
 *   step ended SUCCESS or MAXITER starts warm.  Summary row 7 and hist rows 10 and 11 report what they report without a budget: a
 *   MAXITER step counts as not SUCCESS.  model, horizon, latency and plant combine with budget.
 * Dispatch: the rule of a horizon call -- ONE launch of the single-phase fp64 lane kernel's per-lane-rows build (HORIZON) at every B:
 *   no wave path, no fp32 start, no deferred tails, no pass cuts, no take order; horizon == NULL then means the handle's N for every
 *   instance.  The fused drive runs the one launch where mpc_drive_batch_device_fused_horizon would.  `budget` is one more pointer of
 *   those builds; there is no new kernel.
 * Refusals: an MPC_PRECISION_F32 handle gets MPC_ERR_INVALID with the model message; max_soc > 0 together with a non-NULL budget gets
 *   MPC_ERR_UNSUPPORTED with a message that names both; every refusal of the extended form follows, unchanged.
 * Out of scope: the telemetry handler, run(), the rollouts, the wire forms and the C++ drop-in have no public _budget form.  (The
 *   telemetry handler carries the column internally, to serve the stepwise drive.)
 * Measurements: DESIGN.md section 6p.6 and profiles/drive_budget.json. */
int mpc_solve_batch_device_budget(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs, const double *yaw_lo,
                                  const double *yaw_hi, const double *weights, const double *model, const int32_t *horizon,
                                  const int32_t *budget, const double *warm_in, const int32_t *warm_status, double *warm_out, int64_t ld_warm,
                                  const MpcWarmOpts *opts, double *out, double *traj, int32_t *status, int32_t *iters, void *stream);
int mpc_solve_batch_host_budget(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs, const double *yaw_lo,
                                const double *yaw_hi, const double *weights, const double *model, const int32_t *horizon,
                                const int32_t *budget, const double *warm_in, const int32_t *warm_status, double *warm_out, int64_t ld_warm,
                                const MpcWarmOpts *opts, double *out, double *traj, int32_t *status, int32_t *iters);
int mpc_drive_batch_device_budget(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                                  int n_track, const double *weights, const double *model, const int32_t *horizon, const int32_t *budget,
                                  const double *latency, const double *plant, const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts,
                                  double *summary, double *hist, int32_t *status, int32_t *iters, void *stream);
int mpc_drive_batch_device_fused_budget(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x,
                                        const double *track_y, int n_track, const double *weights, const double *model, const int32_t *horizon,
                                        const int32_t *budget, const double *latency, const double *plant, const MpcDriveOpts *opts,
                                        const MpcWarmOpts *warm_opts, double *summary, double *hist, int32_t *status, int32_t *iters,
                                        void *stream);
int mpc_drive_batch_host_budget(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                                int n_track, const double *weights, const double *model, const int32_t *horizon, const int32_t *budget,
                                const double *latency, const double *plant, const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts,
                                double *summary, double *hist, int32_t *status, int32_t *iters);
#endif /* MPC_AMD_BUDGET_H */
