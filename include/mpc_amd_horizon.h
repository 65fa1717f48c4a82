/*
 * mpc_amd_horizon.h -- the per-instance horizon forms of the C ABI.  Part of include/mpc_amd.h, which includes it (do not include it
 * on its own): the seven mpc_*_horizon entry points and everything a caller needs to know about them.
 */
#ifndef MPC_AMD_HORIZON_H
#define MPC_AMD_HORIZON_H
#ifndef MPC_AMD_H
#error "include mpc_amd.h"
#endif

/* ---- per-instance horizon: the N of every instance -----------------------------------------------------------------------------
 * A batch whose instances differ in the horizon as well -- the reference's N / dt study, a horizon sweep over a fleet, a controller
 * that shortens the horizon of some cars -- in one launch on one handle.  One more rule next to the two above: the _horizon form of
 * an entry point is its _model form plus `horizon`, [ld] int32 addressed like yaw_lo (device or host like its neighbours),
 * directly behind `model`.  Seven entry points have one: the solve (device, host), the warm solve (device, host) and the three
 * rollouts.  The telemetry handler and the track drive have _horizon forms of their own -- their _latency forms plus `horizon` behind
 * `model` -- declared and described in mpc_amd_drive.h ("per-car horizon"); run(), the wire forms and the C++ drop-in have none: their
 * problem is one car's message, and its horizon is the handle's.
 * horizon == NULL: the call IS the _model form, bitwise, with every convention and refusal that form has -- with model == NULL too
 *   the plain form, wave path included.
 * horizon != NULL: instance i is solved as the reference solves it with Config::N = horizon[i] -- 8n - 2 variables, 6n rows -- and
 *   everything else is as in the _model form.  `model` may be NULL: the handle's own six values are then used as they are.
 *   Valid: 3 <= horizon[i] <= the handle's N.  Any other value ends that instance as an unusable model column does:
 *   MPC_STATUS_INFEASIBLE, the start point in `out`, no not-a-number (traj and warm_out hold the start point of the handle's own
 *   horizon), and the batch goes on.
 * Array shapes keep the handle's N.
 *   traj [2N][ld]: column i holds x_0 .. x_{n-1} in rows 0 .. n-1 and y in rows N .. N+n-1; its other rows are not written.
 *   warm_in / warm_out [mpc_warm_rows(N)][ld_warm]: instance i reads and writes the records of its stages 0 .. n-2; the rows behind
 *   them are neither read nor written.  With shift = 1 the repeated last record is record n-2.  A record written under another
 *   horizon is an ordinary candidate: the box test and the cold fallback of every warm call apply, and nothing more.
 *   (Host forms: rows that are not written come back as the caller has them; traj and warm_out travel to the device for that.)
 * Dispatch: as for a model call -- ONE launch of the single-phase fp64 lane kernel at every B, no wave path, no deferred tails, no
 *   pass cuts, no take order; lane compaction at its usual threshold.  The launch is a build of its own (HORIZON): the lanes of a
 *   wave differ in their number of stages, so it addresses its workspace rows per lane and does not stage them through LDS.
 * Cost, and advice: a pass of a wave lasts as long as the longest horizon among its 64 running lanes, and the library does not
 *   reorder instances.  SORT A BATCH BY HORIZON so that neighbouring instances have similar ones.  The unstaged build is also
 *   slower per stage than the staged _model build.  Measured on one MI355X, 65 536 instances: every horizon
 *   equal to the handle's N = 10, 2.53 against 2.18 ms of the _model launch (1.16 x); at N = 25, 177 against 179 ms (the slowest
 *   chains decide); horizons {10, 20, 30, 40, 50} in equal shares on an N = 50 handle, one launch 580 ms sorted / 597 ms shuffled
 *   against 1 016 ms for five _model launches on handles of those N (937 ms on the parent commit's library).  A batch of ONE
 *   horizon is better served by a handle of that N.
 * Accepted handles: the model rule -- every fp64 handle, also one whose ordinary solve starts in fp32, bitwise a handle created
 *   with f64_f32_start = 0.
 * Refusals: an MPC_PRECISION_F32 handle gets MPC_ERR_INVALID with the model message.  max_soc > 0 together with a non-NULL horizon
 *   gets MPC_ERR_UNSUPPORTED with a message that names both (a deliberate cut: there is no SOC build with per-lane rows); with
 *   horizon == NULL nothing changes.  ld < B and ld_warm < B get MPC_ERR_INVALID as ever.
 * mpc_rollout_batch_device_fused_horizon writes bitwise what the stepwise _horizon (warm_start = 0) / _warm_horizon (1) rollout
 *   writes, in one launch at every B >= 1; mpc_rollout_fused_info counts it. */
int mpc_solve_batch_device_horizon(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                   const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                   const int32_t *horizon, double *out, double *traj, int32_t *status, int32_t *iters, void *stream);
int mpc_solve_batch_host_horizon(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                 const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                 const int32_t *horizon, double *out, double *traj, int32_t *status, int32_t *iters);
int mpc_solve_batch_device_warm_horizon(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                        const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                        const int32_t *horizon, const double *warm_in, const int32_t *warm_status, double *warm_out,
                                        int64_t ld_warm, const MpcWarmOpts *opts, double *out, double *traj, int32_t *status,
                                        int32_t *iters, void *stream);
int mpc_solve_batch_host_warm_horizon(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                      const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                      const int32_t *horizon, const double *warm_in, const int32_t *warm_status, double *warm_out,
                                      int64_t ld_warm, const MpcWarmOpts *opts, double *out, double *traj, int32_t *status,
                                      int32_t *iters);
int mpc_rollout_batch_device_horizon(MpcHandle *h, int64_t B, int64_t ld, int steps, double *state, const double *coeffs,
                                     const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                     const int32_t *horizon, double *hist, int32_t *status, int32_t *iters, void *stream);
int mpc_rollout_batch_device_warm_horizon(MpcHandle *h, int64_t B, int64_t ld, int steps, double *state, const double *coeffs,
                                          const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                          const int32_t *horizon, const MpcWarmOpts *opts, double *hist, int32_t *status,
                                          int32_t *iters, void *stream);
int mpc_rollout_batch_device_fused_horizon(MpcHandle *h, int64_t B, int64_t ld, int steps, double *state, const double *coeffs,
                                           const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                           const int32_t *horizon, int warm_start, const MpcWarmOpts *opts, double *hist,
                                           int32_t *status, int32_t *iters, void *stream);

#endif /* MPC_AMD_HORIZON_H */
