/*
 * mpc_amd_noise.h -- the track drive under noise of the C ABI: seeded per-car sensor, actuator and link noise.
 * Part of include/mpc_amd.h, which includes it (do not include it on its own): the three mpc_drive_*_noise entry points, the two
 * functions that need no device, the debug surface of the random stream, and everything a caller needs to know about them.
 */
#ifndef MPC_AMD_NOISE_H
#define MPC_AMD_NOISE_H
#ifndef MPC_AMD_H
#error "include mpc_amd.h"
#endif

/* ---- track drive under noise: a Monte-Carlo over noisy drives as the columns of one launch ------------------------------------------
 * Every other drive is deterministic and noise-free: the handler is told the car's exact position, heading and speed, the actuator
 * does what it was told (or a constant error of it), every reply arrives.  The _noise forms separate "the car" from "what the handler
 * is told about the car" and give every car a reproducible random stream, so seeds x noise levels are the columns of one call.
 *   mpc_drive_batch_device_noise / _device_fused_noise / _host_noise      the _budget forms plus `noise` directly behind `plant` and
 *                                                                          one more output, `seen`, directly behind `hist`
 *
 * The random stream.  The generator is a counter-based Philox4x32-10 as published: multipliers 0xD2511F53, 0xCD9E8D57; key increments
 * 0x9E3779B9, 0xBB67AE85; ten rounds.  Car i at message `step` (0-based) draws two blocks:
 *   key = (s mod 2^32, floor(s / 2^32)), with s the car's seed;
 *   counter = (step, block, 0, 0), block = 0, 1;
 *   each block gives words r0..r3.
 * The stream depends on (seed, step) only.  It does not depend on the instance index, B, ld, the lane or the launch form.
 * From words to values:
 *   uniform: u_j = (r_j + 0.5) * 2^-32, exact in a double, inside (0, 1);
 *   normal pair from (u_a, u_b): rad = sqrt(-2 * log(u_a)), (sn, cs) = sincos(6.283185307179586 * u_b), (z_a, z_b) = (rad * cs, rad * sn)
 *   (log and sincos: the library's own fp64 functions, the ones mpc_debug_math_all shows).
 * Block 0, pairs (r0, r1) and (r2, r3): z_x, z_y, z_psi, z_speed.
 * Block 1: pair (r0, r1): z_steer, z_drift; r2: u_drop; r3 is not used.
 *
 * The column: noise [MPC_NNOISE = 7][ld] doubles, addressed like `plant` (host form: a host array, copied in with the other inputs).
 *   row 0  MPC_NOISE_SEED    s, a double holding an integer, 0 <= s < 2^53
 *   row 1  MPC_NOISE_POS     sigma of the reported x and of the reported y [m], independent
 *   row 2  MPC_NOISE_PSI     sigma of the reported psi [rad]
 *   row 3  MPC_NOISE_SPEED   sigma of the reported speed [mph]
 *   row 4  MPC_NOISE_STEER   sigma of a per-message offset of the steering angle in force [rad]
 *   row 5  MPC_NOISE_DRIFT   sigma of a per-message side speed [m/s] (a gust held for one message)
 *   row 6  MPC_NOISE_DROP    probability that a reply never reaches the car
 * Sensing.  At message t the window is chosen from the TRUE position: the simulator knows where the car is, and the waypoints it sends
 *   are not noisy.  The handler is handed `seen`, not `car`: rows 0..3 are the car's plus sigma * z, rows 4 and 5 are the car's.  A row
 *   whose sigma is exactly 0 is copied, not added to, so the zero column gives the bits of the forms without noise.  With
 *   sigma_speed > 0 the reported speed is max(0, speed + sigma * z): a negative reading is a defect to the handler, and noise must not
 *   manufacture one.  psi is not normalised here; the handler does that.  Everything the handler reads of its message comes from
 *   `seen`: the latency compensation, the vehicle frame, cte0 / epsi0, and the speed in the throttle and the target.  The true `car`
 *   is read by the window, the record and the plant only.
 * Acting.  Between message t and t + 1 the plant column in force gets a per-message perturbation: bias + sigma_steer * z_steer,
 *   drift + sigma_drift * z_drift, on top of the car's `plant` column or the default column; skipped where sigma is 0.
 *   If u_drop < p_drop the reply of message t is discarded: the command in force stays, exactly as for a reply that is not finite;
 *   hist rows 6 and 7 still hold the reply that was sent; rows 4 / 5 of the next record show what was in force.
 * Unchanged: the summary and record rows (MPC_DRIVE_REC stays 13; rows 0..5 stay the TRUE car, rows 8 / 9 stay the handler's own
 *   cte0 / epsi0, which under noise are what it believed); the warm rule; the status and iteration conventions; MpcDriveOpts, MpcParams
 *   and every struct size.
 * A column that cannot be used has any of: a value that is not finite; a sigma below 0; p_drop outside [0, 1]; a seed that is no
 *   integer value or is outside [0, 2^53).  For such a car the `plant` rule applies: the car is driven with the zero column; every
 *   step the handler ended SUCCESS or ACCEPTABLE is INFEASIBLE in hist row 10, summary row 7 and the folded status; the handler's own
 *   status (which the warm rule reads) and the iterations are untouched; there is no not-a-number anywhere; every other car is bit for
 *   bit what it is without the defect.
 * seen: [steps][4][ld] doubles or NULL (host form: a host array): what the handler was told -- x, y, psi, speed -- at every message.
 *   With it a caller can rebuild every handler call.
 * Dispatch and equivalences:
 *   noise == NULL && seen == NULL: the call IS the _budget form, bitwise, with its dispatch, refusals and mpc_drive_info counts.
 *   noise == NULL, seen given: the same, and seen receives the true values.
 *   noise != NULL changes no dispatch rule: the stepwise loop takes the wave kernels up to wave_max_batch as before (the handler is
 *     untouched; only the telemetry it is pointed at differs), and the fused form runs the one launch exactly where it would with
 *     noise == NULL.  `noise` is one more pointer of the builds that exist; there is no new template dimension of the solver kernels.
 *   _fused_noise writes BITWISE what _device_noise writes, seen included.
 * Refusals: with noise or seen non-NULL an MPC_PRECISION_F32 handle is refused first, with the drive's fp64-only text; then everything
 *   the _budget forms refuse, unchanged; a refused call touches nothing.
 * Out of scope: the telemetry handler, run(), the rollouts, the wire forms and the C++ drop-in have no _noise form.  The true lateral
 *   offset of a noisy drive is no record row: a caller computes it from hist rows 0 / 1 and the track.  No time-correlated noise, no
 *   noise on the waypoints, no window chosen from `seen`.
 * Measurements: DESIGN.md section 6p.7 and profiles/drive_noise.json. */
#define MPC_NNOISE 7
enum { MPC_NOISE_SEED = 0, MPC_NOISE_POS, MPC_NOISE_PSI, MPC_NOISE_SPEED, MPC_NOISE_STEER, MPC_NOISE_DRIFT, MPC_NOISE_DROP };
/* rows of out7 of mpc_drive_noise_draw and of out [7][n] of mpc_debug_drive_noise_device */
enum { MPC_DRAW_Z_X = 0, MPC_DRAW_Z_Y, MPC_DRAW_Z_PSI, MPC_DRAW_Z_SPEED, MPC_DRAW_Z_STEER, MPC_DRAW_Z_DRIFT, MPC_DRAW_U_DROP };

int mpc_drive_batch_device_noise(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                                 int n_track, const double *weights, const double *model, const int32_t *horizon, const int32_t *budget,
                                 const double *latency, const double *plant, const double *noise, const MpcDriveOpts *opts,
                                 const MpcWarmOpts *warm_opts, double *summary, double *hist, double *seen, int32_t *status, int32_t *iters,
                                 void *stream);
int mpc_drive_batch_device_fused_noise(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x,
                                       const double *track_y, int n_track, const double *weights, const double *model, const int32_t *horizon,
                                       const int32_t *budget, const double *latency, const double *plant, const double *noise,
                                       const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary, double *hist, double *seen,
                                       int32_t *status, int32_t *iters, void *stream);
int mpc_drive_batch_host_noise(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                               int n_track, const double *weights, const double *model, const int32_t *horizon, const int32_t *budget,
                               const double *latency, const double *plant, const double *noise, const MpcDriveOpts *opts,
                               const MpcWarmOpts *warm_opts, double *summary, double *hist, double *seen, int32_t *status, int32_t *iters);
/* the zero column (seed 0, every sigma 0, p_drop 0), under which a _noise call is the call without noise; no device needed */
int mpc_drive_noise_default(double *col7);
/* The host evaluation of the one draw function: out7 = z_x, z_y, z_psi, z_speed, z_steer, z_drift, u_drop of (seed, step); no device
 * needed.  MPC_ERR_INVALID for a seed that a column may not hold, or step < 0. */
int mpc_drive_noise_draw(double seed, int32_t step, double *out7);
/* Debug surface: the generator on the host, and the draw function on the device for n (seed, step) pairs in one small kernel
 * (seed [n] doubles, step [n] int32, out [7][n]: device pointers; a pair that mpc_drive_noise_draw would refuse gives not-a-number). */
int mpc_debug_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
int mpc_debug_drive_noise_device(MpcHandle *h, int64_t n, const double *seed, const int32_t *step, double *out, void *stream);
#endif /* MPC_AMD_NOISE_H */
