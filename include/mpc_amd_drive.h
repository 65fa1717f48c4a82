/*
 * mpc_amd_drive.h -- track driving on the device.  Part of include/mpc_amd.h, which includes it (do not include it on its own): the
 * mpc_drive_* entry points and everything a caller needs to know about them.
 */
#ifndef MPC_AMD_DRIVE_H
#define MPC_AMD_DRIVE_H
#ifndef MPC_AMD_H
#error "include mpc_amd.h"
#endif

/* ---- track driving: waypoint window, telemetry handler and plant, `steps` times, in one call -------------------------------------
 * Does this configuration get the car round the track, and how well?  A call drives B cars for `steps` telemetry messages.  Per
 * message and car: pick the waypoint window at the car's position, run the telemetry handler on (car, window, extra_latency) -- the
 * very call mpc_telemetry_batch_device makes, or its _warm form -- and move the car under the command it was sent, late.  Nothing
 * returns to the host between the steps and nothing is synchronised.
 *
 * THE PLANT IS NOT THE UNITY SIMULATOR.  It is the reference's own model of it: the kinematic step the reference uses to compensate
 * its latency (Vehicle::move, src/model/Vehicle.cpp:145-168) with the handler's own reading of the telemetry (the sign of the steering
 * angle, src/mpc_main.cpp:131; the acceleration (throttle - v / 50) * 6, src/mpc_main.cpp:156).  A lap under this plant says how the
 * controller does in the world it believes in; it says nothing about tyres, drag or the simulator's actuator dynamics.
 *
 * A car: six doubles, the rows of car [6][ld] = the rows of `tel` of the telemetry entry points --
 *   0, 1, 2  x, y, psi [rad]      3  speed [mph]      4  steering_angle [rad, simulator sign]      5  throttle
 *   Rows 4 and 5 are the command in force.  In: the cars at the first message; out: the cars after the last plant step.
 * A track: track_x [n_track], track_y [n_track], device doubles, cyclic, npts <= n_track <= MPC_DRIVE_MAX_TRACK.
 * Window.  j = the waypoint with the smallest dx * dx + dy * dy (ties: the lowest index; a distance that is not a number never
 *   wins, so j = 0 for a car whose position is not finite); k = j if (p - w_j) . (w_{j+1} - w_j) > 0, else j - 1; the window is
 *   w[k .. k + npts - 1], cyclically, k in 0 .. n_track - 1.  The search has n_track trips: no data decides a branch around a loop.
 * Handler.  mpc_telemetry_batch_device on (car, window, extra_latency), or with warm_start != 0 mpc_telemetry_batch_device_warm (the
 *   run()-path rule: records unshifted by default, psi projected into the new box; step 1 is cold, a car whose previous step did not
 *   succeed starts cold).  The warm buffer lives in the handle, as for mpc_rollout_batch_device_warm.  One addition: weights
 *   [MPC_NW][ld], or NULL, is passed to every solve as mpc_solve_batch_device takes it.  Small batches go through the wave kernels
 *   exactly as the telemetry entry point does.
 * Plant.  sub_old substeps of length h under rows 4 / 5; then rows 4 / 5 become (cmd_steer * max_steering, cmd_throttle) -- if either
 *   is not finite the old command stays in force --; then sub_new substeps.  One substep: v = speed * 1609.34 / 3600,
 *   steer = -steering_angle, accel = (throttle - v / 50) * 6 (recomputed every substep), Vehicle::move(h), speed back to mph.  psi is
 *   not normalised: the handler does that.
 * summary [MPC_DRIVE_NSUM][ld], accumulated in step order:
 *   0 max |cte0|   1 sum cte0^2   2 max |epsi0|   3 sum of speed [mph] at message times   4 min speed   5 progress in waypoints
 *   (sum of the signed cyclic difference of k)   6 first step with |cte0| > cte_limit, or -1   7 steps whose status is not SUCCESS
 *   (cte0, epsi0: rows 4 and 5 of the state run() hands to the solve; a not-a-number never wins a maximum or minimum)
 * hist [steps][MPC_DRIVE_REC][ld] or NULL, per step and car, as doubles:
 *   0..5 the car at message time   6, 7 cmd   8, 9 cte0, epsi0   10, 11 status, iterations   12 k
 * status [ld]: worst (largest) code over the steps; iters [ld] or NULL: iterations summed -- the conventions of the rollouts.
 * Containment: what the telemetry entry points owe a car no caller should send (not-a-number, a negative speed, a position far from
 *   the track) holds at every step: a status, a launch that ends, and every other car bit for bit as in a batch without it.
 *
 * mpc_drive_opts_default needs no device: npts 6, h 0.01, sub_old = round(latency_ms / 10), sub_new = 2 if latency_ms is non-zero and
 *   10 otherwise, warm_start 0, extra_latency 0, cte_limit 3.  opts = NULL: these defaults for the handle's parameters; warm_opts = NULL:
 *   those of mpc_warm_opts_default (read only with warm_start).
 * Refusals.  MPC_ERR_INVALID with a message: a wrong `size`, steps < 1, npts outside 3..8, n_track outside npts..MPC_DRIVE_MAX_TRACK, a
 *   sub count below 0, sub_old + sub_new outside 1..1000, h not finite or <= 0, ld < B, a NULL among car / track / summary / status,
 *   an MPC_PRECISION_F32 handle.  warm_start with max_soc > 0: MPC_ERR_UNSUPPORTED, as for every warm call.
 * mpc_drive_batch_device enqueues steps x (window kernel, the handler's three launches, plant-and-summary kernel) on `stream`: every
 *   step lasts as long as its slowest car.
 * mpc_drive_batch_device_fused: the same arguments, ONE launch: a lane keeps its car for all `steps` messages and starts the next
 *   message as soon as its own is done.  Every array the call writes (car, summary, hist, status, iters) holds BITWISE what the stepwise
 *   call writes.  The one launch serves the handles and sizes of mpc_rollout_batch_device_fused -- a single-phase fp64 lane-kernel
 *   solve (no fp32 start), max_soc = 0, B above the wave limit; everywhere else the call runs the stepwise loop itself.
 * mpc_drive_batch_host: the stepwise loop for host arrays (track included), on the handle's own device and stream; synchronises.
 * mpc_drive_info: out2[0] = calls so far that ran the one launch, out2[1] = calls that ran the stepwise loop.
 *
 * ---- per-car model values: mpc_drive_*_model ---------------------------------------------------------------------------------------
 * How fast can this tuning go round the track, and which limits make it leave the road?  One call, one car per value.  Each _model
 * form is the one without plus `model` directly behind `weights` (the rule of mpc_amd.h for _model forms): [MPC_NMODEL][ld] doubles
 * addressed with the call's ld, rows MPC_MODEL_* (dt, Lf, max_steering, max_acceleration, max_deceleration, max_speed); the host form
 * takes a host array and copies it in with the other inputs.
 * model == NULL: the call IS the entry point without _model -- bitwise, with all of its conventions, dispatch and refusals.
 * model != NULL: car i is driven with its own column in three places.
 *   Handler: the call mpc_telemetry_batch_device_model makes (or, with warm_start, mpc_telemetry_batch_device_warm_model) on (car,
 *     window, extra_latency, model), plus `weights`: the six values in the solve, max_speed in the cap of the speed tables and the
 *     throttle's `keep` term, max_steering in the normalisation of the reply, Lf in the latency compensation, the two acceleration
 *     limits in computeThrottle; warm: a record is judged against the car's own relaxed box.  Dispatch is the handler's: the wave
 *     kernel's MODEL build up to wave_max_batch, the lane kernel's MODEL build above it, the same bits from both.
 *   Plant, both uses: psi += steer * dist / Lf_i, and the reply takes effect as (cmd_steer * max_steering_i, cmd_throttle) -- cmd_steer
 *     was normalised by that same max_steering_i, so the angle in force is the angle the solve chose.
 *   Unchanged: the window rule, the summary and record rows, the status and iteration conventions, MpcDriveOpts.  sub_old, sub_new and h
 *     stay the call's here (per-car latency and substep counts: the _latency forms below; per-car horizon: the _horizon forms at
 *     the end).
 * A column that cannot be used (the _model rule: a value that is not finite, dt <= 0, Lf <= 0, max_steering <= 0, max_speed <= 0,
 *   max_acceleration <= 0, max_deceleration >= 0): the handle's values take its place in the handler's pre- and post-processing and in
 *   the plant, every step of that car ends MPC_STATUS_INFEASIBLE, car / summary / hist hold no not-a-number because of it, and every
 *   other car is bit for bit what it is in a batch without the defect.  The same holds for a car faster than its own relaxed speed limit.
 * Handles: the model rule -- every fp64 handle, also one whose ordinary solve starts in fp32 (served on its fp64 workspace, bitwise a
 *   handle created with f64_f32_start = 0).  An MPC_PRECISION_F32 handle: MPC_ERR_INVALID (per-instance model values: fp64 handles
 *   only), checked first; then every refusal above, unchanged.  warm_start with max_soc > 0: MPC_ERR_UNSUPPORTED.
 * mpc_drive_batch_device_fused_model writes BITWISE what mpc_drive_batch_device_model writes.  It runs the one launch where the
 *   stepwise model loop would launch the lane kernel's MODEL build at every step -- B above the wave limit (wave_max_batch < 0: every
 *   B), max_soc = 0 -- on every fp64 handle: one more case than the form without _model serves, because a model solve is never the
 *   two-launch fp32-start solve.  Everywhere else it runs the stepwise loop itself; mpc_drive_info counts both kinds.
 *
 * ---- per-car latency: mpc_drive_*_latency and mpc_telemetry_batch_*_latency ----------------------------------------------------------
 * How much actuator delay does this tuning survive, and what happens when the delay the handler compensates is not the delay the car
 * has?  Stale command time x compensated time is a 2-D grid; it is the columns of one call.  This replaces the reference's `-latency N`
 * run N times (and config-no-latency.json: comp = 0).
 * Telemetry handler.  mpc_telemetry_batch_device_latency / _host_latency have the arguments of the _warm_model forms plus `comp`, [ld]
 *   doubles (host form: a host array), directly behind extra_latency; model and the warm arguments may be NULL, as there.
 *   comp == NULL: the call IS the _warm_model form -- bitwise, the same dispatch and refusals.
 *   comp != NULL: instance i compensates for comp[i] seconds: Vehicle::move over comp[i] if comp[i] > 0, and no move at comp[i] == 0 (the
 *     reference's `if (Config::latency)` not taken).  MpcParams.latency_ms, MpcParams.lookahead and extra_latency are not read for it.
 *     A value that cannot be used -- not finite, or below 0 -- : the instance is handled exactly as one whose speedometer reading is
 *     negative: the speed handed on is not-a-number, the instance ends with the status that path produces, nothing else in the batch
 *     changes.  Everything else is the _warm_model form's: fp64 handles only, no warm with max_soc > 0, the wave kernels up to
 *     wave_max_batch and the lane kernel above it.
 * Drive.  Each _latency form is the _model form plus `latency` directly behind `model`: [MPC_NLATENCY][ld] doubles addressed with the
 *   call's ld (host form: a host array, copied in with the other inputs), rows
 *     MPC_LATENCY_COMP     comp as above, for the handler call of every step
 *     MPC_LATENCY_SUB_OLD  sub_old of this car in the plant, a double holding an integer value
 *     MPC_LATENCY_SUB_NEW  sub_new of this car in the plant, likewise
 *   latency == NULL: the call IS the _model form, bitwise.
 *   latency != NULL: car i uses its column.  opts->extra_latency, sub_old and sub_new are still validated as above and are the fallback
 *     below; h, npts, cte_limit, the window rule, the summary and record rows, the status and iteration conventions are unchanged.
 *   A column that cannot be used -- a value that is not finite, comp < 0, a count that is no integer value or below 0, sub_old + sub_new
 *     outside 1..1000 -- : the handler treats the car as above, so it carries a status at every step; the plant moves it with the call's
 *     sub_old and sub_new; car / summary / hist hold no not-a-number because of it; every other car is bit for bit what it is without the
 *     defect.  No trip count comes from an unchecked double: a launch that ends.
 *   mpc_drive_batch_device_fused_latency writes BITWISE what mpc_drive_batch_device_latency writes, and runs the one launch under exactly
 *     the rule of _fused_model (model == NULL: the rule of the plain fused form); everywhere else it runs the stepwise loop.
 *     mpc_drive_info counts both.
 *
 * ---- per-car horizon: mpc_drive_*_horizon and mpc_telemetry_batch_*_horizon ----------------------------------------------------------
 * Which N x dt gets this tuning round the track, and how fast?  dt is a row of `model`; N is the column of these forms, so the whole
 * grid is the cars of one call, and a handler that serves connections with different horizons is one batch.  Each _horizon form is its
 * _latency form plus `horizon` directly behind `model` (the rule of mpc_amd_horizon.h for _horizon forms): [ld] int32 addressed by
 * instance; the host forms take a host array and copy it in with the other inputs.  `model`, `comp` / `latency`, `weights` and the warm
 * arguments may each be NULL as in the _latency forms; with model == NULL the handle's own six values are used.
 * horizon == NULL: the call IS the _latency form -- bitwise, with its dispatch (the wave kernels up to wave_max_batch), its refusals and
 *   its mpc_drive_info counts.
 * horizon != NULL: car i's solve is the solve mpc_solve_batch_device_warm_horizon runs for a column with horizon[i] = n: 8n - 2
 *   variables and 6n rows, as the reference poses them with Config::N = n.  Nothing else reads N: the window, the fit, the latency
 *   compensation, the speed tables, the reply, the plant, the summary and record rows are unchanged.
 *   Valid: 3 <= horizon[i] <= the handle's N.  Any other value follows the _horizon rule: that car's solve ends MPC_STATUS_INFEASIBLE at
 *   every step with the start point as its solution; the reply computed from it and the car moved under it hold no not-a-number, and
 *   every other car is bit for bit what it is without the defect.
 *   Warm start: the drive's buffer in the handle keeps the rows of the handle's N (mpc_warm_rows); car i reads and writes records
 *   0 .. n - 2 of its column, the run()-path psi projection applies to those records, step 1 is cold and a car whose previous step did
 *   not succeed starts cold.  The telemetry forms: warm_in / warm_out as for mpc_solve_batch_device_warm_horizon (an instance writes
 *   the records of its own stages only).
 *   Dispatch, as for every horizon call: the lane kernel's HORIZON build at every B -- no wave path, also for a batch of one, and no
 *   fp32 start.  The lanes of a wave differ in their number of stages, so a pass lasts as long as the LONGEST horizon among the wave's
 *   64 lanes: sort the cars by horizon, so that a wave holds one value, or a few neighbouring ones.  These builds are not staged, so
 *   a call whose horizons are all equal is slower than the _latency form on a handle created with that N, and one call over a sorted
 *   N x dt grid was measured about a tenth slower than one _fused_model call per N on handles created with those N, times summed
 *   (DESIGN.md section 6p.3 has the figures).  It is still the only way to mix horizons behind one handle and one handler.
 *   Refusals, checked before anything is touched: an MPC_PRECISION_F32 handle: MPC_ERR_INVALID (per-instance model values: fp64
 *   handles only); max_soc > 0 with a non-NULL horizon: MPC_ERR_UNSUPPORTED (a per-instance horizon is not available with the
 *   second-order correction); then every refusal of the _latency forms, unchanged.
 * mpc_drive_batch_device_fused_horizon writes BITWISE what mpc_drive_batch_device_horizon writes.  With a horizon it runs the one launch
 *   (the lane kernel's ROLL x MODEL x HORIZON x DRIVE builds, cold and warm: not staged, per-lane workspace rows, no lane compaction) at
 *   every B >= 1 on every fp64 handle with max_soc = 0 -- the rule of mpc_rollout_batch_device_fused_horizon, because a horizon call
 *   never takes the wave path or the fp32 start; mpc_drive_info counts it.  horizon == NULL: _fused_latency with that form's own rule.
 *
 * ---- per-car plant values: mpc_drive_*_plant -------------------------------------------------------------------------------------------
 * How wrong may the controller's model be before the car leaves the road?  Everything above varies the controller per car and moves
 * every car in the world that controller believes in.  These forms vary the world: wheelbase error, steering scale and bias,
 * acceleration error, a steady side force -- a robustness grid is the columns of one call.  Each _plant form is its _horizon form plus
 * `plant` directly behind `latency`: [MPC_NPLANT][ld] doubles addressed with the call's ld (host form: a host array, copied in with the
 * other inputs), rows
 *     MPC_PLANT_LF          Lf_p: the wheelbase value the car turns with [m]
 *     MPC_PLANT_STEER_GAIN  g: the actuator's scale, 1 = exact
 *     MPC_PLANT_STEER_BIAS  b: an offset of the steering angle [rad], in the simulator's sign like row 4 of car
 *     MPC_PLANT_ACCEL_GAIN  a: the handler's guess is 6
 *     MPC_PLANT_DRAG_SPEED  d: the handler's guess is 50 [m/s]
 *     MPC_PLANT_DRIFT       w: a steady speed to the car's left [m/s]
 *   There is no telemetry form: the handler reads nothing of the plant.
 * plant == NULL: the call IS the _horizon form -- bitwise, with its dispatch, its refusals and its mpc_drive_info counts.
 * plant != NULL: car i is moved with its column.  One substep of length h:
 *     v = speed * 1609.34 / 3600     steer = -(steering_angle * g + b)     accel = (throttle - v / d) * a     dist = v * h
 *     x += dist * cos(psi) - (w * h) * sin(psi)     y += dist * sin(psi) + (w * h) * cos(psi)     psi += steer * dist / Lf_p
 *     speed = (v + accel * h) * 3600 / 1609.34
 *   The handler is untouched: it believes its own `model` (or the handle), compensates with its own Lf, and is told the angle it asked
 *   for -- rows 4 and 5 of car and of hist stay the commanded values (cmd_steer * max_steering_i, cmd_throttle), the controller's
 *   normalisation; g models the actuator's scale error.  Unchanged: the window, the summary and record rows, sub_old / sub_new (the
 *   call's or the latency column's), the warm rule, the dispatch, the mpc_drive_info counts.
 *   mpc_drive_plant_default needs no device: col6 = {p->Lf, 1, 0, 6, 50, 0}, the column under which the plant is the one above, bit for
 *   bit; a caller with a `model` array sets row 0 to the car's own Lf.
 *   A column that cannot be used -- a value that is not finite, Lf_p <= 0, d <= 0 -- : the car is moved with the default column (its Lf
 *   row: the car's own Lf, the model's or the handle's), and every step of it that the handler ended SUCCESS or ACCEPTABLE is
 *   MPC_STATUS_INFEASIBLE in hist row 10, summary row 7 and the folded status (any other status of the handler stays).  The handler's
 *   own status, which decides whether the car's next step starts warm, is not touched, and neither are the iterations.  car / summary /
 *   hist hold no not-a-number because of it; every other car is bit for bit what it is without the defect.
 *   Refusals: with plant != NULL an MPC_PRECISION_F32 handle is refused first (track driving: fp64 handles only); then those of the
 *   _horizon forms, unchanged.
 *   mpc_drive_batch_device_fused_plant writes BITWISE what mpc_drive_batch_device_plant writes and runs the one launch exactly where
 *   _fused_horizon would with the same other arguments: the column is one more pointer of the builds that exist, read by instance index
 *   at the hand-over only. */
#define MPC_DRIVE_MAX_TRACK 4096
#define MPC_DRIVE_NSUM 8
#define MPC_DRIVE_REC 13
enum { MPC_DRIVE_SUM_MAX_CTE = 0, MPC_DRIVE_SUM_CTE2, MPC_DRIVE_SUM_MAX_EPSI, MPC_DRIVE_SUM_SPEED, MPC_DRIVE_SUM_MIN_SPEED,
       MPC_DRIVE_SUM_PROGRESS, MPC_DRIVE_SUM_FIRST_OFF, MPC_DRIVE_SUM_FAILED };
enum { MPC_DRIVE_REC_CAR = 0, MPC_DRIVE_REC_CMD = 6, MPC_DRIVE_REC_CTE = 8, MPC_DRIVE_REC_EPSI = 9, MPC_DRIVE_REC_STATUS = 10,
       MPC_DRIVE_REC_ITERS = 11, MPC_DRIVE_REC_K = 12 };
#define MPC_NLATENCY 3
enum { MPC_LATENCY_COMP = 0, MPC_LATENCY_SUB_OLD = 1, MPC_LATENCY_SUB_NEW = 2 };
#define MPC_NPLANT 6
enum { MPC_PLANT_LF = 0, MPC_PLANT_STEER_GAIN, MPC_PLANT_STEER_BIAS, MPC_PLANT_ACCEL_GAIN, MPC_PLANT_DRAG_SPEED, MPC_PLANT_DRIFT };

typedef struct MpcDriveOpts {
  int32_t size;            /* sizeof(MpcDriveOpts) */
  int32_t npts;            /* waypoints per window, 3..8 */
  int32_t sub_old;         /* plant substeps under the command in force before the reply takes effect */
  int32_t sub_new;         /* ... and under the reply */
  int32_t warm_start;      /* 0: every step cold; else the _warm handler from step 2 on */
  int32_t reserved;
  double h;                /* length of a plant substep [s] */
  double extra_latency;    /* as for mpc_telemetry_batch_device */
  double cte_limit;        /* summary row 6 */
} MpcDriveOpts;

int mpc_drive_opts_default(const MpcParams *p, MpcDriveOpts *o);
int mpc_drive_batch_device(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                           int n_track, const double *weights, const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary,
                           double *hist, int32_t *status, int32_t *iters, void *stream);
int mpc_drive_batch_device_fused(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                                 int n_track, const double *weights, const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary,
                                 double *hist, int32_t *status, int32_t *iters, void *stream);
int mpc_drive_batch_host(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                         int n_track, const double *weights, const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary,
                         double *hist, int32_t *status, int32_t *iters);
int mpc_drive_batch_device_model(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                                 int n_track, const double *weights, const double *model, const MpcDriveOpts *opts,
                                 const MpcWarmOpts *warm_opts, double *summary, double *hist, int32_t *status, int32_t *iters, void *stream);
int mpc_drive_batch_device_fused_model(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x,
                                       const double *track_y, int n_track, const double *weights, const double *model,
                                       const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary, double *hist, int32_t *status,
                                       int32_t *iters, void *stream);
int mpc_drive_batch_host_model(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                               int n_track, const double *weights, const double *model, const MpcDriveOpts *opts,
                               const MpcWarmOpts *warm_opts, double *summary, double *hist, int32_t *status, int32_t *iters);
int mpc_drive_batch_device_latency(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                                   int n_track, const double *weights, const double *model, const double *latency, const MpcDriveOpts *opts,
                                   const MpcWarmOpts *warm_opts, double *summary, double *hist, int32_t *status, int32_t *iters, void *stream);
int mpc_drive_batch_device_fused_latency(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x,
                                         const double *track_y, int n_track, const double *weights, const double *model,
                                         const double *latency, const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary,
                                         double *hist, int32_t *status, int32_t *iters, void *stream);
int mpc_drive_batch_host_latency(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                                 int n_track, const double *weights, const double *model, const double *latency, const MpcDriveOpts *opts,
                                 const MpcWarmOpts *warm_opts, double *summary, double *hist, int32_t *status, int32_t *iters);
/* (declared here, not beside the other telemetry forms: they take what the drive's row MPC_LATENCY_COMP holds) */
int mpc_telemetry_batch_device_latency(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                                       const double *comp, double *ptsx, double *ptsy, const double *model, const double *warm_in,
                                       const int32_t *warm_status, double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts, double *cmd,
                                       double *out8, int32_t *status, void *stream);
int mpc_telemetry_batch_host_latency(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                                     const double *comp, const double *ptsx, const double *ptsy, const double *model, const double *warm_in,
                                     const int32_t *warm_status, double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts, double *cmd,
                                     int32_t *status);
int mpc_drive_batch_device_horizon(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                                   int n_track, const double *weights, const double *model, const int32_t *horizon, const double *latency,
                                   const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary, double *hist, int32_t *status,
                                   int32_t *iters, void *stream);
int mpc_drive_batch_device_fused_horizon(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x,
                                         const double *track_y, int n_track, const double *weights, const double *model,
                                         const int32_t *horizon, const double *latency, const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts,
                                         double *summary, double *hist, int32_t *status, int32_t *iters, void *stream);
int mpc_drive_batch_host_horizon(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                                 int n_track, const double *weights, const double *model, const int32_t *horizon, const double *latency,
                                 const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary, double *hist, int32_t *status,
                                 int32_t *iters);
int mpc_telemetry_batch_device_horizon(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                                       const double *comp, double *ptsx, double *ptsy, const double *model, const int32_t *horizon,
                                       const double *warm_in, const int32_t *warm_status, double *warm_out, int64_t ld_warm,
                                       const MpcWarmOpts *opts, double *cmd, double *out8, int32_t *status, void *stream);
int mpc_telemetry_batch_host_horizon(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                                     const double *comp, const double *ptsx, const double *ptsy, const double *model, const int32_t *horizon,
                                     const double *warm_in, const int32_t *warm_status, double *warm_out, int64_t ld_warm,
                                     const MpcWarmOpts *opts, double *cmd, int32_t *status);
int mpc_drive_plant_default(const MpcParams *p, double *col6);
int mpc_drive_batch_device_plant(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                                 int n_track, const double *weights, const double *model, const int32_t *horizon, const double *latency,
                                 const double *plant, const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary, double *hist,
                                 int32_t *status, int32_t *iters, void *stream);
int mpc_drive_batch_device_fused_plant(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x,
                                       const double *track_y, int n_track, const double *weights, const double *model,
                                       const int32_t *horizon, const double *latency, const double *plant, const MpcDriveOpts *opts,
                                       const MpcWarmOpts *warm_opts, double *summary, double *hist, int32_t *status, int32_t *iters,
                                       void *stream);
int mpc_drive_batch_host_plant(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                               int n_track, const double *weights, const double *model, const int32_t *horizon, const double *latency,
                               const double *plant, const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary, double *hist,
                               int32_t *status, int32_t *iters);
int mpc_drive_info(const MpcHandle *h, int64_t *out2);

#endif /* MPC_AMD_DRIVE_H */
