/*
 * mpc_amd.h -- C ABI of the MI355X-native batched MPC solver.
 *
 * This is the drop-in boundary for ONE path of dr-tony-lin/CarND-MPC-Project:
 * MPC::solve() + FG_eval (src/control/MPC.cpp:14-155, 183-325), i.e. the call
 *     CppAD::ipopt::solve<Dvector, FG_eval>(options, vars, vars_lowerbound,
 *         vars_upperbound, constraints_lowerbound, constraints_upperbound,
 *         fg_eval, solution);                      // MPC.cpp:290-292
 * together with the set-up before it (MPC.cpp:204-281) and the unpacking after
 * it (MPC.cpp:306-324), for B independent problem instances at once.
 *
 * Plain pointers and sizes only; no C++/torch types; no exceptions cross this
 * boundary (integer return codes + a per-instance status array, mirroring the
 * reference's "print and still return solution.x" behaviour, MPC.cpp:295-303).
 * There is no CPU fallback: every entry point that computes needs a gfx950
 * device and fails with MPC_ERR_NO_DEVICE / MPC_ERR_HIP otherwise.
 *
 * Batch layout is struct-of-arrays ("quantity-major", like the reference's own
 * decision vector, MPC.cpp:56-63): element (q, i) of an array with Q rows is at
 * [q * ld + i], ld >= B, so that consecutive instances are consecutive in
 * memory and a wavefront's loads coalesce.
 */
#ifndef MPC_AMD_H
#define MPC_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPC_ABI_VERSION 5
#define MPC_MAX_TABLE 16
#define MPC_NW 12      /* Config::weights entries read by FG_eval (Config.h:14-61) */
#define MPC_NCOEF 5    /* road polynomial, zero padded: fit order is 2..4 (RoadGeometry.cpp:26-34) */
#define MPC_NSTATE 6   /* x, y, psi, v, cte, epsi (MPC.cpp:213-218) */
#define MPC_NOUT 9     /* x1,y1,psi1,v1,cte1,epsi1,delta0,a0,cost (MPC.cpp:322-324) */
#define MPC_MAX_N 64   /* largest horizon the kernels are sized for */
#define MPC_MAX_SOC 16 /* largest MpcParams.max_soc */
#define MPC_NMODEL 6   /* model values an instance may bring along (the mpc_*_model entry points) */
enum { MPC_MODEL_DT = 0, MPC_MODEL_LF, MPC_MODEL_MAX_STEERING, MPC_MODEL_MAX_ACCELERATION,
       MPC_MODEL_MAX_DECELERATION, MPC_MODEL_MAX_SPEED };      /* rows of model [6][ld], units of MpcParams */

/* return codes */
enum {
  MPC_OK = 0,
  MPC_ERR_INVALID = -1,     /* bad argument (NULL, N out of range, ld < B ...) */
  MPC_ERR_NO_DEVICE = -2,   /* no gfx950 device / HIP runtime unavailable */
  MPC_ERR_HIP = -3,         /* a HIP call failed; see mpc_last_error() */
  MPC_ERR_UNSUPPORTED = -4, /* e.g. branch_mode LIVE, or run() with max_fit_order > 5 */
  MPC_ERR_IO = -5           /* config file unreadable / malformed */
};

/* per-instance status, modelled on CppAD::ipopt::solve_result<>::status_type
 * (MPC.cpp:295): 0 is the only value the reference treats as "ok". */
enum {
  MPC_STATUS_SUCCESS = 0,
  MPC_STATUS_MAXITER = 1,
  MPC_STATUS_LINESEARCH = 2,   /* step length fell below alpha_min (IPOPT: restoration) */
  MPC_STATUS_INFEASIBLE = 3,   /* initial state outside its own bounds (MPC.cpp:229-239 vs :269-281) */
  MPC_STATUS_NUMERIC = 4,      /* NaN/Inf met */
  MPC_STATUS_PENDING = 5,      /* deferred tails only: handed to the tail queue, final after mpc_tail_wait */
  MPC_STATUS_ACCEPTABLE = 6    /* IPOPT's STOP_AT_ACCEPTABLE_POINT = CppAD's stop_at_acceptable_point, which MPC.cpp:295-303 prints
                                * ("Ipopt failed with ...") and returns like every other non-success: acceptable_iter iterates in
                                * a row within the acceptable_* tolerances, or a line search that ran out of step length at such
                                * a point */
};

enum { MPC_BRANCH_FROZEN = 0, MPC_BRANCH_LIVE = 1 };
enum { MPC_F32_START_OFF = 0, MPC_F32_START_ON = 1, MPC_F32_START_AUTO = 2 };   /* MpcParams.f64_f32_start */
#define MPC_F32_START_AUTO_N 15
enum { MPC_PRECISION_F64 = 0, MPC_PRECISION_F32 = 1 };
enum { MPC_TAIL_OFF = 0, MPC_TAIL_AUTO = -1 };   /* MpcParams.tail_cut */
enum { MPC_LANE_COMPACT_AUTO = -1 };             /* MpcParams.lane_compact */

/* Everything the reference reads from `struct Config` statics on this path
 * (src/utils/Config.h:66-177) AFTER Config::load() has applied its unit
 * conversions and table rescaling (src/utils/Config.cpp:31-87).  Passed by
 * value per batch: no global state, unlike the reference's mutable Config. */
typedef struct MpcParams {
  int32_t abi_version;       /* MPC_ABI_VERSION */
  int32_t N;                 /* Config::N,  3..MPC_MAX_N */
  double dt;                 /* Config::dt */
  double Lf;                 /* Config::Lf */
  double weights[MPC_NW];    /* Config::weights[0..11] */
  double cte_panic;          /* Config::ctePanic */
  double epsi_panic;         /* Config::epsiPanic */
  double max_steering;       /* rad  (bounds, MPC.cpp:248-251) */
  double max_acceleration;   /* m/s2 (MPC.cpp:254-257) */
  double max_deceleration;   /* m/s2, negative */
  double max_speed;          /* m/s  (MPC.cpp:236-239) */
  int32_t n_steers, n_steer_speeds;          /* Vehicle::computeSpeedTarget tables */
  double steers[MPC_MAX_TABLE];
  double steer_speeds[MPC_MAX_TABLE];
  /* used only by the run() pre/post-processing entry points */
  int32_t n_yaw_changes, n_yaw_change_speeds;
  double yaw_changes[MPC_MAX_TABLE];
  double yaw_change_speeds[MPC_MAX_TABLE];
  int32_t max_fit_order;     /* Config::maxFitOrder */
  int32_t latency_ms;        /* Config::latency */
  double max_fit_error;      /* Config::maxFitError */
  double lookahead;          /* Config::lookahead = latency * 1e-3 */
  double steer_adj_thresh;   /* Config::steerAdjustmentThresh */
  double steer_adj_ratio;    /* Config::steerAdjustmentRatio (clamped to [0,0.1]) */
  double ipopt_timeout;      /* Config::ipoptTimeout: carried, not read -- the deadline is a per-instance iteration budget, mpc_amd_budget.h */
  /* solver controls (the reference's IPOPT option string, MPC.cpp:160-179, plus
   * the IPOPT defaults it leaves untouched) */
  int32_t branch_mode;       /* MPC_BRANCH_FROZEN: CppAD tape recorded once at the start point */
  int32_t precision;         /* MPC_PRECISION_F64 (default), or MPC_PRECISION_F32: see mpc_solve_batch_device_f32 */
  int32_t max_iter;          /* IPOPT default 3000; default here 200 */
  int32_t pass_cut;          /* multi-phase solve: park instances still running after this many passes and finish them,
                              * re-packed into dense waves, in a further launch (0 = single launch, the default; more
                              * cuts in pass_cut_next; results are bitwise the same) */
  double tol;                /* IPOPT "tol", default 1e-8 */
  /* Termination polish (default on).  IPOPT stops at the FIRST iterate whose scaled optimality error is <= tol
   * (MPC.cpp:290-292 leaves that default untouched).  An output that the objective determines only weakly -- an
   * interior a0: the frozen tape has no a^2 term -- then still moves by up to ~1e-4 per Newton step, so two correct
   * solvers that stop one iterate apart differ by that much.  With polish != 0 an instance is converged when
   * E_0 <= tol AND the barrier parameter has reached its floor (tol/10) AND the last accepted step moved
   * (delta0, a0) by at most out_step_tol and every primal variable (the predicted trajectory, whose far end is the
   * least determined part) by at most out_step_tol / 0.03 = 1e-5: the returned point is then the central-path point IPOPT is converging
   * to, reproducible to ~1e-7 whatever the linear algebra (and a barrier parameter within 3x of the floor goes
   * to the floor directly).  Cost: +0.4 iterations per solve.  polish = 0 is IPOPT's own stopping rule. */
  double out_step_tol;       /* default 3e-7 (rad, m/s^2): leaves delta0 within 7e-8 and a0 within 2e-8 of the limit point */
  double tol_f32;            /* "tol" of the fp32 solver, default 5e-4 (barrier floor tol_f32/25 = 2e-5, polish step 0.6 tol_f32,
                              * line search failing inside 10 x tol_f32 = solved): where the fp32 phase of an F32 handle
                              * hands over at the latest, and the stopping rule of the pure fp32 mode (f32_finish = 0) */
  int32_t polish;            /* default 1 */
  int32_t pass_cut_next[3];  /* further cuts (passes counted from the previous cut; a zero ends the list), e.g.
                              * pass_cut 16, next {16, 32, 0}: four launches (0.3x the wave passes of a heavy-tailed
                              * batch; measured: no gain in time per batch) */
  /* IPOPT defaults the reference's option string (MPC.cpp:160-179) leaves untouched and that shape the answer when a
   * solve starts on a bound (closed loops, test.cpp:79-111): every finite variable bound is relaxed by
   * bound_relax_factor * max(1, |bound|) before the solve, and the returned point is projected back into the caller's
   * bounds (honor_original_bounds = yes in IPOPT 3.12). */
  int32_t honor_original_bounds;   /* default 1 */
  double bound_relax_factor;       /* default 1e-8 */
  /* Deferred tails: a launch lasts as long as its slowest instance.  With tail_cut > 0 an instance that
   * is still running after tail_cut passes is handed to the handle's tail queue (status MPC_STATUS_PENDING) and the
   * launch ends; the queue is worked off by short tail slices on the handle's own tail stream while later batches run.
   * mpc_tail_wait / mpc_tail_poll / mpc_tail_stream_wait mark a batch final.  Results are bitwise those of the single launch. */
  int32_t tail_cut;                /* default 0 = off; MPC_TAIL_AUTO (-1): the handle's own choice (from 20 passes up to N = 12, 24 beyond; it moves
                                    * the cut out while more than 8 % of a batch are handed over; results do not depend on the cut) */
  int32_t tail_ring;               /* batches whose tails may be outstanding at once (2..512), default 128: a batch is final
                                    * only when its slowest straggler is, tens of milliseconds behind its launch */
  int64_t tail_capacity;           /* deferred instances per batch; 0 = max_batch / 8.  A batch with more keeps the rest in its launch */
  /* Mixed precision across phases.  MPC_PRECISION_F32 handles: f32_finish = 1 (default) runs the interior-point
   * iteration in fp32 until its barrier parameter has reached mixed_switch_mu and finishes every instance in fp64
   * (same state machine, tol instead of tol_f32, termination polish), fp32 at the ABI; 0 = the pure fp32 solver.
   * MPC_PRECISION_F64 handles: f64_f32_start = 1 runs the same early iterations on the fp32 record (half the
   * workspace bytes) before the fp64 solve takes over; MPC_F32_START_AUTO (2) does so for horizons of
   * N >= MPC_F32_START_AUTO_N steps, where a full device's workspace no longer lives in the Infinity Cache and the bytes
   * count in full.  The fp64 phase runs to tol and the polish.  Only a CLEAN hand-over is continued (the fp32 phase
   * reached mixed_switch_mu or tol_f32 within 16 iterations); an instance that uses the allowance up or leaves the fp32
   * phase out of trouble (line search, inertia correction, not-a-number) is solved in fp64 from the start point, and
   * so is one the fp64 phase cannot finish from the fp32 iterate: on hard instances fp32 iterates lead into other
   * local minima than fp64 ones.  With that rule the CPU build gives the single-phase solve's status and point (1e-7)
   * on every instance of SURVEY's unfiltered populations (65 536 at N = 10, 32 768 at N = 25).
   * Default MPC_F32_START_AUTO: long horizons start on the fp32 record.  (Launches of at most wave_max_batch instances do not go
   * through the two-launch solve at all: they run one instance per wavefront, every iteration in fp64 -- DESIGN.md section 6d.)  Measured in round 4 with the tail slices on the
   * tail stream's high priority (windows of 600 batches): N = 25, SURVEY's population 9.8-10.0 M against 7.1-8.8 M solves/s,
   * the filtered generator 11.0-11.9 against 7.6 M; 0 status differences and at most 4.1e-8 rad on the first steering
   * angle over the 32 768 instances of SURVEY's N = 25 population (profiles/r04_f32start_vs_plain.jsonl).  Not for short
   * horizons: at N = 10 the workspace of a full device lives in the Infinity Cache and the two launches of the mixed
   * solve cost more than the bytes save (44 against 52 M on the filtered headline): f64_f32_start = 1 stays a choice.
   * MPC_F32_START_OFF gives the single-phase fp64 solve at every horizon (bitwise the host twin's).
   * Reproducibility across batch sizes: with the default AUTO and N >= MPC_F32_START_AUTO_N the BITS of an instance's result depend
   * on the size of the launch it is part of -- up to wave_max_batch (1 024) instances every iteration runs in fp64, a larger launch
   * starts in fp32 -- while status and values agree within the fp64 tolerances (1e-6 rad / m/s^2 on the first actuation, 1e-5 m on
   * the step-1 state and the trajectory, 1e-7 relative on the cost).  Identical bits whatever the batch size need
   * f64_f32_start = MPC_F32_START_OFF (tests/test_f32_horizons_gpu.py asserts both). */
  int32_t f32_finish;
  int32_t f64_f32_start;
  double mixed_switch_mu;          /* default 2e-5 */
  /* Lane compaction.  Memory is fetched in 128-byte lines = the 16-byte groups of 8 neighbouring lanes, so a
   * line is fetched as long as one of its 8 lanes still runs.  With lane_compact = g > 0 a wave whose running lanes are
   * spread over g more 8-lane groups than they need moves the ones outside its fullest groups into free lanes inside
   * them (launches of at least 8 192 instances, single-lane arithmetic unchanged: results are bitwise the same).
   * Default MPC_LANE_COMPACT_AUTO: 2, and 1 for horizons of N >= 15, whose workspace (>= 360 KB per wave) is in HBM proper, where
   * every line not fetched counts (configs[3] share: 6.90 -> 7.26 M solves/s); 0 = off. */
  int32_t lane_compact;
  /* Mixed precision, heavy-tailed workloads (weight sweeps: some instances spend the whole allowance of the fp32 phase
   * while most are handed over after 8-12 iterations).  With f32_phase_refill = 1 a lane of the fp32 phase hands its
   * instance over through a buffer of its own instead of keeping the iterate in its workspace column, so the lane is
   * free: it takes further instances while the launch has any, and its column is there for lane compaction.  Same
   * results bit for bit.  Measured: +12-20 % on the weight sweeps of configs[4], -6...-15 % where every instance needs
   * about the same number of iterations (the copy, and late refills that prolong a wave for a few lanes).  Default 0. */
  int32_t f32_phase_refill;
  /* IPOPT's termination tests beyond `tol` (OptimalityErrorConvergenceCheck; all defaults of IPOPT 3.12 that the reference's
   * option string MPC.cpp:160-179 leaves alone).  Converged = scaled error <= tol AND unscaled dual infeasibility <=
   * dual_inf_tol, constraint violation <= constr_viol_tol, complementarity <= compl_inf_tol.  Acceptable = the same with
   * acceptable_tol and the acceptable_* values; acceptable_iter acceptable iterates in a row, or a failed line search at an
   * acceptable point, end the solve with MPC_STATUS_ACCEPTABLE; a line search that fails at an almost feasible point
   * (constraint violation <= 1e-2 tol) is final without the restart that stands in for IPOPT's restoration phase (IPOPT does
   * not try it there).  acceptable_iter = 0 switches the acceptable-level machinery off (IPOPT's meaning of 0).  fp64 solver
   * only: the fp32 phases stop by tol_f32. */
  int32_t acceptable_iter;         /* default 15 */
  double dual_inf_tol;             /* default 1 */
  double constr_viol_tol;          /* default 1e-4 */
  double compl_inf_tol;            /* default 1e-4 */
  double acceptable_tol;           /* default 1e-6 */
  double acceptable_dual_inf_tol;  /* default 1e10 */
  double acceptable_constr_viol_tol;   /* default 1e-2 */
  double acceptable_compl_inf_tol;     /* default 1e-2 */
  /* IPOPT's error measure in full.  The reference's NLP keeps the initial state as six VARIABLES pinned by six equality rows
   * (MPC.cpp:116-121, 269-281).  Those rows' multipliers and the bound duals of psi_0 / v_0 decouple from the Newton step, so
   * the device solver does not need them for its iterates -- but IPOPT counts the residuals of the six variables' stationarity
   * rows in the dual infeasibility (non-zero after a step the fraction-to-the-boundary rule has cut), their multipliers in its
   * scaling and the two variables' duals in the complementarity and in the dual step length.  1: carried and counted -- the
   * solver then takes the oracle's iteration count on 98.5-99.2 % of a batch instead of 94-96 % (what is left is the last
   * step's rounding) at ~4 % of the rate (ten more fields per instance and sweep).  0 (default): not carried; the barrier
   * parameter then comes down one iteration early on a few per cent of the instances.  Same solution either way. */
  int32_t initial_state_rows;
  /* Launches of at most this many instances run ONE INSTANCE PER WAVEFRONT -- or per 16 / 32 neighbouring lanes of one, a lane
   * per stage (mpc_solve_wave_kernel): the instance's N-step variables in LDS, its stages shared between
   * the lanes, bitwise the results of the lane-per-instance kernel.  A latency mapping: one MPC::solve() 0.30 instead of 0.68 ms,
   * a launch of 1 024 instances 0.55 instead of 1.21 ms, of 4 096 (N <= 17) 0.74 instead of 1.51 ms, level at ~10 000; it spends
   * a SIMD per 1-4 instances, so many launches in flight are better off with the lane kernel.  0 (default) = 1 024; < 0 = never.
   * Not used by an explicit f64_f32_start = 1 or a mixed MPC_PRECISION_F32 handle (those ask for the two-launch solve). */
  int32_t wave_max_batch;
  /* IPOPT's second-order correction (max_soc, W&B A-5.5 .. A-5.10; IPOPT's default is 4, kappa_soc = 0.99): when the first
   * trial point of a line search is rejected and has not reduced the constraint violation, up to max_soc corrected directions
   * -- the same Newton system with the violation at the trial point folded into the residuals -- are tried before the step is
   * shortened.  Measured on SURVEY's hard N = 10 instances (oracle): 8 % fewer iterations, 10 of 29 failures solved.  0 (default)
   * = off, results bitwise those of ABI 4; 0..MPC_MAX_SOC.  fp64 solver only: an MPC_PRECISION_F32 solve ignores it, the fp64
   * finish of one with f32_finish and the fp64 phase of f64_f32_start honour it.  Launches with max_soc > 0 run builds of the
   * kernels that carry it (an extra buffer of 14 reals per stage and instance, allocated by the handle on first use). */
  int32_t max_soc;
} MpcParams;

typedef struct MpcHandle MpcHandle;

/* Aggregate statistics of the last batch (diagnostics for bench/tests). */
typedef struct MpcBatchStats {
  int64_t batch;
  int64_t n_success, n_maxiter, n_linesearch, n_infeasible, n_numeric, n_acceptable;
  int64_t iter_sum;          /* sum of interior-point iterations over the batch */
  int32_t iter_max;
  int32_t n_pending;         /* deferred tails: instances of the batch handed to the tail queue (their iterations are not in iter_sum yet) */
  double kernel_ms;          /* hipEvent time of the solve kernel, on its own stream */
} MpcBatchStats;

/* ---- parameters ---------------------------------------------------------- */
/* Compiled-in defaults of the reference, src/utils/Config.cpp:5-29. */
int mpc_params_default(MpcParams *p);
/* Config::load(fileName), src/utils/Config.cpp:31-87, same JSON keys. */
int mpc_params_load_json(const char *path, MpcParams *p);

/* ---- lifetime -------------------------------------------------------------- */
/* device < 0: current HIP device.  max_batch sizes the device workspace (3.7 KB per instance at N=10; 2.0 KB in fp32).
 * A handle owns its workspace and launch state: calls on one handle must be ordered (one stream at a time).
 * To keep several batches in flight -- which is how to fill the device, see DESIGN.md section 6b -- create one
 * handle per stream. */
int mpc_create(const MpcParams *p, int device, int64_t max_batch, MpcHandle **out);
/* (N, precision and the mixed-precision switches size the workspaces and cannot change on a live handle; with deferred tails
 * outstanding the call first lets them finish under the parameters their batches were issued with) */
int mpc_set_params(MpcHandle *h, const MpcParams *p);
void mpc_destroy(MpcHandle *h);
const char *mpc_last_error(void);
int mpc_abi_version(void);
int mpc_handle_device(const MpcHandle *h);   /* the device the handle's memory and launches live on */

/* ---- the hot path ---------------------------------------------------------- */
/*
 * Solve B instances; all pointers are DEVICE pointers (HBM resident):
 *   state  [6][ld]   initial state per instance            (MPC.cpp:213-218)
 *   coeffs [5][ld]   road polynomial c0..c4, zero padded   (RoadGeometry, MPC.cpp:151-152)
 *   yaw_lo [ld], yaw_hi [ld]   psi bounds = Config::yawLow/yawHigh as MPC::run
 *                    sets them just before solve()          (MPC.cpp:345-352, 229-232)
 *   weights[12][ld]  per-instance Config::weights, or NULL to use p->weights
 *   out    [9][ld]   the vector MPC::solve returns          (MPC.cpp:322-324)
 *   traj   [2N][ld]  x[0..N) then y[0..N) of the solution, or NULL (MPC.cpp:306-311)
 *   status [ld]      per-instance MPC_STATUS_*
 *   iters  [ld]      per-instance iteration count, or NULL
 * stream: the hipStream_t (as void*) to launch on; NULL is HIP's default (null)
 * stream.  The call is asynchronous with respect to the host: order later work
 * on the same stream, or synchronise that stream / the device, before reading.
 */
int mpc_solve_batch_device(MpcHandle *h, int64_t B, int64_t ld, const double *state,
                           const double *coeffs, const double *yaw_lo, const double *yaw_hi,
                           const double *weights, double *out, double *traj, int32_t *status,
                           int32_t *iters, void *stream);
/* MPC_PRECISION_F32 (BASELINE.json configs[4]: "fp32 mixed precision"): the same solve for a handle created with
 * params.precision = MPC_PRECISION_F32 -- fp32 inputs and outputs (136 B of algorithmic HBM traffic per solve with
 * per-instance weights and no trajectory).  Two modes:
 *   f32_finish = 1 (default)  fp32 interior-point iterations (Riccati sweeps and trigonometry in fp32; the road polynomial
 *       and f(x) - y in fp64; residuals as differences of neighbouring states first) until the barrier parameter is about to
 *       go below mixed_switch_mu, then EVERY instance is finished by the fp64 solver (same state machine, tol, polish).
 *       Against the fp64 path, on every instance (tests/test_f32.py, tolerances stated before measuring): |d delta0| <= 1e-3
 *       rad, |d a0| <= 1e-3 m/s^2, step-1 state <= 1e-3, trajectory <= 1e-2 m, same status.  Measured on a 131 072-instance
 *       weight sweep incl. velocity weight 0: delta0 max 5.5e-8, a0 max 1.0e-4, state max 5.5e-6 (the rounding of the fp32
 *       arrays), with ~1 instance in 50 000 converging to a neighbouring local minimum of equal cost (counted by the tests).
 *   f32_finish = 0            the pure fp32 solver: stops at tol_f32 (5e-4; barrier floor tol_f32 / 25 = 2e-5; a failed line
 *       search inside 10 x tol_f32 counts as solved), about twice the rate, measured against fp64 on 65 536 instances:
 *       delta0 max 2.4e-3 (p99 1.9e-4), a0 max 6.8e-2 when interior (p99.9 3.6e-4), state max 6.8e-3, trajectory max 0.12 m;
 *       velocity weight 0 and horizons beyond N = 10 are outside its specification.
 * An fp64 handle refuses this entry point and an fp32 handle refuses the double ones (MPC_ERR_INVALID); the run(),
 * telemetry and rollout entry points are fp64 only. */
int mpc_solve_batch_device_f32(MpcHandle *h, int64_t B, int64_t ld, const float *state,
                               const float *coeffs, const float *yaw_lo, const float *yaw_hi,
                               const float *weights, float *out, float *traj, int32_t *status,
                               int32_t *iters, void *stream);
/* Same as mpc_solve_batch_device, host pointers: one copy in, the launch, one copy out, synchronises. */
int mpc_solve_batch_host(MpcHandle *h, int64_t B, int64_t ld, const double *state,
                         const double *coeffs, const double *yaw_lo, const double *yaw_hi,
                         const double *weights, double *out, double *traj, int32_t *status,
                         int32_t *iters);
/* The same for an MPC_PRECISION_F32 handle (float arrays). */
int mpc_solve_batch_host_f32(MpcHandle *h, int64_t B, int64_t ld, const float *state,
                             const float *coeffs, const float *yaw_lo, const float *yaw_hi,
                             const float *weights, float *out, float *traj, int32_t *status,
                             int32_t *iters);
/* ---- the caller of the path: MPC::run() for a batch -------------
 * Pre-processing (waypoints to the vehicle frame, adaptive polynomial fit, cte0/epsi0, yaw bounds,
 * speed tables: src/control/MPC.cpp:329-356), the solve, and the post-processing (steering adjustment,
 * acceleration clamp, steering normalisation: MPC.cpp:360-381), all on the device:
 *   pose [6][ld]      x, y, psi, v, steering, acceleration of the (latency-compensated) vehicle
 *   ptsx, ptsy [npts][ld]  global waypoints in, VEHICLE-FRAME waypoints out (the reference transforms
 *                     them in place, mpc_main.cpp:189-190 relies on it); 3 <= npts <= 8
 *   out8 [8][ld]      {x1, y1, psi1, v1, steer in [-1,1], accel, cte1, epsi1} (MPC.cpp:381)
 *   traj [2N][ld] or NULL, status [ld], iters [ld] or NULL   as in mpc_solve_batch_device
 *   pre  [15][ld] or NULL  what run() handed to solve(): state[6], coeffs[5], yaw_lo, yaw_hi,
 *                     max_yaw_change, target_speed (diagnostic) */
int mpc_run_batch_device(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *pose, double *ptsx,
                         double *ptsy, double *out8, double *traj, int32_t *status, int32_t *iters,
                         double *pre, void *stream);
/* The same for host arrays (all of them; ptsx / ptsy in: global, out: vehicle frame): one copy in, the kernels, one copy out, on the
 * handle's own device and stream; synchronises.  B = 1 is MPC::run() itself (include/mpc_drop_in.hpp delegates to it). */
int mpc_run_batch_host(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *pose, double *ptsx, double *ptsy,
                       double *out8, double *traj, int32_t *status, int32_t *iters, double *pre);
/* The telemetry handler around run() (src/mpc_main.cpp:126-159, 171-174):
 *   tel [6][ld]   x, y, psi [rad], speed [mph], steering_angle (simulator sign), previous throttle command
 *   extra_latency seconds added to Config::lookahead (the handler's mean solve time, mpc_main.cpp:158)
 *   ptsx, ptsy    as in mpc_run_batch_device (in: global, out: vehicle frame)
 *   cmd [2][ld]   steering_angle and throttle of the reply (mpc_main.cpp:183-184)
 *   out8 [8][ld] or NULL   run()'s own return vector
 * What run() and the handler owe an instance whose inputs no caller should send -- every mpc_run_batch_* and mpc_telemetry_batch_*
 * entry point, their _warm, _model and _host forms, the wire forms, MPC::run() of the drop-in: the same as the solve.  A status
 * other than MPC_STATUS_SUCCESS, a launch that ends (no loop in the device code has a trip count that the data decide), and no effect
 * on the other instances of the batch, which come out bit for bit as in a batch without it.  out8, cmd and pre of such an instance
 * may hold not-a-number.  What counts as such an input:
 *   - a value of tel / pose, or a waypoint, that is not finite, or so large that the frame change overflows;
 *   - psi: any finite value is an angle.  tel's psi is brought to [-pi, pi): up to |psi| = 202 (more than 64 pi) by the reference's
 *     sequential subtraction, bit for bit; beyond that by one reduction psi - rint(psi / 2 pi) * 2 pi, within 4 ulp(|psi|) of the
 *     exact remainder; from |psi| = 1e9 on (the range of the sine / cosine of this library) and for a psi that is not finite the
 *     instance ends with a status.  pose's psi is taken as it is, with the same limit of 1e9;
 *   - speed [mph] below zero (a speedometer has no such reading; v of a pose may be negative, as the state of a solve may), or
 *     beyond the (relaxed) speed limit, which is MPC_STATUS_INFEASIBLE as ever;
 *   - |steering_angle| (tel) or |steering| (pose) above pi / 2, or not a number;
 *   - waypoints whose first and last have the same x in the car's frame (all at one x, all at the car): no road along the car's axis;
 *   - with `model`, a column that is not usable (the _model section below).
 * Waypoints behind the car, in decreasing x, are none: the reference provides for them (RoadGeometry::orientation) and so does
 * this library.  A warm form starts such an instance as the header says for any refused record or failed warm attempt. */
int mpc_telemetry_batch_device(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                               double *ptsx, double *ptsy, double *cmd, double *out8, int32_t *status, void *stream);
/* The same for host arrays (tel, ptsx, ptsy read only; cmd [2][ld], status [ld] written): one copy in, the kernels, one copy
 * out, on the handle's own device and stream whatever the caller's current device is; synchronises. */
int mpc_telemetry_batch_host(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                             const double *ptsx, const double *ptsy, double *cmd, int32_t *status);
/* Closed-loop rollout (the pattern of src/test.cpp:79-111): `steps` times
 * solve() and feed {x1,y1,psi1,v1,cte1,epsi1} back as the next state, cold start each time as the reference does.
 *   state [6][ld]          in: start states; out: the state after the last step
 *   hist  [steps][9][ld]   or NULL: solve()'s 9-vector of every step
 *   status[ld]             worst (largest) status code over the steps;  iters[ld] or NULL: iterations summed
 * The road polynomial and the psi-bounds stay fixed over the rollout, as in test.cpp (one fit, one run()). */
int mpc_rollout_batch_device(MpcHandle *h, int64_t B, int64_t ld, int steps, double *state, const double *coeffs,
                             const double *yaw_lo, const double *yaw_hi, const double *weights, double *hist,
                             int32_t *status, int32_t *iters, void *stream);

/* ---- warm start (opt-in) -----------------------------------------------------------
 * In a closed loop the problem of step t+1 is the problem of step t with its horizon moved on by one stage: the previous
 * solution is almost the answer.  The warm entry points take the final primal-dual iterate of an earlier solve as the INITIAL
 * ITERATE of this one.  Nothing else changes: the NLP is the reference's, with the branch outcomes of FG_eval and IPOPT's
 * objective scaling decided at the reference's start point (the state at index 0, zeros elsewhere) exactly as in a cold solve,
 * so a warm solve converges to the same NLP's solution and the cold solve stays the yardstick.  (The reference cannot warm start:
 * with a non-zero xi, CppAD would record another tape.  That is deliberately not imitated.)
 *
 * The warm buffer, [mpc_warm_rows(N)][ld_warm] doubles, quantity-major like every array here: row k * MPC_WARM_REC + f is field
 * f of the record of stage k = 0 .. N-2,
 *   f  0..5   x, y, psi, v, cte, epsi at index k+1      = vars[x_start + k+1] ... vars[epsi_start + k+1] (MPC.cpp:56-63)
 *   f  6..7   delta, a at index k                       = vars[delta_start + k], vars[a_start + k]
 *   f  8..13  multipliers of the model rows of index k+1 (constraints[1 + x_start + k+1] ..., MPC.cpp:116-152), the solver's sign
 *   f 14..17  duals of the lower bounds of psi_{k+1}, v_{k+1}, delta_k, a_k
 *   f 18..21  duals of their upper bounds
 * (the variables of index 0 are the given state).  Rules:
 *   - an instance is warm-started only where warm_status (the status array of the solve that wrote warm_in) says
 *     MPC_STATUS_SUCCESS; every other instance starts cold, bitwise the cold solve.  warm_status = NULL: every instance is valid;
 *   - a record that is no iterate of this NLP (not-a-number, a bounded quantity outside its bounds) starts cold as well, and a warm
 *     attempt that ends in anything but MPC_STATUS_SUCCESS is followed by the COMPLETE cold solve (least-squares multiplier start,
 *     then the one restart): a warm start never loses an instance, `iters` adds both up;
 *   - warm_in = NULL is a cold solve that still writes warm_out: how a loop starts, and the way to the full primal-dual solution;
 *     warm_out = NULL writes nothing; warm_in == warm_out and warm_status == status are allowed (in-place loops);
 *   - fp64 handles only (MPC_ERR_INVALID otherwise).  MPC_ERR_UNSUPPORTED, never a silent cold solve, on a handle whose solve is
 *     the two-launch mixed-precision one (set f64_f32_start = 0) and with max_soc > 0 (set max_soc = 0).  No deferred tails, pass
 *     cuts or take order: one launch per call. */
#define MPC_WARM_REC 22
typedef struct MpcWarmOpts {
  int32_t size;        /* sizeof(MpcWarmOpts) */
  int32_t shift;       /* 1: record k starts from the previous record k+1 (the last one repeated): the next step of a closed loop;
                        * 0: as it is: the same problem again, or a loop whose steps are short against the horizon */
  double mu_init;      /* barrier parameter the warm attempt starts with (a cold solve: 0.1), in [tol / 10, 0.1] */
  double bound_push;   /* psi, v, delta, a are moved at least this far (relative, like IPOPT's bound_push) inside their bounds */
  int32_t duals;       /* bound duals: 0 = kept, floored at mu_init / (1e10 slack); 1 = re-derived as mu_init / slack */
  int32_t reserved;
} MpcWarmOpts;
int64_t mpc_warm_rows(int N);                       /* (N-1) * MPC_WARM_REC, or MPC_ERR_INVALID */
int mpc_warm_opts_default(MpcWarmOpts *o);
/* opts = NULL: the defaults */
int mpc_solve_batch_device_warm(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                const double *yaw_lo, const double *yaw_hi, const double *weights, const double *warm_in,
                                const int32_t *warm_status, double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts,
                                double *out, double *traj, int32_t *status, int32_t *iters, void *stream);
int mpc_solve_batch_host_warm(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                              const double *yaw_lo, const double *yaw_hi, const double *weights, const double *warm_in,
                              const int32_t *warm_status, double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts,
                              double *out, double *traj, int32_t *status, int32_t *iters);
/* The rollout above with step 1 cold and every later step warm-started from the step before (cars whose previous step did not
 * succeed start cold).  The warm buffer lives in the handle: mpc_warm_rows(N) * 8 bytes per instance of the handle's capacity,
 * allocated by the first call. */
int mpc_rollout_batch_device_warm(MpcHandle *h, int64_t B, int64_t ld, int steps, double *state, const double *coeffs,
                                  const double *yaw_lo, const double *yaw_hi, const double *weights, const MpcWarmOpts *opts,
                                  double *hist, int32_t *status, int32_t *iters, void *stream);
/* The rollout of mpc_rollout_batch_device (warm_start = 0) or mpc_rollout_batch_device_warm (warm_start = 1; opts as there,
 * NULL = defaults) in ONE launch: a lane keeps its car for all `steps` solves and starts the next one as soon as its own is done,
 * instead of every car waiting at every step for the slowest car of that step.
 * Arguments, outputs, status / iters conventions and refusals are those of the stepwise entry points;
 * every array this call writes (state, hist, status, iters) holds BITWISE what the stepwise call writes.
 * The one launch serves fp64 handles whose solve is a single launch of the lane kernel (no fp32 start, max_soc = 0) for batches
 * above the wave limit; on every other handle and size the call runs the stepwise loop itself (mpc_rollout_fused_info tells). */
int mpc_rollout_batch_device_fused(MpcHandle *h, int64_t B, int64_t ld, int steps, double *state, const double *coeffs,
                                   const double *yaw_lo, const double *yaw_hi, const double *weights, int warm_start,
                                   const MpcWarmOpts *opts, double *hist, int32_t *status, int32_t *iters, void *stream);
/* out2: calls so far that ran the fused kernel, calls that ran the stepwise loop instead */
int mpc_rollout_fused_info(const MpcHandle *h, int64_t *out2);
/* Warm start on the run() path: what a telemetry handler calls once per message (mpc_main.cpp).  Every run() problem starts at
 * (0, 0, 0, v, cte, epsi) in its own vehicle frame, and from one message to the next the solution looks almost the same in that
 * frame, so the previous call's records are taken as they are, unshifted by default -- with one change: the psi box moves with the
 * road fit (MPC.cpp:345-352), so psi (field 2 of every record) is projected into the [yaw_lo, yaw_hi] this call derives before the
 * rules above see it (a not-a-number stays one and is refused).  warm_in is only read.  The library remembers no poses: a rigid
 * re-framing of the records was measured and does not beat this.  Each entry point is its cold form plus
 * warm_in, warm_status, warm_out, ld_warm, opts, with every convention of mpc_solve_batch_device_warm (NULL warm_in: a cold call
 * that writes warm_out, bitwise the cold entry point; in-place buffers; the refusals). */
int mpc_run_batch_device_warm(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *pose, double *ptsx, double *ptsy,
                              const double *warm_in, const int32_t *warm_status, double *warm_out, int64_t ld_warm,
                              const MpcWarmOpts *opts, double *out8, double *traj, int32_t *status, int32_t *iters, double *pre,
                              void *stream);
int mpc_run_batch_host_warm(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *pose, double *ptsx, double *ptsy,
                            const double *warm_in, const int32_t *warm_status, double *warm_out, int64_t ld_warm,
                            const MpcWarmOpts *opts, double *out8, double *traj, int32_t *status, int32_t *iters, double *pre);
int mpc_telemetry_batch_device_warm(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                                    double *ptsx, double *ptsy, const double *warm_in, const int32_t *warm_status, double *warm_out,
                                    int64_t ld_warm, const MpcWarmOpts *opts, double *cmd, double *out8, int32_t *status,
                                    void *stream);
int mpc_telemetry_batch_host_warm(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                                  const double *ptsx, const double *ptsy, const double *warm_in, const int32_t *warm_status,
                                  double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts, double *cmd, int32_t *status);
/* ---- per-instance model values (dt, Lf, limits) ----------------------------------------------------------------------------
 * A batch whose instances differ in the time step, the wheelbase or the actuator and speed limits -- a dt study, a fleet of
 * different vehicles, randomised limits over many closed loops -- in one launch on one handle.  Each entry point is the one
 * without `_model` plus `model`, [MPC_NMODEL][ld] doubles addressed like `weights` (rows MPC_MODEL_*, in the units of the MpcParams
 * fields of the same names).
 * model == NULL: the call IS the entry point without `_model`, with every convention it has (deferred tails, take order, the
 *   wave path), bitwise.
 * model != NULL: instance i is solved with dt, Lf, max_steering, max_acceleration, max_deceleration and max_speed of its column.
 *   Everything else is the handle's: N, the weights (unless `weights` is given), the panic thresholds, the speed tables, every
 *   solver control and max_soc.  The speed target is computeSpeedTarget(0, max_speed_i) on the handle's tables; the relaxed bounds
 *   of the solve and the projection of honor_original_bounds use the instance's limits.
 * Dispatch: a model call is always ONE launch of the single-phase fp64 lane kernel, at every B -- no wave path, no deferred
 *   tails (no instance is ever MPC_STATUS_PENDING), no pass cuts, no take order.  A handle whose ordinary solve starts in fp32
 *   (f64_f32_start = 1, or AUTO at N >= 15: the library's default parameters at N = 25) is served the same way on its fp64
 *   workspace; such a call is never refused, allocates nothing, and its results are bitwise those of a handle created with
 *   f64_f32_start = 0.  max_soc > 0 is honoured.  MPC_PRECISION_F32 handles: MPC_ERR_INVALID with a message.
 * A column that is not usable -- a non-finite value, dt <= 0, Lf <= 0, max_steering <= 0, max_speed <= 0 (what mpc_create refuses
 *   in MpcParams), max_acceleration <= 0 or max_deceleration >= 0 (the start point a = 0 must lie inside the box) -- ends that
 *   instance with MPC_STATUS_INFEASIBLE and the start point in `out`, as an infeasible start does, with no not-a-number; the
 *   batch goes on.  A state with |v| beyond the instance's own relaxed speed limit is MPC_STATUS_INFEASIBLE as ever.
 * The rollout is the stepwise cold loop of mpc_rollout_batch_device with `model` passed to every step (warm and in one launch:
 * the next section; run() and the telemetry handler: the section after that). */
int mpc_solve_batch_device_model(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                 const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                 double *out, double *traj, int32_t *status, int32_t *iters, void *stream);
int mpc_solve_batch_host_model(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                               const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                               double *out, double *traj, int32_t *status, int32_t *iters);
int mpc_rollout_batch_device_model(MpcHandle *h, int64_t B, int64_t ld, int steps, double *state, const double *coeffs,
                                   const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                   double *hist, int32_t *status, int32_t *iters, void *stream);
/* ---- warm start and the one-launch rollout with per-instance model values ----------------------------------------------------
 * Each entry point is the one of the same name without `_model` plus `model` directly behind `weights`, [MPC_NMODEL][ld] addressed
 * like `weights`, exactly as in mpc_solve_batch_device_model.
 * model == NULL: the call IS the entry point without `_model`, bitwise, with every convention that one has (the wave path and its
 *   refusals included).
 * model != NULL, what a call solves with: every convention of the warm entry points holds -- only columns whose warm_status is
 *   MPC_STATUS_SUCCESS start warm; a refused record, or a warm attempt that does not end in SUCCESS, is followed by the complete cold
 *   solve and `iters` adds both up; warm_in = NULL is a cold call that writes warm_out, bitwise mpc_solve_batch_device_model; warm_in
 *   may be warm_out and warm_status may be status -- and so does every convention of the model entry points: the six values of
 *   instance i come from its column, everything else from the handle, and an unusable column ends MPC_STATUS_INFEASIBLE with finite
 *   outputs and a finite record in warm_out.
 * model != NULL, the box a record is checked against: the instance's own relaxed box, the one the solve itself uses (relaxed limits
 *   of ITS max_speed, max_steering, max_acceleration, max_deceleration).  A record may therefore have been written under another
 *   column than the one it is handed to: if it still fits it starts warm, if it does not (a delta beyond a narrowed max_steering)
 *   the instance starts cold and is bitwise the cold model solve, iterations included.  shift = 1 moves a record by one stage, which
 *   is that instance's own dt.
 * Dispatch: a warm model call is always ONE launch of the single-phase fp64 lane kernel, at every B -- no wave path, no deferred
 *   tails, no pass cuts, no take order, as for a model call; lane compaction applies as for a warm call and changes no result.
 * Accepted handles: the model rule.  Every fp64 handle, also one whose ordinary solve starts in fp32 (f64_f32_start = 1, or AUTO
 *   at N >= 15): it is served on its fp64 workspace, nothing is allocated for that, and the results are bitwise those of a handle
 *   created with f64_f32_start = 0.  (The warm entry points without `_model` refuse such a handle because their solve would be the
 *   two-launch one; here it never is, so nothing is silently cold.)
 * Refusals: an MPC_PRECISION_F32 handle gets MPC_ERR_INVALID with the model message; max_soc > 0 together with a warm start gets
 *   MPC_ERR_UNSUPPORTED, as for every warm call.
 * mpc_rollout_batch_device_warm_model: the stepwise loop of mpc_rollout_batch_device_warm with `model` passed to every step.
 * mpc_rollout_batch_device_fused_model: writes bitwise what mpc_rollout_batch_device_model writes (warm_start = 0) or what
 *   mpc_rollout_batch_device_warm_model writes (warm_start = 1), into state, hist, status and iters.  The stepwise model loop
 *   launches the lane kernel at every B, so the one launch runs at every B >= 1 on every fp64 handle with max_soc = 0; a cold call
 *   with max_soc > 0 runs the stepwise loop itself.  mpc_rollout_fused_info counts both kinds, as for the call without `_model`.
 *   A car whose step ends MPC_STATUS_INFEASIBLE (an unusable column, a speed beyond its own limit) behaves as in the stepwise
 *   loop: the start point is that step's "solution", the next state is taken from it, and the next step starts cold. */
int mpc_solve_batch_device_warm_model(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                      const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                      const double *warm_in, const int32_t *warm_status, double *warm_out, int64_t ld_warm,
                                      const MpcWarmOpts *opts, double *out, double *traj, int32_t *status, int32_t *iters,
                                      void *stream);
int mpc_solve_batch_host_warm_model(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                    const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                    const double *warm_in, const int32_t *warm_status, double *warm_out, int64_t ld_warm,
                                    const MpcWarmOpts *opts, double *out, double *traj, int32_t *status, int32_t *iters);
int mpc_rollout_batch_device_warm_model(MpcHandle *h, int64_t B, int64_t ld, int steps, double *state, const double *coeffs,
                                        const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                        const MpcWarmOpts *opts, double *hist, int32_t *status, int32_t *iters, void *stream);
int mpc_rollout_batch_device_fused_model(MpcHandle *h, int64_t B, int64_t ld, int steps, double *state, const double *coeffs,
                                         const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                         int warm_start, const MpcWarmOpts *opts, double *hist, int32_t *status, int32_t *iters,
                                         void *stream);
/* ---- per-instance horizon: the N of every instance -----------------------------------------------------------------------------
 * One more rule next to the two above: the _horizon form of an entry point is its _model form plus `horizon`, [ld] int32, directly
 * behind `model`: instance i is solved as the reference solves it with Config::N = horizon[i], 3 .. the handle's N, in one launch on
 * one handle.  Seven entry points have one -- the solve (device, host), the warm solve (device, host) and the three rollouts; the
 * telemetry handler and the track drive have theirs in mpc_amd_drive.h, run(), the wire forms and the C++ drop-in have none.  The section and its seven declarations live in
 * a header of their own, which this one includes: */
#include "mpc_amd_horizon.h"
/* ---- certify a stored solution: IPOPT's final error summary for a point the caller names ---------------------------------------
 * Two entry points evaluate the NLP of the solve once, at a stored primal-dual point (a warm buffer: warm_out of any _warm entry
 * point), and write twelve measures per instance -- objective, constraint violation, dual infeasibility, complementarity, overall
 * NLP error, bound violation, objective scaling, the five cost groups -- and a verdict by the handle's tolerances.  One launch, a
 * lane per instance; nothing is solved and nothing else changes.  The section and its declarations live in a header of their own,
 * which this one includes: */
#include "mpc_amd_certify.h"
/* ---- track driving: window, handler and plant on the device, `steps` messages in one call --------------------------------------
 * The mpc_drive_* entry points drive B cars along a cyclic track of waypoints: per message the waypoint window at the car's position,
 * the telemetry handler of this header (cold or warm, optionally with per-instance weights) and the reference's own kinematic model
 * as the plant, with a summary per car and, if asked for, a record per step.  Nothing returns to the host between the steps.  The
 * section and its declarations live in a header of their own, which this one includes: */
#include "mpc_amd_drive.h"
/* ---- per-instance iteration budget: the reference's solve deadline (ipoptTimeout), counted in iterations -------------------------
 * The _budget forms of the warm horizon solve and of the track drive cap the interior-point iterations of every instance over all of
 * its attempts and hand an unconverged iterate on to the next message.  The section and its declarations live in a header of their
 * own, which this one includes: */
#include "mpc_amd_budget.h"
/* ---- track drive under noise: seeded per-car sensor, actuator and link noise ------------------------------------------------------
 * The _noise forms of the track drive hand the handler a noisy reading of every car (`seen`), perturb the plant per message and drop
 * replies, from a counter-based random stream that depends on the car's seed and the message index alone: a Monte-Carlo over noisy
 * drives is seeds x noise levels as the columns of one call.  The section and its declarations live in a header of their own, which
 * this one includes: */
#include "mpc_amd_noise.h"
/* ---- per-instance model values on the run() path: a fleet of different vehicles behind one handler ----------------------------
 * Each entry point is the one of the same name without `_model` plus `model`, [MPC_NMODEL][ld] doubles addressed with the call's
 * ld (rows MPC_MODEL_*), directly behind `ptsy`; the wire forms further down take it as [MPC_NMODEL][B] directly behind
 * `extra_latency`.  Host forms: a host array, copied in with the other inputs.
 * model == NULL: the call IS the entry point without `_model`, bitwise, with all of its conventions and refusals.
 * model != NULL, what instance i is processed with: the six values of its column in the solve (as in mpc_solve_batch_device_model;
 *   dt enters only there) and, around it, in the five places of MPC::run() and the handler that read them --
 *     max_speed         the cap of the two speed tables: pre[14] (target speed) is what the instance's own max_speed gives
 *                       (the only row of `pre` that depends on the column: pre[11..13] come from the fit); the `keep` term of
 *                       computeThrottle
 *     max_steering      the normalisation of the steering value in out8[4] / cmd[0]
 *     Lf                the heading of the latency compensation (telemetry forms)
 *     max_acceleration, max_deceleration   computeThrottle (telemetry forms)
 *   Everything else is the handle's: the speed tables themselves, max_fit_order / max_fit_error, latency_ms, lookahead,
 *   steer_adj_*, the weights, N, every solver control and max_soc.
 * A column that is not usable (the rule of the section above): the handle's values take its place in the pre- and post-processing as
 *   in the solve, the instance ends MPC_STATUS_INFEASIBLE, out8, cmd, pre and warm_out hold no not-a-number, and the batch goes on.
 *   A car faster than its own (relaxed) speed limit is MPC_STATUS_INFEASIBLE as ever.
 * Dispatch: ONE solve launch between the pre and the post kernel -- the wave kernel's MODEL build (an instance per wavefront, or per
 *   16 / 32 of its lanes) when B <= wave_max_batch (0 means 1 024, below 0 never), cold, with max_soc > 0, and warm; above it the
 *   lane kernel's MODEL build, as for every model call.  No deferred tails, no pass cuts, no take order.  Both write the same bits.
 *   (mpc_solve_*_model and mpc_rollout_*_model are not changed by this: the lane kernel at every B.)
 * Accepted handles: the model rule.  Every fp64 handle, also one whose ordinary solve starts in fp32 (served on its fp64 workspace,
 *   bitwise a handle created with f64_f32_start = 0) -- for the warm forms too, which without `_model` refuse such a handle.
 * Refusals: an MPC_PRECISION_F32 handle gets MPC_ERR_INVALID with the model message; max_soc > 0 together with a warm form gets
 *   MPC_ERR_UNSUPPORTED, as every warm call does (the cold forms honour max_soc); npts outside 3..8, ld < B and ld_warm < B get
 *   MPC_ERR_INVALID as without `_model`.
 * Warm forms: every rule of mpc_solve_batch_device_warm_model (a record is checked against the instance's own relaxed box; one that
 *   no longer fits -- written under a column with a wider max_steering, say -- starts that instance cold, bitwise the cold model
 *   call) and the one extra rule of the run() path: psi of the record is projected into this call's [yaw_lo, yaw_hi] first. */
int mpc_run_batch_device_model(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *pose, double *ptsx, double *ptsy,
                               const double *model, double *out8, double *traj, int32_t *status, int32_t *iters, double *pre,
                               void *stream);
int mpc_run_batch_host_model(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *pose, double *ptsx, double *ptsy,
                             const double *model, double *out8, double *traj, int32_t *status, int32_t *iters, double *pre);
int mpc_telemetry_batch_device_model(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                                     double *ptsx, double *ptsy, const double *model, double *cmd, double *out8, int32_t *status,
                                     void *stream);
int mpc_telemetry_batch_host_model(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                                   const double *ptsx, const double *ptsy, const double *model, double *cmd, int32_t *status);
int mpc_run_batch_device_warm_model(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *pose, double *ptsx, double *ptsy,
                                    const double *model, const double *warm_in, const int32_t *warm_status, double *warm_out,
                                    int64_t ld_warm, const MpcWarmOpts *opts, double *out8, double *traj, int32_t *status,
                                    int32_t *iters, double *pre, void *stream);
int mpc_run_batch_host_warm_model(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *pose, double *ptsx, double *ptsy,
                                  const double *model, const double *warm_in, const int32_t *warm_status, double *warm_out,
                                  int64_t ld_warm, const MpcWarmOpts *opts, double *out8, double *traj, int32_t *status,
                                  int32_t *iters, double *pre);
int mpc_telemetry_batch_device_warm_model(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                                          double *ptsx, double *ptsy, const double *model, const double *warm_in,
                                          const int32_t *warm_status, double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts,
                                          double *cmd, double *out8, int32_t *status, void *stream);
int mpc_telemetry_batch_host_warm_model(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                                        const double *ptsx, const double *ptsy, const double *model, const double *warm_in,
                                        const int32_t *warm_status, double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts,
                                        double *cmd, int32_t *status);
/* Per-instance latency: mpc_telemetry_batch_device_latency and mpc_telemetry_batch_host_latency are the two _warm_model forms above plus
 * `comp` [ld], the seconds each instance compensates for, directly behind extra_latency.  They are declared and described with the
 * drive's _latency forms in mpc_amd_drive.h (included above), section "per-car latency". */
/* ---- the wire side of the handler (src/mpc_main.cpp:26-36, 81-222, DATA.md:5-16) --------
 * Everything between the bytes of a simulator frame and the bytes of the reply; the WebSocket server itself is out of
 * scope.  See csrc/mpc_wire.cpp. */
enum { MPC_WIRE_MANUAL = 0, MPC_WIRE_TELEMETRY = 1, MPC_WIRE_IGNORE = 2 };
typedef struct MpcWireTelemetry {
  double x, y, psi, speed, steering_angle, throttle;   /* as sent: psi [rad], speed [mph], simulator's steering sign */
  int32_t npts, reserved;
  double ptsx[8], ptsy[8];                             /* global waypoints */
} MpcWireTelemetry;
/* One text frame `42["telemetry",{...}]`: MPC_WIRE_TELEMETRY and *out filled; MPC_WIRE_MANUAL when the frame carries no
 * data (the reference answers `42["manual",{}]`, mpc_main.cpp:217-219); MPC_WIRE_IGNORE for anything that is not a "42"
 * telemetry event (the reference stays silent); MPC_ERR_INVALID for a malformed telemetry object (the reference would
 * throw out of json::parse).  A number that is not finite -- `inf`, `nan`, `1e999`, which strtod would read and JSON does not have --
 * anywhere in the object (ptsx, ptsy, x, y, psi, speed, steering_angle, throttle) makes the frame malformed: MPC_ERR_INVALID.
 * lib/mpc_replay answers such a frame like any other it cannot parse: a message on stderr, no reply, exit status 1 at the end, and
 * the other frames of the group get the replies they get without it. */
int mpc_wire_parse(const char *frame, int64_t len, MpcWireTelemetry *out);
/* The reply `42["steer",{...}]` byte for byte as mpc_main.cpp:183-197 builds it with nlohmann::json 2.1.1 (build without
 * PLOT_TRAJECTORY).  Returns the length (NUL-terminated in buf), or MPC_ERR_INVALID if cap is too small. */
int64_t mpc_wire_format_steer(double steering_angle, double throttle, char *buf, int64_t cap);
int64_t mpc_wire_format_manual(char *buf, int64_t cap);
/* B parsed frames, one per connection, through mpc_telemetry_batch_device (host arrays in and out).
 * prev_throttle[B] or NULL: throttle of each connection's previous reply; cmd [2][B]: steering_angle row, throttle row. */
int mpc_wire_telemetry_batch_host(MpcHandle *h, int64_t B, const MpcWireTelemetry *tel, const double *prev_throttle,
                                  double extra_latency, double *cmd, int32_t *status);
/* The same through mpc_telemetry_batch_host_warm: column i of the warm buffers belongs to connection i. */
int mpc_wire_telemetry_batch_host_warm(MpcHandle *h, int64_t B, const MpcWireTelemetry *tel, const double *prev_throttle,
                                       double extra_latency, const double *warm_in, const int32_t *warm_status, double *warm_out,
                                       int64_t ld_warm, const MpcWarmOpts *opts, double *cmd, int32_t *status);
/* The two above for connections with vehicles of their own (mpc_telemetry_batch_host_model / _host_warm_model): model is
 * [MPC_NMODEL][B], column i belonging to connection i; NULL: the entry point without `_model`. */
int mpc_wire_telemetry_batch_host_model(MpcHandle *h, int64_t B, const MpcWireTelemetry *tel, const double *prev_throttle,
                                        double extra_latency, const double *model, double *cmd, int32_t *status);
int mpc_wire_telemetry_batch_host_warm_model(MpcHandle *h, int64_t B, const MpcWireTelemetry *tel, const double *prev_throttle,
                                             double extra_latency, const double *model, const double *warm_in,
                                             const int32_t *warm_status, double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts,
                                             double *cmd, int32_t *status);
/* ---- deferred tails (MpcParams.tail_cut > 0) ----------------------------------------------------------------
 * A launch lasts as long as its slowest instance; on heavy-tailed workloads one 200-iteration straggler prices 65 536
 * solves.  With tail_cut = n the launch of mpc_solve_batch_device(_f32) hands every instance that is still running after
 * n passes to the handle's tail queue and ends: when the call's work on `stream` is complete, every other instance has
 * its final results and the handed-over ones carry status MPC_STATUS_PENDING (mpc_tail_pending counts them).  They are
 * carried on by TAIL SLICES on the handle's own high-priority stream: short launches (a bounded number of passes each)
 * that take the survivors of the slice before them and whatever the launches since have handed over, re-packed into dense
 * waves every time, and write the same arrays; results are bitwise those of an undisturbed launch.  Slices are started by
 * the calls below and by every solve call ("the pump"): nothing runs on its own between calls, so a serving loop that has
 * stopped issuing batches finishes with mpc_tail_wait (or polls).
 * The caller keeps a batch's output arrays alive and does not read its pending entries until the batch is final:
 *   mpc_last_batch_id     id of the batch the most recent solve call issued (ids count up from 1 per handle)
 *   mpc_tail_poll         1 if batch `id` is final, 0 if not yet (runs one turn of the pump, never blocks)
 *   mpc_tail_wait         blocks the host until batch `id` is final (id <= 0: every batch issued so far); for a batch that
 *                         did not defer (small batches, tail_cut = 0, the run()/telemetry/rollout/host entry points) that is
 *                         the completion of its own launch
 *   mpc_tail_stream_wait  orders `stream` behind the batch being final.  A batch that did not defer: a stream-side wait for its
 *                         launch, the host does not block.  A deferring batch is final behind slices that do not exist yet,
 *                         so the host pumps until it is (blocks), then `stream` is ordered behind the tail stream
 *   mpc_tail_flush        one turn of the pump (optional)
 * The handle resolves the ids of its last 1 024 batches; older ones return MPC_ERR_INVALID.  At most tail_ring batches may
 * be outstanding; issuing one more blocks the host until the oldest is final.  The survivors' list is bounded: while it is
 * more than half full, new batches run without deferral (counted in mpc_tail_info).
 * The run(), telemetry, rollout and host entry points never defer. */
int64_t mpc_last_batch_id(const MpcHandle *h);
/* How many batches of B instances to keep in flight (handles on streams of their own, INTEGRATION.md "batches in flight") for
 * these parameters, from the measurements behind DESIGN.md sections 6b/6c/6f: about two devices' worth of lanes (131 072
 * instances), between 2 and 8 launches -- 8 x 16 384 and 4 x 32 768 give what 2 x 65 536 gives -- and at least 4 for two-launch
 * solves (MPC_PRECISION_F32, the fp32 start) and horizons of 15 steps and more.  No device is touched. */
int mpc_inflight_advice(const MpcParams *p, int64_t B);
int mpc_tail_poll(MpcHandle *h, int64_t batch_id);
int mpc_tail_wait(MpcHandle *h, int64_t batch_id);
int mpc_tail_stream_wait(MpcHandle *h, int64_t batch_id, void *stream);
int mpc_tail_flush(MpcHandle *h);
int mpc_tail_pending(MpcHandle *h, int64_t batch_id, int64_t *n);   /* waits for the batch's own launch, then: how many it handed over */
/* out13: batches deferred so far, tail slices so far, ring, capacity of a batch's fresh queue, waves per slice (upper bound), 1 if the
 * tail stream has high priority, number of tail streams (1), batches that ran without deferral because the survivors' list was
 * filling up, passes per slice, survivors after the most recent retired slice, the cut in use (MPC_TAIL_AUTO: the current choice),
 * running mean of the deferred share of a batch in 1/65536 (-1: none retired yet), batches that handed over more than their fresh
 * queue holds (the rest finished in the launch; MPC_TAIL_AUTO then raises its cut) */
int mpc_tail_info(const MpcHandle *h, int64_t *out13);
/* Take order: large single-phase fp64 launches of the solve entry points take their instances bin by bin of
 * predicted work instead of in index order; results do not depend on it.  out2: launches so far that were taken in key order, and
 * the mode (1 = hardest bin first, 2 = easiest first, 0 = off: MPC_TAKE_ORDER in the environment at mpc_create, a measurement aid). */
int mpc_take_order_info(const MpcHandle *h, int64_t *out2);
int mpc_synchronize(MpcHandle *h);
/* Statistics of the most recent mpc_solve_batch_* call: gathered when asked for, from the status / iters arrays that call
 * wrote (they must still be there); waits for that call's launch. */
int mpc_get_stats(MpcHandle *h, MpcBatchStats *stats);

/* ---- diagnostics ------------------------------------------------------------ */
/* Evaluates the device's own light-weight math on n host values (the solver replaces libm's
 * sincos and IEEE division by shorter sequences, see csrc/mpc_core.h): sn[i], cs[i] = sin/cos(x[i]),
 * rc[i] = 1/x[i].  Used by the tests to bound their error on the real hardware. */
int mpc_debug_math(int device, int64_t n, const double *x, double *sn, double *cs, double *rc);
/* the same plus at[i] = atan(x[i]) and lg[i] = log|x[i]| (the solver's own atan and log kernels) */
int mpc_debug_math_ext(int device, int64_t n, const double *x, double *sn, double *cs, double *rc, double *at, double *lg);
/* Every light-weight math function of csrc/mpc_core.h at n points, one point per lane (test infrastructure like the two above, not
 * product API; tests/test_math_conformance.py).  out is [MPC_DEBUG_MATH_ROWS][n]:
 *   rows 0..9   fp64: fsincos2(x, y) -> sin x, cos x, sin y, cos y;  frcp(x), frcp1(x), fatan(x), flog(x);
 *                     hpow(x, 1.1), hpow(x, 2.3) (the two exponents of the line search's switching condition)
 *   rows 10..19 fp32: the same ten from (float)x, (float)y, widened exactly
 * flog and hpow get x as it comes (no fabs): the caller sends only what it means to send. */
#define MPC_DEBUG_MATH_ROWS 20
int mpc_debug_math_all(int device, int64_t n, const double *x, const double *y, double *out);

#ifdef __cplusplus
}
#endif
#endif /* MPC_AMD_H */
