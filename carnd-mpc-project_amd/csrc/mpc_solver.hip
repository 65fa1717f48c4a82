/*
 * mpc_solver.hip -- gfx950 kernels and the C ABI of include/mpc_amd.h.
 *
 * Batched replacement of MPC::solve() (src/control/MPC.cpp:183-325): B
 * independent instances, one per lane (64 per wavefront), struct-of-arrays in
 * HBM.  No CPU fallback exists: without a gfx950 device every compute entry
 * point returns an error.
 */
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "mpc_core.h"
#include "mpc_run_core.h"
#include "mpc_drive_core.h"
#include "mpc_take_key.h"

namespace {

thread_local std::string g_last_error;

#define MPC_HIP_CHECK(expr)                                                              \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) {                                                              \
      g_last_error = std::string(#expr) + ": " + hipGetErrorString(e_);                  \
      return MPC_ERR_HIP;                                                                \
    }                                                                                    \
  } while (0)

/* Every entry point works on the handle's device and leaves the caller's current device as it found it. */
struct DeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) err = hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};
#define MPC_ON_DEVICE(h)                                                                 \
  DeviceGuard guard_((h)->device);                                                       \
  if (guard_.err != hipSuccess) {                                                        \
    g_last_error = std::string("hipSetDevice: ") + hipGetErrorString(guard_.err);        \
    return MPC_ERR_HIP;                                                                  \
  }

constexpr int kBlock = 64; /* one wavefront per workgroup: lanes never synchronise */
constexpr int64_t kLdsPerCu = 160 * 1024;
constexpr int kMaxCuts = 4;         /* cuts of the multi-phase solve: up to 5 launches per batch */
constexpr int kPhaseCounterInts = 16;   /* two counters per phase */
constexpr int kCounterInts = kPhaseCounterInts + mpc::kTakeBins;   /* ... and behind them the take-order key's instances per bin (a block is zeroed by one wave) */
static_assert(kCounterInts <= 64, "a counter block is zeroed by the lanes of one wave");
constexpr int kCounterRing = 32;    /* counter blocks: solve call n uses block n % 32 and zeroes block (n + 16) % 32 for its next user */
constexpr int kParkRows = 47;       /* Solver::PARK_N */
constexpr size_t kMailboxBytes = (size_t)kParkRows * 64 * sizeof(double) + 2 * 64 * sizeof(int);   /* lane compaction: the scalars of up to 64 moving instances, their index and passes */
constexpr int kFinPromote = -2, kFinScratch = -3;   /* a lane that waits to hand its instance to the fp64 phase (promoted / to be solved from scratch) */
constexpr int kTailMaxRing = 512;   /* deferred tails: batches whose stragglers may be outstanding at once */
constexpr int kFreshRing = 24;      /* fresh queues: one per batch between its launch and the completion of the tail slice that absorbs its stragglers */
constexpr int kSliceMaxSrc = 1 + kFreshRing;   /* what one tail slice reads: the survivors of the slice before it + fresh queues */
constexpr int kSliceRing = 4;       /* slices whose events and result blocks are kept (at most two are in flight) */
constexpr int kTailInRows = 6 + MPC_NCOEF + 2 + MPC_NW;   /* the inputs of a deferred instance travel with it: 25 rows */
constexpr int kTailMetaRows = 8;    /* ... and where it belongs: instance, slot, batch id, out, traj, status, iters, ldo */
constexpr int kTailRows = kParkRows + kTailInRows + kTailMetaRows;
/* fixed launch policies (measured; see MpcPhase and MpcHandle for what each one governs) */
constexpr int kRefillMin = 16, kRefillWait = 8;     /* hand-over policy of the persistent kernel, every phase */
constexpr int kCompactCooldown = 2;                 /* lane compaction: passes without another move after one */
constexpr int64_t kPassCutMinBatch = 8192;          /* multi-phase solve: smaller launches run in one phase */
constexpr int64_t kWaveWholeMax = 16;               /* one instance per wavefront: launches up to this size give it the whole wave */
constexpr int64_t kTailMinBatch = 4096;             /* deferred tails: smaller launches finish their own stragglers */
constexpr int kTailFewFrom = 8;                     /* ... a wave's last tail_few lanes are handed over after this many passes */
constexpr int kSliceFreshDiv = 4;                   /* ... a tail slice's grid: a lane per survivor and one per 4 fresh entries */
constexpr int64_t kAutoShareLo = 983, kAutoShareHi = 5243;   /* ... MPC_TAIL_AUTO: 1.5 % and 8 % of a batch, in 1/65536 */

/* One queue of deferred instances: the fresh queue a launch hands its stragglers to, or the list of survivors a tail slice
 * leaves for the next one.  Entry e: column e of `park` ([kTailRows][cap]: Solver::park scalars, the instance's inputs, where
 * its results go) and lane e % 64 of tile e / 64 of `iter` ([cap / 64][N-1][IT_SZ][64] reals: its current iterate). */
struct MpcTailQ {
  int32_t *count;                  /* entries appended so far (may run past cap: min(count, cap) are valid) */
  int32_t cap;                     /* multiple of 64 */
  double *park;
  void *iter;
};

/*
 * One instance per lane.  Inputs/outputs are [quantity][instance] so that a wave's access to one
 * quantity is a single contiguous 512-byte transaction; the workspace is tiled per wave with fields
 * interleaved in pairs per lane (see mpc_core.h).  STAGING: every sweep double-buffers the next
 * stage's record into this workgroup's LDS with LDS-DMA (global_load_lds) while it computes.
 */
template <class R> constexpr size_t staging_lds_bytes() { return 2u * mpc::Fields<R>::STG_SLOT * 64u * 16u; }   /* 36 KB per wave (fp64), 20 KB (fp32) */

#if defined(__HIP_DEVICE_COMPILE__)
#define MPC_WAVE_ANY(p) (__builtin_amdgcn_ballot_w64(p) != 0ull)   /* over the active lanes of the wave */
#define MPC_WAVE_COUNT(p) __builtin_popcountll(__builtin_amdgcn_ballot_w64(p))
#else
#define MPC_WAVE_ANY(p) (p)
#define MPC_WAVE_COUNT(p) ((p) ? 1 : 0)
#endif

/* Persistent form: a wave does not own 64 fixed instances.  Every lane takes the next unsolved instance from a
 * global counter, solves it, writes its results and takes another one, until the counter passes the end; the solver
 * is a per-lane state machine (Solver::step), so the lanes of a wave may be on different instances in different
 * phases.  With a grid of ceil(B/64) waves this is the plain one-instance-per-lane launch.
 *
 * Multi-phase solve (MpcPhase): a wave lasts as long as its slowest instance, and two thirds of the instances are
 * done after ~10 iterations while the slowest need 25 (headline workload) or 100-200 (weight sweeps, long horizons).
 * A phase with a cut therefore PARKS an instance that is still running after `pass_cut` passes (at a pass boundary
 * in the DIR phase: 36 scalars + its current iterate, which stays where it is) and appends it to a list; the next
 * phase, launched right behind on the same stream, is the same kernel taking its work from that list: a lane copies
 * the parked iterate into its own tile, restores the scalars and carries on -- and may park it again if that phase
 * has a cut too.  The arithmetic of an instance does not change (results are bitwise identical), but the unfinished
 * part is re-packed into dense waves after every cut, so a wave slot is not held by one or two stragglers.  Lists,
 * scalars and workspaces alternate between two buffers (phase p reads what phase p-1 wrote).
 *
 * Exit: a lane stops asking once its counter has passed the end; the wave leaves when no lane holds an instance and
 * none can get one -- every pass either advances an instance (bounded by max_iter and the cut) or consumes the
 * counter.  A lane that has parked takes nothing else (its column keeps the iterate), so a phase with a cut needs as
 * many lanes as it may receive instances: the host launches every phase with the grid of the first. */
struct MpcPhase {
  int32_t *take;            /* counter this phase takes its work from */
  const int32_t *n_in;      /* resume: number of parked instances to take (written by the previous phase) */
  int32_t *n_out;           /* number of instances this phase has parked */
  const int32_t *in_inst;   /* resume: instance index ... */
  const int32_t *in_src;    /* ... and wave * 64 + lane of the tile column (of src_ws) that holds its iterate */
  const double *in_park;    /* resume: [PARK_N][ld_park] solver scalars, column = position in the list */
  int32_t *out_inst, *out_src;
  double *out_park;
  int64_t ld_park;
  const void *src_ws;       /* resume: workspace of the previous phase */
  int32_t pass_cut;         /* park after this many passes in this phase (0 = never) */
  int32_t resume;           /* 0 = first phase (fresh instances), 1 = takes parked ones */
  /* Mixed precision across phases (MpcParams.f32_finish, f64_f32_start): a phase with promote_out != 0 runs the fp32 solver
   * with Solver::promote_mu set and parks every instance that returns MPC_PROMOTE; the next phase (promote_in != 0) is the
   * fp64 solver resuming from that list: the parked iterate, in the fp32 record layout of src_ws (tiles of src_tile_reals
   * floats), is converted field by field, the point is re-evaluated in fp64 and the solve goes on to tol and the polish. */
  int32_t promote_out, promote_in;
  int64_t src_tile_reals;
  /* The promoted iterates travel in a buffer of their own, [list position / 64][N-1][IT_SZ][64] reals of the fp32 record:
   * a lane that has handed its instance over is free at once -- it takes the next instance while the launch has any, and
   * its column is there for lane compaction -- and the fp64 phase reads 64 consecutive entries per wave instead of 64
   * columns scattered over the fp32 workspace.  (nullptr: the iterate stays in its column, as in a cut schedule.) */
  void *p_iter;
  /* Hand-over policy.  Writing a finished instance out and fetching the next one (set-up, start point: 270 stores) is
   * divergent code that the whole wave pays for, ~4 us per event against ~80 us per pass, and with 64 lanes finishing at
   * different times nearly every pass would have one.  So finished lanes WAIT until `refill_min` lanes of the wave are
   * waiting, or `refill_wait` passes have gone by, or nothing else is running; then all of them are served at once. */
  int32_t refill_min, refill_wait;
  /* Lane compaction (MPC_LANE_COMPACT=gap, measurement aid).  Memory is fetched in 128-byte lines = the 16-byte groups of 8
   * neighbouring lanes, so a line is fetched as long as ONE of its 8 lanes still runs (tools/traffic_model.py: the launch
   * fetches 1.24 x what its running lanes ask for).  Once the launch's counter is exhausted, a wave whose running lanes are
   * spread over `compact_gap` more 8-lane groups than they need moves the ones outside its fullest groups into free lanes
   * inside them: solver scalars through LDS (the staging buffers are idle between passes), set-up repeated from the inputs,
   * the iterate copied column to column -- the arithmetic of an instance does not depend on its lane. */
  int32_t compact_gap, compact_cooldown;   /* (passes without another move after one) */
  /* Deferred tails (MpcParams.tail_cut): an instance still running after tail_cut passes is handed to the handle's tail
   * queue -- solver scalars, its inputs and its current iterate are COPIED out, so the lane and the workspace are free at
   * once -- and reported as MPC_STATUS_PENDING; mpc_tail_kernel finishes it from another stream.  A full queue (t_cap) makes
   * the instance finish here after all. */
  int32_t tail_cut, t_slot;        /* t_slot: the batch's slot in the handle's ring (its live-instance counter, its final flag) */
  /* ... and a wave does not wait for its last few lanes: once the launch has no work left to hand out and at most tail_few of
   * a wave's lanes are still running (after tail_few_from passes), they are handed over too and the wave leaves.  A launch
   * of one instance per lane lasts as long as its waves do, a wave as long as the slowest of its 64 instances: the mean of
   * that maximum is 19 passes on the survey population with a cut at 20, 17.3 when the last two lanes are not waited for
   * (2.6 % of the instances handed over instead of 1.1 %). */
  int32_t tail_few, tail_few_from;
  int64_t t_batch;                 /* the batch's id */
  MpcTailQ tq;                     /* the batch's fresh queue */
  int32_t *zero_next;              /* first launch of a solve call: kCounterInts counters to reset for a later call (no memset launches on
                                    * the stream: on a full device each of those little launches waits for a free SIMD) */
  /* SOC builds (MpcParams.max_soc > 0): the SOC records, [wave of this launch][N-1][SOC_SZ / G][64][G] reals.  A correction lives
   * within one line search of one lane, so they go with the launch's wave number, not with the workspace tile. */
  void *soc_ws;
  /* Take order (first phase only; nullptr = position p of the counter is instance p).  mpc_take_key_kernel has sorted the launch's
   * instances into mpc::kTakeBins bins of predicted work: ord_cnt[b] instances in bin b, their indices in ord_list[b * ord_ld ..].
   * Position p of the counter is then the p-th instance of the bins laid end to end, so that the 64 instances of a wave need about
   * the same number of passes and the wave lives for about their mean instead of the worst of 64 unrelated draws. */
  const int32_t *ord_cnt, *ord_list;
  int64_t ord_ld;
};

/* What a build of mpc_solve_kernel gets on top of MpcPhase is composed of four parts (the fourth, HORIZON, further down), and
 * MpcPhaseOf<ROLL, WARM, MODEL, HORIZON> inherits exactly the parts its build reads; MpcPhaseOf<false, false, false> is MpcPhase
 * itself, so the kernel arguments of the builds without any of them are what they were.
 *
 * WARM (the mpc_*_warm entry points; the warm rollouts): mpc::WarmCall, the warm buffers addressed by INSTANCE at both ends --
 * quantity-major, so neighbouring lanes coalesce like every other array at the ABI, and lane compaction may move an instance between
 * the two.  A lane reads its instance's column (and its status) when it takes the instance and writes them when it has finished it.
 *
 * MODEL (the mpc_*_model entry points): the model values of every instance, [MPC_NMODEL][ld_model] doubles addressed by INSTANCE
 * like the inputs -- a lane reads its instance's six values wherever it runs set-up for it (the take, an instance that lane
 * compaction has moved) and when it writes the instance out, so the column follows the instance from lane to lane.  These builds
 * are launched as one single phase without cuts and deferred tails (a parked or deferred instance would have to carry its column
 * along).  Also the last argument of the MODEL builds of the wave kernel and of the run() kernels. */
struct MpcModelPart {
  const double *model;
  int64_t ld_model;               /* its own leading dimension: run() solves from the handle's rows, the columns stay the caller's (a rollout: ld) */
};

/* ROLL (mpc_rollout_batch_device_fused): a lane keeps the car it has taken for `steps` solves.  Everything the launch writes AND
 * reads again goes through the pointers below -- the car's state, its status and its iterations here, its warm column (warm_in ==
 * warm_out) in the warm part -- and none of them is const or __restrict__: the lane that has written a value is the one that reads
 * it back, in program order.  The kernel's own state / out / status / iters arguments are not dereferenced in these builds. */
struct MpcRollPart {
  int32_t steps;
  double *hist;                   /* [steps][9][ldo], or the handle's 9 scratch rows with hist_step = 0 */
  int64_t hist_step;              /* doubles from one step's 9 rows to the next */
  double *state;                  /* [6][ld]: read at every step, the next state written in place */
  int32_t *status, *iters;        /* per car: worst status, summed iterations (iters may be nullptr) */
};

/* HORIZON (the mpc_*_horizon entry points): the horizon of every instance, [ld] int32 addressed by INSTANCE like the model values,
 * and read in the same places -- wherever a lane runs set-up for an instance -- so it follows the instance from lane to lane.  These
 * builds are MODEL builds with one more part; their `model` may be nullptr (the handle's own six values). */
struct MpcHorizonPart {
  const int32_t *horizon;         /* nullptr (a budget call without horizons): the handle's N for every instance */
  /* the iteration budget of every instance (the mpc_*_budget entry points), [ld] int32 addressed and read like `horizon`, or nullptr:
   * one more pointer of the per-lane-rows builds, which hand it to set-up in the instance's mpc::HorizonColumn; the rules are
   * mpc::Solver's ("iteration budget").  budget != nullptr also widens the warm rule (mpc::warm_status_ok). */
  const int32_t *budget = nullptr;
};

/* DRIVE (mpc_drive_batch_device_fused): a ROLL build whose car follows a track.  Between two solves the lane runs, for its own car
 * and through the car's own columns of the arrays below, what the stepwise loop runs in five launches: the window (mpc::drive_window),
 * the handler's pre-solve half (mpc::run_pre_instance<true>) at the take and at every hand-over with steps left, and at a finished
 * step the post-solve half (mpc::run_post_instance) and plant, summary and record (mpc::drive_step_instance).  The solve reads its
 * state, coefficients and psi box from the rows of `pre` this lane has just written, so none of these pointers is const or
 * __restrict__, and the kernel's own state / coeffs / yaw_lo / yaw_hi arguments are not dereferenced in these builds.  steps, status
 * and iters are the roll part's; the kernel's ld is the stride of pre and of the weights, ldo the caller's leading dimension.
 * With MODEL (mpc_drive_batch_device_fused_model): the car's column of T.model -- the caller's array, rows T.ld_model = ldo apart -- is
 * read by instance index at the take (the pre-solve half, set-up) and again at the hand-over (unpack, the post-solve half, the plant);
 * it is not carried across the sweeps.
 * With HORIZON (mpc_drive_batch_device_fused_horizon; a MODEL build by construction): the car's horizon is read by instance index in the
 * same two places, through instance_column; T.model may be nullptr there, and drive_model_vals then hands the handle's own six values
 * to the handler's halves and the plant.  These two builds are not staged and address their rows per lane, like every HORIZON build.
 * latency (mpc_drive_batch_device_fused_latency): the car's column of [MPC_NLATENCY][ldo], or nullptr -- the call's own extra_latency and
 * substep counts, the very values the builds read before this pointer existed.  Read like the model column: by instance index at the
 * take (what the pre-solve half compensates for) and again at the hand-over (the plant's counts), and not carried in between.  A
 * pointer, not a template argument: the lane kernel has the builds it had.
 * plant (mpc_drive_batch_device_fused_plant): the car's column of [MPC_NPLANT][ldo], or nullptr -- the default column, the plant of the
 * forms without.  Read by instance index at the hand-over only, where the plant runs, under the one test mpc::drive_plant_vals_of
 * makes; likewise a pointer and no template argument.
 * latency, model and plant reach the plant the way mpc_drive_plant_kernel hands them on: the car's counts, its mpc::ModelVals and its
 * mpc::DrivePlantVals into the one mpc::drive_step_instance, so the one launch and the stepwise loop move a car with the same code. */
struct MpcDrivePart {
  MpcDriveOpts O;
  double *car;                    /* [6][ldo] in / out */
  const double *track_x, *track_y;
  int32_t n_track;
  double *ptsx, *ptsy, *cmd;      /* [8][ldo], [8][ldo], [2][ldo]: the handle's rows */
  double *pre;                    /* [RUN_PRE_ROWS][ld]: the handle's rows */
  double *out9;                   /* [9][ldo]: the handle's rows */
  double *summary, *rec;          /* [MPC_DRIVE_NSUM][ldo]; hist [steps][MPC_DRIVE_REC][ldo] or nullptr */
  const double *latency;          /* [MPC_NLATENCY][ldo] or nullptr */
  const double *plant;            /* [MPC_NPLANT][ldo] or nullptr */
  /* noise (mpc_drive_batch_device_fused_noise): the car's column of [MPC_NNOISE][ldo], or nullptr -- the zero column.  Read by instance
   * index where the stepwise loop's two kernels read it: at the take, where mpc::drive_seen writes what the handler is told into the
   * car's column of the handle's seen rows ([6][ldo] behind cmd in the handle's drive rows, drive_seen6; with both pointers nullptr the
   * pre-solve half reads the car itself, as it did before these pointers existed) and of this step's block of seen ([steps][4][ldo] or
   * nullptr), and at the hand-over, where mpc::drive_step_instance perturbs the plant column and drops replies.  Pointers, no template
   * argument; the seen rows are found from cmd, not carried as a third pointer (a pointer held across the sweeps costs the build registers). */
  const double *noise = nullptr;
  double *seen = nullptr;
};
/* THE layout of the handle's drive rows (h->d_drive), in rows of ld doubles: the one statement of it, read by drive_rows (the size),
 * both drive forms (the pointers) and the lane kernel (the seen rows, found from cmd).  A new row goes in here and nowhere else. */
struct DriveRows {
  static constexpr int kPtsx = 0, kPtsy = kPtsx + mpc::RUN_MAX_PTS;      /* the window's waypoints, [RUN_MAX_PTS][ld] each */
  static constexpr int kCmd = kPtsy + mpc::RUN_MAX_PTS;                  /* the reply, [2][ld] */
  static constexpr int kIdx = kCmd + 2;                                  /* the stepwise loop's two window-index rows, [2][ld] int32: one row of doubles */
  static constexpr int kComp = kIdx + 1;                                 /* the stepwise loop's comp row of a latency call, [ld] */
  static constexpr int kSeen = kComp + 1;                                /* what the handler is told in a noise call, [6][ld] */
  static constexpr int kRows = kSeen + 6;
  static_assert(2 * sizeof(int32_t) == sizeof(double), "two index rows are one row of doubles");
  double *base;
  int64_t ld;
  __host__ __device__ double *at(int row) const { return base + (int64_t)row * ld; }
  __host__ __device__ double *ptsx() const { return at(kPtsx); }
  __host__ __device__ double *ptsy() const { return at(kPtsy); }
  __host__ __device__ double *cmd() const { return at(kCmd); }
  __host__ __device__ int32_t *idx(int which) const { return (int32_t *)at(kIdx) + (int64_t)which * ld; }
  __host__ __device__ double *comp() const { return at(kComp); }
  __host__ __device__ double *seen6() const { return at(kSeen); }
  static size_t bytes(int64_t ld) { return sizeof(double) * (size_t)kRows * (size_t)ld; }
};
/* the handle's seen rows [6][ld] from the reply rows of the same block (the lane kernel carries cmd, not the block's base) */
__host__ __device__ static inline double *drive_seen6(double *cmd, int64_t ld) { return DriveRows{cmd - (int64_t)DriveRows::kCmd * ld, ld}.seen6(); }

template <bool ON, class Part> struct MpcPartIf : Part {};
template <class Part> struct MpcPartIf<false, Part> {};
template <bool ROLL, bool WARM, bool MODEL, bool HORIZON = false, bool DRIVE = false>
struct MpcPhaseParts : MpcPhase, MpcPartIf<WARM, mpc::WarmCall>, MpcPartIf<ROLL, MpcRollPart>, MpcPartIf<MODEL, MpcModelPart>, MpcPartIf<HORIZON, MpcHorizonPart>,
                       MpcPartIf<DRIVE, MpcDrivePart> {};
template <bool ROLL, bool WARM, bool MODEL, bool HORIZON = false, bool DRIVE = false>
using MpcPhaseOf = std::conditional_t<ROLL || WARM || MODEL || HORIZON, MpcPhaseParts<ROLL, WARM, MODEL, HORIZON, DRIVE>, MpcPhase>;
/* a phase's value from its parts: those the build does not inherit are left out */
template <bool ROLL, bool WARM, bool MODEL, bool HORIZON = false, bool DRIVE = false>
static MpcPhaseOf<ROLL, WARM, MODEL, HORIZON, DRIVE> phase_of(const MpcPhase &T, const mpc::WarmCall &warm, const MpcRollPart &roll, const MpcModelPart &model,
                                                              const MpcHorizonPart &horizon = {}, const MpcDrivePart &drive = {}) {
  MpcPhaseOf<ROLL, WARM, MODEL, HORIZON, DRIVE> X;
  if constexpr (DRIVE) static_cast<MpcDrivePart &>(X) = drive;
  static_cast<MpcPhase &>(X) = T;
  if constexpr (WARM) static_cast<mpc::WarmCall &>(X) = warm;
  if constexpr (ROLL) static_cast<MpcRollPart &>(X) = roll;
  if constexpr (MODEL) static_cast<MpcModelPart &>(X) = model;
  if constexpr (HORIZON) static_cast<MpcHorizonPart &>(X) = horizon;
  return X;
}

/* The take-order key of every instance of a launch (csrc/mpc_take_key.h) and the bins' lists: one thread per instance, a wave
 * appends its instances to the bins' lists.  No LDS and few registers: its waves fit beside the resident waves of a bulk
 * launch.  cnt[] is zero on entry (it lives in the launch's counter block). */
template <class R>
__global__ __launch_bounds__(kBlock) void mpc_take_key_kernel(const float horizon_s, const int64_t B, const int64_t ld, const R *__restrict__ state,
                                                           const R *__restrict__ coeffs, const R *__restrict__ yaw_lo, const R *__restrict__ yaw_hi,
                                                           const int reverse, int32_t *__restrict__ cnt, int32_t *__restrict__ list, const int64_t ld_list) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int b = -1;
  if (i < B) {
    R st[6], cf[MPC_NCOEF];
    float f[mpc::kTakeFeats];
#pragma unroll
    for (int q = 0; q < 6; q++) st[q] = state[q * ld + i];
#pragma unroll
    for (int q = 0; q < MPC_NCOEF; q++) cf[q] = coeffs[q * ld + i];
    mpc::take_key_features<R>(horizon_s, st, cf, yaw_lo[i], yaw_hi[i], f);
    b = mpc::take_key_bin(f);
    if (reverse) b = mpc::kTakeBins - 1 - b;
  }
  /* A wave appends its instances with ONE round of atomics: lane k adds the wave's number of instances of bin k and every lane
   * reads the base of its own bin from it.  (One atomic per bin in turn, each waiting for the one before, made this kernel last
   * 200 us on a device that a bulk launch keeps full -- as long as the ordered launch saves.) */
  const unsigned lane = threadIdx.x & 63u;
  static_assert(mpc::kTakeBins <= 64, "a lane per bin");
  int n_mine = 0, rank = 0;
#pragma unroll
  for (int k = 0; k < mpc::kTakeBins; ++k) {
    const unsigned long long m = __builtin_amdgcn_ballot_w64(b == k);
    if (lane == (unsigned)k) n_mine = __builtin_popcountll(m);
    if (b == k) rank = __builtin_popcountll(m & ((1ull << lane) - 1ull));
  }
  int base = 0;
  if (n_mine > 0) base = atomicAdd(&cnt[lane], n_mine);
  const int64_t at = (int64_t)__shfl(base, b < 0 ? 0 : b, 64) + rank;
  if (b >= 0 && at < ld_list) list[(int64_t)b * ld_list + at] = (int32_t)i;
}

/* Copies between queue entries and a lane's workspace column.  Loads first, then stores, a stage (or 16 rows) at a time: written as
 * `dst[..] = src[..]` in one loop the compiler must assume that a store aliases the next load and waits for every load before the
 * next one goes out -- 200 round trips of ~2 us per entry, which priced a wave's life at +10 % per deferred instance. */
/* One iterate of M stages: the whole record of stage k through load(k, f), then store(k, rec).  The ends: */
template <class R, class Load, class Store>
__device__ __forceinline__ void copy_iterate(int M, Load load, Store store) {
  using FL = mpc::Fields<R>;
  for (int k = 0; k < M; ++k) {
    R rec[FL::IT_SZ];
#pragma unroll
    for (int f = 0; f < FL::IT_SZ; f++) rec[f] = load(k, f);
    store(k, rec);
  }
}
/* ... iterate slot I of a workspace column */
template <class R, class WS>
__device__ __forceinline__ auto column_load(const WS &ws, int I) { return [&ws, I](int k, int f) -> R { return ws.it(k, I, f); }; }
template <class R, class WS>
__device__ __forceinline__ auto column_store(WS &ws, int I) {
  return [&ws, I](int k, const R *rec) { ws.template store_run<0, mpc::Fields<R>::IT_SZ>(k, I, rec); };
}
/* ... entry e's place in the [cap / 64][M][IT_SZ][64] reals of a queue (MpcTailQ.iter, MpcPhase.p_iter) */
template <class R>
__device__ __forceinline__ R *tile_place(void *base, int64_t e, int M) { return (R *)base + (e >> 6) * (int64_t)M * mpc::Fields<R>::IT_SZ * 64 + (e & 63); }
template <class R>
__device__ __forceinline__ auto tile_load(const R *src) { return [src](int k, int f) { return src[(k * mpc::Fields<R>::IT_SZ + f) * 64]; }; }
template <class R>
__device__ __forceinline__ auto tile_store(R *dst) {
  return [dst](int k, const R *rec) {
#pragma unroll
    for (int f = 0; f < mpc::Fields<R>::IT_SZ; f++) dst[(k * mpc::Fields<R>::IT_SZ + f) * 64] = rec[f];
  };
}
__device__ __forceinline__ void rows_copy(double *__restrict__ dk, int64_t dl, const double *__restrict__ pk, int64_t lp, int q0, int q1) {
  for (int q = q0; q < q1; q += 16) {
    double t[16];
#pragma unroll
    for (int e = 0; e < 16; e++) t[e] = q + e < q1 ? pk[(q + e) * lp] : 0.0;
#pragma unroll
    for (int e = 0; e < 16; e++) if (q + e < q1) dk[(q + e) * dl] = t[e];
  }
}

/* what Solver::unpack writes through when the arrays at the ABI are of another type than the solver's reals */
template <class RIO, class R> struct OutRef {
  RIO *p;
  __device__ __host__ void operator=(R v) const { *p = (RIO)v; }
};

/* The column argument of Solver::setup / unpack for instance i in the build at hand (mpc::NoColumn, ModelColumn, HorizonColumn).
 * The only place that knows where the model values lie: a rollout's columns are the caller's, rows ld apart like its inputs; a
 * solve's have T.ld_model (MpcModelPart), and so have a drive's (its ld is the stride of the handle's rows, the columns stay the
 * caller's). */
template <bool ROLL, bool MODEL, bool HORIZON, bool DRIVE = false, class Phase>
__device__ __forceinline__ auto instance_column(const MpcParams &P, const Phase &T, int64_t ld, int64_t i) {
  (void)P;
  if constexpr (MODEL) {
    int64_t lm = ld;
    if constexpr (!ROLL || DRIVE) lm = T.ld_model;
    if constexpr (HORIZON) return mpc::HorizonColumn{T.model ? T.model + i : nullptr, lm, T.horizon ? T.horizon[i] : P.N, T.budget ? T.budget[i] : (int)mpc::kNoBudget};
    else return mpc::ModelColumn{T.model + i, lm};
  } else return mpc::NoColumn{};
}
/* ... and the same column as the values mpc_run_core.h and mpc_drive_core.h read (DRIVE builds): the handle's MpcParams itself without
 * MODEL, so that those builds read every field from P where it is used */
template <bool MODEL, bool HORIZON = false, class Phase>
__device__ __forceinline__ decltype(auto) drive_model_vals(const MpcParams &P, const Phase &T, int64_t i) {
  if constexpr (HORIZON) return T.model ? mpc::model_vals_of(P, T.model, T.ld_model, i) : mpc::ModelVals::of(P);      /* (a horizon call's `model` may be nullptr: the handle's six values) */
  else if constexpr (MODEL) return mpc::model_vals_of(P, T.model, T.ld_model, i);
  else return (P);
}

/* Instance i, which this lane has taken as far as the phase goes, is appended to the list of the next phase: its index, this lane's
 * column (where its iterate is, unless the caller copies it out) and the solver's scalars; row 35 says whether the next phase
 * continues the iterate (clean) or solves the instance from the start point (from_scratch).  Returns the list position. */
template <class SV>
__device__ __forceinline__ int64_t park_for_next_phase(const MpcPhase &T, const SV &S, int64_t i, int attempt, int it_total, bool from_scratch) {
  const int64_t pos = (int64_t)atomicAdd(T.n_out, 1);
  T.out_inst[pos] = (int32_t)i;
  T.out_src[pos] = (int32_t)(blockIdx.x * 64u + threadIdx.x);
  double *pk = T.out_park + pos;
  const int64_t lp = T.ld_park;
  S.park([pk, lp](int q) -> double & { return pk[q * lp]; }, attempt, it_total);
  pk[35 * lp] = from_scratch ? 1.0 : 0.0;
  return pos;
}

/* RIO: the type of the arrays at the ABI (inputs, outputs); R: the solver's.  They differ only in the fp64 phase of a
 * mixed-precision solve on an MPC_PRECISION_F32 handle (RIO = float, R = double).  RSRC: the reals of the workspace a
 * promote_in phase takes its iterates from. */
/* ROLL (mpc_rollout_batch_device_fused): a lane keeps the car it has taken for T.steps solves.  At the hand-over point a finished
 * solve of step t goes to row block t of T.hist, its rows 0..5 become the car's state, status and iterations are folded into the
 * car's (mpc::RolloutCar), and -- WARM -- the final iterate goes to the car's warm column; with steps left the lane then takes the
 * SAME car again instead of asking the counter: set-up from the state it has just stored and a cold start, or, WARM and the step
 * succeeded, warm_point() on its own column and begin_warm() -- the code the take runs for a fresh instance.  Step 0 is cold.
 * Exit: a lane with steps left holds its car as `have` (solving) or `fin` (a finished or rejected step waiting for the hand-over),
 * so the wave stays; every pass advances a solve (bounded by max_iter and the one restart), a step (a car has T.steps of them)
 * or consumes the counter.  These builds are launched without lane compaction, cuts and deferred tails (the step index lives in
 * the lane's registers and does not travel). */
/* MODEL (the mpc_*_model entry points): every set-up and the hand-over read dt, Lf and the four limits from the instance's column of
 * T.model instead of P (Solver::setup / unpack with the mpc::ModelColumn of instance_column), by instance index and outside the sweeps;
 * nothing else differs.  With WARM: warm_point() judges a record against the relaxed box that set-up has just set from the column, and the cold solve
 * that follows a refused record or a failed warm attempt starts from the solver's own members -- no set-up in between.  With ROLL:
 * the car taken again is set up from its column like a fresh one, and the hand-over of a step projects into the column's limits. */
/* HORIZON (the mpc_*_horizon entry points): a MODEL build in which every set-up also reads the instance's horizon n from T.horizon
 * (an mpc::HorizonColumn: M = n - 1 stages) and `model` may be nullptr.  The lanes of a wave then differ in their number of stages,
 * so these builds are not staged and address their rows per lane (TiledWorkspace<false, R, true>): every sweep is an ordinary
 * divergent loop, a lane leaves it after its own M stages, and a pass of the wave costs the longest horizon among its running lanes.
 * Their dynamic LDS is the mailbox of lane compaction alone.  A moved instance is set up again from its index, horizon included. */
template <bool STAGING, class R, class RIO = R, class RSRC = RIO, bool SOC = false, bool WARM = false, bool ROLL = false, bool MODEL = false,
          bool HORIZON = false, bool DRIVE = false>
__global__ __launch_bounds__(kBlock, 1) void mpc_solve_kernel(
    const MpcParams P, const int64_t B, const int64_t ld, const int64_t ldo, const RIO *__restrict__ state,
    const RIO *__restrict__ coeffs, const RIO *__restrict__ yaw_lo, const RIO *__restrict__ yaw_hi,
    const RIO *__restrict__ weights, RIO *__restrict__ out, RIO *__restrict__ traj,
    int32_t *__restrict__ status, int32_t *__restrict__ iters, R *__restrict__ wsbase,
    const int64_t tile_reals,
    const MpcPhaseOf<ROLL, WARM, MODEL, HORIZON, DRIVE> T) {
  extern __shared__ double smem[];
  static_assert(!DRIVE || (ROLL && !SOC), "track driving: a ROLL build without SOC");
  static_assert(!HORIZON || (MODEL && !STAGING && !SOC), "per-instance horizon: a MODEL build without staging and SOC");
  static_assert(!WARM || (sizeof(R) == 8 && std::is_same<R, RIO>::value && std::is_same<R, RSRC>::value && !SOC), "warm start: the plain fp64 solve only");
  static_assert(!ROLL || (sizeof(R) == 8 && std::is_same<R, RIO>::value && std::is_same<R, RSRC>::value && !SOC), "fused rollout: the plain fp64 solve only");
  static_assert(!MODEL || (sizeof(R) == 8 && std::is_same<R, RIO>::value && std::is_same<R, RSRC>::value), "per-instance model values: the fp64 solve only");
  using WS = std::conditional_t<SOC, mpc::TiledSocWorkspace<STAGING, R>, mpc::TiledWorkspace<STAGING, R, HORIZON>>;
  using SV = mpc::Solver<WS, R, 0, SOC>;
  using FL = mpc::Fields<R>;
  static_assert(SV::PARK_N == kParkRows, "park buffer rows");
  WS ws;
  ws.tile = (typename WS::greal *)(wsbase + (int64_t)blockIdx.x * tile_reals);
  if constexpr (SOC) ws.soc_tile = (typename WS::greal *)((R *)T.soc_ws + (int64_t)blockIdx.x * (P.N - 1) * FL::SOC_SZ * 64);
  ws.lane = threadIdx.x;
  ws.lbuf = (typename WS::lreal *)smem;
  if (T.zero_next && blockIdx.x == 0 && threadIdx.x < kCounterInts) T.zero_next[threadIdx.x] = 0;
  SV S(P, ws);
  if (T.promote_out) S.promote_mu = (R)P.mixed_switch_mu;
  int64_t i = 0;
  bool have = false, more = true, fin = false;   /* holds a running instance / may still get one / holds a finished one */
  bool queue_full = false;                       /* deferred tails: the batch's queue slot has no room left */
  bool col_busy = false;                         /* this lane's column holds a parked iterate */
  int attempt = 0, it_total = 0, passes = 0, fin_status = 0, waited = 0, cooldown = 0;
  int step = 0;                                  /* ROLL: solves of car i finished so far */
  int drive_k = 0, drive_k_prev = 0;             /* DRIVE: the window index of the car's current step and of the one before */
  (void)drive_k; (void)drive_k_prev;
  const int64_t n_work = T.resume ? (int64_t)*T.n_in : B;
  (void)col_busy; (void)cooldown; (void)step;
  for (;;) {
#if defined(__HIP_DEVICE_COMPILE__)
    /* ---- lane compaction, part 1: is it worth it now?  (see MpcPhase.compact_gap) ---- */
    bool want_compact = false;
    int cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0}, g_min = 0;
    if ((STAGING || HORIZON) && T.compact_gap > 0) {
      if (MPC_WAVE_ANY(more) && (int64_t)__hip_atomic_load(T.take, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= n_work) more = false;
      if (!MPC_WAVE_ANY(more)) {
        if (cooldown > 0) --cooldown;
        else {
          const unsigned long long live = __builtin_amdgcn_ballot_w64(have);
          const int nl = __builtin_popcountll(live);
          int g_now = 0;
#pragma unroll
          for (int g = 0; g < 8; g++) { cnt[g] = __builtin_popcountll((live >> (8 * g)) & 0xffull); g_now += cnt[g] > 0 ? 1 : 0; }
          g_min = (nl + 7) >> 3;
          want_compact = nl > 0 && g_now - g_min >= T.compact_gap;
        }
      }
    }
#else
    const bool want_compact = false;
#endif
    /* ---- hand-over point (wave-uniform decision, see MpcPhase) ---- */
    const int n_wait = MPC_WAVE_COUNT(fin || (!have && more));
    if (n_wait > 0) {
      if (!MPC_WAVE_ANY(have) || n_wait >= T.refill_min || waited >= T.refill_wait || want_compact) {
        waited = 0;
        if (fin && fin_status <= kFinPromote) {
          /* mixed precision, promoted iterates in their own buffer: the hand-over to the next phase happens here, for all the
           * lanes of the wave that are waiting for it at once (done lane by lane as they promote it cost 20 % of the rate) */
          const int64_t pos = park_for_next_phase(T, S, i, attempt, it_total, fin_status != kFinPromote);
          if (fin_status == kFinPromote) {
            ws.stage_drain();                          /* the trial sweep's stores of this wave have landed */
            copy_iterate<R>(P.N - 1, column_load<R>(ws, S.cur ? FL::IT1 : FL::IT0), tile_store(tile_place<R>(T.p_iter, pos, P.N - 1)));
          }
          fin = false;
        }
        bool again = false, again_warm = false;   /* ROLL: this lane goes on with the next step of its car / and may start it warm */
        if constexpr (ROLL) {
          if (fin) {
            using Car = mpc::RolloutCar;
            if constexpr (DRIVE) {
              /* the solve's nine rows, then what the post kernel and the plant-and-summary kernel do for this car */
              double *o = T.out9 + i;
              const int64_t l = ldo;
              const R ylo = (R)T.pre[mpc::RUN_PRE_YAW_LO * ld + i], yhi = (R)T.pre[mpc::RUN_PRE_YAW_HI * ld + i];
              S.unpack(instance_column<ROLL, MODEL, HORIZON, DRIVE>(P, T, ld, i), [o, l](int q) { return OutRef<RIO, R>{o + q * l}; },
                       [](int) { return OutRef<RIO, R>{nullptr}; }, false, ylo, yhi);
              if constexpr (WARM) {
                double *wo = T.warm_out + i;
                const int64_t lw = T.ld_warm;
                S.warm_store([wo, lw](int k, int f, R v) { wo[(int64_t)(k * MPC_WARM_REC + f) * lw] = v; });
              }
              /* (MODEL: the car's column, read again here -- it is not carried across the sweeps) */
              const auto &mv = drive_model_vals<MODEL, HORIZON>(P, T, i);
              mpc::run_post_instance(P, mv, i, T.pre, ld, T.out9, ldo, (double *)nullptr, T.cmd, ldo);
              int sub_old = T.O.sub_old, sub_new = T.O.sub_new;
              if (T.latency) {
                const mpc::DriveLatency dl = mpc::drive_latency_of(T.O, T.latency, ldo, i);
                sub_old = dl.sub_old; sub_new = dl.sub_new;
              }
              mpc::drive_step_instance(P, mv, mpc::drive_plant_vals_of(P, mv, T.plant, ldo, i), mpc::drive_noise_of(T.noise, ldo, i), T.O, sub_old, sub_new, i, ldo, step, T.n_track, T.car, T.cmd, T.pre, ld,
                                       fin_status, S.iters + it_total, drive_k, drive_k_prev, T.summary, T.rec ? T.rec + (int64_t)step * MPC_DRIVE_REC * ldo : nullptr, T.status, T.iters);
            } else {
            double *o = T.hist + (int64_t)step * T.hist_step + i;
            const int64_t l = ldo;
            const R ylo = (R)yaw_lo[i], yhi = (R)yaw_hi[i];
            /* (MODEL: the car's own limits, from its column) */
            S.unpack(instance_column<ROLL, MODEL, HORIZON>(P, T, ld, i), [o, l](int q) { return OutRef<RIO, R>{o + q * l}; },
                     [](int) { return OutRef<RIO, R>{nullptr}; }, false, ylo, yhi);
            double *sp = T.state + i;
            const int64_t ls = ld;
            Car::next_state([o, l](int q) { return o[q * l]; }, [sp, ls](int q, double v) { sp[q * ls] = v; });
            int32_t worst = 0, sum = 0;
            if (step > 0) worst = T.status[i];
            T.status[i] = Car::fold_status(step, worst, fin_status);
            if (T.iters) {
              if (step > 0) sum = T.iters[i];
              T.iters[i] = Car::sum_iters(step, sum, S.iters + it_total);
            }
            if constexpr (WARM) {
              double *wo = T.warm_out + i;
              const int64_t lw = T.ld_warm;
              S.warm_store([wo, lw](int k, int f, R v) { wo[(int64_t)(k * MPC_WARM_REC + f) * lw] = v; });
            }
            }
            ++step;
            again = step < T.steps;
            bool budgeted = false;                 /* (a budget call: a step that stopped at its budget hands its iterate on, mpc::warm_status_ok) */
            if constexpr (HORIZON) budgeted = T.budget != nullptr;
            again_warm = WARM && again && Car::starts_warm(step, fin_status, budgeted);
            if (!again) step = 0;                  /* the car is done: the lane is free for whatever the counter still has */
            fin = false;
          }
        }
        if (fin) {
          RIO *o = out + i;
          RIO *t = traj ? traj + i : nullptr;
          const int64_t l = ldo;
          const R ylo = (R)yaw_lo[i], yhi = (R)yaw_hi[i];
          S.unpack(instance_column<ROLL, MODEL, HORIZON>(P, T, ld, i), [o, l](int q) { return OutRef<RIO, R>{o + q * l}; },
                   [t, l](int q) { return OutRef<RIO, R>{t + q * l}; }, traj != nullptr, ylo, yhi);
          if constexpr (WARM) {
            /* the final iterate, whatever the status (the caller's next solve looks at the status) */
            if (T.warm_out) {
              double *wo = T.warm_out + i;
              const int64_t lw = T.ld_warm;
              S.warm_store([wo, lw](int k, int f, R v) { wo[(int64_t)(k * MPC_WARM_REC + f) * lw] = v; });
            }
          }
          status[i] = fin_status;
          if (iters) iters[i] = S.iters + it_total;
          fin = false;
        }
        bool exhausted = false;
        if ((!have && more) || again) {
          int64_t pos = i;                         /* (ROLL, the same car again: the counter is not asked) */
          if (!again) {
            pos = (int64_t)atomicAdd(T.take, 1);
            more = pos < n_work;
            exhausted = !more;
          }
          if (more || again) {
            if (!again) i = T.resume ? (int64_t)T.in_inst[pos] : pos;
            if (__builtin_expect(T.ord_list != nullptr && !again, 0)) {     /* (placed out of line: the code around the take stays where it was) */
              /* the bins laid end to end: which bin holds position pos (the counts are the same for every lane: scalar loads) */
              int64_t off = pos;
              int b = 0;
#pragma unroll 1
              for (; b < mpc::kTakeBins - 1; ++b) {
                const int64_t c = (int64_t)T.ord_cnt[b];
                if (off < c) break;
                off -= c;
              }
              i = (int64_t)T.ord_list[(int64_t)b * T.ord_ld + (off < T.ord_ld ? off : 0)];
              if ((uint64_t)i >= (uint64_t)B) i = pos;     /* (cannot happen: the lists hold 0 .. B-1 once each; results never go out of bounds) */
            }
            R st[6], cf[MPC_NCOEF], w[MPC_NW];
            R ylo_in, yhi_in;
            if constexpr (DRIVE) {
              /* the car as it stands: its window, the handler's pre-solve half into the car's column of `pre`, and the solve's inputs from there */
              drive_k_prev = drive_k;
              drive_k = mpc::drive_window(T.track_x, T.track_y, T.n_track, T.car[i], T.car[ldo + i]);
              mpc::drive_window_points(T.track_x, T.track_y, T.n_track, drive_k, T.O.npts, T.ptsx, T.ptsy, ldo, i);
              mpc::RunComp lc{false, T.O.extra_latency};
              if (T.latency) lc = mpc::RunComp{true, mpc::drive_latency_of(T.O, T.latency, ldo, i).comp};
              /* (a noise call: the handler is told the car's column of seen6, written here from the car and this message's draw) */
              const double *tel = T.car;
              if (T.noise || T.seen) {
                double *seen6 = drive_seen6(T.cmd, ldo);
                mpc::drive_seen(mpc::drive_noise_of(T.noise, ldo, i), step, T.car, ldo, i, seen6, ldo, T.seen ? T.seen + (int64_t)step * 4 * ldo : nullptr);
                tel = seen6;
              }
              (void)mpc::run_pre_instance<true>(P, drive_model_vals<MODEL, HORIZON>(P, T, i), i, ldo, T.O.npts, tel, lc, T.ptsx, T.ptsy, T.pre, ld);
              mpc::gather_instance(P, i, ld, T.pre + mpc::RUN_PRE_STATE * ld, T.pre + mpc::RUN_PRE_COEFFS * ld, weights, st, cf, w);
              ylo_in = (R)T.pre[mpc::RUN_PRE_YAW_LO * ld + i]; yhi_in = (R)T.pre[mpc::RUN_PRE_YAW_HI * ld + i];
            } else {
              const RIO *sp = state;
              if constexpr (ROLL) sp = T.state;      /* the car's state as it stands: the start state, or the six doubles this lane stored at the step before */
              mpc::gather_instance(P, i, ld, sp, coeffs, weights, st, cf, w);
              ylo_in = (R)yaw_lo[i]; yhi_in = (R)yaw_hi[i];
            }
            const R ylo = ylo_in, yhi = yhi_in;
            const bool from_scratch = T.promote_in && T.in_park[pos + 35 * T.ld_park] != 0.0;   /* the fp32 phase gave up on it */
            bool warm = false, warm_cand = false;   /* WARM: this instance has a valid column in warm_in / starts from it */
            if constexpr (WARM && ROLL) warm_cand = again_warm;   /* (the column this lane stored when it finished the step before) */
            else if constexpr (WARM && HORIZON) warm_cand = T.warm_in != nullptr && (T.warm_status == nullptr || mpc::warm_status_ok(T.warm_status[i], T.budget != nullptr));
            else if constexpr (WARM) warm_cand = T.warm_in != nullptr && (T.warm_status == nullptr || T.warm_status[i] == MPC_STATUS_SUCCESS);
            const int s0 = S.setup(instance_column<ROLL, MODEL, HORIZON, DRIVE>(P, T, ld, i), st, cf, ylo, yhi, w, (!T.resume || from_scratch) && !warm_cand);
            if constexpr (WARM) {
              if (warm_cand) {
                if (s0 == MPC_STATUS_SUCCESS) {
                  const bool box = T.psi_box != 0;
                  warm = S.warm_point(mpc::WarmColumn{T.warm_in + i, T.ld_warm, box ? (double)ylo : -HUGE_VAL, box ? (double)yhi : HUGE_VAL}, T.wopts);
                }
                if (!warm) S.start_point();     /* set-up left slot 0 to the warm point, and the column holds no iterate of this NLP */
              }
            }
            if constexpr (WARM) {
              /* attempt -1: should the warm attempt end in anything but SUCCESS, the instance is solved again the way a cold solve
               * starts -- the convention of an iterate handed over by the fp32 phase, below */
              if (warm) { S.begin_warm(T.wopts); attempt = -1; it_total = 0; passes = 0; have = true; }
            }
            if (warm) {
            } else if (T.promote_in && s0 != MPC_STATUS_SUCCESS) {
              /* a start state that the fp32 set-up let through (outside the relaxed bounds by less than the fp32 spacing) and this
               * solver's set-up rejects: the verdict of the single-phase solve, the start point reported */
              S.start_point();
              S.cur = 0; S.E.f = R(0.0);
              it_total = 0; S.iters = 0; fin = true; fin_status = s0;
            } else if (from_scratch) { S.begin(true); attempt = 0; it_total = (int)T.in_park[pos + 23 * T.ld_park] + (int)T.in_park[pos + 29 * T.ld_park]; passes = 0; have = true; }   /* (the fp32 phase's iterations count) */
            else if (T.resume) {
              /* bring the parked iterate over: the column (src wave, src lane) of phase A's workspace -> own column */
              const double *pk = T.in_park + pos;
              const int64_t lp = T.ld_park;
              S.unpark([pk, lp](int q) -> double { return pk[q * lp]; }, attempt, it_total);
              const int src = T.in_src[pos];
              const int I = S.cur ? FL::IT1 : FL::IT0;
              if (T.promote_in) {
                /* the iterate as the fp32 phase left it: its record layout, its tile size; then this solver's own evaluation */
                using FS = mpc::Fields<RSRC>;
                mpc::TiledWorkspace<false, RSRC> wsrc;
                wsrc.tile = (typename mpc::TiledWorkspace<false, RSRC>::greal *)((const RSRC *)T.src_ws + (int64_t)(src >> 6) * T.src_tile_reals);
                wsrc.lane = src & 63; wsrc.lbuf = nullptr;
                const int Is = S.cur ? FS::IT1 : FS::IT0;
                const RSRC *pit = T.p_iter ? (const RSRC *)T.p_iter + (pos >> 6) * (int64_t)(P.N - 1) * FS::IT_SZ * 64 + (pos & 63) : nullptr;
                for (int k = 0; k < P.N - 1; ++k) {
                  R rec[FL::IT_SZ] = {};
                  mpc::convert_iterate_record<RSRC, R>([&](int f) { return pit ? pit[(k * FS::IT_SZ + f) * 64] : (RSRC)wsrc.it(k, Is, f); }, [&](int f, R v) { rec[f] = v; });
                  ws.template store_run<0, FL::IT_SZ>(k, I, rec);
                  /* the re-evaluation is a trial sweep with step length 0: it multiplies whatever the direction record holds */
                  const R zero[FL::D_N] = {};
                  ws.template store_run<FL::F_D, FL::D_N>(k, 0, zero);
                }
                S.promoted();
                attempt = -1;      /* came in from the fp32 phase: should it fail, it is solved again the way the single-phase solve starts */
              } else {
                WS wsrc = ws;
                wsrc.tile = (typename WS::greal *)((const R *)T.src_ws + (int64_t)(src >> 6) * tile_reals);
                wsrc.lane = src & 63;
                copy_iterate<R>(P.N - 1, column_load<R>(wsrc, I), column_store<R>(ws, I));
              }
              passes = 0; have = true;
            } else if (s0 == MPC_STATUS_SUCCESS) { S.begin(true); attempt = 0; it_total = 0; passes = 0; have = true; }
            else { it_total = 0; S.iters = 0; fin = true; fin_status = s0; }   /* rejected at set-up (initial state outside its own
                                                                               * bounds): the start point is reported at the next hand-over */
          }
        }
        /* The counter only grows: what one lane found empty is empty for all.  (Until then a finished lane does take again,
         * also in a launch that has a lane for every instance: with batches in flight the last waves of a grid start late,
         * and the lanes that finish early in its first waves take their instances -- those waves then find nothing and leave.
         * Declaring the counter exhausted after every lane's first take was measured: -6 % on the headline.) */
        if (MPC_WAVE_ANY(exhausted)) more = false;
      } else ++waited;
    }
#if defined(__HIP_DEVICE_COMPILE__)
    /* ---- lane compaction, part 2 (finished lanes have just been served: their columns are free) ---- */
    if (want_compact) {
      unsigned long long keep = 0;               /* the g_min fullest groups stay where they are */
      for (int t = 0; t < g_min; ++t) {
        int best = 0, bc = -1;
#pragma unroll
        for (int g = 0; g < 8; g++) if (!((keep >> (8 * g)) & 1ull) && cnt[g] > bc) { bc = cnt[g]; best = g; }
        keep |= 0xffull << (8 * best);
      }
      const bool in_keep = (keep >> threadIdx.x) & 1ull;
      const bool movable = have && S.phase == SV::PH_DIR && !in_keep;
      const bool is_free = !have && !fin && !col_busy && in_keep;
      const unsigned long long mv = __builtin_amdgcn_ballot_w64(movable), fr = __builtin_amdgcn_ballot_w64(is_free);
      const int n_mv = __builtin_popcountll(mv), n_fr = __builtin_popcountll(fr);
      const int n = n_mv < n_fr ? n_mv : n_fr;
      if (n > 0) {
        ws.stage_drain();                        /* the trial sweep's stores have landed, the staging buffers are idle */
        static_assert(!STAGING || staging_lds_bytes<R>() >= (size_t)kParkRows * 64 * sizeof(R) + 2 * 64 * sizeof(int), "the mailbox must fit the staging buffers");      /* (HORIZON builds: launched with exactly the mailbox, kMailboxBytes) */
        R *mb = (R *)smem;                       /* [kParkRows][64]: Solver::park scalars (in the solver's own precision) ... */
        int *mi = (int *)(mb + kParkRows * 64);  /* ... [2][64]: instance, passes */
        const unsigned long long below = (1ull << threadIdx.x) - 1ull;
        const bool is_src = movable && __builtin_popcountll(mv & below) < n;
        const int my_f = __builtin_popcountll(fr & below);
        const bool is_dst = is_free && my_f < n;
        if (is_src) {
          const unsigned ln = threadIdx.x;
          S.park([mb, ln](int q) -> R & { return mb[q * 64 + ln]; }, attempt, it_total);
          mi[ln] = (int)i; mi[64 + ln] = passes;
          have = false;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if constexpr (HORIZON) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      /* (not staged: stage_drain() above is empty, and a lane is about to read another lane's column) */
        if (is_dst) {
          unsigned long long m = mv;
          for (int r = 0; r < my_f; ++r) m &= m - 1ull;
          const int src = __builtin_ctzll(m);
          i = (int64_t)mi[src]; passes = mi[64 + src];
          R st[6], cf[MPC_NCOEF], w[MPC_NW];
          mpc::gather_instance(P, i, ld, state, coeffs, weights, st, cf, w);
          const R ylo = (R)yaw_lo[i], yhi = (R)yaw_hi[i];
          /* (the instance has changed lanes: its column and its horizon, if it has any, come with it) */
          (void)S.setup(instance_column<ROLL, MODEL, HORIZON>(P, T, ld, i), st, cf, ylo, yhi, w, false);
          S.unpark([mb, src](int q) -> R { return mb[q * 64 + src]; }, attempt, it_total);
          const int I = S.cur ? FL::IT1 : FL::IT0;
          WS wsrc = ws;
          wsrc.lane = src;
          /* (plain loads: the column was written through this CU's own L1 by a lane of this wave, and stage_drain() has waited
           * for the stores; keeping two stages in flight was measured: no difference) */
          int n_rec = P.N - 1;
          if constexpr (HORIZON) n_rec = S.M;      /* (the instance's own stages; set-up above has read its horizon) */
          copy_iterate<R>(n_rec, column_load<R>(wsrc, I), column_store<R>(ws, I));
          have = true;
        }
        __builtin_amdgcn_wave_barrier();
        cooldown = T.compact_cooldown;
      }
    }
#endif
    if (!MPC_WAVE_ANY(have || more || fin)) break;
    const bool few = T.tail_few > 0 && !MPC_WAVE_ANY(more) && MPC_WAVE_COUNT(have) <= T.tail_few;
    if (have) {
      const int r = S.step();
      ++passes;
      /* Mixed precision.  Only a CLEAN hand-over is continued by the fp64 solver (the fp32 phase reached the switch value of the
       * barrier parameter, or tol_f32).  One that comes out of trouble -- the iteration allowance used up, line search or inertia
       * correction out of single precision, not-a-number -- sends the instance to the fp64 solver FROM THE START POINT (row 35 of
       * the parked scalars): on hard instances the fp32 iterates lead into other local minima than the fp64 ones (SURVEY's
       * unfiltered populations: 7 of 32 768 at N = 25, 24 of 65 536 at N = 10 with the old rule; none with this one). */
      if ((r == SV::MPC_PROMOTE || (T.promote_out && r == MPC_STATUS_NUMERIC)) && T.p_iter) {
        /* mixed precision: this phase has taken the instance as far as it is asked to; it waits for the wave's next hand-over */
        fin = true; fin_status = (r == SV::MPC_PROMOTE && S.promote_clean) ? kFinPromote : kFinScratch; have = false;
      } else if (r == SV::MPC_PROMOTE || (T.promote_out && r == MPC_STATUS_NUMERIC)) {
        /* the same with the iterate left in its column (MpcParams.f32_phase_refill = 0): the next phase's solver takes over.
         * Not-a-number in the fp32 phase (states far from the origin late in a closed loop: x^4 terms, lost digits) is not a
         * verdict on the instance: the fp64 solver gets it from the start point (row 35 of the parked scalars says so). */
        (void)park_for_next_phase(T, S, i, attempt, it_total, !(r == SV::MPC_PROMOTE && S.promote_clean));
        have = false; more = false; col_busy = true;     /* the column keeps the parked iterate: this lane takes nothing else */
      } else if (r != SV::MPC_RUNNING) {
        /* The restart rule (Solver::next_attempt): the stand-in for IPOPT's restoration phase -- once more from the start point,
         * zero multipliers -- and, before it, the instance the fp32 phase started (attempt -1) and the fp64 phase could not finish
         * (1-3 of 8 192 at N = 25: the line search fails from where fp32 left it): it is solved again from the start point exactly
         * as the single-phase solve does it -- first attempt, then the restart if that fails -- so status AND returned point are
         * that solve's (the named hard instances of tests/helpers.py stay what the oracle says).  Trying the restart first is
         * cheaper for these stragglers (their chain: fp32 + the failed fp64 continuation + a whole solve) but was measured to return
         * the restart's local minimum, or its last iterate, where the single-phase solve returns the first attempt's. */
        if (!S.next_attempt(r, attempt, it_total)) { fin = true; fin_status = r; have = false; }
      } else if (T.tail_cut > 0 && (passes >= T.tail_cut || (few && passes >= T.tail_few_from)) && S.phase == SV::PH_DIR && !queue_full) {
        const int pos = atomicAdd(T.tq.count, 1);
        if (pos >= T.tq.cap) queue_full = true;     /* it finishes here, and so does whatever else this lane takes */
        else {
          double *pk = T.tq.park + pos;
          const int64_t lp = T.tq.cap;
          S.park([pk, lp](int q) -> double & { return pk[q * lp]; }, attempt, it_total);
          pk += kParkRows * lp;
          {
            double in[kTailInRows];      /* state, coefficients, psi box, weights: the rows mpc_tail_slice_kernel gathers from */
            mpc::gather_instance(P, i, ld, state, coeffs, weights, in, in + 6, in + 13);
            in[11] = (double)yaw_lo[i]; in[12] = (double)yaw_hi[i];
#pragma unroll
            for (int q = 0; q < kTailInRows; q++) pk[q * lp] = in[q];
          }
          pk += kTailInRows * lp;
          pk[0] = (double)i; pk[lp] = (double)T.t_slot; pk[2 * lp] = (double)T.t_batch;
          pk[3 * lp] = __longlong_as_double((long long)out); pk[4 * lp] = __longlong_as_double((long long)traj);
          pk[5 * lp] = __longlong_as_double((long long)status); pk[6 * lp] = __longlong_as_double((long long)iters);
          pk[7 * lp] = (double)ldo;
          ws.stage_drain();                          /* the trial sweep's stores of this wave have landed */
          /* (copied by the lane itself: the whole wave copying a deferring lane's column -- two round trips instead of twenty --
           * was built in round 4 and measured: no change in the launch's duration, 2.67 ms either way) */
          copy_iterate<R>(P.N - 1, column_load<R>(ws, S.cur ? FL::IT1 : FL::IT0), tile_store(tile_place<R>(T.tq.iter, pos, P.N - 1)));
          status[i] = MPC_STATUS_PENDING;
          if (iters) iters[i] = S.iters + it_total;
          have = false;                              /* the lane takes its next instance at the next hand-over */
        }
      } else if (T.pass_cut > 0 && passes >= T.pass_cut && S.phase == SV::PH_DIR) {
        /* still running: park it for the next phase */
        (void)park_for_next_phase(T, S, i, attempt, it_total, false);
        have = false; more = false; col_busy = true;   /* the column keeps the parked iterate: this lane takes nothing else */
      }
    }
  }
}

/* Deferred tails: a TAIL SLICE works on everything the launches have handed over (MpcPhase.tail_cut) for a bounded number of
 * passes.  Same solver, same arithmetic -- the results are bitwise those of an undisturbed launch -- on the handle's tail
 * stream, a few dense waves beside the launches of later batches.  Its sources are the survivors of the slice before it and
 * the fresh queues of the batches whose launches have ended since; a lane takes entries in turn, carries each one on, and
 * when the slice's budget of passes is spent, whatever is still running is parked again (at a pass boundary) in the
 * survivors' list for the next slice -- so a slice lasts a couple of milliseconds however long the longest chain is, its
 * waves are dense again at every slice, and a batch is final a slice after its own last straggler is.  Entries nobody
 * has taken by then are moved over as they are.  An entry for which the survivors' list has no room left stays with its
 * lane until it is solved (the slice lasts longer; nothing is lost).
 * Finality: remaining[slot] counts a batch's live stragglers -- the slice that absorbs its fresh queue adds their number,
 * every finished one subtracts one -- and whoever brings it to zero writes the batch id into final[slot] (the counter cannot
 * be zero before both have happened: partial sums without the addition are negative, with it positive). */
struct MpcSliceArgs {
  int32_t n_src, budget;           /* sources in use; wave passes after which the slice parks what is still running */
  int32_t ring, pad_;              /* slots of the handle's ring */
  MpcTailQ src[kSliceMaxSrc];      /* [0]: survivors of the previous slice; [1..]: fresh queues absorbed by this slice */
  int32_t fresh_slot[kSliceMaxSrc];
  int64_t fresh_batch[kSliceMaxSrc];
  MpcTailQ dst;                    /* survivors of this slice */
  int32_t *take;                   /* work counter over the concatenated sources */
  int32_t *done;                   /* waves of this slice that have left */
  int32_t *remaining;              /* [ring] */
  long long *final_id;             /* [ring], pinned host memory: the id of the batch that has become final in the slot */
  int32_t *res;                    /* pinned host memory: what the pump reads when the slice has completed -- [0] survivors left,
                                    * [j] entries of source j; [25..27]: entries finished / moved on untouched / parked again */
  int32_t *tally;                  /* [4]: those three, and the most passes a wave of the slice made */
  void *soc_ws;                    /* SOC builds: the SOC records of the slice's waves (see MpcPhase.soc_ws) */
};

template <bool STAGING, class R, class RIO = R, bool SOC = false>
__global__ __launch_bounds__(kBlock, 1) void mpc_tail_slice_kernel(const MpcParams P, const MpcSliceArgs A, R *__restrict__ wsbase,
                                                                     const int64_t tile_reals) {
  extern __shared__ double smem[];
  using WS = std::conditional_t<SOC, mpc::TiledSocWorkspace<STAGING, R>, mpc::TiledWorkspace<STAGING, R>>;
  using SV = mpc::Solver<WS, R, 0, SOC>;
  using FL = mpc::Fields<R>;
  WS ws;
  ws.tile = (typename WS::greal *)(wsbase + (int64_t)blockIdx.x * tile_reals);
  if constexpr (SOC) ws.soc_tile = (typename WS::greal *)((R *)A.soc_ws + (int64_t)blockIdx.x * (P.N - 1) * FL::SOC_SZ * 64);
  ws.lane = threadIdx.x;
  ws.lbuf = (typename WS::lreal *)smem;
  SV S(P, ws);
  const int M = P.N - 1;
  int64_t total = 0;
  for (int j = 0; j < A.n_src; j++) { const int c = *A.src[j].count; total += c < A.src[j].cap ? c : A.src[j].cap; }
  if (blockIdx.x == 0 && threadIdx.x >= 1 && (int)threadIdx.x < A.n_src) {
    /* absorb a fresh queue: its stragglers now count as live instances of their batch (a batch that deferred nothing is final here) */
    const int j = threadIdx.x;
    const int c0 = *A.src[j].count, c = c0 < A.src[j].cap ? c0 : A.src[j].cap;
    const int old = atomicAdd(A.remaining + A.fresh_slot[j], c);
    if (old + c == 0) __hip_atomic_store(A.final_id + A.fresh_slot[j], (long long)A.fresh_batch[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  const double *pk = nullptr;                      /* the entry this lane holds: its column in the source's rows, the rows' stride */
  int64_t lp = 0;
  R ylo_user = 0, yhi_user = 0;
  bool have = false, more = true, fin = false;
  bool keep = false;                               /* no room in the survivors' list: this lane's instance is solved here */
  int attempt = 0, it_total = 0, fin_status = 0, wp = 0;
  for (;;) {
    const bool spent = wp >= A.budget;
    if (fin) {
      const double *pm = pk + (int64_t)(kParkRows + kTailInRows) * lp;
      const int64_t i = (int64_t)pm[0];
      const int slot = (int)pm[lp];
      RIO *ob = (RIO *)__double_as_longlong(pm[3 * lp]);
      RIO *tb = (RIO *)__double_as_longlong(pm[4 * lp]);
      int32_t *st_arr = (int32_t *)__double_as_longlong(pm[5 * lp]), *it_arr = (int32_t *)__double_as_longlong(pm[6 * lp]);
      const int64_t l = (int64_t)pm[7 * lp];
      /* an entry is 80 numbers that have travelled through one or more queues: what it says about where its results go is checked
       * before it is believed (a damaged one is reported to the host -- mpc_last_error -- instead of being written through) */
      if (!(slot >= 0 && slot < A.ring && i >= 0 && i < l && ob && st_arr && l > 0)) {
        __hip_atomic_store(A.res + 28, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(A.res + 29, slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(A.res + 30, (int)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      } else {
        RIO *o = ob + i;
        RIO *t = tb ? tb + i : nullptr;
        S.unpack(mpc::NoColumn{}, [o, l](int q) { return OutRef<RIO, R>{o + q * l}; }, [t, l](int q) { return OutRef<RIO, R>{t + q * l}; }, t != nullptr, ylo_user, yhi_user);
        st_arr[i] = fin_status;
        if (it_arr) it_arr[i] = S.iters + it_total;
        const int old = atomicSub(A.remaining + slot, 1);
        if (old == 1) __hip_atomic_store(A.final_id + slot, (long long)pm[2 * lp], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        atomicAdd(A.tally, 1);
      }
      fin = false;
    }
    if (!have && more) {
      int64_t g = (int64_t)atomicAdd(A.take, 1);
      more = g < total;
      if (more) {
        int sj = 0;
        for (int j = 0; j < A.n_src; j++) {
          const int c0 = *A.src[j].count, c = c0 < A.src[j].cap ? c0 : A.src[j].cap;
          if (g >= c && j == sj) { g -= c; sj = j + 1; }
        }
        const R *it_src = nullptr;
        for (int j = 0; j < A.n_src; j++)
          if (j == sj) { pk = A.src[j].park + g; lp = A.src[j].cap; it_src = tile_place<R>(A.src[j].iter, g, M); }
        int dpos = -1;
        if (spent) {                               /* the budget is spent: the entry moves to the next slice as it is, if there is room */
          dpos = atomicAdd(A.dst.count, 1);
          if (dpos >= A.dst.cap) { dpos = -1; keep = true; }
        }
        if (dpos >= 0) {
          atomicAdd(A.tally + 1, 1);
          double *dk = A.dst.park + dpos;
          const int64_t dl = A.dst.cap;
          rows_copy(dk, dl, pk, lp, 0, kTailRows);
          copy_iterate<R>(M, tile_load(it_src), tile_store(tile_place<R>(A.dst.iter, dpos, M)));
        } else {
          /* the rows the tail cut wrote behind the solver's scalars: the same arrays at stride lp, the psi box between them */
          const double *pin = pk + (int64_t)kParkRows * lp;
          R st[6], cf[MPC_NCOEF], w[MPC_NW];
          mpc::gather_instance(P, 0, lp, pin, pin + 6 * lp, pin + 13 * lp, st, cf, w);
          ylo_user = (R)pin[11 * lp]; yhi_user = (R)pin[12 * lp];
          (void)S.setup(mpc::NoColumn{}, st, cf, ylo_user, yhi_user, w, false);
          const double *pq = pk;
          const int64_t lq = lp;
          S.unpark([pq, lq](int q) -> double { return pq[q * lq]; }, attempt, it_total);
          copy_iterate<R>(M, tile_load(it_src), column_store<R>(ws, S.cur ? FL::IT1 : FL::IT0));
          have = true;
        }
      }
    }
    if (!MPC_WAVE_ANY(have || more || fin)) break;
    if (have) {
      const int r = S.step();
      if (r != SV::MPC_RUNNING) {
        if (!S.next_attempt(r, attempt, it_total)) { fin = true; fin_status = r; have = false; keep = false; }
      } else if (spent && !keep && S.phase == SV::PH_DIR) {
        /* still running when the slice's budget is spent: parked for the next slice (its inputs and destination come along) */
        const int dpos = atomicAdd(A.dst.count, 1);
        if (dpos >= A.dst.cap) keep = true;
        else {
          atomicAdd(A.tally + 2, 1);
          double *dk = A.dst.park + dpos;
          const int64_t dl = A.dst.cap;
          S.park([dk, dl](int q) -> double & { return dk[q * dl]; }, attempt, it_total);
          rows_copy(dk, dl, pk, lp, kParkRows, kTailRows);
          ws.stage_drain();
          copy_iterate<R>(M, column_load<R>(ws, S.cur ? FL::IT1 : FL::IT0), tile_store(tile_place<R>(A.dst.iter, dpos, M)));
          have = false;
        }
      }
    }
    ++wp;
  }
  /* The wave that leaves last closes the slice (no copies or memsets behind it on the stream: on a full device every one of those
   * little launches waits for a free SIMD): it reports the counts to the host, and resets every counter for its next user --
   * the list this slice has read is the next slice's destination, a fresh queue it has absorbed is free for its next batch,
   * its own work counters serve the slice that takes this ring position again.  (Every wave's additions to the counters have
   * returned before it arrives here: their results decided what it did.) */
  if (threadIdx.x == 0) {
    atomicMax(A.tally + 3, wp);
    const int arrived = atomicAdd(A.done, 1);
    if (arrived == (int)gridDim.x - 1) {
      for (int q = 0; q < 4; q++) {
        const int v = __hip_atomic_load(A.tally + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(A.res + (q < 3 ? 25 + q : 31), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(A.tally + q, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      const int dc = __hip_atomic_load(A.dst.count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(A.res, dc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      for (int j = 1; j < A.n_src; j++) {
        const int c = __hip_atomic_load(A.src[j].count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(A.res + j, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      for (int j = 0; j < A.n_src; j++) __hip_atomic_store(A.src[j].count, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(A.take, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(A.done, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

/* ONE INSTANCE PER WAVEFRONT, or per LPI = 16 / 32 neighbouring lanes of one (small launches: one MPC::solve() per telemetry
 * message is the reference's own use).  The instance's N-step variables live in the workgroup's LDS ([stage][field][instance],
 * 3.7 KB per instance at N = 10 in fp64); every lane of the group
 * runs the solver's state machine on them -- the decisions are wave-uniform -- and the sweeps share their work between the
 * lanes (mpc::Solver<WS, R, true>: backward_wave, forward_wave and the wave form of costate_trial in mpc_core.h). */
/* The body is the per-instance driver of mpc_core.h: gather_instance, instance_solve by every lane of the group, instance_store by
 * the group's first lane.
 * WARM (the mpc_*_warm entry points): every lane of the group reads the instance's column of warm_in (Solver::solve_warm: the warm
 * attempt, then the complete cold solve if that does not end in SUCCESS); the first lane writes warm_out.
 * MODEL (the mpc_run_*_model / mpc_telemetry_*_model entry points): every lane of the group reads the group's column once, and
 * Solver::setup / unpack get it as an mpc::ModelColumn; warm_point judges a record against the relaxed box that set-up has just
 * set from the column.
 * `Extra`: what the WARM and MODEL builds take behind the solve arguments, one struct each in this order (mpc::WarmCall,
 * MpcModelPart); a build that is neither has the arguments it had. */
template <bool WARM> struct WaveStatusPtr { typedef int32_t *__restrict__ type; };
template <> struct WaveStatusPtr<true> { typedef int32_t *type; };      /* (warm_status may be the call's own status array) */
template <class R, int LPI, bool SOC = false, bool WARM = false, bool MODEL = false, class... Extra>
__global__ __launch_bounds__(kBlock, 1) void mpc_solve_wave_kernel(
    const MpcParams P, const int64_t B, const int64_t ld, const int64_t ldo, const R *__restrict__ state,
    const R *__restrict__ coeffs, const R *__restrict__ yaw_lo, const R *__restrict__ yaw_hi,
    const R *__restrict__ weights, R *__restrict__ out, R *__restrict__ traj,
    typename WaveStatusPtr<WARM>::type status, int32_t *__restrict__ iters, const Extra... extra) {
  extern __shared__ double smem[];
  static_assert(sizeof...(Extra) == (WARM ? 1 : 0) + (MODEL ? 1 : 0), "the WARM builds take a WarmCall, the MODEL builds an MpcModelPart");
  static_assert(!WARM || (sizeof(R) == 8 && !SOC), "warm start: the plain fp64 solve only");
  static_assert(!MODEL || sizeof(R) == 8, "per-instance model values: the fp64 solve only");
  constexpr int G = 64 / LPI;                       /* instances per wavefront: each on LPI neighbouring lanes */
  using WS = std::conditional_t<SOC, mpc::LdsSocWorkspace<R, G>, mpc::LdsWorkspace<R, G>>;
  using SV = mpc::Solver<WS, R, LPI, SOC>;
  const int group = threadIdx.x / LPI;
  const int64_t i = (int64_t)blockIdx.x * G + group;
  if (i >= B) return;                               /* (whole groups: nobody reads their lanes) */
  WS ws;
  ws.base = (typename WS::lreal *)smem;
  /* SOC builds: the SOC records behind the stage records (the launch asks for that much more dynamic LDS) */
  if constexpr (SOC) ws.soc_base = ws.base + mpc::workspace_fields_per_instance(P.N, sizeof(R) == 4, P.initial_state_rows != 0) * G;
  ws.lane = group;                                  /* every lane of the group addresses the group's instance */
  SV S(P, ws);
  S.wlane = threadIdx.x % LPI; S.wbase = group * LPI;
  R st[6], cf[MPC_NCOEF], w[MPC_NW];
  mpc::gather_instance(P, i, ld, state, coeffs, weights, st, cf, w);
  const R ylo = yaw_lo[i], yhi = yaw_hi[i];
  const auto warm = [&] {
    if constexpr (WARM) return std::get<0>(std::tie(extra...)).instance(i, (double)ylo, (double)yhi);
    else return mpc::NoWarm{};
  }();
  /* (MODEL: the group's column, read once; a column that cannot be used ends INFEASIBLE, mpc::ModelVals::column) */
  [[maybe_unused]] double mv[MPC_NMODEL];
  const auto col = [&] {
    if constexpr (MODEL) {
      const MpcModelPart &W = std::get<sizeof...(Extra) - 1>(std::tie(extra...));
#pragma unroll
      for (int q = 0; q < MPC_NMODEL; q++) mv[q] = W.model[q * W.ld_model + i];
      return mpc::ModelColumn{mv, 1};
    } else return mpc::NoColumn{};
  }();
  const int r = mpc::instance_solve(S, col, warm, st, cf, ylo, yhi, w);
  if (S.wlane == 0) {
    R *o = out + i;
    R *t = traj ? traj + i : nullptr;
    const int64_t l = ldo;
    const int it = mpc::instance_store(S, col, warm, [o, l](int q) -> R & { return o[q * l]; }, [t, l](int q) -> R & { return t[q * l]; },
                                       traj != nullptr, ylo, yhi);
    status[i] = r;
    if (iters) iters[i] = it;
  }
}

/* MPC::run pre- and post-processing, one instance per lane: mpc::run_pre_instance / run_post_instance of mpc_run_core.h (the rows of
 * `pre`: mpc::RUN_PRE_*).  MODEL (the mpc_run_*_model / mpc_telemetry_*_model entry points): one more kernel argument, and a lane
 * reads its instance's column of it once and hands it to mpc_run_core.h as mpc::ModelVals -- Lf in the latency compensation,
 * max_speed as the cap of the speed tables, max_steering in the normalisation, max_speed and the two acceleration limits in the
 * throttle.  A column that cannot be used: the handle's values (mpc::ModelVals::column); the solve in between reports the instance
 * INFEASIBLE.  The builds without it have the arguments they had (`Model` is empty) and read every value from P. */
template <bool TELEMETRY, bool MODEL, class... Model>
__global__ __launch_bounds__(256) void mpc_run_pre_kernel(const MpcParams P, int64_t B, int64_t ld, int npts,
                                                          const double *__restrict__ pose, double extra, double *__restrict__ ptsx,
                                                          double *__restrict__ ptsy, double *__restrict__ pre, int64_t ldp,
                                                          const Model... model) {
  static_assert(sizeof...(Model) == (MODEL ? 1 : 0), "the MODEL builds take one MpcModelPart");
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  if constexpr (MODEL) {
    const MpcModelPart &W = (model, ...);
    mpc::run_pre_instance<TELEMETRY>(P, mpc::model_vals_of(P, W.model, W.ld_model, i), i, ld, npts, pose, extra, ptsx, ptsy, pre, ldp);
  } else mpc::run_pre_instance<TELEMETRY>(P, P, i, ld, npts, pose, extra, ptsx, ptsy, pre, ldp);
}

/* ... the build of the telemetry handler with per-instance latency (mpc_telemetry_batch_*_latency): comp [ld], the seconds instance i
 * compensates for (mpc::RunComp), read once per lane, coalesced like the rows of `pose` and under no condition. */
template <bool MODEL, class... Model>
__global__ __launch_bounds__(256) void mpc_run_pre_comp_kernel(const MpcParams P, int64_t B, int64_t ld, int npts,
                                                               const double *__restrict__ pose, const double *__restrict__ comp,
                                                               double *__restrict__ ptsx, double *__restrict__ ptsy, double *__restrict__ pre,
                                                               int64_t ldp, const Model... model) {
  static_assert(sizeof...(Model) == (MODEL ? 1 : 0), "the MODEL builds take one MpcModelPart");
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const mpc::RunComp lc{true, comp[i]};
  if constexpr (MODEL) {
    const MpcModelPart &W = (model, ...);
    mpc::run_pre_instance<true>(P, mpc::model_vals_of(P, W.model, W.ld_model, i), i, ld, npts, pose, lc, ptsx, ptsy, pre, ldp);
  } else mpc::run_pre_instance<true>(P, P, i, ld, npts, pose, lc, ptsx, ptsy, pre, ldp);
}

template <bool MODEL, class... Model>
__global__ __launch_bounds__(256) void mpc_run_post_kernel(const MpcParams P, int64_t B, const double *__restrict__ pre, int64_t ldp,
                                                           const double *__restrict__ out9, int64_t ld9, double *__restrict__ out8,
                                                           double *__restrict__ cmd, int64_t ld, const Model... model) {
  static_assert(sizeof...(Model) == (MODEL ? 1 : 0), "the MODEL builds take one MpcModelPart");
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  if constexpr (MODEL) {
    const MpcModelPart &W = (model, ...);
    mpc::run_post_instance(P, mpc::model_vals_of(P, W.model, W.ld_model, i), i, pre, ldp, out9, ld9, out8, cmd, ld);
  } else mpc::run_post_instance(P, P, i, pre, ldp, out9, ld9, out8, cmd, ld);
}

/* rollout bookkeeping: next state <- solve()'s step-1 rows; worst status and summed iterations per instance */
__global__ __launch_bounds__(256) void mpc_rollout_step_kernel(int64_t B, int64_t ld, int first, const double *__restrict__ out9,
                                                               double *__restrict__ state, const int32_t *__restrict__ st_step,
                                                               const int32_t *__restrict__ it_step, int32_t *__restrict__ status,
                                                               int32_t *__restrict__ iters) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
#pragma unroll
  for (int q = 0; q < 6; q++) state[q * ld + i] = out9[q * ld + i];
  const int32_t s = st_step[i];
  status[i] = first ? s : (s > status[i] ? s : status[i]);
  if (iters) iters[i] = (first ? 0 : iters[i]) + it_step[i];
}

/* Track driving (mpc_drive_batch_*, include/mpc_amd_drive.h), the two kernels around the handler's three (and, with per-car latency,
 * one before the loop): one car per lane, 256 per block, no LDS, mpc::drive_* of mpc_drive_core.h.  The track is read at the loop index -- the same address in every lane of a wave,
 * scalar loads -- and once per lane at the car's own nearest waypoint and window.
 * Sense: the window index of every car at its position and the window's waypoints, laid out as the handler takes them. */
__global__ __launch_bounds__(256) void mpc_drive_sense_kernel(int64_t B, int64_t ld, int npts, const double *__restrict__ car,
                                                              const double *__restrict__ track_x, const double *__restrict__ track_y,
                                                              int n_track, double *__restrict__ ptsx, double *__restrict__ ptsy,
                                                              int32_t *__restrict__ k_now, const double *__restrict__ noise, int step,
                                                              double *__restrict__ seen6, double *__restrict__ seen) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const int k = mpc::drive_window(track_x, track_y, n_track, car[i], car[ld + i]);
  mpc::drive_window_points(track_x, track_y, n_track, k, npts, ptsx, ptsy, ld, i);
  k_now[i] = k;
  /* a noise call: what the handler is told about the car at this message (mpc::drive_seen), into the handle's rows seen6 [6][ld] and
   * this step's block of the caller's seen [4][ld] (or nullptr).  The window above is the TRUE car's. */
  if (seen6) mpc::drive_seen(mpc::drive_noise_of(noise, ld, i), step, car, ld, i, seen6, ld, seen);
}

/* Plant and summary, the one kernel of every drive entry point: the step's record and summary rows, the car's worst status and summed
 * iterations, then the car moved under the command it was sent (mpc::drive_step_instance).  pre: the handler's own rows of this step
 * (cte0, epsi0).  The three per-car arrays are the caller's or nullptr, and a lane reads its car's column of each once:
 *   latency [MPC_NLATENCY][ld]: the car's own substep counts (mpc::drive_latency_of: checked, 0 .. 1000); nullptr: the call's.
 *   W.model [MPC_NMODEL][W.ld_model]: Lf in the heading update, max_steering in turning the reply into the steering angle in force; a
 *     column that cannot be used: the handle's values (mpc::model_vals_of; the handler has reported the car INFEASIBLE); nullptr: the
 *     handle's values.
 *   plant [MPC_NPLANT][ld]: what the car is moved with (mpc::drive_plant_vals_of: checked; a column that cannot be used becomes a
 *     status); nullptr: the default column, the plant of the entry points without `plant` bit for bit.
 *   noise [MPC_NNOISE][ld]: what message `step` adds to the plant column in force and whether its reply arrives (mpc::drive_noise_of:
 *     checked; a column that cannot be used becomes a status); nullptr: the zero column, which draws nothing. */
__global__ __launch_bounds__(256) void mpc_drive_plant_kernel(const MpcParams P, const MpcDriveOpts O, int64_t B, int64_t ld, int step, int n_track,
                                                              double *__restrict__ car, const double *__restrict__ cmd,
                                                              const double *__restrict__ pre, int64_t ldp, const int32_t *__restrict__ st_step,
                                                              const int32_t *__restrict__ it_step, const int32_t *k_now,
                                                              const int32_t *k_prev, double *__restrict__ summary,
                                                              double *__restrict__ rec, int32_t *__restrict__ status, int32_t *__restrict__ iters,
                                                              const double *__restrict__ latency, const MpcModelPart W,
                                                              const double *__restrict__ plant, const double *__restrict__ noise) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  int sub_old = O.sub_old, sub_new = O.sub_new;
  if (latency) {
    const mpc::DriveLatency dl = mpc::drive_latency_of(O, latency, ld, i);
    sub_old = dl.sub_old; sub_new = dl.sub_new;
  }
  const mpc::ModelVals mv = W.model ? mpc::model_vals_of(P, W.model, W.ld_model, i) : mpc::ModelVals::of(P);
  mpc::drive_step_instance(P, mv, mpc::drive_plant_vals_of(P, mv, plant, ld, i), mpc::drive_noise_of(noise, ld, i), O, sub_old, sub_new, i, ld, step, n_track, car, cmd, pre, ldp, st_step[i],
                           it_step[i], k_now[i], k_prev[i], summary, rec, status, iters);
}
/* What the stepwise loop's handler compensates for, per car: comp [ld] <- row MPC_LATENCY_COMP of the car's column, not-a-number for
 * a column that cannot be used (the handler turns that into a status).  Once per call. */
__global__ __launch_bounds__(256) void mpc_drive_comp_kernel(const MpcDriveOpts O, int64_t B, int64_t ld, const double *__restrict__ latency,
                                                             double *__restrict__ comp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  comp[i] = mpc::drive_latency_of(O, latency, ld, i).comp;
}
/* mpc_debug_drive_noise_device: mpc::drive_noise_draw for n (seed, step) pairs, a pair per lane; out [7][n].  A pair the host
 * evaluation refuses gives not-a-number. */
__global__ __launch_bounds__(256) void mpc_debug_drive_noise_kernel(int64_t n, const double *__restrict__ seed, const int32_t *__restrict__ step,
                                                                    double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double z[mpc::DRIVE_NDRAW];
  const double sd = seed[i];
  const int32_t t = step[i];
  if (mpc::drive_finite(sd) && mpc::drive_seed_ok(sd) && t >= 0) {
    mpc::drive_noise_draw(sd, t, z);
  } else {
    MPC_UNROLL
    for (int q = 0; q < mpc::DRIVE_NDRAW; q++) z[q] = NAN;
  }
  MPC_UNROLL
  for (int q = 0; q < mpc::DRIVE_NDRAW; q++) out[q * n + i] = z[q];
}

/* The certificate of a stored point (mpc_certify_batch_*), one instance per lane: mpc::certify_batch_instance of mpc_core.h.  A lane
 * walks the stage records of its column of `sol` once -- consecutive lanes read consecutive addresses of every row, like `state` --
 * and keeps the neighbouring state, multipliers and steering values in registers: no workspace, no LDS, no loop whose trip count the
 * data decide.  KIND: what the call brought (0 nothing, 1 `model`, 2 `horizon`).  256 lanes per block: the body holds about 60 live
 * doubles (one record, the carried stage, the stage model, the sums) and compiles to about 210 vector registers, no scratch. */
constexpr int kCertBlock = 256;
template <int KIND>
__global__ __launch_bounds__(kCertBlock) void mpc_certify_kernel(const MpcParams P, int64_t B, int64_t ld, const double *__restrict__ state,
                                                                 const double *__restrict__ coeffs, const double *__restrict__ yaw_lo,
                                                                 const double *__restrict__ yaw_hi, const double *__restrict__ weights,
                                                                 const double *__restrict__ model, const int32_t *__restrict__ horizon,
                                                                 const double *__restrict__ sol, int64_t ld_sol, double *__restrict__ cert,
                                                                 int32_t *__restrict__ verdict) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  mpc::certify_batch_instance<KIND>(P, i, ld, state, coeffs, yaw_lo, yaw_hi, weights, model, horizon, sol, ld_sol, cert, verdict);
}

/* Statistics of a batch, accumulated into handle-owned memory right behind the solve (mpc_get_stats never touches
 * the caller's arrays again): acc[0..4] = instances per status code 0..3 and "any other", acc[5] = sum of iterations,
 * acc[6] = max, acc[7] = pending, acc[8] = MPC_STATUS_ACCEPTABLE. */
constexpr int kStatWords = 10;
__global__ __launch_bounds__(256) void mpc_stats_kernel(int64_t B, const int32_t *__restrict__ status, const int32_t *__restrict__ iters,
                                                        unsigned long long *__restrict__ acc) {
  __shared__ unsigned int cnt[6];
  __shared__ unsigned long long isum;
  __shared__ int imax;
  if (threadIdx.x < 6) cnt[threadIdx.x] = 0;
  if (threadIdx.x == 0) { isum = 0; imax = 0; }
  __syncthreads();
  unsigned int my[6] = {0, 0, 0, 0, 0, 0}, pend = 0;
  unsigned long long ms = 0;
  int mm = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t st = status[i];
    if (st == MPC_STATUS_PENDING) { ++pend; continue; }   /* deferred: counted, its iterations are not final */
    const int c = st == MPC_STATUS_ACCEPTABLE ? 5 : ((st >= 0 && st < 4) ? st : 4);
#pragma unroll
    for (int q = 0; q < 6; q++) my[q] += (c == q);
    const int it = iters ? iters[i] : 0;
    ms += (unsigned long long)it;
    mm = it > mm ? it : mm;
  }
#pragma unroll
  for (int q = 0; q < 6; q++) if (my[q]) atomicAdd(&cnt[q], my[q]);
  if (ms) atomicAdd(&isum, ms);
  if (mm) atomicMax(&imax, mm);
  if (pend) atomicAdd(&acc[7], (unsigned long long)pend);
  __syncthreads();
  if (threadIdx.x < 5 && cnt[threadIdx.x]) atomicAdd(&acc[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
  if (threadIdx.x == 5 && isum) atomicAdd(&acc[5], isum);
  if (threadIdx.x == 6 && imax) atomicMax(&acc[6], (unsigned long long)imax);
  if (threadIdx.x == 7 && cnt[5]) atomicAdd(&acc[8], (unsigned long long)cnt[5]);
}

__global__ void mpc_debug_math_kernel(int64_t n, const double *x, double *sn, double *cs, double *rc, double *at, double *lg) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s, c;
  mpc::fsincos(x[i], &s, &c);
  sn[i] = s; cs[i] = c; rc[i] = mpc::frcp(x[i]);
  at[i] = mpc::fatan(x[i]); lg[i] = mpc::flog(fabs(x[i]));
}

/* ten rows of mpc_debug_math_all for one real type: fsincos2 with an argument of its own in each slot, the two reciprocals, atan,
 * log and hpow at the solver's two exponents; out points at this lane's column, rows are n apart */
template <class R>
__device__ __forceinline__ void debug_math_rows(R x, R y, double *out, int64_t n) {
  R sa, ca, sb, cb;
  mpc::fsincos2(x, y, &sa, &ca, &sb, &cb);
  out[0] = (double)sa; out[n] = (double)ca; out[2 * n] = (double)sb; out[3 * n] = (double)cb;
  out[4 * n] = (double)mpc::frcp(x); out[5 * n] = (double)mpc::frcp1(x);
  out[6 * n] = (double)mpc::fatan(x); out[7 * n] = (double)mpc::flog(x);
  out[8 * n] = (double)mpc::hpow(x, mpc::IpmConst<R>::s_theta); out[9 * n] = (double)mpc::hpow(x, mpc::IpmConst<R>::s_phi);
}
__global__ __launch_bounds__(256) void mpc_debug_math_all_kernel(int64_t n, const double *x, const double *y, double *out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double xi = x[i], yi = y[i];
  debug_math_rows<double>(xi, yi, out + i, n);
  debug_math_rows<float>((float)xi, (float)yi, out + 10 * n + i, n);
}

}  // namespace

/* ---- host side from here on ---------------------------------------------------------------------------------------------------- */
#include <optional>
#include <type_traits>

struct MpcHandle {
  MpcParams params;
  int device = 0;
  int64_t max_batch = 0;
  int64_t ws_stride = 0;   /* reals (double, or float for MPC_PRECISION_F32) per wavefront tile of the workspace */
  bool staging = true;
  int64_t wave_max_batch = 0;   /* launches up to this size run one instance per wavefront (mpc_solve_wave_kernel); 0: never */
  bool mixed = false;      /* two phases per solve: fp32 up to MpcParams.mixed_switch_mu, then fp64 to tol (f32_finish on an F32 handle,
                            * f64_f32_start on an F64 handle) */
  int64_t ws_stride_f32 = 0, ws_stride_f64 = 0;   /* reals per wavefront tile of either record layout */
  int64_t io_stride = 0;   /* leading dimension of the handle's own staging arrays */
  void *ws = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  /* staging of the host-pointer entry point: ONE device block and its pinned host mirror, rows with a per-call
   * leading dimension: in = state[6] coeffs[5] ylo yhi weights[12] (25 rows) | out = out[9] traj[2N] | one row holding
   * status and iters (int32 each) -- so a call is one copy in, the launch, one copy out */
  void *d_io = nullptr, *h_io = nullptr;
  unsigned long long *d_stats = nullptr;   /* [kStatWords] statistics of the last batch (mpc_stats_kernel) */
  hipEvent_t ev_stats = nullptr;
  bool have_stats = false;
  double *d_run = nullptr;    /* run(): pre[15] rows */
  double *d_run9 = nullptr;   /* run(), rollout: solve()'s 9 rows, caller's leading dimension (grown on demand) */
  size_t run9_bytes = 0;
  int32_t *d_status = nullptr, *d_iters = nullptr, *d_rstat = nullptr, *d_counter = nullptr;
  int64_t counter_seq = 0;    /* solve calls that used a counter block so far */
  /* statistics are gathered when mpc_get_stats asks for them (a kernel per batch on the launch stream costs the serving loop a
   * few per cent): what the most recent call wrote, and the event behind it */
  const int32_t *st_status = nullptr, *st_iters = nullptr;
  int64_t st_B = 0;
  hipEvent_t st_ev = nullptr;
  bool stats_pending = false;
  int compact_gap = 0;        /* MpcParams.lane_compact, or MPC_LANE_COMPACT in the environment (measurement aid): see MpcPhase.compact_gap */
  bool compact_env = false;
  int64_t compact_min_batch = 8192;   /* smaller launches are latency-bound: the moves cost more than the lines they save */
  /* take order (see MpcPhase.ord_list): 1 = hardest bin first, 2 = easiest bin first, 0 = off; MPC_TAKE_ORDER in the environment
   * (measurement aid).  Applied to single-phase fp64 launches of the solve entry points from take_order_min_batch instances,
   * N < 15, no per-instance weights, no SOC: the cases tools/take_order_model.py and the benchmark have measured. */
  int take_order = 1;
  int64_t take_order_min_batch = 8192;
  int32_t *d_take_list = nullptr;     /* [mpc::kTakeBins][io_stride] (allocated on first use) */
  int64_t n_take_ordered = 0;         /* launches taken in key order so far (mpc_take_order_info) */
  /* multi-phase solve: second workspace, two parked-instance lists and two sets of scalars (allocated on first use) */
  int n_cuts = 0;             /* MpcParams.pass_cut + pass_cut_next[] (none = single launch) */
  int cuts[kMaxCuts] = {0, 0, 0, 0};
  void *ws2 = nullptr;
  double *d_park = nullptr;   /* [2][PARK_ROWS][io_stride] */
  void *d_piter = nullptr;    /* mixed precision: the promoted iterates, [io_stride / 64][N-1][IT_SZ of the fp32 record][64] floats */
  bool promote_buffer = false;   /* MpcParams.f32_phase_refill */
  int32_t *d_list = nullptr;  /* [2][2][io_stride]: instance, source column */
  /* deferred tails (MpcParams.tail_cut > 0; allocated on first use): see "tail slices" below */
  struct TailSlot {                /* one per batch whose stragglers may be outstanding (ring of tail_ring) */
    int64_t batch_id = 0;          /* 0: never used */
    bool final_ = true;
    int64_t deferred = -1;         /* instances the batch handed over (known once the absorbing slice has completed) */
    int64_t B = 0;
  };
  struct FreshQ {                  /* the queue a launch hands its stragglers to, until a slice absorbs it (ring of kFreshRing) */
    int64_t batch_id = 0;
    int slot = 0;
    int state = 0;                 /* 0 free, 1 filled by a launch (bulk recorded), 2 absorbed by slice `slice` */
    int64_t slice = -1;
    hipEvent_t bulk = nullptr;
  };
  struct BatchRec {                /* the last kBatchRecs solve calls: how mpc_tail_wait resolves an id */
    int64_t id = 0;
    int kind = 0;                  /* 0 not deferring: final behind `ev`; 1 deferring: final per its slot */
    int slot = 0;
    hipEvent_t ev = nullptr;
  };
  static constexpr int kBatchRecs = 1024;
  struct SliceRes { int32_t count[32]; };     /* [0]: survivors the slice left; [j]: entries of its source j */
  static_assert(kSliceMaxSrc <= 25, "SliceRes: [25..31] carry the tallies and the damaged-entry report");
  bool tail_ready = false;
  bool tail_double = true;     /* the solver of the tail slices: fp64, or fp32 on a pure MPC_PRECISION_F32 handle */
  int tail_ring = 0, tail_waves = 256, tail_priority = 0, slice_passes = 16;
  /* (a slice's grid: a lane per survivor -- they are the long chains: most use the slice's whole budget -- and one per
   * kSliceFreshDiv fresh entries: an instance just over the cut needs a few more passes, so a lane works off several in turn) */
  int64_t tail_cap = 0, surv_cap = 0;
  hipStream_t tail_stream = nullptr;
  MpcTailQ fq_dev[kFreshRing] = {}, surv_dev[2] = {};   /* device storage of the fresh queues and the two survivor lists */
  int32_t *d_tcount = nullptr;   /* [kFreshRing + 2 + 6 kSliceRing]: counts of the fresh queues, of the survivor lists, slice work and exit counters, slice tallies */
  int32_t *d_remaining = nullptr;
  long long *h_final = nullptr;  /* pinned: [tail_ring] the id of the batch that has become final in each slot (written by the slices) */
  SliceRes *h_res = nullptr;     /* pinned: [kSliceRing], written by each slice's last wave */
  void *tail_ws = nullptr;
  /* SOC records (MpcParams.max_soc > 0, fp64 solver), allocated by the first solve that asks for them: one set for the launches on
   * the caller's stream (a tile per wave of the largest grid), one for the tail slices (they run beside those launches) */
  void *soc_ws = nullptr, *soc_tail = nullptr;
  TailSlot tslot[kTailMaxRing];
  FreshQ fq[kFreshRing];
  BatchRec *brec = nullptr;
  hipEvent_t slice_ev[kSliceRing] = {};
  struct Absorbed { int fq; int slot; int64_t batch; };
  /* measurement aid: MPC_TAIL_TRACE=<file> appends one line per retired slice (see tail_retire) */
  int64_t slice_t0[kSliceRing] = {}, slice_est[kSliceRing] = {}, slice_surv_in[kSliceRing] = {};
  int slice_waves[kSliceRing] = {};
  int slice_nabs[kSliceRing] = {};            /* fresh queues slice k % kSliceRing absorbed, and which (queue, its batch and slot) */
  Absorbed slice_abs[kSliceRing][kFreshRing] = {};
  int64_t n_slice = 0, n_slice_done = 0;      /* slices launched / retired */
  int64_t surv_last = 0;                      /* survivors the most recent retired slice left */
  int64_t fresh_avg = 64;                     /* running estimate of a batch's deferred instances (sizes a slice's grid) */
  int64_t n_not_final = 0;                    /* deferring batches not yet known to be final */
  int64_t n_throttled = 0;                    /* batches that ran without deferral because the survivors' list was filling up */
  int64_t n_overflow = 0;                     /* batches that handed over more than their fresh queue holds */
  /* MpcParams.tail_cut = MPC_TAIL_AUTO: the handle's own choice -- it starts from a cut at 20 passes for horizons up to N = 12, 24
   * beyond (the long horizons need more iterations), moves it out while more than 8 % of a batch are handed over (or a
   * fresh queue overflows) and back while less than 1.5 % is; and a wave does not wait for its last 4 lanes (measured on the survey population:
   * cuts of 16 ... 32 within 5 % of each other, 20 best; few 0 / 2 / 4 / 8: 43.4 / 43.8 / 44.7 / 44.8 M solves/s).  The arithmetic
   * of an instance does not depend on where it is carried on, so these change timing only.  auto_share: running mean of the
   * share of a batch that was handed over, in 1/65536 (mpc_tail_info). */
  int tail_few = 4;                           /* MPC_TAIL_FEW (see MpcPhase.tail_few) */
  int auto_cut = 20, auto_base = 20;
  int64_t auto_share = -1;
  int64_t batch_seq = 0;         /* id of the most recent batch (every solve call counts) */
  int64_t n_deferred = 0;        /* deferring batches so far: batch k of them uses slot k % tail_ring and fresh queue k % kFreshRing */
  /* warm start (allocated on first use): the rollout's warm buffer, [mpc_warm_rows(N)][io_stride] doubles, and the device side of the
   * host entry point's warm_in / warm_out (one block, read and written in place) with the status the warm data came with */
  double *d_warm = nullptr, *d_warm_io = nullptr;
  double *d_warm_o = nullptr;         /* host forms with a horizon: warm_out on its own (rows an instance does not write come back as the caller has them) */
  int32_t *d_horizon = nullptr;       /* ... and the horizons of a host-array call */
  int32_t *d_budget = nullptr;        /* ... and its iteration budgets */
  double *d_model = nullptr;      /* the device side of mpc_solve_batch_host_model's model array (allocated on first use) */
  int32_t *d_warm_st = nullptr;
  int64_t n_roll_fused = 0, n_roll_stepwise = 0;   /* mpc_rollout_batch_device_fused calls that ran the fused kernel / the stepwise loop (mpc_rollout_fused_info) */
  /* track driving (allocated on first use): the window rows, the reply and the window indices of two steps, with the caller's leading
   * dimension -- ptsx [8][ld], ptsy [8][ld], cmd [2][ld], k [2][ld] int32 --; the caller's weights at the handle's stride, as run()'s solve
   * reads its inputs; calls that ran the one launch / the stepwise loop (mpc_drive_info) */
  double *d_drive = nullptr, *d_drive_w = nullptr;
  size_t drive_bytes = 0;
  double *d_drive_host = nullptr;     /* mpc_drive_batch_host: device staging, grown on demand */
  size_t drive_host_bytes = 0;
  int64_t n_drive_fused = 0, n_drive_stepwise = 0;
  double *d_tel = nullptr;       /* mpc_telemetry_batch_host: device staging, grown on demand */
  size_t tel_bytes = 0;
  /* last call */
  int64_t last_B = 0;
  bool timed = false;
};

#define MPC_TRY(expr)                                                                    \
  do {                                                                                   \
    const int rc_ = (expr);                                                              \
    if (rc_ != MPC_OK) return rc_;                                                       \
  } while (0)

/* the handle's lazy device allocations: made by the first call that needs them, kept (mpc_destroy frees whatever exists) */
template <class T>
static int ensure_dev(T **p, size_t bytes) {
  if (!*p) MPC_HIP_CHECK(hipMalloc((void **)p, bytes));
  return MPC_OK;
}
/* ... and the ones that follow the caller's sizes: *have bytes now, at least `need` afterwards */
template <class T>
static int grow_dev(T **p, size_t *have, size_t need) {
  if (*p && *have >= need) return MPC_OK;
  if (*p) MPC_HIP_CHECK(hipFree(*p));
  *p = nullptr; *have = 0;
  MPC_HIP_CHECK(hipMalloc((void **)p, need));
  *have = need;
  return MPC_OK;
}

/* what the entry points with a batch of their own check first (the solve entry points: solve_begin) */
static int check_batch(const MpcHandle *h, int64_t B, int64_t ld) {
  if (!h) { g_last_error = "NULL handle"; return MPC_ERR_INVALID; }
  if (B < 0 || ld < B || B > h->max_batch) { g_last_error = "bad B/ld"; return MPC_ERR_INVALID; }
  return MPC_OK;
}

static void set_wave_limit(MpcHandle *h, const MpcParams *p) {
  h->wave_max_batch = p->wave_max_batch == 0 ? 1024 : (p->wave_max_batch < 0 ? 0 : p->wave_max_batch);
  if (const char *e = getenv("MPC_WAVE_MAX_BATCH")) h->wave_max_batch = atoll(e);      /* (A/B measurements) */
  if (p->f64_f32_start == MPC_F32_START_ON || (p->precision == MPC_PRECISION_F32 && p->f32_finish != 0)) h->wave_max_batch = 0;
}

/* the cut schedule of the multi-phase solve: MpcParams.pass_cut, pass_cut_next[0..2] (a zero ends the list) */
static void set_cuts(MpcHandle *h, const MpcParams *p) {
  h->n_cuts = 0;
  const int32_t given[kMaxCuts] = {p->pass_cut, p->pass_cut_next[0], p->pass_cut_next[1], p->pass_cut_next[2]};
  for (int q = 0; q < kMaxCuts && given[q] > 0; q++) h->cuts[h->n_cuts++] = given[q];
}

/* two phases per solve (fp32 iterations, fp64 finish)?  F32 handles: f32_finish; F64 handles: f64_f32_start = 1, or 2
 * (MPC_F32_START_AUTO; the default is 0 = off) from the horizon at which the workspace of a full device no longer lives in the
 * Infinity Cache */
static bool wants_mixed(const MpcParams *p, int64_t max_batch) {
  (void)max_batch;
  if (p->precision == MPC_PRECISION_F32) return p->f32_finish != 0;
  return p->f64_f32_start == 1 || (p->f64_f32_start == MPC_F32_START_AUTO && p->N >= MPC_F32_START_AUTO_N);
}

static int validate_params(const MpcParams *p) {
  if (!p) return MPC_ERR_INVALID;
  if (p->abi_version != MPC_ABI_VERSION) { g_last_error = "MpcParams.abi_version mismatch"; return MPC_ERR_INVALID; }
  if (p->N < 3 || p->N > MPC_MAX_N) { g_last_error = "N out of range"; return MPC_ERR_INVALID; }
  if (!(p->dt > 0) || !(p->Lf > 0) || !(p->max_speed > 0) || !(p->max_steering > 0)) { g_last_error = "bad dt/Lf/limits"; return MPC_ERR_INVALID; }
  if (p->n_steers < 0 || p->n_steers > MPC_MAX_TABLE || p->n_steer_speeds < 1 || p->n_steer_speeds > MPC_MAX_TABLE) { g_last_error = "bad steer tables"; return MPC_ERR_INVALID; }
  if (p->n_yaw_changes < 0 || p->n_yaw_changes > MPC_MAX_TABLE || p->n_yaw_change_speeds < 0 || p->n_yaw_change_speeds > MPC_MAX_TABLE) { g_last_error = "bad yaw-change tables"; return MPC_ERR_INVALID; }
  if (!(p->out_step_tol >= 0)) { g_last_error = "bad out_step_tol"; return MPC_ERR_INVALID; }
  if (!(p->bound_relax_factor >= 0 && p->bound_relax_factor <= 1e-3)) { g_last_error = "bad bound_relax_factor (IPOPT default 1e-8)"; return MPC_ERR_INVALID; }
  if (p->branch_mode != MPC_BRANCH_FROZEN) { g_last_error = "branch_mode LIVE is not implemented on the device path"; return MPC_ERR_UNSUPPORTED; }
  if (p->precision != MPC_PRECISION_F64 && p->precision != MPC_PRECISION_F32) { g_last_error = "unknown precision"; return MPC_ERR_INVALID; }
  if (p->precision == MPC_PRECISION_F32 && !(p->tol_f32 >= 1e-5)) { g_last_error = "tol_f32 below 1e-5 is beyond single precision"; return MPC_ERR_INVALID; }
  if (p->max_iter < 1 || !(p->tol > 0)) { g_last_error = "bad max_iter/tol"; return MPC_ERR_INVALID; }
  if (p->tail_cut < MPC_TAIL_AUTO || p->tail_ring < 0 || p->tail_capacity < 0) { g_last_error = "bad tail_cut/tail_ring/tail_capacity"; return MPC_ERR_INVALID; }
  if (p->f64_f32_start < 0 || p->f64_f32_start > MPC_F32_START_AUTO) { g_last_error = "f64_f32_start must be 0 (off), 1 (on) or 2 (auto)"; return MPC_ERR_INVALID; }
  if (p->lane_compact < MPC_LANE_COMPACT_AUTO || p->lane_compact > 7) { g_last_error = "lane_compact must be -1 (auto), 0 (off) .. 7"; return MPC_ERR_INVALID; }
  if (p->max_soc < 0 || p->max_soc > MPC_MAX_SOC) { g_last_error = "max_soc must be 0 (off) .. 16 (IPOPT's default is 4)"; return MPC_ERR_INVALID; }
  /* the termination fields (ABI 4): an MpcParams that was never filled by mpc_params_default holds zeros here, with which no iterate
   * passes the convergence check and every instance runs to MPC_STATUS_MAXITER */
  const struct { const char *name; double value; } positive[] = {
      {"dual_inf_tol", p->dual_inf_tol}, {"constr_viol_tol", p->constr_viol_tol}, {"compl_inf_tol", p->compl_inf_tol},
      {"acceptable_tol", p->acceptable_tol}, {"acceptable_dual_inf_tol", p->acceptable_dual_inf_tol},
      {"acceptable_constr_viol_tol", p->acceptable_constr_viol_tol}, {"acceptable_compl_inf_tol", p->acceptable_compl_inf_tol},
      {"mixed_switch_mu", p->mixed_switch_mu}};
  for (const auto &f : positive)
    if (!(f.value > 0)) { g_last_error = std::string(f.name) + " must be positive (mpc_params_default sets it)"; return MPC_ERR_INVALID; }
  if (p->acceptable_iter < 0) { g_last_error = "acceptable_iter must be 0 (off) or positive"; return MPC_ERR_INVALID; }
  return MPC_OK;
}

extern "C" int mpc_abi_version(void) { return MPC_ABI_VERSION; }

extern "C" const char *mpc_last_error(void) { return g_last_error.c_str(); }

extern "C" int mpc_create(const MpcParams *p, int device, int64_t max_batch, MpcHandle **out) {
  if (!out || max_batch < 1) return MPC_ERR_INVALID;
  int rc = validate_params(p);
  if (rc != MPC_OK) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { g_last_error = "no HIP device"; return MPC_ERR_NO_DEVICE; }
  if (device < 0) MPC_HIP_CHECK(hipGetDevice(&device));
  if (device >= ndev) { g_last_error = "device index out of range"; return MPC_ERR_NO_DEVICE; }
  DeviceGuard guard_(device);   /* the caller's current device is restored on return */
  MPC_HIP_CHECK(guard_.err);
  hipDeviceProp_t prop;
  MPC_HIP_CHECK(hipGetDeviceProperties(&prop, device));
  if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) {
    g_last_error = std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
    return MPC_ERR_NO_DEVICE;
  }
  MpcHandle *h = new MpcHandle();
  /* a failing HIP call from here on must not leak the handle */
#define MPC_CREATE_CHECK(expr)                                                          \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) {                                                             \
      g_last_error = std::string(#expr) + ": " + hipGetErrorString(e_);                 \
      mpc_destroy(h);                                                                   \
      return MPC_ERR_HIP;                                                               \
    }                                                                                   \
  } while (0)
  h->params = *p; h->device = device; h->max_batch = max_batch;
  /* Launch shape: each workgroup is one wave; the fp64 kernel needs ~390 registers, so at most one wave runs
   * per SIMD (4 per CU), and the 36 KB of staging LDS per wave fit four times into a CU's 160 KB (fp32: 256
   * registers, two waves per SIMD, 20 KB each).
   * MPC_STAGING=0 selects the variant with ordinary loads (for A/B measurements). */
  h->staging = true;
  if (const char *e = getenv("MPC_STAGING")) h->staging = atoi(e) != 0;
  const bool f32 = p->precision == MPC_PRECISION_F32;
  h->mixed = wants_mixed(p, max_batch);
  /* the staging builds this handle may launch: its own precision's, and the phases of a mixed-precision solve */
  const void *const staged[] = {f32 ? (const void *)mpc_solve_kernel<true, float> : (const void *)mpc_solve_kernel<true, double>,
                                (const void *)mpc_solve_kernel<true, double, float, float>, (const void *)mpc_solve_kernel<true, float, double, double>,
                                (const void *)mpc_solve_kernel<true, double, double, float>};
  for (int q = 0; q < (h->mixed ? 4 : 1); q++)
    MPC_CREATE_CHECK(hipFuncSetAttribute(staged[q], hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsPerCu));
  h->ws_stride = mpc::workspace_fields_per_instance(p->N, f32, p->initial_state_rows != 0) * 64;   /* reals per wavefront tile */
  h->ws_stride_f32 = mpc::workspace_fields_per_instance(p->N, true, p->initial_state_rows != 0) * 64;
  h->ws_stride_f64 = mpc::workspace_fields_per_instance(p->N, false, p->initial_state_rows != 0) * 64;
  /* Small launches run ONE INSTANCE PER WAVEFRONT, or per 16 / 32 of its lanes (mpc_solve_wave_kernel): the lane kernel puts 64
   * instances into a wave, which is bound by the instructions it issues -- one MPC::solve() 0.68 ms; with the sweeps shared
   * between the lanes 0.30 ms, bitwise the same results (MpcParams.wave_max_batch: default 1 024 instances). */
  set_wave_limit(h, p);
  h->io_stride = (max_batch + 63) / 64 * 64;
  const size_t ws_bytes = (size_t)h->ws_stride * (size_t)(h->io_stride / 64) * (f32 ? sizeof(float) : sizeof(double));
  auto fail = [&](hipError_t e, const char *what) { g_last_error = std::string(what) + ": " + hipGetErrorString(e); mpc_destroy(h); return MPC_ERR_HIP; };
  hipError_t e;
  if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) return fail(e, "hipStreamCreate");
  if ((e = hipEventCreate(&h->ev0)) != hipSuccess) return fail(e, "hipEventCreate");
  if ((e = hipEventCreate(&h->ev1)) != hipSuccess) return fail(e, "hipEventCreate");
  if ((e = hipMalloc((void **)&h->ws, ws_bytes)) != hipSuccess) return fail(e, "hipMalloc(workspace)");
  if ((e = hipMalloc((void **)&h->d_status, sizeof(int32_t) * h->io_stride)) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = hipMalloc((void **)&h->d_iters, sizeof(int32_t) * h->io_stride)) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = hipMalloc((void **)&h->d_counter, kCounterRing * kCounterInts * sizeof(int32_t))) != hipSuccess) return fail(e, "hipMalloc");
  /* (on the handle's own stream and waited for: a plain hipMemset of device memory is ordered on the null stream only, which the
   * non-blocking streams the launches run on do not wait for) */
  if ((e = hipMemsetAsync(h->d_counter, 0, kCounterRing * kCounterInts * sizeof(int32_t), h->stream)) != hipSuccess) return fail(e, "hipMemset");
  if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return fail(e, "hipStreamSynchronize");
  if ((e = hipMalloc((void **)&h->d_stats, kStatWords * sizeof(unsigned long long))) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = hipEventCreateWithFlags(&h->ev_stats, hipEventDisableTiming)) != hipSuccess) return fail(e, "hipEventCreate");
  set_cuts(h, p);
  h->compact_gap = p->lane_compact >= 0 ? p->lane_compact : (p->N >= 15 ? 1 : 2);
  if (const char *e9 = getenv("MPC_LANE_COMPACT")) { h->compact_gap = atoi(e9); h->compact_env = true; if (h->compact_gap < 0) h->compact_gap = 0; }
  if (const char *e10 = getenv("MPC_TAKE_ORDER")) { h->take_order = atoi(e10); if (h->take_order < 0 || h->take_order > 2) h->take_order = 0; }
  h->promote_buffer = p->f32_phase_refill != 0;
  *out = h;
  return MPC_OK;
}

static int tail_drain(MpcHandle *h);

extern "C" int mpc_set_params(MpcHandle *h, const MpcParams *p) {
  if (!h) return MPC_ERR_INVALID;
  int rc = validate_params(p);
  if (rc != MPC_OK) return rc;
  if (wants_mixed(p, h->max_batch) != h->mixed) {
    g_last_error = "f32_finish / f64_f32_start cannot change on a live handle (they decide the workspaces)"; return MPC_ERR_INVALID;
  }
  if (p->N != h->params.N || p->precision != h->params.precision || (p->initial_state_rows != 0) != (h->params.initial_state_rows != 0)) {
    g_last_error = "N, precision and initial_state_rows cannot change on a live handle (they size the workspace)"; return MPC_ERR_INVALID;
  }
  if (h->tail_ready && (p->tail_ring != h->params.tail_ring || p->tail_capacity != h->params.tail_capacity)) {
    g_last_error = "tail_ring and tail_capacity cannot change once the tail queue exists"; return MPC_ERR_INVALID;
  }
  if (h->tail_ready) {
    /* stragglers of earlier batches are finished under the parameters their batch was issued with: every tail slice
     * takes the handle's parameters by value when it goes out, so what is still queued is finished first */
    MPC_ON_DEVICE(h);
    const int rf = tail_drain(h);
    if (rf != MPC_OK) return rf;
  }
  h->params = *p;
  set_cuts(h, p);
  set_wave_limit(h, p);
  if (!h->compact_env) h->compact_gap = p->lane_compact >= 0 ? p->lane_compact : (p->N >= 15 ? 1 : 2);
  h->promote_buffer = p->f32_phase_refill != 0;
  return MPC_OK;
}

extern "C" void mpc_destroy(MpcHandle *h) {
  if (!h) return;
  DeviceGuard guard_(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->ws) (void)hipFree(h->ws);
  if (h->d_io) (void)hipFree(h->d_io);
  if (h->h_io) (void)hipHostFree(h->h_io);
  if (h->d_stats) (void)hipFree(h->d_stats);
  if (h->ev_stats) (void)hipEventDestroy(h->ev_stats);
  if (h->d_run) (void)hipFree(h->d_run);
  if (h->d_run9) (void)hipFree(h->d_run9);
  if (h->d_status) (void)hipFree(h->d_status);
  if (h->d_iters) (void)hipFree(h->d_iters);
  if (h->d_rstat) (void)hipFree(h->d_rstat);
  if (h->d_counter) (void)hipFree(h->d_counter);
  if (h->ws2) (void)hipFree(h->ws2);
  if (h->soc_ws) (void)hipFree(h->soc_ws);
  if (h->d_park) (void)hipFree(h->d_park);
  if (h->d_list) (void)hipFree(h->d_list);
  if (h->d_take_list) (void)hipFree(h->d_take_list);
  if (h->d_piter) (void)hipFree(h->d_piter);
  if (h->d_tel) (void)hipFree(h->d_tel);
  if (h->d_drive) (void)hipFree(h->d_drive);
  if (h->d_drive_w) (void)hipFree(h->d_drive_w);
  if (h->d_drive_host) (void)hipFree(h->d_drive_host);
  if (h->d_warm) (void)hipFree(h->d_warm);
  if (h->d_model) (void)hipFree(h->d_model);
  if (h->d_warm_io) (void)hipFree(h->d_warm_io);
  if (h->d_warm_o) (void)hipFree(h->d_warm_o);
  if (h->d_horizon) (void)hipFree(h->d_horizon);
  if (h->d_budget) (void)hipFree(h->d_budget);
  if (h->d_warm_st) (void)hipFree(h->d_warm_st);
  if (h->tail_ready) (void)tail_drain(h);         /* stragglers still queued are finished: their batches' arrays may be read afterwards */
  if (h->tail_stream) (void)hipStreamSynchronize(h->tail_stream);
  for (void *q : {(void *)h->d_tcount, (void *)h->d_remaining, h->tail_ws, h->soc_tail, (void *)h->surv_dev[0].park, h->surv_dev[0].iter,
                  (void *)h->surv_dev[1].park, h->surv_dev[1].iter})
    if (q) (void)hipFree(q);
  for (int q = 0; q < kFreshRing; q++) {
    if (h->fq_dev[q].park) (void)hipFree(h->fq_dev[q].park);
    if (h->fq_dev[q].iter) (void)hipFree(h->fq_dev[q].iter);
    if (h->fq[q].bulk) (void)hipEventDestroy(h->fq[q].bulk);
  }
  if (h->h_final) (void)hipHostFree(h->h_final);
  if (h->h_res) (void)hipHostFree(h->h_res);
  for (int q = 0; q < kSliceRing; q++) if (h->slice_ev[q]) (void)hipEventDestroy(h->slice_ev[q]);
  if (h->brec) {
    for (int q = 0; q < MpcHandle::kBatchRecs; q++) if (h->brec[q].ev) (void)hipEventDestroy(h->brec[q].ev);
    delete[] h->brec;
  }
  if (h->tail_stream) (void)hipStreamDestroy(h->tail_stream);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

/* statistics of (status, iters) into the handle's own counters, behind whatever wrote them on stream s */
static int record_stats(MpcHandle *h, int64_t B, const int32_t *status, const int32_t *iters, hipStream_t s) {
  MPC_HIP_CHECK(hipMemsetAsync(h->d_stats, 0, kStatWords * sizeof(unsigned long long), s));
  unsigned grid = (unsigned)((B + 256 * 8 - 1) / (256 * 8));
  if (grid > 256) grid = 256;
  hipLaunchKernelGGL(mpc_stats_kernel, dim3(grid), dim3(256), 0, s, B, status, iters, h->d_stats);
  MPC_HIP_CHECK(hipGetLastError());
  MPC_HIP_CHECK(hipEventRecord(h->ev_stats, s));
  h->have_stats = true;
  return MPC_OK;
}

/* The SOC records of `waves` wavefront tiles (fp64 solver), allocated once: N cannot change on a live handle */
static int soc_alloc(MpcHandle *h, void **buf, int64_t waves) {
  return ensure_dev(buf, sizeof(double) * (size_t)waves * (size_t)mpc::soc_fields_per_instance(h->params.N) * 64u);
}

/* ---- deferred tails: queues, tail slices, the pump, waiting for a batch -------------------------------------------------
 * A launch with a cut hands its stragglers to the FRESH QUEUE of its batch.  They are carried on by TAIL SLICES
 * (mpc_tail_slice_kernel) on the handle's own high-priority stream: slice k reads the survivors slice k-1 left and the fresh
 * queues of the batches whose launches have ended since, works for a bounded number of passes, and leaves its own survivors.
 * Slices are started by the PUMP (tail_pump), which every solve call and every wait runs: it retires the slices that have
 * completed (reads their counters and the final flags), and starts the next one while at most two are in flight.  Nothing
 * runs between calls: a batch is final when mpc_tail_wait / mpc_tail_poll / mpc_tail_stream_wait says so. */
static int tail_alloc_queue(MpcHandle *h, MpcTailQ &Q, int64_t cap, int32_t *count) {
  const bool f32 = !h->tail_double;
  const size_t real_bytes = f32 ? sizeof(float) : sizeof(double);
  const size_t it_sz = f32 ? (size_t)mpc::Fields<float>::IT_SZ : (size_t)mpc::Fields<double>::IT_SZ;
  Q.cap = (int32_t)cap; Q.count = count;
  MPC_TRY(ensure_dev(&Q.park, sizeof(double) * (size_t)kTailRows * (size_t)cap));
  return ensure_dev(&Q.iter, (size_t)(cap / 64) * (size_t)(h->params.N - 1) * it_sz * 64 * real_bytes);
}

static int tail_prepare(MpcHandle *h) {
  if (h->tail_ready) return MPC_OK;
  const MpcParams &P = h->params;
  h->tail_double = P.precision != MPC_PRECISION_F32 || h->mixed;      /* a mixed-precision solve defers in its fp64 phase */
  const bool f32 = !h->tail_double;
  const size_t real_bytes = f32 ? sizeof(float) : sizeof(double);
  const int64_t tail_stride = f32 ? h->ws_stride_f32 : h->ws_stride_f64;
  h->tail_ring = P.tail_ring < 2 ? 2 : (P.tail_ring > kTailMaxRing ? kTailMaxRing : P.tail_ring);
  int64_t cap = P.tail_capacity > 0 ? P.tail_capacity : h->max_batch / 8;
  if (cap < 256) cap = 256;
  if (cap > h->io_stride) cap = h->io_stride;
  h->tail_cap = (cap + 63) / 64 * 64;
  /* survivors: everything the outstanding batches may have alive at once.  A slice that finds the list full keeps the
   * instance until it is solved, and the solve calls stop deferring while the list is more than half full. */
  int64_t sc = 8 * h->tail_cap;
  if (sc < 16384) sc = 16384;
  h->surv_cap = (sc + 63) / 64 * 64;
  if (const char *e = getenv("MPC_TAIL_WAVES")) { h->tail_waves = atoi(e); if (h->tail_waves < 1) h->tail_waves = 1; }
  if (const char *e = getenv("MPC_SLICE_PASSES")) { h->slice_passes = atoi(e); if (h->slice_passes < 1) h->slice_passes = 1; }
  if (const char *e = getenv("MPC_TAIL_FEW")) { h->tail_few = atoi(e); if (h->tail_few < 0) h->tail_few = 0; }
  h->auto_cut = h->auto_base = P.N <= 12 ? 20 : 24;
  if (const char *e = getenv("MPC_TAIL_AUTO_CUT")) { h->auto_cut = atoi(e); if (h->auto_cut < 4) h->auto_cut = 4; }
  /* The tail stream's priority: high (MPC_TAIL_PRIORITY=low|normal|high to measure the others).  A slice is a few dozen waves that
   * must find free SIMDs on a device the launches keep full: at normal priority a slice at N = 25 waited 6-12 ms for its 1.8 ms of
   * work (p90 of the retirement interval 15-30 ms), the stragglers' backlog grew until every buffer set was taken, and the long
   * windows read 5.4 M solves/s where the launches alone give 7.6 M; at high priority 7.1-8.8 M.  At N = 10 it makes no
   * difference (46.8 M either way; an earlier build of the slices lost 3 % with it). */
  int lo = 0, hi = 0;
  MPC_HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));      /* lo = least, hi = greatest priority (numerically smaller) */
  int prio = hi;
  if (const char *e = getenv("MPC_TAIL_PRIORITY")) prio = !strcmp(e, "low") ? lo : (!strcmp(e, "normal") ? 0 : hi);
  h->tail_priority = prio;
  if (!h->tail_stream) MPC_HIP_CHECK(hipStreamCreateWithPriority(&h->tail_stream, hipStreamNonBlocking, prio));
  /* the counters start from zero BEFORE the first launch that adds to them is issued: cleared on the tail stream and waited for
   * below (a plain hipMemset runs on the null stream, which neither the caller's stream nor the tail stream waits for -- on a
   * device that other handles keep full its fill kernel can start after the launch that follows this call) */
  const int n_counts = kFreshRing + 2 + 6 * kSliceRing;
  MPC_TRY(ensure_dev(&h->d_tcount, sizeof(int32_t) * n_counts));
  MPC_HIP_CHECK(hipMemsetAsync(h->d_tcount, 0, sizeof(int32_t) * n_counts, h->tail_stream));
  MPC_TRY(ensure_dev(&h->d_remaining, sizeof(int32_t) * kTailMaxRing));
  MPC_HIP_CHECK(hipMemsetAsync(h->d_remaining, 0, sizeof(int32_t) * kTailMaxRing, h->tail_stream));
  if (!h->h_final) MPC_HIP_CHECK(hipHostMalloc((void **)&h->h_final, sizeof(long long) * kTailMaxRing, hipHostMallocDefault));
  if (!h->h_res) MPC_HIP_CHECK(hipHostMalloc((void **)&h->h_res, sizeof(MpcHandle::SliceRes) * kSliceRing, hipHostMallocDefault));
  memset(h->h_final, 0, sizeof(long long) * kTailMaxRing);
  memset(h->h_res, 0, sizeof(MpcHandle::SliceRes) * kSliceRing);
  for (int q = 0; q < kFreshRing; q++) {
    MPC_TRY(tail_alloc_queue(h, h->fq_dev[q], h->tail_cap, h->d_tcount + q));
    if (!h->fq[q].bulk) MPC_HIP_CHECK(hipEventCreateWithFlags(&h->fq[q].bulk, hipEventDisableTiming));
  }
  for (int q = 0; q < 2; q++) MPC_TRY(tail_alloc_queue(h, h->surv_dev[q], h->surv_cap, h->d_tcount + kFreshRing + q));
  MPC_TRY(ensure_dev(&h->tail_ws, (size_t)tail_stride * (size_t)h->tail_waves * real_bytes));
  for (int q = 0; q < kSliceRing; q++)
    if (!h->slice_ev[q]) MPC_HIP_CHECK(hipEventCreateWithFlags(&h->slice_ev[q], hipEventDisableTiming));
  MPC_HIP_CHECK(hipStreamSynchronize(h->tail_stream));
  h->tail_ready = true;
  return MPC_OK;
}

/* the records of the last solve calls (allocated with the first one) */
static int batch_rec(MpcHandle *h, int64_t id, MpcHandle::BatchRec **out) {
  if (!h->brec) h->brec = new MpcHandle::BatchRec[MpcHandle::kBatchRecs];
  MpcHandle::BatchRec &R = h->brec[id % MpcHandle::kBatchRecs];
  if (!R.ev) MPC_HIP_CHECK(hipEventCreateWithFlags(&R.ev, hipEventDisableTiming));
  *out = &R;
  return MPC_OK;
}

static int tail_retire(MpcHandle *h, bool block, int *n_retired);

static FILE *g_tail_trace = nullptr;
static std::once_flag g_tail_trace_once;
static int64_t now_us() { return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static FILE *tail_trace() {
  std::call_once(g_tail_trace_once, [] { if (const char *e = getenv("MPC_TAIL_TRACE")) g_tail_trace = fopen(e, "a"); });
  return g_tail_trace;
}

/* Starts tail slice number h->n_slice.  It absorbs every filled fresh queue whose launch has ended (`force`: every filled one --
 * the slice then waits for those launches on the device). */
static int tail_launch_slice(MpcHandle *h, bool force) {
  while (h->n_slice - h->n_slice_done >= kSliceRing - 1) {      /* (the result blocks are a ring: never more than kSliceRing - 1 in flight) */
    int nr = 0;
    const int rc = tail_retire(h, true, &nr);
    if (rc != MPC_OK) return rc;
  }
  const int64_t k = h->n_slice;
  const int kr = (int)(k % kSliceRing);
  hipStream_t ts = h->tail_stream;
  MpcSliceArgs A;
  memset(&A, 0, sizeof(A));
  A.src[0] = h->surv_dev[k & 1];
  A.dst = h->surv_dev[(k + 1) & 1];
  A.n_src = 1;
  h->slice_nabs[kr] = 0;
  int64_t est = h->surv_last;
  /* oldest batch first */
  for (int step = 0; step < kFreshRing; step++) {
    int best = -1;
    for (int q = 0; q < kFreshRing; q++)
      if (h->fq[q].state == 1 && (best < 0 || h->fq[q].batch_id < h->fq[best].batch_id)) best = q;
    if (best < 0) break;
    MpcHandle::FreshQ &F = h->fq[best];
    if (!force) {
      const hipError_t e = hipEventQuery(F.bulk);
      if (e == hipErrorNotReady) { (void)hipGetLastError(); break; }      /* (launches of one handle end in the order they were issued, or nearly) */
      if (e != hipSuccess) { g_last_error = std::string("hipEventQuery: ") + hipGetErrorString(e); return MPC_ERR_HIP; }
    }
    MPC_HIP_CHECK(hipStreamWaitEvent(ts, F.bulk, 0));
    const int j = A.n_src++;
    A.src[j] = h->fq_dev[best]; A.fresh_slot[j] = F.slot; A.fresh_batch[j] = F.batch_id;
    F.state = 2; F.slice = k;
    h->slice_abs[kr][h->slice_nabs[kr]++] = MpcHandle::Absorbed{best, F.slot, F.batch_id};
    est += (h->fresh_avg + kSliceFreshDiv - 1) / kSliceFreshDiv;
  }
  A.budget = h->slice_passes; A.ring = h->tail_ring;
  h->h_res[kr].count[28] = 0;
  A.take = h->d_tcount + kFreshRing + 2 + kr; A.done = h->d_tcount + kFreshRing + 2 + kSliceRing + kr;
  A.remaining = h->d_remaining; A.final_id = h->h_final; A.res = h->h_res[kr].count;
  A.tally = h->d_tcount + kFreshRing + 2 + 2 * kSliceRing + 4 * kr;
  int64_t waves = (est + 63) / 64 + 1;
  if (waves > h->tail_waves) waves = h->tail_waves;
  if (waves < 1) waves = 1;
  const bool f32 = !h->tail_double, io32 = h->params.precision == MPC_PRECISION_F32;
  const int64_t tail_stride = f32 ? h->ws_stride_f32 : h->ws_stride_f64;
  const bool soc = !f32 && h->params.max_soc > 0;     /* (the slice solves under the parameters it is launched with) */
  if (soc) MPC_TRY(soc_alloc(h, &h->soc_tail, h->tail_waves));
  A.soc_ws = h->soc_tail;
  auto go = [&](auto kernel, auto r) {       /* (r: a value of the solver's reals) */
    using R = decltype(r);
    hipLaunchKernelGGL(kernel, dim3((unsigned)waves), dim3(kBlock), staging_lds_bytes<R>(), ts, h->params, A, (R *)h->tail_ws, tail_stride);
  };
  if (soc && io32) go(mpc_tail_slice_kernel<true, double, float, true>, double{});
  else if (soc) go(mpc_tail_slice_kernel<true, double, double, true>, double{});
  else if (f32) go(mpc_tail_slice_kernel<true, float>, float{});
  else if (io32) go(mpc_tail_slice_kernel<true, double, float>, double{});      /* the fp64 phase of a mixed-precision solve: fp32 arrays at the ABI */
  else go(mpc_tail_slice_kernel<true, double>, double{});
  MPC_HIP_CHECK(hipGetLastError());
  /* (what the pump reads when the slice has completed -- the survivors it left, what each absorbed batch handed over, the final
   * flags -- the slice's last wave writes into pinned host memory itself) */
  MPC_HIP_CHECK(hipEventRecord(h->slice_ev[kr], ts));
  if (tail_trace()) { h->slice_t0[kr] = now_us(); h->slice_est[kr] = est; h->slice_surv_in[kr] = h->surv_last; h->slice_waves[kr] = (int)waves; }
  ++h->n_slice;
  return MPC_OK;
}

/* Retires the completed slices in order (`block`: waits for the oldest one in flight first).  Returns how many it retired. */
static int tail_retire(MpcHandle *h, bool block, int *n_retired) {
  *n_retired = 0;
  while (h->n_slice_done < h->n_slice) {
    const int kr = (int)(h->n_slice_done % kSliceRing);
    if (block) MPC_HIP_CHECK(hipEventSynchronize(h->slice_ev[kr]));
    else {
      const hipError_t e = hipEventQuery(h->slice_ev[kr]);
      if (e == hipErrorNotReady) { (void)hipGetLastError(); break; }
      if (e != hipSuccess) { g_last_error = std::string("hipEventQuery: ") + hipGetErrorString(e); return MPC_ERR_HIP; }
    }
    block = false;
    const MpcHandle::SliceRes &res = h->h_res[kr];
    if (res.count[28] != 0) {
      g_last_error = "tail slice: a damaged queue entry (slot " + std::to_string(res.count[29]) + ", instance " + std::to_string(res.count[30]) + ") was dropped";
      return MPC_ERR_HIP;
    }
    h->surv_last = res.count[0] < h->surv_cap ? res.count[0] : h->surv_cap;
    if (FILE *f = tail_trace()) {
      int64_t fresh = 0;
      for (int a = 0; a < h->slice_nabs[kr]; a++) fresh += res.count[1 + a];
      /* handle, slice, issued at / seen complete at (host, microseconds), waves, fresh queues absorbed, survivors known when it was issued,
       * fresh entries, survivors left, finished, moved on untouched, parked again, most passes of a wave, batches not final, slices in flight */
      fprintf(f, "%p %lld %lld %lld %d %d %lld %lld %d %d %d %d %d %d %lld\n", (void *)h, (long long)h->n_slice_done, (long long)h->slice_t0[kr], (long long)now_us(),
              h->slice_waves[kr], h->slice_nabs[kr], (long long)h->slice_surv_in[kr], (long long)fresh, res.count[0], res.count[25], res.count[26], res.count[27],
              res.count[31], (int)h->n_not_final, (long long)(h->n_slice - h->n_slice_done));
    }
    for (int a = 0; a < h->slice_nabs[kr]; a++) {
      const MpcHandle::Absorbed &Ab = h->slice_abs[kr][a];
      MpcHandle::FreshQ &F = h->fq[Ab.fq];
      const int64_t c = res.count[1 + a] < h->tail_cap ? res.count[1 + a] : h->tail_cap;
      /* the queue was too small for what the cut sent its way: the rest of that batch finished in its launch, stragglers included.
       * MPC_TAIL_AUTO moves its cut out of the way (an explicit cut is the caller's: mpc_tail_info counts the overflows) */
      if (res.count[1 + a] > h->tail_cap) { ++h->n_overflow; if (h->params.tail_cut < 0 && h->auto_cut < h->auto_base + 40) h->auto_cut += 4; }
      /* (the queue may hold a later batch by now: a launch may take it again as soon as the slice that absorbed it has been
       * ISSUED -- its stream waits for that slice -- which can be before this retirement) */
      const bool still = F.state == 2 && F.batch_id == Ab.batch && F.slice == h->n_slice_done;
      if (h->tslot[Ab.slot].batch_id == Ab.batch) {
        h->tslot[Ab.slot].deferred = c;
        const int64_t Bs = h->tslot[Ab.slot].B > 0 ? h->tslot[Ab.slot].B : 1;
        const int64_t share = c * 65536 / Bs;
        h->auto_share = h->auto_share < 0 ? share : (3 * h->auto_share + share) / 4;
        /* MPC_TAIL_AUTO follows the workload: a cut that sends more than 8 % of a batch to the slices is too early for this
         * distribution of iteration counts (weight sweeps: mean 16-18 iterations, a fat tail) -- the slices would do the launches'
         * work; one that sends next to nothing can come back towards the handle's base value */
        if (h->params.tail_cut < 0) {
          if (h->auto_share > kAutoShareHi && h->auto_cut < h->auto_base + 40) h->auto_cut += 2;
          else if (h->auto_share < kAutoShareLo && h->auto_cut > h->auto_base) --h->auto_cut;
        }
      }
      h->fresh_avg = (3 * h->fresh_avg + c + 3) / 4;
      if (still) F.state = 0;
    }
    h->slice_nabs[kr] = 0;
    const volatile long long *fin = h->h_final;
    for (int q = 0; q < h->tail_ring; q++) {
      MpcHandle::TailSlot &S = h->tslot[q];
      if (S.batch_id != 0 && !S.final_ && fin[q] == (long long)S.batch_id) { S.final_ = true; --h->n_not_final; }
    }
    ++h->n_slice_done;
    ++*n_retired;
  }
  return MPC_OK;
}

static bool tail_has_filled(const MpcHandle *h) {
  for (int q = 0; q < kFreshRing; q++) if (h->fq[q].state == 1) return true;
  return false;
}

/* One turn of the pump: retire what has completed, start slices while fewer than two are in flight and there is (or may be)
 * something for them to do.  `block`: wait for the oldest slice in flight, or -- if none is -- for the launches whose fresh
 * queues are filled, so that every call makes progress towards "everything final". */
static int tail_pump(MpcHandle *h, bool block) {
  if (!h->tail_ready) return MPC_OK;
  int n = 0;
  int rc = tail_retire(h, block && h->n_slice_done < h->n_slice, &n);
  if (rc != MPC_OK) return rc;
  for (int turn = 0; turn < 2 && h->n_slice - h->n_slice_done < 2; turn++) {
    const bool in_flight = h->n_slice_done < h->n_slice;
    const bool filled = tail_has_filled(h);
    const bool force = block && !in_flight && h->surv_last == 0 && n == 0;
    bool ready = false;
    if (filled && !force)
      for (int q = 0; q < kFreshRing && !ready; q++)
        if (h->fq[q].state == 1) { const hipError_t e = hipEventQuery(h->fq[q].bulk); if (e == hipSuccess) ready = true; else (void)hipGetLastError(); }
    /* (survivors: the slice in flight leaves some if the one before it did -- the second slice takes them along as its
     * source 0 whatever their number, so no time passes between two slices while the host is elsewhere) */
    if (!(ready || (filled && force) || h->surv_last > 0)) break;
    rc = tail_launch_slice(h, force);
    if (rc != MPC_OK) return rc;
  }
  return MPC_OK;
}

/* everything handed over so far is finished (blocks) */
static int tail_drain(MpcHandle *h) {
  if (!h->tail_ready) return MPC_OK;
  for (int guard = 0; guard < (1 << 24); guard++) {
    if (h->n_not_final == 0 && h->n_slice_done == h->n_slice && !tail_has_filled(h) && h->surv_last == 0) return MPC_OK;
    const int rc = tail_pump(h, true);
    if (rc != MPC_OK) return rc;
  }
  g_last_error = "tail_drain: no progress";
  return MPC_ERR_HIP;
}

extern "C" int64_t mpc_last_batch_id(const MpcHandle *h) { return h ? h->batch_seq : 0; }

extern "C" int mpc_tail_flush(MpcHandle *h) {
  if (!h) return MPC_ERR_INVALID;
  MPC_ON_DEVICE(h);
  return tail_pump(h, false);
}

/* 1: batch `id` is final, 0: not yet (after one non-blocking turn of the pump); < 0: error */
static int tail_poll_id(MpcHandle *h, int64_t id, bool pump) {
  if (id <= 0 || id > h->batch_seq) { g_last_error = "no such batch id"; return MPC_ERR_INVALID; }
  if (!h->brec) { g_last_error = "no such batch id"; return MPC_ERR_INVALID; }
  MpcHandle::BatchRec &R = h->brec[id % MpcHandle::kBatchRecs];
  if (R.id != id) { g_last_error = "batch id too old to resolve (the handle keeps the last 1024)"; return MPC_ERR_INVALID; }
  if (R.kind == 2) return 1;                           /* an empty batch */
  if (R.kind == 0) {
    const hipError_t e = hipEventQuery(R.ev);
    if (e == hipSuccess) return 1;
    (void)hipGetLastError();
    if (e == hipErrorNotReady) return 0;
    g_last_error = std::string("hipEventQuery: ") + hipGetErrorString(e);
    return MPC_ERR_HIP;
  }
  const MpcHandle::TailSlot &S = h->tslot[R.slot];
  if (S.batch_id != id || S.final_) return 1;        /* (a slot is only taken again once its batch is final) */
  if (pump) { const int rc = tail_pump(h, false); if (rc != MPC_OK) return rc; }
  return (S.batch_id != id || S.final_) ? 1 : 0;
}

extern "C" int mpc_tail_poll(MpcHandle *h, int64_t batch_id) {
  if (!h) return MPC_ERR_INVALID;
  MPC_ON_DEVICE(h);
  return tail_poll_id(h, batch_id, true);
}

extern "C" int mpc_tail_wait(MpcHandle *h, int64_t batch_id) {
  if (!h) return MPC_ERR_INVALID;
  MPC_ON_DEVICE(h);
  if (batch_id <= 0) {                         /* every batch issued so far: the deferring ones, and the launches of the rest */
    const int rc = tail_drain(h);
    if (rc != MPC_OK) return rc;
    if (h->brec)
      for (int64_t id = h->batch_seq; id > 0 && id > h->batch_seq - MpcHandle::kBatchRecs; --id) {
        MpcHandle::BatchRec &R = h->brec[id % MpcHandle::kBatchRecs];
        if (R.id == id && R.kind == 0 && R.ev) MPC_HIP_CHECK(hipEventSynchronize(R.ev));
      }
    return MPC_OK;
  }
  for (int guard = 0; guard < (1 << 24); guard++) {
    const int r = tail_poll_id(h, batch_id, false);
    if (r < 0) return r;
    if (r == 1) return MPC_OK;
    MpcHandle::BatchRec &R = h->brec[batch_id % MpcHandle::kBatchRecs];
    if (R.kind == 0) { MPC_HIP_CHECK(hipEventSynchronize(R.ev)); return MPC_OK; }
    const int rc = tail_pump(h, true);
    if (rc != MPC_OK) return rc;
  }
  g_last_error = "mpc_tail_wait: no progress";
  return MPC_ERR_HIP;
}

extern "C" int mpc_tail_stream_wait(MpcHandle *h, int64_t batch_id, void *stream) {
  if (!h) return MPC_ERR_INVALID;
  MPC_ON_DEVICE(h);
  if (batch_id <= 0 || batch_id > h->batch_seq || !h->brec) { g_last_error = "no such batch id"; return MPC_ERR_INVALID; }
  MpcHandle::BatchRec &R = h->brec[batch_id % MpcHandle::kBatchRecs];
  if (R.id != batch_id) { g_last_error = "batch id too old to resolve (the handle keeps the last 1024)"; return MPC_ERR_INVALID; }
  if (R.kind == 2) return MPC_OK;
  if (R.kind == 0) {                           /* not deferring: final behind its own launch */
    MPC_HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, R.ev, 0));
    return MPC_OK;
  }
  /* a deferring batch is final behind a slice that has not been issued yet: the host brings it there (the pump is what starts
   * slices), then orders `stream` behind the tail stream's most recent slice */
  const int rc = mpc_tail_wait(h, batch_id);
  if (rc != MPC_OK) return rc;
  if (h->n_slice > 0) MPC_HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, h->slice_ev[(h->n_slice - 1) % kSliceRing], 0));
  return MPC_OK;
}

/* counters of the handle's tail machinery: out[0] batches deferred so far, [1] tail slices so far, [2] ring, [3] capacity of a
 * batch's fresh queue, [4] waves per slice (upper bound), [5] 1 if the tail stream has high priority, [6] tail streams (1),
 * [7] batches that ran without deferral because the survivors' list was filling up, [8] passes per slice, [9] survivors now */
extern "C" int mpc_take_order_info(const MpcHandle *h, int64_t *out) {
  if (!h || !out) { g_last_error = "NULL argument"; return MPC_ERR_INVALID; }
  out[0] = h->n_take_ordered; out[1] = h->take_order;
  return MPC_OK;
}

extern "C" int mpc_tail_info(const MpcHandle *h, int64_t *out) {
  if (!h || !out) return MPC_ERR_INVALID;
  out[0] = h->n_deferred; out[1] = h->n_slice; out[2] = h->tail_ring; out[3] = h->tail_cap; out[4] = h->tail_waves;
  out[5] = h->tail_priority < 0 ? 1 : 0; out[6] = 1; out[7] = h->n_throttled; out[8] = h->slice_passes; out[9] = h->surv_last;
  out[10] = h->params.tail_cut > 0 ? h->params.tail_cut : (h->params.tail_cut < 0 ? h->auto_cut : 0); out[11] = h->auto_share;
  out[12] = h->n_overflow;
  return MPC_OK;
}

extern "C" int mpc_tail_pending(MpcHandle *h, int64_t batch_id, int64_t *n) {
  if (!h || !n) return MPC_ERR_INVALID;
  *n = 0;
  if (!h->tail_ready || !h->brec || batch_id <= 0 || batch_id > h->batch_seq) return MPC_OK;
  MPC_ON_DEVICE(h);
  MpcHandle::BatchRec &R = h->brec[batch_id % MpcHandle::kBatchRecs];
  if (R.id != batch_id || R.kind == 0) return MPC_OK;
  MpcHandle::TailSlot &S = h->tslot[R.slot];
  if (S.batch_id != batch_id) return MPC_OK;            /* long final: its slot holds a later batch */
  if (S.deferred >= 0) { *n = S.deferred; return MPC_OK; }
  for (int q = 0; q < kFreshRing; q++)
    if (h->fq[q].batch_id == batch_id && h->fq[q].state == 2) {       /* absorbed: the slice reports the count (and resets it) */
      for (int guard = 0; guard < 64 && S.deferred < 0 && h->n_slice_done < h->n_slice; guard++) {
        int nr = 0;
        const int rc = tail_retire(h, true, &nr);
        if (rc != MPC_OK) return rc;
      }
      *n = S.deferred >= 0 ? S.deferred : 0;
      return MPC_OK;
    }
  for (int q = 0; q < kFreshRing; q++)
    if (h->fq[q].batch_id == batch_id && h->fq[q].state == 1) {
      MPC_HIP_CHECK(hipEventSynchronize(h->fq[q].bulk));
      int32_t c = 0;
      MPC_HIP_CHECK(hipMemcpy(&c, h->fq_dev[q].count, sizeof(c), hipMemcpyDeviceToHost));
      *n = c < h->tail_cap ? c : h->tail_cap;
      return MPC_OK;
    }
  /* absorbed and retired in the meantime */
  int nr = 0;
  const int rc = tail_retire(h, false, &nr);
  if (rc != MPC_OK) return rc;
  *n = S.deferred >= 0 ? S.deferred : 0;
  return MPC_OK;
}

/* ---- the solve call: one description of it, one way to the device ----------------------------------------------------------
 * What a solve call works on, all arrays on the device: ld = leading dimension of the inputs, ldo = of out / traj.  Host side
 * only: launch_kernel is the one place that spells it out as kernel arguments. */
template <class R>
struct SolveIO {
  int64_t B, ld, ldo;
  const R *state, *coeffs, *yaw_lo, *yaw_hi, *weights;
  R *out, *traj;
  int32_t *status, *iters;
};
/* ... and what a warm call brings on top: the warm buffers and the options in effect, as the kernels take them */
using WarmIO = mpc::WarmCall;
/* What a call brings beyond its family's own arrays.  The entry points follow one rule (include/mpc_amd.h): the _model form puts
 * `model` behind the family's inputs, the _warm form `warm_in, warm_status, warm_out, ld_warm, opts` behind that.  call_extras turns
 * those arguments into this value and checks them against the handle; every family (the solve, run(), the telemetry handler, the
 * rollouts; device and host arrays) takes one and serves the four forms with it. */
struct CallExtras {
  int refused = MPC_OK;            /* call_extras' verdict, its text in g_last_error: a family returns it before it touches anything */
  bool warm = false;               /* a warm call: a _warm form, whichever arrays it brings -- with none it still runs the WARM build */
  WarmIO w{};                      /* ... its buffers and the options in effect */
  const double *model = nullptr;   /* a model call (fp64 handles): [MPC_NMODEL][ld_model], see MpcModelPart */
  int64_t ld_model = 0;            /* 0: the ld of the solve's inputs.  (run() sets its own: it solves from the handle's rows at the handle's stride, the columns stay where the caller has them) */
  bool model_wave = false;         /* a model call of the run() / telemetry entry points: the wave MODEL kernels up to wave_max_batch */
  const int32_t *horizon = nullptr;   /* a horizon call (fp64 handles, no SOC): [ld] like the inputs; dispatched as a model call, `model` may be NULL */
  const int32_t *budget = nullptr;    /* a budget call (include/mpc_amd_budget.h; fp64 handles, no SOC): [ld] like `horizon`, and dispatched like a horizon call -- `horizon` may be NULL */
  const double *latency = nullptr;   /* a latency call (fp64 handles): the telemetry handler's comp [ld]; the drive's [MPC_NLATENCY][ld] */
  const double *plant = nullptr;     /* a plant call (the drive, fp64 handles): [MPC_NPLANT][ld], what the cars are moved with */
  const double *noise = nullptr;     /* a noise call (the drive, include/mpc_amd_noise.h): [MPC_NNOISE][ld], what every message adds to what the handler is told and to the plant */
  double *seen = nullptr;            /* ... and its record of what the handler was told: [steps][4][ld] */
  bool senses() const { return noise != nullptr || seen != nullptr; }      /* the handler reads the handle's `seen` rows, not the car */
  const double *run_weights = nullptr;   /* run() / telemetry only (the drive loop): per-instance weights of the solve, [MPC_NW][io_stride] like the rows run() solves from */
  bool lane_rows() const { return horizon != nullptr || budget != nullptr; }      /* the call runs the lane kernel's per-lane-rows (HORIZON) build */
  bool model_call() const { return model != nullptr || lane_rows(); }
  const WarmIO *warm_io() const { return warm ? &w : nullptr; }
};
/* ... and where a deferring launch hands its stragglers: its batch's slot of the ring and its fresh queue */
struct TailPlace {
  bool defer = false;
  int slot = 0, fq = 0;
};
struct CounterBlocks { int32_t *cb, *zero_next; };

/* `extra`: what the kernel takes behind the solve arguments */
template <class K, class R, class... Extra>
static int launch_kernel(K kernel, unsigned grid, size_t lds, hipStream_t s, const MpcHandle *h, const SolveIO<R> &io, Extra... extra) {
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, s, h->params, io.B, io.ld, io.ldo, io.state, io.coeffs, io.yaw_lo, io.yaw_hi,
                     io.weights, io.out, io.traj, io.status, io.iters, extra...);
  MPC_HIP_CHECK(hipGetLastError());
  return MPC_OK;
}

template <int V> using Int = std::integral_constant<int, V>;
/* f(std::true_type) or f(std::false_type): a run-time switch as a template argument */
template <class F>
static int with_bool(bool b, F f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
/* f(soc, warm, model, horizon): the builds of an fp64 solve kernel, all eight of them -- plain, SOC, WARM, MODEL, MODEL+SOC,
 * MODEL+WARM, and the HORIZON builds of the lane kernel (MODEL builds by construction), cold and WARM.  A warm call has no SOC
 * (call_extras refuses it on a handle with max_soc > 0) and neither has a horizon call, so there is no SOC+WARM or SOC+HORIZON build.
 * (The wave path has no horizon: launch_wave passes false and never sees the last two.) */
template <class F>
static int with_build(bool soc, bool warm, bool model, bool horizon, F f) {
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  if (horizon) return warm ? f(no, yes, yes, yes) : f(no, no, yes, yes);
  if (warm) return model ? f(no, yes, yes, no) : f(no, yes, no, no);
  if (soc) return model ? f(yes, no, yes, no) : f(yes, no, no, no);
  return model ? f(no, no, yes, no) : f(no, no, no, no);
}
/* the argument a kernel takes only in the builds with ON: (*p) or nothing, for std::apply */
template <bool ON, class T>
static auto arg_if(const T *p) {
  if constexpr (ON) return std::make_tuple(*p);
  else return std::tuple<>{};
}

/* Every phase's switches are off unless it sets them; the hand-over and compaction policies are the same for all */
static MpcPhase phase_defaults(const MpcHandle *h, int64_t B) {
  MpcPhase T;
  memset(&T, 0, sizeof(T));
  T.ld_park = h->io_stride;
  T.refill_min = kRefillMin; T.refill_wait = kRefillWait;
  T.compact_gap = B >= h->compact_min_batch ? h->compact_gap : 0; T.compact_cooldown = kCompactCooldown;
  return T;
}

/* The counter block of a solve call that takes its work from counters (the wave path does not, and leaves the ring alone): call n
 * uses block n % kCounterRing, and its first launch zeroes the block half a ring ahead for a later call */
static CounterBlocks take_counters(MpcHandle *h) {
  const int64_t n = h->counter_seq++;
  return {h->d_counter + (n % kCounterRing) * kCounterInts, h->d_counter + ((n + kCounterRing / 2) % kCounterRing) * kCounterInts};
}

/* Lanes per instance on the wave path: a lane per stage -- 16 up to N = 17 (four instances per wavefront), 32 up to N = 33, else
 * the whole wave; a launch of a few instances takes the whole wave anyway (its cross-lane reads are v_readlane instead of
 * ds_bpermute).  MPC_WAVE_LPI in the environment overrides both (measurement aid, read per call). */
static int wave_lpi(const MpcHandle *h, int64_t B) {
  const int stages = h->params.N - 1;
  int lpi = stages <= 16 ? 16 : (stages <= 32 ? 32 : 64);
  if (B <= kWaveWholeMax) lpi = 64;
  if (const char *e = getenv("MPC_WAVE_LPI")) lpi = atoi(e) == 16 ? 16 : (atoi(e) == 32 ? 32 : 64);
  if (lpi < stages) lpi = 64;
  return lpi;
}

/* The wave path: 64 / LPI instances per wavefront, each with its stage records in LDS (the SOC build: and its SOC records behind
 * them).  fp64: the build with_build picks for (soc, warm, model.model); fp32: plain. */
template <class R>
static int launch_wave(MpcHandle *h, const SolveIO<R> &io, hipStream_t s, bool soc, const WarmIO *warm, const MpcModelPart &model) {
  const size_t per = (size_t)mpc::workspace_fields_per_instance(h->params.N, sizeof(R) == 4, h->params.initial_state_rows != 0) * sizeof(R);
  auto go = [&](auto lpi) {
    constexpr int LPI = decltype(lpi)::value, G = 64 / LPI;
    const unsigned grid = (unsigned)((io.B + G - 1) / G);
    if constexpr (sizeof(R) == 8) {
      return with_build(soc, warm != nullptr, model.model != nullptr, false, [&](auto soc_build, auto warm_build, auto model_build, auto) {
        constexpr bool SOC = decltype(soc_build)::value, WARM = decltype(warm_build)::value, MODEL = decltype(model_build)::value;
        const size_t lds = G * (per + (SOC ? (size_t)mpc::soc_fields_per_instance(h->params.N) * sizeof(R) : 0));
        return std::apply([&](auto... extra) {
          return launch_kernel(mpc_solve_wave_kernel<R, LPI, SOC, WARM, MODEL, decltype(extra)...>, grid, lds, s, h, io, extra...);
        }, std::tuple_cat(arg_if<WARM>(warm), arg_if<MODEL>(&model)));
      });
    } else {
      return launch_kernel(mpc_solve_wave_kernel<R, LPI>, grid, G * per, s, h, io);
    }
  };
  switch (wave_lpi(h, io.B)) {
    case 16: return go(Int<16>{});
    case 32: return go(Int<32>{});
    default: return go(Int<64>{});
  }
}

/* The lane kernel (an instance per lane; `ws`: the workspace of the phase).  single: the build that MPC_STAGING and, on an fp64
 * handle, with_build select: max_soc, a warm call, a model call (model.model), a horizon call (`horizon`: the HORIZON builds, never
 * staged, their LDS the mailbox of lane compaction).  The two phases of a mixed-precision solve are builds of
 * their own: the fp32 solver, and the fp64 solver that takes its iterates from fp32 records -- whatever RIO, the type at the ABI, is. */
enum class LaneBuild { single, mixed_f32, mixed_f64 };
template <class RIO>
static int launch_lanes(MpcHandle *h, LaneBuild build, const SolveIO<RIO> &io, hipStream_t s, void *ws, bool soc, const MpcPhase &T,
                        const WarmIO *warm = nullptr, const MpcModelPart &model = {}, const MpcHorizonPart *lane_rows = nullptr) {
  const unsigned grid = (unsigned)((io.B + kBlock - 1) / kBlock);
  /* (r, rsrc: values of the solver's reals and of the reals its resumed iterates come in) */
  auto go = [&](auto staging, auto r, auto rsrc, auto soc_build, auto warm_build, int64_t tile_reals, auto model_build, auto horizon_build) {
    using R = decltype(r);
    constexpr bool HORIZON = decltype(horizon_build)::value, STAGING = decltype(staging)::value && !HORIZON;
    constexpr bool WARM = decltype(warm_build)::value, MODEL = decltype(model_build)::value;
    const size_t lds = HORIZON ? (T.compact_gap > 0 ? kMailboxBytes : 0) : STAGING ? staging_lds_bytes<R>() : 0;
    return launch_kernel(mpc_solve_kernel<STAGING, R, RIO, decltype(rsrc), decltype(soc_build)::value, WARM, false, MODEL, HORIZON>, grid, lds, s, h, io,
                         (R *)ws, tile_reals, phase_of<false, WARM, MODEL, HORIZON>(T, warm ? *warm : WarmIO{}, {}, model, lane_rows ? *lane_rows : MpcHorizonPart{}));
  };
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  if (build == LaneBuild::mixed_f32) return go(yes, float{}, RIO{}, no, no, h->ws_stride_f32, no, no);
  if (build == LaneBuild::mixed_f64) return with_bool(soc, [&](auto soc_build) { return go(yes, double{}, float{}, soc_build, no, h->ws_stride_f64, no, no); });
  return with_bool(h->staging, [&](auto staging) {
    if constexpr (sizeof(RIO) == 8) {
      return with_build(soc, warm != nullptr, model.model != nullptr, lane_rows != nullptr, [&](auto soc_build, auto warm_build, auto model_build, auto horizon_build) {
        return go(staging, RIO{}, RIO{}, soc_build, warm_build, h->ws_stride, model_build, horizon_build);
      });
    } else {
      return go(staging, RIO{}, RIO{}, no, no, h->ws_stride, no, no);
    }
  });
}

/* the tail fields of a phase that may hand instances over (defer = false: the batch's id only) */
static void tail_fields(const MpcHandle *h, const TailPlace &tp, MpcPhase &T) {
  T.tail_cut = tp.defer ? (h->params.tail_cut > 0 ? h->params.tail_cut : h->auto_cut) : 0; T.t_slot = tp.slot; T.t_batch = h->batch_seq;
  if (tp.defer) { T.tq = h->fq_dev[tp.fq]; T.tail_few = h->tail_few; T.tail_few_from = kTailFewFrom; }
}

/* Mixed precision across phases: phase 0 = the fp32 solver on the handle's fp32 workspace, parking every instance at
 * MPC_PROMOTE; phase 1 = the fp64 solver resuming all of them on the fp64 workspace.  RIO is the handle's own precision
 * (the type at the ABI).  Instances the fp32 phase finishes itself (rejected at set-up, not-a-number, iteration cap) are
 * final after phase 0. */
template <class RIO>
static int launch_mixed(MpcHandle *h, const SolveIO<RIO> &io, hipStream_t s, const TailPlace &tp) {
  const int64_t S = h->io_stride, tiles = S / 64, B = io.B;
  const bool soc = h->params.max_soc > 0;     /* the fp64 phase honours MpcParams.max_soc (the fp32 phase never corrects) */
  /* h->ws holds the handle's own layout; the phases need one workspace of each (each allocation on its own: a failure
   * leaves the handle usable for a retry, and mpc_destroy frees whatever exists) */
  MPC_TRY(ensure_dev(&h->ws2, sizeof(RIO) == 4 ? (size_t)h->ws_stride_f64 * tiles * sizeof(double) : (size_t)h->ws_stride_f32 * tiles * sizeof(float)));
  MPC_TRY(ensure_dev(&h->d_park, sizeof(double) * 2 * kParkRows * S));
  MPC_TRY(ensure_dev(&h->d_list, sizeof(int32_t) * 4 * S));
  if (h->promote_buffer) MPC_TRY(ensure_dev(&h->d_piter, sizeof(float) * (size_t)S * (size_t)(h->params.N - 1) * mpc::Fields<float>::IT_SZ));
  if (soc) MPC_TRY(soc_alloc(h, &h->soc_ws, tiles));
  void *ws32 = sizeof(RIO) == 4 ? h->ws : h->ws2, *ws64 = sizeof(RIO) == 4 ? h->ws2 : h->ws;
  const CounterBlocks C = take_counters(h);
  MPC_HIP_CHECK(hipEventRecord(h->ev0, s));
  MpcPhase T = phase_defaults(h, B);
  T.take = C.cb; T.n_out = C.cb + 1; T.zero_next = C.zero_next;
  T.out_inst = h->d_list; T.out_src = h->d_list + S; T.out_park = h->d_park;
  T.promote_out = 1;
  T.p_iter = h->promote_buffer ? h->d_piter : nullptr;
  if (!T.p_iter) T.compact_gap = 0;      /* (without the buffer a handed-over instance keeps its iterate in its column) */
  MPC_TRY(launch_lanes(h, LaneBuild::mixed_f32, io, s, ws32, false, T));
  MpcPhase U = phase_defaults(h, B);
  U.take = C.cb + 2; U.n_out = C.cb + 3; U.n_in = C.cb + 1;
  U.in_inst = h->d_list; U.in_src = h->d_list + S; U.in_park = h->d_park;
  U.out_inst = h->d_list + 2 * S; U.out_src = h->d_list + 3 * S; U.out_park = h->d_park + (int64_t)kParkRows * S;
  U.src_ws = ws32; U.src_tile_reals = h->ws_stride_f32;
  U.resume = 1; U.promote_in = 1;
  U.p_iter = T.p_iter;
  /* deferred tails: the fp64 phase hands its stragglers over (the fp32 phase's chains end at kPromoteIterCap anyway) */
  /* (no early hand-over of a wave's last lanes here: the waves of this phase are partly filled by construction) */
  tail_fields(h, tp, U); U.tail_few = 0;
  if (soc) U.soc_ws = h->soc_ws;
  return launch_lanes(h, LaneBuild::mixed_f64, io, s, ws64, soc, U);
}

/* A launch that wants to defer: brings the tail machinery up, turns the pump and claims the batch's slot and fresh queue -- or
 * decides against (tp.defer = false) */
static int tail_claim(MpcHandle *h, hipStream_t s, TailPlace &tp) {
  MPC_TRY(tail_prepare(h));
  MPC_TRY(tail_pump(h, false));
  /* the survivors' list is filling up (stragglers arrive faster than the slices finish them): this batch keeps its own */
  if (2 * h->surv_last > h->surv_cap) {
    tp.defer = false; ++h->n_throttled;
    if (h->params.tail_cut < 0 && h->auto_cut < h->auto_base + 40) h->auto_cut += 2;
    return MPC_OK;
  }
  tp.slot = (int)(h->n_deferred % h->tail_ring);
  tp.fq = (int)(h->n_deferred % kFreshRing);
  /* the slot is taken again: the batch it held must be final (only if the ring is shorter than the stragglers' latency) */
  for (int guard = 0; h->tslot[tp.slot].batch_id != 0 && !h->tslot[tp.slot].final_; guard++) {
    if (guard > (1 << 22)) { g_last_error = "deferred tails: no progress"; return MPC_ERR_HIP; }
    MPC_TRY(tail_pump(h, true));
  }
  /* the fresh queue is taken again: the slice that absorbed its previous batch must have read it */
  MpcHandle::FreshQ &F = h->fq[tp.fq];
  if (F.state == 1) MPC_TRY(tail_launch_slice(h, true));
  /* (its count is zero again: the slice's last wave has reset it) */
  if (F.state == 2) MPC_HIP_CHECK(hipStreamWaitEvent(s, h->slice_ev[F.slice % kSliceRing], 0));
  return MPC_OK;
}

/* What every solve call starts with: the checks, the batch's id (every call counts, an empty one too), the handle's device (`guard`
 * lives in the caller: as long as the call) and the batch's record.  *rec stays NULL for an empty batch: nothing is left to do. */
template <class R>
static int solve_begin(MpcHandle *h, const SolveIO<R> &io, const WarmIO *warm, std::optional<DeviceGuard> &guard, MpcHandle::BatchRec **rec) {
  if (!h) { g_last_error = "NULL handle"; return MPC_ERR_INVALID; }
  if ((h->params.precision == MPC_PRECISION_F32) != (sizeof(R) == 4)) {
    g_last_error = "this handle was created with the other precision: fp64 handles take the double entry points, "
                   "MPC_PRECISION_F32 handles mpc_solve_batch_device_f32";
    return MPC_ERR_INVALID;
  }
  const int64_t B = io.B;
  if (B < 0 || io.ld < B || io.ldo < B) { g_last_error = "ld < B"; return MPC_ERR_INVALID; }
  if (warm && (warm->warm_in || warm->warm_out) && warm->ld_warm < B) { g_last_error = "ld_warm < B"; return MPC_ERR_INVALID; }
  if (B > h->max_batch) { g_last_error = "B exceeds the handle's max_batch"; return MPC_ERR_INVALID; }
  h->last_B = B; h->timed = false; h->have_stats = false; h->stats_pending = false;
  ++h->batch_seq;
  if (B == 0) {                /* empty batch: nothing to read or write, pointers may be NULL; its id resolves as final */
    if (!h->brec) h->brec = new MpcHandle::BatchRec[MpcHandle::kBatchRecs];
    MpcHandle::BatchRec &R0 = h->brec[h->batch_seq % MpcHandle::kBatchRecs];
    R0.id = h->batch_seq; R0.kind = 2;
    return MPC_OK;
  }
  if (!io.state || !io.coeffs || !io.yaw_lo || !io.yaw_hi || !io.out || !io.status) { g_last_error = "NULL argument"; return MPC_ERR_INVALID; }
  guard.emplace(h->device);    /* workspace, lazy allocations and a NULL stream all belong to the handle's device */
  if (guard->err != hipSuccess) { g_last_error = std::string("hipSetDevice: ") + hipGetErrorString(guard->err); return MPC_ERR_HIP; }
  MPC_TRY(batch_rec(h, h->batch_seq, rec));
  (*rec)->id = 0;              /* (valid once the launch has been issued) */
  return MPC_OK;
}

/* ... and ends with, behind its last launch: the events, the batch's record (what mpc_tail_wait / _poll / _stream_wait resolve its
 * id with), the hand-over bookkeeping of a deferring batch, and what mpc_get_stats will gather if asked */
template <class R>
static int solve_end(MpcHandle *h, const SolveIO<R> &io, hipStream_t s, MpcHandle::BatchRec *rec, const TailPlace &tp, bool with_stats) {
  MPC_HIP_CHECK(hipEventRecord(h->ev1, s));
  h->timed = true;
  rec->id = h->batch_seq; rec->kind = tp.defer ? 1 : 0; rec->slot = tp.slot;
  MPC_HIP_CHECK(hipEventRecord(rec->ev, s));
  if (tp.defer) {
    MpcHandle::FreshQ &F = h->fq[tp.fq];
    F.batch_id = h->batch_seq; F.slot = tp.slot; F.state = 1; F.slice = -1;
    MPC_HIP_CHECK(hipEventRecord(F.bulk, s));
    MpcHandle::TailSlot &S = h->tslot[tp.slot];
    S.batch_id = h->batch_seq; S.final_ = false; S.deferred = -1; S.B = io.B;
    ++h->n_not_final;
    ++h->n_deferred;
    MPC_TRY(tail_pump(h, false));
  }
  if (with_stats) { h->st_status = io.status; h->st_iters = io.iters; h->st_B = io.B; h->st_ev = rec->ev; h->stats_pending = true; }
  return MPC_OK;
}

/* ---- warm start and per-instance model values: options of every call -------------------------------------------------------- */
extern "C" int64_t mpc_warm_rows(int N) { return (N < 3 || N > MPC_MAX_N) ? (int64_t)MPC_ERR_INVALID : (int64_t)(N - 1) * MPC_WARM_REC; }

extern "C" int mpc_warm_opts_default(MpcWarmOpts *o) {
  if (!o) return MPC_ERR_INVALID;
  memset(o, 0, sizeof(*o));
  /* DESIGN.md section 6i has the grid these come from: the fewest iterations among the settings without a status difference or a
   * fork against the oracle on either population -- the previous solution as it is, not moved on by a stage */
  o->size = (int32_t)sizeof(MpcWarmOpts); o->shift = 0; o->mu_init = 1e-6; o->bound_push = 1e-6; o->duals = 0;
  return MPC_OK;
}

/* What an entry point's model and warm arguments come to, checked before anything is touched -- in this order: the handle; which
 * handles are accepted; no SOC for a warm call; the options.  `warm`: the call came through a _warm form (the fused rollout:
 * warm_start != 0).  The model rule decides which handles a model call is accepted on, warm or not -- every fp64 handle, also one
 * whose ordinary solve starts in fp32, because a model call is the single-phase fp64 launch on every handle; a warm call without
 * model needs an fp64 handle that does not start in fp32.  A call with neither is checked for its handle only. */
static CallExtras call_extras(const MpcHandle *h, const double *model = nullptr, bool warm = false, const double *warm_in = nullptr,
                              const int32_t *warm_status = nullptr, double *warm_out = nullptr, int64_t ld_warm = 0,
                              const MpcWarmOpts *opts = nullptr, const int32_t *horizon = nullptr, const double *latency = nullptr,
                              const int32_t *budget = nullptr) {
  CallExtras x;
  x.warm = warm; x.model = model; x.horizon = horizon; x.latency = latency; x.budget = budget;
  x.w = WarmIO{warm_in, warm_status, warm_out, ld_warm, {}, 0};
  const auto refuse = [&x](int rc, const char *why) { g_last_error = why; x.refused = rc; return x; };
  if (!h) return refuse(MPC_ERR_INVALID, "NULL handle");
  const bool f64 = h->params.precision == MPC_PRECISION_F64;
  if ((model || horizon || budget) && !f64) return refuse(MPC_ERR_INVALID, "per-instance model values: fp64 handles only (this one was created with MPC_PRECISION_F32)");
  if (horizon && h->params.max_soc > 0)
    return refuse(MPC_ERR_UNSUPPORTED, "a per-instance horizon is not available with the second-order correction (max_soc > 0): set MpcParams.max_soc = 0, or pass horizon = NULL");
  if (budget && h->params.max_soc > 0)
    return refuse(MPC_ERR_UNSUPPORTED, "a per-instance iteration budget is not available with the second-order correction (max_soc > 0): set MpcParams.max_soc = 0, or pass budget = NULL");
  if (latency && !f64) return refuse(MPC_ERR_INVALID, "per-instance latency: fp64 handles only (this one was created with MPC_PRECISION_F32)");
  if (!warm) return x;
  const bool as_model = model || horizon || budget;      /* (a horizon call and a budget call are dispatched as model calls: the model rule decides) */
  if (!as_model && !f64) return refuse(MPC_ERR_INVALID, "warm start: fp64 handles only (this one was created with MPC_PRECISION_F32)");
  if (!as_model && h->mixed)
    return refuse(MPC_ERR_UNSUPPORTED, "warm start is not available on a handle whose solve starts in fp32 (two launches): create it with MpcParams.f64_f32_start = 0");
  if (h->params.max_soc > 0) return refuse(MPC_ERR_UNSUPPORTED, "warm start is not available with the second-order correction: set MpcParams.max_soc = 0");
  (void)mpc_warm_opts_default(&x.w.wopts);
  if (opts) {
    if (opts->size != (int32_t)sizeof(MpcWarmOpts)) return refuse(MPC_ERR_INVALID, "MpcWarmOpts.size mismatch (fill it with mpc_warm_opts_default)");
    if ((opts->shift != 0 && opts->shift != 1) || (opts->duals != 0 && opts->duals != 1) || !(opts->mu_init > 0 && opts->mu_init <= 0.1) ||
        !(opts->bound_push > 0 && opts->bound_push <= 1e-2))
      return refuse(MPC_ERR_INVALID, "MpcWarmOpts: shift and duals are 0 or 1, 0 < mu_init <= 0.1, 0 < bound_push <= 1e-2");
    x.w.wopts = *opts;
  }
  return x;
}

/* The launch, for every entry point.  flags: kStats -- mpc_get_stats may ask about this call; kDefer -- the caller can wait for the
 * batch's stragglers (mpc_tail_wait); kOrder -- the take order may be applied.  x.warm: a warm call (an fp64 handle, no SOC; without
 * model: not mixed) -- a single phase of the WARM build, or the warm wave kernel; it never defers, cuts or orders.
 * x.model: a model call (an fp64 handle) -- ONE launch of the MODEL build of the single-phase fp64 lane
 * kernel on h->ws at every B, also on a handle whose ordinary solve starts in fp32 (on an fp64 handle h->ws has the fp64 layout):
 * no wave path, no mixed-precision launch, and it never defers, cuts or orders either.  x.warm and x.model together: the same one
 * launch, of the WARM+MODEL build -- lane compaction included, as for a warm call.
 * x.model_wave (the run() / telemetry model entry points, where the small batch is the rule): up to wave_max_batch the one launch
 * is the wave kernel's MODEL build instead -- cold, SOC or warm, launch_wave's own choice of lanes per instance and LDS. */
enum SolveFlag : unsigned { kStats = 1u, kDefer = 2u, kOrder = 4u };
template <class R>
static int launch_solve(MpcHandle *h, const SolveIO<R> &call, void *stream_, unsigned flags, const CallExtras &x) {
  MPC_TRY(x.refused);
  const WarmIO *warm = x.warm_io();
  std::optional<DeviceGuard> guard;
  MpcHandle::BatchRec *rec = nullptr;
  MPC_TRY(solve_begin(h, call, warm, guard, &rec));
  if (!rec) return MPC_OK;
  SolveIO<R> io = call;
  if (!io.iters) io.iters = h->d_iters;
  const int64_t B = io.B;
  hipStream_t s = (hipStream_t)stream_;   /* NULL = HIP's default (null) stream, exactly as passed */
  const MpcModelPart mp{x.model, x.ld_model ? x.ld_model : io.ld};
  const bool model = x.model_call();
  const bool may_defer = (flags & kDefer) && !warm && !model, may_order = (flags & kOrder) && !warm && !model;
  /* MpcParams.max_soc > 0 on an fp64 handle: the SOC builds of the kernels (the mixed-precision launch decides for its fp64 phase
   * itself) */
  const bool soc = sizeof(R) == 8 && h->params.max_soc > 0;
  const bool wave_path = (!model || x.model_wave) && h->wave_max_batch > 0 && B <= h->wave_max_batch;      /* (comes first: set_wave_limit decides which handles have it) */
  TailPlace tp;
  tp.defer = may_defer && h->params.tail_cut != 0 && B >= kTailMinBatch && !wave_path;
  if (tp.defer) MPC_TRY(tail_claim(h, s, tp));
  if (wave_path) {
    MPC_HIP_CHECK(hipEventRecord(h->ev0, s));
    MPC_TRY(launch_wave(h, io, s, soc, warm, mp));
  } else if (h->mixed && !model) {
    MPC_TRY(launch_mixed(h, io, s, tp));
  } else {
    const int64_t S = h->io_stride;
    const int n_cuts = (!warm && !model && !tp.defer && B >= kPassCutMinBatch) ? h->n_cuts : 0;
    if (n_cuts > 0) {
      MPC_TRY(ensure_dev(&h->ws2, (size_t)h->ws_stride * (size_t)(S / 64) * sizeof(R)));
      MPC_TRY(ensure_dev(&h->d_park, sizeof(double) * 2 * kParkRows * S));
      MPC_TRY(ensure_dev(&h->d_list, sizeof(int32_t) * 4 * S));
    }
    if (soc) MPC_TRY(soc_alloc(h, &h->soc_ws, S / 64));
    /* take order: the key kernel goes ahead of the launch on its stream; its counts live behind the phase counters of the block */
    const bool ordered = may_order && h->take_order != 0 && sizeof(R) == 8 && n_cuts == 0 && !soc && !io.weights && h->params.N < 15 &&
                         B >= h->take_order_min_batch;
    if (ordered) MPC_TRY(ensure_dev(&h->d_take_list, sizeof(int32_t) * mpc::kTakeBins * S));
    const CounterBlocks C = take_counters(h);
    MPC_HIP_CHECK(hipEventRecord(h->ev0, s));
    if (ordered) {
      hipLaunchKernelGGL((mpc_take_key_kernel<R>), dim3((unsigned)((B + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, (float)(h->params.N * h->params.dt), B,
                         io.ld, io.state, io.coeffs, io.yaw_lo, io.yaw_hi, h->take_order == 2 ? 1 : 0, C.cb + kPhaseCounterInts, h->d_take_list, S);
      MPC_HIP_CHECK(hipGetLastError());
      ++h->n_take_ordered;
    }
    /* phase p takes from counter [2p], parks into list p & 1 and counts its parked instances in [2p + 1]; phase p > 0
     * reads list (p - 1) & 1 and the workspace of phase p - 1; every phase has the grid of the first (see MpcPhase) */
    for (int p = 0; p <= n_cuts; ++p) {
      MpcPhase T = phase_defaults(h, B);
      const int wr = p & 1, rd = wr ^ 1;
      T.take = C.cb + 2 * p;
      T.n_out = C.cb + 2 * p + 1;
      T.n_in = p > 0 ? C.cb + 2 * (p - 1) + 1 : nullptr;
      T.zero_next = p == 0 ? C.zero_next : nullptr;
      if (!warm) {
        if (h->d_list) {
          T.out_inst = h->d_list + (int64_t)(2 * wr) * S; T.out_src = h->d_list + (int64_t)(2 * wr + 1) * S;
          T.in_inst = h->d_list + (int64_t)(2 * rd) * S; T.in_src = h->d_list + (int64_t)(2 * rd + 1) * S;
        }
        if (h->d_park) { T.out_park = h->d_park + (int64_t)wr * kParkRows * S; T.in_park = h->d_park + (int64_t)rd * kParkRows * S; }
        T.src_ws = rd ? h->ws2 : h->ws;
        T.soc_ws = h->soc_ws;
      }
      T.pass_cut = p < n_cuts ? h->cuts[p] : 0;
      T.resume = p > 0;
      if (n_cuts > 0) T.compact_gap = 0;     /* (a phase that parks keeps iterates in its columns) */
      tail_fields(h, tp, T);
      if (ordered) { T.ord_cnt = C.cb + kPhaseCounterInts; T.ord_list = h->d_take_list; T.ord_ld = S; }
      const MpcHorizonPart hp{x.horizon, x.budget};      /* (a horizon or a budget call: the per-lane-rows build) */
      MPC_TRY(launch_lanes(h, LaneBuild::single, io, s, wr ? h->ws2 : h->ws, soc, T, warm, mp, x.lane_rows() ? &hp : nullptr));
    }
  }
  return solve_end(h, io, s, rec, tp, (flags & kStats) != 0);
}

/* The solve on device arrays, fp64: the four forms.  Only the plain one may defer its stragglers and apply the take order. */
extern "C" int mpc_solve_batch_device(MpcHandle *h, int64_t B, int64_t ld, const double *state,
                                      const double *coeffs, const double *yaw_lo, const double *yaw_hi,
                                      const double *weights, double *out, double *traj, int32_t *status,
                                      int32_t *iters, void *stream_) {
  return launch_solve<double>(h, {B, ld, ld, state, coeffs, yaw_lo, yaw_hi, weights, out, traj, status, iters}, stream_, kStats | kDefer | kOrder,
                              call_extras(h));
}

extern "C" int mpc_solve_batch_device_model(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                            const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                            double *out, double *traj, int32_t *status, int32_t *iters, void *stream_) {
  return launch_solve<double>(h, {B, ld, ld, state, coeffs, yaw_lo, yaw_hi, weights, out, traj, status, iters}, stream_,
                              model ? kStats : kStats | kDefer | kOrder, call_extras(h, model));
}

extern "C" int mpc_solve_batch_device_warm(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                           const double *yaw_lo, const double *yaw_hi, const double *weights, const double *warm_in,
                                           const int32_t *warm_status, double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts,
                                           double *out, double *traj, int32_t *status, int32_t *iters, void *stream_) {
  return launch_solve<double>(h, {B, ld, ld, state, coeffs, yaw_lo, yaw_hi, weights, out, traj, status, iters}, stream_, kStats,
                              call_extras(h, nullptr, true, warm_in, warm_status, warm_out, ld_warm, opts));
}

extern "C" int mpc_solve_batch_device_warm_model(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                                 const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                                 const double *warm_in, const int32_t *warm_status, double *warm_out, int64_t ld_warm,
                                                 const MpcWarmOpts *opts, double *out, double *traj, int32_t *status, int32_t *iters,
                                                 void *stream_) {
  return launch_solve<double>(h, {B, ld, ld, state, coeffs, yaw_lo, yaw_hi, weights, out, traj, status, iters}, stream_, kStats,
                              call_extras(h, model, true, warm_in, warm_status, warm_out, ld_warm, opts));
}

/* ... and the two _horizon forms: the _model forms plus `horizon` (NULL: the _model form itself, which with model == NULL is the plain one) */
extern "C" int mpc_solve_batch_device_horizon(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                              const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                              const int32_t *horizon, double *out, double *traj, int32_t *status, int32_t *iters, void *stream_) {
  return launch_solve<double>(h, {B, ld, ld, state, coeffs, yaw_lo, yaw_hi, weights, out, traj, status, iters}, stream_,
                              model || horizon ? kStats : kStats | kDefer | kOrder, call_extras(h, model, false, nullptr, nullptr, nullptr, 0, nullptr, horizon));
}

/* (include/mpc_amd_budget.h: the _warm_horizon form plus `budget` behind horizon; NULL is the _warm_horizon form itself) */
extern "C" int mpc_solve_batch_device_budget(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                             const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                             const int32_t *horizon, const int32_t *budget, const double *warm_in, const int32_t *warm_status,
                                             double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts, double *out, double *traj,
                                             int32_t *status, int32_t *iters, void *stream_) {
  return launch_solve<double>(h, {B, ld, ld, state, coeffs, yaw_lo, yaw_hi, weights, out, traj, status, iters}, stream_, kStats,
                              call_extras(h, model, true, warm_in, warm_status, warm_out, ld_warm, opts, horizon, nullptr, budget));
}
extern "C" int mpc_solve_batch_device_warm_horizon(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                                   const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                                   const int32_t *horizon, const double *warm_in, const int32_t *warm_status, double *warm_out,
                                                   int64_t ld_warm, const MpcWarmOpts *opts, double *out, double *traj, int32_t *status,
                                                   int32_t *iters, void *stream_) {
  return mpc_solve_batch_device_budget(h, B, ld, state, coeffs, yaw_lo, yaw_hi, weights, model, horizon, nullptr, warm_in, warm_status, warm_out, ld_warm, opts,
                                       out, traj, status, iters, stream_);
}

/* MPC_PRECISION_F32: the same solve with fp32 inputs, outputs and workspace (handle created with precision F32) */
extern "C" int mpc_solve_batch_device_f32(MpcHandle *h, int64_t B, int64_t ld, const float *state,
                                          const float *coeffs, const float *yaw_lo, const float *yaw_hi,
                                          const float *weights, float *out, float *traj, int32_t *status,
                                          int32_t *iters, void *stream_) {
  return launch_solve<float>(h, {B, ld, ld, state, coeffs, yaw_lo, yaw_hi, weights, out, traj, status, iters}, stream_, kStats | kDefer, call_extras(h));
}

/* run() for a batch; `tel` selects the telemetry rows as input (with latency compensation) and `cmd` the reply.  x.warm: the same
 * three kernels, the solve started from the previous call's records with their psi projected
 * into the box run_pre derives for this call (mpc::WarmColumn).  x.model (device, [MPC_NMODEL][ld]): the MODEL
 * forms of the pre and post kernels, and a model solve between them that reads its inputs from the handle's rows at the handle's
 * stride and the columns from the caller's array at the caller's ld (CallExtras::ld_model) -- the array is not copied.
 * x.latency (device, comp [ld], with tel): the pre kernel's build that compensates per instance; `extra` is not read.
 * x.horizon (device, [ld] int32): the solve between the two kernels is the horizon solve -- the lane kernel's HORIZON build at every
 * B, cold or warm, with or without model; the pre and post kernels do not read N and are the builds `model` alone selects.
 * x.budget (device, [ld] int32; no public entry point sets it here, the stepwise drive does): the solve is the budget solve -- the same
 * HORIZON build, with or without x.horizon. */
static int run_impl(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *pose, bool tel, double extra, double *ptsx,
                    double *ptsy, double *out8, double *cmd, double *traj, int32_t *status, int32_t *iters, double *pre,
                    void *stream_, CallExtras x) {
  MPC_TRY(x.refused);
  if (B > 0 && !(tel ? cmd : out8)) { g_last_error = "NULL argument"; return MPC_ERR_INVALID; }
  MPC_TRY(check_batch(h, B, ld));
  if (x.warm && (x.w.warm_in || x.w.warm_out) && x.w.ld_warm < B) { g_last_error = "ld_warm < B"; return MPC_ERR_INVALID; }
  if (npts < 3 || npts > mpc::RUN_MAX_PTS) { g_last_error = "npts must be 3..8"; return MPC_ERR_INVALID; }
  if (B == 0) { h->last_B = 0; return MPC_OK; }
  if (!pose || !ptsx || !ptsy || !status) { g_last_error = "NULL argument"; return MPC_ERR_INVALID; }
  /* the tables MPC::run() looks up (Vehicle.cpp:34-79) must exist, and the fit is built for orders 2..4
   * (Config::maxFitOrder <= 5, as in every config-*.json; the reference would go on to higher orders) */
  if (h->params.n_yaw_change_speeds < 1 || h->params.n_steer_speeds < 1) { g_last_error = "run(): empty speed tables (load a config-*.json)"; return MPC_ERR_INVALID; }
  if (h->params.max_fit_order > 5) { g_last_error = "run(): max_fit_order > 5 is not built (fit orders 2..4)"; return MPC_ERR_UNSUPPORTED; }
  MPC_ON_DEVICE(h);
  const int64_t S = h->io_stride;
  MPC_TRY(ensure_dev(&h->d_run, sizeof(double) * mpc::RUN_PRE_ROWS * S));
  MPC_TRY(grow_dev(&h->d_run9, &h->run9_bytes, sizeof(double) * 9 * ld));       /* solve()'s 9 rows, with the caller's leading dimension (traj shares it) */
  hipStream_t s = (hipStream_t)stream_;
  double *d_pre = h->d_run;
  const unsigned grid = (unsigned)((B + 255) / 256);
  const double *model = x.model;
  /* the two kernels around the solve: f(MODEL build or not, the argument the MODEL builds take behind the others) */
  const auto around = [&](auto f) { return model ? f(std::true_type{}, MpcModelPart{model, ld}) : f(std::false_type{}); };
  if (tel && x.latency)
    around([&](auto model_build, auto... mp) {
      hipLaunchKernelGGL((mpc_run_pre_comp_kernel<decltype(model_build)::value, decltype(mp)...>), dim3(grid), dim3(256), 0, s, h->params, B, ld, npts, pose,
                         x.latency, ptsx, ptsy, d_pre, S, mp...);
      return MPC_OK;
    });
  else around([&](auto model_build, auto... mp) {
    return with_bool(tel, [&](auto telemetry) {
      hipLaunchKernelGGL((mpc_run_pre_kernel<decltype(telemetry)::value, decltype(model_build)::value, decltype(mp)...>), dim3(grid), dim3(256), 0, s,
                         h->params, B, ld, npts, pose, tel ? extra : 0.0, ptsx, ptsy, d_pre, S, mp...);
      return MPC_OK;
    });
  });
  MPC_HIP_CHECK(hipGetLastError());
  x.w.psi_box = 1; x.ld_model = ld; x.model_wave = !x.lane_rows();      /* the run() path's own (a horizon or budget call has no wave path: the lane kernel's HORIZON build at every B) */
  MPC_TRY(launch_solve<double>(h, {B, S, ld, d_pre + mpc::RUN_PRE_STATE * S, d_pre + mpc::RUN_PRE_COEFFS * S, d_pre + mpc::RUN_PRE_YAW_LO * S,
                                   d_pre + mpc::RUN_PRE_YAW_HI * S, x.run_weights, h->d_run9, traj, status, iters}, stream_, kStats, x));
  around([&](auto model_build, auto... mp) {
    hipLaunchKernelGGL((mpc_run_post_kernel<decltype(model_build)::value, decltype(mp)...>), dim3(grid), dim3(256), 0, s, h->params, B, d_pre, S,
                       h->d_run9, ld, out8, cmd, ld, mp...);
    return MPC_OK;
  });
  MPC_HIP_CHECK(hipGetLastError());
  if (pre) MPC_HIP_CHECK(hipMemcpy2DAsync(pre, sizeof(double) * ld, d_pre, sizeof(double) * S, sizeof(double) * B, mpc::RUN_PRE_ROWS, hipMemcpyDeviceToDevice, s));
  return MPC_OK;
}

/* run() and the telemetry handler on device arrays: the four forms of each (include/mpc_amd.h, "warm start on the run() path" and
 * "per-instance model values on the run() path") */
extern "C" int mpc_run_batch_device(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *pose, double *ptsx,
                                    double *ptsy, double *out8, double *traj, int32_t *status, int32_t *iters,
                                    double *pre, void *stream_) {
  return run_impl(h, B, ld, npts, pose, false, 0.0, ptsx, ptsy, out8, nullptr, traj, status, iters, pre, stream_, call_extras(h));
}

extern "C" int mpc_telemetry_batch_device(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                                          double *ptsx, double *ptsy, double *cmd, double *out8, int32_t *status, void *stream_) {
  return run_impl(h, B, ld, npts, tel, true, extra_latency, ptsx, ptsy, out8, cmd, nullptr, status, nullptr, nullptr, stream_, call_extras(h));
}

extern "C" int mpc_run_batch_device_warm(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *pose, double *ptsx,
                                         double *ptsy, const double *warm_in, const int32_t *warm_status, double *warm_out,
                                         int64_t ld_warm, const MpcWarmOpts *opts, double *out8, double *traj, int32_t *status,
                                         int32_t *iters, double *pre, void *stream_) {
  return run_impl(h, B, ld, npts, pose, false, 0.0, ptsx, ptsy, out8, nullptr, traj, status, iters, pre, stream_,
                  call_extras(h, nullptr, true, warm_in, warm_status, warm_out, ld_warm, opts));
}

extern "C" int mpc_telemetry_batch_device_warm(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                                               double *ptsx, double *ptsy, const double *warm_in, const int32_t *warm_status,
                                               double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts, double *cmd, double *out8,
                                               int32_t *status, void *stream_) {
  return run_impl(h, B, ld, npts, tel, true, extra_latency, ptsx, ptsy, out8, cmd, nullptr, status, nullptr, nullptr, stream_,
                  call_extras(h, nullptr, true, warm_in, warm_status, warm_out, ld_warm, opts));
}

extern "C" int mpc_run_batch_device_model(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *pose, double *ptsx, double *ptsy,
                                          const double *model, double *out8, double *traj, int32_t *status, int32_t *iters, double *pre,
                                          void *stream_) {
  return run_impl(h, B, ld, npts, pose, false, 0.0, ptsx, ptsy, out8, nullptr, traj, status, iters, pre, stream_, call_extras(h, model));
}

extern "C" int mpc_telemetry_batch_device_model(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                                                double *ptsx, double *ptsy, const double *model, double *cmd, double *out8, int32_t *status,
                                                void *stream_) {
  return run_impl(h, B, ld, npts, tel, true, extra_latency, ptsx, ptsy, out8, cmd, nullptr, status, nullptr, nullptr, stream_, call_extras(h, model));
}

extern "C" int mpc_run_batch_device_warm_model(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *pose, double *ptsx,
                                               double *ptsy, const double *model, const double *warm_in, const int32_t *warm_status,
                                               double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts, double *out8, double *traj,
                                               int32_t *status, int32_t *iters, double *pre, void *stream_) {
  return run_impl(h, B, ld, npts, pose, false, 0.0, ptsx, ptsy, out8, nullptr, traj, status, iters, pre, stream_,
                  call_extras(h, model, true, warm_in, warm_status, warm_out, ld_warm, opts));
}

/* (include/mpc_amd_drive.h, "per-car horizon": the _latency form plus `horizon` behind model; NULL is the _latency form itself) */
extern "C" int mpc_telemetry_batch_device_horizon(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                                                  const double *comp, double *ptsx, double *ptsy, const double *model, const int32_t *horizon,
                                                  const double *warm_in, const int32_t *warm_status, double *warm_out, int64_t ld_warm,
                                                  const MpcWarmOpts *opts, double *cmd, double *out8, int32_t *status, void *stream_) {
  return run_impl(h, B, ld, npts, tel, true, extra_latency, ptsx, ptsy, out8, cmd, nullptr, status, nullptr, nullptr, stream_,
                  call_extras(h, model, true, warm_in, warm_status, warm_out, ld_warm, opts, horizon, comp));
}
extern "C" int mpc_telemetry_batch_device_latency(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                                                  const double *comp, double *ptsx, double *ptsy, const double *model, const double *warm_in,
                                                  const int32_t *warm_status, double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts,
                                                  double *cmd, double *out8, int32_t *status, void *stream_) {
  return mpc_telemetry_batch_device_horizon(h, B, ld, npts, tel, extra_latency, comp, ptsx, ptsy, model, nullptr, warm_in, warm_status, warm_out, ld_warm, opts,
                                            cmd, out8, status, stream_);
}
extern "C" int mpc_telemetry_batch_device_warm_model(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                                                     double *ptsx, double *ptsy, const double *model, const double *warm_in,
                                                     const int32_t *warm_status, double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts,
                                                     double *cmd, double *out8, int32_t *status, void *stream_) {
  return mpc_telemetry_batch_device_latency(h, B, ld, npts, tel, extra_latency, nullptr, ptsx, ptsy, model, warm_in, warm_status, warm_out, ld_warm, opts, cmd,
                                            out8, status, stream_);
}

/* A host-array call's extras (`hx`) on the device, *dx: what the launch gets.  The model columns are where the family has copied them
 * (d_model; NULL: not a model call).  The warm buffer goes through a device block of its own, rows of the handle's stride, read and
 * written in place, with the status it came with beside it. */
static int host_extras_in(MpcHandle *h, int64_t B, const CallExtras &hx, const double *d_model, hipStream_t s, CallExtras *dx) {
  const int64_t S = h->io_stride, warm_rows = mpc_warm_rows(h->params.N);
  const WarmIO &hw = hx.w;
  dx->warm = hx.warm; dx->model = d_model;
  dx->w = WarmIO{nullptr, nullptr, nullptr, S, hw.wopts, 0};
  if (!hx.warm) return MPC_OK;
  if ((hw.warm_in || hw.warm_out) && hw.ld_warm < B) { g_last_error = "ld_warm < B"; return MPC_ERR_INVALID; }
  if (hw.warm_in || hw.warm_out) MPC_TRY(ensure_dev(&h->d_warm_io, sizeof(double) * (size_t)warm_rows * (size_t)S));
  if (hw.warm_in && hw.warm_status) MPC_TRY(ensure_dev(&h->d_warm_st, sizeof(int32_t) * S));
  if (hw.warm_in) {
    MPC_HIP_CHECK(hipMemcpy2DAsync(h->d_warm_io, sizeof(double) * S, hw.warm_in, sizeof(double) * hw.ld_warm, sizeof(double) * B, warm_rows, hipMemcpyHostToDevice, s));
    dx->w.warm_in = h->d_warm_io;
    if (hw.warm_status) {
      MPC_HIP_CHECK(hipMemcpyAsync(h->d_warm_st, hw.warm_status, sizeof(int32_t) * B, hipMemcpyHostToDevice, s));
      dx->w.warm_status = h->d_warm_st;
    }
  }
  if (hw.warm_out) dx->w.warm_out = h->d_warm_io;
  if (hw.warm_out && hx.lane_rows()) {
    /* an instance writes the records of its own stages only: the rows behind them must come back as the caller has them, so
     * the caller's warm_out goes in first, into a block of its own (warm_in may be another array) */
    MPC_TRY(ensure_dev(&h->d_warm_o, sizeof(double) * (size_t)warm_rows * (size_t)S));
    MPC_HIP_CHECK(hipMemcpy2DAsync(h->d_warm_o, sizeof(double) * S, hw.warm_out, sizeof(double) * hw.ld_warm, sizeof(double) * B, warm_rows, hipMemcpyHostToDevice, s));
    dx->w.warm_out = h->d_warm_o;
  }
  return MPC_OK;
}
static int host_extras_out(MpcHandle *h, int64_t B, const CallExtras &hx, hipStream_t s) {
  if (!hx.warm || !hx.w.warm_out) return MPC_OK;
  MPC_HIP_CHECK(hipMemcpy2DAsync(hx.w.warm_out, sizeof(double) * hx.w.ld_warm, hx.lane_rows() ? h->d_warm_o : h->d_warm_io, sizeof(double) * h->io_stride, sizeof(double) * B,
                                 mpc_warm_rows(h->params.N), hipMemcpyDeviceToHost, s));
  return MPC_OK;
}

/* used by the other translation units of the library (mpc_wire.cpp): the error text of this thread */
extern "C" void mpc_internal_set_error(const char *msg) { g_last_error = msg ? msg : ""; }

/* The telemetry handler for host arrays: one copy in, the kernels, one copy out, on the handle's own device and stream
 * (whatever the caller's current device is), staging kept on the handle.  rows of `tel`, `ptsx`, `ptsy` as in
 * mpc_telemetry_batch_device with leading dimension ld; the waypoint arrays are inputs only here.  x.model (host, [MPC_NMODEL][ld]):
 * six more rows of the staging block, copied in with the other inputs; x.latency (host, comp [ld]): one more; x.horizon (host, [ld]
 * int32): copied to h->d_horizon. */
static int telemetry_host(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency, const double *ptsx,
                          const double *ptsy, double *cmd, int32_t *status, const CallExtras &x) {
  MPC_TRY(x.refused);
  MPC_TRY(check_batch(h, B, ld));
  if (npts < 3 || npts > mpc::RUN_MAX_PTS) { g_last_error = "npts must be 3..8"; return MPC_ERR_INVALID; }
  if (B == 0) { h->last_B = 0; return MPC_OK; }
  if (!tel || !ptsx || !ptsy || !cmd || !status) { g_last_error = "NULL argument"; return MPC_ERR_INVALID; }
  MPC_ON_DEVICE(h);
  const int64_t rows = 6 + 2 * npts, L = (B + 7) / 8 * 8, model_rows = x.model ? MPC_NMODEL : 0, comp_rows = x.latency ? 1 : 0;
  MPC_TRY(grow_dev(&h->d_tel, &h->tel_bytes, sizeof(double) * (size_t)((rows + 2 + model_rows + comp_rows) * L) + sizeof(int32_t) * (size_t)L));
  double *d = h->d_tel, *d_cmd = d + rows * L, *d_model = d_cmd + 2 * L, *d_comp = d_model + model_rows * L;
  int32_t *d_st = (int32_t *)(d_comp + comp_rows * L);
  hipStream_t s = h->stream;
  MPC_HIP_CHECK(hipMemcpy2DAsync(d, sizeof(double) * L, tel, sizeof(double) * ld, sizeof(double) * B, 6, hipMemcpyHostToDevice, s));
  MPC_HIP_CHECK(hipMemcpy2DAsync(d + 6 * L, sizeof(double) * L, ptsx, sizeof(double) * ld, sizeof(double) * B, npts, hipMemcpyHostToDevice, s));
  MPC_HIP_CHECK(hipMemcpy2DAsync(d + (6 + npts) * L, sizeof(double) * L, ptsy, sizeof(double) * ld, sizeof(double) * B, npts, hipMemcpyHostToDevice, s));
  if (x.model) MPC_HIP_CHECK(hipMemcpy2DAsync(d_model, sizeof(double) * L, x.model, sizeof(double) * ld, sizeof(double) * B, MPC_NMODEL, hipMemcpyHostToDevice, s));
  if (x.latency) MPC_HIP_CHECK(hipMemcpyAsync(d_comp, x.latency, sizeof(double) * B, hipMemcpyHostToDevice, s));
  CallExtras dx;
  MPC_TRY(host_extras_in(h, B, x, x.model ? d_model : nullptr, s, &dx));
  if (x.latency) dx.latency = d_comp;
  if (x.horizon) {
    MPC_TRY(ensure_dev(&h->d_horizon, sizeof(int32_t) * (size_t)h->io_stride));
    MPC_HIP_CHECK(hipMemcpyAsync(h->d_horizon, x.horizon, sizeof(int32_t) * B, hipMemcpyHostToDevice, s));
    dx.horizon = h->d_horizon;
  }
  MPC_TRY(run_impl(h, B, L, npts, d, true, extra_latency, d + 6 * L, d + (6 + npts) * L, nullptr, d_cmd, nullptr, d_st, nullptr, nullptr, (void *)s, dx));
  MPC_TRY(host_extras_out(h, B, x, s));
  MPC_HIP_CHECK(hipMemcpy2DAsync(cmd, sizeof(double) * ld, d_cmd, sizeof(double) * L, sizeof(double) * B, 2, hipMemcpyDeviceToHost, s));
  MPC_HIP_CHECK(hipMemcpyAsync(status, d_st, sizeof(int32_t) * B, hipMemcpyDeviceToHost, s));
  MPC_HIP_CHECK(hipStreamSynchronize(s));
  return MPC_OK;
}

extern "C" int mpc_telemetry_batch_host(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                                        const double *ptsx, const double *ptsy, double *cmd, int32_t *status) {
  return telemetry_host(h, B, ld, npts, tel, extra_latency, ptsx, ptsy, cmd, status, call_extras(h));
}

extern "C" int mpc_telemetry_batch_host_warm(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                                             const double *ptsx, const double *ptsy, const double *warm_in, const int32_t *warm_status,
                                             double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts, double *cmd, int32_t *status) {
  return telemetry_host(h, B, ld, npts, tel, extra_latency, ptsx, ptsy, cmd, status,
                        call_extras(h, nullptr, true, warm_in, warm_status, warm_out, ld_warm, opts));
}

extern "C" int mpc_telemetry_batch_host_model(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                                              const double *ptsx, const double *ptsy, const double *model, double *cmd, int32_t *status) {
  return telemetry_host(h, B, ld, npts, tel, extra_latency, ptsx, ptsy, cmd, status, call_extras(h, model));
}

extern "C" int mpc_telemetry_batch_host_horizon(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                                                const double *comp, const double *ptsx, const double *ptsy, const double *model, const int32_t *horizon,
                                                const double *warm_in, const int32_t *warm_status, double *warm_out, int64_t ld_warm,
                                                const MpcWarmOpts *opts, double *cmd, int32_t *status) {
  return telemetry_host(h, B, ld, npts, tel, extra_latency, ptsx, ptsy, cmd, status,
                        call_extras(h, model, true, warm_in, warm_status, warm_out, ld_warm, opts, horizon, comp));
}
extern "C" int mpc_telemetry_batch_host_latency(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                                                const double *comp, const double *ptsx, const double *ptsy, const double *model, const double *warm_in,
                                                const int32_t *warm_status, double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts,
                                                double *cmd, int32_t *status) {
  return mpc_telemetry_batch_host_horizon(h, B, ld, npts, tel, extra_latency, comp, ptsx, ptsy, model, nullptr, warm_in, warm_status, warm_out, ld_warm, opts, cmd,
                                          status);
}
extern "C" int mpc_telemetry_batch_host_warm_model(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *tel, double extra_latency,
                                                   const double *ptsx, const double *ptsy, const double *model, const double *warm_in,
                                                   const int32_t *warm_status, double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts,
                                                   double *cmd, int32_t *status) {
  return mpc_telemetry_batch_host_latency(h, B, ld, npts, tel, extra_latency, nullptr, ptsx, ptsy, model, warm_in, warm_status, warm_out, ld_warm, opts, cmd,
                                          status);
}

/* MPC::run() for host arrays (the drop-in's B = 1 case, include/mpc_drop_in.hpp): one copy in, the three kernels of
 * mpc_run_batch_device on the handle's own device and stream, one copy out; synchronises.  ptsx / ptsy are transformed in place
 * like the reference does (MPC.cpp:329; mpc_main.cpp:189-190 relies on it).  x.model: as in telemetry_host. */
static int run_host(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *pose, double *ptsx, double *ptsy, double *out8,
                    double *traj, int32_t *status, int32_t *iters, double *pre, const CallExtras &x) {
  MPC_TRY(x.refused);
  MPC_TRY(check_batch(h, B, ld));
  if (npts < 3 || npts > mpc::RUN_MAX_PTS) { g_last_error = "npts must be 3..8"; return MPC_ERR_INVALID; }
  if (h->params.precision != MPC_PRECISION_F64) { g_last_error = "run() entry points are fp64 only"; return MPC_ERR_INVALID; }
  if (B == 0) { h->last_B = 0; return MPC_OK; }
  if (!pose || !ptsx || !ptsy || !out8 || !status) { g_last_error = "NULL argument"; return MPC_ERR_INVALID; }
  MPC_ON_DEVICE(h);
  const int N = h->params.N;
  const int64_t L = (B + 7) / 8 * 8;
  const int64_t in_rows = 6 + 2 * npts, out_rows = 8 + 2 * N + mpc::RUN_PRE_ROWS, model_rows = x.model ? MPC_NMODEL : 0;
  MPC_TRY(grow_dev(&h->d_tel, &h->tel_bytes, sizeof(double) * (size_t)((in_rows + out_rows + model_rows) * L) + sizeof(int32_t) * (size_t)(2 * L)));
  double *d = h->d_tel, *d_px = d + 6 * L, *d_py = d_px + (int64_t)npts * L, *d_o8 = d + in_rows * L, *d_tr = d_o8 + 8 * L, *d_pre = d_tr + 2 * (int64_t)N * L;
  double *d_model = d_pre + mpc::RUN_PRE_ROWS * L;
  int32_t *d_st = (int32_t *)(d_model + model_rows * L), *d_it = d_st + L;
  hipStream_t s = h->stream;
  MPC_HIP_CHECK(hipMemcpy2DAsync(d, sizeof(double) * L, pose, sizeof(double) * ld, sizeof(double) * B, 6, hipMemcpyHostToDevice, s));
  MPC_HIP_CHECK(hipMemcpy2DAsync(d_px, sizeof(double) * L, ptsx, sizeof(double) * ld, sizeof(double) * B, npts, hipMemcpyHostToDevice, s));
  MPC_HIP_CHECK(hipMemcpy2DAsync(d_py, sizeof(double) * L, ptsy, sizeof(double) * ld, sizeof(double) * B, npts, hipMemcpyHostToDevice, s));
  if (x.model) MPC_HIP_CHECK(hipMemcpy2DAsync(d_model, sizeof(double) * L, x.model, sizeof(double) * ld, sizeof(double) * B, MPC_NMODEL, hipMemcpyHostToDevice, s));
  CallExtras dx;
  MPC_TRY(host_extras_in(h, B, x, x.model ? d_model : nullptr, s, &dx));
  MPC_TRY(run_impl(h, B, L, npts, d, false, 0.0, d_px, d_py, d_o8, nullptr, traj ? d_tr : nullptr, d_st, d_it, d_pre, (void *)s, dx));
  MPC_TRY(host_extras_out(h, B, x, s));
  MPC_HIP_CHECK(hipMemcpy2DAsync(ptsx, sizeof(double) * ld, d_px, sizeof(double) * L, sizeof(double) * B, npts, hipMemcpyDeviceToHost, s));
  MPC_HIP_CHECK(hipMemcpy2DAsync(ptsy, sizeof(double) * ld, d_py, sizeof(double) * L, sizeof(double) * B, npts, hipMemcpyDeviceToHost, s));
  MPC_HIP_CHECK(hipMemcpy2DAsync(out8, sizeof(double) * ld, d_o8, sizeof(double) * L, sizeof(double) * B, 8, hipMemcpyDeviceToHost, s));
  if (traj) MPC_HIP_CHECK(hipMemcpy2DAsync(traj, sizeof(double) * ld, d_tr, sizeof(double) * L, sizeof(double) * B, 2 * N, hipMemcpyDeviceToHost, s));
  if (pre) MPC_HIP_CHECK(hipMemcpy2DAsync(pre, sizeof(double) * ld, d_pre, sizeof(double) * L, sizeof(double) * B, mpc::RUN_PRE_ROWS, hipMemcpyDeviceToHost, s));
  MPC_HIP_CHECK(hipMemcpyAsync(status, d_st, sizeof(int32_t) * B, hipMemcpyDeviceToHost, s));
  if (iters) MPC_HIP_CHECK(hipMemcpyAsync(iters, d_it, sizeof(int32_t) * B, hipMemcpyDeviceToHost, s));
  MPC_HIP_CHECK(hipStreamSynchronize(s));
  return MPC_OK;
}

extern "C" int mpc_run_batch_host(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *pose, double *ptsx, double *ptsy,
                                  double *out8, double *traj, int32_t *status, int32_t *iters, double *pre) {
  return run_host(h, B, ld, npts, pose, ptsx, ptsy, out8, traj, status, iters, pre, call_extras(h));
}

extern "C" int mpc_run_batch_host_warm(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *pose, double *ptsx, double *ptsy,
                                       const double *warm_in, const int32_t *warm_status, double *warm_out, int64_t ld_warm,
                                       const MpcWarmOpts *opts, double *out8, double *traj, int32_t *status, int32_t *iters, double *pre) {
  return run_host(h, B, ld, npts, pose, ptsx, ptsy, out8, traj, status, iters, pre,
                  call_extras(h, nullptr, true, warm_in, warm_status, warm_out, ld_warm, opts));
}

extern "C" int mpc_run_batch_host_model(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *pose, double *ptsx, double *ptsy,
                                        const double *model, double *out8, double *traj, int32_t *status, int32_t *iters, double *pre) {
  return run_host(h, B, ld, npts, pose, ptsx, ptsy, out8, traj, status, iters, pre, call_extras(h, model));
}

extern "C" int mpc_run_batch_host_warm_model(MpcHandle *h, int64_t B, int64_t ld, int npts, const double *pose, double *ptsx, double *ptsy,
                                             const double *model, const double *warm_in, const int32_t *warm_status, double *warm_out,
                                             int64_t ld_warm, const MpcWarmOpts *opts, double *out8, double *traj, int32_t *status,
                                             int32_t *iters, double *pre) {
  return run_host(h, B, ld, npts, pose, ptsx, ptsy, out8, traj, status, iters, pre,
                  call_extras(h, model, true, warm_in, warm_status, warm_out, ld_warm, opts));
}

/* the device a handle lives on (mpc_create's `device`, resolved) */
extern "C" int mpc_handle_device(const MpcHandle *h) { return h ? h->device : MPC_ERR_INVALID; }

/* what the rollout entry points check before they touch anything (an empty batch may come with NULL arrays) */
static int rollout_args(const MpcHandle *h, int64_t B, int64_t ld, int steps, const double *state, const double *coeffs, const double *yaw_lo,
                        const double *yaw_hi, const int32_t *status) {
  MPC_TRY(check_batch(h, B, ld));
  if (steps < 1) { g_last_error = "steps < 1"; return MPC_ERR_INVALID; }
  if (B > 0 && (!state || !coeffs || !yaw_lo || !yaw_hi || !status)) { g_last_error = "NULL argument"; return MPC_ERR_INVALID; }
  return MPC_OK;
}

/* The rollout: `steps` solves, each followed by the step kernel.  x.warm: every step after the first is warm-started from the step
 * before (the handle keeps the buffer; of x.w only the options count).  x.model: the cars' columns go to every step, cold or warm. */
static int rollout_impl(MpcHandle *h, int64_t B, int64_t ld, int steps, double *state, const double *coeffs, const double *yaw_lo,
                        const double *yaw_hi, const double *weights, double *hist, int32_t *status, int32_t *iters, void *stream_,
                        CallExtras x) {
  MPC_TRY(x.refused);
  MPC_TRY(rollout_args(h, B, ld, steps, state, coeffs, yaw_lo, yaw_hi, status));
  if (B == 0) { h->last_B = 0; return MPC_OK; }
  MPC_ON_DEVICE(h);
  if (!hist) MPC_TRY(grow_dev(&h->d_run9, &h->run9_bytes, sizeof(double) * 9 * ld));
  MPC_TRY(ensure_dev(&h->d_rstat, sizeof(int32_t) * h->io_stride));
  if (x.warm) MPC_TRY(ensure_dev(&h->d_warm, sizeof(double) * (size_t)mpc_warm_rows(h->params.N) * (size_t)h->io_stride));
  hipStream_t s = (hipStream_t)stream_;
  const unsigned grid = (unsigned)((B + 255) / 256);
  for (int t = 0; t < steps; t++) {
    double *o9 = hist ? hist + (int64_t)t * 9 * ld : h->d_run9;
    /* (warm, in place: a lane reads its car's column and its previous status (d_rstat) before it writes either) */
    x.w = WarmIO{t == 0 ? nullptr : h->d_warm, h->d_rstat, h->d_warm, h->io_stride, x.w.wopts, 0};
    MPC_TRY(launch_solve<double>(h, {B, ld, ld, state, coeffs, yaw_lo, yaw_hi, weights, o9, nullptr, h->d_rstat, h->d_iters}, stream_, 0, x));
    hipLaunchKernelGGL(mpc_rollout_step_kernel, dim3(grid), dim3(256), 0, s, B, ld, t == 0, o9, state, h->d_rstat, h->d_iters, status, iters);
    MPC_HIP_CHECK(hipGetLastError());
  }
  return record_stats(h, B, status, iters, s);   /* worst status per instance, iterations summed over the steps */
}

extern "C" int mpc_rollout_batch_device(MpcHandle *h, int64_t B, int64_t ld, int steps, double *state, const double *coeffs,
                                        const double *yaw_lo, const double *yaw_hi, const double *weights, double *hist,
                                        int32_t *status, int32_t *iters, void *stream_) {
  return rollout_impl(h, B, ld, steps, state, coeffs, yaw_lo, yaw_hi, weights, hist, status, iters, stream_, call_extras(h));
}

extern "C" int mpc_rollout_batch_device_model(MpcHandle *h, int64_t B, int64_t ld, int steps, double *state, const double *coeffs,
                                              const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                              double *hist, int32_t *status, int32_t *iters, void *stream_) {
  return rollout_impl(h, B, ld, steps, state, coeffs, yaw_lo, yaw_hi, weights, hist, status, iters, stream_, call_extras(h, model));
}

extern "C" int mpc_rollout_batch_device_warm(MpcHandle *h, int64_t B, int64_t ld, int steps, double *state, const double *coeffs,
                                             const double *yaw_lo, const double *yaw_hi, const double *weights, const MpcWarmOpts *opts,
                                             double *hist, int32_t *status, int32_t *iters, void *stream_) {
  return rollout_impl(h, B, ld, steps, state, coeffs, yaw_lo, yaw_hi, weights, hist, status, iters, stream_,
                      call_extras(h, nullptr, true, nullptr, nullptr, nullptr, 0, opts));
}

extern "C" int mpc_rollout_batch_device_warm_model(MpcHandle *h, int64_t B, int64_t ld, int steps, double *state, const double *coeffs,
                                                   const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                                   const MpcWarmOpts *opts, double *hist, int32_t *status, int32_t *iters, void *stream_) {
  return rollout_impl(h, B, ld, steps, state, coeffs, yaw_lo, yaw_hi, weights, hist, status, iters, stream_,
                      call_extras(h, model, true, nullptr, nullptr, nullptr, 0, opts));
}

extern "C" int mpc_rollout_batch_device_horizon(MpcHandle *h, int64_t B, int64_t ld, int steps, double *state, const double *coeffs,
                                                const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                                const int32_t *horizon, double *hist, int32_t *status, int32_t *iters, void *stream_) {
  return rollout_impl(h, B, ld, steps, state, coeffs, yaw_lo, yaw_hi, weights, hist, status, iters, stream_,
                      call_extras(h, model, false, nullptr, nullptr, nullptr, 0, nullptr, horizon));
}

extern "C" int mpc_rollout_batch_device_warm_horizon(MpcHandle *h, int64_t B, int64_t ld, int steps, double *state, const double *coeffs,
                                                     const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                                     const int32_t *horizon, const MpcWarmOpts *opts, double *hist, int32_t *status,
                                                     int32_t *iters, void *stream_) {
  return rollout_impl(h, B, ld, steps, state, coeffs, yaw_lo, yaw_hi, weights, hist, status, iters, stream_,
                      call_extras(h, model, true, nullptr, nullptr, nullptr, 0, opts, horizon));
}

/* The rollout in one launch: the ROLL build of the lane kernel, a lane per car for all `steps` solves (see mpc_solve_kernel).  One
 * rule decides: fused == stepwise on every handle.  The fused kernel is the single-phase fp64 lane kernel, so it runs where the
 * stepwise loop would launch exactly that at every step (an fp64 handle, no fp32 start, no SOC, B above the wave limit); everywhere
 * else -- and for an fp32 handle, which the loop refuses -- the call IS the stepwise loop.  x.warm: warm_start != 0.
 * x.model (an fp64 handle): the stepwise model loop launches the single-phase fp64 lane kernel at every B
 * and on a handle whose ordinary solve starts in fp32 as well, so the one launch -- the ROLL+MODEL builds -- runs at every B >= 1 of
 * every handle without SOC; with SOC (a cold call; a warm one has been refused) the call is the stepwise model loop. */
static int rollout_fused_impl(MpcHandle *h, int64_t B, int64_t ld, int steps, double *state, const double *coeffs, const double *yaw_lo,
                              const double *yaw_hi, const double *weights, double *hist, int32_t *status, int32_t *iters, void *stream_,
                              const CallExtras &x) {
  MPC_TRY(x.refused);
  MPC_TRY(rollout_args(h, B, ld, steps, state, coeffs, yaw_lo, yaw_hi, status));
  const double *model = x.model;
  const bool as_model = x.model_call();          /* (a horizon call is dispatched as a model call) */
  const bool wave_path = !as_model && h->wave_max_batch > 0 && B <= h->wave_max_batch;
  if (B == 0 || h->params.precision != MPC_PRECISION_F64 || (h->mixed && !as_model) || h->params.max_soc > 0 || wave_path) {
    MPC_TRY(rollout_impl(h, B, ld, steps, state, coeffs, yaw_lo, yaw_hi, weights, hist, status, iters, stream_, x));
    ++h->n_roll_stepwise;
    return MPC_OK;
  }
  MPC_ON_DEVICE(h);
  if (!hist) MPC_TRY(grow_dev(&h->d_run9, &h->run9_bytes, sizeof(double) * 9 * ld));
  if (x.warm) MPC_TRY(ensure_dev(&h->d_warm, sizeof(double) * (size_t)mpc_warm_rows(h->params.N) * (size_t)h->io_stride));
  double *o9 = hist ? hist : h->d_run9;          /* (no history: every car's 9 rows go to its own column of the scratch rows) */
  const SolveIO<double> io{B, ld, ld, state, coeffs, yaw_lo, yaw_hi, weights, o9, nullptr, status, iters ? iters : h->d_iters};
  std::optional<DeviceGuard> guard;
  MpcHandle::BatchRec *rec = nullptr;
  MPC_TRY(solve_begin(h, io, nullptr, guard, &rec));
  hipStream_t s = (hipStream_t)stream_;
  const CounterBlocks C = take_counters(h);
  MPC_HIP_CHECK(hipEventRecord(h->ev0, s));
  MpcPhase T = phase_defaults(h, B);
  T.take = C.cb; T.n_out = C.cb + 1; T.zero_next = C.zero_next;
  T.compact_gap = 0;                             /* (the step index does not travel with a moved instance) */
  const TailPlace tp;
  tail_fields(h, tp, T);
  double *warm = x.warm ? h->d_warm : nullptr;
  const WarmIO wc{warm, nullptr, warm, h->io_stride, x.w.wopts, 0};
  const MpcRollPart roll{steps, o9, hist ? 9 * ld : 0, state, status, iters};
  const unsigned grid = (unsigned)((B + kBlock - 1) / kBlock);
  MPC_TRY(with_bool(h->staging, [&](auto staging) {
    /* (no SOC here: those handles loop; the ROLL+HORIZON builds: not staged, no LDS -- no lane compaction here) */
    return with_build(false, x.warm, model != nullptr, x.horizon != nullptr, [&](auto, auto warm_build, auto model_build, auto horizon_build) {
      constexpr bool HORIZON = decltype(horizon_build)::value, STAGING = decltype(staging)::value && !HORIZON;
      constexpr bool WARM = decltype(warm_build)::value, MODEL = decltype(model_build)::value;
      return launch_kernel(mpc_solve_kernel<STAGING, double, double, double, false, WARM, true, MODEL, HORIZON>, grid, STAGING ? staging_lds_bytes<double>() : 0,
                           s, h, io, (double *)h->ws, h->ws_stride, phase_of<true, WARM, MODEL, HORIZON>(T, wc, roll, {model, ld}, {x.horizon}));
    });
  }));
  MPC_TRY(solve_end(h, io, s, rec, tp, false));
  ++h->n_roll_fused;
  return record_stats(h, B, status, iters, s);   /* as the stepwise loop: worst status per instance, iterations summed over the steps */
}

extern "C" int mpc_rollout_batch_device_fused(MpcHandle *h, int64_t B, int64_t ld, int steps, double *state, const double *coeffs,
                                              const double *yaw_lo, const double *yaw_hi, const double *weights, int warm_start,
                                              const MpcWarmOpts *opts, double *hist, int32_t *status, int32_t *iters, void *stream_) {
  return rollout_fused_impl(h, B, ld, steps, state, coeffs, yaw_lo, yaw_hi, weights, hist, status, iters, stream_,
                            call_extras(h, nullptr, warm_start != 0, nullptr, nullptr, nullptr, 0, opts));
}

extern "C" int mpc_rollout_batch_device_fused_model(MpcHandle *h, int64_t B, int64_t ld, int steps, double *state, const double *coeffs,
                                                    const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                                    int warm_start, const MpcWarmOpts *opts, double *hist, int32_t *status, int32_t *iters,
                                                    void *stream_) {
  return rollout_fused_impl(h, B, ld, steps, state, coeffs, yaw_lo, yaw_hi, weights, hist, status, iters, stream_,
                            call_extras(h, model, warm_start != 0, nullptr, nullptr, nullptr, 0, opts));
}

extern "C" int mpc_rollout_batch_device_fused_horizon(MpcHandle *h, int64_t B, int64_t ld, int steps, double *state, const double *coeffs,
                                                      const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                                      const int32_t *horizon, int warm_start, const MpcWarmOpts *opts, double *hist,
                                                      int32_t *status, int32_t *iters, void *stream_) {
  return rollout_fused_impl(h, B, ld, steps, state, coeffs, yaw_lo, yaw_hi, weights, hist, status, iters, stream_,
                            call_extras(h, model, warm_start != 0, nullptr, nullptr, nullptr, 0, opts, horizon));
}

extern "C" int mpc_rollout_fused_info(const MpcHandle *h, int64_t *out2) {
  if (!h || !out2) { g_last_error = "NULL argument"; return MPC_ERR_INVALID; }
  out2[0] = h->n_roll_fused; out2[1] = h->n_roll_stepwise;
  return MPC_OK;
}

/* ---- track driving (include/mpc_amd_drive.h) -------------------------------------------------------------------------------------- */
extern "C" int mpc_drive_opts_default(const MpcParams *p, MpcDriveOpts *o) {
  if (!p || !o) { g_last_error = "NULL argument"; return MPC_ERR_INVALID; }
  memset(o, 0, sizeof(*o));
  o->size = (int32_t)sizeof(MpcDriveOpts); o->npts = 6; o->h = 0.01;
  o->sub_old = (p->latency_ms + 5) / 10;             /* the command in force lasts for the latency, in substeps of 10 ms */
  o->sub_new = p->latency_ms != 0 ? 2 : 10;
  o->warm_start = 0; o->extra_latency = 0.0; o->cte_limit = 3.0;
  return MPC_OK;
}

/* the plant column under which the _plant forms move a car as the forms without do (the car's own Lf belongs in row 0) */
extern "C" int mpc_drive_plant_default(const MpcParams *p, double *col6) {
  if (!p || !col6) { g_last_error = "NULL argument"; return MPC_ERR_INVALID; }
  col6[MPC_PLANT_LF] = p->Lf; col6[MPC_PLANT_STEER_GAIN] = 1.0; col6[MPC_PLANT_STEER_BIAS] = 0.0;
  col6[MPC_PLANT_ACCEL_GAIN] = 6.0; col6[MPC_PLANT_DRAG_SPEED] = 50.0; col6[MPC_PLANT_DRIFT] = 0.0;
  return MPC_OK;
}

/* what the drive entry points check before they touch anything; *O: the options in effect (opts = NULL: the defaults) */
static int drive_args(const MpcHandle *h, int64_t B, int64_t ld, int steps, const double *car, const double *track_x, const double *track_y,
                      int n_track, const MpcDriveOpts *opts, const double *summary, const int32_t *status, MpcDriveOpts *O) {
  const auto refuse = [](const char *why) { g_last_error = why; return MPC_ERR_INVALID; };
  if (!h) return refuse("NULL handle");
  if (opts) {
    if (opts->size != (int32_t)sizeof(MpcDriveOpts)) return refuse("MpcDriveOpts.size mismatch (fill it with mpc_drive_opts_default)");
    *O = *opts;
  } else (void)mpc_drive_opts_default(&h->params, O);
  if (h->params.precision != MPC_PRECISION_F64) return refuse("track driving: fp64 handles only (this one was created with MPC_PRECISION_F32)");
  if (steps < 1) return refuse("steps < 1");
  if (O->npts < 3 || O->npts > mpc::RUN_MAX_PTS) return refuse("MpcDriveOpts.npts must be 3..8");
  if (n_track < O->npts || n_track > MPC_DRIVE_MAX_TRACK) return refuse("n_track must be npts..MPC_DRIVE_MAX_TRACK");
  if (O->sub_old < 0 || O->sub_new < 0) return refuse("MpcDriveOpts: a substep count below 0");
  if ((int64_t)O->sub_old + O->sub_new < 1 || (int64_t)O->sub_old + O->sub_new > 1000) return refuse("MpcDriveOpts: sub_old + sub_new must be 1..1000");
  if (!(O->h > 0.0) || !mpc::drive_finite(O->h)) return refuse("MpcDriveOpts.h must be finite and > 0");
  if (B < 0 || ld < B) return refuse("ld < B");
  if (B > h->max_batch) return refuse("B exceeds the handle's max_batch");
  if (!car || !track_x || !track_y || !summary || !status) return refuse("NULL argument");
  return MPC_OK;
}

/* the handle's rows both forms work in: the window rows and the reply, the stepwise loop's two index rows and its comp row, the six rows of what the handler is told in a
 * noise call (DriveRows), the warm buffer of a warm call, and the caller's weights copied to the handle's stride (*w_out; NULL without weights) */
static int drive_rows(MpcHandle *h, int64_t B, int64_t ld, bool warm, const double *weights, hipStream_t s, const double **w_out) {
  const int64_t S = h->io_stride;
  MPC_TRY(grow_dev(&h->d_drive, &h->drive_bytes, DriveRows::bytes(ld)));
  if (warm) MPC_TRY(ensure_dev(&h->d_warm, sizeof(double) * (size_t)mpc_warm_rows(h->params.N) * (size_t)S));
  *w_out = nullptr;
  if (weights) {
    MPC_TRY(ensure_dev(&h->d_drive_w, sizeof(double) * MPC_NW * S));
    MPC_HIP_CHECK(hipMemcpy2DAsync(h->d_drive_w, sizeof(double) * S, weights, sizeof(double) * ld, sizeof(double) * B, MPC_NW, hipMemcpyDeviceToDevice, s));
    *w_out = h->d_drive_w;
  }
  return MPC_OK;
}

/* The stepwise loop: `steps` x (sense kernel, the telemetry handler -- run_impl with tel, the weights and an iterations pointer --,
 * plant-and-summary kernel) on the caller's stream; no host synchronisation.  x.warm: every step after the first is the _warm handler
 * on the handle's own buffer, in place (rollout_impl's arrangement).  x.model (device, [MPC_NMODEL][ld]): the handler is the
 * telemetry _model call -- run_impl reads the columns where the caller has them.
 * x.latency (device, [MPC_NLATENCY][ld]): one more kernel first, the comp row the handler takes (not-a-number for a column that cannot
 * be used); the handler is the telemetry _latency call on it, with or without model.
 * x.plant (device, [MPC_NPLANT][ld]): the handler's calls are what they are without it.
 * x.noise (device, [MPC_NNOISE][ld]) or x.seen (device, [steps][4][ld]): the sense kernel also writes what the handler is told into the
 * handle's seen rows, and the handler is pointed at those instead of the car -- the same handler, on the same dispatch.
 * The plant kernel is one, and takes the caller's latency, model and plant as they came, each an array or nullptr. */
static int drive_impl(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y, int n_track,
                      const double *weights, const MpcDriveOpts &O, CallExtras x, double *summary, double *hist, int32_t *status,
                      int32_t *iters, void *stream_) {
  MPC_ON_DEVICE(h);
  const int64_t S = h->io_stride;
  hipStream_t s = (hipStream_t)stream_;
  MPC_TRY(drive_rows(h, B, ld, x.warm, weights, s, &x.run_weights));
  MPC_TRY(ensure_dev(&h->d_rstat, sizeof(int32_t) * S));
  const DriveRows R{h->d_drive, ld};
  double *ptsx = R.ptsx(), *ptsy = R.ptsy(), *cmd = R.cmd();
  double *seen6 = x.senses() ? R.seen6() : nullptr;
  const unsigned grid = (unsigned)((B + 255) / 256);
  const double *latency = x.latency;
  if (latency) {
    double *comp = R.comp();
    hipLaunchKernelGGL(mpc_drive_comp_kernel, dim3(grid), dim3(256), 0, s, O, B, ld, latency, comp);
    MPC_HIP_CHECK(hipGetLastError());
    x.latency = comp;                              /* what run_impl takes: the handler's comp [ld] */
  }
  for (int t = 0; t < steps; t++) {
    /* (the first step has no step before it: it is handed its own row, and mpc::drive_step_instance does not look at the value) */
    int32_t *k_now = R.idx(t & 1), *k_prev = t == 0 ? k_now : R.idx((t & 1) ^ 1);
    hipLaunchKernelGGL(mpc_drive_sense_kernel, dim3(grid), dim3(256), 0, s, B, ld, (int)O.npts, car, track_x, track_y, n_track, ptsx, ptsy, k_now, x.noise, t, seen6,
                       x.seen ? x.seen + (int64_t)t * 4 * ld : nullptr);
    MPC_HIP_CHECK(hipGetLastError());
    x.w = WarmIO{t == 0 ? nullptr : h->d_warm, h->d_rstat, h->d_warm, S, x.w.wopts, 0};
    MPC_TRY(run_impl(h, B, ld, O.npts, seen6 ? seen6 : car, true, O.extra_latency, ptsx, ptsy, nullptr, cmd, nullptr, h->d_rstat, h->d_iters, nullptr, stream_, x));
    double *rec = hist ? hist + (int64_t)t * MPC_DRIVE_REC * ld : nullptr;
    hipLaunchKernelGGL(mpc_drive_plant_kernel, dim3(grid), dim3(256), 0, s, h->params, O, B, ld, t, n_track, car, cmd, h->d_run, S, h->d_rstat, h->d_iters,
                       k_now, k_prev, summary, rec, status, iters, latency, MpcModelPart{x.model, ld}, x.plant, x.noise);
    MPC_HIP_CHECK(hipGetLastError());
  }
  ++h->n_drive_stepwise;
  return record_stats(h, B, status, iters, s);   /* as the rollouts: worst status per car, iterations summed over the steps */
}

/* What every drive entry point does first: with `model`, the model rule (which handles a model call is accepted on, call_extras);
 * drive_args; then the call's extras -- the warm refusals and the options in effect. */
static int drive_call(const MpcHandle *h, int64_t B, int64_t ld, int steps, const double *car, const double *track_x, const double *track_y,
                      int n_track, const double *model, const int32_t *horizon, const int32_t *budget, const double *latency, const double *plant,
                      const double *noise, double *seen, const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, const double *summary, const int32_t *status,
                      MpcDriveOpts *O, CallExtras *x) {
  if (h && (plant || noise || seen) && h->params.precision != MPC_PRECISION_F64) {
    g_last_error = "track driving: fp64 handles only (this one was created with MPC_PRECISION_F32)";
    return MPC_ERR_INVALID;
  }
  if (h && (model || horizon || budget)) MPC_TRY(call_extras(h, model, false, nullptr, nullptr, nullptr, 0, nullptr, horizon, nullptr, budget).refused);
  MPC_TRY(drive_args(h, B, ld, steps, car, track_x, track_y, n_track, opts, summary, status, O));
  *x = call_extras(h, model, O->warm_start != 0, nullptr, nullptr, nullptr, 0, warm_opts, horizon, latency, budget);
  x->plant = plant;
  x->noise = noise;
  x->seen = seen;
  return x->refused;
}

/* (the _plant forms, "per-car plant values" in include/mpc_amd_drive.h: the _horizon forms plus `plant` behind latency; NULL is the _horizon form itself) */
/* (the _budget forms, include/mpc_amd_budget.h: the _plant forms plus `budget` behind horizon; NULL is the _plant form itself) */
/* (the _noise forms, include/mpc_amd_noise.h: the _budget forms plus `noise` behind plant and `seen` behind hist; both NULL is the _budget form itself) */
extern "C" int mpc_drive_batch_device_noise(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x,
                                            const double *track_y, int n_track, const double *weights, const double *model, const int32_t *horizon,
                                            const int32_t *budget, const double *latency, const double *plant, const double *noise, const MpcDriveOpts *opts,
                                            const MpcWarmOpts *warm_opts, double *summary, double *hist, double *seen, int32_t *status, int32_t *iters,
                                            void *stream_) {
  MpcDriveOpts O;
  CallExtras x;
  MPC_TRY(drive_call(h, B, ld, steps, car, track_x, track_y, n_track, model, horizon, budget, latency, plant, noise, seen, opts, warm_opts, summary, status, &O, &x));
  if (B == 0) { h->last_B = 0; return MPC_OK; }
  return drive_impl(h, B, ld, steps, car, track_x, track_y, n_track, weights, O, x, summary, hist, status, iters, stream_);
}
extern "C" int mpc_drive_batch_device_budget(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x,
                                             const double *track_y, int n_track, const double *weights, const double *model, const int32_t *horizon,
                                             const int32_t *budget, const double *latency, const double *plant, const MpcDriveOpts *opts,
                                             const MpcWarmOpts *warm_opts, double *summary, double *hist, int32_t *status, int32_t *iters, void *stream_) {
  return mpc_drive_batch_device_noise(h, B, ld, steps, car, track_x, track_y, n_track, weights, model, horizon, budget, latency, plant, nullptr, opts, warm_opts,
                                      summary, hist, nullptr, status, iters, stream_);
}
extern "C" int mpc_drive_batch_device_plant(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x,
                                            const double *track_y, int n_track, const double *weights, const double *model, const int32_t *horizon,
                                            const double *latency, const double *plant, const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts,
                                            double *summary, double *hist, int32_t *status, int32_t *iters, void *stream_) {
  return mpc_drive_batch_device_budget(h, B, ld, steps, car, track_x, track_y, n_track, weights, model, horizon, nullptr, latency, plant, opts, warm_opts, summary,
                                       hist, status, iters, stream_);
}
/* (the _horizon forms, "per-car horizon" in include/mpc_amd_drive.h: the _latency forms plus `horizon` behind model; NULL is the _latency form itself) */
extern "C" int mpc_drive_batch_device_horizon(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x,
                                              const double *track_y, int n_track, const double *weights, const double *model, const int32_t *horizon,
                                              const double *latency, const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary,
                                              double *hist, int32_t *status, int32_t *iters, void *stream_) {
  return mpc_drive_batch_device_plant(h, B, ld, steps, car, track_x, track_y, n_track, weights, model, horizon, latency, nullptr, opts, warm_opts, summary, hist,
                                      status, iters, stream_);
}
extern "C" int mpc_drive_batch_device_latency(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x,
                                              const double *track_y, int n_track, const double *weights, const double *model, const double *latency,
                                              const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary, double *hist,
                                            int32_t *status, int32_t *iters, void *stream_) {
  return mpc_drive_batch_device_horizon(h, B, ld, steps, car, track_x, track_y, n_track, weights, model, nullptr, latency, opts, warm_opts, summary, hist, status,
                                        iters, stream_);
}
extern "C" int mpc_drive_batch_device_model(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x,
                                            const double *track_y, int n_track, const double *weights, const double *model,
                                            const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary, double *hist,
                                            int32_t *status, int32_t *iters, void *stream_) {
  return mpc_drive_batch_device_latency(h, B, ld, steps, car, track_x, track_y, n_track, weights, model, nullptr, opts, warm_opts, summary, hist, status, iters,
                                        stream_);
}
extern "C" int mpc_drive_batch_device(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                                      int n_track, const double *weights, const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts,
                                      double *summary, double *hist, int32_t *status, int32_t *iters, void *stream_) {
  return mpc_drive_batch_device_model(h, B, ld, steps, car, track_x, track_y, n_track, weights, nullptr, opts, warm_opts, summary, hist, status, iters,
                                      stream_);
}

/* The loop in one launch: the DRIVE build of the lane kernel (see mpc_solve_kernel and MpcDrivePart), a lane per car for all `steps`
 * messages.  rollout_fused_impl's rule decides: the one launch runs where the stepwise loop would launch exactly the single-phase fp64
 * lane kernel at every step (no fp32 start, no SOC, B above the wave limit); everywhere else the call IS the stepwise loop.
 * x.model: the DRIVE x MODEL builds, where the stepwise model loop launches the lane kernel's MODEL build at every step -- the same
 * rule, but on a handle whose ordinary solve starts in fp32 as well: a model solve is the single-phase fp64 launch on h->ws there.
 * x.horizon: the DRIVE x MODEL x HORIZON builds (cold, WARM), where the stepwise horizon loop launches the lane kernel's HORIZON build
 * at every step: every B >= 1 of every fp64 handle without SOC. */
static int drive_fused_impl(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y, int n_track,
                            const double *weights, const MpcDriveOpts &O, const CallExtras &x, double *summary, double *hist, int32_t *status,
                            int32_t *iters, void *stream_) {
  /* (a horizon call never takes the wave path or the fp32 start: the one launch at every B >= 1, the rule of rollout_fused_impl) */
  const bool wave_path = !x.lane_rows() && h->wave_max_batch > 0 && B <= h->wave_max_batch;      /* (a budget call: the horizon call's rule) */
  const double *model = x.model;
  if ((h->mixed && !x.model_call()) || h->params.max_soc > 0 || wave_path)
    return drive_impl(h, B, ld, steps, car, track_x, track_y, n_track, weights, O, x, summary, hist, status, iters, stream_);
  MPC_TRY(check_batch(h, B, ld));
  if (h->params.n_yaw_change_speeds < 1 || h->params.n_steer_speeds < 1) { g_last_error = "run(): empty speed tables (load a config-*.json)"; return MPC_ERR_INVALID; }
  if (h->params.max_fit_order > 5) { g_last_error = "run(): max_fit_order > 5 is not built (fit orders 2..4)"; return MPC_ERR_UNSUPPORTED; }
  MPC_ON_DEVICE(h);
  const int64_t S = h->io_stride;
  hipStream_t s = (hipStream_t)stream_;
  const double *w_dev = nullptr;
  MPC_TRY(drive_rows(h, B, ld, x.warm, weights, s, &w_dev));
  MPC_TRY(ensure_dev(&h->d_run, sizeof(double) * mpc::RUN_PRE_ROWS * S));
  MPC_TRY(grow_dev(&h->d_run9, &h->run9_bytes, sizeof(double) * 9 * ld));
  const DriveRows R{h->d_drive, ld};
  double *d_pre = h->d_run, *ptsx = R.ptsx(), *ptsy = R.ptsy(), *cmd = R.cmd();
  const SolveIO<double> io{B, S, ld, d_pre + mpc::RUN_PRE_STATE * S, d_pre + mpc::RUN_PRE_COEFFS * S, d_pre + mpc::RUN_PRE_YAW_LO * S,
                           d_pre + mpc::RUN_PRE_YAW_HI * S, w_dev, h->d_run9, nullptr, status, iters ? iters : h->d_iters};
  std::optional<DeviceGuard> guard;
  MpcHandle::BatchRec *rec = nullptr;
  MPC_TRY(solve_begin(h, io, nullptr, guard, &rec));
  const CounterBlocks C = take_counters(h);
  MPC_HIP_CHECK(hipEventRecord(h->ev0, s));
  MpcPhase T = phase_defaults(h, B);
  T.take = C.cb; T.n_out = C.cb + 1; T.zero_next = C.zero_next;
  T.compact_gap = 0;                             /* (the step index does not travel with a moved instance) */
  const TailPlace tp;
  tail_fields(h, tp, T);
  double *warm = x.warm ? h->d_warm : nullptr;
  const WarmIO wc{warm, nullptr, warm, S, x.w.wopts, 1};      /* (psi_box: the run() path's rule) */
  const MpcRollPart roll{steps, nullptr, 0, nullptr, status, iters};
  const MpcDrivePart drive{O, car, track_x, track_y, n_track, ptsx, ptsy, cmd, d_pre, h->d_run9, summary, hist, x.latency, x.plant, x.noise, x.seen};
  const unsigned grid = (unsigned)((B + kBlock - 1) / kBlock);
  if (x.lane_rows()) {
    /* the DRIVE x HORIZON builds: MODEL builds whose `model` may be nullptr, not staged, per-lane workspace rows, no LDS (no lane compaction here) */
    MPC_TRY(with_bool(x.warm, [&](auto warm_build) {
      constexpr bool WARM = decltype(warm_build)::value;
      return launch_kernel(mpc_solve_kernel<false, double, double, double, false, WARM, true, true, true, true>, grid, 0, s, h, io, (double *)h->ws, h->ws_stride,
                           phase_of<true, WARM, true, true, true>(T, wc, roll, {model, ld}, {x.horizon, x.budget}, drive));
    }));
  } else
  MPC_TRY(with_bool(h->staging, [&](auto staging) {
    return with_bool(x.warm, [&](auto warm_build) {
      return with_bool(model != nullptr, [&](auto model_build) {
        constexpr bool STAGING = decltype(staging)::value, WARM = decltype(warm_build)::value, MODEL = decltype(model_build)::value;
        return launch_kernel(mpc_solve_kernel<STAGING, double, double, double, false, WARM, true, MODEL, false, true>, grid, STAGING ? staging_lds_bytes<double>() : 0,
                             s, h, io, (double *)h->ws, h->ws_stride, phase_of<true, WARM, MODEL, false, true>(T, wc, roll, {model, ld}, {}, drive));
      });
    });
  }));
  MPC_TRY(solve_end(h, io, s, rec, tp, false));
  ++h->n_drive_fused;
  return record_stats(h, B, status, iters, s);
}

extern "C" int mpc_drive_batch_device_fused_noise(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x,
                                                  const double *track_y, int n_track, const double *weights, const double *model,
                                                  const int32_t *horizon, const int32_t *budget, const double *latency, const double *plant,
                                                  const double *noise, const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary, double *hist,
                                                  double *seen, int32_t *status, int32_t *iters, void *stream_) {
  MpcDriveOpts O;
  CallExtras x;
  MPC_TRY(drive_call(h, B, ld, steps, car, track_x, track_y, n_track, model, horizon, budget, latency, plant, noise, seen, opts, warm_opts, summary, status, &O, &x));
  if (B == 0) { h->last_B = 0; return MPC_OK; }
  return drive_fused_impl(h, B, ld, steps, car, track_x, track_y, n_track, weights, O, x, summary, hist, status, iters, stream_);
}
extern "C" int mpc_drive_batch_device_fused_budget(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x,
                                                   const double *track_y, int n_track, const double *weights, const double *model,
                                                   const int32_t *horizon, const int32_t *budget, const double *latency, const double *plant,
                                                   const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary, double *hist, int32_t *status,
                                                   int32_t *iters, void *stream_) {
  return mpc_drive_batch_device_fused_noise(h, B, ld, steps, car, track_x, track_y, n_track, weights, model, horizon, budget, latency, plant, nullptr, opts,
                                            warm_opts, summary, hist, nullptr, status, iters, stream_);
}
extern "C" int mpc_drive_batch_device_fused_plant(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x,
                                                  const double *track_y, int n_track, const double *weights, const double *model,
                                                  const int32_t *horizon, const double *latency, const double *plant, const MpcDriveOpts *opts,
                                                  const MpcWarmOpts *warm_opts, double *summary, double *hist, int32_t *status, int32_t *iters,
                                                  void *stream_) {
  return mpc_drive_batch_device_fused_budget(h, B, ld, steps, car, track_x, track_y, n_track, weights, model, horizon, nullptr, latency, plant, opts, warm_opts,
                                             summary, hist, status, iters, stream_);
}
extern "C" int mpc_drive_batch_device_fused_horizon(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x,
                                                    const double *track_y, int n_track, const double *weights, const double *model,
                                                    const int32_t *horizon, const double *latency, const MpcDriveOpts *opts,
                                                    const MpcWarmOpts *warm_opts, double *summary, double *hist, int32_t *status, int32_t *iters,
                                                    void *stream_) {
  return mpc_drive_batch_device_fused_plant(h, B, ld, steps, car, track_x, track_y, n_track, weights, model, horizon, latency, nullptr, opts, warm_opts, summary,
                                            hist, status, iters, stream_);
}
extern "C" int mpc_drive_batch_device_fused_latency(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x,
                                                    const double *track_y, int n_track, const double *weights, const double *model,
                                                    const double *latency, const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary, double *hist,
                                                  int32_t *status, int32_t *iters, void *stream_) {
  return mpc_drive_batch_device_fused_horizon(h, B, ld, steps, car, track_x, track_y, n_track, weights, model, nullptr, latency, opts, warm_opts, summary, hist,
                                              status, iters, stream_);
}
extern "C" int mpc_drive_batch_device_fused_model(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x,
                                                  const double *track_y, int n_track, const double *weights, const double *model,
                                                  const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary, double *hist,
                                                  int32_t *status, int32_t *iters, void *stream_) {
  return mpc_drive_batch_device_fused_latency(h, B, ld, steps, car, track_x, track_y, n_track, weights, model, nullptr, opts, warm_opts, summary, hist, status,
                                              iters, stream_);
}
extern "C" int mpc_drive_batch_device_fused(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                                            int n_track, const double *weights, const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts,
                                            double *summary, double *hist, int32_t *status, int32_t *iters, void *stream_) {
  return mpc_drive_batch_device_fused_model(h, B, ld, steps, car, track_x, track_y, n_track, weights, nullptr, opts, warm_opts, summary, hist, status,
                                            iters, stream_);
}

/* The same for host arrays: one copy in, the loop on the handle's own device and stream, one copy out; synchronises.  Staging kept on
 * the handle and grown on demand, like the telemetry handler's.  model (host, [MPC_NMODEL][ld]), latency (host, [MPC_NLATENCY][ld]) and
 * horizon (host, [ld] int32, to h->d_horizon) are copied in with the other inputs, and so are plant (host, [MPC_NPLANT][ld]) and noise
 * (host, [MPC_NNOISE][ld]); seen (host, [steps][4][ld]) is copied out with hist. */
extern "C" int mpc_drive_batch_host_noise(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                                          int n_track, const double *weights, const double *model, const int32_t *horizon, const int32_t *budget,
                                          const double *latency, const double *plant, const double *noise, const MpcDriveOpts *opts,
                                          const MpcWarmOpts *warm_opts, double *summary, double *hist, double *seen, int32_t *status, int32_t *iters) {
  MpcDriveOpts O;
  CallExtras x;
  MPC_TRY(drive_call(h, B, ld, steps, car, track_x, track_y, n_track, model, horizon, budget, latency, plant, noise, seen, opts, warm_opts, summary, status, &O, &x));
  if (B == 0) { h->last_B = 0; return MPC_OK; }
  MPC_ON_DEVICE(h);
  const int64_t L = (B + 7) / 8 * 8;
  const int64_t rows = 6 + MPC_DRIVE_NSUM + (weights ? MPC_NW : 0) + (hist ? (int64_t)steps * MPC_DRIVE_REC : 0) + (model ? MPC_NMODEL : 0) +
                       (latency ? MPC_NLATENCY : 0) + (plant ? MPC_NPLANT : 0) + (noise ? MPC_NNOISE : 0) + (seen ? (int64_t)steps * 4 : 0);
  MPC_TRY(grow_dev(&h->d_drive_host, &h->drive_host_bytes, sizeof(double) * (size_t)(rows * L + 2 * n_track) + sizeof(int32_t) * (size_t)(2 * L)));
  double *d = h->d_drive_host;
  double *d_car = d, *d_sum = d_car + 6 * L, *d_w = d_sum + MPC_DRIVE_NSUM * L, *d_hist = d_w + (weights ? MPC_NW * L : 0);
  double *d_model = d_hist + (hist ? (int64_t)steps * MPC_DRIVE_REC * L : 0), *d_lat = d_model + (model ? MPC_NMODEL * L : 0), *d_plant = d_lat + (latency ? MPC_NLATENCY * L : 0),
         *d_noise = d_plant + (plant ? MPC_NPLANT * L : 0), *d_seen = d_noise + (noise ? MPC_NNOISE * L : 0),
         *d_tx = d_seen + (seen ? (int64_t)steps * 4 * L : 0), *d_ty = d_tx + n_track;
  int32_t *d_st = (int32_t *)(d_ty + n_track), *d_it = d_st + L;
  hipStream_t s = h->stream;
  MPC_HIP_CHECK(hipMemcpy2DAsync(d_car, sizeof(double) * L, car, sizeof(double) * ld, sizeof(double) * B, 6, hipMemcpyHostToDevice, s));
  if (weights) MPC_HIP_CHECK(hipMemcpy2DAsync(d_w, sizeof(double) * L, weights, sizeof(double) * ld, sizeof(double) * B, MPC_NW, hipMemcpyHostToDevice, s));
  if (model) {
    MPC_HIP_CHECK(hipMemcpy2DAsync(d_model, sizeof(double) * L, model, sizeof(double) * ld, sizeof(double) * B, MPC_NMODEL, hipMemcpyHostToDevice, s));
    x.model = d_model;
  }
  if (latency) {
    MPC_HIP_CHECK(hipMemcpy2DAsync(d_lat, sizeof(double) * L, latency, sizeof(double) * ld, sizeof(double) * B, MPC_NLATENCY, hipMemcpyHostToDevice, s));
    x.latency = d_lat;
  }
  if (plant) {
    MPC_HIP_CHECK(hipMemcpy2DAsync(d_plant, sizeof(double) * L, plant, sizeof(double) * ld, sizeof(double) * B, MPC_NPLANT, hipMemcpyHostToDevice, s));
    x.plant = d_plant;
  }
  if (noise) {
    MPC_HIP_CHECK(hipMemcpy2DAsync(d_noise, sizeof(double) * L, noise, sizeof(double) * ld, sizeof(double) * B, MPC_NNOISE, hipMemcpyHostToDevice, s));
    x.noise = d_noise;
  }
  if (seen) x.seen = d_seen;
  if (horizon) {
    MPC_TRY(ensure_dev(&h->d_horizon, sizeof(int32_t) * (size_t)h->io_stride));
    MPC_HIP_CHECK(hipMemcpyAsync(h->d_horizon, horizon, sizeof(int32_t) * B, hipMemcpyHostToDevice, s));
    x.horizon = h->d_horizon;
  }
  if (budget) {
    MPC_TRY(ensure_dev(&h->d_budget, sizeof(int32_t) * (size_t)h->io_stride));
    MPC_HIP_CHECK(hipMemcpyAsync(h->d_budget, budget, sizeof(int32_t) * B, hipMemcpyHostToDevice, s));
    x.budget = h->d_budget;
  }
  MPC_HIP_CHECK(hipMemcpyAsync(d_tx, track_x, sizeof(double) * n_track, hipMemcpyHostToDevice, s));
  MPC_HIP_CHECK(hipMemcpyAsync(d_ty, track_y, sizeof(double) * n_track, hipMemcpyHostToDevice, s));
  MPC_TRY(drive_impl(h, B, L, steps, d_car, d_tx, d_ty, n_track, weights ? d_w : nullptr, O, x, d_sum, hist ? d_hist : nullptr, d_st, d_it, (void *)s));
  MPC_HIP_CHECK(hipMemcpy2DAsync(car, sizeof(double) * ld, d_car, sizeof(double) * L, sizeof(double) * B, 6, hipMemcpyDeviceToHost, s));
  MPC_HIP_CHECK(hipMemcpy2DAsync(summary, sizeof(double) * ld, d_sum, sizeof(double) * L, sizeof(double) * B, MPC_DRIVE_NSUM, hipMemcpyDeviceToHost, s));
  if (hist) MPC_HIP_CHECK(hipMemcpy2DAsync(hist, sizeof(double) * ld, d_hist, sizeof(double) * L, sizeof(double) * B, (size_t)steps * MPC_DRIVE_REC, hipMemcpyDeviceToHost, s));
  if (seen) MPC_HIP_CHECK(hipMemcpy2DAsync(seen, sizeof(double) * ld, d_seen, sizeof(double) * L, sizeof(double) * B, (size_t)steps * 4, hipMemcpyDeviceToHost, s));
  MPC_HIP_CHECK(hipMemcpyAsync(status, d_st, sizeof(int32_t) * B, hipMemcpyDeviceToHost, s));
  if (iters) MPC_HIP_CHECK(hipMemcpyAsync(iters, d_it, sizeof(int32_t) * B, hipMemcpyDeviceToHost, s));
  MPC_HIP_CHECK(hipStreamSynchronize(s));
  return MPC_OK;
}
extern "C" int mpc_drive_batch_host_budget(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                                           int n_track, const double *weights, const double *model, const int32_t *horizon, const int32_t *budget,
                                           const double *latency, const double *plant, const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts,
                                           double *summary, double *hist, int32_t *status, int32_t *iters) {
  return mpc_drive_batch_host_noise(h, B, ld, steps, car, track_x, track_y, n_track, weights, model, horizon, budget, latency, plant, nullptr, opts, warm_opts, summary,
                                    hist, nullptr, status, iters);
}
/* the zero column, under which a _noise call is the call without noise */
extern "C" int mpc_drive_noise_default(double *col7) {
  if (!col7) { g_last_error = "NULL argument"; return MPC_ERR_INVALID; }
  for (int q = 0; q < MPC_NNOISE; q++) col7[q] = 0.0;
  return MPC_OK;
}
/* mpc::drive_noise_draw on the host, for a seed as a column holds it */
extern "C" int mpc_drive_noise_draw(double seed, int32_t step, double *out7) {
  if (!out7) { g_last_error = "NULL argument"; return MPC_ERR_INVALID; }
  if (!mpc::drive_finite(seed) || !mpc::drive_seed_ok(seed)) { g_last_error = "mpc_drive_noise_draw: the seed must be an integer value in [0, 2^53)"; return MPC_ERR_INVALID; }
  if (step < 0) { g_last_error = "mpc_drive_noise_draw: step < 0"; return MPC_ERR_INVALID; }
  mpc::drive_noise_draw(seed, step, out7);
  return MPC_OK;
}
extern "C" int mpc_debug_philox4x32(const uint32_t *ctr, const uint32_t *key, uint32_t *out) {
  if (!ctr || !key || !out) { g_last_error = "NULL argument"; return MPC_ERR_INVALID; }
  mpc::philox4x32(ctr, key, out);
  return MPC_OK;
}
extern "C" int mpc_debug_drive_noise_device(MpcHandle *h, int64_t n, const double *seed, const int32_t *step, double *out, void *stream_) {
  if (!h) { g_last_error = "NULL handle"; return MPC_ERR_INVALID; }
  if (n < 0 || n > (int64_t)1 << 24 || (n > 0 && (!seed || !step || !out))) { g_last_error = "mpc_debug_drive_noise_device: n outside 0 .. 2^24, or a NULL argument"; return MPC_ERR_INVALID; }
  if (n == 0) return MPC_OK;
  MPC_ON_DEVICE(h);
  hipLaunchKernelGGL(mpc_debug_drive_noise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, n, seed, step, out);
  MPC_HIP_CHECK(hipGetLastError());
  return MPC_OK;
}
extern "C" int mpc_drive_batch_host_plant(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                                          int n_track, const double *weights, const double *model, const int32_t *horizon, const double *latency,
                                          const double *plant, const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary, double *hist,
                                          int32_t *status, int32_t *iters) {
  return mpc_drive_batch_host_budget(h, B, ld, steps, car, track_x, track_y, n_track, weights, model, horizon, nullptr, latency, plant, opts, warm_opts, summary,
                                     hist, status, iters);
}
extern "C" int mpc_drive_batch_host_horizon(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                                            int n_track, const double *weights, const double *model, const int32_t *horizon, const double *latency,
                                            const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts, double *summary, double *hist, int32_t *status,
                                            int32_t *iters) {
  return mpc_drive_batch_host_plant(h, B, ld, steps, car, track_x, track_y, n_track, weights, model, horizon, latency, nullptr, opts, warm_opts, summary, hist,
                                    status, iters);
}
extern "C" int mpc_drive_batch_host_latency(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                                            int n_track, const double *weights, const double *model, const double *latency, const MpcDriveOpts *opts,
                                            const MpcWarmOpts *warm_opts, double *summary, double *hist, int32_t *status, int32_t *iters) {
  return mpc_drive_batch_host_horizon(h, B, ld, steps, car, track_x, track_y, n_track, weights, model, nullptr, latency, opts, warm_opts, summary, hist, status,
                                      iters);
}
extern "C" int mpc_drive_batch_host_model(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                                          int n_track, const double *weights, const double *model, const MpcDriveOpts *opts,
                                          const MpcWarmOpts *warm_opts, double *summary, double *hist, int32_t *status, int32_t *iters) {
  return mpc_drive_batch_host_latency(h, B, ld, steps, car, track_x, track_y, n_track, weights, model, nullptr, opts, warm_opts, summary, hist, status, iters);
}
extern "C" int mpc_drive_batch_host(MpcHandle *h, int64_t B, int64_t ld, int steps, double *car, const double *track_x, const double *track_y,
                                    int n_track, const double *weights, const MpcDriveOpts *opts, const MpcWarmOpts *warm_opts,
                                    double *summary, double *hist, int32_t *status, int32_t *iters) {
  return mpc_drive_batch_host_model(h, B, ld, steps, car, track_x, track_y, n_track, weights, nullptr, opts, warm_opts, summary, hist, status, iters);
}

extern "C" int mpc_drive_info(const MpcHandle *h, int64_t *out2) {
  if (!h || !out2) { g_last_error = "NULL argument"; return MPC_ERR_INVALID; }
  out2[0] = h->n_drive_fused; out2[1] = h->n_drive_stepwise;
  return MPC_OK;
}

extern "C" int mpc_synchronize(MpcHandle *h) {
  if (!h) return MPC_ERR_INVALID;
  MPC_ON_DEVICE(h);
  MPC_HIP_CHECK(hipStreamSynchronize(h->stream));
  return tail_drain(h);
}

/* rows of a host array <-> the pinned staging block: on a few threads when there is enough to move (a 65 536-instance batch is
 * 22 MB in and 16 MB out; one core copies pageable memory at ~10 GB/s, which was most of the call's 4 ms) */
template <class Fn>
static void for_rows(int n_rows, size_t row_bytes, Fn fn) {
  const size_t total = (size_t)n_rows * row_bytes;
  int nt = total >= ((size_t)4 << 20) ? 4 : 1;
  if (nt > n_rows) nt = n_rows;
  if (nt <= 1) { for (int q = 0; q < n_rows; q++) fn(q); return; }
  std::vector<std::thread> th;
  th.reserve(nt);
  for (int t = 0; t < nt; t++)
    th.emplace_back([=]() { for (int q = t; q < n_rows; q += nt) fn(q); });
  for (auto &x : th) x.join();
}

/* host pointers: one copy in, the launch(es), one copy out, on the handle's own stream; R = the handle's precision */
/* (x.warm: the host arrays of mpc_solve_batch_host_warm and the options in effect; x.model: the host array of mpc_solve_batch_host_model,
 * which goes through a device block of its own, rows packed like the inputs; both fp64 handles only) */
template <class R>
static int solve_host(MpcHandle *h, int64_t B, int64_t ld, const R *state, const R *coeffs, const R *yaw_lo, const R *yaw_hi,
                      const R *weights, R *out, R *traj, int32_t *status, int32_t *iters, const CallExtras &x) {
  MPC_TRY(x.refused);
  if ((h->params.precision == MPC_PRECISION_F32) != (sizeof(R) == 4)) {
    g_last_error = "this handle was created with the other precision (mpc_solve_batch_host for fp64 handles, mpc_solve_batch_host_f32 for MPC_PRECISION_F32)";
    return MPC_ERR_INVALID;
  }
  MPC_TRY(check_batch(h, B, ld));
  if (B == 0) { h->last_B = 0; h->have_stats = false; return MPC_OK; }
  if (!state || !coeffs || !yaw_lo || !yaw_hi || !out || !status) { g_last_error = "NULL argument"; return MPC_ERR_INVALID; }
  MPC_ON_DEVICE(h);
  const int N = h->params.N;
  const int64_t S = h->io_stride;
  constexpr int kInRows = 6 + MPC_NCOEF + 2 + MPC_NW;              /* 25 */
  constexpr int kIntRows = sizeof(R) == 8 ? 1 : 2;                 /* status and iters: 2 x int32 per instance */
  const int kOutRows = MPC_NOUT + 2 * N + kIntRows;                /* out, traj, status|iters (N is fixed per handle) */
  MPC_TRY(ensure_dev(&h->d_io, sizeof(R) * (kInRows + kOutRows) * S));
  if (!h->h_io) MPC_HIP_CHECK(hipHostMalloc((void **)&h->h_io, sizeof(R) * (kInRows + kOutRows) * S, hipHostMallocDefault));
  /* rows packed with leading dimension L (B rounded up to 16: 64-byte rows), so each direction is ONE copy */
  const int64_t L = (B + 15) / 16 * 16;
  const int in_rows = weights ? kInRows : kInRows - MPC_NW;
  const int out_rows = MPC_NOUT + (traj ? 2 * N : 0) + kIntRows;
  R *hi = (R *)h->h_io, *ho = (R *)h->h_io + kInRows * S;
  R *di = (R *)h->d_io, *d_oblk = (R *)h->d_io + kInRows * S;
  for_rows(in_rows, sizeof(R) * B, [=](int q) {
    const R *src = q < 6 ? state + q * ld : q < 11 ? coeffs + (q - 6) * ld : q == 11 ? yaw_lo : q == 12 ? yaw_hi : weights + (q - 13) * ld;
    memcpy(hi + q * L, src, sizeof(R) * B);
  });
  hipStream_t s = h->stream;
  MPC_HIP_CHECK(hipMemcpyAsync(di, hi, sizeof(R) * in_rows * L, hipMemcpyHostToDevice, s));
  R *d_o = d_oblk, *d_t = d_o + MPC_NOUT * L;
  int32_t *d_st = (int32_t *)(d_o + (out_rows - kIntRows) * L), *d_it = d_st + L;
  CallExtras dx;
  MPC_TRY(host_extras_in(h, B, x, nullptr, s, &dx));
  if (x.model) {
    MPC_TRY(ensure_dev(&h->d_model, sizeof(double) * MPC_NMODEL * (size_t)S));
    MPC_HIP_CHECK(hipMemcpy2DAsync(h->d_model, sizeof(double) * L, x.model, sizeof(double) * ld, sizeof(double) * B, MPC_NMODEL, hipMemcpyHostToDevice, s));
    dx.model = h->d_model;
  }
  if (x.lane_rows()) {
    /* the horizons go along like the model columns, and so do the budgets.  An instance writes only the first n points of each half
     * of its traj column: the rows behind them come back as the caller has them, so the caller's traj goes in with the inputs */
    if (x.horizon) {
      MPC_TRY(ensure_dev(&h->d_horizon, sizeof(int32_t) * (size_t)S));
      MPC_HIP_CHECK(hipMemcpyAsync(h->d_horizon, x.horizon, sizeof(int32_t) * B, hipMemcpyHostToDevice, s));
      dx.horizon = h->d_horizon;
    }
    if (x.budget) {
      MPC_TRY(ensure_dev(&h->d_budget, sizeof(int32_t) * (size_t)S));
      MPC_HIP_CHECK(hipMemcpyAsync(h->d_budget, x.budget, sizeof(int32_t) * B, hipMemcpyHostToDevice, s));
      dx.budget = h->d_budget;
    }
    if (traj) {
      for_rows(2 * N, sizeof(R) * B, [=](int q) { memcpy(ho + (MPC_NOUT + q) * L, traj + q * ld, sizeof(R) * B); });
      MPC_HIP_CHECK(hipMemcpyAsync(d_t, ho + MPC_NOUT * L, sizeof(R) * 2 * N * L, hipMemcpyHostToDevice, s));
    }
  }
  MPC_TRY(launch_solve<R>(h, {B, L, L, di, di + 6 * L, di + 11 * L, di + 12 * L, weights ? di + 13 * L : nullptr, d_o, traj ? d_t : nullptr, d_st, d_it},
                          (void *)s, kStats | kOrder, dx));
  MPC_TRY(host_extras_out(h, B, x, s));
  MPC_HIP_CHECK(hipMemcpyAsync(ho, d_o, sizeof(R) * out_rows * L, hipMemcpyDeviceToHost, s));
  MPC_HIP_CHECK(hipStreamSynchronize(s));
  for_rows(MPC_NOUT + (traj ? 2 * N : 0), sizeof(R) * B, [=](int q) {
    R *dst = q < MPC_NOUT ? out + q * ld : traj + (q - MPC_NOUT) * ld;
    memcpy(dst, ho + q * L, sizeof(R) * B);
  });
  const int32_t *h_st = (const int32_t *)(ho + (out_rows - kIntRows) * L);
  memcpy(status, h_st, sizeof(int32_t) * B);
  if (iters) memcpy(iters, h_st + L, sizeof(int32_t) * B);
  return MPC_OK;
}

extern "C" int mpc_solve_batch_host(MpcHandle *h, int64_t B, int64_t ld, const double *state,
                                    const double *coeffs, const double *yaw_lo, const double *yaw_hi,
                                    const double *weights, double *out, double *traj, int32_t *status,
                                    int32_t *iters) {
  return solve_host<double>(h, B, ld, state, coeffs, yaw_lo, yaw_hi, weights, out, traj, status, iters, call_extras(h));
}

extern "C" int mpc_solve_batch_host_model(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                          const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                          double *out, double *traj, int32_t *status, int32_t *iters) {
  return solve_host<double>(h, B, ld, state, coeffs, yaw_lo, yaw_hi, weights, out, traj, status, iters, call_extras(h, model));
}

extern "C" int mpc_solve_batch_host_warm(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                         const double *yaw_lo, const double *yaw_hi, const double *weights, const double *warm_in,
                                         const int32_t *warm_status, double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts,
                                         double *out, double *traj, int32_t *status, int32_t *iters) {
  return solve_host<double>(h, B, ld, state, coeffs, yaw_lo, yaw_hi, weights, out, traj, status, iters,
                            call_extras(h, nullptr, true, warm_in, warm_status, warm_out, ld_warm, opts));
}

extern "C" int mpc_solve_batch_host_warm_model(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                               const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                               const double *warm_in, const int32_t *warm_status, double *warm_out, int64_t ld_warm,
                                               const MpcWarmOpts *opts, double *out, double *traj, int32_t *status, int32_t *iters) {
  return solve_host<double>(h, B, ld, state, coeffs, yaw_lo, yaw_hi, weights, out, traj, status, iters,
                            call_extras(h, model, true, warm_in, warm_status, warm_out, ld_warm, opts));
}

extern "C" int mpc_solve_batch_host_horizon(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                            const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                            const int32_t *horizon, double *out, double *traj, int32_t *status, int32_t *iters) {
  return solve_host<double>(h, B, ld, state, coeffs, yaw_lo, yaw_hi, weights, out, traj, status, iters,
                            call_extras(h, model, false, nullptr, nullptr, nullptr, 0, nullptr, horizon));
}

extern "C" int mpc_solve_batch_host_budget(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                           const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                           const int32_t *horizon, const int32_t *budget, const double *warm_in, const int32_t *warm_status,
                                           double *warm_out, int64_t ld_warm, const MpcWarmOpts *opts, double *out, double *traj,
                                           int32_t *status, int32_t *iters) {
  return solve_host<double>(h, B, ld, state, coeffs, yaw_lo, yaw_hi, weights, out, traj, status, iters,
                            call_extras(h, model, true, warm_in, warm_status, warm_out, ld_warm, opts, horizon, nullptr, budget));
}
extern "C" int mpc_solve_batch_host_warm_horizon(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                                 const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                                 const int32_t *horizon, const double *warm_in, const int32_t *warm_status, double *warm_out,
                                                 int64_t ld_warm, const MpcWarmOpts *opts, double *out, double *traj, int32_t *status,
                                                 int32_t *iters) {
  return mpc_solve_batch_host_budget(h, B, ld, state, coeffs, yaw_lo, yaw_hi, weights, model, horizon, nullptr, warm_in, warm_status, warm_out, ld_warm, opts, out,
                                     traj, status, iters);
}

extern "C" int mpc_solve_batch_host_f32(MpcHandle *h, int64_t B, int64_t ld, const float *state,
                                        const float *coeffs, const float *yaw_lo, const float *yaw_hi,
                                        const float *weights, float *out, float *traj, int32_t *status,
                                        int32_t *iters) {
  return solve_host<float>(h, B, ld, state, coeffs, yaw_lo, yaw_hi, weights, out, traj, status, iters, call_extras(h));
}

/* ---- the certificate of a stored point (include/mpc_amd_certify.h) ---- */
/* What both forms check before they touch anything: the handle and the model rule (call_extras), the precision -- also of a call
 * without model and horizon -- and the batch (check_batch).  *empty: B == 0, nothing to do (the arrays may be NULL). */
static int certify_args(const MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs, const double *yaw_lo,
                        const double *yaw_hi, const double *model, const double *sol, int64_t ld_sol, const double *cert,
                        const int32_t *verdict, bool *empty) {
  MPC_TRY(call_extras(h, model).refused);
  if (h->params.precision != MPC_PRECISION_F64) {
    g_last_error = "certificate: fp64 handles only (this one was created with MPC_PRECISION_F32)";
    return MPC_ERR_INVALID;
  }
  MPC_TRY(check_batch(h, B, ld));
  if (ld_sol < B) { g_last_error = "ld_sol < B"; return MPC_ERR_INVALID; }
  *empty = B == 0;
  if (B > 0 && (!state || !coeffs || !yaw_lo || !yaw_hi || !sol || !cert || !verdict)) { g_last_error = "NULL argument"; return MPC_ERR_INVALID; }
  return MPC_OK;
}

/* the one launch, on device arrays */
static int certify_launch(const MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs, const double *yaw_lo,
                          const double *yaw_hi, const double *weights, const double *model, const int32_t *horizon, const double *sol,
                          int64_t ld_sol, double *cert, int32_t *verdict, hipStream_t s) {
  const dim3 grid((unsigned)((B + kCertBlock - 1) / kCertBlock)), block(kCertBlock);
  const auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, block, 0, s, h->params, B, ld, state, coeffs, yaw_lo, yaw_hi, weights, model, horizon, sol, ld_sol, cert, verdict);
  };
  if (horizon) launch(mpc_certify_kernel<2>);
  else if (model) launch(mpc_certify_kernel<1>);
  else launch(mpc_certify_kernel<0>);
  MPC_HIP_CHECK(hipGetLastError());
  return MPC_OK;
}

extern "C" int mpc_certify_batch_device(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                        const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                        const int32_t *horizon, const double *sol, int64_t ld_sol, double *cert, int32_t *verdict,
                                        void *stream_) {
  bool empty = false;
  MPC_TRY(certify_args(h, B, ld, state, coeffs, yaw_lo, yaw_hi, model, sol, ld_sol, cert, verdict, &empty));
  if (empty) return MPC_OK;
  MPC_ON_DEVICE(h);
  return certify_launch(h, B, ld, state, coeffs, yaw_lo, yaw_hi, weights, model, horizon, sol, ld_sol, cert, verdict, (hipStream_t)stream_);
}

/* Host arrays: one copy in, the launch, one copy out on the handle's own device and stream; synchronises.  The staging block is the
 * one the run() and telemetry host forms keep on the handle (grown on demand), rows of leading dimension L:
 * state 6 | coeffs 5 | yaw_lo | yaw_hi | weights 12 | model 6 | sol | cert 12 | horizon and verdict (int32 each, one row). */
extern "C" int mpc_certify_batch_host(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                      const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                                      const int32_t *horizon, const double *sol, int64_t ld_sol, double *cert, int32_t *verdict) {
  bool empty = false;
  MPC_TRY(certify_args(h, B, ld, state, coeffs, yaw_lo, yaw_hi, model, sol, ld_sol, cert, verdict, &empty));
  if (empty) return MPC_OK;
  MPC_ON_DEVICE(h);
  const int64_t L = (B + 7) / 8 * 8, sol_rows = mpc_warm_rows(h->params.N);
  const int64_t in_rows = 6 + MPC_NCOEF + 2 + MPC_NW + MPC_NMODEL;
  MPC_TRY(grow_dev(&h->d_tel, &h->tel_bytes, sizeof(double) * (size_t)((in_rows + sol_rows + MPC_NCERT + 1) * L)));
  double *d_st = h->d_tel, *d_cf = d_st + 6 * L, *d_yl = d_cf + MPC_NCOEF * L, *d_yh = d_yl + L, *d_w = d_yh + L, *d_model = d_w + MPC_NW * L;
  double *d_sol = d_model + MPC_NMODEL * L, *d_cert = d_sol + sol_rows * L;
  int32_t *d_hz = (int32_t *)(d_cert + MPC_NCERT * L), *d_verdict = d_hz + L;
  hipStream_t s = h->stream;
  const auto rows_in = [&](double *dst, const double *src, int64_t src_ld, int64_t rows) {
    return hipMemcpy2DAsync(dst, sizeof(double) * L, src, sizeof(double) * src_ld, sizeof(double) * B, (size_t)rows, hipMemcpyHostToDevice, s);
  };
  MPC_HIP_CHECK(rows_in(d_st, state, ld, 6));
  MPC_HIP_CHECK(rows_in(d_cf, coeffs, ld, MPC_NCOEF));
  MPC_HIP_CHECK(rows_in(d_yl, yaw_lo, ld, 1));
  MPC_HIP_CHECK(rows_in(d_yh, yaw_hi, ld, 1));
  if (weights) MPC_HIP_CHECK(rows_in(d_w, weights, ld, MPC_NW));
  if (model) MPC_HIP_CHECK(rows_in(d_model, model, ld, MPC_NMODEL));
  MPC_HIP_CHECK(rows_in(d_sol, sol, ld_sol, sol_rows));
  if (horizon) MPC_HIP_CHECK(hipMemcpyAsync(d_hz, horizon, sizeof(int32_t) * B, hipMemcpyHostToDevice, s));
  MPC_TRY(certify_launch(h, B, L, d_st, d_cf, d_yl, d_yh, weights ? d_w : nullptr, model ? d_model : nullptr, horizon ? d_hz : nullptr, d_sol, L,
                         d_cert, d_verdict, s));
  MPC_HIP_CHECK(hipMemcpy2DAsync(cert, sizeof(double) * ld, d_cert, sizeof(double) * L, sizeof(double) * B, MPC_NCERT, hipMemcpyDeviceToHost, s));
  MPC_HIP_CHECK(hipMemcpyAsync(verdict, d_verdict, sizeof(int32_t) * B, hipMemcpyDeviceToHost, s));
  MPC_HIP_CHECK(hipStreamSynchronize(s));
  return MPC_OK;
}

extern "C" int mpc_get_stats(MpcHandle *h, MpcBatchStats *st) {
  if (!h || !st) return MPC_ERR_INVALID;
  memset(st, 0, sizeof(*st));
  st->batch = h->last_B;
  if (h->last_B == 0 || !(h->have_stats || h->stats_pending)) return MPC_OK;
  MPC_ON_DEVICE(h);
  if (h->stats_pending) {                      /* gathered now, behind the call's own launch (its arrays must still be there) */
    MPC_HIP_CHECK(hipStreamWaitEvent(h->stream, h->st_ev, 0));
    const int rc = record_stats(h, h->st_B, h->st_status, h->st_iters, h->stream);
    if (rc != MPC_OK) return rc;
    h->stats_pending = false;
  }
  MPC_HIP_CHECK(hipEventSynchronize(h->ev_stats));
  unsigned long long acc[kStatWords];
  MPC_HIP_CHECK(hipMemcpy(acc, h->d_stats, sizeof(acc), hipMemcpyDeviceToHost));
  st->n_success = (int64_t)acc[MPC_STATUS_SUCCESS]; st->n_maxiter = (int64_t)acc[MPC_STATUS_MAXITER];
  st->n_linesearch = (int64_t)acc[MPC_STATUS_LINESEARCH]; st->n_infeasible = (int64_t)acc[MPC_STATUS_INFEASIBLE];
  st->n_numeric = (int64_t)acc[4]; st->n_acceptable = (int64_t)acc[8]; st->iter_sum = (int64_t)acc[5]; st->iter_max = (int32_t)acc[6]; st->n_pending = (int32_t)acc[7];
  if (h->timed) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) st->kernel_ms = ms;
  }
  return MPC_OK;
}

extern "C" int mpc_debug_math_ext(int device, int64_t n, const double *x, double *sn, double *cs, double *rc, double *at, double *lg) {
  if (n < 0 || (n > 0 && (!x || !sn || !cs || !rc || !at || !lg))) return MPC_ERR_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { g_last_error = "no HIP device"; return MPC_ERR_NO_DEVICE; }
  if (device >= 0) MPC_HIP_CHECK(hipSetDevice(device));
  if (n == 0) return MPC_OK;
  double *d = nullptr;
  MPC_HIP_CHECK(hipMalloc((void **)&d, sizeof(double) * 6 * n));
  hipError_t e = hipMemcpy(d, x, sizeof(double) * n, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(mpc_debug_math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, n, d, d + n, d + 2 * n, d + 3 * n, d + 4 * n, d + 5 * n);
    e = hipGetLastError();
  }
  double *outs[5] = {sn, cs, rc, at, lg};
  for (int q = 0; q < 5 && e == hipSuccess; q++) e = hipMemcpy(outs[q], d + (q + 1) * n, sizeof(double) * n, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) { g_last_error = std::string("mpc_debug_math: ") + hipGetErrorString(e); return MPC_ERR_HIP; }
  return MPC_OK;
}

extern "C" int mpc_debug_math_all(int device, int64_t n, const double *x, const double *y, double *out) {
  if (n < 0 || n > (int64_t)1 << 24 || (n > 0 && (!x || !y || !out))) return MPC_ERR_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { g_last_error = "no HIP device"; return MPC_ERR_NO_DEVICE; }
  if (device >= 0) MPC_HIP_CHECK(hipSetDevice(device));
  if (n == 0) return MPC_OK;
  const size_t rows = MPC_DEBUG_MATH_ROWS, un = (size_t)n;
  double *d = nullptr;   /* x, y, then the rows */
  MPC_HIP_CHECK(hipMalloc((void **)&d, sizeof(double) * (rows + 2) * un));
  hipError_t e = hipMemcpy(d, x, sizeof(double) * un, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + un, y, sizeof(double) * un, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(mpc_debug_math_all_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, n, d, d + un, d + 2 * un);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, d + 2 * un, sizeof(double) * rows * un, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) { g_last_error = std::string("mpc_debug_math_all: ") + hipGetErrorString(e); return MPC_ERR_HIP; }
  return MPC_OK;
}

extern "C" int mpc_debug_math(int device, int64_t n, const double *x, double *sn, double *cs, double *rc) {
  if (n < 0) return MPC_ERR_INVALID;
  std::vector<double> at((size_t)n), lg((size_t)n);
  return mpc_debug_math_ext(device, n, x, sn, cs, rc, at.data(), lg.data());
}
