/*
 * mpc_amd_certify.h -- the certificate of a stored solution.  Part of include/mpc_amd.h, which includes it (do not include it on its
 * own): the two mpc_certify_batch_* entry points and everything a caller needs to know about them.
 */
#ifndef MPC_AMD_CERTIFY_H
#define MPC_AMD_CERTIFY_H
#ifndef MPC_AMD_H
#error "include mpc_amd.h"
#endif

/* ---- certify a stored primal-dual point: IPOPT's final error summary ------------------------------------------------------------
 * Every solve reports one status and an iteration count per instance.  These two entry points say how good a POINT is: they evaluate
 * the NLP of the solve -- the reference's, branch outcomes and objective scaling decided at the reference's start point -- once, at
 * a primal-dual point the caller names, and write what IPOPT prints when it stops: objective, dual infeasibility, constraint
 * violation, complementarity, overall NLP error; and a verdict by the handle's tolerances.  Nothing is solved, nothing of the handle
 * changes (mpc_get_stats and the batch ids do not see the call), and no existing entry point is touched.
 *
 * Arguments.  state .. horizon: exactly those of mpc_solve_batch_device_horizon, with its conventions: weights, model and horizon
 *   may each be NULL, and with all three NULL the call certifies points of mpc_solve_batch_device.
 *   sol [mpc_warm_rows(N)][ld_sol]: records in the layout of MPC_WARM_REC -- what warm_out of any _warm entry point holds (a cold
 *     _warm call, warm_in = NULL, is the way to get one).  It is read AS IT IS: no push into the interior, no floor on the duals, no
 *     projection of psi, no shift.  With `horizon`, only the first horizon[i] - 1 records of instance i are read.
 *   cert [MPC_NCERT][ld]: the measures, rows MPC_CERT_*.  verdict [ld]: MPC_CERT_CONVERGED .. MPC_CERT_NO_PROBLEM.
 *   Columns from B on are neither read nor written.
 * A run() solve is certified without an entry point of its own: mpc_run_batch_device_warm with warm_in = NULL writes warm_out and
 *   pre [15][ld]; rows 0-5 of pre are the state, rows 6-10 the coefficients, rows 11 and 12 the psi bounds: pass those rows, with
 *   the same ld, and weights = NULL.
 * Scaling and signs.  The multipliers and bound duals of a record live in the SCALED problem (objective times df), as the solver
 *   keeps them.  The rows called unscaled below are divided by df, as the solver's own termination test does.  lam belongs to the
 *   model rows as the reference writes them, x1 - (x0 + ...), and the Lagrangian is df f + lam^T g - zL^T (x - l) + zU^T (u - x).
 *   The six variables of index 0 are the given state: the record holds no multipliers for them, and their rows are no part of the
 *   certificate (an error summary as with MpcParams.initial_state_rows = 0, whatever the handle says).
 * Verdict.  E_0 is IPOPT's scaled overall error at barrier parameter 0 (the row MPC_CERT_NLP_ERROR).
 *   CONVERGED: E_0 <= tol and the unscaled dual infeasibility, constraint violation and complementarity within dual_inf_tol,
 *   constr_viol_tol, compl_inf_tol -- the test every fp64 solve here ends on.  ACCEPTABLE: the same with the acceptable_* values
 *   (never with acceptable_iter = 0).  NOT_CONVERGED: neither.  The termination polish (out_step_tol) is no part of it: that
 *   describes the path of a solve, not a point.
 * Instances that cannot be certified.  NO_PROBLEM: the set-up of the solve refuses the instance -- a state outside its own bounds,
 *   an unusable model column, a horizon outside 3 .. N -- and all rows hold not-a-number.  NOT_A_POINT: a value of the record is not
 *   finite (beyond 1e300 in size, or not-a-number), a bounded quantity lies outside its relaxed box, or a dual is negative;
 *   MPC_CERT_BOUND_VIOL is written if the record's values are finite, every other row holds not-a-number.  Either way the launch
 *   ends (no loop of the kernel has a trip count that the data decide) and every other instance comes out bit for bit as without.
 * Handles.  Every fp64 handle, also one whose solve starts in fp32 (the model-call rule).  MPC_PRECISION_F32: MPC_ERR_INVALID with
 *   a message.  NULL arguments, ld < B, ld_sol < B, B above the handle's capacity: MPC_ERR_INVALID.
 * Cost.  The device form is ONE launch on `stream`, a lane per instance, 22 (n - 1) doubles read per instance; it allocates
 *   nothing, defers nothing and synchronises nothing.  The host form is one copy in, that launch, one copy out on the handle's own
 *   device and stream, and synchronises. */
#define MPC_NCERT 12
enum { MPC_CERT_OBJ = 0,        /* f at the point, unscaled, the i = 0 constants included: what out[8] of a solve reports */
       MPC_CERT_CONSTR_VIOL,    /* max |model row|, rows of index 1 .. n-1 (MPC.cpp:145-152) */
       MPC_CERT_DUAL_INF,       /* max |grad_x Lagrangian| over the variables the record holds, UNSCALED (the solver's dinf / df) */
       MPC_CERT_COMPL,          /* max slack x dual over the 8 (n-1) bounds, relaxed bounds, unscaled (the solver's cmax / df) */
       MPC_CERT_NLP_ERROR,      /* IPOPT's scaled overall error E_0 */
       MPC_CERT_BOUND_VIOL,     /* how far psi, v, delta, a lie outside the CALLER's bounds (0 inside; up to bound_relax_factor max(1,|b|) is normal) */
       MPC_CERT_OBJ_SCALING,    /* df, IPOPT's gradient-based objective scaling at the start point */
       MPC_CERT_COST_CTE, MPC_CERT_COST_EPSI, MPC_CERT_COST_V, MPC_CERT_COST_DELTA, MPC_CERT_COST_DDELTA };
                                /* the five groups of terms of the frozen objective, i = 0 included; the w[9] v_0^2 term of a
                                 * negative start speed counts under COST_V; they add up to OBJ */
enum { MPC_CERT_CONVERGED = 0, MPC_CERT_ACCEPTABLE = 1, MPC_CERT_NOT_CONVERGED = 2,
       MPC_CERT_NOT_A_POINT = 3,   /* a value of the record is not finite, a bounded quantity lies outside its relaxed box, a dual is negative */
       MPC_CERT_NO_PROBLEM = 4 };  /* the set-up refuses the instance: state outside its own bounds, unusable model column, horizon outside 3..N */

int mpc_certify_batch_device(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                             const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                             const int32_t *horizon, const double *sol, int64_t ld_sol, double *cert, int32_t *verdict, void *stream);
int mpc_certify_batch_host(MpcHandle *h, int64_t B, int64_t ld, const double *state, const double *coeffs,
                           const double *yaw_lo, const double *yaw_hi, const double *weights, const double *model,
                           const int32_t *horizon, const double *sol, int64_t ld_sol, double *cert, int32_t *verdict);

#endif /* MPC_AMD_CERTIFY_H */
