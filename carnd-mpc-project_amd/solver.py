"""BatchedMPC: thin Python handle over the C ABI (include/mpc_amd.h).

Mirrors, for a batch, what ``MPC::solve(state, target_velocity, x_traj, y_traj)``
returns in the reference (src/control/MPC.cpp:183-325): a 9-vector per instance
``{x1,y1,psi1,v1,cte1,epsi1,delta0,a0,cost}`` plus the optional N-point (x,y)
trajectory, and a status per instance (the reference only prints it).
torch is used for device memory and streams only.
"""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import MpcBatchStats, MpcParams, check, library


class BatchedMPC:
    def __init__(self, params: MpcParams, max_batch: int, device: int = -1):
        self.params = params.copy()
        self.max_batch = int(max_batch)
        self._h = C.c_void_p()
        check(library().mpc_create(C.byref(self.params), int(device), self.max_batch, C.byref(self._h)), "mpc_create")

    # -- lifetime ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            library().mpc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def N(self):
        return self.params.N

    @property
    def f32(self):
        """True for a handle created with params.precision = MPC_PRECISION_F32 (float32 tensors in and out)."""
        return self.params.precision == _abi.PRECISION_F32

    def _dtype(self):
        import torch
        return torch.float32 if self.f32 else torch.float64

    def set_params(self, params: MpcParams):
        check(library().mpc_set_params(self._h, C.byref(params)), "mpc_set_params")
        self.params = params.copy()

    # -- device path (torch tensors resident in HBM) -------------------------
    def alloc_outputs(self, B, device, want_traj=False):
        import torch
        dt = self._dtype()
        out = {
            "out": torch.empty((_abi.NOUT, B), dtype=dt, device=device),
            "status": torch.empty((B,), dtype=torch.int32, device=device),
            "iters": torch.empty((B,), dtype=torch.int32, device=device),
            "traj": torch.empty((2 * self.N, B), dtype=dt, device=device) if want_traj else None,
        }
        return out

    def warm_rows(self):
        """Rows of this handle's warm buffers: (N-1) * WARM_REC."""
        return _abi.warm_rows(self.N)

    def _call(self, family, head, outs, model=None, warm=None, horizon=None, budget=None):
        """Call `family`'s entry point for this call, chosen by the rule of include/mpc_amd.h: the name is the family's, + "_warm"
        for a warm call (`warm`: the values the _warm form takes -- warm_in, warm_status, warm_out, ld_warm, opts; the stepwise
        rollout: opts alone), + "_model" with `model` (a pointer) or "_horizon" with `horizon` (a pointer; `model` may then be
        None); the arguments are the handle, head, [model, [horizon]], warm, outs.  With `budget` (a pointer; the solve families,
        include/mpc_amd_budget.h): the _budget form -- head, model, horizon, budget, the five warm values (a call without: NULL
        buffers), outs."""
        if budget is not None:
            name = family + "_budget"
            rc = getattr(library(), name)(self._h, *head, model, horizon, budget, *(warm or (None, None, None, head[0], None)), *outs)
            if rc != 0:
                check(rc, name)
            return
        extra = () if model is None and horizon is None else ((model,) if horizon is None else (model, horizon))
        name = family + ("_warm" if warm is not None else "") + ("_horizon" if horizon is not None else "_model" if model is not None else "")
        rc = getattr(library(), name)(self._h, *head, *extra, *(warm or ()), *outs)
        if rc != 0:
            check(rc, name)

    def solve_torch(self, state, coeffs, yaw_lo, yaw_hi, weights=None, want_traj=False, outputs=None, stream=None,
                    warm=None, warm_status=None, want_warm=False, warm_opts=None, model=None, horizon=None, budget=None):
        """state [6,B], coeffs [5,B], yaw_lo/hi [B], weights [12,B] or None: CUDA tensors, float64 (float32 for a
        handle created with precision F32).  Asynchronous on ``stream`` (default: torch's current stream).  Returns the
        dict of output tensors.

        Warm start (opt-in, fp64 handles; mpc_solve_batch_device_warm): ``warm`` [warm_rows(), B] is the "warm" tensor an
        earlier call returned and ``warm_status`` [B] int32 that call's status (None: every column is valid); with
        ``want_warm`` (implied by ``warm``) the result holds "warm", the final primal-dual iterate -- written in place when
        ``outputs`` carries the same tensor.  ``warm_opts``: an MpcWarmOpts (None: the library's defaults).

        ``model`` [6, B] float64 (fp64 handles; mpc_solve_batch_device_model): dt, Lf, max_steering, max_acceleration,
        max_deceleration and max_speed of every instance (rows _abi.MODEL_*, scenarios.model_rows gives a handle's own) -- one
        launch of the single-phase fp64 solver whatever the handle's dispatch; an unusable column ends INFEASIBLE.  Together
        with the warm arguments: mpc_solve_batch_device_warm_model -- a record is judged against the instance's own limits.

        ``horizon`` [B] int32 (fp64 handles, max_soc = 0; mpc_solve_batch_device_horizon, _warm_horizon): the N of every instance,
        3 .. the handle's N, with or without ``model``; dispatched like a model call.  "traj" and "warm" keep the handle's shapes:
        instance i writes x, y of its n points (rows 0..n-1 and N..N+n-1) and the records of its n-1 stages, nothing behind them.
        Any other value ends that instance INFEASIBLE.  Sort a batch by horizon: a wave is as slow as its longest one.

        ``budget`` [B] int32 (fp64 handles, max_soc = 0; mpc_solve_batch_device_budget): the interior-point iterations every instance
        may take over all of its attempts -- the reference's solve deadline, counted in iterations.  An instance that uses its
        budget up ends MAXITER with its current iterate (iters == budget), and with ``budget`` a "warm" record that came with MAXITER is a
        candidate like one with SUCCESS.  budget < 1 ends that instance INFEASIBLE.  Dispatched like a horizon call."""
        import torch
        B = state.shape[1]
        dt = self._dtype()
        for name, t, rows in (("state", state, 6), ("coeffs", coeffs, 5)):
            if t.dtype != dt or not t.is_cuda or not t.is_contiguous() or t.shape != (rows, B):
                raise ValueError("%s must be a contiguous %s CUDA tensor of shape (%d, B)" % (name, dt, rows))
        for name, t in (("yaw_lo", yaw_lo), ("yaw_hi", yaw_hi)):
            if t.dtype != dt or not t.is_cuda or not t.is_contiguous() or t.shape != (B,):
                raise ValueError("%s must be a contiguous %s CUDA tensor of shape (B,)" % (name, dt))
        if weights is not None and (weights.dtype != dt or not weights.is_cuda or
                                    not weights.is_contiguous() or weights.shape != (_abi.NW, B)):
            raise ValueError("weights must be a contiguous %s CUDA tensor of shape (12, B)" % dt)
        if outputs is None:
            outputs = self.alloc_outputs(B, state.device, want_traj)
        s = stream if stream is not None else torch.cuda.current_stream(state.device)
        traj = outputs.get("traj")
        if model is not None:
            self._check_model(model, B)
        if horizon is not None:
            self._check_horizon(horizon, B)
        if budget is not None:
            self._check_horizon(budget, B, "budget")
        warm_args = None
        if warm is not None or want_warm:
            rows = self.warm_rows()
            if warm is not None and (warm.dtype != torch.float64 or not warm.is_cuda or not warm.is_contiguous() or tuple(warm.shape) != (rows, B)):
                raise ValueError("warm must be a contiguous float64 CUDA tensor of shape (%d, B)" % rows)
            if warm_status is not None and (warm_status.dtype != torch.int32 or not warm_status.is_cuda or tuple(warm_status.shape) != (B,)):
                raise ValueError("warm_status must be an int32 CUDA tensor of shape (B,)")
            if outputs.get("warm") is None:
                outputs["warm"] = torch.empty((rows, B), dtype=torch.float64, device=state.device)
            warm_args = (warm.data_ptr() if warm is not None else None, warm_status.data_ptr() if warm_status is not None else None,
                         outputs["warm"].data_ptr(), B, C.byref(warm_opts) if warm_opts is not None else None)
        head = (B, B, state.data_ptr(), coeffs.data_ptr(), yaw_lo.data_ptr(), yaw_hi.data_ptr(),
                weights.data_ptr() if weights is not None else None)
        outs = (outputs["out"].data_ptr(), traj.data_ptr() if traj is not None else None, outputs["status"].data_ptr(),
                outputs["iters"].data_ptr(), C.c_void_p(s.cuda_stream))
        if self.f32 and model is None and warm_args is None and horizon is None and budget is None:
            check(library().mpc_solve_batch_device_f32(self._h, *head, *outs), "mpc_solve_batch_device")
        else:
            self._call("mpc_solve_batch_device", head, outs, model.data_ptr() if model is not None else None, warm_args,
                       horizon.data_ptr() if horizon is not None else None, budget.data_ptr() if budget is not None else None)
        return outputs

    @staticmethod
    def _check_horizon(horizon, B, what="horizon"):
        import torch
        if horizon.dtype != torch.int32 or not horizon.is_cuda or not horizon.is_contiguous() or tuple(horizon.shape) != (B,):
            raise ValueError("%s must be a contiguous int32 CUDA tensor of shape (B,)" % what)

    @staticmethod
    def _host_horizon(horizon, B, what="horizon"):
        horizon = np.ascontiguousarray(np.asarray(horizon, dtype=np.int32))
        if horizon.shape != (B,):
            raise ValueError("%s must have shape (B,)" % what)
        return horizon

    @staticmethod
    def _check_model(model, B):
        import torch
        if model.dtype != torch.float64 or not model.is_cuda or not model.is_contiguous() or tuple(model.shape) != (_abi.NMODEL, B):
            raise ValueError("model must be a contiguous float64 CUDA tensor of shape (%d, B)" % _abi.NMODEL)

    def _warm_args(self, res, B, device, warm, warm_status, warm_out):
        """The warm arguments of a run()-path call (checked); the "warm" tensor of the result is `warm_out` if given (in-place
        loops pass the `warm` tensor itself), else a new one."""
        import torch
        rows = self.warm_rows()
        if warm is not None and (warm.dtype != torch.float64 or not warm.is_cuda or not warm.is_contiguous() or tuple(warm.shape) != (rows, B)):
            raise ValueError("warm must be a contiguous float64 CUDA tensor of shape (%d, B)" % rows)
        if warm_status is not None and (warm_status.dtype != torch.int32 or not warm_status.is_cuda or tuple(warm_status.shape) != (B,)):
            raise ValueError("warm_status must be an int32 CUDA tensor of shape (B,)")
        if warm_out is not None and (warm_out.dtype != torch.float64 or not warm_out.is_cuda or not warm_out.is_contiguous() or tuple(warm_out.shape) != (rows, B)):
            raise ValueError("warm_out must be a contiguous float64 CUDA tensor of shape (%d, B)" % rows)
        res["warm"] = warm_out if warm_out is not None else torch.empty((rows, B), dtype=torch.float64, device=device)
        return (warm.data_ptr() if warm is not None else None, warm_status.data_ptr() if warm_status is not None else None,
                res["warm"].data_ptr(), B)

    def run_torch(self, pose, ptsx, ptsy, want_traj=False, want_pre=False, stream=None, warm=None, warm_status=None, want_warm=False,
                  warm_opts=None, warm_out=None, status_out=None, model=None):
        """MPC::run() for a batch on the device (src/control/MPC.cpp:327-382): pose [6,B] = x,y,psi,v,steering,
        acceleration; ptsx/ptsy [npts,B] global waypoints, overwritten with the vehicle-frame waypoints as the
        reference does.  Returns out8 [8,B] = {x1,y1,psi1,v1,steer in [-1,1],accel,cte1,epsi1} etc.

        Warm start from the previous call (opt-in, mpc_run_batch_device_warm): ``warm`` / ``warm_status`` are the "warm" and
        "status" tensors that call returned, as in solve_torch; ``want_warm`` (implied by ``warm``) puts "warm" into the result.
        ``warm_out`` / ``status_out``: tensors to write them into -- the ones passed as ``warm`` / ``warm_status`` for a loop in
        place.

        ``model`` [6, B] float64 as in solve_torch (mpc_run_batch_device_model, _warm_model; fp64 handles): every car's own dt, Lf
        and limits, in the solve and in run()'s pre- and post-processing (the speed-table cap, the steering normalisation)."""
        import torch
        B = pose.shape[1]
        npts = ptsx.shape[0]
        for name, t in (("pose", pose), ("ptsx", ptsx), ("ptsy", ptsy)):
            if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or t.shape[1] != B:
                raise ValueError("%s must be a contiguous float64 CUDA tensor [rows, B]" % name)
        dev = pose.device
        res = {"out8": torch.empty((8, B), dtype=torch.float64, device=dev),
               "status": status_out if status_out is not None else torch.empty((B,), dtype=torch.int32, device=dev),
               "iters": torch.empty((B,), dtype=torch.int32, device=dev),
               "traj": torch.empty((2 * self.N, B), dtype=torch.float64, device=dev) if want_traj else None,
               "pre": torch.empty((15, B), dtype=torch.float64, device=dev) if want_pre else None}
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        if model is not None:
            self._check_model(model, B)
        outs = (res["out8"].data_ptr(), res["traj"].data_ptr() if want_traj else None, res["status"].data_ptr(), res["iters"].data_ptr(),
                res["pre"].data_ptr() if want_pre else None, C.c_void_p(s.cuda_stream))
        warm_args = None
        if warm is not None or want_warm or warm_out is not None:
            warm_args = self._warm_args(res, B, dev, warm, warm_status, warm_out) + (C.byref(warm_opts) if warm_opts is not None else None,)
        self._call("mpc_run_batch_device", (B, B, int(npts), pose.data_ptr(), ptsx.data_ptr(), ptsy.data_ptr()), outs,
                   model.data_ptr() if model is not None else None, warm_args)
        return res

    def run_numpy(self, pose, ptsx, ptsy, want_traj=False, warm=None, warm_status=None, want_warm=False, warm_opts=None, model=None):
        """MPC::run() for host arrays (mpc_run_batch_host; B = 1 is what include/mpc_drop_in.hpp's MPC::run calls): pose [6,B],
        ptsx / ptsy [npts,B] global waypoints.  Returns out8, status, iters, pre [15,B], the vehicle-frame waypoints and traj.
        ``warm`` / ``warm_status`` / ``want_warm`` / ``warm_opts``: mpc_run_batch_host_warm, as in run_torch ("warm" in the result).
        ``model`` [6, B]: per-instance dt, Lf and limits as in run_torch (mpc_run_batch_host_model, _host_warm_model)."""
        import numpy as np
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        pose, px, py = f(pose), f(ptsx).copy(), f(ptsy).copy()
        B, npts = pose.shape[1], px.shape[0]
        out8 = np.empty((8, B)); pre = np.empty((15, B)); status = np.empty(B, dtype=np.int32); iters = np.empty(B, dtype=np.int32)
        traj = np.empty((2 * self.N, B)) if want_traj else None
        p = lambda a: a.ctypes.data if a is not None else None
        if model is not None:
            model = f(model)
            if model.shape != (_abi.NMODEL, B):
                raise ValueError("model must have shape (%d, B)" % _abi.NMODEL)
        res = {"out8": out8, "status": status, "iters": iters, "pre": pre, "ptsx": px, "ptsy": py, "traj": traj}
        warm_args = None
        if warm is not None or want_warm:
            rows = self.warm_rows()
            if warm is not None:
                warm = f(warm)
                assert warm.shape == (rows, B)
            if warm_status is not None:
                warm_status = np.ascontiguousarray(warm_status, dtype=np.int32)
            res["warm"] = np.empty((rows, B))
            warm_args = (p(warm), p(warm_status), p(res["warm"]), B, C.byref(warm_opts) if warm_opts is not None else None)
        self._call("mpc_run_batch_host", (B, B, int(npts), p(pose), p(px), p(py)), (p(out8), p(traj), p(status), p(iters), p(pre)),
                   p(model), warm_args)
        return res

    def telemetry_torch(self, tel, ptsx, ptsy, extra_latency=0.0, want_out8=False, stream=None, warm=None, warm_status=None,
                        want_warm=False, warm_opts=None, warm_out=None, status_out=None, model=None, comp=None, horizon=None):
        """The telemetry handler around run() (src/mpc_main.cpp:126-174) for a batch: tel [6,B] = x, y, psi,
        speed [mph], steering_angle (simulator sign), previous throttle.  Returns cmd [2,B] = (steering_angle,
        throttle) of the reply, status, and optionally run()'s 8-vector.  The warm arguments are run_torch's
        (mpc_telemetry_batch_device_warm).  ``model`` [6, B] as in run_torch (mpc_telemetry_batch_device_model, _warm_model): each
        car's own Lf in the latency compensation and its own limits in the steering normalisation and the throttle.
        ``comp`` [B] float64 (mpc_telemetry_batch_device_latency; fp64 handles): the seconds every instance compensates for, in
        the place of the handle's latency_ms / lookahead and of ``extra_latency``; 0: no compensation.  Always the warm form of the call.
        ``horizon`` [B] int32 (mpc_telemetry_batch_device_horizon; fp64 handles, max_soc = 0): every instance's own N, 3 .. the handle's,
        as in solve_torch; the lane kernel's HORIZON build at every B.  With or without ``comp`` and ``model``; always the warm form."""
        import torch
        B = tel.shape[1]
        npts = ptsx.shape[0]
        for name, t in (("tel", tel), ("ptsx", ptsx), ("ptsy", ptsy)):
            if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or t.shape[1] != B:
                raise ValueError("%s must be a contiguous float64 CUDA tensor [rows, B]" % name)
        dev = tel.device
        res = {"cmd": torch.empty((2, B), dtype=torch.float64, device=dev),
               "status": status_out if status_out is not None else torch.empty((B,), dtype=torch.int32, device=dev),
               "out8": torch.empty((8, B), dtype=torch.float64, device=dev) if want_out8 else None}
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        if model is not None:
            self._check_model(model, B)
        outs = (res["cmd"].data_ptr(), res["out8"].data_ptr() if want_out8 else None, res["status"].data_ptr(), C.c_void_p(s.cuda_stream))
        warm_args = None
        if warm is not None or want_warm or warm_out is not None:
            warm_args = self._warm_args(res, B, dev, warm, warm_status, warm_out) + (C.byref(warm_opts) if warm_opts is not None else None,)
        if horizon is not None:
            self._check_horizon(horizon, B)
        if comp is not None or horizon is not None:
            if comp is not None and (comp.dtype != torch.float64 or not comp.is_cuda or not comp.is_contiguous() or tuple(comp.shape) != (B,)):
                raise ValueError("comp must be a contiguous float64 CUDA tensor of shape (B,)")
            if warm_args is None:
                warm_args = (None, None, None, 0, C.byref(warm_opts) if warm_opts is not None else None)
            name = "mpc_telemetry_batch_device" + ("_horizon" if horizon is not None else "_latency")
            hz = (horizon.data_ptr(),) if horizon is not None else ()
            check(getattr(library(), name)(self._h, B, B, int(npts), tel.data_ptr(), float(extra_latency), comp.data_ptr() if comp is not None else None,
                                           ptsx.data_ptr(), ptsy.data_ptr(), model.data_ptr() if model is not None else None, *hz,
                                           *warm_args, *outs), name)
            return res
        self._call("mpc_telemetry_batch_device", (B, B, int(npts), tel.data_ptr(), float(extra_latency), ptsx.data_ptr(), ptsy.data_ptr()),
                   outs, model.data_ptr() if model is not None else None, warm_args)
        return res

    def telemetry_numpy(self, tel, ptsx, ptsy, extra_latency=0.0, model=None, comp=None, warm_opts=None, horizon=None):
        """telemetry_torch for host arrays through the _latency form (mpc_telemetry_batch_host_latency; without ``comp`` that is
        mpc_telemetry_batch_host_warm_model, started cold): one copy in, the kernels, one copy out; synchronises.  Returns "cmd" [2, B]
        and "status".  ``model`` [6, B], ``comp`` [B]: as in telemetry_torch; ``horizon`` [B] int32: mpc_telemetry_batch_host_horizon."""
        f = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64)) if a is not None else None
        tel, ptsx, ptsy, model, comp = f(tel), f(ptsx), f(ptsy), f(model), f(comp)
        B, npts = tel.shape[1], ptsx.shape[0]
        if tel.shape != (6, B) or ptsx.shape != (npts, B) or ptsy.shape != (npts, B):
            raise ValueError("tel [6, B], ptsx and ptsy [npts, B]")
        if model is not None and model.shape != (_abi.NMODEL, B):
            raise ValueError("model must have shape (%d, B)" % _abi.NMODEL)
        if comp is not None and comp.shape != (B,):
            raise ValueError("comp must have shape (B,)")
        res = {"cmd": np.empty((2, B)), "status": np.empty(B, dtype=np.int32)}
        p = lambda a: a.ctypes.data if a is not None else None
        hz = ()
        if horizon is not None:
            horizon = np.ascontiguousarray(np.asarray(horizon))
            if horizon.dtype != np.int32 or horizon.shape != (B,):
                raise ValueError("horizon must be an int32 array of shape (B,)")
            hz = (p(horizon),)
        name = "mpc_telemetry_batch_host" + ("_horizon" if horizon is not None else "_latency")
        check(getattr(library(), name)(self._h, B, B, int(npts), p(tel), float(extra_latency), p(comp), p(ptsx), p(ptsy), p(model), *hz,
                                       None, None, None, 0, C.byref(warm_opts) if warm_opts is not None else None,
                                       p(res["cmd"]), p(res["status"])), name)
        return res

    def rollout_torch(self, state, coeffs, yaw_lo, yaw_hi, steps, weights=None, want_hist=True, stream=None, warm_start=False,
                      warm_opts=None, fused=False, model=None, horizon=None):
        """Closed loop of src/test.cpp:79-111 for a batch: `steps` cold-started solves, each fed with the previous
        step-1 state.  `state` [6,B] is advanced in place.  Returns hist [steps,9,B], worst status, summed iters.
        ``warm_start``: every step after the first starts from the solution of the step before
        (mpc_rollout_batch_device_warm; same NLP, fewer iterations).
        ``fused``: the same rollout in one launch, every car advancing on its own (mpc_rollout_batch_device_fused; bitwise the
        same results, rollout_fused_info() tells whether the fused kernel or the stepwise loop ran).
        ``model`` [6, B]: every car's own dt, Lf and limits, as in solve_torch -- with every combination of ``warm_start`` and
        ``fused`` (mpc_rollout_batch_device_model, _warm_model, _fused_model).
        ``horizon`` [B] int32: every car's own N as in solve_torch, with every combination as well (mpc_rollout_batch_device_horizon,
        _warm_horizon, _fused_horizon; the one launch runs at every B)."""
        import torch
        B = state.shape[1]
        dev = state.device
        for name, t, shape in (("state", state, (6, B)), ("coeffs", coeffs, (5, B)), ("yaw_lo", yaw_lo, (B,)), ("yaw_hi", yaw_hi, (B,))):
            if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shape:
                raise ValueError("%s must be a contiguous float64 CUDA tensor of shape %s" % (name, shape))
        res = {"hist": torch.empty((steps, _abi.NOUT, B), dtype=torch.float64, device=dev) if want_hist else None,
               "status": torch.empty((B,), dtype=torch.int32, device=dev),
               "iters": torch.empty((B,), dtype=torch.int32, device=dev)}
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        if model is not None:
            self._check_model(model, B)
        if horizon is not None:
            self._check_horizon(horizon, B)
        head = (B, B, int(steps), state.data_ptr(), coeffs.data_ptr(), yaw_lo.data_ptr(), yaw_hi.data_ptr(),
                weights.data_ptr() if weights is not None else None)
        outs = (res["hist"].data_ptr() if want_hist else None, res["status"].data_ptr(), res["iters"].data_ptr(), C.c_void_p(s.cuda_stream))
        opts = C.byref(warm_opts) if warm_opts is not None else None
        m = model.data_ptr() if model is not None else None
        hz = horizon.data_ptr() if horizon is not None else None
        if fused:      # (two forms: warm_start and opts are arguments of both)
            self._call("mpc_rollout_batch_device_fused", head, (1 if warm_start else 0, opts) + outs, m, horizon=hz)
        else:
            self._call("mpc_rollout_batch_device", head, outs, m, (opts,) if warm_start else None, horizon=hz)
        return res

    # -- track driving (include/mpc_amd_drive.h) --------------------------------
    def drive_opts(self, **overrides):
        """This handle's MpcDriveOpts defaults (mpc_drive_opts_default), with keyword overrides."""
        return _abi.drive_opts_default(self.params, **overrides)

    def drive_plant_default(self, B=None, model=None):
        """The default plant column of this handle (mpc_drive_plant_default: Lf, 1, 0, 6, 50, 0), or with B the array [6, B] of it --
        row 0 from ``model``'s Lf row if one is given: the ``plant=`` under which a drive is the drive without one."""
        return _abi.drive_plant_default(self.params, B, model)

    @staticmethod
    def drive_noise_default(B=None, seeds=None):
        """The zero noise column (mpc_drive_noise_default), or with B / seeds the array [7, B] of it with the seeds in row 0: the
        ``noise=`` under which a drive is the drive without one, ready to have its sigma rows set (_abi.NOISE_*)."""
        return _abi.drive_noise_default(B, seeds)

    def drive_torch(self, car, track_x, track_y, steps, weights=None, opts=None, warm_opts=None, want_hist=True, fused=False, stream=None,
                    model=None, latency=None, horizon=None, plant=None, budget=None, noise=None, seen=False):
        """Drive B cars along a cyclic track for `steps` telemetry messages on the device (mpc_drive_batch_device): per message the
        waypoint window at the car's position, the telemetry handler (cold, or warm with opts.warm_start) and the plant -- the
        reference's own kinematic model, not the simulator.  car [6, B] = x, y, psi, speed [mph], steering_angle, throttle is advanced
        in place; track_x / track_y [n] float64 CUDA tensors; weights [12, B] or None; opts: an MpcDriveOpts (None: drive_opts()).
        Returns a dict of tensors: "car" (the same tensor), "summary" [8, B] (rows _abi.DRIVE_SUM_*), "hist" [steps, 13, B] (rows
        _abi.DRIVE_REC_*) or None, "status" (worst), "iters" (summed).  ``fused``: the same drive in one launch, every car advancing on
        its own (mpc_drive_batch_device_fused; bitwise the same results, drive_info() tells whether the one launch or the stepwise loop
        ran).  ``model`` [6, B] float64 as in telemetry_torch (mpc_drive_batch_device_model, _fused_model; fp64 handles): every car's own
        dt, Lf and limits, in the handler and in the plant (Lf in the heading update, max_steering in the steering angle in force) --
        one call answers "how fast can this tuning go round the track" with a row of max_speed values.
        ``latency`` [3, B] float64 (mpc_drive_batch_device_latency, _fused_latency; rows _abi.LATENCY_*): every car's own compensated
        time [s] in the handler and its own sub_old / sub_new in the plant (scenarios.latency_grid builds a stale-time x compensation
        grid) -- one call answers "how much delay does this tuning survive, compensated or not".
        ``horizon`` [B] int32 (mpc_drive_batch_device_horizon, _fused_horizon; fp64 handles, max_soc = 0): every car's own N, 3 .. the
        handle's, in the handler's solve; with ``model``'s dt row an N x dt grid is the cars of one call.  The lane kernel at every B,
        the one launch included; sort the cars by horizon (a wave's pass lasts as long as its longest one).
        ``plant`` [6, B] float64 (mpc_drive_batch_device_plant, _fused_plant; rows _abi.PLANT_*): the values every car is MOVED with --
        Lf, steering gain and bias, acceleration gain, drag speed, side drift -- while its handler goes on believing ``model``: one call
        answers "how wrong may the model be before the car leaves the road".  drive_plant_default(B, model) is the column that changes
        nothing.
        ``budget`` [B] int32 (mpc_drive_batch_device_budget, _fused_budget; fp64 handles, max_soc = 0): the interior-point iterations
        every car's handler may spend per message, over all attempts of its solve -- the reference's solve deadline (ipoptTimeout),
        counted in iterations.  A message that uses its budget up drives the car with the current iterate (status MAXITER) and, with
        opts.warm_start, hands that iterate to the next message: one call answers "how much solver work per message does this tuning
        need to stay on the road, cold or warm-started".  The lane kernel at every B, like ``horizon``.
        ``noise`` [7, B] float64 (mpc_drive_batch_device_noise, _fused_noise; rows _abi.NOISE_*: seed, then the sigmas of the reported
        position, heading and speed, of a per-message steering offset and side gust, and the probability that a reply is lost): every
        car's own seeded sensor, actuator and link noise -- a Monte-Carlo over noisy drives is seeds x noise levels as the columns of
        one call.  The draws depend on (seed, message index) alone.  drive_noise_default(B, seeds) is the column that changes nothing.
        ``seen`` = True: the result has "seen" [steps, 4, B], what the handler was told (x, y, psi, speed) at every message (None
        otherwise).  Neither changes which kernels run."""
        import torch
        B = car.shape[1]
        if noise is not None and (noise.dtype != torch.float64 or not noise.is_cuda or not noise.is_contiguous() or
                                  tuple(noise.shape) != (_abi.NNOISE, B)):
            raise ValueError("noise must be a contiguous float64 CUDA tensor of shape (%d, B)" % _abi.NNOISE)
        if budget is not None:
            self._check_horizon(budget, B, "budget")
        if plant is not None and (plant.dtype != torch.float64 or not plant.is_cuda or not plant.is_contiguous() or
                                  tuple(plant.shape) != (_abi.NPLANT, B)):
            raise ValueError("plant must be a contiguous float64 CUDA tensor of shape (%d, B)" % _abi.NPLANT)
        if model is not None:
            self._check_model(model, B)
        if horizon is not None:
            self._check_horizon(horizon, B)
        if latency is not None and (latency.dtype != torch.float64 or not latency.is_cuda or not latency.is_contiguous() or
                                    tuple(latency.shape) != (_abi.NLATENCY, B)):
            raise ValueError("latency must be a contiguous float64 CUDA tensor of shape (%d, B)" % _abi.NLATENCY)
        dev = car.device
        n = int(track_x.shape[0])
        for name, t, shape in (("car", car, (6, B)), ("track_x", track_x, (n,)), ("track_y", track_y, (n,)), ("weights", weights, (_abi.NW, B))):
            if t is not None and (t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shape):
                raise ValueError("%s must be a contiguous float64 CUDA tensor of shape %s" % (name, shape))
        res = {"car": car, "summary": torch.empty((_abi.DRIVE_NSUM, B), dtype=torch.float64, device=dev),
               "hist": torch.empty((steps, _abi.DRIVE_REC, B), dtype=torch.float64, device=dev) if want_hist else None,
               "status": torch.empty((B,), dtype=torch.int32, device=dev), "iters": torch.empty((B,), dtype=torch.int32, device=dev),
               "seen": torch.empty((steps, 4, B), dtype=torch.float64, device=dev) if seen else None}
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        name = ("mpc_drive_batch_device_fused" if fused else "mpc_drive_batch_device") + (
            "_budget" if budget is not None else "_plant" if plant is not None else "_horizon" if horizon is not None else
            "_latency" if latency is not None else "_model" if model is not None else "")
        extra = (model.data_ptr(),) if model is not None else ()
        if latency is not None or horizon is not None:
            extra = (model.data_ptr() if model is not None else None,) + ((horizon.data_ptr(),) if horizon is not None else ()) + (
                latency.data_ptr() if latency is not None else None,)
        if plant is not None:
            extra = tuple(t.data_ptr() if t is not None else None for t in (model, horizon, latency, plant))
        if budget is not None:
            extra = tuple(t.data_ptr() if t is not None else None for t in (model, horizon, budget, latency, plant))
        seen_arg = ()
        if noise is not None or seen:
            name = ("mpc_drive_batch_device_fused" if fused else "mpc_drive_batch_device") + "_noise"
            extra = tuple(t.data_ptr() if t is not None else None for t in (model, horizon, budget, latency, plant, noise))
            seen_arg = (res["seen"].data_ptr() if seen else None,)
        check(getattr(library(), name)(self._h, B, B, int(steps), car.data_ptr(), track_x.data_ptr(), track_y.data_ptr(), n,
                                               weights.data_ptr() if weights is not None else None, *extra,
                                               C.byref(opts) if opts is not None else None, C.byref(warm_opts) if warm_opts is not None else None,
                                               res["summary"].data_ptr(), res["hist"].data_ptr() if want_hist else None, *seen_arg,
                                               res["status"].data_ptr(), res["iters"].data_ptr(), C.c_void_p(s.cuda_stream)),
              name)
        return res

    def drive_numpy(self, car, track_x, track_y, steps, weights=None, opts=None, warm_opts=None, want_hist=True, model=None, latency=None, horizon=None,
                    plant=None, budget=None, noise=None, seen=False):
        """drive_torch for host arrays (mpc_drive_batch_host): one copy in, the loop, one copy out; synchronises.  `car` is copied:
        the cars after the last step are "car" of the result.  ``model`` [6, B]: as in drive_torch (mpc_drive_batch_host_model); ``latency`` [3, B]: as in
        drive_torch (mpc_drive_batch_host_latency); ``horizon`` [B] int32: as in drive_torch (mpc_drive_batch_host_horizon); ``plant`` [6, B]: as in
        drive_torch (mpc_drive_batch_host_plant); ``budget`` [B] int32: as in drive_torch (mpc_drive_batch_host_budget); ``noise`` [7, B] and ``seen``: as in
        drive_torch (mpc_drive_batch_host_noise)."""
        f = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64)) if a is not None else None
        car, tx, ty, weights = f(car).copy(), f(track_x), f(track_y), f(weights)
        B, n = car.shape[1], tx.shape[0]
        assert car.shape == (6, B) and ty.shape == (n,) and (weights is None or weights.shape == (_abi.NW, B))
        if model is not None:
            model = f(model)
            if model.shape != (_abi.NMODEL, B):
                raise ValueError("model must have shape (%d, B)" % _abi.NMODEL)
        res = {"car": car, "summary": np.empty((_abi.DRIVE_NSUM, B)), "hist": np.empty((steps, _abi.DRIVE_REC, B)) if want_hist else None,
               "status": np.empty(B, dtype=np.int32), "iters": np.empty(B, dtype=np.int32), "seen": np.empty((steps, 4, B)) if seen else None}
        p = lambda a: a.ctypes.data if a is not None else None
        if noise is not None:
            noise = np.asarray(noise)
            if noise.dtype != np.float64 or noise.shape != (_abi.NNOISE, B):
                raise ValueError("noise must be a float64 array of shape (%d, B)" % _abi.NNOISE)
            noise = np.ascontiguousarray(noise)
        if latency is not None:
            latency = f(latency)
            if latency.shape != (_abi.NLATENCY, B):
                raise ValueError("latency must have shape (%d, B)" % _abi.NLATENCY)
        if horizon is not None:
            horizon = np.ascontiguousarray(np.asarray(horizon))
            if horizon.dtype != np.int32 or horizon.shape != (B,):
                raise ValueError("horizon must be an int32 array of shape (B,)")
        name = "mpc_drive_batch_host" + ("_horizon" if horizon is not None else "_latency" if latency is not None else "_model" if model is not None else "")
        extra = (p(model), p(latency)) if latency is not None else ((p(model),) if model is not None else ())
        if horizon is not None:
            extra = (p(model), p(horizon), p(latency))
        if plant is not None:
            plant = f(plant)
            if plant.shape != (_abi.NPLANT, B):
                raise ValueError("plant must have shape (%d, B)" % _abi.NPLANT)
            name, extra = "mpc_drive_batch_host_plant", (p(model), p(horizon), p(latency), p(plant))
        if budget is not None:
            budget = np.ascontiguousarray(np.asarray(budget))
            if budget.dtype != np.int32 or budget.shape != (B,):
                raise ValueError("budget must be an int32 array of shape (B,)")
            name, extra = "mpc_drive_batch_host_budget", (p(model), p(horizon), p(budget), p(latency), p(plant))
        seen_arg = ()
        if noise is not None or seen:
            name, extra, seen_arg = "mpc_drive_batch_host_noise", (p(model), p(horizon), p(budget), p(latency), p(plant), p(noise)), (p(res["seen"]),)
        check(getattr(library(), name)(self._h, B, B, int(steps), p(car), p(tx), p(ty), n, p(weights), *extra,
                                       C.byref(opts) if opts is not None else None, C.byref(warm_opts) if warm_opts is not None else None,
                                       p(res["summary"]), p(res["hist"]), *seen_arg, p(res["status"]), p(res["iters"])), name)
        return res

    def drive_info(self):
        a = (C.c_int64 * 2)()
        check(library().mpc_drive_info(self._h, a), "mpc_drive_info")
        return {"fused_launches": int(a[0]), "stepwise_loops": int(a[1])}

    # -- host path (numpy arrays; copies through PCIe) ------------------------
    def solve_numpy(self, state, coeffs, yaw_lo, yaw_hi, weights=None, want_traj=False, model=None, horizon=None, traj_out=None):
        """Host arrays through mpc_solve_batch_host (float64), or mpc_solve_batch_host_f32 for an MPC_PRECISION_F32 handle.
        ``model`` [6, B] float64: per-instance dt, Lf and limits as in solve_torch (mpc_solve_batch_host_model, fp64 handles).
        ``horizon`` [B] int32: per-instance N as in solve_torch (mpc_solve_batch_host_horizon); the rows of "traj" that an instance
        does not write hold NaN, or what ``traj_out`` [2N, B] (written in place) held."""
        dt = np.float32 if self.f32 else np.float64
        f = lambda a: np.ascontiguousarray(np.asarray(a, dtype=dt))
        state, coeffs, yaw_lo, yaw_hi = f(state), f(coeffs), f(yaw_lo), f(yaw_hi)
        B = state.shape[1]
        assert state.shape == (6, B) and coeffs.shape == (5, B) and yaw_lo.shape == (B,) and yaw_hi.shape == (B,)
        if weights is not None:
            weights = f(weights)
            assert weights.shape == (_abi.NW, B)
        out = np.empty((_abi.NOUT, B), dtype=dt); status = np.empty(B, dtype=np.int32); iters = np.empty(B, dtype=np.int32)
        traj = self._host_traj(B, dt, want_traj, horizon, traj_out)
        p = lambda a: a.ctypes.data if a is not None else None
        head = (B, B, p(state), p(coeffs), p(yaw_lo), p(yaw_hi), p(weights))
        outs = (p(out), p(traj), p(status), p(iters))
        if model is not None:
            model = np.ascontiguousarray(np.asarray(model, dtype=np.float64))
            assert model.shape == (_abi.NMODEL, B)
        if horizon is not None:
            horizon = self._host_horizon(horizon, B)
        if self.f32 and model is None and horizon is None:
            check(library().mpc_solve_batch_host_f32(self._h, *head, *outs), "mpc_solve_batch_host")
        else:
            self._call("mpc_solve_batch_host", head, outs, p(model), horizon=p(horizon))
        return {"out": out, "status": status, "iters": iters, "traj": traj}

    def _host_traj(self, B, dt, want_traj, horizon, traj_out):
        if traj_out is not None:
            assert traj_out.shape == (2 * self.N, B) and traj_out.dtype == dt and traj_out.flags.c_contiguous
            return traj_out
        if not want_traj:
            return None
        return np.full((2 * self.N, B), np.nan, dtype=dt) if horizon is not None else np.empty((2 * self.N, B), dtype=dt)

    def solve_numpy_warm(self, state, coeffs, yaw_lo, yaw_hi, warm=None, warm_status=None, weights=None, want_traj=False, warm_opts=None,
                         model=None, horizon=None, traj_out=None, warm_out=None, budget=None):
        """Host arrays through mpc_solve_batch_host_warm (fp64 handles): like solve_numpy, with "warm" [warm_rows(), B] in the
        result; ``warm`` / ``warm_status``: that array and the status of an earlier call.  ``model`` [6, B]: as in solve_numpy
        (mpc_solve_batch_host_warm_model).  ``horizon`` [B] int32: as in solve_numpy (mpc_solve_batch_host_warm_horizon): an instance
        reads and writes the records of its own n-1 stages; the rows of "warm" behind them hold NaN, or what ``warm_out``
        [warm_rows(), B] (written in place; may be ``warm`` itself) held.  ``budget`` [B] int32: as in solve_torch
        (mpc_solve_batch_host_budget)."""
        f = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64))
        state, coeffs, yaw_lo, yaw_hi = f(state), f(coeffs), f(yaw_lo), f(yaw_hi)
        B = state.shape[1]
        rows = self.warm_rows()
        if warm is not None:
            warm = f(warm)
            assert warm.shape == (rows, B)
        if warm_status is not None:
            warm_status = np.ascontiguousarray(warm_status, dtype=np.int32)
        if weights is not None:
            weights = f(weights)
        out = np.empty((_abi.NOUT, B)); status = np.empty(B, dtype=np.int32); iters = np.empty(B, dtype=np.int32)
        traj = self._host_traj(B, np.float64, want_traj, horizon, traj_out)
        if warm_out is not None:
            assert warm_out.shape == (rows, B) and warm_out.dtype == np.float64 and warm_out.flags.c_contiguous
            wout = warm_out
        else:
            wout = np.full((rows, B), np.nan) if horizon is not None else np.empty((rows, B))
        p = lambda a: a.ctypes.data if a is not None else None
        if model is not None:
            model = f(model)
            assert model.shape == (_abi.NMODEL, B)
        if horizon is not None:
            horizon = self._host_horizon(horizon, B)
        if budget is not None:
            budget = self._host_horizon(budget, B, "budget")
        self._call("mpc_solve_batch_host", (B, B, p(state), p(coeffs), p(yaw_lo), p(yaw_hi), p(weights)), (p(out), p(traj), p(status), p(iters)),
                   p(model), (p(warm), p(warm_status), p(wout), B, C.byref(warm_opts) if warm_opts is not None else None), horizon=p(horizon),
                   budget=p(budget))
        return {"out": out, "status": status, "iters": iters, "traj": traj, "warm": wout}

    # -- the certificate of a stored point (include/mpc_amd_certify.h) ----------
    def certify_torch(self, state, coeffs, yaw_lo, yaw_hi, sol, weights=None, model=None, horizon=None, stream=None):
        """IPOPT's final error summary for stored primal-dual points (mpc_certify_batch_device; fp64 handles): ``sol``
        [warm_rows(), B] float64 is the "warm" tensor of any warm-capable call (a cold one with want_warm=True gives the solution
        of a solve), read as it is; the other arguments are those of the solve that wrote it.  One launch on ``stream``, nothing is
        solved.  Returns {"cert": [NCERT, B] float64 (rows _abi.CERT_*), "verdict": [B] int32 (_abi.CERT_VERDICT_NAMES)}."""
        import torch
        B = state.shape[1]
        for name, t, shape in (("state", state, (6, B)), ("coeffs", coeffs, (5, B)), ("yaw_lo", yaw_lo, (B,)), ("yaw_hi", yaw_hi, (B,)),
                               ("sol", sol, (self.warm_rows(), B)), ("weights", weights, (_abi.NW, B))):
            if t is not None and (t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shape):
                raise ValueError("%s must be a contiguous float64 CUDA tensor of shape %s" % (name, shape))
        if model is not None:
            self._check_model(model, B)
        if horizon is not None:
            self._check_horizon(horizon, B)
        s = stream if stream is not None else torch.cuda.current_stream(state.device)
        res = {"cert": torch.empty((_abi.NCERT, B), dtype=torch.float64, device=state.device),
               "verdict": torch.empty((B,), dtype=torch.int32, device=state.device)}
        p = lambda t: t.data_ptr() if t is not None else None
        check(library().mpc_certify_batch_device(self._h, B, B, p(state), p(coeffs), p(yaw_lo), p(yaw_hi), p(weights), p(model), p(horizon),
                                                 p(sol), B, p(res["cert"]), p(res["verdict"]), C.c_void_p(s.cuda_stream)),
              "mpc_certify_batch_device")
        return res

    def certify_numpy(self, state, coeffs, yaw_lo, yaw_hi, sol, weights=None, model=None, horizon=None):
        """certify_torch for host arrays (mpc_certify_batch_host): one copy in, the launch, one copy out; synchronises."""
        f = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64)) if a is not None else None
        state, coeffs, yaw_lo, yaw_hi, sol, weights, model = f(state), f(coeffs), f(yaw_lo), f(yaw_hi), f(sol), f(weights), f(model)
        B = state.shape[1]
        assert state.shape == (6, B) and coeffs.shape == (5, B) and yaw_lo.shape == (B,) and yaw_hi.shape == (B,)
        assert sol.shape == (self.warm_rows(), B) and (weights is None or weights.shape == (_abi.NW, B))
        assert model is None or model.shape == (_abi.NMODEL, B)
        if horizon is not None:
            horizon = self._host_horizon(horizon, B)
        cert = np.empty((_abi.NCERT, B)); verdict = np.empty(B, dtype=np.int32)
        p = lambda a: a.ctypes.data if a is not None else None
        check(library().mpc_certify_batch_host(self._h, B, B, p(state), p(coeffs), p(yaw_lo), p(yaw_hi), p(weights), p(model), p(horizon),
                                               p(sol), B, p(cert), p(verdict)), "mpc_certify_batch_host")
        return {"cert": cert, "verdict": verdict}

    # -- deferred tails (MpcParams.tail_cut > 0, include/mpc_amd.h) -------------
    def last_batch_id(self):
        return int(library().mpc_last_batch_id(self._h))

    def tail_wait(self, batch_id=0):
        """Block until batch `batch_id` is final (0: every batch issued so far)."""
        check(library().mpc_tail_wait(self._h, int(batch_id)), "mpc_tail_wait")

    def tail_poll(self, batch_id):
        """True if batch `batch_id` is final (one non-blocking turn of the pump that starts tail slices)."""
        r = library().mpc_tail_poll(self._h, int(batch_id))
        if r < 0:
            check(r, "mpc_tail_poll")
        return bool(r)

    def tail_stream_wait(self, batch_id, stream):
        check(library().mpc_tail_stream_wait(self._h, int(batch_id), C.c_void_p(stream.cuda_stream)), "mpc_tail_stream_wait")

    def tail_flush(self):
        check(library().mpc_tail_flush(self._h), "mpc_tail_flush")

    def tail_pending(self, batch_id):
        n = C.c_int64(0)
        check(library().mpc_tail_pending(self._h, int(batch_id), C.byref(n)), "mpc_tail_pending")
        return int(n.value)

    def tail_info(self):
        a = (C.c_int64 * 13)()
        check(library().mpc_tail_info(self._h, a), "mpc_tail_info")
        return {"batches_deferred": int(a[0]), "tail_launches": int(a[1]), "ring": int(a[2]), "capacity_per_batch": int(a[3]),
                "waves_per_tail_launch": int(a[4]), "tail_stream_high_priority": bool(a[5]), "tail_streams": int(a[6]),
                "batches_not_deferred_survivors_full": int(a[7]), "passes_per_slice": int(a[8]), "survivors": int(a[9]),
                "tail_cut_in_use": int(a[10]), "deferred_share": (int(a[11]) / 65536.0 if a[11] >= 0 else None), "queue_overflows": int(a[12])}

    def take_order_info(self):
        a = (C.c_int64 * 2)()
        check(library().mpc_take_order_info(self._h, a), "mpc_take_order_info")
        return {"launches_in_key_order": int(a[0]), "mode": int(a[1])}

    def rollout_fused_info(self):
        a = (C.c_int64 * 2)()
        check(library().mpc_rollout_fused_info(self._h, a), "mpc_rollout_fused_info")
        return {"fused_launches": int(a[0]), "stepwise_loops": int(a[1])}

    def synchronize(self):
        check(library().mpc_synchronize(self._h), "mpc_synchronize")

    def stats(self) -> MpcBatchStats:
        st = MpcBatchStats()
        check(library().mpc_get_stats(self._h, C.byref(st)), "mpc_get_stats")
        return st
