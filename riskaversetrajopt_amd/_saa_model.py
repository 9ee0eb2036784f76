"""What ``drone_risk.Model`` and ``driving.Model`` share: the lazily filled state, the parameter-struct cache, control
upload and buffer reuse, the statistics plumbing around the rollout / linearize launches, the re-tiled noise cache and the
glue of the reduced SCP.  Everything about layouts and every launch stays in the two facades; a subclass sets a handful of
class attributes and four small methods (``_params_key``, ``_params_build``, ``_batch_shape``, ``_tile_noise``)."""
import numpy as np
import torch

from . import _lib, cvar_cuts, stats


class SaaModel:
    N_U = None          # controls per step
    N_NOISE = None      # noise rows per step of the kernel layout dW [S][N_NOISE][ld]
    PARAMS = None       # the ctypes struct of the system's kernels (_lib.DroneParams / _lib.CarParams)
    KAPPA = 1.0         # scale of the constraint rows in the reference's QP (certificate.certify)
    CUT_ROWS = 1        # constraint rows per sample and step (R of the cut solver)
    CUT_RHS0 = 0.0      # right-hand side of the baseline method's max-row constraint (cvar_cuts.py)
    RCOST = None        # the control cost matrix R of the system's parameter module

    TILED_NOISE = True        # (class-level switch for A/B runs and the equality test)

    def _init_state(self):
        """Every attribute that is filled on first use, at its empty value."""
        self._group, self._world = None, 1                      # shard()
        self._cut_solver = self._gen_buffers = self._lin_buffers = self._define_host = None     # solve_reduced
        self._native_define = self._rollout_params = None       # the native define / SCP loops
        self._fast = None                                       # get_constraints_coeffs' cached sparsity pattern
        self._dW_tiled_cache = None                             # _tiled_noise
        self._noise_seed = self._sampler_dt = None              # from_device(dW=None, noise_seed=...)
        self._params_cache = {}

    def _drop_solver_state(self):
        """Forget what a ``solve_reduced`` left behind (the cut solver and the buffers it linearized into)."""
        self._cut_solver = self._gen_buffers = self._lin_buffers = self._define_host = None

    # ---- layout helpers (drone_risk.py:95-120, driving.py:122-143) ---------
    def convert_us_vec_to_us_mat(self, us_vec):
        return np.reshape(np.asarray(us_vec), (self.N_U, self.S), 'F').T.copy()

    def convert_us_mat_to_us_jaxvec(self, us_mat):
        return np.reshape(np.asarray(us_mat), (self.S * self.N_U), 'C')

    # ---- plumbing ----------------------------------------------------------
    def _params(self, *args):
        """a fresh parameter struct for this Model (callers set the stats_* fields on it): a copy of a template built once
        per ``_params_key(*args)`` -- ~40 ctypes field stores cost 15-20 us, more than a small kernel"""
        key = self._params_key(*args)
        cache = self._params_cache
        t = cache.get(key)
        if t is None:
            if len(cache) > 64:
                cache.clear()
            t = cache[key] = self._params_build(*args)
        return self.PARAMS.from_buffer_copy(t)

    def _us_device(self, us_mat):
        if isinstance(us_mat, torch.Tensor) and us_mat.is_cuda:
            us = us_mat.float().contiguous()
        else:
            us = torch.as_tensor(np.ascontiguousarray(np.asarray(us_mat), dtype=np.float32), device=self.device)
        if tuple(us.shape) != (self.S, self.N_U):
            raise ValueError(f"us_mat must be ({self.S},{self.N_U}), got {tuple(us.shape)}")
        return us

    def _us_batch_device(self, us_batch):
        if isinstance(us_batch, torch.Tensor) and us_batch.is_cuda:
            us = us_batch.float().contiguous()
        else:
            us = torch.as_tensor(np.ascontiguousarray(np.asarray(us_batch), dtype=np.float32), device=self.device)
        if us.dim() != 3 or tuple(us.shape[1:]) != (self.S, self.N_U):
            raise ValueError(f"us_batch must be (K,{self.S},{self.N_U}), got {tuple(us.shape)}")
        return us

    def _empty(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    def _reuse(self, o, key, shape, alloc=None):
        """a buffer of an earlier call is reused only if it has exactly the shape this launch writes (``o`` may
        come from another batch size or S: the kernels would write past a smaller buffer)"""
        t = o.get(key)
        if t is not None and tuple(t.shape) == tuple(shape) and t.dtype == torch.float32 and t.is_contiguous():
            return t
        return self._empty(*shape) if alloc is None else alloc()

    # ---- statistics around the rollout / linearize launches ----------------
    @staticmethod
    def _request_stats(p, stats_request):
        """``stats_request`` = (workspace, record, alpha[, in_launch]) of ``eval_device`` into the params of its launch"""
        stats.request_in_launch(p, *stats_request[:3], flags=(stats.STATS_IN_LAUNCH if (len(stats_request) > 3 and
                                                                                         stats_request[3]) else 0))

    def mc_step_device(self, us_mat, alpha=None, out=None, workspace=None, stats_out=None, inputs=None, in_launch=False):
        """One Monte-Carlo validation step on the device (drone_risk.py:711-714, driving.py:630-671: rollout -> max over
        the constraint rows -> fraction satisfied / VaR / AVaR) as ONE library call -- for small batches one launch.
        -> (Z [M], record double[N_STATS]), device tensors; ``out`` / ``workspace`` / ``stats_out`` are reused when given
        (a captured step must pass them)."""
        alpha = self.alpha if alpha is None else alpha
        if workspace is None:
            workspace = stats.new_workspace(self._batch_shape(inputs)[0], self.device)
        if stats_out is None:
            stats_out = torch.empty(stats.N_STATS, dtype=torch.float64, device=self.device)
        Z, _, _ = self.eval_device(us_mat, inputs=inputs, out=out, stats_request=(workspace, stats_out, alpha, in_launch))
        return Z, stats_out

    def _batch_buffers(self, o, K, M, ld, want_stats, workspace):
        """-> (Z [K][ld], records [K][N_STATS] or None, workspace or None) of ``eval_batch_device``, kept in ``o``"""
        Z = o.get("_Zb")
        if Z is None or tuple(Z.shape) != (K, ld):
            Z = self._empty(K, ld)
        rec = None
        if want_stats:
            rec = o.get("_recb")
            if rec is None or tuple(rec.shape) != (K, stats.N_STATS):
                rec = torch.empty((K, stats.N_STATS), dtype=torch.float64, device=self.device)
            if workspace is None:
                workspace = o.get("_wsb")
            if workspace is None:
                workspace = stats.new_workspace(M, self.device)
        o["_Zb"], o["_recb"], o["_wsb"] = Z, rec, workspace
        return Z, rec, workspace

    def _check_alphas(self, alpha, alphas, K):
        """``eval_batch_device(alphas=...)``: K entries, and no scalar ``alpha`` beside them"""
        if alpha is not None:
            raise ValueError("pass either alpha (one for every row) or alphas (one per row), not both")
        n = alphas.numel() if isinstance(alphas, torch.Tensor) else len(alphas)
        if n != K:
            raise ValueError(f"alphas has {n} entries for {K} control sequences")

    def _rows_records(self, o, Z, M, alphas, workspace):
        """The records of the rows of Z [K][ld], row k at alphas[k] (rato_risk_stats_rows behind the rollouts' launch);
        the record buffer and the rows workspace are kept in ``o``"""
        K = Z.shape[0]
        rec = o.get("_recrows")
        if rec is None or tuple(rec.shape) != (K, stats.N_STATS):
            rec = torch.empty((K, stats.N_STATS), dtype=torch.float64, device=self.device)
        if workspace is None and o.get("_wsrows_shape") == (M, K):
            workspace = o.get("_wsrows")
        if workspace is None:
            workspace = stats.new_rows_workspace(M, K, self.device)
        o["_recrows"], o["_wsrows"], o["_wsrows_shape"] = rec, workspace, (M, K)
        return stats.risk_stats_rows_device(Z, alphas, workspace=workspace, out=rec, M=M)

    def _fused_step(self, us_mat, alpha, M, workspace, stats_out, **kw):
        """``step_device`` where the linearize launch computes the statistics of its own Z: -> (result dict, record)"""
        if workspace is None:
            workspace = stats.new_workspace(M, self.device)
        if stats_out is None:
            stats_out = torch.empty(stats.N_STATS, dtype=torch.float64, device=self.device)
        return self.linearize_device(us_mat, stats_request=(workspace, stats_out, alpha), **kw), stats_out

    # ---- the model's noise --------------------------------------------------
    def _tiled_noise(self, dW, M, ld=None):
        """The [tile][N_NOISE S][64] copy of the MODEL'S OWN noise that the row-parallel kernel reads (``ld``: the row stride
        of dW, default M: no padding, as the driving arrays have it); made once, kept with
        the source tensor itself (compared by identity: an address can be recycled by the allocator, a live tensor
        cannot).  A caller's ``inputs`` are never cached -- ``None`` sends them through the kernel that reads dW as it
        lies.  Whoever rewrites ``self._dW`` in place through raw pointers (the library's samplers do not bump a
        tensor's version counter) must call ``set_noise`` / ``invalidate_noise``."""
        if dW is not self._dW:
            return None
        if ld is None:
            ld = M
        c = self._dW_tiled_cache
        if c is None or c[0] is not dW or c[1] != dW._version or c[3] != (M, ld, self.S):
            c = self._dW_tiled_cache = (dW, dW._version, self._tile_noise(dW, M, ld), (M, ld, self.S))
        return c[2]

    def invalidate_noise(self):
        """Forget every copy derived from ``self._dW`` (after an in-place refill of the noise array)."""
        self._dW_tiled_cache = None

    def set_noise(self, dW):
        """Replace the batch's Brownian increments (kernel layout [S][N_NOISE][ld], fp32, on the model's device)."""
        dW = _lib.require_f32_device(dW, "dW")
        shape = (self.S, self.N_NOISE, self._batch_shape()[1])
        if tuple(dW.shape) != shape:
            raise ValueError(f"dW must be {shape}, got {tuple(dW.shape)}")
        self._dW = dW
        self.invalidate_noise()

    # ---- L4: host QP (drone_risk.py:457-469, driving.py:444-456) -----------
    def _solve(self, verbose):
        S, n_u = self.S, self.N_U
        self.res = self.osqp_prob.solve()
        if self.res.info.status != 'solved':
            print("[solve]: Problem infeasible.")
        us_sol = self.convert_us_vec_to_us_mat(self.res.x[:(n_u * S)])
        ys, t_risk_sol = self.res.x[(n_u * S):-2], self.res.x[-1]
        if verbose:
            print("y_min =", np.min(ys))
            print("slack_var =", self.res.x[-2])
        return us_sol, t_risk_sol

    # ---- L4 at large M: reduced (u, slack) problem with device CVaR cuts ----------------------
    def shard(self, group=None):
        """Declare this Model one shard of a sample-sharded batch (one process per GPU, torch.distributed already
        initialised, equal shard sizes): ``solve_reduced`` then merges the sample means (the drone's; the final rows of the
        driving problem are sample independent) and runs the cutting-plane oracle across the ranks (cvar_cuts.py); every
        rank returns the same iterate."""
        import torch.distributed as tdist
        from . import dist as rdist
        rdist.check_equal_shards(self.M, group)          # raises on every rank if the shards differ
        rdist.check_equal_shards(self.S, group, what="horizons S")   # (... the lengths of every exchanged buffer)
        self._group, self._world = group, tdist.get_world_size(group)
        # buffers a single-process solve_reduced may have left behind are single-process shaped (pinned HOST sums that
        # the partial-sum kernel writes into directly): a sharded solve must not inherit them
        self._drop_solver_state()
        return self

    def _reduced_cut_solver(self, M, ld=None):
        cs = self._cut_solver
        if cs is None:
            cs = cvar_cuts.CvarCutSolver(self._lib, self.device, n_u=self.N_U, S=self.S, M=M, ld=(M if ld is None else ld),
                                         R=self.CUT_ROWS, alpha=self.alpha, dt=self.dt, Rcost=self.RCOST,
                                         slack_penalty=self.SLACK_PENALTY, u_min=self.u_min, u_max=self.u_max,
                                         group=self._group, world=self._world, mode=self.method, rhs0=self.CUT_RHS0)
            self._cut_solver = cs
        return cs

    def certify_reduced(self, info):
        """Matrix-free KKT certificate of the last ``solve_reduced`` (its ``info``; table-free oracle, an iteration with the
        CVaR rows, before any other solve) against the reference's full QP (drone_risk.py:327-368, driving.py:330-373):
        certificate.py."""
        from . import certificate
        return certificate.certify(self._cut_solver, info, info["final_du"], info["final_rhs"], kappa=self.KAPPA)

    # ---- Monte-Carlo validation (drone_risk.py:649-695, driving.py:623-671) ----
    def _monte_carlo_verification(self, us_mat):
        """vmap of drone_risk.py:656-662 / driving.py:630-638 -> (B_satisfied (M,) bool, max_constraint (M,))."""
        Z, _, _ = self.eval_device(us_mat)
        Zh = Z.double().cpu().numpy()
        return Zh <= 1e-6, Zh

    monte_carlo_statistics = stats.monte_carlo_statistics
    monte_carlo_avar = staticmethod(stats.monte_carlo_avar)
    monte_carlo_var = staticmethod(stats.monte_carlo_var)
