"""Driver loops around the hot path -- counterparts of the reference's timed experiment loops, so that the
recorded tables (step_time / regret, the three BO timers, the active-learning curve) can be regenerated on this
library:

  online_regression   experiments/regression.py:41-81      evaluate -> update per incoming batch, `online_metrics` rows
  bayesopt            experiments/bayesopt/bayesopt.py:180-236   re-initialise from the kernel cache + fit / acquisition /
                                                            condition, one row of timers per step
  qnipv_active_learning  experiments/active_learning/qnIPV_experiment.py:150-215   look-ahead variance reduction through
                                                            batched fantasies

Hydra, datasets, loggers and BoTorch's optimisers are out of scope: callers pass tensors and get rows
back; ``write_csv`` stores them.  Two acquisition optimisers: a random search over candidate sets, and ``optimize_acqf`` --
the gradient optimiser of the reference's loop (BoTorch's ``optimize_acqf``: raw samples, restarts, L-BFGS), driven by the
posterior's gradients w.r.t. its query points.
"""
import csv
import math
import time

import torch

from . import grid_ops, settings
from .distributions import sampling_cholesky
from .mlls import BatchedWoodburyMarginalLogLikelihood


def write_csv(rows, path):
    if not rows:
        return
    cols = list(rows[0].keys())
    with open(path, "w", newline="") as fh:
        w = csv.DictWriter(fh, fieldnames=cols)
        w.writeheader()
        for r in rows:
            w.writerow(r)


def settle_interpreter_heap():
    """Collect, then freeze the interpreter's long-lived object graph (torch + numpy: ~10^6 objects).  A streaming loop of
    0.1 - 0.3 ms steps otherwise meets a FULL cyclic-GC pass every few hundred steps, and that pass costs ~80 ms
    (tools/stall_probe.py) -- several hundred steps' worth.  After the freeze the collector only scans objects created since.
    Call once after the models are built; harmless to call again (it unfreezes, collects and re-freezes)."""
    import gc

    gc.unfreeze()
    gc.collect()
    gc.freeze()


def _sync(t):
    if torch.is_tensor(t) and t.is_cuda:
        torch.cuda.synchronize(t.device)


# ------------------------------------------------------------------------------------------------ streaming regression
def online_regression(online_model, train_x, train_y, test_x, test_y, batch_size=1, logging_freq=1, update_stem=True,
                      batch_model=None, max_steps=None):
    """For every incoming batch: evaluate (rmse, nll of the batch *before* it is absorbed), then update; `step_time`
    covers exactly those two calls.  Every `logging_freq` steps a row with the cumulative online metrics, the regret
    against `batch_model` (a model fitted on the whole stream, optional), test metrics, the learned noise and the step time
    is appended.  Returns the rows of the reference's `online_metrics` table."""
    rows = []
    on_rmse = on_nll = b_rmse_sum = b_nll_sum = 0.0
    settle_interpreter_heap()
    n = train_x.shape[-2]
    steps = n // batch_size if max_steps is None else min(max_steps, n // batch_size)
    for t in range(steps):
        x = train_x[t * batch_size:(t + 1) * batch_size]
        y = train_y[t * batch_size:(t + 1) * batch_size]
        _sync(x)
        t0 = time.perf_counter()
        with settings.detach_interp_coeff(True):
            o_rmse, o_nll = online_model.evaluate(x, y)
        stem_loss, gp_loss = online_model.update(x, y, update_stem=update_stem)
        _sync(x)
        step_time = time.perf_counter() - t0
        on_rmse += o_rmse
        on_nll += o_nll
        if batch_model is not None:
            with torch.no_grad():
                br, bn = batch_model.evaluate(x, y)
            b_rmse_sum += br
            b_nll_sum += bn
        if t % logging_freq == logging_freq - 1:
            rmse, nll = online_model.evaluate(test_x, test_y)
            rows.append({"step": (t + 1) * batch_size, "stem_loss": float(stem_loss), "gp_loss": float(gp_loss),
                         "batch_rmse": b_rmse_sum, "batch_nll": b_nll_sum, "online_rmse": on_rmse, "online_nll": on_nll,
                         "regret": on_rmse - b_rmse_sum, "test_rmse": rmse, "test_nll": nll,
                         "noise": float(online_model.noise.detach().mean()), "step_time": step_time})
    return rows


# ---------------------------------------------------------------------------------------------------------- BayesOpt
def fit_mll(model, num_iter=30, lr=0.1):
    """Maximise the Woodbury MLL (+ registered priors) over the model's hyper-parameters with Adam; the reference calls
    BoTorch's L-BFGS-B wrapper here.  Returns the final MLL value."""
    mll = BatchedWoodburyMarginalLogLikelihood(model.likelihood, model)
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=lr)
    model.train()
    val = None
    for _ in range(num_iter):
        opt.zero_grad()
        val = mll(None, None).sum()
        (-val).backward()
        opt.step()
        model.zero_grad()
    model.eval()
    return float(val.detach()) if val is not None else float("nan")


def ucb_random_search(model, q, d, num_candidates=512, beta=2.0, generator=None, device=None, dtype=None):
    """argmax over random candidate sets X [num_candidates, q, d] in the unit cube of mean_q(mu + sqrt(beta) sigma): a
    derivative-free stand-in for optimize_acqf(qUCB)."""
    device = device if device is not None else model._device
    dtype = dtype if dtype is not None else model._dtype
    cand = torch.rand((num_candidates, q, d), generator=generator, device="cpu").to(device, dtype)
    with torch.no_grad():
        post = model.posterior(cand)
        score = (post.mean[..., 0] + math.sqrt(beta) * post.variance[..., 0].clamp_min(0).sqrt()).max(dim=-1).values
    return cand[int(score.argmax())]


# ------------------------------------------------------------------------------------- look-ahead acquisitions (dense regime)
def _dense_parts(model):
    """(grid, M, mu, sigma2, fantasy noise, err flag) of a single-output model in the dense regime: what the collapsed look-ahead
    acquisitions read.  The fantasy noise is the one ``fantasize`` passes: the mean of the likelihood's noise."""
    if not hasattr(model, "prediction_cache") or not hasattr(model, "_grid"):
        raise ValueError("look-ahead acquisitions (qnipv, kg) need an online SKI model")
    pc = model.prediction_cache
    M = getattr(pc["pred_cov"], "dense", None)
    if M is None or model.num_outputs > 1:
        raise NotImplementedError("look-ahead acquisitions (qnipv, kg) are implemented in the dense regime only (a cached posterior M: "
                                  "m <= settings.max_cholesky_size with settings.dense_small_grids on) and for a single output")
    noise = model.likelihood.noise.detach().mean().to(M)
    return model._grid, M, pc["pred_mean"][0, :, 0].contiguous(), float(model._sigma2(0)), noise, model._err


class QNIPVCache:
    """What qNIPV needs of a (model, MC set) pair, built once: with R = W_Z M (one row gather of M over the N MC points Z),
    H = R^T R / N (one GEMM) and the constant c0 = mean_p w_p^T M w_p.  Every later evaluation reads only q x q blocks of M and H,
    so it costs nothing that grows with N."""

    def __init__(self, model, mc_points):
        grid, M, mu, s2, noise, err = _dense_parts(model)
        Z = mc_points.to(M).reshape(-1, grid.d).contiguous()
        with torch.no_grad():
            R = grid_ops.gather_rows(grid, Z, M, err)                                       # [N, m]: rows w_p^T M
            H = grid_ops.gemm(R, R, ta=True, alpha=1.0 / Z.shape[0])                         # M (sum_p w_p w_p^T / N) M
            self.H = 0.5 * (H + H.t())
            self.c0 = grid_ops.gather(grid, Z, R, err, diag=True).mean()                     # mean_p w_p^T M w_p
        flag = grid_ops.read_flag(err)
        if flag:
            model._raise_out_of_bounds(flag)
        self.grid, self.M, self.sigma2, self.noise, self.err = grid, M, s2, noise, err
        self.model = model
        # the posterior factor itself is kept (not its id: a rebuilt factor can reuse a freed one's address)
        self._key = (model.prediction_cache["pred_cov"], mc_points, mc_points._version)

    def matches(self, model, mc_points):
        return self._key[0] is model.prediction_cache["pred_cov"] and self._key[1] is mc_points and self._key[2] == mc_points._version

    def values(self, X):
        """qNIPV = -IPV of every q-batch X [b, q, d] ([b]): IPV = sigma2 (c0 - tr(L^-1 W_X H W_X^T L^-T)), S = L L^T = W_X M W_X^T + diag(noise).
        The fantasy variance does not depend on the sampled targets, so no fantasies are drawn."""
        grid = self.grid
        q = X.shape[-2]
        S = grid_ops.interp_bilinear(grid, self.M, X, None, self.err)
        S = S + torch.diag_embed(self.noise.clamp_min(1e-7).expand(X.shape[:-1]))
        B = grid_ops.interp_bilinear(grid, self.H, X, None, self.err)
        flag = grid_ops.read_flag(self.err)
        if flag:
            self.model._raise_out_of_bounds(flag)
        L, info = torch.linalg.cholesky_ex(S)
        if bool((info != 0).any()):
            raise RuntimeError("fantasy covariance block is not positive definite")
        C = torch.linalg.solve_triangular(L, B, upper=False)                                  # L^-1 B
        D = torch.linalg.solve_triangular(L, C.transpose(-1, -2), upper=False)                # L^-1 B L^-T
        ipv = self.sigma2 * (self.c0 - D.diagonal(dim1=-2, dim2=-1).sum(-1))
        return -ipv


def qnipv_cache(model, mc_points):
    """The :class:`QNIPVCache` of (model, mc_points), memoised on the model."""
    c = model.__dict__.get("_qnipv_cache")          # valid while the model's posterior factor is the same object
    if c is None or not c.matches(model, mc_points):
        c = QNIPVCache(model, mc_points)
        model.__dict__["_qnipv_cache"] = c
    return c


def kg_values(model, X, Xp, base_samples, current_value):
    """One-shot qKG (BoTorch's qKnowledgeGradient) of every restart: q-batch X [b, q, d] and one look-ahead point per fantasy
    Xp [b, J, d], fixed standard normals `base_samples` z [J, q].  Fantasy j draws its targets at X as ``fantasize`` does,
    y_j = W_X mu + L_obs z_j with L_obs = sampling_cholesky(sigma2 (W_X M W_X^T + I)) (the factor the posterior's rsample uses), and
    conditions on them with S = W_X M W_X^T + diag(noise); its posterior mean at x'_j is w'_j^T mu + w'_j^T M W_X^T S^-1 L_obs z_j.
    Returns mean_j of those means minus `current_value` ([b]), differentiable w.r.t. X and Xp.  With the fantasy noise equal to the
    observation noise this is w'^T mu + c_j L^-T z_j of the one-shot form (c_j = sigma2 w'_j^T M W_X^T, L = chol(sigma2 S))."""
    grid, M, mu, s2, noise, err = _dense_parts(model)
    b, q, J = X.shape[0], X.shape[-2], Xp.shape[-2]
    z = base_samples.to(M)
    B = grid_ops.interp_bilinear(grid, M, X, None, err)                                       # W_X M W_X^T    [b, q, q]
    C = grid_ops.interp_bilinear(grid, M, X, Xp, err)                                         # W_X M W'^T     [b, q, J]
    mp = grid_ops.Gather.apply(grid, Xp.reshape(-1, grid.d), mu[None], err)[:, 0].reshape(b, J)         # w'^T mu
    flag = grid_ops.read_flag(err)
    if flag:
        model._raise_out_of_bounds(flag)
    cov = s2 * (B + torch.eye(q, dtype=M.dtype, device=M.device))
    # the factor fantasize's rsample draws through, with each restart's own diagonal scale (rsample sees one candidate set at a time)
    Lobs = sampling_cholesky(cov, cov.diagonal(dim1=-2, dim2=-1).mean(-1).clamp_min(1e-30)[:, None, None])
    L, info = torch.linalg.cholesky_ex(B + torch.diag_embed(noise.clamp_min(1e-7).expand(b, q)))
    if bool((info != 0).any()):
        raise RuntimeError("fantasy covariance block is not positive definite")
    resid = torch.matmul(Lobs, z.t())                                                          # y_j - W_X mu   [b, q, J]
    alpha = torch.cholesky_solve(resid, L)                                                     # S^-1 (y_j - W_X mu)
    return (mp + (C * alpha).sum(-2)).mean(-1) - float(current_value)


# ------------------------------------------------------------------------------------- pathwise acquisitions (every regime)
def _paths_for(model, want):
    """How many of `want` sample paths the model can draw: any number in the dense regime, its probe count beyond it."""
    if not hasattr(model, "sample_paths"):
        raise ValueError("pathwise acquisitions (ts, nei) need an online SKI model")
    P = model._kernel_cache.get("path_probes")
    if model._use_dense() or P is None:
        return want                       # (beyond the dense regime without probes sample_paths raises and says how to get them)
    return min(want, P.shape[1])


def ts_values(paths, X):
    """q-batch Thompson sampling: point j of every q-batch X [b, q, d] is scored by path j; value = sum_j f_j(x_j) ([b])."""
    q = X.shape[-2]
    if paths.num_paths != q:
        raise ValueError(f"ts needs one path per point of the batch: {paths.num_paths} paths for q = {q}")
    F = paths(X)                                                       # [q, b, q]
    return F.diagonal(dim1=0, dim2=-1).sum(-1)


def nei_values(paths, X, baseline_max):
    """Pathwise qNoisyExpectedImprovement of every q-batch X [b, q, d]: mean_s (max_j f_s(x_j) - max_i f_s(X_baseline_i))^+ ([b]); the
    candidates and the baseline are scored by the SAME draws (`baseline_max` [num_paths] = ``paths.max_values(X_baseline)``)."""
    F = paths(X)                                                       # [S, b, q]
    return (F.max(-1).values - baseline_max[:, None]).clamp_min(0).mean(0)


def thompson_sample(model, candidates, q, seed=0):
    """Discrete Thompson sampling (BoTorch's ``MaxPosteriorSampling``): draw q posterior sample paths and return, for each, the
    candidate [N, d] that maximises it: [q, d]."""
    paths = model.sample_paths(q, seed=seed)
    cand = candidates.reshape(-1, candidates.shape[-1])
    return cand[paths.argmax(cand).to(cand.device)]


_ACQFS = ("ucb", "ei", "qei", "qnipv", "kg", "ts", "nei")


def acqf_values(model, X, acqf, beta=2.0, best_f=None, base_samples=None, mc_points=None, current_value=None, X_baseline=None, paths=None,
                baseline_max=None, seed=0, num_mc_samples=256):
    """Acquisition value of every q-batch X [b, q, d] ([b]) from ONE batched posterior call, differentiable w.r.t. X:
    ``"ucb"`` mu + sqrt(beta) sigma for q = 1, BoTorch's qUCB (mean_s max_q mu + sqrt(beta pi / 2) |s - mu|) otherwise;
    ``"ei"`` analytic expected improvement over `best_f` for q = 1, qEI otherwise; ``"qei"`` qEI (mean_s max_q (s - best_f)^+).
    The MC forms draw through the fixed standard normals `base_samples` [S, q] (a sample-average approximation: the value is a
    deterministic function of X).
    Look-ahead forms (dense regime): ``"qnipv"`` qNegIntegratedPosteriorVariance over `mc_points` [N, d] in its
    collapsed form (:class:`QNIPVCache`); ``"kg"`` one-shot qKG (:func:`kg_values`): X is [b, q + J, d], the q-batch followed by
    one point per fantasy, `base_samples` [J, q] are the fantasies' normals and `current_value` (default `best_f`) is subtracted.
    Pathwise forms (every regime), on posterior sample paths (`paths`, or drawn from `seed` by ``model.sample_paths``):
    ``"ts"`` q-batch Thompson sampling, sum_j f_j(x_j) with one path per point of the batch; ``"nei"`` qNoisyExpectedImprovement,
    mean_s (max_j f_s(x_j) - max_i f_s(`X_baseline`_i))^+ over `num_mc_samples` paths (at most the model's probe count beyond the dense
    regime); `baseline_max` may carry ``paths.max_values(X_baseline)`` computed once."""
    if acqf not in _ACQFS:
        raise ValueError(f"unknown acquisition function {acqf!r} ({', '.join(_ACQFS)})")
    if acqf in ("ei", "qei") and best_f is None:
        raise ValueError("expected improvement needs best_f")
    if acqf == "qnipv":
        if mc_points is None:
            raise ValueError("qnipv needs mc_points")
        return qnipv_cache(model, mc_points).values(X)
    if acqf == "ts":
        return ts_values(paths if paths is not None else model.sample_paths(X.shape[-2], seed=seed), X)
    if acqf == "nei":
        if X_baseline is None and baseline_max is None:
            raise ValueError("nei needs X_baseline")
        if paths is None:
            paths = model.sample_paths(_paths_for(model, num_mc_samples), seed=seed)
        if baseline_max is None:
            baseline_max = paths.max_values(X_baseline.to(paths.values))
        return nei_values(paths, X, baseline_max)
    if acqf == "kg":
        if base_samples is None or base_samples.dim() != 2:
            raise ValueError("kg needs base_samples [num_fantasies, q]")
        cv = best_f if current_value is None else current_value
        if cv is None:
            raise ValueError("kg needs current_value (or best_f)")
        J, q = base_samples.shape
        if X.shape[-2] != q + J:
            raise ValueError(f"kg expects X [b, q + num_fantasies = {q + J}, d], got {tuple(X.shape)}")
        return kg_values(model, X[..., :q, :], X[..., q:, :], base_samples, cv)
    lead = X.shape[:-1]
    post = model.posterior(X)
    mu = post.mean[..., 0].reshape(lead)
    if lead[-1] == 1 and acqf in ("ucb", "ei"):
        mu, sd = mu[..., 0], post.variance[..., 0].reshape(lead)[..., 0].clamp_min(1e-18).sqrt()
        if acqf == "ucb":
            return mu + math.sqrt(beta) * sd
        u = (mu - float(best_f)) / sd
        return sd * (u * torch.special.ndtr(u) + torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi))
    S = base_samples.shape[0]
    z = base_samples.to(mu)[:, None, :].expand(S, *lead)
    samples = post.rsample(torch.Size([S]), base_samples=z)[..., 0].reshape(S, *lead)
    if acqf == "ucb":
        return (mu + math.sqrt(beta * math.pi / 2) * (samples - mu).abs()).max(-1).values.mean(0)
    return (samples - float(best_f)).clamp_min(0).max(-1).values.mean(0)


def optimize_acqf(model, acqf, bounds, q, num_restarts=10, raw_samples=512, maxiter=200, seed=0, beta=2.0, best_f=None, num_mc_samples=256,
                  mc_points=None, num_fantasies=64, current_value=None, X_baseline=None):
    """The reference's ``optimize_acqf`` (experiments/bayesopt/utils.py:149-161, same defaults): score `raw_samples` random q-batches
    in the box `bounds` [2, d], start from the `num_restarts` best and optimise all restarts at once -- one batched posterior call
    (and its backward) per evaluation -- with ``torch.optim.LBFGS`` (strong-Wolfe line search, at most `maxiter` iterations) on a
    sigmoid reparameterisation X = lo + (hi - lo) sigmoid(Z).  The sigmoid keeps every iterate strictly inside the box, hence
    inside the model's grid (queries outside it raise), without a projection step that an unmodified L-BFGS would not expect; a
    maximiser on the boundary is approached to within the sigmoid's saturation.  A restart that ends below its start keeps its
    start.  `acqf` / `beta` / `best_f` as in :func:`acqf_values`; MC forms use `num_mc_samples` fixed normals drawn from `seed`.
    ``"qnipv"`` needs `mc_points`.  ``"kg"`` is one-shot: the variables are [b, q + num_fantasies, d] (the q-batch and one look-ahead
    point per fantasy) under the same reparameterisation, the fantasies' normals [num_fantasies, q] are drawn from `seed`, and
    `current_value` defaults to `best_f`.  ``"ts"`` draws q sample paths and ``"nei"`` `num_mc_samples` of them (at most the model's
    probe count beyond the dense regime) ONCE per call, from `seed`; ``"nei"`` needs `X_baseline`, whose per-path maxima are computed
    once.  Returns (best q-batch [q, d], its value)."""
    if acqf not in _ACQFS:
        raise ValueError(f"unknown acquisition function {acqf!r} ({', '.join(_ACQFS)})")
    if acqf == "qnipv" and mc_points is None:
        raise ValueError("qnipv needs mc_points")
    if acqf == "kg" and current_value is None and best_f is None:
        raise ValueError("kg needs current_value (or best_f)")
    if acqf == "nei" and X_baseline is None:
        raise ValueError("nei needs X_baseline")
    bounds = torch.as_tensor(bounds)
    device = getattr(model, "_device", bounds.device)
    dtype = getattr(model, "_dtype", bounds.dtype if bounds.is_floating_point() else torch.float64)
    lo, hi = bounds[0].to(device, dtype), bounds[1].to(device, dtype)
    span = hi - lo
    d = lo.numel()
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    nv = q + num_fantasies if acqf == "kg" else q
    raw = lo + span * torch.rand((raw_samples, nv, d), generator=g, dtype=torch.float64).to(device, dtype)
    base = torch.randn((num_fantasies if acqf == "kg" else num_mc_samples, q), generator=g, dtype=torch.float64).to(device, dtype)
    paths = baseline_max = None
    if acqf in ("ts", "nei"):
        paths = model.sample_paths(q if acqf == "ts" else _paths_for(model, num_mc_samples), seed=int(seed))
        if acqf == "nei":
            baseline_max = paths.max_values(X_baseline.to(device, dtype))
    f = lambda X: acqf_values(model, X, acqf, beta=beta, best_f=best_f, base_samples=base, mc_points=mc_points, current_value=current_value,
                              paths=paths, baseline_max=baseline_max)
    with torch.no_grad():
        vals = f(raw)
    top = vals.topk(min(num_restarts, raw_samples)).indices
    X0, v0 = raw[top], vals[top]
    Z = torch.logit(((X0 - lo) / span).clamp(1e-6, 1 - 1e-6)).detach().requires_grad_(True)
    opt = torch.optim.LBFGS([Z], lr=1.0, max_iter=maxiter, line_search_fn="strong_wolfe", tolerance_grad=1e-9, tolerance_change=1e-12)

    def closure():
        opt.zero_grad()
        loss = -f(lo + span * torch.sigmoid(Z)).sum()
        loss.backward()
        return loss

    opt.step(closure)
    with torch.no_grad():
        X1 = lo + span * torch.sigmoid(Z)
        v1 = f(X1)
        better = v1 > v0
        X = torch.where(better[:, None, None], X1, X0)
        v = torch.where(better, v1, v0)
        best = int(v.argmax())
    return X[best, :q].detach(), v[best].detach()


def bayesopt(test_function, bounds, make_model, init_x, init_y, num_steps, batch_size=3, noise=None, fit_iters=30,
             num_candidates=512, beta=2.0, seed=0, on_step=None, acqf_optimizer="random", acqf="ucb", num_restarts=10, maxiter=200,
             num_fantasies=256):
    """The reference's BO loop with its three timers.  Per step:
        t0  re-initialise the model from the previous model's kernel cache (``make_model(train_x, train_y, old_model)``,
            bayesopt.py:86-96) and refit the hyper-parameters on the MLL,
        t1  optimise the acquisition over q-batches in the unit cube, evaluate ``test_function`` on the un-normalised points,
        t2  ``condition_on_observations`` (functional: returns the model of the next step).
    `bounds` [d, 2] are the test function's bounds; inputs handed to the model live in the unit cube (and the grid covers
    the raw bounds: the reference's quirk).  Targets are standardised with the initial statistics.  Returns
    (rows, train_x, train_y) with rows = dict(fit_time, acqf_time, condition_time, total, max_achieved).
    `acqf_optimizer`: ``"random"`` -- :func:`ucb_random_search` over `num_candidates` sets; ``"gradient"`` -- :func:`optimize_acqf`
    of `acqf` with `num_candidates` raw samples, `num_restarts` restarts and `maxiter` L-BFGS iterations (the reference's loop);
    ``acqf="kg"`` is the reference's ``--acqf kg``: one-shot qKG with `num_fantasies` fantasies and current_value = max train_y;
    ``acqf="ts"`` q-batch Thompson sampling and ``acqf="nei"`` the reference's ``--acqf nei`` (pathwise, X_baseline = train_x), both on
    posterior sample paths: beyond the dense regime `make_model` must build its models with ``num_path_probes``."""
    if acqf_optimizer not in ("random", "gradient"):
        raise ValueError(f"acqf_optimizer must be 'random' or 'gradient', got {acqf_optimizer!r}")
    g = torch.Generator(device="cpu").manual_seed(seed)
    d = bounds.shape[0]
    lo, hi = bounds[:, 0], bounds[:, 1]
    mean, std = init_y.mean(), init_y.std().clamp_min(1e-12)
    train_x, train_y = init_x, (init_y - mean) / std
    model = None
    rows = []
    for step in range(num_steps):
        _sync(train_x); t = time.perf_counter()
        model = make_model(train_x, train_y, model)
        fit_mll(model, fit_iters)
        _sync(train_x); t0 = time.perf_counter() - t
        t = time.perf_counter()
        if acqf_optimizer == "random":
            new_x = ucb_random_search(model, batch_size, d, num_candidates, beta, g)
        else:
            unit = torch.stack([torch.zeros(d, dtype=torch.float64), torch.ones(d, dtype=torch.float64)])
            new_x, _ = optimize_acqf(model, acqf, unit, batch_size, num_restarts=num_restarts, raw_samples=num_candidates, maxiter=maxiter,
                                     seed=int(torch.randint(2 ** 31 - 1, (1,), generator=g)), beta=beta, best_f=float(train_y.max()),
                                     num_fantasies=num_fantasies, X_baseline=train_x if acqf == "nei" else None)
            new_x = new_x.to(train_x)
        raw = test_function(lo.to(new_x) + (hi - lo).to(new_x) * new_x)
        new_y = ((raw.reshape(-1, 1) - mean) / std).to(train_y)
        train_x, train_y = torch.cat([train_x, new_x]), torch.cat([train_y, new_y])
        _sync(train_x); t1 = time.perf_counter() - t
        t = time.perf_counter()
        kw = {} if noise is None else {"noise": torch.full_like(new_y, float(noise))}
        model = model.condition_on_observations(X=new_x, Y=new_y, **kw)
        _sync(train_x); t2 = time.perf_counter() - t
        rows.append({"step": step, "fit_time": t0, "acqf_time": t1, "condition_time": t2, "total": t0 + t1 + t2,
                     "max_achieved": float(train_y.max() * std + mean)})
        if on_step is not None:
            on_step(step, model, train_x, train_y)
    return rows, train_x, train_y, model


# ------------------------------------------------------------------------------------------- qNIPV active learning
def qnipv_select(model, candidate_sets, mc_points, sampler):
    """Negative integrated posterior variance of every candidate set [b, q, d] (BoTorch's qNegIntegratedPosteriorVariance):
    fantasize on the set, average the fantasy posterior variance over `mc_points` and over the fantasies.  Returns the scores [b]
    (higher = better)."""
    with torch.no_grad():
        fm = model.fantasize(candidate_sets, sampler, observation_noise=True)
        var = fm.posterior(mc_points).variance                  # [num_fantasies, b, N, 1]
        return -var.mean(dim=-2).squeeze(-1).mean(dim=0)


def snap_to_pool(model, X, pool_x, avail):
    """Indices of distinct available pool points for the candidates X [q, d], greedily in order: each takes the still-available
    point of maximal base-kernel covariance (the product over dims of the kernel's lag profile) and removes it."""
    k = model.covar_module.base_kernel
    P = pool_x.to(X)
    free = avail.to(P.device).clone()
    picks = []
    with torch.no_grad():
        for i in range(X.shape[0]):
            lag = (P - X[i]).abs()
            cov = torch.ones(P.shape[0], dtype=P.dtype, device=P.device)
            for dim in range(P.shape[1]):
                cov = cov * k.lag_column(dim, lag[:, dim]).to(P)
            cov = torch.where(free, cov, torch.full_like(cov, -math.inf))
            j = int(cov.argmax())
            free[j] = False
            picks.append(j)
    return torch.tensor(picks, dtype=torch.long)


def qnipv_active_learning(model, pool_x, observe, mc_points, batch_size=6, num_steps=10, num_candidate_sets=32, num_fantasies=4,
                          noise_fn=None, seed=0, on_step=None, selector="random"):
    """Per step: choose a q-subset of the remaining pool by qNIPV, query ``observe`` at it, condition the model (functional).
    Returns (rows, model, chosen indices); rows carry the selection / conditioning times and the integrated posterior variance
    over `mc_points` after the step.
    `selector`: ``"random"`` scores `num_candidate_sets` random q-subsets through batched fantasies (`num_fantasies` each);
    ``"gradient"`` is the reference's loop (qnIPV_experiment.py:177-205): ``optimize_acqf("qnipv", unit box, q=batch_size,
    num_restarts=1, raw_samples=10, maxiter=200)`` on the collapsed qNIPV, then each candidate snaps to the available pool point
    of maximal base-kernel covariance (:func:`snap_to_pool`).  Unlike the reference, which can pick the same pool point twice,
    the snap is greedy over the still-available points, so the q picks are distinct.  With either selector a row's ``qnipv_best`` is the
    qNIPV of the q pool points chosen (for ``"gradient"`` the snapped set, not the optimiser's continuous batch)."""
    if selector not in ("random", "gradient"):
        raise ValueError(f"selector must be 'random' or 'gradient', got {selector!r}")
    g = torch.Generator(device="cpu").manual_seed(seed)
    d = pool_x.shape[-1]
    unit = torch.stack([torch.zeros(d, dtype=torch.float64), torch.ones(d, dtype=torch.float64)])

    class _Sampler:
        def __init__(self, n):
            self.sample_shape = torch.Size([n])

        def __call__(self, posterior):
            return posterior.rsample(self.sample_shape)

    avail = torch.ones(pool_x.shape[0], dtype=torch.bool)
    rows, chosen = [], []
    for step in range(num_steps):
        _sync(pool_x); t = time.perf_counter()
        if selector == "gradient":
            Xc, _ = optimize_acqf(model, "qnipv", unit, batch_size, num_restarts=1, raw_samples=10, maxiter=200,
                                  seed=int(torch.randint(2 ** 31 - 1, (1,), generator=g)), mc_points=mc_points)
            pick = snap_to_pool(model, Xc, pool_x, avail)
            with torch.no_grad():                            # the score of the pool points actually chosen, as for the random selector
                best_val = float(acqf_values(model, pool_x[pick.to(pool_x.device)][None], "qnipv", mc_points=mc_points)[0])
        else:
            idx_pool = avail.nonzero()[:, 0]
            sets = torch.stack([idx_pool[torch.randperm(idx_pool.numel(), generator=g)[:batch_size]] for _ in range(num_candidate_sets)])
            cand = pool_x[sets.to(pool_x.device)]
            scores = qnipv_select(model, cand, mc_points, _Sampler(num_fantasies))
            best = int(scores.argmax())
            pick = sets[best]
            best_val = float(scores[best])
        _sync(pool_x); t_sel = time.perf_counter() - t
        avail[pick] = False
        chosen.append(pick)
        x_new = pool_x[pick.to(pool_x.device)]
        y_new = observe(x_new).reshape(-1, 1)
        t = time.perf_counter()
        kw = {} if noise_fn is None else {"noise": noise_fn(x_new).reshape(-1, 1)}
        model = model.condition_on_observations(X=x_new, Y=y_new.to(x_new), **kw)
        with torch.no_grad():
            ipv = float(model.posterior(mc_points).variance.mean())
        _sync(pool_x); t_cond = time.perf_counter() - t
        rows.append({"step": step, "select_time": t_sel, "condition_time": t_cond, "integrated_posterior_variance": ipv,
                     "qnipv_best": best_val, "num_data": int(model.num_data)})
        if on_step is not None:
            on_step(step, model)
    return rows, model, torch.cat(chosen)
