"""Noise schedules of the path: float64 host tables (as the reference keeps them) and the fp32
coefficient tables the HIP scheduler kernels gather from.

Mirrors ``DDPMScheduler`` (reference latent_module.py:1241-1297) by name and argument meaning; the
tables are constants built once on the host in NumPy float64, exactly like upstream; every per-sample
use on the device goes through dn_q_sample / dn_ddim_step.
"""
import math

import numpy as np
import torch


def betas_for_alpha_bar(n: int, alpha_bar, max_beta: float = 0.999) -> np.ndarray:
    """reference latent_module.py:1145-1162."""
    return np.array([min(1 - alpha_bar((i + 1) / n) / alpha_bar(i / n), max_beta) for i in range(n)])


def get_named_beta_schedule(name: str, n: int) -> np.ndarray:
    """reference latent_module.py:1199-1223 ("linear" | "cosine")."""
    if name == "linear":
        scale = 1000 / n
        return np.linspace(scale * 0.0001, scale * 0.02, n, dtype=np.float64)
    if name == "cosine":
        return betas_for_alpha_bar(n, lambda t: math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2)
    raise NotImplementedError(f"unknown beta schedule: {name}")


class ScheduleTables:
    """The float64 tables shared by DDPMScheduler and GaussianDiffusion (:1247-1276)."""

    def __init__(self, betas: np.ndarray):
        betas = np.asarray(betas, dtype=np.float64)
        assert betas.ndim == 1 and (betas > 0).all() and (betas <= 1).all()
        self.betas = betas
        self.num_timesteps = int(betas.shape[0])
        alphas = 1.0 - betas
        self.alphas_cumprod = np.cumprod(alphas, axis=0)
        self.alphas_cumprod_prev = np.append(1.0, self.alphas_cumprod[:-1])
        self.alphas_cumprod_next = np.append(self.alphas_cumprod[1:], 0.0)
        self.sqrt_alphas_cumprod = np.sqrt(self.alphas_cumprod)
        self.sqrt_one_minus_alphas_cumprod = np.sqrt(1.0 - self.alphas_cumprod)
        self.log_one_minus_alphas_cumprod = np.log(1.0 - self.alphas_cumprod)
        self.sqrt_recip_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod)
        self.sqrt_recipm1_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod - 1)
        self.posterior_variance = betas * (1.0 - self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_log_variance_clipped = (
            np.log(np.append(self.posterior_variance[1], self.posterior_variance[1:]))
            if len(self.posterior_variance) > 1 else np.array([]))
        self.posterior_mean_coef1 = betas * np.sqrt(self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_mean_coef2 = (1.0 - self.alphas_cumprod_prev) * np.sqrt(alphas) / (1.0 - self.alphas_cumprod)

    def f32(self, name_or_array, device=None) -> torch.Tensor:
        """fp32 cast of a table, the form every gather upstream produces (`.float()`, :1235)."""
        if isinstance(name_or_array, str):  # the named tables are immutable: one device copy each (a pageable H2D copy per call
            key = (name_or_array, str(device))  # synchronises the stream -- per training update, that drained the pipeline)
            cache = self.__dict__.setdefault("_f32_cache", {})
            if key not in cache:
                t = torch.from_numpy(np.ascontiguousarray(getattr(self, name_or_array).astype(np.float32)))
                cache[key] = t.to(device) if device is not None else t
            return cache[key]
        t = torch.from_numpy(np.ascontiguousarray(name_or_array.astype(np.float32)))
        return t.to(device) if device is not None else t

    def gaussian_table(self, device=None, fixed_large: bool = False) -> torch.Tensor:
        """fp32 [timesteps, DN_GD_COLS = 12] table of dn_gaussian_step / dn_gaussian_moments / dn_ddpm_loop: {sqrt_recip_abar,
        sqrt_recipm1_abar, posterior_mean_coef1, posterior_mean_coef2, fixed log-variance (FIXED_SMALL: the clipped posterior
        log-variance; FIXED_LARGE: log [posterior_variance[1], betas[1:]], diffusion/gaussian_diffusion.py:300-310),
        posterior_log_variance_clipped, log betas, abar, abar_prev, abar_next, posterior_variance, the fixed variance}."""
        fixed_var = np.append(self.posterior_variance[1], self.betas[1:]) if fixed_large else self.posterior_variance
        fixed_log = np.log(np.append(self.posterior_variance[1], self.betas[1:])) if fixed_large else self.posterior_log_variance_clipped
        cols = [self.sqrt_recip_alphas_cumprod, self.sqrt_recipm1_alphas_cumprod, self.posterior_mean_coef1, self.posterior_mean_coef2,
                fixed_log, self.posterior_log_variance_clipped, np.log(self.betas), self.alphas_cumprod, self.alphas_cumprod_prev,
                np.append(self.alphas_cumprod[1:], 0.0), self.posterior_variance, fixed_var]
        t = torch.from_numpy(np.stack(cols, axis=1).astype(np.float32)).contiguous()
        return t.to(device) if device is not None else t

    def ddim_coef_table(self, device=None) -> torch.Tensor:
        """[timesteps, 4] fp32 rows {sqrt_abar, sqrt(1-abar), sqrt(abar_prev), sqrt(1-abar_prev)} with the
        last two formed in fp32 from the fp32-cast abar_prev, as the eta=0 update does (:1426-1437)."""
        sa, s1, abp = self.f32("sqrt_alphas_cumprod"), self.f32("sqrt_one_minus_alphas_cumprod"), self.f32("alphas_cumprod_prev")
        t = torch.stack([sa, s1, torch.sqrt(abp), torch.sqrt(1 - abp)], dim=1).contiguous()  # torch.sqrt, as upstream
        return t.to(device) if device is not None else t

    def ddim_steps(self, start_step: int, sampling_steps=None, steps=None) -> list:
        """The evaluation timesteps e_0 > ... > e_{n-1} of a DDIM chain entered at `start_step` (x noised by q_sample at
        start_step and treated as level e_0 = start_step-1, reference latent_module.py:1405-1445):

        * `steps`: an explicit list -- non-empty, strictly descending, inside [0, timesteps-1];
        * `sampling_steps` = N evaluations spread uniformly over start_step-1 .. 1 (2 <= start_step, 1 <= N <= start_step-1):
          e_i = (start_step-1) - floor((2 i (start_step-2) + (N-1)) / (2 (N-1))), integers, halves rounded up (N = 1: [start_step-1]);
          N = start_step-1 is every timestep;
        * neither: every timestep, start_step-1 .. 1 ([0] when start_step == 1) -- the chain of `ddim_coef_table`."""
        T = self.num_timesteps
        if steps is not None:
            if sampling_steps is not None:
                raise ValueError("ddim_schedule: give sampling_steps or an explicit list of steps, not both")
            e = [int(v) for v in (steps.tolist() if hasattr(steps, "tolist") else steps)]
            if not e:
                raise ValueError("ddim_schedule: the schedule is empty")
            for i, v in enumerate(e):
                if not 0 <= v <= T - 1:
                    raise ValueError(f"ddim_schedule: step {i} = {v} is outside [0, {T - 1}]")
                if i and v >= e[i - 1]:
                    raise ValueError(f"ddim_schedule: step {i} = {v} does not descend from {e[i - 1]}")
            return e
        s = int(start_step)
        if not 1 <= s <= T - 1:
            raise ValueError(f"ddim_schedule: start_step={s} must be in [1, {T - 1}]")
        if sampling_steps is None:
            return list(range(s - 1, 0, -1)) if s > 1 else [0]
        N = int(sampling_steps)
        if s < 2 or not 1 <= N <= s - 1:
            raise ValueError(f"ddim_schedule: sampling_steps={N} must be in [1, start_step-1 = {s - 1}] (start_step >= 2)")
        if N == 1:
            return [s - 1]
        return [(s - 1) - (2 * i * (s - 2) + (N - 1)) // (2 * (N - 1)) for i in range(N)]

    def ddim_schedule(self, start_step: int, sampling_steps=None, steps=None, eta: float = 0.0, device=None):
        """-> (steps int32 [n], coef fp32 [n, 5]) of dn_ddim_sched_loop for the chain `ddim_steps` selects.  Update i moves x from
        abar[e_i] to abar_tgt(i) = abar[e_{i+1}]; the last one to abar[0], or to 1 (alphas_cumprod_prev[0]) when e_{n-1} == 0.
        Row i = {sqrt abar_e, sqrt(1-abar_e), sqrt abar_tgt, sqrt(1-abar_tgt-sigma^2), sigma} with sigma = eta sqrt((1-abar_tgt) /
        (1-abar_e)) sqrt(1 - abar_e/abar_tgt) (reference diffusion/gaussian_diffusion.py:513-560).  eta == 0: columns 0-3 are formed
        as `ddim_coef_table` forms them (2 and 3 in fp32 from the fp32-cast abar_tgt), so every-timestep rows are its rows bit for
        bit; eta > 0: columns 3 and 4 in float64, then cast."""
        eta = float(eta)
        if not eta >= 0.0:
            raise ValueError(f"ddim_schedule: eta={eta} must be >= 0")
        e = np.asarray(self.ddim_steps(start_step, sampling_steps, steps), dtype=np.int64)
        ab = self.alphas_cumprod[e]
        ab_tgt = np.append(self.alphas_cumprod[e[1:]], self.alphas_cumprod[0] if e[-1] >= 1 else 1.0)
        abt32 = torch.from_numpy(ab_tgt.astype(np.float32))
        sa = torch.from_numpy(self.sqrt_alphas_cumprod[e].astype(np.float32))
        s1 = torch.from_numpy(self.sqrt_one_minus_alphas_cumprod[e].astype(np.float32))
        if eta == 0.0:
            direction, sigma = torch.sqrt(1 - abt32), torch.zeros_like(abt32)
        else:
            sg = eta * np.sqrt((1.0 - ab_tgt) / (1.0 - ab)) * np.sqrt(1.0 - ab / ab_tgt)
            if (1.0 - ab_tgt - sg ** 2 < 0.0).any():
                raise ValueError(f"ddim_schedule: eta={eta} leaves no variance for the direction term (sigma^2 > 1 - abar_tgt)")
            direction = torch.from_numpy(np.sqrt(1.0 - ab_tgt - sg ** 2).astype(np.float32))
            sigma = torch.from_numpy(sg.astype(np.float32))
        coef = torch.stack([sa, s1, torch.sqrt(abt32), direction, sigma], dim=1).contiguous()
        st = torch.from_numpy(e.astype(np.int32))
        return (st.to(device), coef.to(device)) if device is not None else (st, coef)

    def dpm_rows64(self, steps, order: int = 2, lower_order_final: bool = True) -> np.ndarray:
        """float64 [n, 6] coefficient rows of DPM-Solver++(2M) (Lu et al. 2022, data-prediction multistep form) for the validated
        evaluation timesteps `steps`; see `dpm_schedule`."""
        if order not in (1, 2):
            raise ValueError(f"dpm_schedule: order={order} must be 1 or 2")
        e = np.asarray(steps, dtype=np.int64)
        n = len(e)
        ab = self.alphas_cumprod[e]
        ab_tgt = np.append(self.alphas_cumprod[e[1:]], self.alphas_cumprod[0] if e[-1] >= 1 else 1.0)
        al_s, sg_s = np.sqrt(ab), np.sqrt(1.0 - ab)
        lam_s = np.log(al_s / sg_s)
        rows = np.zeros((n, 6), dtype=np.float64)
        for i in range(n):
            c1, c0 = 1.0, 0.0
            if ab_tgt[i] >= 1.0:  # to the clean level: x <- x0, formed without evaluating lambda_t = inf
                a, b = 0.0, 1.0
            else:
                al_t, sg_t = np.sqrt(ab_tgt[i]), np.sqrt(1.0 - ab_tgt[i])
                h = np.log(al_t / sg_t) - lam_s[i]
                a, b = sg_t / sg_s[i], -al_t * np.expm1(-h)
                if order == 2 and i > 0 and not (lower_order_final and i == n - 1):
                    r = (lam_s[i] - lam_s[i - 1]) / h
                    c1, c0 = 1.0 + 0.5 / r, -0.5 / r
            rows[i] = (al_s[i], sg_s[i], a, b, c1, c0)
        return rows

    def dpm_schedule(self, start_step: int, sampling_steps=None, steps=None, order: int = 2, lower_order_final: bool = True, device=None):
        """-> (steps int32 [n], coef fp32 [n, DN_DPM_COLS = 6]) of dn_dpm_loop for the chain `ddim_steps` selects (the same selection
        rule and validation as `ddim_schedule`).  With alpha = sqrt abar, sigma = sqrt(1 - abar), lambda = log(alpha / sigma), s =
        e_i, t = `ddim_schedule`'s target level of update i (abar[e_{i+1}]; the last one abar[0], or 1 when e_{n-1} == 0) and h_i =
        lambda_t - lambda_s, row i = {alpha_s, sigma_s, a, b, c1, c0} drives

            x0_i = (x - sigma_s eps) / max(alpha_s, 1e-10);  x <- a x + b (c1 x0_i + c0 x0_{i-1})

        a = sigma_t / sigma_s, b = -alpha_t expm1(-h_i).  First-order rows (c1 = 1, c0 = 0): row 0, every row when order == 1, the
        last row under `lower_order_final`, and a row whose target level is 1 (there a = 0, b = 1).  Second-order rows: r =
        (lambda_{e_i} - lambda_{e_{i-1}}) / h_i, c1 = 1 + 1/(2r), c0 = -1/(2r).  Everything is formed in float64 and cast once."""
        if order not in (1, 2):
            raise ValueError(f"dpm_schedule: order={order} must be 1 or 2")
        try:
            e = self.ddim_steps(start_step, sampling_steps, steps)
        except ValueError as err:
            raise ValueError(str(err).replace("ddim_schedule:", "dpm_schedule:", 1)) from None
        coef = torch.from_numpy(self.dpm_rows64(e, order, lower_order_final).astype(np.float32)).contiguous()
        st = torch.from_numpy(np.asarray(e, dtype=np.int32))
        return (st.to(device), coef.to(device)) if device is not None else (st, coef)


def dpm_chain_reference(x, eps_fn, steps, coef64):
    """The chain `dpm_schedule`'s rows drive, stepped on the host in whatever precision `x` and `coef64` carry (float64 rows from
    `dpm_rows64` for a reference): eps_fn(x, e_i) -> eps.  Returns the end point."""
    prev = None
    for i, e in enumerate(steps):
        al, sg, a, b, c1, c0 = (coef64[i][j] for j in range(6))
        x0 = (x - sg * eps_fn(x, int(e))) / max(al, 1e-10)
        d = c1 * x0 + (c0 * prev if c0 != 0.0 else 0.0)
        x = a * x + b * d
        prev = x0
    return x


class DDPMScheduler(ScheduleTables):
    """Cosine schedule with the getters of the reference class (latent_module.py:1241-1297).

    Getters return the fp32 value per sample shaped for broadcasting against `shape` (the reference
    materialises the full broadcast; the HIP kernels gather per sample instead)."""

    def __init__(self, timesteps: int, scale: float = 1.0):
        self.scale = scale
        super().__init__(get_named_beta_schedule("cosine", timesteps))

    def _get(self, name, t: torch.Tensor, shape):
        v = self.f32(name, t.device)[t.long()]
        return v.view(-1, *([1] * (len(shape) - 1)))

    def get_beta(self, t, shape):
        return self._get("betas", t, shape)

    def get_sqrt_alpha_cum(self, t, shape):
        return self._get("sqrt_alphas_cumprod", t, shape)

    def get_alpha_cum(self, t, shape):
        return self._get("alphas_cumprod", t, shape)

    def get_alpha_prev_cum(self, t, shape):
        return self._get("alphas_cumprod_prev", t, shape)

    def get_sqrt_one_minus_alpha_cum(self, t, shape):
        return self._get("sqrt_one_minus_alphas_cumprod", t, shape)

    def get_snr(self, t):
        sa = self.get_sqrt_alpha_cum(t, t.shape)
        s1 = self.get_sqrt_one_minus_alpha_cum(t, t.shape)
        return (sa ** 2) / (s1 ** 2)
