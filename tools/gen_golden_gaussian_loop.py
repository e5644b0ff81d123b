#!/usr/bin/env python3
"""Golden vectors for the generic Gaussian scheduler's device loop, dn_gaussian_loop (the method of oracle/gen_golden_ddpm.py): the
REAL reference's SpacedDiffusion (diffusion/respace.py:63-129) -- "ddim5" over 100 steps of the cosine schedule, eps-prediction, fixed
large variance -- running its own p_sample_loop and ddim_sample_loop (eta = 0.5), clip_denoised=False, over the REAL reference
eps-predictor (latent_module.Model, the chain-sized config), with every torch.randn_like the loops draw recorded (the injected noise
of the parity run).  Writes tests/golden/gaussian_loop.npz: arrays only.
Run in the build container only: python tools/gen_golden_gaussian_loop.py"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import diffnorm_oracle as O  # noqa: E402
import ref_loader  # noqa: E402
from gen_golden import record_draws, ref_eps_model, save  # noqa: E402
from gen_golden_configs import CHAIN_EPS, seeded  # noqa: E402

TIMESTEPS, RESPACING, ETA = 100, "ddim5", 0.5
B, T = 3, 24
LENS = (24, 17, 9)


def main():
    lm, gd = ref_loader.load_reference()
    G, R = sys.modules["refdiffusion.gaussian_diffusion"], sys.modules["refdiffusion.respace"]
    cfg = CHAIN_EPS
    model = ref_eps_model(lm, cfg, O.make_eps_state_dict(cfg, "chain"))
    lens = torch.tensor(LENS)
    mask = O.lengths_to_mask(lens, T)
    diff = R.SpacedDiffusion(use_timesteps=R.space_timesteps(TIMESTEPS, RESPACING), betas=lm.get_named_beta_schedule("cosine", TIMESTEPS),
                             model_mean_type=G.ModelMeanType.EPSILON, model_var_type=G.ModelVarType.FIXED_LARGE, loss_type=G.LossType.MSE)
    fn = lambda x, t: model(x, t, input_mask=mask, cond_drop_prob=0)  # noqa: E731  (elementwise scheduler: the [B,T,z] layout is fine)
    x_T = seeded((B, T, cfg.latent_dim), 91)
    out = dict(lens=lens, timestep_map=torch.tensor(diff.timestep_map), x_T=x_T, eta=torch.tensor(ETA))
    torch.manual_seed(400)
    for name, run in (("p_sample", lambda: diff.p_sample_loop(fn, x_T.shape, noise=x_T, clip_denoised=False, device="cpu")),
                      ("ddim", lambda: diff.ddim_sample_loop(fn, x_T.shape, noise=x_T, clip_denoised=False, device="cpu", eta=ETA))):
        with torch.no_grad(), record_draws() as rec:
            x = run()
        assert len(rec.draws) == diff.num_timesteps and all(d.shape == x_T.shape for d in rec.draws)
        out[f"{name}_noise"] = torch.stack(rec.draws)  # row k belongs to the k-th update, respaced index num_timesteps-1-k
        out[f"{name}_out"] = x
    save("gaussian_loop", **out)


if __name__ == "__main__":
    main()
