"""Fixtures for tests/test_group_widths.py: the reference EXECUTED on the configurations of tests/group_width_configs.py (normalised
widths of 16, 48, 80 and 144 channels: GroupNorm groups of 16, 48, 40 and 36).  Build container only (reads the reference):

    python tests/golden/make_golden_groups.py      -> tests/golden/groups.pt

Same inputs, seeds and sampling as make_golden.py --wide (gen_wide), on the other configurations."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _refimport as R  # noqa: E402

R.install()

from diamond_amd.testing import fill_module_, synthetic_actions, synthetic_frames  # noqa: E402


def main():
    from data import Batch
    from models.actor_critic import ActorCritic, ActorCriticConfig
    from models.diffusion import Denoiser, DenoiserConfig, InnerModelConfig, SigmaDistributionConfig
    from models.rew_end_model import RewEndModel, RewEndModelConfig
    from tests import group_width_configs as W

    s = W.SIZE
    out = {}
    # -- denoiser: inference at a scalar and at a per-sample sigma
    den = Denoiser(DenoiserConfig(inner_model=InnerModelConfig(**W.DENOISER), sigma_data=0.5, sigma_offset_noise=0.3))
    fill_module_(den, W.WEIGHT_SEED)
    den.eval()
    g = torch.Generator().manual_seed(5)
    obs, act, x = synthetic_frames(g, 2, 12, s, s), synthetic_actions(g, 4, 2, 4), torch.randn(2, 3, s, s, generator=g)
    with torch.no_grad():
        for i, sigma in enumerate((torch.tensor(0.7), torch.tensor([0.05, 3.0]))):
            out[f"model_output_{i}"] = den.compute_model_output(x, obs, act, den.compute_conditioners(sigma)).clone()
    # -- denoiser: training step
    den.train()
    den.setup_training(SigmaDistributionConfig(**W.SIGMA_DIST))
    g = torch.Generator().manual_seed(31)
    obs, act = synthetic_frames(g, 1, 5, 3, s, s), synthetic_actions(g, 4, 1, 5)
    den.zero_grad()
    torch.manual_seed(77)
    loss, _ = den(Batch(obs=obs, act=act, rew=None, end=None, trunc=None, mask_padding=torch.ones(1, 5, dtype=torch.bool), info=None,
                        segment_ids=None))
    loss.backward()
    out["train"] = {"loss": loss.detach().clone(), "grad_norms": {k: p.grad.double().norm() for k, p in den.named_parameters()},
                    "grads": {k: W.sample_grad(p.grad) for k, p in den.named_parameters()}}
    # -- reward / end model: inference and a training step
    m = RewEndModel(RewEndModelConfig(**W.REW_END))
    fill_module_(m, W.WEIGHT_SEED + 1)
    m.eval()
    g = torch.Generator().manual_seed(9)
    obs, act = synthetic_frames(g, 2, 3, 3, s, s), synthetic_actions(g, 4, 2, 2)
    with torch.no_grad():
        lr, le, (h, c) = m.predict_rew_end(obs[:, :-1], act, obs[:, 1:])
    out["rew_end"] = {"logits_rew": lr.clone(), "logits_end": le.clone(), "h": h.clone(), "c": c.clone()}
    m.train()
    m.zero_grad()
    loss, logs = m(Batch(**W.rew_end_train_batch(torch.Generator().manual_seed(41))))
    loss.backward()
    out["rew_end_train"] = {"loss": loss.detach().clone(), "loss_rew": logs["loss_rew"], "loss_end": logs["loss_end"],
                            "grad_norms": {k: p.grad.double().norm() for k, p in m.named_parameters()},
                            "grads": {k: W.sample_grad(p.grad) for k, p in m.named_parameters()}}
    # -- actor-critic: forward + backward
    ac = ActorCritic(ActorCriticConfig(**W.ACTOR_CRITIC))
    fill_module_(ac, W.WEIGHT_SEED + 2)
    g = torch.Generator().manual_seed(11)
    obs = synthetic_frames(g, 2, 3, s, s)
    o = ac.predict_act_value(obs, None)
    (o.logits_act.square().sum() + o.val.sum()).backward()
    out["actor_critic"] = {"logits": o.logits_act.detach().clone(), "val": o.val.detach().clone(),
                           "grad_norms": {k: p.grad.double().norm() for k, p in ac.named_parameters()},
                           "grads": {k: W.sample_grad(p.grad) for k, p in ac.named_parameters()}}
    path = os.path.join(HERE, "groups.pt")
    torch.save(out, path)
    print(f"wrote groups.pt: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
