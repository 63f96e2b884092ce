"""Network configurations whose normalised widths are NOT multiples of 32 channels: the reference forms max(1, C // 32) GroupNorm
groups of C / groups channels (models/blocks.py:27,38), i.e. groups of 16 (C = 16), 48 (48), 40 (80) and 36 (144) channels here,
and its U-Net's up path concatenates two such widths (blocks.py:203: list_in_channels = [2 * c2] * n + [c1 + c2]) into tensors
whose 32-channel groups straddle the two sources (cat(144, 80), cat(80, 48), cat(48, 48) ...).  Shared by
tests/golden/make_golden_groups.py (which runs the reference on them) and tests/test_group_widths.py.  Small on purpose: three
levels at 32x32, so that the SIMT interpreter runs a forward + backward in seconds."""

WEIGHT_SEED = 5
DENOISER = dict(img_channels=3, num_steps_conditioning=4, cond_channels=256, depths=[1, 1, 1], channels=[48, 80, 144],
                attn_depths=[0, 0, 1], num_actions=4)
REW_END = dict(lstm_dim=512, img_channels=3, img_size=32, cond_channels=128, depths=[1, 1, 1], channels=[16, 48, 80],
               attn_depths=[0, 0, 1], num_actions=4)
ACTOR_CRITIC = dict(lstm_dim=512, img_channels=3, img_size=32, channels=[16, 48, 80, 144], down=[1, 1, 1, 1], num_actions=4)
SIZE = 32
SIGMA_DIST = dict(loc=-0.4, scale=1.2, sigma_min=2e-3, sigma_max=20)
GRAD_STRIDE = 251  # gradients of more than 2048 elements are stored as every 251st element (plus every tensor's norm)


def sample_grad(g):
    return g if g.numel() <= 2048 else g.flatten()[::GRAD_STRIDE].clone()


def agent_config(AgentConfig, DenoiserConfig, InnerModelConfig, RewEndModelConfig, ActorCriticConfig):
    """The three networks above as one AgentConfig, from the config classes of either package (the reference's or diamond_amd's)"""
    strip = lambda d: {k: v for k, v in d.items() if k != "num_actions"}
    return AgentConfig(denoiser=DenoiserConfig(inner_model=InnerModelConfig(**strip(DENOISER)), sigma_data=0.5, sigma_offset_noise=0.3),
                       rew_end_model=RewEndModelConfig(**strip(REW_END)), actor_critic=ActorCriticConfig(**strip(ACTOR_CRITIC)), num_actions=4)


def rew_end_train_batch(g, b=2, t=4):
    """Synthetic (B, T) segment for RewEndModel.forward at SIZE x SIZE: rewards in {-2..2}, one episode end (sample 1, step 2) with
    its `final_observation`, padded steps behind it (tensors on CPU)."""
    import torch

    from diamond_amd.testing import synthetic_actions, synthetic_frames

    obs = synthetic_frames(g, b, t, 3, SIZE, SIZE)
    act = synthetic_actions(g, 4, b, t)
    rew = torch.randint(-2, 3, (b, t), generator=g).float()
    end = torch.zeros(b, t, dtype=torch.long)
    end[1, 2] = 1
    mask = torch.ones(b, t, dtype=torch.bool)
    mask[1, 3:] = False
    info = [{} for _ in range(b)]
    info[1]["final_observation"] = synthetic_frames(g, 1, 3, SIZE, SIZE)[0]
    return dict(obs=obs, act=act, rew=rew, end=end, trunc=torch.zeros(b, t, dtype=torch.long), mask_padding=mask, info=info,
                segment_ids=None)
