"""Fixtures for tests/test_offgrid_train.py: the reference's world-model TRAINING steps EXECUTED at image sizes whose U-Net /
encoder levels are not multiples of the kernels' 8-pixel tiles.  Build container only (reads the reference):

    python tests/golden/make_golden_offgrid_train.py

writes
    denoiser_train_72x72.pt            Denoiser.forward + backward, default configuration, 72x72 (levels 72 / 36 / 18 / 9)
    denoiser_train_attn0011_68x76.pt   the same with attention at the two deepest levels, 68x76 frames (the reference pads them to
                                       72x80 inside UNet.forward and crops, blocks.py:227-229,247)
    rew_end_train_72x72.pt             RewEndModel.forward + backward, img_size 72 (attention at 9x9)

Inputs, seeds and the stored quantities are those of make_golden.py's gen_denoiser_train / gen_rew_end_train.  Gradients of more
than 4,096 elements are stored as every `stride`-th element (13, as in denoiser_train.pt, unless the file would exceed 1 MiB) plus
their exact fp64 norms."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import ref_agent, save  # noqa: E402  (installs the reference's import stubs)

from diamond_amd.testing import rew_end_train_batch, synthetic_actions, synthetic_frames  # noqa: E402

MAX_BYTES = 1 << 20


def _sampled(grads, numel_budget):
    """every stride-th element of the tensors larger than 4,096 elements: the smallest stride >= 13 that fits the budget"""
    stride = 13
    while sum(v.numel() if v.numel() <= 4096 else (v.numel() + stride - 1) // stride for v in grads.values()) > numel_budget:
        stride += 2
    return stride, {k: (v if v.numel() <= 4096 else v.flatten()[::stride].clone()) for k, v in grads.items()}


def _save_train(name, out, grads):
    out["grad_norms"] = {k: v.double().norm() for k, v in grads.items()}
    out["stride"], out["grads"] = _sampled(grads, (3 * MAX_BYTES // 4) // 4)  # (a quarter for the names, norms and pickling)
    save(name, out)
    assert os.path.getsize(os.path.join(HERE, name)) < MAX_BYTES, name


def gen_denoiser_train(name, h, w, b, t, attn_depths=(0, 0, 0, 0)):
    from data import Batch
    from models.diffusion import SigmaDistributionConfig

    agent = ref_agent(denoiser_attn_depths=attn_depths)
    den = agent.denoiser
    den.setup_training(SigmaDistributionConfig(loc=-0.4, scale=1.2, sigma_min=2e-3, sigma_max=20))
    g = torch.Generator().manual_seed(31)
    obs = synthetic_frames(g, b, t, 3, h, w)
    act = synthetic_actions(g, 4, b, t)
    mask = torch.ones(b, t, dtype=torch.bool)
    if b > 1:
        mask[1, t - 1] = False  # a padded step: excluded from the loss of the last prediction
    batch = Batch(obs=obs, act=act, rew=None, end=None, trunc=None, mask_padding=mask, info=None, segment_ids=None)
    den.zero_grad()
    torch.manual_seed(77)  # consumed by sample_sigma / apply_noise (denoiser.py:55,62-63)
    loss, _ = den(batch)
    loss.backward()
    grads = {k: p.grad.clone() for k, p in den.named_parameters()}
    assert all(v is not None for v in grads.values())
    _save_train(name, {"seed": 31, "rng_seed": 77, "b": b, "t": t, "h": h, "w": w, "attn_depths": tuple(attn_depths),
                       "mask": mask, "loss": loss.detach()}, grads)
    print(f"{name}: loss", float(loss))


def gen_rew_end_train(name, size):
    from data import Batch

    agent = ref_agent(img_size=size)
    m = agent.rew_end_model
    g = torch.Generator().manual_seed(41)
    batch = Batch(**rew_end_train_batch(g, h=size, w=size))
    m.zero_grad()
    loss, logs = m(batch)
    loss.backward()
    grads = {k: p.grad.clone() for k, p in m.named_parameters()}
    assert all(v is not None for v in grads.values())
    _save_train(name, {"seed": 41, "size": size, "loss": loss.detach(), "loss_rew": logs["loss_rew"], "loss_end": logs["loss_end"],
                       "cm_rew": logs["confusion_matrix"]["rew"], "cm_end": logs["confusion_matrix"]["end"]}, grads)
    print(f"{name}: loss", float(loss), "cm_rew", logs["confusion_matrix"]["rew"].tolist())


def main():
    gen_denoiser_train("denoiser_train_72x72.pt", 72, 72, b=2, t=6)
    gen_denoiser_train("denoiser_train_attn0011_68x76.pt", 68, 76, b=1, t=5, attn_depths=(0, 0, 1, 1))
    gen_rew_end_train("rew_end_train_72x72.pt", 72)


if __name__ == "__main__":
    main()
