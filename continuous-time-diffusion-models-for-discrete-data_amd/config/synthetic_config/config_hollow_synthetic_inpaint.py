"""Synthetic 2-D toy hollow transformer trained to inpaint: InpaintCatRM (ratio matching, reverse_prob logits) with independently
held bits -- the data is not an image, so the mask is "bernoulli" (lib/losses/masks.py) -- sampled with ConditionalLBJF
(`inpaint(model, x_known, mask)`; `sample(model, N, conditioner)` completes the first of the two 16-bit coordinates,
condition_dim = 16).  Everything else is config_hollow_synthetic."""
from config.synthetic_config.config_hollow_synthetic import get_config as _base


def get_config():
    c = _base()
    c.experiment_name = "synthetic_inpaint"
    c.loss.update(name="InpaintCatRM", loss_type="rm", logit_type="reverse_prob", nll_weight=0.0, mask="bernoulli", mask_rate=[0.1, 0.9])
    c.sampler.update(name="ConditionalLBJF", condition_dim=16)
    return c
