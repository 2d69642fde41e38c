"""MNIST tauLDR U-Net trained to inpaint: InpaintCTElbo under a mixture of masks -- a held half of the image, a free or held
rectangle, independently held pixels (lib/losses/masks.py) -- sampled with ConditionalTauLeaping, whose
`inpaint(model, x_known, mask)` takes any mask (its `sample(model, N, conditioner)` completes the top half, condition_dim = 392).
Everything else is config_tauUnet_mnist."""
from config.mnist_config.config_tauUnet_mnist import get_config as _base


def get_config():
    c = _base()
    c.experiment_name = "mnist_inpaint"
    c.loss.update(name="InpaintCTElbo", mask="mixture", mask_mixture=[["half", 1.0], ["box", 1.0], ["bernoulli", 1.0]],
                  mask_rate=[0.1, 0.9])
    c.sampler.update(name="ConditionalTauLeaping", condition_dim=392)
    return c
