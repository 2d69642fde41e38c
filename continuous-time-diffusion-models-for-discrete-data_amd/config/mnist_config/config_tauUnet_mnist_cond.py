"""MNIST tauLDR U-Net trained to complete a held prefix: CondCTElbo on the bottom 14 rows given the top 14 (392 of the 784
row-major pixels), sampled with ConditionalTauLeaping (reference lib/losses/losses.py:547-781, lib/sampling/sampling.py:649-758).
Everything else is config_tauUnet_mnist."""
from config.mnist_config.config_tauUnet_mnist import get_config as _base


def get_config():
    c = _base()
    c.experiment_name = "mnist_cond"
    c.loss.update(name="CondCTElbo", condition_dim=392)
    c.sampler.update(name="ConditionalTauLeaping", condition_dim=392)
    return c
