"""MNIST D3PM baseline (D=784, S=256): the tauLDR U-Net as x_start predictor under a discrete-time Gaussian-transition
diffusion, T = 1000, hybrid loss (reference config/mnist_config/config_mnist_d3pm.py).  The scripts build the objective as
`d3pm_loss(cfg, make_diffusion(cfg.model))`; cfg.loss / cfg.sampler are carried for the bookkeeping that prints them."""
from config._common import skeleton, image_data, tau_unet, d3pm_model


def get_config():
    c = skeleton("SavedModels/MNIST/")
    c.experiment_name = "mnist"
    c.init_model_path = None
    c.loss.update(name="CTElbo", eps_ratio=1e-9, nll_weight=0, min_time=0.01, one_forward_pass=True)
    c.training.update(n_iters=600000, grad_norm=2, max_t=1)
    image_data(c, "DiscreteMNIST", 256, 28, 1, 64)
    c.data.random_flips = True
    tau_unet(c, 96, [1, 2, 2], 1, 28, "logits")
    d3pm_model(c, 256, 1000, "gaussian", 1e-4, 0.02, 0.001, True, fused=True)
    c.saving.checkpoint_freq = 10000
    c.sampler.update(name="ElboTauL", num_steps=1000, min_t=0.01, initial_dist="uniform", sample_freq=200000000, is_ordinal=False)
    return c
