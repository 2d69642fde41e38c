"""Synthetic 2-D toy (D=32, S=2) D3PM baseline: the x0-prediction transformer without a rate class (UniBertD3PM) under a
discrete-time uniform-transition diffusion, T = 500, hybrid loss (reference config/synthetic_config/config_synthetic_d3pm.py)."""
from config._common import skeleton, encoder, d3pm_model


def get_config():
    c = skeleton("SavedModels/Synthetic")
    c.loss.update(name="CTElbo", eps_ratio=1e-9, nll_weight=0, min_time=0.007, ce_coeff=0, one_forward_pass=True)
    c.training.update(n_iters=200000, grad_norm=1, max_t=0.9999, resume=True)
    c.data.update(name="SyntheticData", type="2spirals", is_img=False, S=2, batch_size=128, shuffle=True, binmode="gray",
                  int_scale=6003.0107336488345, plot_size=4.458594271092115, shape=[32],
                  location="lib/datasets/Synthetic/data_2spirals.npy")
    c.model.update(rate_const=2, t_func="sqrt_cos")
    encoder(c, "UniBertD3PM", 64, 3, 256, 32, 2)
    c.model.update(use_one_hot_input=True, use_cat=True)        # (the one-hot input layer: outside the HIP inference plan, torch device ops)
    d3pm_model(c, 2, 500, "uniform", 0.02, 1, 0.01, False, fused=True)
    c.saving.checkpoint_freq = 10000
    c.sampler.update(name="ElboTauL", num_steps=1000, min_t=0.007, initial_dist="uniform", sample_freq=200000000, is_ordinal=False)
    return c
