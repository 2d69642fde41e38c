"""Synthetic 2-D toy (D=32, S=2) masked transformer, 4 layers, CatRMNLL + LBJF
(reference config/synthetic_config/config_masked_synthetic.py).  One forward at batch 128 is 4096 sequences of 33 tokens."""
from config._common import skeleton, encoder


def get_config():
    c = skeleton("SavedModels/Synthetic")
    c.loss.update(name="CatRMNLL", loss_type="rm", logit_type="reverse_prob", eps_ratio=1e-9, nll_weight=0.001, min_time=0.007,
                  ce_coeff=0)
    c.training.update(n_iters=200000, grad_norm=3, max_t=0.007, resume=True)
    c.data.update(name="SyntheticData", type="2spirals", is_img=False, S=2, batch_size=128, shuffle=True, binmode="gray",
                  int_scale=6003.0107336488345, plot_size=4.458594271092115, shape=[32],
                  location="lib/datasets/Synthetic/data_2spirals.npy")
    c.model.update(rate_const=1.7, t_func="sqrt_cos")
    encoder(c, "UniVarMaskedEMA", 64, 4, 256, 32, 2)
    c.optimizer.lr = 1.5e-4
    c.saving.checkpoint_freq = 10000
    c.sampler.update(name="LBJF", num_steps=500, min_t=0.007, initial_dist="uniform", sample_freq=200000000, is_ordinal=False)
    return c
