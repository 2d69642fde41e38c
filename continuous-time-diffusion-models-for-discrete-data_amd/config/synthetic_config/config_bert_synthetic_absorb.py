"""Synthetic 2-D toy (D=32, two real states + the mask state: S=3) x0-prediction transformer, 3 layers, absorbing-state
("masked") diffusion: AbsorbingElbo + AbsorbingLeap (no counterpart in the reference; network and data as config_bert_synthetic)."""
from config._common import skeleton, encoder


def get_config():
    c = skeleton("SavedModels/Synthetic")
    c.loss.update(name="AbsorbingElbo", nll_weight=0, min_time=0.007)
    c.training.update(n_iters=200000, grad_norm=1, max_t=0.9999, resume=True)
    c.data.update(name="SyntheticData", type="2spirals", is_img=False, S=3, batch_size=128, shuffle=True, binmode="gray",
                  int_scale=6003.0107336488345, plot_size=4.458594271092115, shape=[32],
                  location="lib/datasets/Synthetic/data_2spirals.npy")
    c.model.update(rate_const=1, t_func="loglinear", alpha_eps=1e-3, mask_state=2)
    encoder(c, "AbsorbingBertEMA", 64, 3, 256, 32, 3)
    c.optimizer.lr = 1.5e-4
    c.saving.checkpoint_freq = 20000
    c.sampler.update(name="AbsorbingLeap", rule="ancestral", num_steps=32, min_t=0.007, initial_dist="absorbing",
                     sample_freq=200000000)
    return c
