"""Maze 15x15 (D=225, S=3) x0-prediction transformer, 12 layers, CT-ELBO + tau-leaping
(reference config/maze_config/config_bert_maze.py)."""
from config._common import skeleton, encoder


def get_config():
    c = skeleton("SavedModels/MAZE")
    c.loss.update(name="CTElbo", eps_ratio=1e-9, nll_weight=0.001, min_time=0.007, one_forward_pass=True)
    c.training.update(n_iters=400000, grad_norm=1, max_t=0.995, resume=True)
    c.data.update(name="Maze3S", S=3, is_img=True, batch_size=128, shuffle=True, train=True, download=True, image_size=15,
                  shape=[1, 15, 15], use_augm=False, crop_wall=False, limit=1, random_transform=True)
    c.model.update(rate_const=1.55, t_func="sqrt_cos")
    encoder(c, "UniVarBertEMA", 128, 12, 1024, 15 * 15, 3, num_output_ffresiduals=4)
    c.saving.checkpoint_freq = 5000
    c.sampler.update(name="ElboTauL", num_steps=1000, min_t=0.007, initial_dist="uniform", sample_freq=200000000)
    return c
