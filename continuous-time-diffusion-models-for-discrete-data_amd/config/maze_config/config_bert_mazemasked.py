"""Maze 15x15 (D=225, S=3) masked transformer, 4 layers, categorical ratio matching + LBJF
(reference config/maze_config/config_bert_mazemasked.py).  One forward is D = 225 encoder passes per sample."""
from config._common import skeleton, encoder


def get_config():
    c = skeleton("SavedModels/MAZE")
    c.loss.update(name="CatRM", loss_type="rm", logit_type="reverse_prob", eps_ratio=1e-9, nll_weight=0.001, min_time=0.007,
                  ce_coeff=0)
    c.training.update(n_iters=400000, grad_norm=1, max_t=0.9999, resume=True)
    c.data.update(name="Maze3S", S=3, is_img=True, batch_size=16, shuffle=True, image_size=15, shape=[1, 15, 15], use_augm=False,
                  crop_wall=False, limit=1, random_transform=True)
    c.model.update(rate_const=1.7, t_func="sqrt_cos")
    encoder(c, "UniVarMaskedEMA", 64, 4, 256, 15 * 15, 3)
    c.saving.checkpoint_freq = 5000
    c.sampler.update(name="LBJF", num_steps=1000, min_t=0.007, initial_dist="uniform", sample_freq=200000000)
    return c
