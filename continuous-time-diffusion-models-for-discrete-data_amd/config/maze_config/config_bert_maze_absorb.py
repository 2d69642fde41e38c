"""Maze 15x15 (D=225, three real states + the mask state: S=4) x0-prediction transformer, 12 layers, absorbing-state
("masked") diffusion: AbsorbingElbo + AbsorbingLeap (no counterpart in the reference; network and data as config_bert_maze)."""
from config._common import skeleton, encoder


def get_config():
    c = skeleton("SavedModels/MAZE")
    c.loss.update(name="AbsorbingElbo", nll_weight=0.001, min_time=0.007)
    c.training.update(n_iters=400000, grad_norm=1, max_t=0.995, resume=True)
    c.data.update(name="Maze3S", S=4, is_img=True, batch_size=128, shuffle=True, train=True, download=True, image_size=15,
                  shape=[1, 15, 15], use_augm=False, crop_wall=False, limit=1, random_transform=True)
    c.model.update(rate_const=1, t_func="loglinear", alpha_eps=1e-3, mask_state=3)
    encoder(c, "AbsorbingBertEMA", 128, 12, 1024, 15 * 15, 4, num_output_ffresiduals=4)
    c.saving.checkpoint_freq = 5000
    c.sampler.update(name="AbsorbingLeap", rule="ancestral", num_steps=225, min_t=0.007, initial_dist="absorbing",
                     sample_freq=200000000)
    return c
