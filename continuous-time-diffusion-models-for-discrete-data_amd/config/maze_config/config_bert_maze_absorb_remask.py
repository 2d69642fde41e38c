"""config_bert_maze_absorb with the remasking sampler (AbsorbingRemask): 32 sampler steps instead of 225, as config_bert_maze_absorb_conf;
network, data, objective and schedule unchanged.  remask_eta = 0.02 is a starting value: it has not been tuned on a trained model."""
from config.maze_config.config_bert_maze_absorb import get_config as _base


def get_config():
    c = _base()
    c.sampler.update(name="AbsorbingRemask", num_steps=32, remask="cap", remask_eta=0.02, remask_temp=1.0)
    return c
