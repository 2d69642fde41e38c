"""config_bert_maze_absorb with confidence-ordered unmasking (AbsorbingConfidence): 32 sampler steps instead of 225; network, data,
objective and schedule unchanged."""
from config.maze_config.config_bert_maze_absorb import get_config as _base


def get_config():
    c = _base()
    c.sampler.update(name="AbsorbingConfidence", num_steps=32, conf_temp=1.0, candidate="sample")
    return c
