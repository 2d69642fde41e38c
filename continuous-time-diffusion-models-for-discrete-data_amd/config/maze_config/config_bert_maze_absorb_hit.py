"""config_bert_maze_absorb with the first-hitting sampler (AbsorbingFirstHit): num_steps = concat_dim = 225, so every forward takes one
event per sample -- the exact sampler of the fixed network, in the 225 forwards config_bert_maze_absorb's grid spends; network, data,
objective and schedule unchanged.  A smaller num_steps takes several events per forward and is an approximation."""
from config.maze_config.config_bert_maze_absorb import get_config as _base


def get_config():
    c = _base()
    c.sampler.update(name="AbsorbingFirstHit", num_steps=c.model.concat_dim, candidate="sample")
    return c
