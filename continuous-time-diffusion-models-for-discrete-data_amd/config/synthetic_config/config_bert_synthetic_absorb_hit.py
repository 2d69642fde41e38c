"""config_bert_synthetic_absorb with the first-hitting sampler (AbsorbingFirstHit): num_steps = concat_dim = 32, so every forward takes
one event per sample -- the exact sampler of the fixed network, in the 32 forwards config_bert_synthetic_absorb's grid spends;
network, data, objective and schedule unchanged."""
from config.synthetic_config.config_bert_synthetic_absorb import get_config as _base


def get_config():
    c = _base()
    c.sampler.update(name="AbsorbingFirstHit", num_steps=c.model.concat_dim, candidate="sample")
    return c
