"""config_bert_synthetic_absorb with the remasking sampler (AbsorbingRemask); network, data, objective, schedule and the 32 sampler
steps unchanged.  remask_eta = 0.02 is a starting value: it has not been tuned on a trained model."""
from config.synthetic_config.config_bert_synthetic_absorb import get_config as _base


def get_config():
    c = _base()
    c.sampler.update(name="AbsorbingRemask", remask="cap", remask_eta=0.02, remask_temp=1.0)
    return c
