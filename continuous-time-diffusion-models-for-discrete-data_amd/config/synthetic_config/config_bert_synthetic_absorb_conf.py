"""config_bert_synthetic_absorb with confidence-ordered unmasking (AbsorbingConfidence): 16 sampler steps instead of 32; network,
data, objective and schedule unchanged."""
from config.synthetic_config.config_bert_synthetic_absorb import get_config as _base


def get_config():
    c = _base()
    c.sampler.update(name="AbsorbingConfidence", num_steps=16, conf_temp=1.0, candidate="sample")
    return c
