"""Regenerate tests/golden/bert.npz: reference logits of tiny x0-prediction ("BERT") and masked transformer score models.

Runs only where the reference checkout is present: it is imported through oracle/stubs with the helpers of oracle/gen_golden.py.
Weights are re-drawn (matrices ~ N(0, 1/fan_in), the masked nets' output layer four times that, norm gains ~ 1, the rest small) so that the logits are O(1); every case
asserts max|out| >= 1, since the tests hold the engine to an absolute bar.

    python tools/gen_golden_bert.py
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle.gen_golden import base_cfg, ref_mu, save  # noqa: E402  (puts the reference and its stubs on sys.path)

#        tag         model name         S   D   E  layers heads mlp n_res readout conditional_dim
CASES = (("bert_a", "UniVarBertEMA", 3, 12, 32, 2, 4, 32, 1, "resnet", 0),
         ("bert_b", "UniformBertEMA", 5, 17, 64, 1, 4, 16, 0, "resnet", 0),
         ("mask_a", "UniVarMaskedEMA", 3, 12, 16, 2, 4, 32, 2, "resnet", 0),
         ("mask_c", "UniVarMaskedEMA", 2, 16, 16, 1, 4, 16, 1, "resnet", 4),
         ("mask_mlp", "UniVarMaskedEMA", 3, 8, 16, 1, 4, 16, 0, "mlp", 0))


def main():
    import lib.models.models  # noqa: F401  (the reference's registry)
    arrs = {}
    for tag, mname, S, D, E, layers, heads, mlp, n_res, readout, cdim in CASES:
        cfg = base_cfg(S, D, mname)
        meta = dict(S=S, D=D, embed_dim=E, num_layers=layers, num_heads=heads, mlp_dim=mlp, num_output_ffresiduals=n_res,
                    readout=readout, conditional_dim=cdim, time_scale_factor=1000, t_func="sqrt_cos", rate_const=1.7, name=mname)
        cfg.model.update(dict(use_cat=False, use_one_hot_input=False, embed_dim=E, readout=readout, dropout_rate=0.1, num_layers=layers,
                              num_heads=heads, attention_dropout_rate=0.1, transformer_norm_type="prenorm", mlp_dim=mlp, out_dim=S,
                              readout_dim=S, num_output_ffresiduals=n_res, qkv_dim=E, ema_decay=0.999, time_scale_factor=1000,
                              is_ebm=False, conditional_dim=cdim))
        torch.manual_seed(31)
        model = ref_mu.create_model(cfg, torch.device("cpu"))
        g = torch.Generator().manual_seed(32)
        with torch.no_grad():
            for name, p in model.named_parameters():
                gain = name.endswith("weight") and ("norm" in name or name.split(".")[-2].isdigit() and "resid_layers" in name)
                last = tag.startswith("mask") and ("logits_layer" in name or ".model.layers.2." in name)   # their output layer: x 4 (max|logit| >= 1)
                if p.dim() > 1:
                    p.copy_(torch.randn(p.shape, generator=g) * ((4.0 if last else 1.0) / math.sqrt(p.shape[-1])))
                elif last:
                    p.copy_(torch.randn(p.shape, generator=g))
                elif gain:
                    p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
                else:
                    p.copy_(0.1 * torch.randn(p.shape, generator=g))
        model.init_ema()
        model.eval()
        x = torch.randint(0, S, (3, D), generator=g)
        t = torch.tensor([0.05, 0.5, 0.97])
        with torch.no_grad():
            out = model(x, t)
        assert out.shape == (3, D, S) and float(out.abs().max()) >= 1.0, (tag, out.shape, float(out.abs().max()))
        if cdim:
            assert float(out[:, :cdim].abs().max()) == 0.0
        print(tag, "max|out|", float(out.abs().max()), "params", sum(p.numel() for p in model.parameters()))
        sd = {k: v for k, v in model.state_dict().items() if isinstance(v, torch.Tensor)}
        arrs.update({f"{tag}__x": x, f"{tag}__t": t, f"{tag}__out": out})
        arrs.update({f"{tag}__sd__{k}": v for k, v in sd.items()})
        arrs[f"{tag}__cfg"] = np.array(repr(meta))
    save("bert", **arrs)


if __name__ == "__main__":
    main()
