"""Mask distributions of InpaintCTElbo: named samplers of the (B, D) bool tensor `free` (True = the entry is noised and
carries the objective, False = it is held at its data value), the training-time counterpart of the `mask` argument of the
samplers' `inpaint(model, x_known, mask)` (there True = held).

Every sampler draws on the host from torch's global CPU generator -- `torch.manual_seed` reproduces the masks, the number of
free entries is known without asking the device, and the mask is uploaded once per training step -- and leaves at least one
free entry in every sample.

cfg.loss.mask names the distribution:
  "prefix"     the first cfg.loss.condition_dim entries are held (CondCTElbo's split);
  "bernoulli"  each entry is held independently with a per-sample rate r ~ U(lo, hi), (lo, hi) = cfg.loss.mask_rate;
  "half"       the top, bottom, left or right half of the image is held (cfg.data.shape = (C, H, W), same in every channel);
  "box"        a uniformly drawn axis-aligned rectangle is the free set, or the held set, with equal probability;
  "mixture"    every sample draws its distribution from cfg.loss.mask_mixture = [(name, weight), ...].
"""
import torch


def _image_shape(cfg, D, name):
    shape = getattr(getattr(cfg, "data", None), "shape", None)
    if shape is None or len(shape) != 3:
        raise ValueError(f"mask {name!r} needs image data: cfg.data.shape = (C, H, W), got {shape!r}")
    C, H, W = (int(v) for v in shape)
    if min(C, H, W) < 1 or C * H * W != D:
        raise ValueError(f"mask {name!r}: cfg.data.shape = {tuple(shape)} against D = {D}")
    return C, H, W


def _over_channels(free_hw, C):
    """(n, H, W) -> (n, C * H * W), the row-major flattening of the minibatch."""
    n = free_hw.shape[0]
    return free_hw.unsqueeze(1).expand(n, C, *free_hw.shape[1:]).reshape(n, -1)


def _prefix_args(cfg, D):
    k = getattr(cfg.loss, "condition_dim", None)
    if not (isinstance(k, int) and not isinstance(k, bool) and 0 < k < D):
        raise ValueError(f"mask 'prefix': loss.condition_dim must be an integer in (0, {D}), got {k!r}")
    return k


def _prefix(cfg, n, D):
    free = torch.ones((n, D), dtype=torch.bool)
    free[:, :_prefix_args(cfg, D)] = False
    return free


def _bernoulli_args(cfg, D):
    r = getattr(cfg.loss, "mask_rate", None)
    try:
        lo, hi = (float(v) for v in r)
    except (TypeError, ValueError):
        raise ValueError(f"mask 'bernoulli': loss.mask_rate must be a (lo, hi) pair, got {r!r}") from None
    if not 0.0 <= lo <= hi <= 1.0:
        raise ValueError(f"mask 'bernoulli': loss.mask_rate must satisfy 0 <= lo <= hi <= 1, got {r!r}")
    return lo, hi


def _bernoulli(cfg, n, D):
    lo, hi = _bernoulli_args(cfg, D)
    rate = torch.rand((n, 1)) * (hi - lo) + lo
    free = torch.rand((n, D)) >= rate
    pick = torch.randint(0, D, (n,))                    # a sample that held everything frees one entry, uniformly
    none = ~free.any(dim=1)
    free[none, pick[none]] = True
    return free


def _half_args(cfg, D):
    C, H, W = _image_shape(cfg, D, "half")
    sides = ([0, 1] if H >= 2 else []) + ([2, 3] if W >= 2 else [])
    if not sides:
        raise ValueError(f"mask 'half': a {H} x {W} image has no halves")
    return C, H, W, torch.tensor(sides)


def _half(cfg, n, D):
    C, H, W, sides = _half_args(cfg, D)
    side = sides[torch.randint(0, len(sides), (n,))].view(n, 1, 1)       # 0 top, 1 bottom, 2 left, 3 right is held
    r, c = torch.arange(H).view(1, H, 1), torch.arange(W).view(1, 1, W)
    held = ((side == 0) & (r < H // 2)) | ((side == 1) & (r >= H // 2)) | ((side == 2) & (c < W // 2)) | ((side == 3) & (c >= W // 2))
    return _over_channels(~held, C)


def _box_args(cfg, D):
    return _image_shape(cfg, D, "box")


def _box(cfg, n, D):
    C, H, W = _box_args(cfg, D)

    def span(L):
        size = torch.randint(1, L + 1, (n,))
        start = torch.minimum(torch.floor(torch.rand((n,)) * (L - size + 1).float()).long(), L - size)
        i = torch.arange(L).view(1, L)
        return (i >= start.view(n, 1)) & (i < (start + size).view(n, 1))
    box = span(H).view(n, H, 1) & span(W).view(n, 1, W)
    box_is_free = torch.rand((n,)) < 0.5
    box_is_free |= box.view(n, -1).all(dim=1)           # (a held box over the whole image would leave nothing free)
    return _over_channels(torch.where(box_is_free.view(n, 1, 1), box, ~box), C)


def _mixture_args(cfg, D):
    mix = getattr(cfg.loss, "mask_mixture", None)
    try:
        parts = [(str(name), float(w)) for name, w in mix]
    except (TypeError, ValueError):
        raise ValueError(f"mask 'mixture': loss.mask_mixture must be a list of (name, weight), got {mix!r}") from None
    if not parts or any(w < 0 for _, w in parts) or sum(w for _, w in parts) <= 0:
        raise ValueError(f"mask 'mixture': loss.mask_mixture needs non-negative weights with a positive sum, got {mix!r}")
    for name, _ in parts:
        if name == "mixture" or name not in MASKS:
            raise ValueError(f"mask 'mixture': unknown component {name!r} (one of {sorted(set(MASKS) - {'mixture'})})")
        MASKS[name][1](cfg, D)
    return parts


def _mixture(cfg, n, D):
    parts = _mixture_args(cfg, D)
    which = torch.multinomial(torch.tensor([w for _, w in parts], dtype=torch.float64), n, replacement=True)
    free = torch.empty((n, D), dtype=torch.bool)
    for j, (name, _) in enumerate(parts):
        idx = (which == j).nonzero().view(-1)
        if idx.numel():
            free[idx] = MASKS[name][0](cfg, int(idx.numel()), D)
    return free


MASKS = {"prefix": (_prefix, _prefix_args), "bernoulli": (_bernoulli, _bernoulli_args), "half": (_half, _half_args),
         "box": (_box, _box_args), "mixture": (_mixture, _mixture_args)}          # name -> (sampler, argument check)


def check_mask_config(cfg, D):
    """ValueError unless cfg.loss.mask names a distribution whose fields are usable for D-entry samples.  No device work."""
    name = getattr(cfg.loss, "mask", None)
    if not isinstance(name, str) or name not in MASKS:
        raise ValueError(f"loss.mask must be one of {sorted(MASKS)}, got {name!r}")
    if not (isinstance(D, int) and D >= 1):
        raise ValueError(f"mask {name!r}: D = {D!r}")
    MASKS[name][1](cfg, D)
    return name


def sample_free(cfg, B, D):
    """(B, D) bool on the host: True where the entry is free.  At least one True per row."""
    name = check_mask_config(cfg, D)
    if not (isinstance(B, int) and B >= 1):
        raise ValueError(f"mask {name!r}: B = {B!r}")
    free = MASKS[name][0](cfg, B, D)
    assert free.shape == (B, D) and free.dtype == torch.bool
    return free.contiguous()
