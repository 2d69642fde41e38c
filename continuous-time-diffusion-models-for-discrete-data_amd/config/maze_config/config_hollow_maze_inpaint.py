"""Maze 15x15 hollow transformer trained to inpaint: InpaintScoreElbo under a mixture of masks -- a held half of the maze, a
free or held rectangle, independently held cells (lib/losses/masks.py) -- sampled with ConditionalLBJF, whose
`inpaint(model, x_known, mask)` takes any mask (its `sample(model, N, conditioner)` completes the top 7 rows,
condition_dim = 105).  Everything else is config_hollow_maze."""
from config.maze_config.config_hollow_maze import get_config as _base


def get_config():
    c = _base()
    c.experiment_name = "maze_inpaint"
    c.loss.update(name="InpaintScoreElbo", mask="mixture", mask_mixture=[["half", 1.0], ["box", 1.0], ["bernoulli", 1.0]],
                  mask_rate=[0.1, 0.9])
    c.sampler.update(name="ConditionalLBJF", condition_dim=105)
    return c
