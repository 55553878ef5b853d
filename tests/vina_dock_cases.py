"""Inputs shared by test_vina_dock_config.py (restatement) and test_vina_dock_gpu.py (kernel): the trajectory cases of the search and
the boxes of the full runs.  Nothing here depends on an implementation."""
import numpy as np

from .molecule_cases import f32
from .vina_min_cases import case

# The trajectory shape: two chains (the input pose and one random start), three Monte-Carlo steps of at most three iterations each,
# a refinement of at most five.
DOCK_SHAPE = dict(n_chains=2, n_steps=3, n_modes=2)
DOCK_PARAMS = dict(step_iters=3, max_iters=5)
# (case seed, search seed): test_vina_dock_config.py checks on the CPU that the restatement and its reversed-sum twin take the same
# decisions with every margin >= 1e-9 and positions within DOCK_MEASURED_DEV (a pair that fails is replaced there, never on the GPU)
DOCK_SEEDS = ((4, 15), (5, 16), (6, 17), (10, 21))
BOX_ADD = 4.0


def dock_case(seed):
    """(symbols, pos, pocket symbols, pocket pos): a grown ligand of 9 .. 14 atoms in a pocket of 40 atoms in a receptor's frame."""
    return case(seed, lo=9, hi=15, m=40, shift=(20.0, -17.0, 31.0))


def own_box(pos, add=BOX_ADD):
    """The bounding box of an fp32 pose widened by `add`, in fp32: what Molecules.vina_dock takes without box and autobox_ligand."""
    pos = f32(pos)
    return pos.min(axis=0) - np.float32(add), pos.max(axis=0) + np.float32(add)
