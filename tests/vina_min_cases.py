"""Inputs shared by test_vina_min_config.py (restatement) and test_vina_min_gpu.py (kernel): small molecules whose torsion trees are
written out by hand, the mixed batch of the full runs, and the seeds of the gradient and trajectory tests.  Nothing here depends on
an implementation."""
import numpy as np

from .molecule_cases import TWO_ETHANOLS_CL, f32
from .relax_cases import grow, make_pocket
from .vina_cases import biphenyl, chlorobenzene, ethylbenzene, place

# seeds of the gradient test: test_vina_min_config.py asserts that no pair of theirs, ligand x pocket or inside the ligand, lies
# within 1e-3 A of a kink of d or of the cutoff, and that the ligand has rotors and intramolecular pairs
GRAD_SEEDS = (1, 4, 6, 12)
# seeds of the trajectory test: test_vina_min_config.py checks on the CPU that the restatement and its reversed-sum twin take the
# same decisions over five iterations with every margin >= 1e-9 (a seed that fails is replaced there, never on the GPU)
TRAJ_SEEDS = (1, 2, 5, 36)


def hexane():
    """n-hexane, heavy atoms only: 1.53 A bonds, 111 degree angles, dihedrals 180, 65, -170 (three rotors)."""
    p = [np.array([0.0, 0.0, 0.0]), np.array([1.53, 0.0, 0.0])]
    p.append(place([0.0, 1.0, 0.0], p[0], p[1], 1.53, 111.0, 180.0))
    for dih in (180.0, 65.0, -170.0):
        p.append(place(p[-3], p[-2], p[-1], 1.53, 111.0, dih))
    return ['C'] * 6, f32(np.array(p))


# (name, bonds in bond_ij order, frag, rotors (a, b) in active order, moved sets, depth, pieces (lowest atom of each), pairs i < j)
_RING = [(0, 1), (0, 5), (1, 2), (2, 3), (3, 4), (4, 5)]
_RING2 = [(6, 7), (6, 11), (7, 8), (8, 9), (9, 10), (10, 11)]
_D0, _D9 = [0, 1, 2, 3, 2, 1], {6: 3, 7: 2, 8: 1, 9: 0, 10: 1, 11: 2}       # bonds from atom 0 in the first ring, from atom 9 in the second
TREES = [
    ('ethylbenzene', sorted(_RING + [(0, 6), (6, 7)]), [0] * 8, [(0, 6)], [{6, 7}], [1], [0, 0, 0, 0, 0, 0, 6, 6],
     [(2, 7), (3, 6), (3, 7), (4, 7)]),
    ('biphenyl', sorted(_RING + _RING2 + [(0, 9)]), [0] * 12, [(0, 9)], [set(range(6, 12))], [1], [0] * 6 + [6] * 6,
     sorted((i, j) for i in range(6) for j in range(6, 12) if _D0[i] + 1 + _D9[j] >= 4)),
    ('hexane', [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)], [0] * 6, [(1, 2), (2, 3), (3, 4)], [{2, 3, 4, 5}, {3, 4, 5}, {4, 5}], [1, 2, 3],
     [0, 0, 2, 3, 4, 4], [(0, 4), (0, 5), (1, 5)]),
    ('chlorobenzene', sorted(_RING + [(0, 6)]), [0] * 7, [], [], [], [0] * 7, []),
    ('two ethanols + Cl', [(0, 1), (1, 2), (3, 4), (4, 5)], [0, 0, 0, 1, 1, 1, 2], [], [], [], [0, 0, 0, 3, 3, 3, 6],
     sorted([(i, j) for i in range(3) for j in range(3, 7)] + [(i, 6) for i in range(3, 6)])),
    # the chain 1 - 2 - 3 - 0 - 4: the side of j holds atom 0 for the rotor (2, 3), which therefore moves the side of 2
    ('a rotor whose far side holds the lowest atom', [(0, 3), (0, 4), (1, 2), (2, 3)], [0] * 5, [(0, 3), (3, 2)], [{1, 2, 3}, {1, 2}], [1, 2],
     [0, 1, 1, 3, 0], [(1, 4)]),
]


def tree_molecule(name):
    """(symbols, pos) of the TREES entries that have coordinates."""
    rng = np.random.default_rng(2)
    return {'ethylbenzene': ethylbenzene, 'biphenyl': biphenyl, 'chlorobenzene': chlorobenzene, 'hexane': lambda r: hexane(),
            'two ethanols + Cl': lambda r: (TWO_ETHANOLS_CL[0], TWO_ETHANOLS_CL[1])}[name](rng)


def case(seed, lo=9, hi=17, m=60, keep_out=1.5, shift=(0.0, 0.0, 0.0)):
    """(symbols, pos, pocket symbols, pocket pos): a grown ligand of lo .. hi - 1 atoms in a pocket of m atoms, moved by `shift`."""
    rng = np.random.default_rng(4000 + seed)
    sym, pos = grow(rng, int(rng.integers(lo, hi)))
    psym, ppos = make_pocket(rng, m, pos, reach=5.0, keep_out=keep_out)
    return sym, f32(pos + np.array(shift)), psym, f32(ppos + np.array(shift))


def traj_case(seed):
    """One trajectory seed: a pocket of 40 atoms somewhere in a receptor's frame (tens of Angstrom from the origin, where an fp32
    coordinate has an ulp of 2e-6 A)."""
    return case(seed, m=40, shift=(20.0, -17.0, 31.0))


def mixed_batch():
    """Ligands [(symbols, pos)] (ring only, one rotor, three rotors, three bodies, a lone atom, biphenyl, two grown ones of 14 and
    25 atoms), pockets [(symbols, pos)] of 40, 80 and 120 atoms around them, and pocket_of."""
    rng = np.random.default_rng(12)
    ligs = [chlorobenzene(rng), ethylbenzene(rng), hexane(), (TWO_ETHANOLS_CL[0], TWO_ETHANOLS_CL[1]), (['C'], f32([[0.4, -0.3, 0.2]])),
            biphenyl(rng), grow(rng, 14), grow(rng, 25)]
    anchor = np.concatenate([p for _, p in ligs])
    pockets = [make_pocket(rng, m, anchor, reach=4.0, keep_out=1.6) for m in (40, 80, 120)]
    return ligs, pockets, [0, 1, 2, 0, 1, 2, 1, 2]
