"""Hand-made ligands shared by test_molecule_config.py (restatement) and test_molecule_gpu.py (kernels): textbook fragments,
heavy atoms only, built analytically and kept >= 0.02 A away from every threshold of the rule in include/kpd.h.  The expected
bonds and orders are written out by hand, not taken from any implementation."""
import numpy as np

ELEMENTS = ['C', 'N', 'O', 'S', 'P', 'F', 'Cl', 'Br', 'I', 'B']
Z = [6, 7, 8, 16, 15, 9, 17, 35, 53, 5]
ALLOWED = [4, 3, 2, 4, 5, 1, 1, 1, 1, 3]                   # upstream's allowed_bonds maxima for ELEMENTS

TET = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64) / np.sqrt(3.0)
BIPYRAMID = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [-0.5, np.sqrt(0.75), 0], [-0.5, -np.sqrt(0.75), 0]], dtype=np.float64)


def one_hot(symbols):
    f = np.zeros((len(symbols), len(ELEMENTS)), dtype=np.float32)
    f[np.arange(len(symbols)), [ELEMENTS.index(s) for s in symbols]] = 1.0
    return f


def chain(l1, l2, angle_deg):
    """Three atoms a - b - c: b at the origin, a at distance l1 along -x, c at distance l2 at the given a-b-c angle."""
    t = np.deg2rad(angle_deg)
    return np.array([[-l1, 0, 0], [0, 0, 0], [-l2 * np.cos(t), l2 * np.sin(t), 0]], dtype=np.float64)


def star(lengths, directions):
    """Centre at the origin (atom 0), one neighbour per length along the unit directions."""
    return np.concatenate([np.zeros((1, 3)), np.asarray(lengths)[:, None] * directions[:len(lengths)]])


def f32(x):
    return np.asarray(x, dtype=np.float32)


ETHANOL = chain(1.52, 1.43, 109.5)                       # C C O
FIVE = star([1.50, 1.52, 1.54, 1.58, 1.56], BIPYRAMID)  # a carbon with five carbon neighbours; neighbour 4 (1.58 A) is the farthest

# (name, element symbols, positions fp32, {(i, j): order})
TEXTBOOK = [
    ('ethanol', ['C', 'C', 'O'], f32(ETHANOL), {(0, 1): 1, (1, 2): 1}),
    ('acetonitrile', ['C', 'C', 'N'], f32(chain(1.46, 1.15, 180.0)), {(0, 1): 1, (1, 2): 3}),
    ('CO2', ['O', 'C', 'O'], f32(chain(1.20, 1.20, 180.0)), {(0, 1): 2, (1, 2): 2}),
    ('short CO2', ['O', 'C', 'O'], f32(chain(1.13, 1.13, 180.0)), {(0, 1): 2, (1, 2): 2}),
    ('propene', ['C', 'C', 'C'], f32(chain(1.50, 1.34, 124.0)), {(0, 1): 1, (1, 2): 2}),
    ('propyne', ['C', 'C', 'C'], f32(chain(1.46, 1.20, 180.0)), {(0, 1): 1, (1, 2): 3}),
    ('acetamide', ['O', 'C', 'N'], f32(chain(1.22, 1.34, 122.0)), {(0, 1): 2, (1, 2): 1}),
    ('dimethyl sulfone', ['S', 'O', 'O', 'C', 'C'], f32(star([1.44, 1.44, 1.78, 1.78], TET)), {(0, 1): 2, (0, 2): 2, (0, 3): 1, (0, 4): 1}),
    ('phosphate', ['P', 'O', 'O', 'O', 'O'], f32(star([1.48, 1.60, 1.60, 1.60], TET)), {(0, 1): 2, (0, 2): 1, (0, 3): 1, (0, 4): 1}),
    ('CFClBrI', ['C', 'F', 'Cl', 'Br', 'I'], f32(star([1.35, 1.77, 1.94, 2.14], TET)), {(0, 1): 1, (0, 2): 1, (0, 3): 1, (0, 4): 1}),
    # five neighbours: the farthest is dropped and ends isolated (and invalid); centre first, then centre last
    ('five neighbours, centre first', ['C'] * 6, f32(FIVE), {(0, 1): 1, (0, 2): 1, (0, 3): 1, (0, 5): 1}),
    ('five neighbours, centre last', ['C'] * 6, f32(FIVE[[1, 2, 3, 4, 5, 0]]), {(0, 5): 1, (1, 5): 1, (2, 5): 1, (4, 5): 1}),
    # two atoms 0.3 A apart are not bonded to each other; both bond to the third (1.5075 A from each)
    ('0.3 A apart', ['C', 'C', 'C'], f32([[0, 0, 0], [0.3, 0, 0], [0.15, 1.5, 0]]), {(0, 2): 1, (1, 2): 1}),
]

# two ethanols 6 A apart plus a lone Cl: three fragments, the largest 3 of 7 atoms
TWO_ETHANOLS_CL = (['C', 'C', 'O', 'C', 'C', 'O', 'Cl'],
                   f32(np.concatenate([ETHANOL, ETHANOL + np.array([0.0, 0.0, 6.0]), np.array([[6.0, 6.0, 0.0]])])),
                   {(0, 1): 1, (1, 2): 1, (3, 4): 1, (4, 5): 1})
