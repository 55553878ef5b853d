"""Inputs shared by test_vina_config.py (restatement) and test_vina_gpu.py (kernels): radii for the test elements, hand-made
molecules whose types and rotor counts are written out by hand, a Gly-Ser-Pro fragment built from ideal bond lengths, and the
seeds of the gradient test.  Nothing here depends on an implementation."""
import numpy as np

from .molecule_cases import BIPYRAMID, ELEMENTS, TET, TEXTBOOK, Z, f32, star
from .relax_cases import grow, make_pocket, ring6

H, D, A = 1, 2, 4
# a radius per element of ELEMENTS and of the pockets: any positive numbers would do, nothing relies on their being Vina's
RADII = {'C': 1.9, 'N': 1.8, 'O': 1.7, 'S': 2.0, 'P': 2.1, 'F': 1.5, 'Cl': 1.8, 'Br': 2.0, 'I': 2.2, 'B': 2.0, 'Zn': 1.2}
LIG_RADIUS = np.array([RADII[e] for e in ELEMENTS], dtype=np.float32)                # [F], the kernel's lig_radius
ZMAP = dict(zip(ELEMENTS, Z), Zn=30, H=1)

# seeds of the gradient test: test_vina_config.py asserts that no pair of theirs lies within 1e-3 A of a kink of d or of the cutoff
# and that all five terms are at work
GRAD_SEEDS = (6, 7, 13, 14, 21, 22, 24, 25)


def radii_of(symbols):
    return np.array([RADII[s] for s in symbols], dtype=np.float32)


def z_of(symbols):
    return np.array([ZMAP[s] for s in symbols], dtype=np.int64)


def grad_case(seed):
    """(symbols, pos, pocket symbols, pocket pos): a 12-atom ligand in a 60-atom pocket."""
    rng = np.random.default_rng(1000 + seed)
    sym, pos = grow(rng, 12)
    psym, ppos = make_pocket(rng, 60, pos, reach=5.0, keep_out=1.5)
    return sym, pos, psym, ppos


def biphenyl(rng):
    """Two six-rings in one plane joined by a 1.48 A bond between atom 0 of the first and atom 3 of the second (atom 9)."""
    a, b = ring6(rng)[1], ring6(rng)[1]
    return ['C'] * 12, f32(np.concatenate([a, b + np.array([4.28, 0.0, 0.0], dtype=np.float32)]))


def ethylbenzene(rng):
    ring = ring6(rng)[1]
    return ['C'] * 8, f32(np.concatenate([ring, [[2.91, 0.0, 0.0], [3.43, 1.44, 0.0]]]))


def chlorobenzene(rng):
    return ['C'] * 6 + ['Cl'], f32(np.concatenate([ring6(rng)[1], [[3.14, 0.0, 0.0]]]))


_PLANE = BIPYRAMID[2:]                                    # three directions 120 degrees apart
# (name, symbols, pos, expected types)
TYPED = [
    ('ethanol', TEXTBOOK[0][1], TEXTBOOK[0][2], [H, 0, D | A]),
    ('acetone', ['C', 'C', 'C', 'O'], f32(star([1.51, 1.51, 1.22], _PLANE)), [0, H, H, A]),
    ('acetonitrile', TEXTBOOK[1][1], TEXTBOOK[1][2], [H, 0, A]),
    ('trimethylamine', ['N', 'C', 'C', 'C'], f32(star([1.47, 1.47, 1.47], TET)), [0, 0, 0, 0]),
    ('methylamine', ['C', 'N'], f32([[0, 0, 0], [1.47, 0, 0]]), [0, D]),
    ('chlorobenzene',) + chlorobenzene(np.random.default_rng(2)) + ([0, H, H, H, H, H, H],),
]

# (name, atomic numbers, bonds, orders, N_rot): graphs written out by hand
_RING = [(k, (k + 1) % 6) for k in range(6)]
ROTOR_GRAPHS = [
    ('butane', [6] * 4, [(0, 1), (1, 2), (2, 3)], [1, 1, 1], 1),
    ('propane', [6] * 3, [(0, 1), (1, 2)], [1, 1], 0),
    ('cyclohexane', [6] * 6, _RING, [1] * 6, 0),
    ('biphenyl', [6] * 12, _RING + [(6 + i, 6 + j) for i, j in _RING] + [(0, 9)], [1] * 13, 1),
    ('ethylbenzene', [6] * 8, _RING + [(0, 6), (6, 7)], [1] * 8, 1),
    ('two ethanols + Cl', [6, 6, 8, 6, 6, 8, 17], [(0, 1), (1, 2), (3, 4), (4, 5)], [1] * 4, 0),
    ('two three-rings joined by a bridge', [6] * 6, [(0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (3, 5), (2, 3)], [1] * 7, 1),
    ('decalin: the shared bond is in both rings', [6] * 10, _RING + [(0, 6), (6, 7), (7, 8), (8, 9), (9, 1)], [1] * 11, 0),
    ('2-butene: the double bond is no rotor', [6] * 4, [(0, 1), (1, 2), (2, 3)], [1, 2, 1], 0),
    ('a hydrogen does not make a heavy degree', [6, 6, 6, 1], [(0, 1), (1, 2), (2, 3)], [1, 1, 1], 0),
]


def place(a, b, c, length, angle_deg, dihedral_deg):
    """The point d with |cd| = length, angle b-c-d and dihedral a-b-c-d (natural extension reference frame)."""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in (a, b, c))
    t, p = np.deg2rad(angle_deg), np.deg2rad(dihedral_deg)
    bc = (c - b) / np.linalg.norm(c - b)
    nrm = np.cross(b - a, bc)
    nrm /= np.linalg.norm(nrm)
    m = np.cross(nrm, bc)
    d2 = np.array([-length * np.cos(t), length * np.sin(t) * np.cos(p), length * np.sin(t) * np.sin(p)])
    return c + d2[0] * bc + d2[1] * m + d2[2] * nrm


def gly_ser_pro():
    """A Gly-Ser-Pro fragment, heavy atoms only, from ideal bond lengths (N-CA 1.458, CA-C 1.525, C-N 1.329, C=O 1.231, CA-CB 1.53,
    CB-OG 1.417) in an extended conformation; the proline ring is an envelope closed by CD-N (1.47 A).
    Returns (names, symbols, pos float32, bonds as a set of index pairs, expected types by name)."""
    names, pos = [], []

    def add(name, p):
        names.append(name)
        pos.append(np.asarray(p, dtype=np.float64))
        return len(pos) - 1

    n1 = add('GLY N', [0.0, 0.0, 0.0])
    ca1 = add('GLY CA', [1.458, 0.0, 0.0])
    c1 = add('GLY C', place([0.0, 1.0, 0.0], pos[n1], pos[ca1], 1.525, 111.0, 180.0))
    o1 = add('GLY O', place(pos[n1], pos[ca1], pos[c1], 1.231, 120.5, -40.0))
    n2 = add('SER N', place(pos[n1], pos[ca1], pos[c1], 1.329, 116.5, 140.0))
    ca2 = add('SER CA', place(pos[ca1], pos[c1], pos[n2], 1.458, 121.7, 180.0))
    c2 = add('SER C', place(pos[c1], pos[n2], pos[ca2], 1.525, 111.0, -120.0))
    o2 = add('SER O', place(pos[n2], pos[ca2], pos[c2], 1.231, 120.5, -40.0))
    cb2 = add('SER CB', place(pos[c1], pos[n2], pos[ca2], 1.53, 110.5, 120.0))
    og2 = add('SER OG', place(pos[n2], pos[ca2], pos[cb2], 1.417, 111.0, 60.0))
    n3 = add('PRO N', place(pos[n2], pos[ca2], pos[c2], 1.329, 116.5, 140.0))
    ca3 = add('PRO CA', place(pos[ca2], pos[c2], pos[n3], 1.458, 121.7, 180.0))
    c3 = add('PRO C', place(pos[c2], pos[n3], pos[ca3], 1.525, 111.0, -65.0))
    o3 = add('PRO O', place(pos[n3], pos[ca3], pos[c3], 1.231, 120.5, -40.0))
    cb3 = add('PRO CB', place(pos[c2], pos[n3], pos[ca3], 1.53, 104.0, 170.0))
    cg3 = add('PRO CG', place(pos[n3], pos[ca3], pos[cb3], 1.50, 105.0, 0.0))
    cd3 = add('PRO CD', place(pos[ca3], pos[cb3], pos[cg3], 1.50, 105.0, -25.0))
    bonds = {(n1, ca1), (ca1, c1), (c1, o1), (c1, n2), (n2, ca2), (ca2, c2), (c2, o2), (ca2, cb2), (cb2, og2), (c2, n3), (n3, ca3),
             (ca3, c3), (c3, o3), (ca3, cb3), (cb3, cg3), (cg3, cd3), (n3, cd3)}
    want = {'GLY N': D, 'SER N': D, 'PRO N': 0, 'GLY O': A, 'SER O': A, 'PRO O': A, 'SER OG': D | A, 'GLY CA': 0, 'SER CA': 0, 'PRO CA': 0,
            'PRO CB': H, 'PRO CG': H, 'SER CB': 0, 'PRO CD': 0, 'GLY C': 0, 'SER C': 0, 'PRO C': 0}
    return names, [n.split()[1][0] for n in names], f32(np.array(pos)), bonds, want
