"""Graphs with coordinates for the pose-RMSD tests (tests/test_pose_rmsd_config.py, tests/test_pose_rmsd_gpu.py): named molecules
whose automorphism groups are known by hand, graphs written by hand, the seeded ligands of tests/sanitize_cases.py, and the poses
that are compared with the reference pose.  A case is a dict: name, sym (element symbols), pos [n,3] float32, bonds [(i, j)]
(local rows), frag [n] (the connected components in order of their first atom), auto (a known automorphism as a list: atom a
goes to auto[a]; None where none is named) and group (the order of the automorphism group of the element-and-connectivity graph
without hydrogens, None where it is not known by hand)."""
import numpy as np

from . import molecule_ref as MR
from . import sanitize_cases as C
from . import smiles_cases as SC
from .molecule_cases import ALLOWED, ELEMENTS, ETHANOL, TET, TWO_ETHANOLS_CL, Z

ELEMENTS_ALL = ELEMENTS + ['H', 'Si']
Z_ALL = Z + [1, 14]
ALLOWED_ALL = ALLOWED + [1, 4]


def components(n, bonds):
    comp = list(range(n))
    for _ in range(n):
        for i, j in bonds:
            comp[i] = comp[j] = min(comp[i], comp[j])
    names = {c: k for k, c in enumerate(sorted(set(comp)))}
    return [names[c] for c in comp]


def case(name, sym, pos, bonds=None, auto=None, group=None):
    """bonds None: those the perception rule of include/kpd.h finds in the coordinates (tests/molecule_ref.py)."""
    pos = np.asarray(pos, dtype=np.float32)
    if bonds is None:
        feat = np.zeros((len(sym), len(ELEMENTS_ALL)), dtype=np.float32)
        feat[np.arange(len(sym)), [ELEMENTS_ALL.index(s) for s in sym]] = 1.0
        bonds = [tuple(map(int, ij)) for ij in MR.perceive(pos, feat, Z_ALL, ALLOWED_ALL)['bonds']]
    bonds = [tuple(b) for b in bonds]
    return dict(name=name, sym=list(sym), pos=pos, bonds=bonds, frag=components(len(sym), bonds), auto=auto, group=group)


def tripod(axis, length, twist_deg=0.0):
    """Three vectors of the given length at the tetrahedral angle to -axis and 120 degrees from each other."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    e1 = np.cross(a, [0.0, 0.0, 1.0] if abs(a[2]) < 0.9 else [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(a, e1)
    out = []
    for k in range(3):
        t = np.deg2rad(twist_deg + 120.0 * k)
        out.append(length * (a / 3.0 + np.sqrt(8.0) / 3.0 * (np.cos(t) * e1 + np.sin(t) * e2)))
    return np.array(out)


def _ring6():
    return C.polygon(6, 1.397)


def _toluene():
    pos, sym = C.with_substituents(_ring6(), ['C'] * 6, [(0, [('C', 1.51, 0.0)])])
    return case('toluene', sym, pos, auto=[0, 5, 4, 3, 2, 1, 6], group=2)


def _xylene(name, second, auto, group):
    pos, sym = C.with_substituents(_ring6(), ['C'] * 6, [(0, [('C', 1.51, 0.0)]), (second, [('C', 1.51, 0.0)])])
    return case(name, sym, pos, auto=auto, group=group)


def _biphenyl():
    p = _ring6()
    d = p[0] / np.linalg.norm(p[0])
    return case('biphenyl', ['C'] * 12, np.concatenate([p, -p + (2.0 * p[0] + 1.48 * d)]),
                auto=[6, 7, 8, 9, 10, 11, 0, 1, 2, 3, 4, 5], group=8)


def _naphthalene():
    c = case('naphthalene', ['C'] * 10, C.NAPHTHALENE, group=4)
    p = c['pos'].astype(np.float64)
    mirrored = p * np.array([-1.0, 1.0, 1.0]) + np.array([p[:, 0].max() + p[:, 0].min(), 0.0, 0.0])      # the mirror across the long axis' normal
    c['auto'] = [int(np.argmin(np.linalg.norm(p - m, axis=1))) for m in mirrored]
    return c


def _cf3():
    pos = np.concatenate([[[0.0, 0.0, 0.0], [-1.52, 0.0, 0.0]], tripod([1.0, 0.0, 0.0], 1.35)])
    return case('CF3', ['C', 'C', 'F', 'F', 'F'], pos, bonds=[(0, 1), (0, 2), (0, 3), (0, 4)], auto=[0, 1, 3, 4, 2], group=6)


def _tert_butyl():
    """(CH3)3C-C-O: the three methyls permute."""
    pos = np.concatenate([[[0.0, 0.0, 0.0], [-1.54, 0.0, 0.0], [-2.05, 1.34, 0.0]], tripod([1.0, 0.0, 0.0], 1.53)])
    return case('tert-butyl', ['C', 'C', 'O', 'C', 'C', 'C'], pos, bonds=[(0, 1), (1, 2), (0, 3), (0, 4), (0, 5)], auto=[0, 1, 2, 4, 5, 3],
                group=6)


def _carboxylate():
    t = np.deg2rad(120.0)
    pos = [[-1.52, 0.0, 0.0], [0.0, 0.0, 0.0], [-1.26 * np.cos(t), 1.26 * np.sin(t), 0.0], [-1.26 * np.cos(t), -1.26 * np.sin(t), 0.0]]
    return case('carboxylate-like', ['C', 'C', 'O', 'O'], pos, bonds=[(0, 1), (1, 2), (1, 3)], auto=[0, 1, 3, 2], group=2)


def _neopentane_cf3():
    """C(CF3)4 as a graph by hand: 4! x 3!^4 = 31 104 automorphisms."""
    pos, sym, bonds = [np.zeros(3)], ['C'], []
    for k in range(4):
        c = 1.54 * TET[k]
        pos.append(c)
        sym.append('C')
        bonds.append((0, 1 + k))
    for k in range(4):
        for f in tripod(TET[k], 1.35, twist_deg=60.0):
            bonds.append((1 + k, len(pos)))
            pos.append(1.54 * TET[k] + f)
            sym.append('F')
    auto = [0, 2, 3, 4, 1] + [5 + 3 * ((k + 1) % 4) + (q + 1) % 3 for k in range(4) for q in range(3)]
    return case('C(CF3)4', sym, np.array(pos), bonds=bonds, auto=auto, group=31104)


def _methane_h():
    pos = np.concatenate([np.zeros((1, 3)), 1.09 * TET])
    return case('methane with hydrogens', ['C', 'H', 'H', 'H', 'H'], pos, bonds=[(0, k) for k in range(1, 5)], auto=[0, 2, 3, 4, 1], group=1)


def _ethane_h():
    pos = np.concatenate([[[0.0, 0.0, 0.0], [1.53, 0.0, 0.0]], tripod([-1.0, 0.0, 0.0], 1.09), np.array([1.53, 0.0, 0.0]) + tripod([1.0, 0.0, 0.0], 1.09, 60.0)])
    return case('ethane with hydrogens', ['C', 'C'] + ['H'] * 6, pos, bonds=[(0, 1), (0, 2), (0, 3), (0, 4), (1, 5), (1, 6), (1, 7)],
                auto=[1, 0, 5, 6, 7, 2, 3, 4], group=2)


def _chorded_ring():
    Zs, _, _, sym, bonds, _ = SC.chorded_ring(256, 2, 3)
    pos = np.random.default_rng(256).standard_normal((256, 3)) * 6.0
    return case('chorded ring of 256', sym, pos, bonds=bonds)


def named():
    sym7, pos7, bonds7 = TWO_ETHANOLS_CL
    return [
        case('one atom', ['C'], [[0.3, -0.2, 0.1]], bonds=[], auto=[0], group=1),
        case('two carbons', ['C', 'C'], [[0.0, 0.0, 0.0], [1.52, 0.0, 0.0]], bonds=[(0, 1)], auto=[1, 0], group=2),
        case('ethanol', ['C', 'C', 'O'], ETHANOL, bonds=[(0, 1), (1, 2)], auto=[0, 1, 2], group=1),
        case('benzene', ['C'] * 6, _ring6(), auto=[1, 2, 3, 4, 5, 0], group=12),
        _toluene(),
        _xylene('p-xylene', 3, [3, 4, 5, 0, 1, 2, 7, 6], 4),
        _biphenyl(),
        _naphthalene(),
        _carboxylate(),
        _cf3(),
        _tert_butyl(),
        _neopentane_cf3(),
        case('cyclohexane chair', ['C'] * 6, C.chair(), auto=[2, 3, 4, 5, 0, 1], group=12),
        case('two ethanols and a chloride', sym7, pos7, bonds=list(bonds7), auto=[3, 4, 5, 0, 1, 2, 6], group=2),
        _methane_h(),
        _ethane_h(),
    ]


def o_xylene():
    """Its one symmetry is the mirror through the middle of the bond 0-1, which swaps the two Kekule patterns of the ring."""
    return _xylene('o-xylene', 1, [1, 0, 5, 4, 3, 2, 7, 6], 2)


def big():
    return [_chorded_ring()]


def generated(count=48):
    return [case(f'generated {k}', sym, pos) for k, (sym, pos, _) in enumerate(C.generated(count))]


def all_cases():
    return named() + big() + generated()


def permuted_rows(pos, auto):
    """The pose in which atom auto[a] sits where atom a sat: row auto[a] of the result is row a of pos."""
    out = np.empty_like(pos)
    for a, v in enumerate(auto):
        out[v] = pos[a]
    return out


def poses(c, K, seed=0):
    """[K,n,3] float32 for one case: pose 0 the reference's rows permuted by the named automorphism (or by a seeded shuffle where
    none is named), pose 1 a seeded shuffle of the rows (no automorphism unless by chance), pose 2 a seeded Gaussian displacement
    of 0.3 A, and from there on in turn: the automorphism pose displaced by 0.05 A, displacements of 0.1 A and of 0.5 A."""
    rng = np.random.default_rng(1000 + seed + 7 * len(c['sym']))
    ref, n = c['pos'], len(c['sym'])
    auto = c['auto'] if c['auto'] is not None else [int(v) for v in rng.permutation(n)]
    out = []
    for k in range(K):
        if k == 0:
            p = permuted_rows(ref, auto)
        elif k == 1:
            p = permuted_rows(ref, [int(v) for v in rng.permutation(n)])
        elif k == 2:
            p = ref + rng.standard_normal((n, 3)) * 0.3
        elif k % 3 == 0:
            p = permuted_rows(ref, auto) + rng.standard_normal((n, 3)) * 0.05
        else:
            p = ref + rng.standard_normal((n, 3)) * (0.1 if k % 3 == 1 else 0.5)
        out.append(np.asarray(p, dtype=np.float32))
    return np.stack(out) if K else np.zeros((0, n, 3), dtype=np.float32)


def renumbered(c, rng):
    """The same case with its atoms renumbered by a seeded permutation p (atom a becomes p[a]); returns (case, p)."""
    n = len(c['sym'])
    p = [int(v) for v in rng.permutation(n)]
    sym, pos = [None] * n, np.empty_like(c['pos'])
    for a in range(n):
        sym[p[a]] = c['sym'][a]
        pos[p[a]] = c['pos'][a]
    bonds = [(p[i], p[j]) for i, j in c['bonds']]
    return dict(name=c['name'] + ' renumbered', sym=sym, pos=pos, bonds=bonds, frag=components(n, bonds), auto=None, group=c['group']), p
