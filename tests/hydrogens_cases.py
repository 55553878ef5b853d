"""Ligands for the hydrogen placement tests (test_hydrogens_config.py: restatement, test_hydrogens_gpu.py: kernel): 22 small
molecules of 1 to 5 heavy atoms from ideal coordinates (tetrahedral centres at acos(-1/3), planar ones at 120 degrees, linear
ones on a line) with the hydrogen counts and centre classes written by hand, a flat three-neighbour carbon, the all-carbon
chains around the 256-atom cap, and the chain of reference calls (perceive, sanitise, add hydrogens) the tests share.
Heavy atoms only; every molecule is turned by one fixed rotation so that no bond lies along an axis."""
import numpy as np

from . import hydrogens_ref as HR
from . import molecule_ref as R
from . import sanitize_cases as SC
from . import sanitize_ref as SR
from .molecule_cases import ALLOWED, ELEMENTS, TET, Z

ELEMENTS_H, Z_H, ALLOWED_H, MASS_H_TABLE = ELEMENTS + ['H'], Z + [1], ALLOWED + [1], SC.MASS + [SC.MASS_H]
H_CLASS = len(ELEMENTS)
TET_ANGLE = float(np.degrees(np.arccos(-1.0 / 3.0)))
LIN, PLA, TETC = HR.LINEAR, HR.PLANAR, HR.TET
ROT = np.linalg.qr(np.random.default_rng(11).standard_normal((3, 3)))[0]


def one_hot_h(symbols):
    f = np.zeros((len(symbols), len(ELEMENTS_H)), dtype=np.float32)
    f[np.arange(len(symbols)), [ELEMENTS_H.index(s) for s in symbols]] = 1.0
    return f


def zigzag(lengths):
    """A planar all-anti chain: len(lengths) + 1 atoms, every angle tetrahedral."""
    s, c = np.sqrt(2.0 / 3.0), np.sqrt(1.0 / 3.0)
    pts = [np.zeros(3)]
    for k, d in enumerate(lengths):
        pts.append(pts[-1] + d * np.array([s, c if k % 2 == 0 else -c, 0.0]))
    return np.array(pts)


def star(lengths, dirs):
    """A centre at the origin (atom 0) and one atom along every direction."""
    return np.concatenate([np.zeros((1, 3)), np.array([d * np.asarray(u, dtype=np.float64) for d, u in zip(lengths, dirs)])])


def trigonal(l0, l1, l2):
    """Atom 1 at the origin with atoms 0, 2, 3 around it at 120 degrees in a plane."""
    u = lambda deg: np.array([np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg)), 0.0])
    return np.array([l0 * u(0.0), np.zeros(3), l1 * u(120.0), l2 * u(240.0)])


LINE = np.array([1.0, 0.0, 0.0])
# (name, symbols, positions, hydrogens, {atom: class} of the atoms that get hydrogens)
_SMALL = [
    ('methane', ['C'], np.zeros((1, 3)), 4, {0: TETC}),
    ('ammonia', ['N'], np.zeros((1, 3)), 3, {0: TETC}),
    ('water', ['O'], np.zeros((1, 3)), 2, {0: TETC}),
    ('hydrogen fluoride', ['F'], np.zeros((1, 3)), 1, {0: TETC}),
    ('hydrogen sulfide', ['S'], np.zeros((1, 3)), 2, {0: TETC}),
    ('ethane', ['C', 'C'], zigzag([1.53]), 6, {0: TETC, 1: TETC}),
    ('ethene', ['C', 'C'], zigzag([1.33]), 4, {0: PLA, 1: PLA}),
    ('ethyne', ['C', 'C'], zigzag([1.20]), 2, {0: LIN, 1: LIN}),
    ('methanol', ['C', 'O'], zigzag([1.43]), 4, {0: TETC, 1: TETC}),
    ('methylamine', ['C', 'N'], zigzag([1.47]), 5, {0: TETC, 1: TETC}),
    ('formaldehyde', ['C', 'O'], zigzag([1.21]), 2, {0: PLA}),
    ('hydrogen cyanide', ['C', 'N'], zigzag([1.16]), 1, {0: LIN}),
    # the reference atom of the methyl group (N) is on the line C-C: perp() gives the azimuth
    ('acetonitrile', ['C', 'C', 'N'], np.array([-1.46 * LINE, 0.0 * LINE, 1.16 * LINE]), 3, {0: TETC}),
    ('propane', ['C'] * 3, zigzag([1.53] * 2), 8, {0: TETC, 1: TETC, 2: TETC}),
    ('butane', ['C'] * 4, zigzag([1.53] * 3), 10, {a: TETC for a in range(4)}),
    ('dimethyl ether', ['C', 'O', 'C'], zigzag([1.42] * 2), 6, {0: TETC, 2: TETC}),
    ('isobutane', ['C'] * 4, star([1.53] * 3, TET[:3]), 10, {a: TETC for a in range(4)}),
    ('neopentane', ['C'] * 5, star([1.53] * 4, TET), 12, {a: TETC for a in range(1, 5)}),
    ('acetamide', ['C', 'C', 'O', 'N'], trigonal(1.51, 1.23, 1.35), 5, {0: TETC, 3: PLA}),
    ('acetic acid', ['C', 'C', 'O', 'O'], trigonal(1.50, 1.21, 1.36), 4, {0: TETC, 3: TETC}),
    ('propene', ['C'] * 3, trigonal(1.33, 1.50, 9.0)[:3], 6, {0: PLA, 1: PLA, 2: TETC}),
    ('ethanol', ['C', 'C', 'O'], zigzag([1.52, 1.43]), 6, {0: TETC, 1: TETC, 2: TETC}),
]
SMALL = [(name, sym, (np.asarray(p) @ ROT.T + np.array([0.7, -1.1, 0.4])).astype(np.float32), h, cls) for name, sym, p, h, cls in _SMALL]
IDEAL = {TETC: TET_ANGLE, PLA: 120.0, LIN: 180.0}

# a carbon with three single-bonded neighbours in one plane: the sum of the unit vectors vanishes, the normal does not
FLAT = (['C', 'C', 'C', 'O'], (trigonal(1.53, 1.53, 1.43)[[1, 0, 2, 3]] @ ROT.T).astype(np.float32))


def carbon_chain(n):
    return ['C'] * n, (zigzag([1.53] * (n - 1)) @ ROT.T).astype(np.float32)


def concat(ligs):
    pos = [np.asarray(p, dtype=np.float32).reshape(-1, 3) for _, p in ligs]
    sizes = [len(p) for p in pos]
    feat = [SC.one_hot(sym) for sym, _ in ligs if len(sym)]
    return (np.concatenate(pos), np.concatenate(feat) if feat else np.zeros((0, len(ELEMENTS)), dtype=np.float32),
            np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))


def mol_of(perceived):
    return {k: perceived[k] for k in ('elem', 'frag', 'bonds', 'order', 'bond_ptr', 'status')}


def reference(ligs, largest=False):
    """Perceive, sanitise and hydrogenate [(symbols, positions)] by the restatements.  Returns pos, ptr, mol, san, hyd."""
    pos, feat, ptr = concat(ligs)
    mol = mol_of(R.perceive_batch(pos, feat, ptr, Z, ALLOWED))
    san = SR.sanitize_batch(pos, ptr, mol, Z, ALLOWED, SC.MASS, SC.MASS_H, largest)
    hyd = HR.add_hs_batch(pos, ptr, mol, san, Z_H, ALLOWED_H, H_CLASS, largest)
    return pos, ptr, mol, san, hyd


def ligand(hyd, b):
    """Ligand b of a hydrogenated batch: positions, classes, local bonds, orders, parents (local), source."""
    o0, o1, q0, q1 = (int(hyd[k][b + d]) for k in ('out_ptr', 'out_bond_ptr') for d in (0, 1))
    return dict(pos=hyd['pos'][o0:o1], elem=hyd['elem'][o0:o1], bonds=hyd['bonds'][q0:q1] - o0, order=hyd['order'][q0:q1],
                parent=hyd['parent'][o0:o1] - o0, source=hyd['source'][o0:o1], frag=hyd['frag'][o0:o1], valence=hyd['valence'][o0:o1])


def reperceive(lig):
    """molecule_ref.perceive on the hydrogenated coordinates with the hydrogen class added."""
    return R.perceive(lig['pos'], one_hot_h([ELEMENTS_H[e] for e in lig['elem']]), Z_H, ALLOWED_H)


def resanitize(lig, largest=False):
    return SR.sanitize(lig['pos'], lig['elem'], lig['frag'], lig['bonds'], lig['order'], Z_H, ALLOWED_H, MASS_H_TABLE, SC.MASS_H, largest)
