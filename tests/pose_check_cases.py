"""Cases for the plausibility checks (kpd_pose_check): molecules written by hand as kpd_mol_perceive and kpd_mol_sanitize would have
left them (the graph from the ideal pose), the distorted poses that must each set exactly the named bits, the lattice cases, and
the helpers that pack cases into the arrays of the C ABI.  Hydrogens, where a case needs them for its geometry, are atoms of the
graph with the class 'H'."""
import numpy as np

from .molecule_cases import ELEMENTS, Z
from .vina_cases import place
from . import pose_check_ref as R

ELEMENTS_H, Z_H = ELEMENTS + ['H'], Z + [1]
# van der Waals radii after Bondi 1964 as the test's own table; 'H' is 0 unless a case asks for hydrogens
VDW = {'C': 1.7, 'N': 1.55, 'O': 1.52, 'S': 1.8, 'P': 1.8, 'F': 1.47, 'Cl': 1.75, 'Br': 1.85, 'I': 1.98, 'B': 1.92, 'H': 1.2}


def lig_radius(with_h=False, **override):
    t = dict(VDW, **override)
    return np.array([t[e] if e != 'H' or with_h or 'H' in override else 0.0 for e in ELEMENTS_H], dtype=np.float32)


def components(n, bonds):
    lab = list(range(n))
    for _ in range(n):
        for i, j in bonds:
            lab[i] = lab[j] = min(lab[i], lab[j])
    order = sorted(set(lab))
    return [order.index(v) for v in lab]


def mol(name, sym, pos, bonds, h=None, aromatic=(), expect=0):
    """bonds: (i, j, order_k[, 'a' aromatic ring bond | 'r' ring bond]); aromatic: the aromatic atoms; h: hydrogen counts."""
    n = len(sym)
    rows = sorted((min(b[0], b[1]), max(b[0], b[1]), b[2], b[3] if len(b) > 3 else '') for b in bonds)
    flags = [{'a': 7, 'r': 1, '': 0}[r[3]] for r in rows]
    return dict(name=name, sym=list(sym), pos=np.asarray(pos, dtype=np.float32), bonds=[(r[0], r[1]) for r in rows], order=[r[2] for r in rows],
                bond_flags=flags, h=list(h) if h is not None else [0] * n, atom_flags=[3 if a in aromatic else 0 for a in range(n)],
                frag=components(n, [(r[0], r[1]) for r in rows]), expect=expect, pocket=None, radius={}, pose=None)


def posed(c, name, pose, expect, pocket=None, radius=None):
    """The graph of c with another pose (and pocket): what a relaxed or docked pose of it looks like to the call."""
    return dict(c, name=name, pose=np.asarray(pose, dtype=np.float32), expect=expect, pocket=pocket if pocket is not None else c['pocket'],
                radius=radius if radius is not None else c['radius'])


def polygon(k, side):
    r = side / (2.0 * np.sin(np.pi / k))
    t = 2.0 * np.pi * np.arange(k) / k
    return np.stack([r * np.cos(t), r * np.sin(t), np.zeros(k)], axis=1)


SHIFT = np.array([3.3, -2.2, 1.1])      # off the lattice and off the axes


def benzene():
    ring = [(k, (k + 1) % 6, 2 if k % 2 == 0 else 1, 'a') for k in range(6)]
    return mol('benzene', ['C'] * 6, polygon(6, 1.39) + SHIFT, ring, h=[1] * 6, aromatic=range(6))


def ethene():
    cc, ch = 1.34, 1.08
    s, c = ch * np.sin(np.deg2rad(60.0)), ch * np.cos(np.deg2rad(60.0))
    pos = np.array([[0, 0, 0], [cc, 0, 0], [-c, s, 0], [-c, -s, 0], [cc + c, s, 0], [cc + c, -s, 0]]) + SHIFT
    return mol('ethene', ['C', 'C', 'H', 'H', 'H', 'H'], pos, [(0, 1, 2), (0, 2, 1), (0, 3, 1), (1, 4, 1), (1, 5, 1)])


def alkane(n, dihedrals=None, length=1.53, angle=112.0):
    p = [np.zeros(3), np.array([length, 0.0, 0.0])]
    t = np.deg2rad(angle)
    if n > 2:
        p.append(p[1] + length * np.array([-np.cos(t), np.sin(t), 0.0]))
    for k in range(n - 3):
        p.append(place(p[-3], p[-2], p[-1], length, angle, 180.0 if dihedrals is None else dihedrals[k]))
    return np.array(p[:n]) + SHIFT


def propane():
    return mol('propane', ['C'] * 3, alkane(3), [(0, 1, 1), (1, 2, 1)], h=[3, 2, 3])


def hexane():
    return mol('hexane', ['C'] * 6, alkane(6), [(k, k + 1, 1) for k in range(5)], h=[3, 2, 2, 2, 2, 3])


def acetamide_pos(cn_deg=120.0, lift=0.0):
    """C0 (methyl), C1, O2, N3 in the plane z = 0; the angle C0-C1-N3 is cn_deg (N turned in the plane, away from O), C1 lifted."""
    d = lambda deg, L: L * np.array([np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg)), 0.0])
    return np.array([d(180.0, 1.51), [0.0, 0.0, lift], d(60.0, 1.23), d(180.0 + cn_deg, 1.34)]) + SHIFT


def acetamide():
    return mol('acetamide', ['C', 'C', 'O', 'N'], acetamide_pos(), [(0, 1, 1), (1, 2, 2), (1, 3, 1)], h=[3, 0, 0, 2])


def ideal():
    return [benzene(), ethene(), propane(), acetamide(), hexane()]


def slab(z_top, half=6.0, step=1.5, layers=3):
    g = np.arange(-half, half + 1e-9, step)
    return np.array([[x, y, z_top - k * step] for k in range(layers) for x in g for y in g]) + np.array([SHIFT[0], SHIFT[1], 0.0])


def carbon_pocket(x):
    x = np.asarray(x, dtype=np.float32).reshape(-1, 3)
    return dict(x=x, radius=np.full(len(x), VDW['C'], dtype=np.float32))


def distorted():
    """Every distortion with the fail bits it must set, and no other."""
    out = []
    b = benzene()
    p = b['pos'].copy()
    p[0, 2] += 0.6
    out.append(posed(b, 'benzene, one atom lifted 0.6 A', p, R.F_RING))
    a = acetamide()
    out.append(posed(a, 'acetamide, carbonyl carbon lifted 0.4 A', acetamide_pos(lift=0.4), R.F_CENTRE))
    out.append(posed(a, 'acetamide, C-C-N squeezed to 75 degrees', acetamide_pos(cn_deg=75.0), R.F_ANGLE))
    e = ethene()
    p = e['pos'].astype(np.float64) - SHIFT
    t = np.deg2rad(45.0)
    for k in (4, 5):                                    # the far CH2 turned about the C=C axis (x)
        y, z = p[k, 1], p[k, 2]
        p[k, 1], p[k, 2] = y * np.cos(t) - z * np.sin(t), y * np.sin(t) + z * np.cos(t)
    out.append(posed(e, 'ethene twisted 45 degrees', p + SHIFT, R.F_TWIST))
    pr = propane()
    p = pr['pos'].astype(np.float64)
    p[0] = p[1] + 1.3 * (p[0] - p[1])
    out.append(posed(pr, 'propane, a bond stretched x 1.3', p, R.F_BOND))
    h = hexane()
    out.append(posed(h, 'hexane folded, 1-6 contact at 2.0 A', alkane(6, (-60.0, -5.0, 70.0)), R.F_CLASH))
    p = h['pos'].astype(np.float64)
    away = (p[0] - p[1]) / np.linalg.norm(p[0] - p[1])
    out.append(posed(h, 'hexane, 2.0 A from a pocket carbon', h['pos'], R.F_POCKET, pocket=carbon_pocket(p[0] + 2.0 * away)))
    # benzene lying flat with its centre half a radius above the top layer of a slab: clash and overlap come together
    out.append(posed(b, 'benzene half-way into a slab', b['pos'], R.F_POCKET | R.F_OVERLAP, pocket=carbon_pocket(slab(SHIFT[2] - 0.85))))
    return out


def lattice_cases():
    """(case, what it is about).  All have a pocket, since no point is counted without one."""
    far = carbon_pocket([[40.0, 40.0, 40.0]])
    one = mol('one carbon on a lattice point, R = 1.5', ['C'], [[1.0, -0.5, 2.0]], [], h=[4])
    one = posed(one, one['name'], one['pos'], 0, pocket=far, radius=dict(C=1.5))
    b = benzene()
    origin = posed(b, 'benzene straddling the origin', b['pos'] - SHIFT + np.array([0.1, -0.2, 0.05]), 0, pocket=far)
    inside = posed(b, 'benzene straddling the origin, a pocket atom inside it', origin['pose'], R.F_POCKET | R.F_OVERLAP,
                   pocket=carbon_pocket([[0.3, 0.1, -0.4], [-1.2, 0.9, 0.3]]))
    return [one, origin, inside]


def all_cases():
    return ideal() + distorted() + lattice_cases()


# ---- packing -----------------------------------------------------------------------------------------------------------------------------
def arrays(cases, K=1, cap_bonds=None, elements=ELEMENTS_H):
    """Cases -> (ptr, mol, san, pos [K,N,3], pocket) in the layout of the C ABI; every case with a pocket gets a pocket of its own.
    Pose k of a case is its pose moved by k * (0.37, -0.21, 0.13) while the pocket stays: the poses differ in checks 5 and 6."""
    ptr, elem, frag, bonds, order, flags, bond_ptr, h, af, rows = [0], [], [], [], [], [], [0], [], [], []
    px, pr, pptr, pof = [], [], [0], []
    for c in cases:
        a0 = ptr[-1]
        elem += [elements.index(s) for s in c['sym']]
        frag += list(c['frag'])
        bonds += [(a0 + i, a0 + j) for i, j in c['bonds']]
        order += list(c['order'])
        flags += list(c['bond_flags'])
        h += list(c['h'])
        af += list(c['atom_flags'])
        ptr.append(a0 + len(c['sym']))
        bond_ptr.append(len(bonds))
        rows.append(c['pose'] if c.get('pose') is not None else c['pos'])
        if c.get('pocket') is not None:
            pof.append(len(pptr) - 1)
            px.append(c['pocket']['x'])
            pr.append(c['pocket']['radius'])
            pptr.append(pptr[-1] + len(c['pocket']['x']))
        else:
            pof.append(-1)
    cap = len(bonds) if cap_bonds is None else cap_bonds
    pad = cap - len(bonds)
    i64 = lambda x: np.asarray(x, dtype=np.int64)
    mol_ = dict(elem=i64(elem), frag=i64(frag), bonds=i64(bonds + [(0, 0)] * pad).reshape(-1, 2), bond_ptr=i64(bond_ptr),
                status=np.zeros(len(cases), dtype=np.int64))
    san = dict(order_k=i64(order + [0] * pad), bond_flags=i64(flags + [0] * pad), atom_h=i64(h), atom_flags=i64(af),
               status=np.zeros(len(cases), dtype=np.int64))
    base = np.concatenate(rows).astype(np.float32) if rows else np.zeros((0, 3), dtype=np.float32)
    pos = np.stack([(base.astype(np.float64) + k * np.array([0.37, -0.21, 0.13])).astype(np.float32) for k in range(K)])
    pocket = dict(x=np.concatenate(px).astype(np.float32) if px else np.zeros((0, 3), dtype=np.float32),
                  radius=np.concatenate(pr).astype(np.float32) if pr else np.zeros(0, dtype=np.float32), ptr=i64(pptr), of=i64(pof))
    return i64(ptr), mol_, san, pos, pocket


def run_case(c, margins=None, lattice=R.lattice_counts, with_h=False, params=None):
    """The restatement on one case alone; returns its dict of [1,1,..] arrays."""
    ptr, mol_, san, pos, pocket = arrays([c])
    return R.pose_check_batch(ptr, mol_, san, Z_H, pos, lig_radius(with_h, **c['radius']), pocket, params=params, margins=margins, lattice=lattice)


def chain_case(n, seed=0, name=None):
    """A carbon zigzag of n atoms with a seeded jitter and a hetero atom here and there: the shapes of the GPU tests."""
    rng = np.random.default_rng(100 + n + seed)
    pos = alkane(max(n, 2))[:n] + rng.standard_normal((n, 3)) * 0.05
    sym = [('C', 'C', 'C', 'N', 'O')[int(rng.integers(5))] if 0 < k < n - 1 else 'C' for k in range(n)]
    return mol(name or f'chain {n}', sym, pos, [(k, k + 1, 1) for k in range(n - 1)], h=[1] * n)
