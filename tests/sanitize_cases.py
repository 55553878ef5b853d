"""Ligands for the sanitisation tests (test_sanitize_config.py: restatement, test_sanitize_gpu.py: kernel): named molecules
from ideal coordinates with expectations written by hand, a seeded generator of molecule-like ligands (ring systems joined by
sp3 chains, substituents, rotation, jitter, atom permutation) and the two caps.  Heavy atoms only.  Everything is planar by
construction before the jitter; the chair of cyclohexane is the one exception."""
import numpy as np

from .molecule_cases import ALLOWED, ELEMENTS, Z, one_hot

# monoisotopic masses for ELEMENTS and for hydrogen.  RECALLED, NOT CHECKED: the tests only need the same numbers on both sides.
MASS = [12.0, 14.00307400443, 15.99491461957, 31.9720711744, 30.97376199842, 18.99840316273, 34.968852682, 78.9183376, 126.9044719,
        11.00930536]
MASS_H = 1.00782503223


def polygon(k, side, start_deg=0.0):
    """A regular k-gon of the given side in the xy plane, atoms in ring order."""
    r = side / (2.0 * np.sin(np.pi / k))
    t = np.deg2rad(start_deg) + 2.0 * np.pi * np.arange(k) / k
    return np.stack([r * np.cos(t), r * np.sin(t), np.zeros(k)], axis=1)


def equiangular_hexagon(sides):
    p, d, out = np.zeros(3), 0.0, []
    for s in sides:
        out.append(p.copy())
        p = p + s * np.array([np.cos(d), np.sin(d), 0.0])
        d += np.pi / 3.0
    return np.array(out)


def chair(side=1.53, h=0.25):
    r = np.sqrt(side * side - 4.0 * h * h)
    t = np.pi / 3.0 * np.arange(6)
    return np.stack([r * np.cos(t), r * np.sin(t), h * (-1.0) ** np.arange(6)], axis=1)


def honeycomb(centres, side):
    """The distinct corners of pointy-top hexagons at the lattice places (q, r), sorted by (y, x)."""
    pts = {}
    for q, r in centres:
        c = side * np.array([np.sqrt(3.0) * (q + 0.5 * r), 1.5 * r])
        for k in range(6):
            t = np.deg2rad(30.0 + 60.0 * k)
            v = c + side * np.array([np.cos(t), np.sin(t)])
            pts[(int(round(v[1] / side * 2)), int(round(v[0] / side * 2 / np.sqrt(3.0))))] = v
    keys = sorted(pts)
    return np.array([[pts[k][0], pts[k][1], 0.0] for k in keys])


def outward(pos, ring_nbrs, a):
    """The unit vector from the middle of a's ring neighbours through a."""
    d = pos[a] - np.mean([pos[j] for j in ring_nbrs[a]], axis=0)
    return d / np.linalg.norm(d)


def ring_neighbours(pos, limit=1.6):
    d = np.linalg.norm(pos[:, None] - pos[None], axis=2)
    return [[int(j) for j in np.nonzero((d[a] < limit) & (d[a] > 0.1))[0]] for a in range(len(pos))]


def with_substituents(pos, sym, subs):
    """subs: [(ring atom, [(symbol, length, in-plane angle off the ring atom's outward direction in degrees)])]: the first atom
    of a list hangs on the ring atom, the others on that first atom."""
    pos, sym = [np.asarray(p, dtype=np.float64) for p in pos], list(sym)
    nb = ring_neighbours(np.array(pos))
    for a, chain_ in subs:
        d = outward(np.array(pos), nb, a)
        first = None
        for s, length, ang in chain_:
            t = np.deg2rad(ang)
            rot = np.array([d[0] * np.cos(t) - d[1] * np.sin(t), d[0] * np.sin(t) + d[1] * np.cos(t), 0.0])
            base = pos[a] if first is None else pos[first]
            pos.append(base + length * rot)
            sym.append(s)
            if first is None:
                first = len(pos) - 1
    return np.array(pos), sym


def thiophene():
    """S, C, C, C, C in ring order from real bond lengths: S-C 1.714, C=C 1.370, C-C 1.423, the angle at C3 112.5 degrees."""
    c3, c4 = np.array([0.7115, 0.0, 0.0]), np.array([-0.7115, 0.0, 0.0])
    t = np.deg2rad(67.5)
    c2 = c3 + 1.370 * np.array([np.cos(t), np.sin(t), 0.0])
    c5 = c2 * np.array([-1.0, 1.0, 1.0])
    s = np.array([0.0, c2[1] + np.sqrt(1.714 ** 2 - c2[0] ** 2), 0.0])
    return np.array([s, c2, c3, c4, c5])


def indole(side=1.40):
    """Benzene (atoms 0 .. 5) and a regular pentagon on its bond (0, 1): 6 = N next to atom 1, then 7, 8 back to atom 0."""
    hexa = polygon(6, side, 0.0)
    a, b = hexa[0], hexa[1]
    mid, out = 0.5 * (a + b), 0.5 * (a + b) / np.linalg.norm(0.5 * (a + b))
    apothem, r5 = side / (2.0 * np.tan(np.pi / 5.0)), side / (2.0 * np.sin(np.pi / 5.0))
    c = mid + apothem * out
    t0 = np.arctan2(b[1] - c[1], b[0] - c[0])
    sign = 1.0 if np.cross(b - c, a - c)[2] < 0 else -1.0
    five = [c + r5 * np.array([np.cos(t0 + sign * 2.0 * np.pi * k / 5.0), np.sin(t0 + sign * 2.0 * np.pi * k / 5.0), 0.0]) for k in (1, 2, 3)]
    return np.concatenate([hexa, np.array(five)])


BENZENE_DOUBLES = [(0, 1), (2, 3), (4, 5)]
FIVE_DOUBLES = [(1, 2), (3, 4)]
NAPHTHALENE = honeycomb([(0, 0), (1, 0)], 1.40)
ANTHRACENE = honeycomb([(0, 0), (1, 0), (2, 0)], 1.40)
PHENANTHRENE = honeycomb([(0, 0), (1, 0), (1, 1)], 1.40)
PYRENE = honeycomb([(0, 0), (1, 0), (0, 1), (1, 1)], 1.40)
PHENOL = with_substituents(polygon(6, 1.397), ['C'] * 6, [(0, [('O', 1.36, 0.0)])])
PYRIDONE = with_substituents(polygon(6, 1.38), ['N'] + ['C'] * 5, [(1, [('O', 1.23, 0.0)])])
NITROBENZENE = with_substituents(polygon(6, 1.397), ['C'] * 6, [(0, [('N', 1.47, 0.0), ('O', 1.21, 60.0), ('O', 1.21, -60.0)])])

# (name, symbols, positions, expectations).  Expectation keys: doubles (the sorted local pairs with order_k 2), n_doubles,
# n_arom (aromatic cycles), n_planar, h ({atom: h}), h_all, donors, acceptors (atoms with the flag among N and O ... see the
# test), unsatisfied, valid.
TEXTBOOK = [
    ('benzene 1.397', ['C'] * 6, polygon(6, 1.397), dict(doubles=BENZENE_DOUBLES, n_arom=1, h_all=1, valid=1)),
    ('benzene 1.38', ['C'] * 6, polygon(6, 1.38), dict(doubles=BENZENE_DOUBLES, n_arom=1, h_all=1, valid=1)),
    ('pyridine', ['N'] + ['C'] * 5, polygon(6, 1.37), dict(doubles=BENZENE_DOUBLES, n_arom=1, h={0: 0, 1: 1}, donors=[], acceptors=[0], valid=1)),
    ('pyrrole', ['N'] + ['C'] * 4, polygon(5, 1.38), dict(doubles=FIVE_DOUBLES, n_arom=1, h={0: 1}, donors=[0], acceptors=[], valid=1)),
    ('furan', ['O'] + ['C'] * 4, polygon(5, 1.37), dict(doubles=FIVE_DOUBLES, n_arom=1, h={0: 0}, donors=[], acceptors=[0], valid=1)),
    ('imidazole', ['N', 'C', 'N', 'C', 'C'], polygon(5, 1.36), dict(doubles=[(0, 1), (3, 4)], n_arom=1, h={0: 0, 2: 1}, donors=[2],
                                                                     acceptors=[0], valid=1)),
    ('cyclopentadienyl', ['C'] * 5, polygon(5, 1.40), dict(doubles=[(0, 1), (2, 3)], n_arom=0, unsatisfied=[4], valid=0)),
    ('1,4-cyclohexadiene', ['C'] * 6, equiangular_hexagon([1.50, 1.34, 1.50, 1.50, 1.34, 1.50]),
     dict(doubles=[(1, 2), (4, 5)], n_arom=0, n_planar=1, valid=1)),
    ('cyclohexane', ['C'] * 6, chair(), dict(doubles=[], n_arom=0, n_planar=0, h_all=2, valid=1)),
    ('naphthalene', ['C'] * 10, NAPHTHALENE, dict(n_doubles=5, n_arom=2, fused=True, valid=1)),
    ('anthracene', ['C'] * 14, ANTHRACENE, dict(n_doubles=7, n_arom=3, fused=True, valid=1)),
    ('phenanthrene', ['C'] * 14, PHENANTHRENE, dict(n_doubles=7, n_arom=3, fused=True, valid=1)),
    ('pyrene', ['C'] * 16, PYRENE, dict(n_doubles=8, n_arom=4, fused=True, valid=1)),
    ('indole', ['C'] * 6 + ['N', 'C', 'C'], indole(), dict(n_doubles=4, n_arom=2, h={6: 1}, donors=[6], acceptors=[], valid=1)),
    ('phenol', PHENOL[1], PHENOL[0], dict(doubles=BENZENE_DOUBLES, n_arom=1, h={6: 1, 0: 0}, donors=[6], acceptors=[6], valid=1)),
    # the C=O carbon (atom 1) is not in G; the ring is aromatic by the 0-electron rule: N-H 2, C=O 0, four matched carbons
    ('2-pyridone-like', PYRIDONE[1], PYRIDONE[0], dict(doubles=[(1, 6), (2, 3), (4, 5)], n_arom=1, h={0: 1, 6: 0}, donors=[0],
                                                       acceptors=[6], not_in_g=[1], valid=1)),
    # no formal charges: valence repair leaves the nitro N with three single bonds, so both O read as hydroxyls (the limit)
    ('nitrobenzene', NITROBENZENE[1], NITROBENZENE[0], dict(doubles=BENZENE_DOUBLES, n_arom=1, h={6: 0, 7: 1, 8: 1}, valid=1)),
    # pinned by hand from the rule: S (degree 2) gives 2 electrons, the four carbons match along their path
    ('thiophene', ['S'] + ['C'] * 4, thiophene(), dict(doubles=FIVE_DOUBLES, n_arom=1, h={0: 0, 1: 1, 2: 1, 3: 1, 4: 1}, valid=1)),
]


# ---- (b) the generator --------------------------------------------------------------------------------------------------
def _templates():
    return [
        ('benzene', ['C'] * 6, polygon(6, 1.39)), ('pyridine', ['N'] + ['C'] * 5, polygon(6, 1.37)),
        ('pyrrole', ['N'] + ['C'] * 4, polygon(5, 1.38)), ('furan', ['O'] + ['C'] * 4, polygon(5, 1.37)),
        ('thiophene', ['S'] + ['C'] * 4, thiophene()), ('imidazole', ['N', 'C', 'N', 'C', 'C'], polygon(5, 1.36)),
        ('naphthalene', ['C'] * 10, NAPHTHALENE), ('indole', ['C'] * 6 + ['N', 'C', 'C'], indole()),
    ]


TEMPLATES = _templates()
CYCLOPENTADIENYL = ('cyclopentadienyl', ['C'] * 5, polygon(5, 1.40))
SUBSTITUENTS = [('O', 1.43), ('N', 1.47), ('F', 1.35), ('Cl', 1.77)]


def _rot2(v, deg):
    t = np.deg2rad(deg)
    return np.array([v[0] * np.cos(t) - v[1] * np.sin(t), v[0] * np.sin(t) + v[1] * np.cos(t), v[2]])


def _place(pos, nb, a_in, at, direction):
    """Rotates the planar system about z and moves it so that atom a_in sits at `at` with its outward vector along -direction."""
    d = outward(pos, nb, a_in)
    ang = np.arctan2(-direction[1], -direction[0]) - np.arctan2(d[1], d[0])
    c, s = np.cos(ang), np.sin(ang)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    q = pos @ R.T
    return q + (at - q[a_in])


def generate(seed, sigma=0.01, plant=None):
    """One ligand: (symbols, positions fp32, planted).  `plant`: None, 'cyclopentadienyl' (a ring system that cannot be
    kekulised) or 'sulfone' (a chain S with two S=O and two more bonds: valence 6 over upstream's allowed 4)."""
    rng = np.random.default_rng(seed)
    n_sys = max(int(rng.integers(1, 4)), 2 if plant == 'sulfone' else 1)
    pos, sym = [], []
    at, direction = np.zeros(3), np.array([1.0, 0.0, 0.0])
    prev, prev_is_s = None, False
    for k in range(n_sys):
        name, s_sym, s_pos = TEMPLATES[int(rng.integers(0, len(TEMPLATES)))]
        if plant == 'cyclopentadienyl' and k == 0:
            name, s_sym, s_pos = CYCLOPENTADIENYL
        nb = ring_neighbours(s_pos)
        free = [a for a in range(len(s_sym)) if s_sym[a] == 'C' and len(nb[a]) == 2]
        a_in = free[int(rng.integers(0, len(free)))]
        placed = _place(s_pos, nb, a_in, at if prev is None else at + (1.80 if prev_is_s else 1.51) * direction, direction)
        base = len(pos)
        pos.extend(placed)
        sym.extend(s_sym)
        d_in = outward(placed, nb, a_in)
        rest = [a for a in free if a != a_in]
        a_out = max(rest, key=lambda a: -float(np.dot(outward(placed, nb, a), d_in)) + 1e-9 * a)
        others = [a for a in rest if a != a_out and a_in not in nb[a] and a_out not in nb[a]]
        if others and rng.random() < 0.5:                           # a substituent on the ring
            a = others[int(rng.integers(0, len(others)))]
            s, length = SUBSTITUENTS[int(rng.integers(0, len(SUBSTITUENTS)))]
            pos.append(placed[a] + length * outward(placed, nb, a))
            sym.append(s)
        if k == n_sys - 1:
            break
        # the sp3 chain in the plane: a zigzag off the outward vector of a_out; substituents leave the plane
        d0 = outward(placed, nb, a_out)
        n_chain = int(rng.integers(1, 5))
        p = placed[a_out]
        sulfone_at = int(rng.integers(0, n_chain)) if plant == 'sulfone' and k == 0 else -1
        prev_is_s = False
        for c in range(n_chain):
            step = _rot2(d0, 35.25 if c % 2 == 0 else -35.25)
            is_s = c == sulfone_at
            q = p + (1.80 if is_s or prev_is_s else 1.52) * step
            nxt = _rot2(d0, 35.25 if (c + 1) % 2 == 0 else -35.25)
            pos.append(q)
            sym.append('S' if is_s else 'C')
            b = -step + nxt
            b = b / np.linalg.norm(b)
            up = np.array([0.0, 0.0, 1.0])
            if is_s:
                for sgn in (1.0, -1.0):
                    pos.append(q + 1.44 * (-0.577 * b + sgn * 0.816 * up))
                    sym.append('O')
            else:
                kind = int(rng.integers(0, 5))
                if kind == 4:                                        # C=O: in the plane, opposite the bisector
                    pos.append(q - 1.22 * b)
                    sym.append('O')
                elif kind < 3 and rng.random() < 0.6:
                    s, length = SUBSTITUENTS[kind if kind < 2 else 2 + int(rng.integers(0, 2))]
                    pos.append(q + length * (-0.577 * b + 0.816 * up))
                    sym.append(s)
            p, prev_is_s = q, is_s
        at, direction, prev = p, nxt, base
    pos = np.array(pos)
    A = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    pos = pos @ A.T + rng.standard_normal(3) * 3.0 + rng.standard_normal(pos.shape) * sigma
    perm = rng.permutation(len(sym))
    return [sym[i] for i in perm], pos[perm].astype(np.float32), plant


def generated(n, seed=4242):
    """n ligands: every eighth carries a cyclopentadienyl, every eighth (offset four) a sulfone."""
    return [generate(seed + k, plant='cyclopentadienyl' if k % 8 == 3 else 'sulfone' if k % 8 == 7 else None) for k in range(n)]


# ---- (c) the caps ---------------------------------------------------------------------------------------------------------
def flat_honeycomb(n_hex):
    """n_hex hexagons of a flat 1.54 A honeycomb (an 8 x 8 patch and then one more): all carbon, nothing eligible for G."""
    centres = [(q, r) for r in range(8) for q in range(8)][:min(n_hex, 64)] + [(8, 0)] * (n_hex > 64)
    p = honeycomb(centres, 1.54)
    return ['C'] * len(p), p.astype(np.float32)


def coronene():
    """24 atoms in one component of G."""
    p = honeycomb([(0, 0), (1, 0), (-1, 0), (0, 1), (-1, 1), (0, -1), (1, -1)], 1.40)
    return ['C'] * len(p), p.astype(np.float32)


def cyclopenta_pentacene():
    """25 atoms in one component of G: pentacene and a pentagon on the far bond of its last ring."""
    p = honeycomb([(q, 0) for q in range(5)], 1.40)
    x_max = p[:, 0].max()
    edge = [a for a in range(len(p)) if abs(p[a, 0] - x_max) < 1e-6]
    a, b = p[edge[0]], p[edge[1]]
    apothem, r5 = 1.40 / (2.0 * np.tan(np.pi / 5.0)), 1.40 / (2.0 * np.sin(np.pi / 5.0))
    c = 0.5 * (a + b) + np.array([apothem, 0.0, 0.0])
    t0 = np.arctan2(a[1] - c[1], a[0] - c[0])
    t1 = np.arctan2(b[1] - c[1], b[0] - c[0])
    sign = 1.0 if np.sin(t1 - t0) < 0 else -1.0
    extra = [c + r5 * np.array([np.cos(t0 + sign * 2.0 * np.pi * k / 5.0), np.sin(t0 + sign * 2.0 * np.pi * k / 5.0), 0.0]) for k in (1, 2, 3)]
    p = np.concatenate([p, np.array(extra)])
    return ['C'] * len(p), p.astype(np.float32)
