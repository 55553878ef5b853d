"""Inputs shared by test_relax_config.py (restatement) and test_relax_gpu.py (kernel): seeded molecule-like ligands, pockets,
hand-made geometries with known minima, and the seeds of the trajectory test.  Nothing here depends on an implementation."""
import numpy as np

from .molecule_cases import ELEMENTS, Z, chain, f32

# {x, D} per element of ELEMENTS for the tests: any positive numbers would do, nothing relies on their being UFF's
VDW = {'C': (3.851, 0.105), 'N': (3.660, 0.069), 'O': (3.500, 0.060), 'S': (4.035, 0.274), 'P': (4.147, 0.305), 'F': (3.364, 0.050),
       'Cl': (3.947, 0.227), 'Br': (4.189, 0.251), 'I': (4.500, 0.339), 'B': (4.083, 0.180)}
LIG_VDW = np.array([VDW[e] for e in ELEMENTS], dtype=np.float32)          # [F,2], the kernel's lig_vdw
POCKET_POOL = ('C', 'C', 'C', 'N', 'O', 'S')

# seeds of the trajectory test: test_relax_config.py checks on the CPU that every decision margin of their first five iterations
# is >= 1e-9 (a seed that fails is replaced there, never on the GPU)
TRAJ_SEEDS = (11, 14, 17, 20)


def unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def grow(rng, n, pool=('C', 'C', 'C', 'C', 'N', 'O', 'S', 'F', 'Cl'), noise=0.06):
    """A molecule-like tree of n heavy atoms: every new atom sits 1.45 A (+- noise) from a random earlier atom with fewer than three
    neighbours, at least 2.0 A from every other atom.  Returns (symbols, pos float32)."""
    pos, deg, sym = [np.zeros(3)], [0], ['C']
    tries = 0
    while len(pos) < n:
        tries += 1
        assert tries < 20000, 'grow: no room'
        parent = int(rng.integers(len(pos)))
        if deg[parent] >= 3 or sym[parent] in ('F', 'Cl'):
            continue
        new = pos[parent] + unit(rng) * (1.45 + noise * rng.standard_normal())
        d = np.linalg.norm(np.array(pos) - new, axis=1)
        d[parent] = 9.0
        if d.min() < 2.0:
            continue
        pos.append(new)
        deg.append(1)
        deg[parent] += 1
        sym.append(pool[int(rng.integers(len(pool)))])
        if not any(d < 3 and e not in ('F', 'Cl') for d, e in zip(deg, sym)):
            sym[-1] = 'C'                                # keep a site to grow from
    return sym, f32(np.array(pos))


def make_pocket(rng, m, lig_pos, reach=7.0, keep_out=1.2):
    """m pocket atoms scattered around the ligand: uniform in its bounding box grown by `reach`, none closer than keep_out to a
    ligand atom (close enough for the soft core to matter).  Returns (symbols, pos float32)."""
    lig = np.asarray(lig_pos, dtype=np.float64).reshape(-1, 3)
    lo, hi = lig.min(axis=0) - reach, lig.max(axis=0) + reach
    out = []
    while len(out) < m:
        q = lo + (hi - lo) * rng.random(3)
        if np.linalg.norm(lig - q, axis=1).min() >= keep_out:
            out.append(q)
    sym = [POCKET_POOL[int(rng.integers(len(POCKET_POOL)))] for _ in range(m)]
    return sym, f32(np.array(out).reshape(-1, 3))


def vdw_rows(symbols):
    return np.array([VDW[s] for s in symbols], dtype=np.float32).reshape(-1, 2)


def traj_case(seed):
    """(symbols, pos, pocket symbols, pocket pos) of one trajectory seed: 9 .. 16 atoms in a pocket of 40, somewhere in a
    receptor's frame (tens of Angstrom from the origin, where an fp32 coordinate has an ulp of 2e-6 A)."""
    rng = np.random.default_rng(seed)
    sym, pos = grow(rng, int(rng.integers(9, 17)))
    psym, ppos = make_pocket(rng, 40, pos, keep_out=2.2)
    shift = np.array([20.0, -17.0, 31.0])
    return sym, f32(pos + shift), psym, f32(ppos + shift)


def ring6(rng, side=1.40, noise=0.02):
    """A planar six-ring of carbons, `side` A bonds, with in-plane noise: bonds stay inside (1.38, 1.46), angles near 120."""
    t = np.deg2rad(60.0 * np.arange(6))
    p = np.stack([side * np.cos(t), side * np.sin(t), np.zeros(6)], axis=1)           # circumradius = side
    p[:, :2] += noise * (rng.random((6, 2)) - 0.5)
    return ['C'] * 6, f32(p)


# (name, symbols, pos, expected bond lengths {(i, j): A}, expected angles {(i, j, k): degrees}); w_intra = 0, no pocket
MINIMA = [
    ('C-C 1.70 -> 1.50', ['C', 'C'], f32([[0, 0, 0], [1.70, 0, 0]]), {(0, 1): 1.50}, {}),
    ('C-C 1.36 -> 1.34', ['C', 'C'], f32([[0, 0, 0], [0.8, 1.1, 0]]) * np.float32(1.0), {(0, 1): 1.34}, {}),
    ('chain 104 -> 109.47', ['C'] * 3, f32(chain(1.52, 1.52, 104.0)), {(0, 1): 1.50, (1, 2): 1.50}, {(0, 1, 2): 109.47122}),
    ('chain 124 -> 120', ['C'] * 3, f32(chain(1.50, 1.34, 124.0)), {(0, 1): 1.50, (1, 2): 1.34}, {(0, 1, 2): 120.0}),
    ('chain 170 -> 180', ['C'] * 3, f32(chain(1.46, 1.20, 170.0)), {(0, 1): 1.50, (1, 2): 1.20}, {(0, 1, 2): 180.0}),
    ('triangle keeps 60', ['C'] * 3, f32([[0, 0, 0], [1.53, 0, 0], [0.765, 1.53 * np.sqrt(0.75), 0]]), {(0, 1): 1.50, (0, 2): 1.50, (1, 2): 1.50},
     {(1, 0, 2): 60.0, (0, 1, 2): 60.0, (0, 2, 1): 60.0}),
]
assert abs(np.linalg.norm(MINIMA[1][2][1]) - 1.36) < 1e-3


def measure(pos, bonds, angles):
    """Bond lengths and angles (degrees) of pos for the keys of the two dicts."""
    p = np.asarray(pos, dtype=np.float64)
    L = {k: float(np.linalg.norm(p[k[0]] - p[k[1]])) for k in bonds}
    A = {}
    for (i, j, k) in angles:
        u, w = p[i] - p[j], p[k] - p[j]
        A[(i, j, k)] = float(np.degrees(np.arccos(np.clip(u @ w / np.linalg.norm(u) / np.linalg.norm(w), -1.0, 1.0))))
    return L, A
