"""Float64 numpy restatement of the scoring function of include/kpd.h (kpd_vina_pocket_types, kpd_vina_score), the yardstick of
test_vina_gpu.py.  d2 = (dx*dx + dy*dy) + dz*dz in float64 on exact differences of the fp32 coordinates, r = sqrt(d2),
d = (r - R_i) - R_j: the cutoff and every branch are decided as in the kernel.  Typing and the rotor count are integers and
compare exactly; the sums compare within `tolerances`."""
import numpy as np

from .molecule_ref import TABLE, _test

H, D, A = 1, 2, 4
NO_MOLECULE, BAD_INPUT, ATOM_OUT = 1, 2, 4
HALOGENS, METALS = (9, 17, 35, 53), (12, 20, 25, 26, 27, 28, 29, 30)
WEIGHTS = ('w_gauss1', 'w_gauss2', 'w_repulsion', 'w_hydrophobic', 'w_hbond')
DEFAULTS = dict(w_gauss1=-0.035579, w_gauss2=-0.005156, w_repulsion=0.840245, w_hydrophobic=-0.035069, w_hbond=-0.587439,
                w_rot=0.05846, r_c=8.0)


def flags(z, nbr_z, nbr_order):
    """The flags of one atom: its atomic number, and the atomic numbers and bond orders of its neighbours."""
    heavy = [(zz, o) for zz, o in zip(nbr_z, nbr_order) if zz != 1]
    deg = len(heavy)
    if z == 6:
        return 0 if any(zz != 6 for zz, _ in heavy) else H
    if z in HALOGENS:
        return H
    if z == 7:
        if deg > 2:
            return 0
        return A if (deg == 1 and heavy[0][1] == 3) else D
    if z == 8:
        return A | (D if deg == 0 or (deg == 1 and heavy[0][1] == 1) else 0)
    if z in METALS:
        return D
    return 0


def _neighbours(n, bonds, orders):
    nb = [[] for _ in range(n)]
    for (i, j), o in zip(np.asarray(bonds).reshape(-1, 2).tolist(), list(orders)):
        nb[i].append((j, int(o)))
        nb[j].append((i, int(o)))
    return nb


def ligand_types(z_atoms, bonds, orders, radius, type_in=None):
    """Types [n] of one ligand: z_atoms [n] atomic numbers, bonds [m,2] local, orders [m], radius [n] float32; -1 takes no part."""
    n = len(z_atoms)
    nb = _neighbours(n, bonds, orders)
    out = np.zeros(n, dtype=np.int64)
    for a in range(n):
        f = flags(int(z_atoms[a]), [int(z_atoms[j]) for j, _ in nb[a]], [o for _, o in nb[a]])
        if type_in is not None and int(type_in[a]) >= 0:
            f = int(type_in[a]) & 7
        out[a] = -1 if (int(z_atoms[a]) == 1 or not np.float32(radius[a]) > 0) else f
    return out


def pocket_bonds(pos, z):
    """The neighbour pairs of one pocket (step 1 of the bond rule, no pruning) and their step-3 orders: adj [m,m] bool, order [m,m]."""
    pos, z = np.asarray(pos, dtype=np.float32).reshape(-1, 3), np.asarray(z, dtype=np.int64)
    rows = np.array([TABLE.get(int(v), (0, 0, 0, 0)) for v in z], dtype=np.int64).reshape(-1, 4)[:, :3].copy()
    finite = np.isfinite(pos).all(axis=1)
    rows[~finite] = 0
    p = pos.astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        dx, dy, dz = (p[:, None, c] - p[None, :, c] for c in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        adj = (d2 > 0.16) & _test(d2, rows[:, 0], rows[:, 0], 45)
        t3, t2 = _test(d2, rows[:, 2], rows[:, 2], 3), _test(d2, rows[:, 1], rows[:, 1], 5)
    np.fill_diagonal(adj, False)
    return adj, np.where(t3, 3, np.where(t2, 2, 1))


def pocket_types(pos, z):
    """(types [m], status) of one pocket: pos [m,3] float32, z [m] atomic numbers."""
    pos, z = np.asarray(pos, dtype=np.float32).reshape(-1, 3), np.asarray(z, dtype=np.int64)
    m = len(z)
    if m == 0:
        return np.zeros(0, dtype=np.int64), 0
    finite = np.isfinite(pos).all(axis=1)
    adj, order = pocket_bonds(pos, z)
    out = np.zeros(m, dtype=np.int64)
    for a in range(m):
        js = np.nonzero(adj[a])[0]
        out[a] = -1 if (not finite[a] or z[a] == 1) else flags(int(z[a]), z[js].tolist(), order[a, js].tolist())
    return out, (0 if finite.all() else 2)


def rotors(z_atoms, bonds, orders):
    """N_rot: bonds of order 1 whose ends both have heavy degree >= 2 and stay disconnected when the bond is removed."""
    n = len(z_atoms)
    bonds = np.asarray(bonds).reshape(-1, 2).tolist()
    nb = _neighbours(n, bonds, orders)
    hdeg = [sum(1 for j, _ in nb[a] if int(z_atoms[j]) != 1) for a in range(n)]
    count = 0
    for (i, j), o in zip(bonds, list(orders)):
        if int(o) != 1 or hdeg[i] < 2 or hdeg[j] < 2:
            continue
        seen, todo = {i}, [i]
        while todo:
            u = todo.pop()
            for v, _ in nb[u]:
                if (u == i and v == j) or (u == j and v == i) or v in seen:
                    continue
                seen.add(v)
                todo.append(v)
        count += j not in seen
    return count


def pair_terms(d, hydrophobic, hbond):
    """The five unweighted terms and their derivatives with respect to d, for arrays d and the two boolean masks."""
    u, v = d / 0.5, (d - 3.0) / 2.0
    g1, g2 = np.exp(-(u * u)), np.exp(-(v * v))
    t = np.stack([g1, g2, np.where(d < 0, d * d, 0.0),
                  np.where(hydrophobic, np.where(d < 0.5, 1.0, np.where(d < 1.5, 1.5 - d, 0.0)), 0.0),
                  np.where(hbond, np.where(d < -0.7, 1.0, np.where(d < 0, d / -0.7, 0.0)), 0.0)])
    dt = np.stack([-4.0 * u * g1, -v * g2, np.where(d < 0, 2.0 * d, 0.0),
                   np.where(hydrophobic & (d >= 0.5) & (d < 1.5), -1.0, 0.0),
                   np.where(hbond & (d >= -0.7) & (d < 0), 1.0 / -0.7, 0.0)])
    return t, dt


def evaluate(pos, types, radius, ppos, ptypes, pradius, n_rot, params=None):
    """One evaluation.  pos [n,3] (float32, or float64 for the finite-difference test), types [n], radius [n] float32; the pocket
    likewise.  Returns terms [5] (weighted), inter, score, grad [n,3], atom_score [n], the surface distances `d` and the mask
    `on` of the pairs that take part, and the sums of absolute values `tolerances` reads."""
    P = dict(DEFAULTS, **(params or {}))
    w = np.array([P[k] for k in WEIGHTS], dtype=np.float64)
    x, q = np.asarray(pos).astype(np.float64).reshape(-1, 3), np.asarray(ppos).astype(np.float64).reshape(-1, 3)
    types, ptypes = np.asarray(types, dtype=np.int64), np.asarray(ptypes, dtype=np.int64)
    R, Q = np.asarray(radius, dtype=np.float32).astype(np.float64), np.asarray(pradius, dtype=np.float32).astype(np.float64)
    n, m = len(x), len(q)
    diff = x[:, None, :] - q[None, :, :]
    d2 = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
    part_i, part_j = types >= 0, (ptypes >= 0) & (Q > 0)
    on = (d2 < P['r_c'] * P['r_c']) & part_i[:, None] & part_j[None, :]
    r = np.sqrt(d2)
    d = (r - R[:, None]) - Q[None, :]
    ti, tj = np.where(part_i, types, 0), np.where(part_j, ptypes & 7, 0)
    hyd = ((ti[:, None] & H) != 0) & ((tj[None, :] & H) != 0)
    hb = (((ti[:, None] & D) != 0) & ((tj[None, :] & A) != 0)) | (((ti[:, None] & A) != 0) & ((tj[None, :] & D) != 0))
    t, dt = pair_terms(d, hyd, hb)
    t, dt = np.where(on[None], t, 0.0), np.where(on[None], dt, 0.0)
    norm = 1.0 + P['w_rot'] * n_rot
    terms = w * t.sum(axis=(1, 2))
    wt = (w[:, None, None] * t)
    k = np.where(r >= 1e-6, (w[:, None, None] * dt).sum(axis=0) / np.where(r >= 1e-6, r, 1.0), 0.0)
    contrib = k[..., None] * diff
    inter = terms.sum()
    return dict(terms=terms, inter=inter, score=inter / norm, n_rot=n_rot, grad=contrib.sum(axis=1) / norm, atom_score=wt.sum(axis=(0, 2)),
                d=d, on=on, d2=d2, abs_terms=np.abs(wt).sum(), abs_atom=np.abs(wt).sum(axis=(0, 2)),
                abs_grad=np.abs(contrib).sum(axis=1) / norm)


def tolerances(e, factor):
    """(for the terms, inter and score; for grad [n,3]; for atom_score [n]): `factor` times the sum of the absolute weighted pair
    terms (of the absolute gradient contributions per component; of the atom's absolute terms).  Two fp64 sums of the same terms
    in different orders, with exp off by an ulp, differ by a small multiple of 1e-16 times the number of terms of that sum."""
    return factor * e['abs_terms'], factor * e['abs_grad'], factor * e['abs_atom']


def score_ligand(pos, z_atoms, bonds, orders, radius, ppos, pz, pradius, params=None, type_in=None, ptypes=None):
    """Typing, rotors and one evaluation of one ligand in one pocket; the pocket is typed here unless `ptypes` is given."""
    types = ligand_types(z_atoms, bonds, orders, radius, type_in)
    if ptypes is None:
        ptypes = pocket_types(ppos, pz)[0]
    e = evaluate(pos, types, radius, ppos, ptypes, pradius, rotors(z_atoms, bonds, orders), params)
    e.update(types=types, ptypes=np.asarray(ptypes))
    return e
