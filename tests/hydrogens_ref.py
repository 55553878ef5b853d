"""Float64 restatement of the hydrogen placement rule of include/kpd.h (kpd_mol_add_hs), the yardstick of
test_hydrogens_config.py and test_hydrogens_gpu.py.  Same arithmetic as the kernel, in the same order: differences of the fp32
coordinates in float64, every product and sum rounded once (Python floats, no fused multiply-add), math.sqrt and `/` correctly
rounded; so every comparison against the GPU is exact equality, of the fp32 coordinates too.
Builds on molecule_ref.TABLE and on the outputs of sanitize_ref.sanitize (order_k, atom_h, atom_flags)."""
import math

import numpy as np

from .molecule_ref import BAD_SEGMENT, CAPACITY, EMPTY, MAX_ATOMS, TABLE
from .sanitize_ref import ATOM_AROMATIC, MAX_DEG, NO_MOLECULE as SAN_NO_MOLECULE

NO_MOLECULE, TOO_MANY_ATOMS, NO_ROOM, GENERAL, NONFINITE = 1, 2, 4, 8, 16
LINEAR, PLANAR, TET = 0, 1, 2
R_H = 32                                            # r1 of hydrogen, pm
THIRD, TET1 = 0.3333333333333333, 0.9428090415820634
S3, TET2, H3 = 0.5773502691896258, 0.816496580927726, 0.8660254037844386
TET_DIRS = ((1.0, 1.0, 1.0), (1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.0, -1.0, 1.0))


# ---- vectors: tuples of Python floats, every operation written out ------------------------------------------------------------
def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def over(a, s):
    return (a[0] / s, a[1] / s, a[2] / s)


def neg(a):
    return (-a[0], -a[1], -a[2])


def comb(x, a, y, b):
    """x a + y b, component by component: (x a_c) + (y b_c)."""
    return (x * a[0] + y * b[0], x * a[1] + y * b[1], x * a[2] + y * b[2])


def perp(u):
    e = 0
    if abs(u[1]) < abs(u[e]):
        e = 1
    if abs(u[2]) < abs(u[e]):
        e = 2
    ue = u[e]
    q = tuple((1.0 if c == e else 0.0) - ue * u[c] for c in range(3))
    return over(q, math.sqrt(dot(q, q)))


def directions(P, a, nbrs, cls, h):
    """The h unit directions of atom a and (general rule used, coincident neighbour ignored).  P: [n] tuples of floats; nbrs:
    {atom: ascending list of its neighbours in S}."""
    us, first, coincident = [], -1, False
    for b in nbrs[a]:
        v = sub(P[b], P[a])
        n2 = dot(v, v)
        if n2 < 1e-12:
            coincident = True
            continue
        if first < 0:
            first = b
        us.append(over(v, math.sqrt(n2)))
    k = len(us)

    def azimuth():
        u, b = us[0], first
        c = next((x for x in nbrs[b] if x != a), None)
        p0 = None
        if c is not None:
            w = sub(P[c], P[b])
            wu = dot(w, u)
            q = (w[0] - wu * u[0], w[1] - wu * u[1], w[2] - wu * u[2])
            qq = dot(q, q)
            if qq >= 1e-12:
                p0 = over(neg(q), math.sqrt(qq))
        if p0 is None:
            p0 = perp(u)
        t = cross(u, p0)
        return p0, comb(-0.5, p0, H3, t), comb(-0.5, p0, -H3, t)

    out = None
    if cls == TET and k == 0 and h <= 4:
        out = [(S3 * d[0], S3 * d[1], S3 * d[2]) for d in TET_DIRS[:h]]
    elif cls == TET and k == 1 and h <= 3:
        out = [comb(-THIRD, us[0], TET1, p) for p in azimuth()[:h]]
    elif cls == TET and k == 2 and h <= 2:
        s, x = add(us[0], us[1]), cross(us[0], us[1])
        ss, xx = dot(s, s), dot(x, x)
        if ss >= 1e-12 and xx >= 1e-12:
            w, n = over(neg(s), math.sqrt(ss)), over(x, math.sqrt(xx))
            out = [comb(S3, w, TET2, n), comb(S3, w, -TET2, n)][:h]
    elif cls == TET and k == 3 and h == 1:
        s = add(add(us[0], us[1]), us[2])
        x = cross(sub(us[1], us[0]), sub(us[2], us[0]))
        ss, xx = dot(s, s), dot(x, x)
        if xx >= 1e-12:
            n = over(x, math.sqrt(xx))
            out = [neg(n) if dot(n, s) > 0.0 else n]
        elif ss >= 1e-4:
            out = [over(neg(s), math.sqrt(ss))]
    elif cls == PLANAR and k == 1 and h <= 2:
        p0 = azimuth()[0]
        out = [comb(-0.5, us[0], H3, p0), comb(-0.5, us[0], -H3, p0)][:h]
    elif cls == PLANAR and k == 2 and h == 1:
        s = add(us[0], us[1])
        ss = dot(s, s)
        if ss >= 1e-4:
            out = [over(neg(s), math.sqrt(ss))]
    elif cls == LINEAR and k == 1 and h == 1:
        out = [neg(us[0])]
    if out is not None:
        return out, False, coincident
    out, s = [], (0.0, 0.0, 0.0)
    for u in us:
        s = add(s, u)
    for t in range(h):
        ss = dot(s, s)
        if k + t > 0 and ss >= 1e-4:
            d = over(neg(s), math.sqrt(ss))
        elif k + t > 0:
            d = perp(us[0] if k else out[0])
        else:
            d = (S3 * 1.0, S3 * 1.0, S3 * 1.0)
        out.append(d)
        s = add(s, d)
    return out, True, coincident


def add_hs(pos, elem, frag, bonds, order_k, atom_h, atom_flags, z, largest_only=False):
    """One ligand: pos [n,3] fp32, elem / frag / atom_h / atom_flags [n], bonds [m,2] local, order_k [m], z [F].  Returns None
    where there is no molecule (status bit 0), else a dict: h_eff [n] (hydrogens per atom, 0 outside S), h_pos [H,3] fp32 in
    output order, classes {atom: class}, general / coincident (sets of atoms), finite."""
    pos = np.asarray(pos, dtype=np.float32).reshape(-1, 3)
    n, F = pos.shape[0], len(z)
    elem, frag, atom_h = [int(e) for e in elem], [int(f) for f in frag], [int(x) for x in atom_h]
    bonds = [(int(i), int(j)) for i, j in bonds]
    order_k = [int(o) for o in order_k]
    if n <= 0 or n > MAX_ATOMS or any(e < 0 or e >= F for e in elem) or any(f < 0 or f >= n for f in frag):
        return None
    if any(x < 0 or x > 4 for x in atom_h):
        return None
    if any(not (0 <= i < j < n) or o < 1 or o > 3 for (i, j), o in zip(bonds, order_k)):
        return None
    if any(bonds[r - 1] >= bonds[r] for r in range(1, len(bonds))):         # rows in (i, j) order, none twice
        return None
    if largest_only:
        rank = int(np.argmax(np.bincount(frag, minlength=n)))
        inS = [f == rank for f in frag]
    else:
        inS = [True] * n
    nb = {a: {} for a in range(n) if inS[a]}
    for row, (i, j) in enumerate(bonds):
        if not (inS[i] and inS[j]):
            continue
        if len(nb[i]) >= MAX_DEG or len(nb[j]) >= MAX_DEG:
            return None
        nb[i][j] = nb[j][i] = row
    Z = [int(z[e]) if 0 <= int(z[e]) <= 255 else 0 for e in elem]
    h_eff = [atom_h[a] if inS[a] else 0 for a in range(n)]
    res = dict(h_eff=h_eff, inS=inS, Z=Z, finite=bool(np.isfinite(pos).all()), classes={}, general=set(), coincident=set(),
               h_pos=np.zeros((0, 3), dtype=np.float32))
    if not res['finite'] or n + sum(h_eff) > MAX_ATOMS:
        return res
    P = [tuple(float(v) for v in row) for row in pos]
    nbrs = {a: sorted(nb[a]) for a in nb}
    top = {a: [order_k[r] for r in nb[a].values()] for a in nb}
    out = []
    for a in sorted(nb):
        if not h_eff[a]:
            continue
        if 3 in top[a] or top[a].count(2) >= 2:
            cls = LINEAR
        elif 2 in top[a] or (int(atom_flags[a]) & ATOM_AROMATIC) or (
                Z[a] == 7 and any((int(atom_flags[b]) & ATOM_AROMATIC) or max(top[b]) >= 2 for b in nbrs[a])):
            cls = PLANAR
        else:
            cls = TET
        res['classes'][a] = cls
        ds, general, coincident = directions(P, a, nbrs, cls, h_eff[a])
        if general:
            res['general'].add(a)
        if coincident:
            res['coincident'].add(a)
        L = float(TABLE.get(Z[a], (0, 0, 0, 0))[0] + R_H) * 0.01
        for d in ds:
            out.append([np.float32(P[a][c] + L * d[c]) for c in range(3)])
    res['h_pos'] = np.array(out, dtype=np.float32).reshape(-1, 3)
    return res


def bond_length(zz):
    return float(TABLE.get(int(zz), (0, 0, 0, 0))[0] + R_H) * 0.01


def add_hs_batch(pos, ptr, mol, san, z, allowed, h_class, largest_only=False, cap_atoms=None, cap_bonds=None):
    """The outputs of kpd_mol_add_hs for a batch, in its layout.  `mol`: elem / frag [N], bonds [cap,2] (global rows), bond_ptr
    [B+1], status [B]; `san`: order_k [cap], valence_k / atom_h / atom_flags [N], status [B] (sanitize_batch's, or hand-written).
    Returns out_ptr / out_bond_ptr [B+1], pos [cap_atoms,3] fp32 (0 where nothing is written), elem / valence / frag / parent /
    source [cap_atoms] (-1 where nothing is written), bonds [cap_bonds,2] (-1), order [cap_bonds] (0), summary [B,4], n_h /
    status [B], and `mols`: the per-ligand dicts of add_hs (None where there is no molecule)."""
    pos = np.asarray(pos, dtype=np.float32).reshape(-1, 3)
    N, B, cap_in = pos.shape[0], len(ptr) - 1, len(san['order_k'])
    plan = []
    for b in range(B):
        a0, a1 = int(ptr[b]), int(ptr[b + 1])
        if not (0 <= a0 <= a1 <= N):
            plan.append(dict(n=0, m=0, H=0, status=NO_MOLECULE, res=None, a0=0, p0=0))
            continue
        n = a1 - a0
        p0, p1 = int(mol['bond_ptr'][b]), int(mol['bond_ptr'][b + 1])
        rng = p0 >= 0 and p1 >= p0 and p1 <= cap_in and p1 - p0 <= 3 * MAX_ATOMS
        m = p1 - p0 if rng else 0
        ok = (rng and 0 < n <= MAX_ATOMS and not (int(mol['status'][b]) & (EMPTY | CAPACITY | BAD_SEGMENT)) and
              not (int(san['status'][b]) & SAN_NO_MOLECULE) and int(z[h_class]) == 1)
        res = None
        if ok:
            res = add_hs(pos[a0:a1], mol['elem'][a0:a1], mol['frag'][a0:a1], np.asarray(mol['bonds'][p0:p1]).reshape(-1, 2) - a0,
                         san['order_k'][p0:p1], san['atom_h'][a0:a1], san['atom_flags'][a0:a1], z, largest_only)
            if res is not None and not any(res['inS']):
                res = None
        status, H = 0, 0
        if res is None:
            status = NO_MOLECULE
        elif not res['finite']:
            status = NONFINITE
        elif n + sum(res['h_eff']) > MAX_ATOMS:
            status = TOO_MANY_ATOMS
        else:
            H = sum(res['h_eff'])
            status = GENERAL if (res['general'] or res['coincident']) else 0
        plan.append(dict(n=n, m=m, H=H, status=status, res=res, a0=a0, p0=p0))
    out_ptr = np.concatenate([[0], np.cumsum([p['n'] + p['H'] for p in plan])]).astype(np.int64)
    out_bptr = np.concatenate([[0], np.cumsum([p['m'] + p['H'] for p in plan])]).astype(np.int64)
    ca = int(out_ptr[B]) if cap_atoms is None else cap_atoms
    cb = int(out_bptr[B]) if cap_bonds is None else cap_bonds
    neg1 = lambda k: np.full(k, -1, dtype=np.int64)
    out = dict(out_ptr=out_ptr, out_bond_ptr=out_bptr, pos=np.zeros((ca, 3), dtype=np.float32), elem=neg1(ca), valence=neg1(ca),
               frag=neg1(ca), parent=neg1(ca), source=neg1(ca), bonds=np.full((cb, 2), -1, dtype=np.int64),
               order=np.zeros(cb, dtype=np.int64), summary=np.zeros((B, 4), dtype=np.int64), n_h=np.zeros(B, dtype=np.int64),
               status=np.zeros(B, dtype=np.int64), mols=[p['res'] for p in plan])
    for b, p in enumerate(plan):
        n, m, H, res, a0, p0 = p['n'], p['m'], p['H'], p['res'], p['a0'], p['p0']
        o0, o1, q0, q1 = int(out_ptr[b]), int(out_ptr[b + 1]), int(out_bptr[b]), int(out_bptr[b + 1])
        out['n_h'][b] = H
        h_eff = res['h_eff'] if (res is not None and H) else [0] * n
        before = np.concatenate([[0], np.cumsum(h_eff)]).astype(np.int64)       # hydrogens of the atoms < i
        fits = o1 <= ca and q1 <= cb
        out['status'][b] = p['status'] | (0 if fits else NO_ROOM)
        val = [int(san['valence_k'][a0 + a]) + h_eff[a] for a in range(n)] + [1] * H
        cls = [int(mol['elem'][a0 + a]) for a in range(n)] + [h_class] * H
        frag = [int(mol['frag'][a0 + a]) for a in range(n)]
        parent = list(range(n))
        for a in range(n):
            parent += [a] * h_eff[a]
        frag += [frag[a] for a in parent[n:]]
        if res is None:
            out['summary'][b] = [m + H, 0, 0, 0]
        else:
            sizes = np.bincount(frag, minlength=n)
            invalid = sum(1 for v, c in zip(val, cls) if v == 0 or v > int(allowed[c]) or int(z[c]) not in TABLE)
            out['summary'][b] = [m + H, int((sizes > 0).sum()), int(sizes.max()), invalid]
        if not fits:
            continue
        out['pos'][o0:o0 + n] = pos[a0:a0 + n]
        if H:
            out['pos'][o0 + n:o1] = res['h_pos']
        out['elem'][o0:o1], out['valence'][o0:o1], out['frag'][o0:o1] = cls, val, frag
        out['parent'][o0:o1] = np.asarray(parent) + o0
        out['source'][o0:o1] = list(range(a0, a0 + n)) + [-1] * H
        rows_upto = np.zeros(n, dtype=np.int64)                             # bond rows whose first atom is <= i
        for r in range(m):
            i, j = (int(x) - a0 for x in mol['bonds'][p0 + r])
            at = r + (int(before[i]) if H else 0)
            out['bonds'][q0 + at] = [i + o0, j + o0]
            out['order'][q0 + at] = int(san['order_k'][p0 + r])
            if H:
                rows_upto[i:] += 1
        if H:
            for a in range(n):
                for s in range(h_eff[a]):
                    at = int(rows_upto[a]) + int(before[a]) + s
                    out['bonds'][q0 + at] = [a + o0, n + int(before[a]) + s + o0]
                    out['order'][q0 + at] = 1
    return out
