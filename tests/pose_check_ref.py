"""The plausibility checks of include/kpd.h (kpd_pose_check) restated in plain Python floats, in the header's operation order: every
product, sum, difference and quotient is one IEEE double operation, math.sqrt is correctly rounded, and every per-pose result is a
minimum, a maximum or an integer count, so the kernel has to agree with this file in every bit.  Nothing here is shared with the
library.  The lattice count of check 6 exists twice: `lattice_counts` walks the box of every atom (the kernel's plan) and
`lattice_brute` walks one box around the whole ligand and asks every point about every atom; the tests hold them equal.
`margins` (optional) collects |value - threshold| of every comparison against a threshold of the params, so that a test can assert
that no case sits on a threshold; the membership tests of the lattice (d2 <= R R) are exact on both sides and are not collected."""
import math

import numpy as np

NO_MOLECULE, BAD_INPUT, ATOM_OUT = 1, 2, 4
F_BOND, F_ANGLE, F_CLASH, F_RING, F_CENTRE, F_TWIST, F_POCKET, F_OVERLAP = (1 << k for k in range(8))
FAIL_NAMES = ('bond', 'angle', 'clash', 'ring', 'centre', 'twist', 'pocket', 'overlap')
REPORT = ('bond_min', 'bond_max', 'angle_min', 'angle_max', 'clash_min', 'ring_max', 'centre_max', 'twist_min', 'pocket_min', 'overlap')
COUNTS = ('bonds', 'bonds_fail', 'angles', 'angles_fail', 'pairs', 'pairs_fail', 'rings', 'rings_fail', 'centres', 'centres_fail',
          'torsions', 'torsions_fail', 'torsions_skipped', 'pocket_pairs', 'pocket_pairs_fail', 'n_lig_points', 'n_overlap_points')
DEFAULTS = dict(bond_lo=0.75, bond_hi=1.25, angle_lo=0.75, angle_hi=1.25, clash_min=0.7, ring_max=0.25, centre_max=0.25, twist_min=0.75,
                pocket_min=0.75, pocket_scale=0.8, overlap_max=0.075, h=0.5)
MOL_MAX, MOL_DEG, MAX_H, MAX_COORD, MAX_RADIUS, T3, TINY = 256, 6, 9, 1048576.0, 8.0, 0.3333333333333333, 1e-12
AROM, RING = 4, 1                # bond_flags bits
AT_AROMATIC = 2                  # atom_flags bit

# r1, r2, r3 of the element table of include/kpd.h (pm)
RADII = {1: (32, 0, 0), 5: (85, 78, 0), 6: (75, 67, 60), 7: (71, 60, 54), 8: (63, 57, 0), 9: (64, 0, 0), 14: (116, 0, 0), 15: (111, 102, 0),
         16: (103, 94, 0), 17: (99, 0, 0), 33: (121, 0, 0), 35: (114, 0, 0), 53: (133, 0, 0)}


# ---- vectors, every operation rounded once ---------------------------------------------------------------------------------------------
def vsub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def vadd(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def vdot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def vcross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def vover(a, s):
    return (a[0] / s, a[1] / s, a[2] / s)


def d2(a, b):
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return (dx * dx + dy * dy) + dz * dz


def r0_half(za, zb, order, aromatic):
    ra, rb = RADII.get(za, (0, 0, 0)), RADII.get(zb, (0, 0, 0))
    if not ra[0] or not rb[0]:
        return 0
    L1 = 2 * (ra[0] + rb[0])
    L2 = 2 * (ra[1] + rb[1]) if ra[1] and rb[1] else 0
    L3 = 2 * (ra[2] + rb[2]) if ra[2] and rb[2] else 0
    if aromatic:
        return (L1 + L2) // 2 if L2 else L1
    if order == 3:
        return L3 or L1
    if order == 2:
        return L2 or L1
    return L1


# ---- check 6 ---------------------------------------------------------------------------------------------------------------------------
def _axis_range(c, R, h):
    return int(math.floor((c - R) / h - 1e-3)), int(math.floor((c + R) / h + 1e-3))


def _in_pocket(pt, pocket, scale):
    for q, r in pocket:
        sr = scale * r
        if d2(pt, q) <= sr * sr:
            return True
    return False


def lattice_counts(atoms, pocket, h, scale):
    """atoms: [(index, P, R)] taking part, ascending index; pocket: [(Q, R)] taking part.  Returns (n_lig_points, n_overlap_points,
    the atoms that own an overlapping point).  The kernel's plan: the box of every atom, a point counted at its lowest atom."""
    n_lig = n_over = 0
    owners = set()
    for t, (a, P, R) in enumerate(atoms):
        R2 = R * R
        rx, ry, rz = (_axis_range(P[c], R, h) for c in range(3))
        for iz in range(rz[0], rz[1] + 1):
            for iy in range(ry[0], ry[1] + 1):
                for ix in range(rx[0], rx[1] + 1):
                    pt = (h * float(ix), h * float(iy), h * float(iz))
                    if not d2(pt, P) <= R2:
                        continue
                    if any(d2(pt, P2) <= R2b * R2b for _, P2, R2b in atoms[:t]):
                        continue
                    n_lig += 1
                    if _in_pocket(pt, pocket, scale):
                        n_over += 1
                        owners.add(a)
    return n_lig, n_over, owners


def lattice_brute(atoms, pocket, h, scale):
    """The same two counts by brute force: every lattice point of one box around all spheres (two points wider than needed on
    every side), asked about every atom."""
    if not atoms:
        return 0, 0
    lo = [int(math.floor(min(P[c] - R for _, P, R in atoms) / h)) - 2 for c in range(3)]
    hi = [int(math.floor(max(P[c] + R for _, P, R in atoms) / h)) + 2 for c in range(3)]
    n_lig = n_over = 0
    for ix in range(lo[0], hi[0] + 1):
        for iy in range(lo[1], hi[1] + 1):
            for iz in range(lo[2], hi[2] + 1):
                pt = (h * float(ix), h * float(iy), h * float(iz))
                if any(d2(pt, P) <= R * R for _, P, R in atoms):
                    n_lig += 1
                    n_over += _in_pocket(pt, pocket, scale)
    return n_lig, n_over


# ---- one pose ----------------------------------------------------------------------------------------------------------------------------
def _graph(n, a0, elem, frag, z, F, bonds, order_k, bond_flags, p0, p1, atom_h, atom_flags, largest):
    """The front end: None for "no molecule", else (S, nbrs, zv, arom_atom).  nbrs[a] = [(partner, order, aromatic, ring)] ascending."""
    zv = []
    for a in range(n):
        e, f, h = int(elem[a0 + a]), int(frag[a0 + a]), int(atom_h[a0 + a])
        if not (0 <= e < F and 0 <= f < n and 0 <= h <= MAX_H):
            return None
        zz = int(z[e])
        zv.append(zz if 0 <= zz <= 255 else 0)
    fr = [int(frag[a0 + a]) for a in range(n)]
    if largest:
        size = {}
        for f in fr:
            size[f] = size.get(f, 0) + 1
        best = max(size, key=lambda f: (size[f], -f))
        S = [a for a in range(n) if fr[a] == best]
    else:
        S = list(range(n))
    inS = set(S)
    nbrs = {a: [] for a in S}
    seen = set()
    for k in range(p0, p1):
        i, j, o = int(bonds[k][0]) - a0, int(bonds[k][1]) - a0, int(order_k[k])
        if not (0 <= i < n and 0 <= j < n and i != j and 1 <= o <= 3):
            return None
        if i not in inS or j not in inS:
            continue
        key = (min(i, j), max(i, j))
        if key in seen:
            return None
        seen.add(key)
        fl = int(bond_flags[k])
        nbrs[i].append((j, o, bool(fl & AROM), bool(fl & RING)))
        nbrs[j].append((i, o, bool(fl & AROM), bool(fl & RING)))
    for a in S:
        if len(nbrs[a]) > MOL_DEG or any(fr[e[0]] != fr[a] for e in nbrs[a]):
            return None
        nbrs[a].sort()
    if not S:
        return None
    return S, nbrs, zv, [bool(int(atom_flags[a0 + a]) & AT_AROMATIC) for a in range(n)]


def check_pose(S, nbrs, zv, arom_atom, P, R, pocket, has_pocket, prm, margins=None, lattice=lattice_counts):
    """P [n] tuples and R [n] floats of the ligand, pocket: [(Q, R)] of the pocket atoms that take part.  Returns (fail, report,
    counts, atom_fail dict)."""
    inf = math.inf
    cnt = dict.fromkeys(COUNTS, 0)
    ext = dict(bond_min=inf, bond_max=-inf, angle_min=inf, angle_max=-inf, clash_min=inf, ring_max=-inf, centre_max=-inf, twist_min=inf,
               pocket_min=inf)
    af = {}

    def mark(bit, *atoms):
        for a in atoms:
            af[a] = af.get(a, 0) | bit

    def near(v, *thresholds):
        if margins is not None:
            margins.extend(abs(v - t) for t in thresholds)

    bonded = {(a, e[0]) for a in S for e in nbrs[a]}
    info = {}
    for a in S:
        orders = [e[1] for e in nbrs[a]]
        info[a] = dict(triple=3 in orders, doubles=orders.count(2), arom=arom_atom[a])
    unsat = lambda a: info[a]['triple'] or info[a]['doubles'] >= 1 or info[a]['arom']

    def cls(a):
        i = info[a]
        if i['triple'] or i['doubles'] >= 2:
            return 'LINEAR'
        if i['doubles'] >= 1 or i['arom'] or (zv[a] == 7 and any(unsat(e[0]) for e in nbrs[a])):
            return 'PLANAR'
        return 'TET'

    r0 = lambda a, e: r0_half(zv[a], zv[e[0]], e[1], e[2])
    for a in S:
        # check 1 and the twist
        for e in nbrs[a]:
            b = e[0]
            if b < a:
                continue
            L = r0(a, e)
            if L:
                v = math.sqrt(d2(P[a], P[b])) / (float(L) * 0.005)
                cnt['bonds'] += 1
                ext['bond_min'], ext['bond_max'] = min(ext['bond_min'], v), max(ext['bond_max'], v)
                near(v, prm['bond_lo'], prm['bond_hi'])
                if v < prm['bond_lo'] or v > prm['bond_hi']:
                    cnt['bonds_fail'] += 1
                    mark(F_BOND, a, b)
            if e[1] != 2 or e[3]:
                continue
            b2 = vsub(P[b], P[a])
            for ec in nbrs[a]:
                c = ec[0]
                if c == b:
                    continue
                n1 = vcross(vsub(P[a], P[c]), b2)
                n11 = vdot(n1, n1)
                for ed in nbrs[b]:
                    d = ed[0]
                    if d == a:
                        continue
                    n2 = vcross(b2, vsub(P[d], P[b]))
                    n22 = vdot(n2, n2)
                    near(n11, TINY)
                    near(n22, TINY)
                    if n11 < TINY or n22 < TINY:
                        cnt['torsions_skipped'] += 1
                        continue
                    dd = vdot(n1, n2)
                    v = (dd * dd) / (n11 * n22)
                    cnt['torsions'] += 1
                    ext['twist_min'] = min(ext['twist_min'], v)
                    near(v, prm['twist_min'])
                    if v < prm['twist_min']:
                        cnt['torsions_fail'] += 1
                        mark(F_TWIST, a, b, c, d)
        # check 2
        dg = len(nbrs[a])
        if dg >= 2:
            k = cls(a)
            if dg >= 4:
                cos0 = -T3
            elif dg == 3:
                cos0 = -T3 if k == 'TET' else -0.5
            else:
                cos0 = {'LINEAR': -1.0, 'PLANAR': -0.5, 'TET': -T3}[k]
            for s in range(dg):
                for t in range(s + 1, dg):
                    ei, eq = nbrs[a][s], nbrs[a][t]
                    Li, Lq = r0(a, ei), r0(a, eq)
                    if not Li or not Lq or (ei[0], eq[0]) in bonded:
                        continue
                    x, y = float(Li) * 0.005, float(Lq) * 0.005
                    d0sq = ((x * x) + (y * y)) - (((2.0 * x) * y) * cos0)
                    v = math.sqrt(d2(P[ei[0]], P[eq[0]])) / math.sqrt(d0sq)
                    cnt['angles'] += 1
                    ext['angle_min'], ext['angle_max'] = min(ext['angle_min'], v), max(ext['angle_max'], v)
                    near(v, prm['angle_lo'], prm['angle_hi'])
                    if v < prm['angle_lo'] or v > prm['angle_hi']:
                        cnt['angles_fail'] += 1
                        mark(F_ANGLE, a, ei[0], eq[0])
        # check 3
        if R[a] > 0.0:
            ball = {a}
            for _ in range(3):
                ball |= {e[0] for x in ball for e in nbrs[x]}
            for b in S:
                if b <= a or b in ball or not R[b] > 0.0:
                    continue
                v = math.sqrt(d2(P[a], P[b])) / (R[a] + R[b])
                cnt['pairs'] += 1
                ext['clash_min'] = min(ext['clash_min'], v)
                near(v, prm['clash_min'])
                if v < prm['clash_min']:
                    cnt['pairs_fail'] += 1
                    mark(F_CLASH, a, b)
        # check 4, planar centres
        if dg == 3 and (info[a]['doubles'] >= 1 or info[a]['arom']):
            q = [P[e[0]] for e in nbrs[a]]
            N = vcross(vsub(q[1], q[0]), vsub(q[2], q[0]))
            n2 = vdot(N, N)
            cnt['centres'] += 1
            fails = True
            near(n2, TINY)
            if n2 >= TINY:
                v = abs(vdot(vsub(P[a], q[0]), vover(N, math.sqrt(n2))))
                ext['centre_max'] = max(ext['centre_max'], v)
                near(v, prm['centre_max'])
                fails = v > prm['centre_max']
            if fails:
                cnt['centres_fail'] += 1
                mark(F_CENTRE, a)
    # check 4, aromatic rings: simple cycles of 5 and 6 over the aromatic bonds, from the lowest atom towards its lower ring neighbour
    arom_nb = {a: [e[0] for e in nbrs[a] if e[2]] for a in S}
    rings = []

    def walk(path):
        for v in arom_nb[path[-1]]:
            if v == path[0] and len(path) in (5, 6) and path[1] < path[-1]:
                rings.append(list(path))
            if v > path[0] and v not in path and len(path) < 6:
                walk(path + [v])

    for a in S:
        walk([a])
    for ring in rings:
        m = len(ring)
        c = P[ring[0]]
        for t in range(1, m):
            c = vadd(c, P[ring[t]])
        c = vover(c, float(m))
        N = (0.0, 0.0, 0.0)
        for t in range(m):
            N = vadd(N, vcross(vsub(P[ring[t]], c), vsub(P[ring[(t + 1) % m]], c)))
        n2 = vdot(N, N)
        cnt['rings'] += 1
        fails = True
        near(n2, TINY)
        if n2 >= TINY:
            u = vover(N, math.sqrt(n2))
            v = max(abs(vdot(vsub(P[t], c), u)) for t in ring)
            ext['ring_max'] = max(ext['ring_max'], v)
            near(v, prm['ring_max'])
            fails = v > prm['ring_max']
        if fails:
            cnt['rings_fail'] += 1
            mark(F_RING, *ring)
    # checks 5 and 6
    overlap = 0.0
    owners = set()
    if has_pocket:
        takes = [(a, P[a], R[a]) for a in S if R[a] > 0.0]
        for Q, Rj in pocket:
            for a, Pa, Ra in takes:
                v = math.sqrt(d2(Pa, Q)) / (Ra + Rj)
                cnt['pocket_pairs'] += 1
                ext['pocket_min'] = min(ext['pocket_min'], v)
                near(v, prm['pocket_min'])
                if v < prm['pocket_min']:
                    cnt['pocket_pairs_fail'] += 1
                    mark(F_POCKET, a)
        out = lattice(takes, pocket, prm['h'], prm['pocket_scale'])
        cnt['n_lig_points'], cnt['n_overlap_points'] = out[0], out[1]
        owners = out[2] if len(out) > 2 else set()
        if cnt['n_lig_points']:
            overlap = float(cnt['n_overlap_points']) / float(cnt['n_lig_points'])
        near(overlap, prm['overlap_max'])
    overlap_fails = overlap > prm['overlap_max']
    if overlap_fails:
        mark(F_OVERLAP, *owners)
    rep = [ext['bond_min'] if cnt['bonds'] else 0.0, ext['bond_max'] if cnt['bonds'] else 0.0, ext['angle_min'] if cnt['angles'] else 0.0,
           ext['angle_max'] if cnt['angles'] else 0.0, ext['clash_min'] if cnt['pairs'] else 0.0, max(ext['ring_max'], 0.0),
           max(ext['centre_max'], 0.0), ext['twist_min'] if cnt['torsions'] else 0.0, ext['pocket_min'] if cnt['pocket_pairs'] else 0.0, overlap]
    fail = ((F_BOND if cnt['bonds_fail'] else 0) | (F_ANGLE if cnt['angles_fail'] else 0) | (F_CLASH if cnt['pairs_fail'] else 0) |
            (F_RING if cnt['rings_fail'] else 0) | (F_CENTRE if cnt['centres_fail'] else 0) | (F_TWIST if cnt['torsions_fail'] else 0) |
            (F_POCKET if cnt['pocket_pairs_fail'] else 0) | (F_OVERLAP if overlap_fails else 0))
    return fail, rep, [cnt[k] for k in COUNTS], af


def _f32_ok_coord(x):
    return abs(float(x)) < MAX_COORD            # False for NaN


def pose_check_batch(ptr, mol, san, z, pos, lig_radius, pocket=None, largest=False, max_atoms=MOL_MAX, params=None, margins=None,
                     lattice=lattice_counts):
    """The whole call.  ptr [B+1]; mol: elem, frag, bonds [cap,2], bond_ptr, status; san: order_k, bond_flags, atom_h, atom_flags,
    status; z [F]; pos [K,N,3] float32; lig_radius [F] float32; pocket: None or dict(x [M,3] float32, radius [M] float32, ptr [P+1],
    of [B]).  Returns dict(fail [B,K], report [B,K,10], counts [B,K,17], atom_fail [K,N], status [B,K])."""
    prm = dict(DEFAULTS, **(params or {}))
    pos = np.asarray(pos, dtype=np.float32)
    K, N = pos.shape[0], pos.shape[1]
    B, F = len(ptr) - 1, len(z)
    bonds = np.asarray(mol['bonds']).reshape(-1, 2)
    cap = len(bonds)
    lig_radius = np.asarray(lig_radius, dtype=np.float32)
    if pocket is None:
        pocket = dict(x=np.zeros((0, 3), np.float32), radius=np.zeros(0, np.float32), ptr=[0], of=[-1] * B)
    px, pr = np.asarray(pocket['x'], dtype=np.float32).reshape(-1, 3), np.asarray(pocket['radius'], dtype=np.float32)
    M, n_pockets = len(px), len(pocket['ptr']) - 1
    out = dict(fail=np.zeros((B, K), np.int64), report=np.zeros((B, K, len(REPORT))), counts=np.zeros((B, K, len(COUNTS)), np.int64),
               atom_fail=np.zeros((K, N), np.int64), status=np.zeros((B, K), np.int64))
    for b in range(B):
        a0, a1 = int(ptr[b]), int(ptr[b + 1])
        n = a1 - a0
        if not (0 <= a0 <= a1 <= N) or n <= 0 or n > MOL_MAX or n > max_atoms or int(mol['status'][b]) & (1 | 2 | 8):
            out['status'][b, :] = NO_MOLECULE
            continue
        p0, p1 = int(mol['bond_ptr'][b]), int(mol['bond_ptr'][b + 1])
        if not (0 <= p0 <= p1 <= cap and p1 - p0 <= 3 * MOL_MAX):
            out['status'][b, :] = NO_MOLECULE
            continue
        po = int(pocket['of'][b])
        if po < -1 or po >= n_pockets:
            out['status'][b, :] = BAD_INPUT
            continue
        q0 = q1 = 0
        if po >= 0:
            q0, q1 = int(pocket['ptr'][po]), int(pocket['ptr'][po + 1])
            if not 0 <= q0 <= q1 <= M:
                out['status'][b, :] = BAD_INPUT
                continue
        g = None
        if not int(san['status'][b]) & 1:
            g = _graph(n, a0, mol['elem'], mol['frag'], z, F, bonds, san['order_k'], san['bond_flags'], p0, p1, san['atom_h'],
                       san['atom_flags'], largest)
        if g is None:
            out['status'][b, :] = NO_MOLECULE
            continue
        S, nbrs, zv, arom_atom = g
        R32 = [lig_radius[int(mol['elem'][a0 + a])] for a in range(n)]
        lig_bad = any(not (math.isfinite(float(r)) and float(r) <= MAX_RADIUS) for r in R32)
        pk_bad = any(not (all(_f32_ok_coord(c) for c in px[j]) and math.isfinite(float(pr[j])) and float(pr[j]) <= MAX_RADIUS)
                     for j in range(q0, q1))
        pk = [(tuple(float(c) for c in px[j]), float(pr[j])) for j in range(q0, q1) if float(pr[j]) > 0.0] if not pk_bad else []
        R = [float(r) for r in R32]
        for k in range(K):
            rows = pos[k, a0:a1]
            if lig_bad or pk_bad or not all(_f32_ok_coord(c) for c in rows.reshape(-1)):
                out['status'][b, k] = BAD_INPUT
                continue
            P = [tuple(float(c) for c in r) for r in rows]
            fail, rep, cnt, af = check_pose(S, nbrs, zv, arom_atom, P, R, pk, po >= 0, prm, margins, lattice)
            st = ATOM_OUT if any(not R[a] > 0.0 for a in S) or (po >= 0 and len(pk) < q1 - q0) else 0
            out['fail'][b, k], out['status'][b, k] = fail, st
            out['report'][b, k], out['counts'][b, k] = rep, cnt
            for a, bits in af.items():
                out['atom_fail'][k, a0 + a] = bits
    return out
