"""Integer and float64 restatement of the sanitisation rule of include/kpd.h (kpd_mol_sanitize), the yardstick of
test_sanitize_config.py and test_sanitize_gpu.py.  Same arithmetic as the kernel: differences of the fp32 coordinates in
float64, every product and sum rounded once, so every comparison against the GPU is exact equality.
The Kekule matching is here twice: `matching_exhaustive` walks every matching of the candidate graph and keeps the best (the
definition), `matching_fast` is the algorithm of the kernel (a greedy pass over the atoms with an exhaustive search for
alternating paths, then the lexicographic choice bond by bond).  The cycles are here twice as well: `cycles56` by start atom,
as the kernel walks them, and `cycles56_brute`, which walks every simple path and sorts out the repeats afterwards."""
import numpy as np

from .molecule_ref import BAD_SEGMENT, CAPACITY, EMPTY, MAX_ATOMS, TABLE

NO_MOLECULE, TOO_MANY_RINGS, COMPONENT_TOO_LARGE = 1, 2, 4
BOND_RING, BOND_PLANAR, BOND_AROMATIC = 1, 2, 4
ATOM_RING, ATOM_AROMATIC, ATOM_DONOR, ATOM_ACCEPTOR, ATOM_UNSATISFIED, ATOM_OVERVALENT = 1, 2, 4, 8, 16, 32
MAX_CYCLES, MAX_COMPONENT, MAX_DEG = 64, 24, 6
COS20 = 0.9396926207859084
DESC_I = ('n_heavy', 'n_h', 'hbd', 'hba', 'n_rot', 'n_rings', 'n_arom_rings', 'n_arom_atoms', 'lipinski4', 'n_cycles')
VN_H, VN_D, VN_A = 1, 2, 4


def normal_valence(z: int, val: int) -> int:
    if z in (6, 14):
        return 4
    if z in (7, 5, 33):
        return 3
    if z == 8:
        return 2
    if z in (1, 9, 17, 35, 53):
        return 1
    if z == 16:
        return 2 if val <= 2 else 4 if val <= 4 else 6
    if z == 15:
        return 3 if val <= 3 else 5
    return 0


# ---- cycles ------------------------------------------------------------------------------------------------------------
def cycles56(nbrs):
    """The simple cycles of length 5 and 6, each once: from its smallest atom, the second atom smaller than the last; sorted
    by start atom, then lexicographically.  nbrs: {atom: iterable of neighbours}."""
    out = []
    for s in sorted(nbrs):
        path = [s]

        def walk():
            cur = path[-1]
            for v in nbrs[cur]:
                if v <= s or v in path:
                    continue
                path.append(v)
                if len(path) >= 5 and s in nbrs[v] and path[1] < v:
                    out.append(tuple(path))
                if len(path) < 6:
                    walk()
                path.pop()
        walk()
    return sorted(out)


def cycles56_brute(nbrs):
    """The same set by brute force: every simple path of 5 or 6 atoms from every atom, closed, canonicalised, repeats dropped."""
    seen = set()
    for s in nbrs:
        stack = [(s,)]
        while stack:
            path = stack.pop()
            if len(path) in (5, 6) and path[0] in nbrs[path[-1]]:
                k = path.index(min(path))
                rot = path[k:] + path[:k]
                if rot[1] > rot[-1]:
                    rot = (rot[0],) + rot[:0:-1]
                seen.add(rot)
            if len(path) < 6:
                stack.extend(path + (v,) for v in nbrs[path[-1]] if v not in path)
    return sorted(seen)


# ---- planarity ----------------------------------------------------------------------------------------------------------
def _cross(x, y):
    return np.array([x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]])


def _dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def planar(p64, cyc) -> bool:
    k = len(cyc)
    with np.errstate(invalid='ignore', over='ignore'):
        for t in range(k):
            a, b, c, d = (p64[cyc[(t + q) % k]] for q in range(4))
            n1, n2 = _cross(b - a, c - b), _cross(c - b, d - c)
            q = _dot(n1, n1) * _dot(n2, n2)
            if not (q >= 1e-12 and _dot(n1, n2) >= COS20 * np.sqrt(q)):
                return False
    return True


# ---- matching -------------------------------------------------------------------------------------------------------------
def matching_exhaustive(edges, carbon):
    """edges: [(row, u, v)]; carbon: {atom: bool} of the atoms of G.  The matching that maximises the matched carbons, then the
    matched atoms, then is the lexicographically smallest ascending list of rows -- found by walking every matching."""
    edges = sorted(edges)
    best = [None]

    def walk(k, used, rows, nc):
        if k == len(edges):
            key = (-nc, -2 * len(rows), tuple(rows))
            if best[0] is None or key < best[0]:
                best[0] = key
            return
        row, u, v = edges[k]
        if u not in used and v not in used:
            walk(k + 1, used | {u, v}, rows + [row], nc + carbon[u] + carbon[v])
        walk(k + 1, used, rows, nc)
    walk(0, frozenset(), [], 0)
    return list(best[0][2])


def _greedy_value(verts, adj, carbon):
    """(matched carbons, matched atoms) of an optimal matching of the graph on `verts`: atoms in order, carbons first; an atom
    is taken iff an alternating path from it ends at a free atom, or, after an even number of bonds, at a matched atom that
    was not taken yet (that one is given up).  The search walks every simple alternating path: exact with odd rings too."""
    verts = sorted(verts)
    vs = set(verts)
    mate, taken = {}, set()

    def search(v):
        xs, ys = [v], []
        visited = {v}
        tried = [set()]
        while True:
            x = xs[-1]
            cand = [y for y in sorted(adj[x]) if y in vs and y not in visited and y not in tried[-1]]
            if not cand:
                if len(xs) == 1:
                    return False
                visited.discard(x)
                visited.discard(mate[x])
                xs.pop()
                ys.pop()
                tried.pop()
                continue
            y = cand[0]
            tried[-1].add(y)
            m = mate.get(y)
            if m is not None and m in visited:
                continue
            if m is None or m not in taken:
                if m is not None:
                    del mate[m]
                ys.append(y)
                for xd, yd in zip(xs, ys):
                    mate[xd], mate[yd] = yd, xd
                return True
            visited.update((y, m))
            ys.append(y)
            xs.append(m)
            tried.append(set())

    for want in (True, False):
        for v in verts:
            if bool(carbon[v]) != want:
                continue
            if v in mate or search(v):
                taken.add(v)
    return sum(1 for v in taken if carbon[v]), len(taken), mate


def matching_fast(edges, carbon):
    """The same matching as `matching_exhaustive`, the way the kernel finds it."""
    edges = sorted(edges)
    verts = set(carbon)
    adj = {v: set() for v in verts}
    for _, u, v in edges:
        adj[u].add(v)
        adj[v].add(u)
    opt_c, opt_a, mate = _greedy_value(verts, adj, carbon)
    rows, nc, avail = [], 0, set(verts)
    for row, u, v in edges:                         # `mate` is always an optimal matching that holds the rows taken so far
        if u not in avail or v not in avail:
            continue
        rest = avail - {u, v}
        if mate.get(u) != v:                        # a bond of that matching needs no search
            c, a, found = _greedy_value(rest, adj, carbon)
            if (c + nc + carbon[u] + carbon[v], a + 2 * len(rows) + 2) != (opt_c, opt_a):
                continue
            mate = {x: y for x, y in mate.items() if x not in avail}
            mate.update(found)
            mate[u], mate[v] = v, u
        rows.append(row)
        nc += carbon[u] + carbon[v]
        avail = rest
    return rows


# ---- one ligand -----------------------------------------------------------------------------------------------------------
def sanitize(pos, elem, frag, bonds, order, z, allowed, mass, mass_h, largest_only=False, matching=matching_fast, cycles=cycles56):
    """One ligand with a molecule.  pos [n,3] float32; elem / frag [n]; bonds [m,2] local; order [m]; z / allowed / mass: F
    entries each.  Returns None for a graph kpd_mol_keys rejects, else a dict: order_k / bond_flags [m], valence_k / atom_h /
    atom_flags [n] (-1, 0, 0 outside S), desc_i (10 ints), mw, valid, status, and the working sets the tests look at."""
    pos = np.asarray(pos, dtype=np.float32).reshape(-1, 3)
    n, F = pos.shape[0], len(z)
    elem, frag = [int(e) for e in elem], [int(f) for f in frag]
    bonds = [(int(i), int(j)) for i, j in bonds]
    order = [int(o) for o in order]
    if n <= 0 or n > MAX_ATOMS or any(e < 0 or e >= F for e in elem) or any(f < 0 or f >= n for f in frag):
        return None
    if largest_only:
        sizes = np.bincount(frag, minlength=n)
        rank = int(np.argmax(sizes))
        inS = [f == rank for f in frag]
    else:
        inS = [True] * n
    if any(i < 0 or i >= n or j < 0 or j >= n or i == j or o < 1 or o > 3 for (i, j), o in zip(bonds, order)):
        return None
    nb = {a: {} for a in range(n) if inS[a]}            # atom -> {neighbour: row}
    for row, (i, j) in enumerate(bonds):
        if not (inS[i] and inS[j]):
            continue
        if j in nb[i] or len(nb[i]) >= MAX_DEG or len(nb[j]) >= MAX_DEG:
            return None
        nb[i][j] = nb[j][i] = row
    S = sorted(nb)
    Z = [int(z[e]) for e in elem]
    m = sum(len(v) for v in nb.values()) // 2
    status = 0
    # step 1: ring bonds, ring count, cycles
    def connected_without(i, j):
        seen, todo = {i}, [i]
        while todo:
            u = todo.pop()
            for v in nb[u]:
                if (u == i and v == j) or v in seen:
                    continue
                seen.add(v)
                todo.append(v)
        return j in seen
    ring_rows = {row for i in S for j, row in nb[i].items() if i < j and connected_without(i, j)}
    n_rings = m - len(S) + len({frag[a] for a in S})
    cyc = cycles({a: sorted(nb[a]) for a in S})
    if len(cyc) > MAX_CYCLES:
        status |= TOO_MANY_RINGS
    # step 2: planar rings
    p64 = pos.astype(np.float64)
    planar_cyc = [c for c in cyc if planar(p64, c)] if not status else []
    planar_rows = {nb[c[t]][c[(t + 1) % len(c)]] for c in planar_cyc for t in range(len(c))}
    planar_atoms = {a for c in planar_cyc for a in c}
    # step 3: the candidate graph and its matching
    def d2(i, j):
        d = p64[i] - p64[j]
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    inG = set()
    for a in planar_atoms:
        if Z[a] not in (6, 7):
            continue
        n_pl = sum(1 for row in nb[a].values() if row in planar_rows)
        other = sum(order[row] for row in nb[a].values() if row not in planar_rows)
        if TABLE[Z[a]][3] - n_pl - other >= 1:
            inG.add(a)
    g_edges = []
    for row in sorted(planar_rows):
        i, j = bonds[row]
        T = TABLE[Z[i]][0] + TABLE[Z[j]][0] - 3 if i in inG and j in inG else None
        with np.errstate(invalid='ignore'):
            if T is not None and d2(i, j) <= float(T * T) * 1e-4:
                g_edges.append((row, i, j))
    label = {a: a for a in inG}
    changed = True
    while changed:
        changed = False
        for _, i, j in g_edges:
            lo = min(label[i], label[j])
            if label[i] != lo or label[j] != lo:
                label[i] = label[j] = lo
                changed = True
    comps = {}
    for a in inG:
        comps.setdefault(label[a], []).append(a)
    matched_rows, too_large, unsatisfied = set(), set(), set()
    for root, atoms in comps.items():
        edges = [e for e in g_edges if label[e[1]] == root]
        if not edges:
            continue
        if len(atoms) > MAX_COMPONENT:
            status |= COMPONENT_TOO_LARGE
            too_large.update(atoms)
            unsatisfied.update(a for a in atoms if Z[a] == 6)
            continue
        rows = matching(edges, {a: Z[a] == 6 for a in atoms})
        matched_rows.update(rows)
        covered = {v for row in rows for v in bonds[row]}
        unsatisfied.update(a for a in atoms if Z[a] == 6 and a not in covered)
    matched_atoms = {v for row in matched_rows for v in bonds[row]}
    order_k = list(order)
    for row in planar_rows:
        i, j = bonds[row]
        if i in too_large or j in too_large:
            continue
        order_k[row] = 2 if row in matched_rows else 1
    # step 5 first: step 4 reads the valences
    deg = {a: len(nb[a]) for a in S}
    val = {a: sum(order_k[row] for row in nb[a].values()) for a in S}
    lone_pair = {a for a in planar_atoms if a not in matched_atoms and Z[a] == 7 and deg[a] in (2, 3) and val[a] == deg[a]}
    # step 4: aromatic rings
    def contribution(a):
        if a in matched_atoms:
            return 1
        if Z[a] in (8, 16) and deg[a] == 2:
            return 2
        if a in lone_pair:
            return 2
        if Z[a] == 6 and any(order_k[row] == 2 and row not in planar_rows and Z[j] in (7, 8, 16) for j, row in nb[a].items()):
            return 0
        return None
    arom_cyc = []
    for c in planar_cyc:
        e = [contribution(a) for a in c]
        if None not in e and sum(e) == 6:
            arom_cyc.append(c)
    arom_rows = {nb[c[t]][c[(t + 1) % len(c)]] for c in arom_cyc for t in range(len(c))}
    arom_atoms = {a for c in arom_cyc for a in c}
    ring_atoms = {v for row in ring_rows for v in bonds[row]}
    # steps 5 and 6
    valence_k, atom_h, atom_flags = [-1] * n, [0] * n, [0] * n
    for a in S:
        h = max(0, normal_valence(Z[a], val[a]) - val[a])
        donor = Z[a] in (7, 8) and h >= 1
        acceptor = Z[a] == 8 or (Z[a] == 7 and not donor and deg[a] <= 2 and a not in lone_pair)
        valence_k[a], atom_h[a] = val[a], h
        atom_flags[a] = (ATOM_RING * (a in ring_atoms) | ATOM_AROMATIC * (a in arom_atoms) | ATOM_DONOR * donor | ATOM_ACCEPTOR * acceptor |
                         ATOM_UNSATISFIED * (a in unsatisfied) | ATOM_OVERVALENT * (val[a] > int(allowed[elem[a]])))
    bond_flags = [0] * len(bonds)
    for a in S:
        for row in nb[a].values():
            bond_flags[row] = BOND_RING * (row in ring_rows) | BOND_PLANAR * (row in planar_rows) | BOND_AROMATIC * (row in arom_rows)
    # steps 7 and 8
    valid = int(not status and not any(atom_flags[a] & (ATOM_UNSATISFIED | ATOM_OVERVALENT) for a in S))
    n_h = sum(atom_h)
    mw = 0.0
    for c in range(F):
        mw = mw + float(sum(1 for a in S if elem[a] == c)) * float(mass[c])
    mw = mw + float(n_h) * float(mass_h)
    hdeg = {a: sum(1 for j in nb[a] if Z[j] != 1) for a in S}
    n_rot = sum(1 for a in S for j, row in nb[a].items() if a < j and order_k[row] == 1 and row not in ring_rows and hdeg[a] >= 2 and hdeg[j] >= 2)
    hbd = sum(1 for a in S if atom_flags[a] & ATOM_DONOR)
    hba = sum(1 for a in S if atom_flags[a] & ATOM_ACCEPTOR)
    lip = int(mw < 500.0) + int(hbd <= 5) + int(hba <= 10) + int(n_rot <= 10)
    desc_i = [sum(1 for a in S if Z[a] != 1), n_h, hbd, hba, n_rot, n_rings, len(arom_cyc), len(arom_atoms), lip, len(cyc)]
    return dict(order_k=order_k, bond_flags=bond_flags, valence_k=valence_k, atom_h=atom_h, atom_flags=atom_flags, desc_i=desc_i, mw=mw,
                valid=valid, status=status, cycles=cyc, planar_cycles=planar_cyc, aromatic_cycles=arom_cyc, g_edges=g_edges, g_atoms=inG,
                matched_rows=sorted(matched_rows), aromatic_atoms=arom_atoms, aromatic_rows=arom_rows, components=comps)


def vina_types(z_atoms, atom_h, atom_flags, valence_k):
    """The flags of kpd_vina_score from hydrogen counts, per atom: what `Sanitized.vina_types` computes.  -1 (outside S, and
    every element but N and O) keeps the rule of kpd_vina_score."""
    out = []
    for zz, h, fl, v in zip(z_atoms, atom_h, atom_flags, valence_k):
        if v < 0:
            out.append(-1)
        elif zz == 7:
            out.append(VN_D if h >= 1 else VN_A if fl & ATOM_ACCEPTOR else 0)
        elif zz == 8:
            out.append(VN_A | (VN_D if h >= 1 else 0))
        else:
            out.append(-1)
    return out


# ---- a batch, in the layout of kpd_mol_sanitize ---------------------------------------------------------------------------------
def sanitize_batch(pos, ptr, mol, z, allowed, mass, mass_h, largest_only=False, cap_bonds=None):
    """The outputs of kpd_mol_sanitize for a batch.  `mol`: elem / frag [N], bonds [cap,2] (global rows), order [cap], bond_ptr
    [B+1], status [B] as integer arrays (what perceive_batch returns, or hand-written).  Returns order_k / bond_flags [cap] (0
    where nothing is written), valence_k / atom_h / atom_flags [N], desc_i [B,10], desc_f [B,2], valid / status [B], and
    `mols`: the per-ligand dicts (None where there is no molecule)."""
    pos = np.asarray(pos, dtype=np.float32).reshape(-1, 3)
    N, B = pos.shape[0], len(ptr) - 1
    cap = len(mol['order']) if cap_bonds is None else cap_bonds
    out = dict(order_k=np.zeros(cap, dtype=np.int64), bond_flags=np.zeros(cap, dtype=np.int64), valence_k=np.full(N, -1, dtype=np.int64),
               atom_h=np.zeros(N, dtype=np.int64), atom_flags=np.zeros(N, dtype=np.int64), desc_i=np.zeros((B, 10), dtype=np.int64),
               desc_f=np.zeros((B, 2), dtype=np.float64), valid=np.zeros(B, dtype=np.int64), status=np.zeros(B, dtype=np.int64), mols=[])
    for b in range(B):
        a0, a1 = int(ptr[b]), int(ptr[b + 1])
        res = None
        seg = 0 <= a0 <= a1 <= N
        ok = seg and 0 < a1 - a0 <= MAX_ATOMS and not (int(mol['status'][b]) & (EMPTY | CAPACITY | BAD_SEGMENT))
        p0, p1 = int(mol['bond_ptr'][b]), int(mol['bond_ptr'][b + 1])
        rng = p0 >= 0 and p1 >= p0 and p1 <= cap and p1 - p0 <= 3 * MAX_ATOMS
        if ok and rng:
            res = sanitize(pos[a0:a1], mol['elem'][a0:a1], mol['frag'][a0:a1], np.asarray(mol['bonds'][p0:p1]) - a0, mol['order'][p0:p1], z,
                           allowed, mass, mass_h, largest_only)
        out['mols'].append(res)
        if res is None:
            out['status'][b] = NO_MOLECULE
            if rng:                                                  # the rows keep the orders they came with
                out['order_k'][p0:p1] = mol['order'][p0:p1]
            continue
        out['order_k'][p0:p1], out['bond_flags'][p0:p1] = res['order_k'], res['bond_flags']
        for k in ('valence_k', 'atom_h', 'atom_flags'):
            out[k][a0:a1] = res[k]
        out['desc_i'][b], out['desc_f'][b, 0] = res['desc_i'], res['mw']
        out['valid'][b], out['status'][b] = res['valid'], res['status']
    return out
