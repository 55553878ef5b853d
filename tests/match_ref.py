"""Plain-Python restatement of kpd_mol_match as include/kpd.h defines it: the labels, the predicate, the search with its order and
its node count, both modes, the anchor bits that "$(...)" rows read, and the typing epilogue with one fp64 addition at a time.
Next to it a second, independent brute force: every injective map of the query's atoms into S is tested against the definition
of an embedding; no search order is involved, and it reads the labels off the arrays and evaluates the predicate with code of its
own (only the decoding of the table is shared).  This restates the header, not RDKit."""
import itertools

import numpy as np

Q_ATOMS, Q_BONDS, Q_ALT, Q_PATTERNS, Q_TOP, Q_MAGIC = 16, 24, 8, 512, 15, 0x4b505101
Q_HEAD, Q_ROW_HEAD, Q_ATOM_WORDS, Q_CLOSE_WORDS, Q_ALT_WORDS = 4, 4, 4, 4, 16
ANCHORS, ALL = 0, 1
NO_MOLECULE, MAX_NODES = 1, 2
MAX_ATOMS, MAX_DEG, MAX_H = 256, 6, 9
DEFAULT_MAX_NODES = 65536


# ---- the table ------------------------------------------------------------------------------------------------------------------
def decode(words):
    """The rows of a well-formed table: dicts na, parent, pmask, alts (per atom a list of dicts), closures [(s, t, mask)]."""
    w = [int(x) for x in words]
    assert w[0] == Q_MAGIC and w[2] == len(w)
    rows = []
    for p in range(w[1]):
        o = w[Q_HEAD + p]
        na, nc, nalt = w[o], w[o + 1], w[o + 2]
        qa = o + Q_ROW_HEAD
        qc = qa + Q_ATOM_WORDS * na
        ql = qc + Q_CLOSE_WORDS * nc
        alts = []
        for k in range(nalt):
            r = w[ql + Q_ALT_WORDS * k:ql + Q_ALT_WORDS * (k + 1)]
            alts.append(dict(z=sum((r[i] & 0xffffffff) << (32 * i) for i in range(4)), cls=r[4], D=r[5], H=r[6], X=r[7], v=r[8], x=r[9],
                             need=[x for x in r[10:12] if x >= 0], forbid=[x for x in r[12:14] if x >= 0]))
        atoms = [w[qa + Q_ATOM_WORDS * t:qa + Q_ATOM_WORDS * (t + 1)] for t in range(na)]
        rows.append(dict(na=na, parent=[a[0] for a in atoms], pmask=[a[1] for a in atoms], alts=[alts[a[2]:a[2] + a[3]] for a in atoms],
                         closures=[tuple(w[qc + Q_CLOSE_WORDS * c:qc + Q_CLOSE_WORDS * c + 3]) for c in range(nc)]))
    return rows


# ---- one ligand: the scope, the graph and the labels ------------------------------------------------------------------------------
def graph_of(ptr, mol, san, z, b, largest_only=False):
    """None where kpd_mol_match has no molecule, else dict(a0, n, S, nbrs {a: [(v, bond bit)] ascending}, lab {a: dict})."""
    N, F = len(mol['elem']), len(z)
    cap = len(mol['order']) if 'order' in mol else len(san['order_k'])
    a0, a1 = int(ptr[b]), int(ptr[b + 1])
    if not (0 <= a0 <= a1 <= N) or not (0 < a1 - a0 <= MAX_ATOMS) or int(mol['status'][b]) & (1 | 2 | 8):
        return None
    p0, p1 = int(mol['bond_ptr'][b]), int(mol['bond_ptr'][b + 1])
    if not (p0 >= 0 and p1 >= p0 and p1 <= cap and p1 - p0 <= 3 * MAX_ATOMS) or int(san['status'][b]) & 1:
        return None
    n = a1 - a0
    elem, frag = [int(e) for e in mol['elem'][a0:a1]], [int(f) for f in mol['frag'][a0:a1]]
    if any(e < 0 or e >= F for e in elem) or any(f < 0 or f >= n for f in frag):
        return None
    if largest_only:
        sizes = np.bincount(frag, minlength=n)
        rank = int(np.argmax(sizes))                  # most atoms, the lowest label on a tie
        S = [a for a in range(n) if frag[a] == rank]
    else:
        S = list(range(n))
    inS = set(S)
    nbrs = {a: {} for a in S}
    for r in range(p0, p1):
        i, j, o = int(mol['bonds'][r][0]) - a0, int(mol['bonds'][r][1]) - a0, int(san['order_k'][r])
        if not (0 <= i < n and 0 <= j < n and i != j and 1 <= o <= 3):
            return None
        if i not in inS or j not in inS:
            continue
        if j in nbrs[i] or len(nbrs[i]) >= MAX_DEG or len(nbrs[j]) >= MAX_DEG:
            return None
        fl = int(san['bond_flags'][r])
        nbrs[i][j] = nbrs[j][i] = (3 if fl & 4 else o - 1) + 4 * (fl & 1)
    if not S:
        return None
    Z = [int(z[e]) if 0 <= int(z[e]) <= 255 else 0 for e in elem]
    lab = {}
    for a in S:
        h, val, fl = int(san['atom_h'][a0 + a]), int(san['valence_k'][a0 + a]), int(san['atom_flags'][a0 + a])
        if h < 0 or h > MAX_H or val < 0:
            return None
        deg, heavy = len(nbrs[a]), sum(Z[v] != 1 for v in nbrs[a])
        lab[a] = dict(z=Z[a] if Z[a] < 128 else 0, aromatic=(fl >> 1) & 1, ring=fl & 1, D=min(heavy, Q_TOP), H=min(h + deg - heavy, Q_TOP),
                      X=min(deg + h, Q_TOP), v=min(val + h, Q_TOP), x=min(sum(bit >> 2 for bit in nbrs[a].values()), Q_TOP))
    return dict(a0=a0, n=n, S=S, nbrs={a: sorted(nbrs[a].items()) for a in S}, lab=lab)


def alt_holds(alt, lab, bits):
    """`bits`: the rows whose anchor bit the atom has."""
    if not (alt['z'] >> lab['z']) & (alt['cls'] >> lab['aromatic']) & (alt['cls'] >> (2 + lab['ring'])) & 1:
        return False
    if not all((alt[f] >> lab[f]) & 1 for f in 'DHXvx'):
        return False
    return all(r in bits for r in alt['need']) and not any(r in bits for r in alt['forbid'])


def pred(row, t, g, v, anc):
    return any(alt_holds(alt, g['lab'][v], anc[v]) for alt in row['alts'][t])


def bond_bit(g, u, v):
    return dict(g['nbrs'][u]).get(v)


# ---- the search of the header ------------------------------------------------------------------------------------------------------
def search(row, g, a, anc, mode, max_nodes):
    """The embeddings (tuples f(0) .. f(na-1), local atoms) the search from anchor a finds, in the order it finds them, and whether
    it stopped at max_nodes."""
    if not pred(row, 0, g, a, anc):
        return [], False
    na, found, f = row['na'], [], [a]
    if na == 1:
        return [(a,)], False
    nodes = [0]

    class Stop(Exception):
        pass

    def descend(t):
        for v, bit in g['nbrs'][f[row['parent'][t]]]:
            if v in f or not (row['pmask'][t] >> bit) & 1 or not pred(row, t, g, v, anc):
                continue
            if not all(bond_bit(g, v, f[s]) is not None and (m >> bond_bit(g, v, f[s])) & 1 for s, tt, m in row['closures'] if tt == t):
                continue
            nodes[0] += 1
            if nodes[0] > max_nodes:
                raise Stop
            f.append(v)
            if t == na - 1:
                found.append(tuple(f))
                if mode == ANCHORS:
                    raise Stop
            else:
                descend(t + 1)
            f.pop()

    try:
        descend(1)
    except Stop:
        return found, nodes[0] > max_nodes
    return found, False


# ---- the brute force: its own reading of the arrays, its own predicate, no search -------------------------------------------------
def _bits(mask, width):
    return {k for k in range(width) if (mask >> k) & 1}


def brute_force(rows, ptr, mol, san, z, b):
    """Per row the set of ALL embeddings of ligand b (every atom in scope; the ligand must have a molecule), by testing every
    injective map against the definition of include/kpd.h.  Nothing is shared with the search above but the decoded table: the
    labels are read off the batch arrays bond row by bond row, the sets of an alternative are Python sets, and there is no order."""
    a0, a1 = int(ptr[b]), int(ptr[b + 1])
    atoms = list(range(a0, a1))
    bond = {}                                       # (i, j) global, both ways -> (kind, in a ring)
    for r in range(int(mol['bond_ptr'][b]), int(mol['bond_ptr'][b + 1])):
        i, j = int(mol['bonds'][r][0]), int(mol['bonds'][r][1])
        flags = int(san['bond_flags'][r])
        bond[i, j] = bond[j, i] = ('aromatic' if flags & 4 else int(san['order_k'][r]), bool(flags & 1))
    number = {a: int(z[int(mol['elem'][a])]) for a in atoms}
    label = {}
    for a in atoms:
        partners = [j for (i, j) in bond if i == a]
        hydrogens = [j for j in partners if number[j] == 1]
        h, flags = int(san['atom_h'][a]), int(san['atom_flags'][a])
        label[a] = dict(z=number[a] if 0 <= number[a] <= 127 else 0, aromatic=bool(flags & 2), ring=bool(flags & 1),
                        D=min(15, len(partners) - len(hydrogens)), H=min(15, h + len(hydrogens)), X=min(15, len(partners) + h),
                        v=min(15, int(san['valence_k'][a]) + h), x=min(15, sum(1 for j in partners if bond[a, j][1])))

    def holds(alt, a, anchors):
        lab = label[a]
        allowed = _bits(alt['cls'], 4)
        if lab['z'] not in _bits(alt['z'], 128) or (1 if lab['aromatic'] else 0) not in allowed or (3 if lab['ring'] else 2) not in allowed:
            return False
        if any(lab[f] not in _bits(alt[f], 16) for f in ('D', 'H', 'X', 'v', 'x')):
            return False
        return all(a in anchors[r] for r in alt['need']) and all(a not in anchors[r] for r in alt['forbid'])

    def in_mask(mask, i, j):
        if (i, j) not in bond:
            return False
        kind, ring = bond[i, j]
        return ({1: 0, 2: 1, 3: 2, 'aromatic': 3}[kind] + (4 if ring else 0)) in _bits(mask, 8)

    anchors, out = [], []
    for row in rows:
        fits = [[a for a in atoms if any(holds(alt, a, anchors) for alt in row['alts'][t])] for t in range(row['na'])]
        query_bonds = [(row['parent'][t], t, row['pmask'][t]) for t in range(1, row['na'])] + list(row['closures'])
        embeds = {tuple(a - a0 for a in f) for f in itertools.product(*fits)
                  if len(set(f)) == len(f) and all(in_mask(m, f[s], f[t]) for s, t, m in query_bonds)}
        anchors.append({a0 + f[0] for f in embeds})
        out.append(embeds)
    return out


def match_ligand(rows, g, mode=ANCHORS, max_nodes=DEFAULT_MAX_NODES):
    """Per row: dict(anchors [local atoms], first (the first embedding from the lowest anchor with one, or None), n_embed, cover
    (set of local atoms), embeddings (list, in search order)); and whether any search stopped at max_nodes."""
    anc = {a: set() for a in g['S']}
    out, capped = [], False
    for p, row in enumerate(rows):
        res = dict(anchors=[], first=None, n_embed=0, cover=set(), embeddings=[])
        for a in g['S']:
            found, stopped = search(row, g, a, anc, mode, max_nodes)
            capped = capped or stopped
            if found:
                res['anchors'].append(a)
                if res['first'] is None:
                    res['first'] = found[0]
                if mode == ALL:
                    res['n_embed'] += len(found)
                    res['embeddings'] += found
                    for f in found:
                        res['cover'].update(f)
        for a in res['anchors']:                    # complete before the next row reads them
            anc[a].add(p)
        out.append(res)
    return out, capped


# ---- a batch, in the layout of kpd_mol_match -------------------------------------------------------------------------------------
def match_batch(ptr, mol, san, z, table, mode=ANCHORS, max_nodes=DEFAULT_MAX_NODES, type_group=None, value=None, G=0, largest_only=False):
    rows = decode(table)
    P, N, B = len(rows), len(mol['elem']), len(ptr) - 1
    W = (P + 31) // 32
    out = dict(anchor=np.zeros((N, W), dtype=np.uint32), hits=np.zeros((B, P), dtype=np.int64), first_map=np.full((B, P, Q_ATOMS), -1, dtype=np.int64),
               n_embed=np.zeros((B, P), dtype=np.int64), cover=np.zeros((N, W), dtype=np.uint32), status=np.zeros(B, dtype=np.int64),
               atom_type=np.full((G, N), -1, dtype=np.int64), type_sum=np.zeros((B, G), dtype=np.float64), untyped=np.zeros((B, G), dtype=np.int64),
               ligands=[], graphs=[])
    for b in range(B):
        g = graph_of(ptr, mol, san, z, b, largest_only)
        out['graphs'].append(g)
        if g is None:
            out['status'][b] = NO_MOLECULE
            out['ligands'].append(None)
            continue
        res, capped = match_ligand(rows, g, mode, max_nodes)
        out['ligands'].append(res)
        out['status'][b] = MAX_NODES if capped else 0
        a0 = g['a0']
        for p, r in enumerate(res):
            out['hits'][b, p] = len(r['anchors'])
            for a in r['anchors']:
                out['anchor'][a0 + a, p >> 5] |= np.uint32(1 << (p & 31))
            if r['first'] is not None:
                out['first_map'][b, p, :len(r['first'])] = [a0 + a for a in r['first']]
            if mode == ALL:
                out['n_embed'][b, p] = r['n_embed']
                for a in r['cover']:
                    out['cover'][a0 + a, p >> 5] |= np.uint32(1 << (p & 31))
    out.update(typing(out, type_group, value, G))
    return out


def typing(out, type_group, value, G):
    """The typing epilogue on the anchors of a finished match_batch: atom_type [G, N], type_sum [B, G], untyped [B, G]."""
    N, B = out['anchor'].shape[0], len(out['graphs'])
    res = dict(atom_type=np.full((G, N), -1, dtype=np.int64), type_sum=np.zeros((B, G), dtype=np.float64), untyped=np.zeros((B, G), dtype=np.int64))
    for b, g in enumerate(out['graphs']):
        if g is None:
            continue
        anchors = [set(r['anchors']) for r in out['ligands'][b]]
        for gi in range(G):
            rows = [p for p in range(len(anchors)) if p < len(type_group) and int(type_group[p]) == gi]
            s, none = 0.0, 0
            for a in g['S']:
                t = next((p for p in rows if a in anchors[p]), -1)
                res['atom_type'][gi, g['a0'] + a] = t
                if t < 0:
                    none += 1
                else:
                    s = s + float(value[t])             # one rounded fp64 addition at a time, in ascending atom index
            res['type_sum'][b, gi], res['untyped'][b, gi] = s, none
    return res
