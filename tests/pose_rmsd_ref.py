"""Plain Python restatement of the symmetry-corrected RMSD of include/kpd.h (kpd_pose_rmsd), the yardstick of
tests/test_pose_rmsd_gpu.py, and an independent brute force that the restatement itself is held against
(tests/test_pose_rmsd_config.py).  Written from the header comment alone: the classes in Python integers reduced modulo 2^64, the
costs in Python floats (IEEE fp64, every operation rounded once), one ligand and one search at a time.  Not imported by the
package."""
import itertools
import math

import numpy as np

from .molset_ref import K1, K2, K3, MAX_ATOMS, MOL_CAPACITY, MOL_EMPTY, MOL_LEFT_OUT, distances, mix, step

NO_MOLECULE, HIT_MAX_NODES, NONFINITE = 1, 2, 4
MAX_DEG = 6
MAX_ATOM_LABEL, MAX_BOND_LABEL, MAX_PAIR_POSES = 2 ** 20 - 1, 15, 64
DEFAULT_MAX_NODES = 65536


def d2(x, y):
    """fp64 squared distance of two fp32 rows: the differences, then (dx^2 + dy^2) + dz^2, every product and sum rounded once."""
    dx, dy, dz = float(x[0]) - float(y[0]), float(x[1]) - float(y[1]), float(x[2]) - float(y[2])
    return (dx * dx + dy * dy) + dz * dz


class Graph:
    """The labelled graph in the scope S: A [n], nbrs[a] = [(b, L)] in ascending b (bonds with both ends in S only), S ascending,
    c [n] (the class, None outside S), order = u_0 .. and parent[u] (None for a start atom)."""

    def __init__(self, Z, bonds, bond_label=None, atom_label=None, S=None):
        n = len(Z)
        self.n = n
        self.S = sorted(range(n) if S is None else S)
        inside = set(self.S)
        atom_label = [0] * n if atom_label is None else atom_label
        bond_label = [1] * len(bonds) if bond_label is None else bond_label
        self.A = [int(Z[a]) + 256 * int(atom_label[a]) for a in range(n)]
        self.nbrs = [[] for _ in range(n)]
        for (i, j), l in zip(bonds, bond_label):
            if i in inside and j in inside:
                self.nbrs[i].append((j, int(l)))
                self.nbrs[j].append((i, int(l)))
        for row in self.nbrs:
            row.sort()
        self.label = {(a, b): l for a in self.S for b, l in self.nbrs[a]}
        # the class: inv_n of kpd_mol_keys with Z replaced by A and l by L
        inv = {}
        for a in self.S:
            d = distances(n, self.nbrs, a)
            inv[a] = mix(self.A[a] + len(self.nbrs[a]) * K3 + K1 * sum(mix(self.A[b] * K2 + d[b]) for b in self.S if b != a))
        for _ in range(len(self.S)):
            inv = step(inv, self.nbrs, self.S)
        self.c = [inv.get(a) for a in range(n)]
        # the source order: breadth-first from the lowest atom not yet listed, neighbours in ascending index
        self.order, self.parent = [], {}
        listed = set()
        for s in self.S:
            if s in listed:
                continue
            listed.add(s)
            self.parent[s] = None
            self.order.append(s)
            head = len(self.order) - 1
            while head < len(self.order):
                u = self.order[head]
                head += 1
                for w, _ in self.nbrs[u]:
                    if w not in listed:
                        listed.add(w)
                        self.parent[w] = u
                        self.order.append(w)
        self.place = {u: t for t, u in enumerate(self.order)}


class _Stop(Exception):
    pass


def search(g, X, Y, max_nodes=DEFAULT_MAX_NODES):
    """One search of the rule: dict(best, s_id, map {u: image}, nodes, hit)."""
    n = len(g.order)
    s_id = 0.0
    for u in g.order:
        s_id = s_id + d2(X[u], Y[u])
    state = dict(best=s_id, map={u: u for u in g.order}, nodes=0, hit=False)
    image, taken = {}, set()

    def descend(t, s_t):
        u = g.order[t]
        p = g.parent[u]
        pool = [v for v, _ in g.nbrs[image[p]]] if p is not None else g.S
        cands = []
        for v in pool:
            if v in taken or g.A[v] != g.A[u] or len(g.nbrs[v]) != len(g.nbrs[u]) or g.c[v] != g.c[u]:
                continue
            if all(g.label.get((v, image[w])) == l for w, l in g.nbrs[u] if g.place[w] < t):
                cands.append((d2(X[u], Y[v]), v))
        for d, v in sorted(cands):
            state['nodes'] += 1
            if state['nodes'] > max_nodes:
                state['hit'] = True
                raise _Stop
            s = s_t + d
            if s >= state['best']:
                return
            if t == n - 1:
                state['best'] = s
                state['map'] = {**image, u: v}
            else:
                image[u] = v
                taken.add(v)
                descend(t + 1, s)
                taken.discard(v)
                del image[u]

    try:
        descend(0, 0.0)
    except _Stop:
        pass
    return state | dict(s_id=s_id)


def automorphisms(g):
    """Every automorphism of the labelled graph as a dict, by plain means: for at most 8 atoms every permutation of S is tested
    against the definition; above that, backtracking on adjacency over the atoms of S in ascending index -- an image must carry
    the same A and every bond to an atom placed before must land on a bond of the same label.  No classes, no degrees, no bound,
    no source order.  (A bijection that maps every bond onto a bond of its label is onto the bonds: both sets are equally large.)"""
    S = g.S
    bonds = [(a, b, l) for a in S for b, l in g.nbrs[a] if a < b]
    if len(S) <= 8:
        out = []
        for perm in itertools.permutations(S):
            pi = dict(zip(S, perm))
            if all(g.A[pi[a]] == g.A[a] for a in S) and all(g.label.get((pi[a], pi[b])) == l for a, b, l in bonds):
                out.append(pi)
        return out
    out, pi, used = [], {}, set()

    def place(k):
        if k == len(S):
            out.append(dict(pi))
            return
        u = S[k]
        for v in S:
            if v in used or g.A[v] != g.A[u]:
                continue
            if any(w in pi and g.label.get((v, pi[w])) != l for w, l in g.nbrs[u]):
                continue
            if any(w in pi and (u, w) not in g.label and (v, pi[w]) in g.label for w in pi):      # a non-bond stays a non-bond
                continue
            pi[u] = v
            used.add(v)
            place(k + 1)
            used.discard(v)
            del pi[u]
    place(0)
    return out


def brute_best(g, X, Y, autos=None):
    """The minimum over every automorphism of the cost summed in source order."""
    best = None
    for pi in automorphisms(g) if autos is None else autos:
        s = 0.0
        for u in g.order:
            s = s + d2(X[u], Y[pi[u]])
        best = s if best is None or s < best else best
    return best


def rms(total, n):
    return math.sqrt(total / n)


def largest_fragment(frag):
    sizes = {}
    for f in frag:
        sizes[f] = sizes.get(f, 0) + 1
    best = max(sizes, key=lambda f: (sizes[f], -f))
    return [a for a, f in enumerate(frag) if f == best]


def ligand_graph(elem, frag, bonds, bond_label, atom_label, z, largest_only, skip_h):
    """One ligand, local rows: its Graph, or None under every no-molecule condition of kpd_pose_rmsd."""
    n, F = len(elem), len(z)
    if n <= 0 or n > MAX_ATOMS:
        return None
    if any(e < 0 or e >= F for e in elem) or any(f < 0 or f >= n for f in frag):
        return None
    if atom_label is not None and any(l < 0 or l > MAX_ATOM_LABEL for l in atom_label):
        return None
    if any(i < 0 or i >= n or j < 0 or j >= n or i == j for i, j in bonds):
        return None
    if bond_label is not None and any(l < 1 or l > MAX_BOND_LABEL for l in bond_label):
        return None
    Zs = [int(z[e]) for e in elem]
    S = largest_fragment(frag) if largest_only else list(range(n))
    if skip_h:
        S = [a for a in S if Zs[a] != 1]
    inside, seen, deg = set(S), set(), [0] * n
    for i, j in bonds:
        if i in inside and j in inside:
            if (min(i, j), max(i, j)) in seen or deg[i] >= MAX_DEG or deg[j] >= MAX_DEG:
                return None
            seen.add((min(i, j), max(i, j)))
            deg[i] += 1
            deg[j] += 1
    if not S:
        return None
    return Graph(Zs, bonds, bond_label, atom_label, S)


def pose_rmsd_batch(ptr, mol, z, pos, ref_pos=None, pairs=False, largest_only=False, skip_h=True, max_nodes=DEFAULT_MAX_NODES,
                    bond_label=None, atom_label=None):
    """The outputs of kpd_pose_rmsd for a batch.  `mol`: elem / frag [N], bonds [cap,2] (global rows), bond_ptr [B+1], status [B];
    pos [K,N,3] float32, ref_pos [N,3]; bond_label [cap] / atom_label [N] or None.  Returns dict(rmsd, plain, nodes [B,K] or
    [B,K,K], map [K,N] (pairs: None), status [B])."""
    pos = np.asarray(pos, dtype=np.float32)
    K, N = pos.shape[0], pos.shape[1]
    B, cap = len(ptr) - 1, len(mol['bonds'])
    shape = (B, K, K) if pairs else (B, K)
    rmsd, plain, nodes = np.zeros(shape), np.zeros(shape), np.zeros(shape, dtype=np.int64)
    amap = None if pairs else np.full((K, N), -1, dtype=np.int64)
    status = np.zeros(B, dtype=np.int64)
    for b in range(B):
        a0, a1 = int(ptr[b]), int(ptr[b + 1])
        p0, p1 = int(mol['bond_ptr'][b]), int(mol['bond_ptr'][b + 1])
        ok = (0 <= a0 <= a1 <= N and not int(mol['status'][b]) & (MOL_EMPTY | MOL_CAPACITY | MOL_LEFT_OUT) and 0 <= p0 <= p1 <= cap and
              p1 - p0 <= 3 * MAX_ATOMS)
        g = None
        if ok:
            rows = [(int(i) - a0, int(j) - a0) for i, j in mol['bonds'][p0:p1]]
            g = ligand_graph([int(e) for e in mol['elem'][a0:a1]], [int(f) for f in mol['frag'][a0:a1]], rows,
                             None if bond_label is None else [int(l) for l in bond_label[p0:p1]],
                             None if atom_label is None else [int(l) for l in atom_label[a0:a1]], z, largest_only, skip_h)
        if g is None:
            status[b] = NO_MOLECULE
            continue
        n = len(g.S)
        todo = [(i, j) for i in range(K) for j in range(i + 1, K)] if pairs else [(None, k) for k in range(K)]
        for i, j in todo:
            X = (ref_pos if i is None else pos[i])[a0:a1]
            Y = pos[j][a0:a1]
            if not (np.isfinite(np.asarray(X)[g.S]).all() and np.isfinite(Y[g.S]).all()):
                status[b] |= NONFINITE
                continue
            r = search(g, X, Y, max_nodes)
            if r['hit']:
                status[b] |= HIT_MAX_NODES
            if pairs:
                rmsd[b, i, j] = rmsd[b, j, i] = rms(r['best'], n)
                plain[b, i, j] = plain[b, j, i] = rms(r['s_id'], n)
                nodes[b, i, j] = nodes[b, j, i] = r['nodes']
            else:
                rmsd[b, j], plain[b, j], nodes[b, j] = rms(r['best'], n), rms(r['s_id'], n), r['nodes']
                for u, v in r['map'].items():
                    amap[j, a0 + u] = a0 + v
    return dict(rmsd=rmsd, plain=plain, nodes=nodes, map=amap, status=status)
