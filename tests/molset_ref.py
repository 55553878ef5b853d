"""Plain Python integer restatement of the molecule keys, fingerprints and Tanimoto diversity of include/kpd.h (kpd_mol_keys,
kpd_fp_diversity), the yardstick of tests/test_molset_gpu.py.  Written from the header comment alone: unsigned 64-bit
arithmetic as Python integers reduced with `& MASK`, one ligand at a time, no batching.  Not imported by the package."""
from collections import deque

import numpy as np

MASK = 2 ** 64 - 1
K1, K2, K3 = 0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9
FAR = 65535
NO_MOLECULE, BAD_SEGMENT = 1, 1
MOL_EMPTY, MOL_CAPACITY, MOL_LEFT_OUT = 1, 2, 8             # status bits of kpd_mol_perceive that leave no molecule
MAX_ATOMS = 256


def mix(x):
    x &= MASK
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & MASK
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & MASK
    return x ^ x >> 31


def distances(n, nbrs, a):
    """Shortest-path lengths in bonds from a; FAR where there is no path."""
    d = [FAR] * n
    d[a] = 0
    queue = deque([a])
    while queue:
        i = queue.popleft()
        for j, _ in nbrs[i]:
            if d[j] == FAR:
                d[j] = d[i] + 1
                queue.append(j)
    return d


def step(x, nbrs, S):
    return {a: mix(K1 * x[a] + sum(mix(x[b] + l * K2) for b, l in nbrs[a])) for a in S}


def graph_key(Z, bonds, labels=None, S=None, radius=2, nbits=2048):
    """Z: atomic number of every atom, bonds: (i, j) pairs, labels: the bond labels l (None: all 1), S: the atoms in scope
    (None: all).  Returns dict(key, inv [n] (0 outside S), fp: nbits / 32 words)."""
    n = len(Z)
    S = sorted(range(n) if S is None else S)
    inside = set(S)
    labels = [1] * len(bonds) if labels is None else labels
    nbrs = [[] for _ in range(n)]
    m = 0
    for (i, j), l in zip(bonds, labels):
        if i in inside and j in inside:
            nbrs[i].append((j, int(l)))
            nbrs[j].append((i, int(l)))
            m += 1
    # fingerprint: local seeds
    words = [0] * (nbits // 32)
    f = {a: mix(Z[a] + len(nbrs[a]) * K3) for a in S}
    for r in range(radius + 1):
        if r:
            f = step(f, nbrs, S)
        for a in S:
            bit = f[a] % nbits
            words[bit >> 5] |= 1 << (bit & 31)
    # key: seeds that see every other atom by element and distance
    inv = {}
    for a in S:
        d = distances(n, nbrs, a)
        inv[a] = mix(Z[a] + len(nbrs[a]) * K3 + K1 * sum(mix(Z[b] * K2 + d[b]) for b in S if b != a))
    for _ in range(len(S)):
        inv = step(inv, nbrs, S)
    key = mix(len(S) + m * K3 + K1 * sum(mix(inv[a]) for a in S))
    return dict(key=key, inv=[inv.get(a, 0) for a in range(n)], fp=words)


def largest_fragment(frag):
    """The atoms of the largest fragment: most atoms, the lowest rank on a tie."""
    sizes = np.bincount(np.asarray(frag, dtype=np.int64))
    return [a for a, f in enumerate(frag) if f == int(np.argmax(sizes))]          # argmax: the first maximum


def signed(x):
    return x - 2 ** 64 if x >= 2 ** 63 else x


def keys_batch(ref, ptr, z, largest_only=True, with_orders=True, radius=2, nbits=2048):
    """The outputs of kpd_mol_keys on what molecule_ref.perceive_batch returned: key [B] int64, fp [B, nbits/32] (uint32 values
    as int64), atom_inv [N] int64, status [B]."""
    B, N = len(ptr) - 1, len(ref['elem'])
    key, fp = np.zeros(B, dtype=np.int64), np.zeros((B, nbits // 32), dtype=np.int64)
    atom_inv, status = np.zeros(N, dtype=np.int64), np.zeros(B, dtype=np.int64)
    for b in range(B):
        m = ref['mols'][b]
        if m is None or int(ref['status'][b]) & (MOL_EMPTY | MOL_CAPACITY | MOL_LEFT_OUT):
            status[b] = NO_MOLECULE
            continue
        S = largest_fragment(m['frag']) if largest_only else None
        r = graph_key([int(z[e]) for e in m['elem']], [tuple(map(int, ij)) for ij in m['bonds']],
                      [int(o) for o in m['order']] if with_orders else None, S, radius, nbits)
        key[b], fp[b] = signed(r['key']), r['fp']
        atom_inv[int(ptr[b]):int(ptr[b + 1])] = [signed(v) for v in r['inv']]
    return dict(key=key, fp=fp, atom_inv=atom_inv, status=status)


def tanimoto_distance(a, b):
    c = sum(bin(int(x) & int(y)).count('1') for x, y in zip(a, b))
    u = sum(bin(int(x) | int(y)).count('1') for x, y in zip(a, b))
    return 1.0 - (c / u if u else 1.0)


def diversity(fp, use, group_ptr):
    """The outputs of kpd_fp_diversity: (div_sum [G] float64, n_pairs [G], status [G]).  The sum is taken in Python's order,
    i ascending then j ascending; the kernel's order differs, which the test's summation bound covers."""
    B, G = len(fp), len(group_ptr) - 1
    rows = [int.from_bytes(np.asarray(r, dtype=np.uint32).tobytes(), 'little') for r in np.asarray(fp, dtype=np.int64) & 0xffffffff]
    div_sum, n_pairs, status = np.zeros(G), np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.int64)
    for g in range(G):
        g0, g1 = int(group_ptr[g]), int(group_ptr[g + 1])
        if not 0 <= g0 <= g1 <= B:
            status[g] = BAD_SEGMENT
            continue
        members = [i for i in range(g0, g1) if use[i]]
        for q, j in enumerate(members):
            for i in members[:q]:
                c, u = bin(rows[i] & rows[j]).count('1'), bin(rows[i] | rows[j]).count('1')
                div_sum[g] += 1.0 - (c / u if u else 1.0)
                n_pairs[g] += 1
    return div_sum, n_pairs, status
