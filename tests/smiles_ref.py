"""Plain Python restatement of the SMILES rule of include/kpd.h (kpd_mol_smiles), the yardstick of tests/test_smiles_gpu.py, and
a small SMILES reader for the subset that rule emits.  The writer is written from the header comment alone: unsigned 64-bit
arithmetic as Python integers reduced with `& MASK`, strings, one ligand at a time.  The reader is written from the SMILES
definition (organic-subset and bracket atoms, - = #, branches, ring-closure digits and %nn, '.', lower case for aromatic atoms,
implied hydrogens), not from the writer.  Not imported by the package."""
from .molset_ref import K1, K2, K3, MASK, MAX_ATOMS, distances, mix

NO_MOLECULE, CLOSURES_EXHAUSTED, CAPACITY = 1, 2, 4
MOL_EMPTY, MOL_CAPACITY, MOL_LEFT_OUT = 1, 2, 8             # status bits of kpd_mol_perceive that leave no molecule
ATOM_AROMATIC, BOND_AROMATIC = 2, 4                         # of kpd_mol_sanitize's atom_flags and bond_flags
MAX_DEG, MAX_H, MAX_CLOSURE = 6, 9, 99
# the organic subset: atomic number -> normal valences; the aromatic organic subset is b c n o p s
NORMAL = {5: (3,), 6: (4,), 7: (3, 5), 8: (2,), 15: (3, 5), 16: (2, 4, 6), 9: (1,), 17: (1,), 35: (1,), 53: (1,)}
AROMATIC_SUBSET = (5, 6, 7, 8, 15, 16)


class Exhausted(Exception):
    pass


def implied_h(Z, ar, labels):
    """The hydrogens a SMILES reader gives a bare atom of the organic subset with these bond labels (4 = aromatic)."""
    total = sum(1 if l == 4 else l for l in labels)
    if ar:                                          # an aromatic atom counts one more, and only the smallest valence is tried
        return max(0, NORMAL[Z][0] - (total + 1))
    for v in NORMAL[Z]:
        if v >= total:
            return v - total
    return 0


def neighbours(n, bonds, labels, S):
    inside = set(S)
    nbrs = [[] for _ in range(n)]
    for (i, j), l in zip(bonds, labels):
        if i in inside and j in inside:
            nbrs[i].append((j, int(l)))
            nbrs[j].append((i, int(l)))
    return nbrs


def distinct(x, S):
    return len({x[a] for a in S})


def canonical_ranks(Z, h, ar, bonds, labels, S=None):
    """rank[a] for a in S (a dict) and the number of tie-breaking rounds taken."""
    n = len(Z)
    S = sorted(range(n) if S is None else S)
    nbrs = neighbours(n, bonds, labels, S)

    def step(x):
        return {a: mix(K1 * x[a] + sum(mix(x[b] + l * K2) for b, l in nbrs[a])) for a in S}
    x = {}
    for a in S:
        d = distances(n, nbrs, a)
        x[a] = mix(Z[a] + len(nbrs[a]) * K3 + (2 * h[a] + ar[a]) * K2 + K1 * sum(mix(Z[b] * K2 + d[b]) for b in S if b != a))
    for _ in range(len(S)):
        x = step(x)
    rounds = 0
    while True:
        count = distinct(x, S)
        if count == len(S):
            break
        values = sorted(x[a] for a in S)
        shared = min(v for k, v in enumerate(values[:-1]) if values[k + 1] == v)
        a = min(a for a in S if x[a] == shared)             # the only place the numbering enters
        x[a] = mix(x[a] + K3)
        count += 1
        rounds += 1
        for _ in range(len(S)):
            x = step(x)
            now = distinct(x, S)
            if now == count:
                break
            count = now
    return {a: sum(1 for b in S if x[b] < x[a]) for a in S}, rounds


def atom_token(Z, h, ar, symbol, labels):
    text = symbol[:1].lower() + symbol[1:] if ar else symbol
    if Z in NORMAL and (not ar or Z in AROMATIC_SUBSET) and implied_h(Z, ar, labels) == h:
        return text
    return '[' + text + ('' if h == 0 else 'H' if h == 1 else 'H%d' % h) + ']'


def bond_symbol(l, ar_a, ar_b):
    if l == 1:
        return '-' if ar_a and ar_b else ''
    return {2: '=', 3: '#', 4: ''}[l]


def closure_text(d):
    return str(d) if d < 10 else '%%%02d' % d


def write(Z, h, ar, symbols, bonds, labels, S=None, frag=None):
    """The string of one labelled graph: (text, status).  Z / h / ar / symbols per atom, bonds (i, j) with labels 1 .. 4, S the
    atoms in scope (None: all), frag: the fragment label of every atom (None: the connected components)."""
    n = len(Z)
    S = sorted(range(n) if S is None else S)
    nbrs = neighbours(n, bonds, labels, S)
    if frag is not None:                            # the labels must be the connected components of S
        for a in S:
            if any(frag[b] != frag[a] for b, _ in nbrs[a]):
                return '', NO_MOLECULE
    rank, _ = canonical_ranks(Z, h, ar, bonds, labels, S)
    for a in S:
        nbrs[a].sort(key=lambda e: rank[e[0]])
    label_of = {(a, b): l for a in S for b, l in nbrs[a]}
    seen_comp, comp = {}, {}
    for a in S:                                     # components, to name the start atoms
        if a in comp:
            continue
        todo, comp[a] = [a], a
        while todo:
            u = todo.pop()
            for v, _ in nbrs[u]:
                if v not in comp:
                    comp[v] = a
                    todo.append(v)
    if frag is not None:
        for a in S:
            if seen_comp.setdefault(frag[a], comp[a]) != comp[a]:
                return '', NO_MOLECULE
    starts = {}
    for a in S:
        key = (len(nbrs[a]), rank[a])
        if comp[a] not in starts or key < starts[comp[a]][0]:
            starts[comp[a]] = (key, a)
    vis, par, children = {}, {}, {a: [] for a in S}

    def walk(a):
        vis[a] = len(vis)
        for b, _ in nbrs[a]:
            if b not in vis:
                par[b] = a
                children[a].append(b)
                walk(b)
    free, digit = [True] * (MAX_CLOSURE + 1), {}

    def emit(a):
        out = atom_token(Z[a], h[a], ar[a], symbols[a], [l for _, l in nbrs[a]])
        ending = sorted(digit[(b, a)] for b, _ in nbrs[a] if vis[b] < vis[a] and par.get(a) != b)
        for d in ending:
            out += closure_text(d)
            free[d] = True
        for b, l in nbrs[a]:
            if vis[b] > vis[a] and par[b] != a:
                d = next((k for k in range(1, MAX_CLOSURE + 1) if free[k]), None)
                if d is None:
                    raise Exhausted
                free[d] = False
                digit[(a, b)] = d
                out += bond_symbol(l, ar[a], ar[b]) + closure_text(d)
        for k, c in enumerate(children[a]):
            s = bond_symbol(label_of[(a, c)], ar[a], ar[c]) + emit(c)
            out += s if k == len(children[a]) - 1 else '(' + s + ')'
        return out
    parts = []
    try:
        for _, a in sorted(starts.values(), key=lambda e: rank[e[1]]):
            walk(a)
            parts.append(emit(a))
    except Exhausted:
        return '', CLOSURES_EXHAUSTED
    return '.'.join(parts), 0


def largest_fragment(frag):
    sizes = {}
    for f in frag:
        sizes[f] = sizes.get(f, 0) + 1
    best = max(sizes, key=lambda f: (sizes[f], -f))
    return [a for a, f in enumerate(frag) if f == best]


def smiles_ligand(elem, frag, bonds, order_k, bond_flags, atom_h, atom_flags, z, symbols, largest_only, aromatic):
    """One ligand, local rows: (text, status) with every no-molecule condition of kpd_mol_smiles."""
    n, F = len(elem), len(z)
    if n <= 0 or n > MAX_ATOMS:
        return '', NO_MOLECULE
    if any(e < 0 or e >= F for e in elem) or any(f < 0 or f >= n for f in frag) or any(x < 0 or x > MAX_H for x in atom_h):
        return '', NO_MOLECULE
    if any(i < 0 or i >= n or j < 0 or j >= n or i == j or o < 1 or o > 3 for (i, j), o in zip(bonds, order_k)):
        return '', NO_MOLECULE
    S = largest_fragment(frag) if largest_only else list(range(n))
    inside, seen, deg = set(S), set(), [0] * n
    for i, j in bonds:
        if i in inside and j in inside:
            if (min(i, j), max(i, j)) in seen or deg[i] >= MAX_DEG or deg[j] >= MAX_DEG:
                return '', NO_MOLECULE
            seen.add((min(i, j), max(i, j)))
            deg[i] += 1
            deg[j] += 1
    Zs = [int(z[e]) for e in elem]
    ar = [int(bool(aromatic and f & ATOM_AROMATIC)) for f in atom_flags]
    labels = [4 if aromatic and f & BOND_AROMATIC else int(o) for o, f in zip(order_k, bond_flags)]
    return write(Zs, [int(x) for x in atom_h], ar, [symbols[e] for e in elem], bonds, labels, S, frag)


def smiles_batch(ptr, mol, san, z, symbols, largest_only=False, aromatic=True, capacity=None):
    """The outputs of kpd_mol_smiles for a batch: (the bytes of every ligand, text_ptr list of B + 1, status list of B); ligand b's
    bytes stand at text[text_ptr[b]:text_ptr[b + 1]] unless its status has the capacity bit.  `mol`: elem / frag [N], bonds [cap,2]
    (global rows), bond_ptr [B+1], status [B]; `san`: order_k / bond_flags [cap], atom_h / atom_flags [N], status [B]."""
    B, N, cap = len(ptr) - 1, len(mol['elem']), len(san['order_k'])
    texts, status = [], []
    for b in range(B):
        a0, a1 = int(ptr[b]), int(ptr[b + 1])
        p0, p1 = int(mol['bond_ptr'][b]), int(mol['bond_ptr'][b + 1])
        ok = (0 <= a0 <= a1 <= N and not int(mol['status'][b]) & (MOL_EMPTY | MOL_CAPACITY | MOL_LEFT_OUT) and not int(san['status'][b]) & 1 and
              0 <= p0 <= p1 <= cap and p1 - p0 <= 3 * MAX_ATOMS)
        t, st = '', NO_MOLECULE
        if ok:
            rows = [(int(i) - a0, int(j) - a0) for i, j in mol['bonds'][p0:p1]]
            t, st = smiles_ligand([int(e) for e in mol['elem'][a0:a1]], [int(f) for f in mol['frag'][a0:a1]], rows,
                                  [int(o) for o in san['order_k'][p0:p1]], [int(f) for f in san['bond_flags'][p0:p1]],
                                  [int(x) for x in san['atom_h'][a0:a1]], [int(f) for f in san['atom_flags'][a0:a1]], z, symbols,
                                  largest_only, aromatic)
        texts.append(t.encode('ascii'))
        status.append(st)
    text_ptr = [0]
    for t in texts:
        text_ptr.append(text_ptr[-1] + len(t))
    for b in range(B):                              # a ligand that ends beyond the capacity is not written
        if capacity is not None and not status[b] and text_ptr[b + 1] > capacity:
            status[b] |= CAPACITY
    return texts, text_ptr, status


# ---- the reader -----------------------------------------------------------------------------------------------------------------
# The reader shares no table and no function with the writer above: an error in the writer's implied-hydrogen rule must not
# read back as if it were right.  From the SMILES definition: a bare atom of the organic subset is filled with hydrogens up to the
# lowest of its normal valences that its bonds do not exceed; an aromatic atom has given one valence to the ring's pi system, and
# only its lowest valence is considered.
ORGANIC_SYMBOLS = ('B', 'C', 'N', 'O', 'P', 'S', 'F', 'Cl', 'Br', 'I')
READER_VALENCES = dict(B=[3], C=[4], N=[3, 5], O=[2], P=[3, 5], S=[2, 4, 6], F=[1], Cl=[1], Br=[1], I=[1])
BOND_ORDER_USED = {1: 1, 2: 2, 3: 3, 4: 1}          # an aromatic bond uses one valence; the atom's pi share is counted once below


def reader_hydrogens(symbol, aromatic, bond_labels):
    used = 0
    for l in bond_labels:
        used += BOND_ORDER_USED[l]
    if aromatic:
        lowest = READER_VALENCES[symbol][0]
        return lowest - used - 1 if lowest > used + 1 else 0
    for valence in READER_VALENCES[symbol]:
        if used <= valence:
            return valence - used
    return 0


def read(text):
    """A SMILES string of the subset above -> (atoms, bonds): atoms [(symbol with a capital first letter, h, aromatic)], bonds
    [(i, j, label)] with label 4 for an aromatic bond.  Raises ValueError on anything else."""
    atoms, explicit_h, bonds = [], [], []
    prev, pending, stack, rings = None, None, [], {}

    def add_atom(symbol, aromatic, h):
        nonlocal prev, pending
        atoms.append([symbol, aromatic])
        explicit_h.append(h)
        if prev is not None:
            bonds.append([prev, len(atoms) - 1, pending])
        elif pending is not None:
            raise ValueError('a bond symbol with no atom before it')
        prev, pending = len(atoms) - 1, None
    k = 0
    while k < len(text):
        c = text[k]
        if c == '(':
            if prev is None:
                raise ValueError('a branch with no atom before it')
            stack.append(prev)
            k += 1
        elif c == ')':
            prev = stack.pop()
            k += 1
        elif c == '.':
            if pending is not None or stack:
                raise ValueError('a dot inside a bond or a branch')
            prev = None
            k += 1
        elif c in '-=#':
            pending = {'-': 1, '=': 2, '#': 3}[c]
            k += 1
        elif c.isdigit() or c == '%':
            if c == '%':
                if not (text[k + 1:k + 3].isdigit() and len(text[k + 1:k + 3]) == 2):
                    raise ValueError('%nn needs two digits')
                number, k = int(text[k + 1:k + 3]), k + 3
            else:
                number, k = int(c), k + 1
            if prev is None:
                raise ValueError('a ring closure with no atom before it')
            if number in rings:
                other, first = rings.pop(number)
                if first is not None and pending is not None and first != pending:
                    raise ValueError('the two ends of a ring closure disagree')
                if other == prev:
                    raise ValueError('a ring closure onto its own atom')
                bonds.append([other, prev, first if first is not None else pending])
            else:
                rings[number] = (prev, pending)
            pending = None
        elif c == '[':
            end = text.index(']', k)
            body = text[k + 1:end]
            if not body or not body[0].isalpha():
                raise ValueError('an empty bracket atom')
            m = 2 if len(body) > 1 and body[1].islower() else 1
            symbol, rest = body[:m], body[m:]
            h = 0
            if rest.startswith('H'):
                h = int(rest[1:]) if len(rest) > 1 else 1
            elif rest:
                raise ValueError(f'unsupported bracket atom [{body}]')
            add_atom(symbol[0].upper() + symbol[1:], symbol[0].islower(), h)
            k = end + 1
        else:
            symbol = text[k:k + 2] if text[k:k + 2] in ('Cl', 'Br') else c
            if symbol in ORGANIC_SYMBOLS:
                add_atom(symbol, False, None)
            elif symbol in 'bcnops':
                add_atom(symbol.upper(), True, None)
            else:
                raise ValueError(f'unexpected character {c!r}')
            k += len(symbol)
    if rings or stack or pending is not None:
        raise ValueError('an unclosed ring, branch or bond')
    out_bonds = []
    for i, j, l in bonds:                           # no symbol: aromatic between two aromatic atoms, else single
        out_bonds.append((i, j, l if l is not None else 4 if atoms[i][1] and atoms[j][1] else 1))
    if len({(min(i, j), max(i, j)) for i, j, _ in out_bonds}) != len(out_bonds):
        raise ValueError('a bond twice')
    out_atoms = []
    for a, (symbol, aromatic) in enumerate(atoms):
        h = explicit_h[a]
        if h is None:                               # a bare atom: the smallest normal valence that holds its bonds
            h = reader_hydrogens(symbol, aromatic, [l for i, j, l in out_bonds if a in (i, j)])
        out_atoms.append((symbol, h, int(aromatic)))
    return out_atoms, out_bonds
