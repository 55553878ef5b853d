"""Labelled graphs for the SMILES tests (tests/test_smiles_config.py, tests/test_smiles_gpu.py): molecules written by hand with the
bytes the rule of include/kpd.h gives them, the seeded random graphs of tests/test_molset_config.py, renumbering of a labelled
graph, and the graphs that reach closure number 10 and that run out of numbers.  A labelled graph is the tuple
(Z, h, ar, symbols, bonds, labels): per atom the atomic number, hydrogens, aromatic flag and element symbol; per bond (i, j) and
the label 1 .. 3, or 4 for an aromatic bond."""
import random

import numpy as np

from . import sanitize_ref as SR

NUMBERS = {'H': 1, 'B': 5, 'C': 6, 'N': 7, 'O': 8, 'F': 9, 'Si': 14, 'P': 15, 'S': 16, 'Cl': 17, 'Br': 35, 'I': 53}


def graph(symbols, bonds, aromatic=(), h=None):
    """symbols per atom, bonds {(i, j): label}, aromatic: the aromatic atoms; h: {atom: hydrogens}, for every other atom the
    hydrogen rule of kpd_mol_sanitize (step 5) on the Kekule orders, an aromatic bond counting as the orders 1 and 2 in turn."""
    n = len(symbols)
    Z = [NUMBERS[s] for s in symbols]
    ar = [int(a in aromatic) for a in range(n)]
    val = [0] * n
    for (i, j), l in bonds.items():
        for a in (i, j):
            val[a] += 1 if l == 4 else l
    hs = []
    for a in range(n):
        v = val[a] + ar[a]                          # an aromatic atom has one double bond in any Kekule structure (or a lone pair: h)
        hs.append(max(0, SR.normal_valence(Z[a], v) - v))
    for a, x in (h or {}).items():
        hs[a] = x
    return Z, hs, ar, list(symbols), list(bonds), list(bonds.values())


def ring(n, label=1, at=0):
    return {(at + k, at + (k + 1) % n): label for k in range(n)}


def kekule(n, at=0):
    return {(at + k, at + (k + 1) % n): 2 - k % 2 for k in range(n)}


BIPHENYL = {**ring(6, 4), **ring(6, 4, 6), (0, 6): 1}
NAPHTHALENE = {**{(k, k + 1): 4 for k in range(9)}, (9, 0): 4, (0, 5): 4}          # a ring of ten and the shared bond
DICYCLOPROPYL = {(0, 1): 1, (1, 2): 1, (1, 5): 1, **ring(3, 1, 2), **ring(3, 1, 5)}     # CH3-CH(C3H5)2
SPIRO = {**ring(5), (0, 5): 1, (5, 6): 1, (6, 7): 1, (7, 8): 1, (8, 0): 1}         # spiro[4.4]nonane: atom 0 in both rings

# (name, graph, aromatic mode, expected bytes).  What the rule fixes without a hash is said in the comment; where two atoms compete
# on their hashed values alone (which end of ethanol is the start) the bytes record the choice, and the round trip of
# tests/test_smiles_config.py shows that either would be the same molecule.
BY_HAND = [
    # one atom, no bond: C has 4 - 0 hydrogens = what a reader implies for a bare C; O likewise 2
    ('methane', graph(['C'], {}), 1, 'C'),
    ('water', graph(['O'], {}), 1, 'O'),
    # C-C-O: the ends have degree 1, the start is the one of lower rank (here the O), then the chain; every atom bare
    ('ethanol', graph(['C', 'C', 'O'], {(0, 1): 1, (1, 2): 1}), 1, 'OCC'),
    ('ethene', graph(['C', 'C'], {(0, 1): 2}), 1, 'C=C'),
    ('ethyne', graph(['C', 'C'], {(0, 1): 3}), 1, 'C#C'),
    # three fragments in the order of their start atoms' ranks, '.' between them; inside an ethanol as above
    ('two ethanols and a chloride', graph(['C', 'C', 'O', 'C', 'C', 'O', 'Cl'], {(0, 1): 1, (1, 2): 1, (3, 4): 1, (4, 5): 1}), 1, 'Cl.OCC.OCC'),
    # six equivalent atoms: the start opens closure 1, five atoms follow, the last ends it; aromatic bonds have no symbol
    ('benzene', graph(['C'] * 6, ring(6, 4), aromatic=range(6)), 1, 'c1ccccc1'),
    # the Kekule form: the walk enters the ring over a single or a double bond, then they alternate; the closure carries the
    # symbol where it opens
    ('benzene, Kekule', graph(['C'] * 6, kekule(6)), 0, 'C=1C=CC=CC1'),
    # n with two aromatic bonds: 2 + 1 = 3 = the valence, no hydrogen implied, none there: bare
    ('pyridine', graph(['N'] + ['C'] * 5, ring(6, 4), aromatic=range(6)), 1, 'c1ccccn1'),
    # the N-H: a reader implies max(0, 3 - (2 + 1)) = 0, the atom has 1: [nH]
    ('pyrrole', graph(['N'] + ['C'] * 4, ring(5, 4), aromatic=range(5), h={0: 1}), 1, '[nH]1cccc1'),
    # n with a methyl: t = 3, implied max(0, 3 - 4) = 0 = h: bare n
    ('N-methylpyrrole', graph(['N'] + ['C'] * 5, {**ring(5, 4), (0, 5): 1}, aromatic=range(5), h={0: 0}), 1, 'Cn1cccc1'),
    ('furan', graph(['O'] + ['C'] * 4, ring(5, 4), aromatic=range(5)), 1, 'c1occc1'),
    ('thiophene', graph(['S'] + ['C'] * 4, ring(5, 4), aromatic=range(5), h={0: 0}), 1, 'c1cscc1'),
    # 2-pyridone: the C=O carbon is aromatic with t = 1 + 1 + 2 = 4, implied max(0, 4 - 5) = 0 = h: bare c, '=' to the O; N-H [nH].
    # The O has degree 1 and is the only such atom: it is the start
    ('2-pyridone', graph(['N'] + ['C'] * 5 + ['O'], {**ring(6, 4), (1, 6): 2}, aromatic=range(6), h={0: 1, 1: 0}), 1, 'O=c1cccc[nH]1'),
    # the bond between the rings is single between two aromatic atoms: '-'
    ('biphenyl', graph(['C'] * 12, BIPHENYL, aromatic=range(12), h={0: 0, 6: 0}), 1, 'c1cccc(-c2ccccc2)c1'),
    # two rings share the bond (0, 5): two closures
    ('naphthalene', graph(['C'] * 10, NAPHTHALENE, aromatic=range(10), h={0: 0, 5: 0}), 1, 'c1c2ccccc2ccc1'),
    # every atom of minimal degree (2) is a ring CH2, so the walk starts INSIDE a ring and opens closure 1 there; the spiro centre
    # is reached with 1 still open, so the second ring takes 2, is written as the branch, and 1 ends last.  Which CH2 starts is
    # the hashed ranks' choice (here one two bonds from the centre); no number is reused in this molecule
    ('spiro[4.4]nonane', graph(['C'] * 9, SPIRO), 1, 'C1CCC2(CCCC2)C1'),
    # 1,1-dicyclopropylethane, a number reused after it has ended, derived without a hash.  Degrees: the methyl (atom 0) 1, the CH
    # (atom 1) 3, the ring atoms 2 and 5 that hang on it 3, the four ring CH2 2.  The methyl is the only atom of degree 1: the
    # start, "C".  Its one neighbour follows, "C".  That atom has two unvisited neighbours, atoms 2 and 5; the two cyclopropyls are
    # images of each other, so either order gives the same bytes: the first child goes in parentheses.  At a ring's first atom the
    # two CH2 are unvisited and equivalent: one becomes the child, the other will be reached through it, so its bond is a closure
    # that OPENS here with the lowest free number, 1: "C1".  The child "C", its child "C", where the closure ENDS: "1", and the
    # number is free again: "(C1CC1)".  The second child is the last one, no parentheses, and its closure takes the lowest free
    # number, which is 1 once more: "C1CC1".  Every atom is bare: the bond sums 1, 3, 3, 2, 2 imply the 3, 1, 1, 2, 2 hydrogens
    ('1,1-dicyclopropylethane', graph(['C'] * 8, DICYCLOPROPYL), 1, 'CC(C1CC1)C1CC1'),
    # N with four single bonds: t = 4, the reader would take valence 5 and imply one hydrogen, the atom has none: [N]
    ('tetramethyl N, over-valent', graph(['N'] + ['C'] * 4, {(0, k): 1 for k in range(1, 5)}, h={0: 0}), 1, 'C[N](C)(C)C'),
    # a lone B has 3 hydrogens, as a reader implies: bare; Si is outside the organic subset: always in brackets
    ('borane', graph(['B'], {}), 1, 'B'),
    ('silane', graph(['Si'], {}), 1, '[SiH4]'),
]


# ---- the seeded random graphs of tests/test_molset_config.py (random_graph, copied: that file is a test module) ---------------------
def random_graph(rng):
    """A connected molecule-like graph: 4-9 atoms of C / N / O, degree <= 4, bond labels 1 / 2."""
    C, N, O = 6, 7, 8
    n = rng.randint(4, 9)
    Z = [rng.choice([C, C, C, N, O]) for _ in range(n)]
    deg, bonds = [0] * n, set()
    for a in range(1, n):
        open_ = [b for b in range(a) if deg[b] < 4]
        b = rng.choice(open_)
        bonds.add((b, a))
        deg[a] += 1
        deg[b] += 1
    for _ in range(rng.randint(0, 3)):
        i, j = sorted(rng.sample(range(n), 2))
        if (i, j) not in bonds and deg[i] < 4 and deg[j] < 4:
            bonds.add((i, j))
            deg[i] += 1
            deg[j] += 1
    bonds = sorted(bonds)
    return Z, bonds, [rng.choice([1, 1, 2]) for _ in bonds]


def random_set(count=700, seed=1):
    """The graphs of random_graph(random.Random(seed)) as labelled graphs: ar = 0, h from the valence rule of kpd_mol_sanitize."""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        Z, bonds, labels = random_graph(rng)
        val = [0] * len(Z)
        for (i, j), l in zip(bonds, labels):
            val[i] += l
            val[j] += l
        h = [max(0, SR.normal_valence(z, v) - v) for z, v in zip(Z, val)]
        out.append((Z, h, [0] * len(Z), [{6: 'C', 7: 'N', 8: 'O'}[z] for z in Z], bonds, labels))
    return out


def permuted(g, rng):
    """The same labelled graph with its atoms renumbered, its bonds shuffled and their ends swapped at random."""
    Z, h, ar, sym, bonds, labels = g
    n = len(Z)
    p = list(range(n))
    rng.shuffle(p)

    def moved(x):
        y = [None] * n
        for a in range(n):
            y[p[a]] = x[a]
        return y
    rows = [((p[i], p[j]) if rng.random() < 0.5 else (p[j], p[i]), l) for (i, j), l in zip(bonds, labels)]
    rng.shuffle(rows)
    return moved(Z), moved(h), moved(ar), moved(sym), [r[0] for r in rows], [r[1] for r in rows]


# ---- many closures open at once: a ring of n carbons with seeded chords, every atom of degree 2 + matchings --------------------------
def chorded_ring(n, matchings, seed):
    """A ring of n carbons and `matchings` seeded perfect matchings of chords on top (no bond twice): degree 2 + matchings."""
    rng = random.Random(seed)
    bonds = {(k, (k + 1) % n) if k + 1 < n else (0, k) for k in range(n)}
    for _ in range(matchings):
        while True:
            p = list(range(n))
            rng.shuffle(p)
            chords = {(min(p[2 * k], p[2 * k + 1]), max(p[2 * k], p[2 * k + 1])) for k in range(n // 2)}
            if not chords & bonds:
                break
        bonds |= chords
    bonds = sorted(bonds)
    deg = np.bincount(np.array(bonds).flatten(), minlength=n)
    return [6] * n, [max(0, 4 - int(d)) for d in deg], [0] * n, ['C'] * n, bonds, [1] * len(bonds)


TEN_CLOSURES = chorded_ring(40, 1, 3)               # reaches %10 (checked in tests/test_smiles_config.py)
EXHAUSTED = chorded_ring(256, 2, 3)                 # more than 99 closures open at once
