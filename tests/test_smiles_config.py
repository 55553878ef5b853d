"""The SMILES rule of include/kpd.h as restated in tests/smiles_ref.py, checked without a GPU against facts that do not come from
it: strings written out by hand, a reader written from the SMILES definition (every string reads back to the labelled graph it
was written from), independence of the numbering of the atoms, string equality against labelled-graph isomorphism on a seeded
random set, the closure numbers from %10 to exhaustion, and the declarations and refusals of the C ABI and the Python surface."""
import ctypes
import itertools
import os
import random

import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import hip, molecule, utils
from . import molecule_ref as R
from . import sanitize_cases as C
from . import sanitize_ref as SR
from . import smiles_cases as SC
from . import smiles_ref as S
from .molecule_cases import ALLOWED, ELEMENTS, Z, one_hot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RENUMBERINGS = 8


def labelled(sym, pos, aromatic=True):
    """(symbols, positions) -> the labelled graph kpd_mol_smiles sees, by the restatements of perception and sanitisation."""
    pos = np.asarray(pos, dtype=np.float32)
    m = R.perceive(pos, one_hot(sym), Z, ALLOWED)
    r = SR.sanitize(pos, m['elem'], m['frag'], m['bonds'], m['order'], Z, ALLOWED, C.MASS, C.MASS_H)
    ar = [int(bool(aromatic and f & S.ATOM_AROMATIC)) for f in r['atom_flags']]
    labels = [4 if aromatic and f & S.BOND_AROMATIC else int(o) for o, f in zip(r['order_k'], r['bond_flags'])]
    return ([Z[e] for e in m['elem']], [int(x) for x in r['atom_h']], ar, [ELEMENTS[e] for e in m['elem']],
            [tuple(map(int, ij)) for ij in m['bonds']], labels)


@pytest.fixture(scope='module')
def inputs():
    """(name, labelled graph): TEXTBOOK and TEMPLATES of tests/sanitize_cases.py in both modes, generated(48), the 700 random graphs."""
    out = []
    for aromatic in (True, False):
        out += [(f'{name}, aromatic={aromatic}', labelled(sym, pos, aromatic)) for name, sym, pos, _ in C.TEXTBOOK]
        out += [(f'template {name}, aromatic={aromatic}', labelled(sym, pos, aromatic)) for name, sym, pos in C.TEMPLATES]
    out += [(f'generated {k}', labelled(sym, pos)) for k, (sym, pos, _) in enumerate(C.generated(48))]
    out += [(f'random {k}', g) for k, g in enumerate(SC.random_set())]
    return out


def nx_graph(nx, atoms, bonds):
    G = nx.Graph()
    G.add_nodes_from((a, dict(label=lab)) for a, lab in enumerate(atoms))
    G.add_edges_from((i, j, dict(label=l)) for i, j, l in bonds)
    return G


def reads_back(nx, text, g):
    """The string read by tests/smiles_ref.read is isomorphic to g with node labels (Z, h, ar) and edge labels the bond labels."""
    from networkx.algorithms.isomorphism import categorical_edge_match, categorical_node_match
    Zs, h, ar, sym, bonds, labels = g
    atoms, read_bonds = S.read(text)
    got = nx_graph(nx, [(SC.NUMBERS[s], hh, a) for s, hh, a in atoms], read_bonds)
    want = nx_graph(nx, list(zip(Zs, h, ar)), [(i, j, l) for (i, j), l in zip(bonds, labels)])
    return nx.is_isomorphic(got, want, node_match=categorical_node_match('label', None), edge_match=categorical_edge_match('label', None))


# ---- 1. by hand ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', SC.BY_HAND, ids=[c[0] for c in SC.BY_HAND])
def test_strings_written_out_by_hand(case):
    _, g, _, expected = case
    assert S.write(*g) == (expected, 0)


def test_the_implied_hydrogens_of_a_reader():
    assert [S.implied_h(6, 0, [1] * k) for k in range(6)] == [4, 3, 2, 1, 0, 0]
    assert [S.implied_h(7, 0, [1] * k) for k in range(6)] == [3, 2, 1, 0, 1, 0]            # the valences 3 and 5
    assert [S.implied_h(16, 0, [2] * k) for k in range(4)] == [2, 0, 0, 0]                 # 2, 4, 6
    assert S.implied_h(6, 1, [4, 4]) == 1 and S.implied_h(6, 1, [4, 4, 4]) == 0 and S.implied_h(6, 1, [4, 4, 2]) == 0
    assert S.implied_h(7, 1, [4, 4]) == 0 and S.implied_h(7, 1, [4, 4, 1]) == 0 and S.implied_h(8, 1, [4, 4]) == 0
    assert S.atom_token(7, 1, 1, 'N', [4, 4]) == '[nH]' and S.atom_token(14, 0, 0, 'Si', [1] * 4) == '[Si]'
    assert S.atom_token(1, 0, 0, 'H', [1]) == '[H]' and S.atom_token(6, 2, 0, 'C', [1]) == '[CH2]' and S.atom_token(17, 0, 0, 'Cl', [1]) == 'Cl'
    assert S.atom_token(33, 0, 1, 'As', [4, 4]) == '[as]'
    # the reader's own rule and table, from the SMILES definition: C, CC, C=C, C#C, N with three and four single bonds, SF4-like and
    # sulfone-like S, a benzene c, a fused or substituted c, pyridine n, n-methyl, furan o, the c of c=O
    R = S.reader_hydrogens
    assert [R('C', False, b) for b in ([], [1], [2], [3], [1, 1, 1, 1])] == [4, 3, 2, 1, 0]
    assert R('N', False, [1] * 3) == 0 and R('N', False, [1] * 4) == 1 and R('S', False, [1] * 4) == 0 and R('S', False, [2, 2, 1]) == 1
    assert R('O', False, [1]) == 1 and R('Cl', False, []) == 1 and R('B', False, []) == 3 and R('P', False, [2, 1, 1, 1]) == 0
    assert [R('C', True, b) for b in ([4, 4], [4, 4, 4], [4, 4, 1], [4, 4, 2])] == [1, 0, 0, 0]
    assert R('N', True, [4, 4]) == 0 and R('N', True, [4, 4, 1]) == 0 and R('O', True, [4, 4]) == 0 and R('S', True, [4, 4]) == 0
    for z, sym in ((5, 'B'), (6, 'C'), (7, 'N'), (8, 'O'), (15, 'P'), (16, 'S'), (9, 'F'), (17, 'Cl'), (35, 'Br'), (53, 'I')):
        for labels in itertools.chain.from_iterable(itertools.combinations_with_replacement((1, 2, 3, 4), k) for k in range(5)):
            for ar in (0, 1):                       # the writer's rule is the reader's, on every bond pattern of up to four bonds
                assert S.implied_h(z, ar, list(labels)) == R(sym, bool(ar), list(labels)), (sym, ar, labels)


# ---- 2. round trip ----------------------------------------------------------------------------------------------------------------
def test_every_string_reads_back_to_its_graph(inputs):
    nx = pytest.importorskip('networkx')
    for name, g in inputs + [(c[0], c[1]) for c in SC.BY_HAND]:
        text, status = S.write(*g)
        assert status == 0 and text, name
        assert reads_back(nx, text, g), (name, text)


def test_the_reader_on_strings_it_did_not_write():
    atoms, bonds = S.read('OC(=O)c1ccccc1C#N')                    # by the definition: a carboxylic acid and a nitrile on a benzene ring
    assert [a[0] for a in atoms] == ['O', 'C', 'O', 'C', 'C', 'C', 'C', 'C', 'C', 'C', 'N']
    assert [a[1] for a in atoms] == [1, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0] and [a[2] for a in atoms] == [0, 0, 0] + [1] * 6 + [0, 0]
    assert sorted((min(i, j), max(i, j), l) for i, j, l in bonds) == [(0, 1, 1), (1, 2, 2), (1, 3, 1), (3, 4, 4), (3, 8, 4), (4, 5, 4), (5, 6, 4),
                                                                      (6, 7, 4), (7, 8, 4), (8, 9, 1), (9, 10, 3)]
    assert S.read('C%12CC%12.[nH]1cccc1')[1][:3] == [(0, 1, 1), (1, 2, 1), (0, 2, 1)]
    assert S.read('c1ccccc1-c1ccccc1')[1][6] == (5, 6, 1) and S.read('[SiH4].[H][H]')[0] == [('Si', 4, 0), ('H', 0, 0), ('H', 0, 0)]
    for broken in ('C1CC', 'C(C', 'C=', 'C%1C', '[C', 'Cx', 'C11'):
        with pytest.raises((ValueError, IndexError)):
            S.read(broken)


# ---- 3. numbering ------------------------------------------------------------------------------------------------------------------
def test_strings_do_not_depend_on_the_numbering(inputs):
    moved = []
    for name, g in inputs + [(c[0], c[1]) for c in SC.BY_HAND]:
        text, _ = S.write(*g)
        rng = random.Random(name)
        if any(S.write(*SC.permuted(g, rng))[0] != text for _ in range(RENUMBERINGS)):
            moved.append(name)
    assert moved == []                              # no exceptions allowed


def test_the_tie_breaking_loop_is_short(inputs):
    rounds = [S.canonical_ranks(g[0], g[1], g[2], g[4], g[5])[1] for _, g in inputs]
    print('tie-breaking rounds: max', max(rounds), 'mean', sum(rounds) / len(rounds))
    assert max(rounds) <= 8                         # benzene takes 2: one atom, then one of its two neighbours


# ---- 4. identity -------------------------------------------------------------------------------------------------------------------
def test_string_equality_is_labelled_graph_isomorphism_on_a_random_set():
    nx = pytest.importorskip('networkx')
    from networkx.algorithms.isomorphism import categorical_edge_match, categorical_node_match
    classes = {}
    for g in SC.random_set():
        Zs, h, ar, _, bonds, labels = g
        G = nx_graph(nx, list(zip(Zs, h, ar)), [(i, j, l) for (i, j), l in zip(bonds, labels)])
        classes.setdefault((len(Zs), tuple(sorted(Zs)), len(bonds)), []).append((G, S.write(*g)[0]))
    pairs = same = wrong = 0
    nm, em = categorical_node_match('label', None), categorical_edge_match('label', None)
    for members in classes.values():
        for (G1, s1), (G2, s2) in itertools.combinations(members, 2):
            iso = nx.is_isomorphic(G1, G2, node_match=nm, edge_match=em)
            pairs += 1
            same += iso
            wrong += iso != (s1 == s2)
    print(f'{pairs} pairs of equal size, composition and bond count, {same} isomorphic, {wrong} disagreements')
    assert pairs >= 500 and same >= 10
    assert wrong == 0


# ---- 5. closure numbers -------------------------------------------------------------------------------------------------------------
def test_closure_numbers_from_ten_to_exhaustion():
    nx = pytest.importorskip('networkx')
    text, status = S.write(*SC.TEN_CLOSURES)
    assert status == 0 and '%10' in text and '%100' not in text
    assert reads_back(nx, text, SC.TEN_CLOSURES)
    assert S.write(*SC.EXHAUSTED) == ('', S.CLOSURES_EXHAUSTED)
    assert S.closure_text(9) == '9' and S.closure_text(10) == '%10' and S.closure_text(99) == '%99'


# ---- 6. ABI and surface --------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'kpd.h')).read()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for s in ('kpd_mol_smiles', 'kpd_smiles_scratch_bytes'):
        assert s + '(' in header and s in hip.EXPORTS and hasattr(lib, s), s
    assert callable(hip.mol_smiles) and callable(molecule.Sanitized.smiles) and callable(molecule.Sanitized.unique)
    assert callable(utils.sampled_ligands_smiles) and callable(utils.write_smiles_file)
    for text in ('NOT RDKit', 'no charges, no stereo, no isotopes', 'LOWEST INDEX', 'analysis/metrics.py:102-147', '%nn'):
        assert text in header, text
    L = hip.lib()
    assert L.kpd_smiles_scratch_bytes(-1, 0) == -1 and L.kpd_smiles_scratch_bytes(0, 0) > 0
    assert L.kpd_smiles_scratch_bytes(1000, 10) >= 36 * 1000 + 12 * 10

    def call(capacity=0, aromatic=1, B=0, n_atoms=0, F=1):       # null pointers: refused before anything is launched
        return L.kpd_mol_smiles(None, n_atoms, B, None, F, None, None, None, None, None, None, None, 0, None, None, None, None, 1, aromatic,
                                None, capacity, None, None, None, None)
    for bad in (dict(capacity=-1), dict(aromatic=2), dict(aromatic=-1), dict(B=-1), dict(n_atoms=-1), dict(F=0), dict()):
        assert call(**bad) != 0, bad


def test_host_tensors_are_refused():
    ptr = torch.tensor([0, 5], dtype=torch.int32)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    mol = dict(elem=i32(5), frag=i32(5), bonds=i32(15, 2), order=i32(15), bond_ptr=i32(2), status=i32(1))
    san = dict(order_k=i32(15), bond_flags=i32(15), valence_k=i32(5), atom_h=i32(5), atom_flags=i32(5), desc_i=i32(1, 10),
               desc_f=torch.zeros(1, 2, dtype=torch.float64), valid=i32(1), status=i32(1))
    with pytest.raises(hip.KpdError):
        hip.mol_smiles(ptr, [6] * 10, ['C'] * 10, mol, san)
    m = molecule.Molecules(ptr, i32(1, 4), i32(1), mol['elem'], i32(5), mol['frag'], mol['bonds'], mol['order'], mol['bond_ptr'],
                           torch.zeros(5, 3), ['C'] * 10)
    s = molecule.Sanitized(m, san, [6] * 10, True)
    for call in (s.smiles, s.unique):
        with pytest.raises(hip.KpdError):
            call()
    with pytest.raises(hip.KpdError):
        utils.sampled_ligands_smiles([torch.randn(5, 3)], [torch.eye(5, 10)], ELEMENTS)
    with pytest.raises(ValueError):
        s.metrics(by='inchi')
    empty = molecule.build_molecules([], [], ELEMENTS)
    assert molecule.Sanitized(empty, {k: v[:0] for k, v in san.items()}, Z, True).smiles() == []
