"""Keys, fingerprints and diversity without a GPU: the integer restatement of include/kpd.h (tests/molset_ref.py) against
what a key must do (equal under renumbering, different for graphs that are not isomorphic, ring sizes included), against
labelled-graph isomorphism on a seeded random set, and the declarations and refusals of the Python surface."""
import ctypes
import itertools
import os
import random

import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import hip, molecule
from . import molset_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, N, O = 6, 7, 8


def ring(n, at=0):
    return [(at + k, at + (k + 1) % n) for k in range(n)]


DECALIN = ring(10) + [(0, 5)]                                    # two fused six-rings
BICYCLOPENTYL = ring(5) + ring(5, 5) + [(0, 5)]                  # two five-rings joined by a bond: the same degrees everywhere


def permuted(Z, bonds, labels, rng):
    """The same graph with its atoms renumbered, its bonds shuffled and their ends swapped at random."""
    n = len(Z)
    p = list(range(n))
    rng.shuffle(p)
    Zp = [0] * n
    for a in range(n):
        Zp[p[a]] = Z[a]
    rows = [((p[i], p[j]) if rng.random() < 0.5 else (p[j], p[i]), l) for (i, j), l in zip(bonds, labels)]
    rng.shuffle(rows)
    return Zp, [r[0] for r in rows], [r[1] for r in rows], p


def random_graph(rng):
    """A connected molecule-like graph: 4-9 atoms of C / N / O, degree <= 4, bond labels 1 / 2."""
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


def test_mix_is_the_splitmix64_finaliser():
    # the first outputs of splitmix64 seeded with 0 (Vigna's reference implementation): mix of successive multiples of K1
    assert S.mix(S.K1) == 0xE220A8397B1DCDAF and S.mix(2 * S.K1 & S.MASK) == 0x6E789E6AA1B965F4
    assert S.K1 == 0x9E3779B97F4A7C15 and S.mix(0) == 0


def test_key_and_fingerprint_do_not_depend_on_the_numbering():
    rng = random.Random(5)
    for _ in range(40):
        Z, bonds, labels = random_graph(rng)
        want = S.graph_key(Z, bonds, labels)
        Zp, bp, lp, p = permuted(Z, bonds, labels, rng)
        got = S.graph_key(Zp, bp, lp)
        assert got['key'] == want['key'] and got['fp'] == want['fp']
        assert [got['inv'][p[a]] for a in range(len(Z))] == want['inv']
        assert any(want['fp']) and want['key'] != 0


def test_ring_sizes_are_told_apart():
    Z = [C] * 10
    a, b = S.graph_key(Z, DECALIN), S.graph_key(Z, BICYCLOPENTYL)
    assert sorted(np.bincount(np.array(DECALIN).flatten())) == sorted(np.bincount(np.array(BICYCLOPENTYL).flatten()))
    assert a['key'] != b['key']
    # cyclohexane against two cyclopropanes in one ligand, every atom in scope: equal degrees, equal counts
    assert S.graph_key([C] * 6, ring(6))['key'] != S.graph_key([C] * 6, ring(3) + ring(3, 3))['key']
    # the scope: the largest fragment alone is a cyclopropane
    assert S.graph_key([C] * 6, ring(3) + ring(3, 3), S=[0, 1, 2])['key'] == S.graph_key([C] * 3, ring(3))['key']
    assert S.graph_key([C] * 6, ring(3) + ring(3, 3), S=[0, 1, 2])['inv'][3:] == [0, 0, 0]


def test_bond_orders_count_only_on_request():
    ethane, ethene = S.graph_key([C, C], [(0, 1)], [1]), S.graph_key([C, C], [(0, 1)], [2])
    assert ethane['key'] != ethene['key'] and ethane['fp'] != ethene['fp']
    assert S.graph_key([C, C], [(0, 1)], None)['key'] == ethane['key']                     # with_orders = 0: every label is 1
    assert S.graph_key([C, C], [(0, 1)])['key'] != S.graph_key([C, O], [(0, 1)])['key']    # elements count
    assert S.graph_key([C, O], [(0, 1)])['key'] == S.graph_key([O, C], [(0, 1)])['key']


def test_fingerprints_share_the_bits_of_shared_substructures():
    ethanol = S.graph_key([C, C, O], [(0, 1), (1, 2)], radius=1, nbits=4096)
    propanol = S.graph_key([C, C, C, O], [(0, 1), (1, 2), (2, 3)], radius=1, nbits=4096)
    bits = lambda r: {32 * w + k for w, x in enumerate(r['fp']) for k in range(32) if x >> k & 1}
    shared = bits(ethanol) & bits(propanol)
    assert len(shared) >= 4                     # CH3, OH at radius 0 and 1, CH2 at radius 0 ...
    assert 0.0 < S.tanimoto_distance(ethanol['fp'], propanol['fp']) < 1.0
    assert len(bits(S.graph_key([C, C, O], [(0, 1), (1, 2)], radius=0, nbits=64))) == 3
    # the Tanimoto distance by hand
    assert S.tanimoto_distance([0b1110, 0], [0b0111, 1 << 31]) == 1.0 - 2 / 5
    assert S.tanimoto_distance([0, 0], [0, 0]) == 0.0 and S.tanimoto_distance([1, 0], [0, 1]) == 1.0
    d, n, st = S.diversity(np.array([[0b1110, 0], [0b0111, 1 << 31], [0, 0], [0, 0]]), [1, 1, 1, 1], [0, 2, 4, 9, 4])
    assert d.tolist() == [1.0 - 2 / 5, 0.0, 0.0, 0.0] and n.tolist() == [1, 1, 0, 0] and st.tolist() == [0, 0, 1, 1]


def test_key_equality_is_labelled_graph_isomorphism_on_a_random_set():
    nx = pytest.importorskip('networkx')
    from networkx.algorithms.isomorphism import categorical_edge_match, categorical_node_match
    rng = random.Random(1)
    graphs = [random_graph(rng) for _ in range(700)]
    classes = {}
    for Z, bonds, labels in graphs:
        G = nx.Graph()
        G.add_nodes_from((a, dict(z=z)) for a, z in enumerate(Z))
        G.add_edges_from((i, j, dict(l=l)) for (i, j), l in zip(bonds, labels))
        classes.setdefault((len(Z), tuple(sorted(Z)), len(bonds)), []).append((G, S.graph_key(Z, bonds, labels)['key']))
    pairs = same = wrong = 0
    nm, em = categorical_node_match('z', None), categorical_edge_match('l', None)
    for members in classes.values():
        for (G1, k1), (G2, k2) in itertools.combinations(members, 2):
            iso = nx.is_isomorphic(G1, G2, node_match=nm, edge_match=em)
            pairs += 1
            same += iso
            wrong += iso != (k1 == k2)
    print(f'{pairs} pairs of equal size, composition and bond count, {same} isomorphic, {wrong} disagreements')
    assert pairs >= 500 and same >= 10          # the set can show both kinds of error
    assert wrong == 0


def test_entry_points_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'kpd.h')).read()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for s in ('kpd_mol_keys', 'kpd_fp_diversity'):
        assert s + '(' in header and s in hip.EXPORTS and hasattr(lib, s), s
    for name in ('mol_keys', 'fp_diversity'):
        assert callable(getattr(hip, name)), name
    for name in ('keys', 'fingerprints', 'set_metrics'):
        assert callable(getattr(molecule.Molecules, name)), name
    assert callable(molecule.training_keys)
    for text in ('0x9E3779B97F4A7C15', '0xC2B2AE3D27D4EB4F', '0x165667B19E3779F9', '0xBF58476D1CE4E5B9', '0x94D049BB133111EB', '65535',
                 'analysis/metrics.py:135-147', 'analysis/metrics.py:263-277', 'no stereo'):
        assert text in header, text
    # invalid settings are refused before anything is launched
    L = hip.lib()
    for radius, nbits in ((5, 2048), (-1, 2048), (2, 32), (2, 8192), (2, 96)):
        assert L.kpd_mol_keys(None, 0, 0, None, 1, None, None, None, None, None, 0, None, 1, 1, radius, nbits, None, None, None, None, None) != 0
    assert L.kpd_fp_diversity(None, None, 0, 0, None, 0, None, None, None, None) != 0


def test_host_tensors_are_refused():
    ptr = torch.tensor([0, 5], dtype=torch.int32)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    mol = dict(elem=i32(5), frag=i32(5), bonds=i32(15, 2), order=i32(15), bond_ptr=i32(2), status=i32(1))
    with pytest.raises(hip.KpdError):
        hip.mol_keys(ptr, [6] * 10, mol)
    with pytest.raises(hip.KpdError):
        hip.fp_diversity(i32(2, 64), torch.ones(2, dtype=torch.bool), torch.tensor([0, 2], dtype=torch.int32))
    m = molecule.Molecules(ptr, i32(1, 4), i32(1), mol['elem'], i32(5), mol['frag'], mol['bonds'], mol['order'], mol['bond_ptr'],
                           torch.zeros(5, 3), ['C'] * 10)
    for call in (m.keys, m.fingerprints, m.set_metrics):
        with pytest.raises(hip.KpdError):
            call()
    with pytest.raises(hip.KpdError):
        molecule.Molecules(ptr, i32(1, 4), i32(1)).keys()               # no bond graph at all
    with pytest.raises(hip.KpdError):
        molecule.training_keys([torch.randn(5, 3)], [torch.eye(5, 10)], ['C', 'N', 'O', 'S', 'P', 'F', 'Cl', 'Br', 'I', 'B'])
    with pytest.raises(hip.KpdError):
        molecule.analyze_samples([{'positions': [torch.randn(5, 3)], 'features': [torch.eye(5, 10)]}], ['C'] * 10, set_metrics=True)


def test_an_empty_set_gives_upstreams_zeros():
    m = molecule.build_molecules([], [], ['C', 'N', 'O'])
    assert m.keys().shape == (0,) and m.fingerprints(nbits=64).shape == (0, 2)
    out = m.set_metrics(group_ptr=[0, 0], train_keys=torch.tensor([1, 2]))
    assert out.pop('diversity_per_group').tolist() == [0.0]
    assert out == dict(uniqueness=0.0, novelty=0.0, diversity=0.0, diversity_std=0.0)
    assert m.set_metrics() == dict(uniqueness=0.0)
