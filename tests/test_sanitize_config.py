"""The sanitisation rule of include/kpd.h as restated in tests/sanitize_ref.py, checked without a GPU: the named molecules of
tests/sanitize_cases.py read as chemistry, the fast matching (the kernel's algorithm) equals the exhaustive one (the definition),
the cycle walk equals brute force, the results that must not depend on the numbering of the atoms do not, and the generated
ligands meet the conditions the GPU tests lean on.  Per-atom hydrogen counts and the Kekule pattern MAY move under renumbering
(tautomers, and the lexicographic rule reads bond rows): they are deliberately not asserted there."""
import inspect

import numpy as np
import pytest

from keypoint_diffusion_amd import hip, molecule
from . import molecule_ref as R
from . import sanitize_cases as C
from . import sanitize_ref as SR
from .molecule_cases import ALLOWED, ELEMENTS, Z, one_hot


def run(sym, pos, **kw):
    pos = np.asarray(pos, dtype=np.float32)
    m = R.perceive(pos, one_hot(sym), Z, ALLOWED)
    return m, SR.sanitize(pos, m['elem'], m['frag'], m['bonds'], m['order'], Z, ALLOWED, C.MASS, C.MASS_H, **kw)


@pytest.fixture(scope='module')
def generated():
    ligs = C.generated(200)
    return [(sym, pos, plant) + run(sym, pos) for sym, pos, plant in ligs]


def flags(r, bit):
    return [a for a, f in enumerate(r['atom_flags']) if f & bit]


@pytest.mark.parametrize('case', C.TEXTBOOK, ids=[c[0] for c in C.TEXTBOOK])
def test_textbook_expectations(case):
    name, sym, pos, exp = case
    m, r = run(sym, pos)
    assert r['status'] == 0 and r['valid'] == exp['valid']
    doubles = sorted((int(i), int(j)) for (i, j), o in zip(m['bonds'], r['order_k']) if o == 2)
    if 'doubles' in exp:
        assert doubles == exp['doubles']
    if 'n_doubles' in exp:
        assert len(doubles) == exp['n_doubles']
    assert len(r['aromatic_cycles']) == exp['n_arom'] == r['desc_i'][6]
    if 'n_planar' in exp:
        assert len(r['planar_cycles']) == exp['n_planar']
    if 'h_all' in exp:
        assert r['atom_h'] == [exp['h_all']] * len(sym)
    for a, h in exp.get('h', {}).items():
        assert r['atom_h'][a] == h, a
    if 'donors' in exp:
        assert flags(r, SR.ATOM_DONOR) == exp['donors'] and flags(r, SR.ATOM_ACCEPTOR) == exp['acceptors']
        assert r['desc_i'][2] == len(exp['donors']) and r['desc_i'][3] == len(exp['acceptors'])
    assert flags(r, SR.ATOM_UNSATISFIED) == exp.get('unsatisfied', [])
    if exp.get('fused'):                            # every ring aromatic, and no hydrogen exactly on the fusion atoms
        assert len(r['cycles']) == exp['n_arom'] and all(f & SR.ATOM_AROMATIC for f in r['atom_flags'])
        deg = np.bincount(np.asarray(m['bonds']).flatten(), minlength=len(sym))
        assert r['atom_h'] == [0 if d == 3 else 1 for d in deg]
    for a in exp.get('not_in_g', []):
        assert a not in r['g_atoms']
    assert SR.sanitize(np.asarray(pos, dtype=np.float32), m['elem'], m['frag'], m['bonds'], m['order'], Z, ALLOWED, C.MASS, C.MASS_H,
                       matching=SR.matching_exhaustive, cycles=SR.cycles56_brute)['order_k'] == r['order_k']


def test_benzene_by_hand():
    for k in (0, 1):                                # 1.397 A reads as six singles, 1.38 A as six doubles repaired: one molecule after
        m, r = run(C.TEXTBOOK[k][1], C.TEXTBOOK[k][2])
        assert r['order_k'] == [2, 1, 1, 2, 1, 2] and r['bond_flags'] == [7] * 6 and r['valence_k'] == [4 - 1] * 6
        assert r['desc_i'] == [6, 6, 0, 0, 0, 1, 1, 6, 4, 1] and r['mw'] == 6 * 12.0 + 6 * C.MASS_H
    assert sorted(R.perceive(np.float32(C.TEXTBOOK[0][2]), one_hot(['C'] * 6), Z, ALLOWED)['order']) != \
        sorted(R.perceive(np.float32(C.TEXTBOOK[1][2]), one_hot(['C'] * 6), Z, ALLOWED)['order'])


def test_fast_matching_equals_exhaustive_and_cycles_equal_brute_force(generated):
    n_comp = 0
    for sym, pos, _, m, r in generated:
        slow = SR.sanitize(pos, m['elem'], m['frag'], m['bonds'], m['order'], Z, ALLOWED, C.MASS, C.MASS_H, matching=SR.matching_exhaustive,
                           cycles=SR.cycles56_brute)
        assert slow['cycles'] == r['cycles'] and slow['matched_rows'] == r['matched_rows'] and slow['desc_i'] == r['desc_i']
        n_comp += len(r['components'])
    assert n_comp >= 200
    rng = np.random.default_rng(5)                  # and on graphs chemistry does not make: odd rings, pendant atoms, mixed elements
    for _ in range(300):
        n = int(rng.integers(2, 11))
        pairs = [(u, v) for u in range(n) for v in range(u + 1, n) if rng.random() < 0.35]
        deg = [0] * n
        edges = []
        for u, v in pairs:
            if deg[u] < 3 and deg[v] < 3:
                deg[u] += 1
                deg[v] += 1
                edges.append((len(edges), u, v))
        rows = rng.permutation(len(edges))
        edges = [(int(rows[k]), u, v) for k, (_, u, v) in enumerate(edges)]
        carbon = {a: bool(rng.random() < 0.6) for a in range(n)}
        if edges:
            assert SR.matching_fast(edges, carbon) == SR.matching_exhaustive(edges, carbon), (edges, carbon)


def test_cycles_on_clouds_and_caps():
    from .test_molecule_gpu import random_batch
    most, planar, eligible = 0, 0, 0
    for feat, pos in random_batch():
        m = R.perceive(pos, feat, Z, ALLOWED)
        r = SR.sanitize(pos, m['elem'], m['frag'], m['bonds'], m['order'], Z, ALLOWED, C.MASS, C.MASS_H)
        nbrs = {a: [] for a in range(len(pos))}
        for i, j in m['bonds']:
            nbrs[int(i)].append(int(j))
            nbrs[int(j)].append(int(i))
        assert r['cycles'] == SR.cycles56_brute(nbrs)
        most, planar, eligible = max(most, len(r['cycles'])), planar + len(r['planar_cycles']), eligible + len(r['g_edges'])
    # the clouds never reach the ring cap and never exercise step 3: they are for steps 1 and 2 and for robustness only
    assert most <= 22 and planar <= 1 and eligible == 0
    for n_hex, status in ((64, 0), (65, SR.TOO_MANY_RINGS)):
        _, r = run(*C.flat_honeycomb(n_hex))
        assert r['status'] == status and r['desc_i'][9] == n_hex == r['desc_i'][5] and not r['g_edges'] and r['valid'] == (not status)
    _, r = run(*C.coronene())
    assert r['status'] == 0 and [len(v) for v in r['components'].values()] == [24] and r['desc_i'][6] == 7 and r['valid'] == 1
    _, r = run(*C.cyclopenta_pentacene())
    assert r['status'] == SR.COMPONENT_TOO_LARGE and [len(v) for v in r['components'].values()] == [25] and r['valid'] == 0
    assert r['order_k'] == [1] * 30 and len(flags(r, SR.ATOM_UNSATISFIED)) == 25


def test_generator_meets_its_conditions(generated):
    assert all(r['status'] == 0 for *_, r in generated)                                  # no cap bit on any generated ligand
    assert sum(r['desc_i'][6] > 0 for *_, r in generated) >= 0.9 * len(generated)        # an aromatic ring in at least 90 %
    invalid = sum(not r['valid'] for *_, r in generated)
    assert 0.05 * len(generated) <= invalid <= 0.5 * len(generated)                      # both branches of `valid`
    planted = [(plant, r) for _, _, plant, _, r in generated if plant]
    assert sum(not r['valid'] for _, r in planted) >= 0.9 * len(planted)
    assert any(flags(r, SR.ATOM_UNSATISFIED) for p, r in planted if p == 'cyclopentadienyl')
    assert any(flags(r, SR.ATOM_OVERVALENT) for p, r in planted if p == 'sulfone')


def test_invariance_under_renumbering(generated):
    rng = np.random.default_rng(11)
    for sym, pos, _, m, r in generated:
        perm = rng.permutation(len(sym))                # new atom k is old atom perm[k]
        m2, r2 = run([sym[i] for i in perm], pos[perm])
        old_of = {k: int(perm[k]) for k in range(len(sym))}
        assert {old_of[a] for a in r2['aromatic_atoms']} == set(r['aromatic_atoms'])
        rows = lambda mm, rr: {tuple(sorted((int(i), int(j)))) for row, (i, j) in enumerate(mm['bonds']) if row in rr['aromatic_rows']}
        assert {tuple(sorted((old_of[i], old_of[j]))) for i, j in rows(m2, r2)} == rows(m, r)
        assert r2['valid'] == r['valid'] and r2['desc_i'] == r['desc_i'] and r2['mw'] == r['mw'] and r2['status'] == r['status']
        # NOT asserted: atom_h per atom and order_k per bond (which N of an imidazole carries the H follows the bond rows)


def test_largest_only_scope():
    sym = ['C'] * 6 + ['C', 'C', 'O']
    pos = np.concatenate([C.TEXTBOOK[0][2], np.array([[8.0, 0, 0], [9.52, 0, 0], [10.2, 1.25, 0]])]).astype(np.float32)
    m, r = run(sym, pos, largest_only=True)
    assert r['valence_k'][6:] == [-1, -1, -1] and r['desc_i'][:2] == [6, 6] and r['desc_i'][5] == 1
    m, r = run(sym, pos)
    assert r['desc_i'][0] == 9 and r['desc_i'][5] == 1 and min(r['valence_k']) >= 1


def test_vina_types_from_hydrogen_counts():
    _, sym, pos, _ = C.TEXTBOOK[5]                  # imidazole: N0 acceptor, N2 donor; carbons keep the rule of kpd_vina_score
    m, r = run(sym, pos)
    assert SR.vina_types([Z[e] for e in m['elem']], r['atom_h'], r['atom_flags'], r['valence_k']) == [SR.VN_A, -1, SR.VN_D, -1, -1]
    _, sym, pos, _ = C.TEXTBOOK[14]                 # phenol: O-H is acceptor and donor
    m, r = run(sym, pos)
    assert SR.vina_types([Z[e] for e in m['elem']], r['atom_h'], r['atom_flags'], r['valence_k'])[6] == SR.VN_A | SR.VN_D


def test_python_surface_without_a_gpu():
    assert 'kpd_mol_sanitize' in hip.EXPORTS and hip.SAN_DESC_I == SR.DESC_I
    assert (hip.SAN_NO_MOLECULE, hip.SAN_TOO_MANY_RINGS, hip.SAN_COMPONENT_TOO_LARGE) == (SR.NO_MOLECULE, SR.TOO_MANY_RINGS, SR.COMPONENT_TOO_LARGE)
    assert (hip.SAN_ATOM_RING, hip.SAN_ATOM_AROMATIC, hip.SAN_ATOM_DONOR, hip.SAN_ATOM_ACCEPTOR, hip.SAN_ATOM_UNSATISFIED,
            hip.SAN_ATOM_OVERVALENT) == (SR.ATOM_RING, SR.ATOM_AROMATIC, SR.ATOM_DONOR, SR.ATOM_ACCEPTOR, SR.ATOM_UNSATISFIED, SR.ATOM_OVERVALENT)
    sig = inspect.signature(molecule.analyze_samples)
    assert sig.parameters['sanitize'].default is False and sig.parameters['set_metrics'].default is False
    assert inspect.signature(molecule.Molecules.set_metrics).parameters['valid_only'].default is False
    masses, mass_h = molecule.mass_table(ELEMENTS)
    assert masses == C.MASS and mass_h == C.MASS_H
    with pytest.raises(hip.KpdError):
        molecule.mass_table(['Xx'])
    import torch
    e = torch.zeros(0, dtype=torch.int32)
    host = molecule.Molecules(torch.zeros(2, dtype=torch.int32), e.reshape(0, 4), e, e, e, e, e.reshape(0, 2), e, torch.zeros(2, dtype=torch.int32),
                              torch.zeros(0, 3), ELEMENTS)
    with pytest.raises(hip.KpdError):
        host.sanitize()
