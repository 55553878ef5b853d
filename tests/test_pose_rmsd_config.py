"""The symmetry-corrected RMSD of include/kpd.h (kpd_pose_rmsd) without a GPU: the restatement of the rule (tests/pose_rmsd_ref.py)
against an independent brute force over every automorphism, the properties the rule promises, the node counts of the named
molecules, and the refusals of the Python surface."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import hip, molecule
from . import pose_rmsd_cases as PC
from . import pose_rmsd_ref as R
from . import smiles_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM = SC.NUMBERS


def graph_of(c, largest=False, skip_h=True, bond_label=None, atom_label=None):
    Zs = [NUM[s] for s in c['sym']]
    S = R.largest_fragment(c['frag']) if largest else list(range(len(Zs)))
    if skip_h:
        S = [a for a in S if Zs[a] != 1]
    return R.Graph(Zs, c['bonds'], bond_label, atom_label, S)


@pytest.fixture(scope='module')
def named():
    return PC.named()


def random_cases(limit=14):
    """The 700 seeded graphs of tests/smiles_cases.py (at most `limit` atoms: all of them) with seeded coordinates and their bond
    labels; the coordinates mean nothing, the brute force and the restatement see the same ones."""
    out = []
    for k, (Zs, _, _, sym, bonds, labels) in enumerate(SC.random_set()):
        if len(Zs) > limit:
            continue
        pos = np.random.default_rng(k).standard_normal((len(Zs), 3)).astype(np.float32) * 2.0
        out.append((PC.case(f'random {k}', sym, pos, bonds=bonds), labels))
    return out


def test_the_restatement_finds_the_minimum_over_every_automorphism(named):
    """best, bit for bit, on every case of at most 12 atoms in S and on the random set: the bound and the classes lose nothing."""
    checked = searches = 0
    for c, labels in [(c, None) for c in named] + random_cases():
        for skip_h, largest in ((True, False), (False, False), (True, True)):
            if labels is not None and (not skip_h or largest):
                continue
            for use_labels in ((False, True) if labels is not None else (False,)):
                g = graph_of(c, largest, skip_h, labels if use_labels else None)
                if not g.S or len(g.S) > 12:
                    continue
                autos = R.automorphisms(g)
                if c['group'] is not None and skip_h and not largest and labels is None:
                    assert len(autos) == c['group'], c['name']
                stack = PC.poses(c, 4 if labels is None else 2, seed=3)
                for Y in stack:
                    r = R.search(g, c['pos'], Y)
                    assert not r['hit'] and r['best'] == R.brute_best(g, c['pos'], Y, autos), c['name']
                    assert r['best'] <= r['s_id']
                    searches += 1
                checked += 1
    print(f'{checked} graphs, {searches} searches equal the brute force in every bit')
    assert checked >= 700


def test_an_automorphism_pose_has_rmsd_zero_and_a_trivial_group_has_the_plain_number(named):
    for c in named:
        if c['auto'] is None or c['auto'] == list(range(len(c['sym']))):
            continue
        g = graph_of(c, skip_h=False)
        r = R.search(g, c['pos'], PC.permuted_rows(c['pos'], c['auto']))
        assert r['best'] == 0.0 and r['s_id'] > 0.0, c['name']
        assert all(r['map'][a] == c['auto'][a] for a in g.S), c['name']         # distinct coordinates: the one map of cost 0
    ethanol = next(c for c in named if c['name'] == 'ethanol')
    g = graph_of(ethanol)
    for Y in PC.poses(ethanol, 5):
        r = R.search(g, ethanol['pos'], Y)
        assert r['best'] == r['s_id'] and r['map'] == {0: 0, 1: 1, 2: 2}


def test_benzene_rotated_by_one_position():
    c = PC.named()[3]
    assert c['name'] == 'benzene'
    r = R.search(graph_of(c), c['pos'], PC.permuted_rows(c['pos'], c['auto']))
    assert R.rms(r['best'], 6) == 0.0 and R.rms(r['s_id'], 6) > 1.0 and [r['map'][a] for a in range(6)] == c['auto']


def test_scopes():
    two = next(c for c in PC.named() if c['name'] == 'two ethanols and a chloride')
    swapped = PC.permuted_rows(two['pos'], two['auto'])
    whole = R.search(graph_of(two), two['pos'], swapped)
    assert whole['best'] == 0.0 and [whole['map'][a] for a in range(7)] == two['auto']
    first = graph_of(two, largest=True)
    assert first.S == [0, 1, 2]
    r = R.search(first, two['pos'], swapped)
    assert r['best'] == r['s_id'] > 0.0                                         # the other fragment is not there to swap with
    methane = next(c for c in PC.named() if c['name'] == 'methane with hydrogens')
    turned = PC.permuted_rows(methane['pos'], methane['auto'])
    assert R.search(graph_of(methane, skip_h=False), methane['pos'], turned)['best'] == 0.0
    heavy = graph_of(methane)
    assert heavy.S == [0] and R.search(heavy, methane['pos'], turned)['nodes'] == 1


def ring_labels(c):
    """(Kekule orders 2, 1, 2, 1, 2, 1 around the ring from the bond 0-1; 4 on every ring bond), 1 on every other bond."""
    ring = {frozenset((k, (k + 1) % 6)) for k in range(6)}
    kekule = [2 - (min(i, j) % 2 if {i, j} != {0, 5} else 1) if frozenset((i, j)) in ring else 1 for i, j in c['bonds']]
    assert sorted(kekule) == [1] * (len(c['bonds']) - 3) + [2] * 3
    return kekule, [4 if frozenset((i, j)) in ring else 1 for i, j in c['bonds']]


def test_labels_decide_the_group():
    """A mirror that passes through ring ATOMS (toluene, through atoms 0 and 3) swaps the two Kekule patterns, so Kekule orders
    as labels lose it and aromatic labels keep it.  The one mirror of o-xylene passes through the BONDS 0-1 and 3-4 and maps
    each Kekule pattern onto itself: there every labelling keeps it."""
    toluene = next(c for c in PC.named() if c['name'] == 'toluene')
    for c, kekule_keeps_it in ((toluene, False), (PC.o_xylene(), True)):
        mirrored = PC.permuted_rows(c['pos'], c['auto'])
        kekule, aromatic = ring_labels(c)
        assert R.search(graph_of(c), c['pos'], mirrored)['best'] == 0.0
        assert R.search(graph_of(c, bond_label=aromatic), c['pos'], mirrored)['best'] == 0.0
        r = R.search(graph_of(c, bond_label=kekule), c['pos'], mirrored)
        assert (r['best'] == 0.0) if kekule_keeps_it else (r['best'] == r['s_id'] > 0.0), c['name']


def test_renumbering_moves_the_value_by_rounding_only(named):
    """The summation order moves with the numbering, so equality is to 1e-12 relative, not to the bit: n <= 256 terms of one sign
    summed in fp64 differ by at most n ulp ~ 6e-14 relative between any two orders."""
    rng = np.random.default_rng(5)
    for c in named + PC.generated(8):
        g = graph_of(c)
        stack = PC.poses(c, 4, seed=1)
        for _ in range(2):
            d, p = PC.renumbered(c, rng)
            gd = graph_of(d)
            for Y in stack:
                Yd = np.empty_like(Y)
                Yd[p] = Y
                a, b = R.search(g, c['pos'], Y)['best'], R.search(gd, d['pos'], Yd)['best']
                assert abs(a - b) <= 1e-12 * max(a, b), c['name']


def test_a_tiny_budget_sets_the_bit_and_gives_an_upper_bound(named):
    for c in named:
        g = graph_of(c)
        if len(g.S) < 2:
            continue
        for Y in PC.poses(c, 3, seed=2):
            full = R.search(g, c['pos'], Y)
            for budget in (1, 5):
                cut = R.search(g, c['pos'], Y, max_nodes=budget)
                assert cut['hit'] == (full['nodes'] > budget) and cut['nodes'] == min(full['nodes'], budget + 1), c['name']
                assert full['best'] <= cut['best'] <= cut['s_id'] and (cut['hit'] or cut['best'] == full['best']), c['name']
    benzene = named[3]
    turned = PC.permuted_rows(benzene['pos'], benzene['auto'])
    cut = R.search(graph_of(benzene), benzene['pos'], turned, max_nodes=5)
    assert cut['hit'] and cut['nodes'] == 6 and cut['best'] == cut['s_id'] > 0.0          # six atoms need six nodes to reach cost 0


def test_node_counts_of_the_named_molecules_stay_below_the_default_budget(named):
    worst = 0
    for c in named + PC.big():
        for skip_h in (True, False):
            g = graph_of(c, skip_h=skip_h)
            counts = [R.search(g, c['pos'], Y)['nodes'] for Y in PC.poses(c, 6)]
            print(f"{c['name']:32s} skip_h={int(skip_h)} n={len(g.S):3d} nodes {counts}")
            worst = max(worst, max(counts))
    assert worst < R.DEFAULT_MAX_NODES


def test_entry_points_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'kpd.h')).read()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for s in ('kpd_pose_rmsd', 'kpd_pose_rmsd_scratch_bytes'):
        assert re.search(r'\b' + s + r'\s*\(', header) and hasattr(lib, s) and s in hip.EXPORTS
    L = hip.lib()
    assert 800 <= L.kpd_pose_rmsd_scratch_bytes(100, 1, 0) < 100 * 64 * 8                  # one stack of fp64 per search in flight
    assert L.kpd_pose_rmsd_scratch_bytes(100, 200, 0) >= 100 * 64 * 8 and L.kpd_pose_rmsd_scratch_bytes(100, 5, 1) >= 100 * 10 * 8
    assert L.kpd_pose_rmsd_scratch_bytes(100, 65, 1) == -1 and L.kpd_pose_rmsd_scratch_bytes(100, 0, 0) == -1
    assert L.kpd_pose_rmsd_scratch_bytes(-1, 1, 0) == -1 and L.kpd_pose_rmsd_scratch_bytes(0, 1, 0) > 0


def test_the_python_surface_refuses_host_tensors_and_too_many_poses():
    ptr = torch.tensor([0, 5], dtype=torch.int32)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    mol = dict(elem=i32(5), frag=i32(5), bonds=i32(15, 2), order=i32(15), bond_ptr=i32(2), status=i32(1))
    with pytest.raises(hip.KpdError):
        hip.pose_rmsd(ptr, [6] * 10, mol, torch.zeros(1, 5, 3), torch.zeros(5, 3))
    m = molecule.Molecules(ptr, i32(1, 4), i32(1), mol['elem'], i32(5), mol['frag'], mol['bonds'], mol['order'], mol['bond_ptr'],
                           torch.zeros(5, 3), ['C'] * 10)
    with pytest.raises(hip.KpdError, match='GPU'):
        m.pose_rmsd(torch.zeros(5, 3))
    with pytest.raises(hip.KpdError, match='GPU'):
        m.pose_rmsd([torch.zeros(2, 5, 3)], pairs=True)
    with pytest.raises(hip.KpdError, match='at most 64'):
        m.pose_rmsd(torch.zeros(65, 5, 3), pairs=True)
    with pytest.raises(hip.KpdError, match='at least 1'):
        m.pose_rmsd(torch.zeros(0, 5, 3))
    with pytest.raises(hip.KpdError):
        m.pose_rmsd(torch.zeros(5, 2))
    for cls, name in ((molecule.Relaxed, 'sym_rmsd'), (molecule.VinaMinimized, 'sym_rmsd'), (molecule.VinaDocked, 'sym_rmsd'),
                      (molecule.VinaDocked, 'mode_rmsd'), (molecule.VinaDocked, 'distinct_modes'), (molecule.Sanitized, 'pose_rmsd')):
        assert callable(getattr(cls, name))
