"""Molecule building without a GPU: the tables of keypoint_diffusion_amd.molecule against upstream's settings
(tests/golden/allowed_bonds.json, make_molecule_golden.py), `Molecules.metrics` against upstream's formulas on hand-made
summaries, the entry points' declarations, and the refusal of CPU tensors.  The float64 restatement (tests/molecule_ref.py)
is checked here against the hand-derived textbook cases as well, so that the yardstick of the GPU test is itself pinned."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import hip, molecule, utils
from . import molecule_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ['kpd_mol_scratch_bytes', 'kpd_mol_perceive', 'kpd_sdf_scratch_bytes', 'kpd_sdf_emit']


def golden():
    with open(os.path.join(ROOT, 'tests', 'golden', 'allowed_bonds.json')) as f:
        return json.load(f)


def test_entry_points_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'kpd.h')).read()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for s in SYMBOLS:
        assert s + '(' in header and s in hip.EXPORTS and hasattr(lib, s), s
    L = hip.lib()
    assert L.kpd_mol_scratch_bytes(1000, 4) >= 1000 * 36 and L.kpd_mol_scratch_bytes(-1, 4) == -1
    assert L.kpd_sdf_scratch_bytes(1000, 4) > 0 and L.kpd_sdf_scratch_bytes(1, -1) == -1
    for name in ('build_molecules', 'Molecules', 'analyze_samples', 'ALLOWED_BONDS', 'ATOMIC_NUMBERS'):
        assert hasattr(molecule, name), name
    assert hasattr(utils, 'sampled_ligands_sdf') and hasattr(utils, 'write_sdf_file')
    for cite in ('analysis/molecule_builder.py:38-60', 'analysis/metrics.py:156-206', 'sample.py'):
        assert cite in header, cite


def test_default_allowed_bonds_are_upstreams_maxima():
    up = golden()['allowed_bonds']
    assert len(up) >= 14
    for el, v in up.items():
        if el in molecule.ALLOWED_BONDS:
            assert molecule.ALLOWED_BONDS[el] == (v if isinstance(v, int) else max(v)), el
    for el in ('C', 'N', 'O', 'S', 'P', 'F', 'Cl', 'Br', 'I', 'B'):
        assert el in up and el in molecule.ALLOWED_BONDS, el
    # the lists pass through as upstream reads them (metrics.py:180-183)
    assert molecule._class_tables(['P', 'S', 'Xx'], up) == ([15, 16, 0], [5, 4, 0])


def test_symbol_map_covers_every_shipped_configuration():
    files = golden()['lig_elements']
    assert len(files) == 9
    for name, elements in files.items():
        assert elements, name
        for el in elements:
            assert molecule.ATOMIC_NUMBERS.get(el, 0) in R.TABLE, (name, el)        # known to the map and to the bond rule
            assert el in molecule.ALLOWED_BONDS, (name, el)
    # the restatement's element table is the one include/kpd.h prints
    header = ' '.join(open(os.path.join(ROOT, 'include', 'kpd.h')).read().replace('*', ' ').split())
    for el, z in molecule.ATOMIC_NUMBERS.items():
        if z in R.TABLE:
            r1, r2, r3, cap = R.TABLE[z]
            assert f'{el} {z}: {r1} {r2} {r3} {cap}' in header, el


def molecules_of(sizes, largest, invalid, status=None, elem=None):
    ptr = torch.tensor([0] + list(sizes), dtype=torch.int64).cumsum(0).to(torch.int32)
    summary = torch.zeros(len(sizes), 4, dtype=torch.int32)
    summary[:, 2] = torch.tensor(largest, dtype=torch.int32)
    summary[:, 3] = torch.tensor(invalid, dtype=torch.int32)
    st = torch.zeros(len(sizes), dtype=torch.int32) if status is None else torch.tensor(status, dtype=torch.int32)
    return molecule.Molecules(ptr, summary, st, elem=elem)


def test_metrics_reproduce_upstreams_formulas_on_the_cpu():
    # metrics.py:156-206 by hand: 3 ligands of 10, 6, 4 atoms; largest fragments 10, 3, 1; isolated / over-valent atoms 0, 2, 3
    m = molecules_of([10, 6, 4], [10, 3, 1], [0, 2, 3]).metrics()
    assert set(m) == {'atom_validity', 'avg_frag_frac', 'connectivity'}
    assert m['atom_validity'] == 1 - 5 / 20
    assert m['avg_frag_frac'] == pytest.approx((1.0 + 0.5 + 0.25) / 3, rel=1e-15)
    assert m['connectivity'] == pytest.approx(2 / 3, rel=1e-15)                       # 3 / 6 >= 0.5: the threshold is inclusive
    assert molecules_of([6], [3], [0]).metrics()['connectivity'] == 1.0
    assert molecules_of([7], [3], [0]).metrics()['connectivity'] == 0.0
    assert molecules_of([7], [3], [0]).metrics(connectivity_thresh=3 / 7)['connectivity'] == 1.0
    # isolated atoms lower atom_validity
    assert molecules_of([5], [5], [0]).metrics()['atom_validity'] == 1.0
    assert molecules_of([5], [4], [1]).metrics()['atom_validity'] == pytest.approx(0.8, rel=1e-15)
    # empty batches, and batches of which nothing is left, give upstream's 0.0
    assert molecules_of([], [], []).metrics() == dict(atom_validity=0.0, avg_frag_frac=0.0, connectivity=0.0)
    assert molecules_of([0, 300], [0, 0], [0, 0], status=[1, 8]).metrics() == dict(atom_validity=0.0, avg_frag_frac=0.0, connectivity=0.0)
    # a ligand that was left out does not count
    assert molecules_of([4, 300], [4, 0], [0, 0], status=[0, 8]).metrics() == dict(atom_validity=1.0, avg_frag_frac=1.0, connectivity=1.0)


def test_atom_type_kl_divergence_by_hand():
    # LigandTypeDistribution.kl_divergence (metrics.py:225-236): p from the training counts, q from the sampled classes
    counts = torch.tensor([6, 3, 1])
    elem = torch.tensor([0, 0, 1, 1, 1, 0, 0, 0], dtype=torch.int32)                  # q = 5/8, 3/8, 0
    m = molecules_of([8], [8], [0], elem=elem).metrics(type_counts=counts)
    eps = 1e-10
    p, q = [0.6, 0.3, 0.1], [5 / 8, 3 / 8, 0.0]
    want = -sum(pi * math.log(qi / (pi + eps) + eps) for pi, qi in zip(p, q))
    assert want > 2.0                                                                 # the class that was never sampled dominates
    assert m['atom_type_kldiv'] == pytest.approx(want, rel=1e-12)
    same = molecules_of([10], [10], [0], elem=torch.tensor([0] * 6 + [1] * 3 + [2], dtype=torch.int32)).metrics(type_counts=counts)
    assert abs(same['atom_type_kldiv']) < 1e-8                                        # q == p: zero up to EPS
    with pytest.raises(ValueError):
        molecules_of([8], [8], [0], elem=elem).metrics(type_counts=torch.tensor([7]))


def test_wrappers_refuse_cpu_tensors():
    pos, feat = [torch.randn(5, 3)], [torch.eye(5, 10)]
    elements = ['C', 'N', 'O', 'S', 'P', 'F', 'Cl', 'Br', 'I', 'B']
    with pytest.raises(hip.KpdError):
        utils.sampled_ligands_xyz(pos, feat, elements)
    with pytest.raises(hip.KpdError):
        molecule.build_molecules(pos, feat, elements)
    with pytest.raises(hip.KpdError):
        utils.sampled_ligands_sdf(pos, feat, elements)
    with pytest.raises(hip.KpdError):
        utils.write_sdf_file(os.devnull, pos, feat, elements)
    with pytest.raises(hip.KpdError):
        molecule.analyze_samples([{'positions': pos, 'features': feat}], elements)
    ptr = torch.tensor([0, 5], dtype=torch.int32)
    with pytest.raises(hip.KpdError):
        hip.mol_perceive(pos[0], feat[0], ptr, [6] * 10, [4] * 10)
    with pytest.raises(hip.KpdError):
        hip.sdf_emit(pos[0], ptr, elements, {})
    with pytest.raises(hip.KpdError):
        molecules_of([5], [5], [0]).sdf()


# ---- the restatement against chemistry written out by hand (the same cases test_molecule_gpu.py runs on the GPU) ----------
def test_restatement_on_the_textbook_fragments():
    from .molecule_cases import TEXTBOOK, ELEMENTS, Z, ALLOWED, one_hot
    assert len(TEXTBOOK) >= 10
    for name, symbols, pos, bonds in TEXTBOOK:
        m = R.perceive(pos, one_hot(symbols), Z, ALLOWED)
        got = {(int(i), int(j)): int(o) for (i, j), o in zip(m['bonds'], m['order'])}
        assert got == bonds, (name, got)
    name, symbols, pos, bonds = [c for c in TEXTBOOK if c[0] == 'dimethyl sulfone'][0]
    m = R.perceive(pos, one_hot(symbols), Z, ALLOWED)
    assert m['valence'][0] == 6 and m['summary'] == [4, 1, 5, 1]                      # S: valence 6 > allowed 4, the one invalid atom
