"""The hydrogen placement rule of include/kpd.h (kpd_mol_add_hs) on its float64 restatement (tests/hydrogens_ref.py): ideal
geometry on small molecules, the flat three-neighbour centre, re-perception and re-sanitisation of the hydrogenated molecules,
the 256-atom cap, the largest-fragment scope, and what of the Python surface needs no GPU."""
import inspect

import numpy as np
import pytest

from keypoint_diffusion_amd import hip, molecule, utils
from keypoint_diffusion_amd.hip import HS_GENERAL, HS_NO_MOLECULE, HS_NO_ROOM, HS_NONFINITE, HS_TOO_MANY_ATOMS     # the library's status bits
from . import hydrogens_cases as HC
from . import hydrogens_ref as HR
from . import sanitize_cases as SC
from . import sanitize_ref as SR
from .molecule_cases import Z
from .molecule_ref import TABLE


@pytest.fixture(scope='module')
def small():
    return HC.reference([(sym, p) for _, sym, p, _, _ in HC.SMALL])


@pytest.fixture(scope='module')
def textbook():
    return HC.reference([(sym, p) for _, sym, p, _ in SC.TEXTBOOK])


@pytest.fixture(scope='module')
def generated():
    return HC.reference([(sym, p) for sym, p, _ in SC.generated(48)])


def angle(a, b):
    return float(np.degrees(np.arccos(np.clip(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)), -1.0, 1.0))))


def test_small_molecules_have_ideal_geometry(small):
    _, ptr, mol, san, hyd = small
    assert not hyd['status'].any()                  # no molecule problem, and no atom uses the general rule
    for b, (name, sym, p, n_h, classes) in enumerate(HC.SMALL):
        lig, res, n = HC.ligand(hyd, b), hyd['mols'][b], len(sym)
        assert hyd['n_h'][b] == n_h and len(lig['pos']) == n + n_h and res['classes'] == classes, name
        assert not res['general'] and not res['coincident'], name
        assert np.array_equal(lig['pos'][:n], p) and lig['source'].tolist() == list(range(int(ptr[b]), int(ptr[b]) + n)) + [-1] * n_h, name
        assert lig['parent'][n:].tolist() == sorted(lig['parent'][n:].tolist()), name          # grouped by parent, ascending
        pos = lig['pos'].astype(np.float64)
        nbrs = {a: [] for a in range(n + n_h)}
        for i, j in lig['bonds']:
            nbrs[int(i)].append(int(j))
            nbrs[int(j)].append(int(i))
        for x in range(n, n + n_h):
            a = int(lig['parent'][x])
            L = HR.bond_length(Z[int(lig['elem'][a])])
            assert abs(np.linalg.norm(pos[x] - pos[a]) - L) < 2e-6, (name, x)            # fp32 rounding of coordinates of a few A
            assert nbrs[x] == [a] and lig['valence'][x] == 1 and lig['elem'][x] == HC.H_CLASS, (name, x)
        for a, cls in classes.items():
            hs_of = [x for x in nbrs[a] if x >= n]
            for x in hs_of:
                for y in nbrs[a]:
                    if y != x:
                        assert abs(angle(pos[x] - pos[a], pos[y] - pos[a]) - HC.IDEAL[cls]) < 0.01, (name, a, x, y)
    # the first methyl hydrogen is anti to c: ethanol's C0 against O2, butane's C0 against C2
    for name, a, b_, c in (('ethanol', 0, 1, 2), ('butane', 0, 1, 2), ('acetamide', 3, 1, 0)):
        k = [s[0] for s in HC.SMALL].index(name)
        lig = HC.ligand(hyd, k)
        pos, n = lig['pos'].astype(np.float64), len(HC.SMALL[k][1])
        first = next(x for x in range(n, len(pos)) if lig['parent'][x] == a)
        axis = (pos[b_] - pos[a]) / np.linalg.norm(pos[b_] - pos[a])
        flat = lambda v: v - np.dot(v, axis) * axis
        assert abs(angle(flat(pos[first] - pos[a]), flat(pos[c] - pos[b_])) - 180.0) < 0.01, name


def test_bond_lengths_are_the_rest_lengths_of_relax():
    assert [HR.bond_length(zz) for zz in (6, 7, 8, 16)] == [(75 + 32) * 0.01, (71 + 32) * 0.01, (63 + 32) * 0.01, (103 + 32) * 0.01]
    assert TABLE[1][0] == HR.R_H


def test_flat_three_neighbour_centre_puts_its_hydrogen_on_the_normal():
    _, _, _, san, hyd = HC.reference([HC.FLAT])
    lig, res = HC.ligand(hyd, 0), hyd['mols'][0]
    assert san['atom_h'][0] == 1 and res['classes'][0] == HR.TET and not hyd['status'][0]
    pos = lig['pos'].astype(np.float64)
    h = next(x for x in range(4, len(pos)) if lig['parent'][x] == 0)
    normal = np.cross(pos[1] - pos[0], pos[2] - pos[0])
    assert angle(pos[h] - pos[0], normal) % 180.0 < 0.01 or angle(pos[h] - pos[0], normal) > 179.99
    assert min(np.linalg.norm(pos[h] - pos[k]) for k in (1, 2, 3)) >= 1.0


def same_bonds(lig):
    again = HC.reperceive(lig)
    return sorted(map(tuple, again['bonds'].tolist())) == sorted(map(tuple, np.asarray(lig['bonds']).tolist()))


def test_reperception_returns_the_bond_set(small, textbook, generated):
    for what, (_, _, _, _, hyd) in (('small', small), ('textbook', textbook)):
        for b in range(len(hyd['n_h'])):
            assert same_bonds(HC.ligand(hyd, b)), (what, b)
    hyd = generated[4]
    equal = sum(same_bonds(HC.ligand(hyd, b)) for b in range(48))
    print('generated ligands whose hydrogenated coordinates perceive to the same bonds:', equal, 'of 48')
    assert equal >= 40


def test_sanitising_the_hydrogenated_molecule_again(small, textbook, generated):
    n_checked = 0
    for what, (_, ptr, mol, san, hyd) in (('small', small), ('textbook', textbook), ('generated', generated)):
        for b, before in enumerate(san['mols']):
            lig = HC.ligand(hyd, b)
            after = HC.resanitize(lig)
            n = int(ptr[b + 1] - ptr[b])
            m = len(before['order_k'])
            assert after is not None and not any(after['atom_h']), (what, b)
            assert {a for a in after['aromatic_atoms']} == set(before['aromatic_atoms']), (what, b)
            heavy_rows = [r for r, (i, j) in enumerate(lig['bonds']) if j < n]
            assert len(heavy_rows) == m and [after['order_k'][r] for r in heavy_rows] == list(before['order_k']), (what, b)
            for name in ('n_heavy', 'n_rot', 'n_rings', 'n_arom_rings', 'n_arom_atoms', 'n_cycles'):
                k = SR.DESC_I.index(name)
                assert after['desc_i'][k] == before['desc_i'][k], (what, b, name)
            assert np.float64(after['mw']).view(np.int64) == np.float64(before['mw']).view(np.int64), (what, b)
            assert after['valid'] == 1 or before['valid'] == 0, (what, b)
            n_checked += 1
    assert n_checked == 22 + 18 + 48


def test_the_cap_of_256_atoms():
    _, _, _, san, hyd = HC.reference([HC.carbon_chain(84), HC.carbon_chain(85)])
    assert hyd['status'].tolist() == [0, HS_TOO_MANY_ATOMS] and hyd['n_h'].tolist() == [170, 0]
    assert hyd['out_ptr'].tolist() == [0, 254, 254 + 85] and hyd['out_bond_ptr'].tolist() == [0, 83 + 170, 83 + 170 + 84]
    tail = HC.ligand(hyd, 1)
    assert (tail['source'] >= 0).all() and tail['valence'].tolist() == [1] + [2] * 83 + [1]       # copied through: rows, bonds, no H
    assert hyd['summary'].tolist() == [[253, 1, 254, 0], [84, 1, 85, 0]]
    assert same_bonds(HC.ligand(hyd, 0))


def test_largest_fragment_scope():
    ethanol, methane = HC.SMALL[21], HC.SMALL[0]
    sym = ethanol[1] + methane[1]
    pos = np.concatenate([ethanol[2], methane[2] + np.float32(8.0)])
    _, _, _, _, hyd = HC.reference([(sym, pos)], largest=True)
    lig = HC.ligand(hyd, 0)
    assert hyd['n_h'].tolist() == [6] and sorted(set(lig['parent'][4:].tolist())) == [0, 1, 2]
    assert lig['valence'][:4].tolist() == [4, 4, 2, -1] and hyd['summary'][0].tolist() == [2 + 6, 2, 9, 0]
    _, _, _, _, every = HC.reference([(sym, pos)], largest=False)
    assert every['n_h'].tolist() == [10] and every['summary'][0].tolist() == [2 + 10, 2, 9, 0]


def test_atom_h_out_of_range_and_hand_written_graphs_are_no_molecule():
    pos, ptr, mol, san, _ = HC.reference([(s, p) for _, s, p, _, _ in HC.SMALL[13:16]])
    for value in (5, -1):
        bad = dict(san, atom_h=san['atom_h'].copy())
        bad['atom_h'][int(ptr[1])] = value
        hyd = HR.add_hs_batch(pos, ptr, mol, bad, HC.Z_H, HC.ALLOWED_H, HC.H_CLASS)
        assert hyd['status'].tolist() == [0, HS_NO_MOLECULE, 0] and hyd['n_h'].tolist() == [8, 0, 6]
        assert hyd['summary'][1].tolist() == [3, 0, 0, 0] and (HC.ligand(hyd, 1)['source'] >= 0).all()
    swapped = dict(mol, bonds=mol['bonds'].copy())
    swapped['bonds'][[0, 1]] = swapped['bonds'][[1, 0]]             # rows out of (i, j) order
    assert HR.add_hs_batch(pos, ptr, swapped, san, HC.Z_H, HC.ALLOWED_H, HC.H_CLASS)['status'].tolist() == [HS_NO_MOLECULE, 0, 0]
    assert HR.add_hs_batch(pos, ptr, mol, san, HC.Z_H, HC.ALLOWED_H, 0)['status'].tolist() == [HS_NO_MOLECULE] * 3     # z[h_class] != 1


def test_python_surface_without_a_gpu():
    assert 'kpd_mol_add_hs' in hip.EXPORTS and 'kpd_mol_add_hs_scratch_bytes' in hip.EXPORTS
    assert (HS_NO_MOLECULE, HS_TOO_MANY_ATOMS, HS_NO_ROOM, HS_GENERAL, HS_NONFINITE) == (
        HR.NO_MOLECULE, HR.TOO_MANY_ATOMS, HR.NO_ROOM, HR.GENERAL, HR.NONFINITE)
    assert hip.lib().kpd_mol_add_hs_scratch_bytes(100, 7) >= 8 * (7 + 7 + 1) and hip.lib().kpd_mol_add_hs_scratch_bytes(-1, 0) == -1
    for fn in (molecule.relax_samples, utils.sampled_ligands_sdf, utils.write_sdf_file):
        assert inspect.signature(fn).parameters['add_hs'].default is False
    assert callable(molecule.hydrogenate_samples) and callable(molecule.Sanitized.add_hs)
    import torch
    mols = molecule.build_molecules([], [], ['C', 'N'])
    with pytest.raises(hip.KpdError):               # no coordinates, and nothing on a GPU
        mols.sanitize()
    p = torch.zeros(1, 3)
    with pytest.raises(hip.KpdError):
        hip.mol_add_hs(p, torch.zeros(2, dtype=torch.int32), [6, 1], [4, 1], 1, {}, {})
