"""Sanitisation of perceived ligands on the GPU (kpd_mol_sanitize, Molecules.sanitize) against the integer / float64 restatement
of the rule in include/kpd.h (tests/sanitize_ref.py).  Every comparison is exact equality: integers, `valid`, `status`, and mw
bit for bit.  The restatement runs on the bond graph the GPU perceived, so only the sanitisation is under test here.
Every raw call runs with canary bytes behind each output buffer."""
import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import hip, molecule
from . import sanitize_cases as C
from . import sanitize_ref as SR
from .molecule_cases import ALLOWED, ELEMENTS, Z, one_hot
from .test_molecule_gpu import Guarded, cloud, concat, perceive_gpu, random_batch

pytestmark = pytest.mark.gpu
INT_KEYS = ('order_k', 'bond_flags', 'valence_k', 'atom_h', 'atom_flags', 'desc_i', 'valid', 'status')


def sanitize_gpu(dev, pos, ptr, mol, largest=False, z=Z, allowed=ALLOWED, mass=C.MASS, mass_h=C.MASS_H):
    """kpd_mol_sanitize through the C ABI.  mol: elem / frag [N], bonds [cap,2], order [cap], bond_ptr [B+1], status [B] as
    integer numpy arrays.  Returns numpy outputs in the layout of sanitize_ref.sanitize_batch."""
    t = lambda a, dt=torch.int32: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    pos_d = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float32)).reshape(-1, 3).to(dev)
    ptr_d = t(np.asarray(ptr))
    N, B, cap = pos_d.shape[0], len(ptr) - 1, len(mol['order'])
    ins = [t(mol['elem']), t(mol['frag']), t(np.asarray(mol['bonds']).reshape(-1)), t(mol['order']), t(mol['bond_ptr']), t(mol['status'])]
    before = [x.clone() for x in ins + [pos_d, ptr_d]]
    zt, at = t(np.asarray(z)), t(np.asarray(allowed))
    mt = torch.tensor(mass, dtype=torch.float64, device=dev)
    g = Guarded(dev)
    sizes = dict(order_k=cap, bond_flags=cap, valence_k=N, atom_h=N, atom_flags=N, desc_i=10 * B, desc_f=2 * B, valid=B, status=B)
    o = {k: g.new(n, torch.float64 if k == 'desc_f' else torch.int32) for k, n in sizes.items()}
    hip.check(hip.lib().kpd_mol_sanitize(pos_d.data_ptr(), ptr_d.data_ptr(), N, B, ins[0].data_ptr(), len(z), zt.data_ptr(), at.data_ptr(),
                                         mt.data_ptr(), float(mass_h), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(),
                                         ins[4].data_ptr(), cap, ins[5].data_ptr(), int(largest), *[o[k].data_ptr() for k in sizes],
                                         torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    g.check()
    for x, y in zip(ins + [pos_d, ptr_d], before):                  # inputs are never written
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    out = {k: o[k][:n].cpu().numpy() for k, n in sizes.items()}
    out = {k: (v if k == 'desc_f' else v.astype(np.int64)) for k, v in out.items()}
    out['desc_i'], out['desc_f'] = out['desc_i'].reshape(B, 10), out['desc_f'].reshape(B, 2)
    return out


def mol_of(got):
    return dict(elem=got['elem'], frag=got['frag'], bonds=got['bonds'], order=got['order'], bond_ptr=got['bond_ptr'], status=got['status'])


def assert_same(got, ref, what=''):
    for k in INT_KEYS:
        bad = np.nonzero(np.asarray(got[k] != ref[k]).reshape(len(ref[k]), -1).any(axis=1))[0]
        assert bad.size == 0, (what, k, bad[:8], np.asarray(got[k])[bad[:4]], np.asarray(ref[k])[bad[:4]])
    assert np.array_equal(got['desc_f'].view(np.int64), ref['desc_f'].view(np.int64)), (what, 'desc_f')


def run_both(dev, ligs, largest=False, edit=None):
    """Perceive on the GPU, sanitise on the GPU and by the restatement.  `edit(mol, pos, ptr)` may change the graph in between."""
    pos, feat, ptr = concat(ligs)
    perceived, _ = perceive_gpu(dev, pos, feat, ptr)
    mol = mol_of(perceived)
    if edit is not None:
        pos, ptr = edit(mol, pos, ptr) or (pos, ptr)
    ref = SR.sanitize_batch(pos, ptr, mol, Z, ALLOWED, C.MASS, C.MASS_H, largest)
    return sanitize_gpu(dev, pos, ptr, mol, largest), ref, mol, pos, ptr


@pytest.fixture(scope='module')
def generated():
    return [(sym, pos) for sym, pos, _ in C.generated(150)]


# ---- 1. parity with the restatement ---------------------------------------------------------------------------------------------
def test_textbook_matches_and_reads_as_chemistry(cuda):
    got, ref, mol, _, ptr = run_both(cuda, [(sym, p) for _, sym, p, _ in C.TEXTBOOK])
    assert_same(got, ref, 'textbook')
    for b, (name, sym, _, exp) in enumerate(C.TEXTBOOK):
        a0, p0, p1 = int(ptr[b]), int(mol['bond_ptr'][b]), int(mol['bond_ptr'][b + 1])
        doubles = sorted((int(i - a0), int(j - a0)) for (i, j), o in zip(mol['bonds'][p0:p1], got['order_k'][p0:p1]) if o == 2)
        if 'doubles' in exp:
            assert doubles == exp['doubles'], name
        assert got['valid'][b] == exp['valid'] and got['desc_i'][b, 6] == exp['n_arom'], name
    by_name = {c[0]: b for b, c in enumerate(C.TEXTBOOK)}
    assert got['desc_i'][by_name['pyrene'], 6] == 4 and got['desc_i'][by_name['cyclohexane'], 1] == 12


def test_generated_ligands_match(cuda, generated):
    for largest in (False, True):
        got, ref, _, _, _ = run_both(cuda, generated, largest)
        assert_same(got, ref, f'generated, largest_only={largest}')
    assert (ref['desc_i'][:, 6] > 0).mean() >= 0.9 and 0.05 <= (ref['valid'] == 0).mean() <= 0.5 and not ref['status'].any()


def test_random_clouds_match_in_both_scopes(cuda):
    ligs = random_batch()
    for largest in (False, True):
        got, ref, _, _, _ = run_both(cuda, ligs, largest)
        assert_same(got, ref, f'clouds, largest_only={largest}')


def test_caps_sit_at_their_edges(cuda):
    ligs = [C.flat_honeycomb(64), C.flat_honeycomb(65), C.coronene(), C.cyclopenta_pentacene()]
    got, ref, _, _, _ = run_both(cuda, ligs)
    assert_same(got, ref, 'caps')
    assert got['status'].tolist() == [0, SR.TOO_MANY_RINGS, 0, SR.COMPONENT_TOO_LARGE] and got['valid'].tolist() == [1, 0, 1, 0]
    assert got['desc_i'][:, 9].tolist() == [64, 65, 7, 6] and got['desc_i'][:, 6].tolist() == [0, 0, 7, 0]


def test_sizes_left_out_and_bad_status_bits(cuda):
    rng = np.random.default_rng(7)
    ligs = [cloud(rng, n) for n in (1, 2, 5, 6, 63, 64, 65, 256, 257, 0)] + [(sym, p) for _, sym, p, _ in C.TEXTBOOK[:6]]

    def edit(mol, pos, ptr):                        # each bad bit of mol_status on a ligand of its own; bit 2 alone leaves it in
        for k, bit in enumerate((1, 2, 4, 8)):
            mol['status'][10 + k] |= bit
    got, ref, mol, _, _ = run_both(cuda, ligs, edit=edit)
    assert_same(got, ref, 'sizes')
    assert got['status'][8] == SR.NO_MOLECULE and got['status'][9] == SR.NO_MOLECULE and not got['status'][7] & SR.NO_MOLECULE
    assert got['status'][10:14].tolist() == [1, 1, 0, 1] and got['valid'][12] == 1


def test_malformed_segment_and_hand_written_graphs(cuda):
    ring = [(sym, p) for _, sym, p, _ in C.TEXTBOOK[:5]]

    def bad_ptr(mol, pos, ptr):                     # [-1, 6, 100000, 18, 23, 28]: ligand 0 starts below 0, ligand 1 ends beyond the
        ptr = np.array(ptr)                         # atoms, ligand 2 ends before it starts; ligands 3 and 4 stand, and no two
        ptr[0], ptr[2] = -1, 100000                 # accepted segments share an atom (kpd.h leaves such rows unspecified)
        return pos, ptr
    got, ref, _, _, _ = run_both(cuda, ring, edit=bad_ptr)
    assert_same(got, ref, 'malformed lig_ptr')
    assert got['status'].tolist() == [SR.NO_MOLECULE] * 3 + [0, 0] and got['valid'].tolist() == [0, 0, 0, 1, 1]
    assert (got['valence_k'][:18] == -1).all() and (got['valence_k'][18:] > 0).all()

    def graphs(mol, pos, ptr):                      # no output of perceive: a bond twice, order 0, a seventh neighbour, a bond leaving
        bp = mol['bond_ptr']
        mol['bonds'][bp[0] + 1] = mol['bonds'][bp[0]][::-1]
        mol['order'][bp[1]] = 0
        mol['bonds'][bp[3]] = [ptr[3], ptr[4] + 1]
    got, ref, _, _, _ = run_both(cuda, ring, edit=graphs)
    assert_same(got, ref, 'hand-written graphs')
    assert got['status'].tolist() == [1, 1, 0, 1, 0]
    # a seventh neighbour: a hub with seven spokes, written by hand
    sym, n = ['C'] * 8, 8
    pos = np.concatenate([np.zeros((1, 3)), 1.5 * np.eye(3), -1.5 * np.eye(3), [[1.0, 1.0, 1.0]]]).astype(np.float32)
    mol = dict(elem=np.zeros(n, dtype=np.int64), frag=np.zeros(n, dtype=np.int64), bonds=np.array([[0, k] for k in range(1, 8)]),
               order=np.ones(7, dtype=np.int64), bond_ptr=np.array([0, 7]), status=np.zeros(1, dtype=np.int64))
    ref = SR.sanitize_batch(pos, [0, n], mol, Z, ALLOWED, C.MASS, C.MASS_H)
    assert_same(sanitize_gpu(cuda, pos, [0, n], mol), ref, 'seventh neighbour')
    assert ref['status'].tolist() == [SR.NO_MOLECULE]
    mol['bonds'], mol['order'], mol['bond_ptr'] = mol['bonds'][:6], mol['order'][:6], np.array([0, 6])
    ref = SR.sanitize_batch(pos, [0, n], mol, Z, ALLOWED, C.MASS, C.MASS_H)
    assert_same(sanitize_gpu(cuda, pos, [0, n], mol), ref, 'six neighbours')
    assert ref['status'].tolist() == [0]


def test_nan_coordinate(cuda):
    ring = [(sym, p) for _, sym, p, _ in C.TEXTBOOK[:4]]

    def poison(mol, pos, ptr):                      # the graph of the clean rings, then a NaN and an Inf under it
        pos = np.array(pos)
        pos[ptr[0] + 2, 1] = np.nan
        pos[ptr[2], 0] = np.inf
        return pos, ptr
    got, ref, _, _, _ = run_both(cuda, ring, edit=poison)
    assert_same(got, ref, 'NaN under a clean graph')
    assert got['status'].tolist() == [0, 0, 0, 0] and got['desc_i'][:, 6].tolist() == [0, 1, 0, 1]
    pos = np.array(C.TEXTBOOK[0][2], dtype=np.float32)
    pos[3, 2] = np.nan                              # and through perception: the atom is never bonded
    got, ref, _, _, _ = run_both(cuda, [(C.TEXTBOOK[0][1], pos)])
    assert_same(got, ref, 'NaN through perception')


# ---- 2. independence of the batch and of the repeat ---------------------------------------------------------------------------------
def test_alone_in_a_batch_elsewhere_and_again(cuda, generated):
    pos, feat, ptr = concat(generated)
    perceived, _ = perceive_gpu(cuda, pos, feat, ptr)
    mol = mol_of(perceived)
    whole = sanitize_gpu(cuda, pos, ptr, mol)
    again = sanitize_gpu(cuda, pos, ptr, mol)
    for k in INT_KEYS + ('desc_f',):
        assert np.array_equal(whole[k], again[k], equal_nan=True), k
    rev = list(reversed(generated))
    pos_r, feat_r, ptr_r = concat(rev)
    perceived_r, _ = perceive_gpu(cuda, pos_r, feat_r, ptr_r)
    turned = sanitize_gpu(cuda, pos_r, ptr_r, mol_of(perceived_r))
    B = len(generated)
    for b in (0, 17, 76, B - 1):
        one_pos, one_feat, one_ptr = concat([generated[b]])
        one_perceived, _ = perceive_gpu(cuda, one_pos, one_feat, one_ptr)
        alone = sanitize_gpu(cuda, one_pos, one_ptr, mol_of(one_perceived))
        a0, a1, p0, p1 = int(ptr[b]), int(ptr[b + 1]), int(mol['bond_ptr'][b]), int(mol['bond_ptr'][b + 1])
        r = B - 1 - b
        ra0, rp0 = int(ptr_r[r]), int(perceived_r['bond_ptr'][r])
        for k in ('valence_k', 'atom_h', 'atom_flags'):
            assert np.array_equal(whole[k][a0:a1], alone[k][:a1 - a0]) and np.array_equal(whole[k][a0:a1], turned[k][ra0:ra0 + a1 - a0]), (b, k)
        for k in ('order_k', 'bond_flags'):
            assert np.array_equal(whole[k][p0:p1], alone[k][:p1 - p0]) and np.array_equal(whole[k][p0:p1], turned[k][rp0:rp0 + p1 - p0]), (b, k)
        for k in ('desc_i', 'desc_f', 'valid', 'status'):
            assert np.array_equal(whole[k][b], alone[k][0]) and np.array_equal(whole[k][b], turned[k][r]), (b, k)


# ---- 3. the Python surface -------------------------------------------------------------------------------------------------------
def build(dev, ligs):
    return molecule.build_molecules([torch.from_numpy(np.asarray(p, dtype=np.float32)).to(dev) for _, p in ligs],
                                    [torch.from_numpy(one_hot(sym)).to(dev) for sym, _ in ligs], ELEMENTS)


def test_sanitized_molecules_sdf_and_keys(cuda):
    b1, b2 = C.TEXTBOOK[0], C.TEXTBOOK[1]           # benzene at 1.397 A and at 1.38 A
    mols = build(cuda, [(b1[1], b1[2]), (b2[1], b2[2])])
    raw = mols.keys(with_orders=True)
    assert raw[0] != raw[1]                         # the length classes split one molecule: six singles against six doubles repaired
    s = mols.sanitize()
    keys = s.molecules.keys(with_orders=True)
    assert keys[0] == keys[1] and s.valid.tolist() == [True, True]
    for block in s.molecules.sdf():
        bond_lines = block.splitlines()[4 + 6:4 + 12]
        assert sorted(line[6:9] for line in bond_lines) == ['  1'] * 3 + ['  2'] * 3
    assert s.h.tolist() == [1] * 12 and bool(s.aromatic_atoms.all()) and int(s.aromatic_bonds.sum()) == 12
    d = s.descriptors()
    assert d['n_arom_rings'].tolist() == [1, 1] and d['mw'].tolist() == [6 * 12.0 + 6 * molecule.MONOISOTOPIC_MASS['H']] * 2
    assert s.table()['lig_idx'] == [0, 1]
    met = s.metrics()
    assert met['validity'] == 1.0 and met['connectivity'] == 1.0 and met['uniqueness'] == 0.5 and met['hbd_mean'] == 0.0
    bad = build(cuda, [(C.TEXTBOOK[6][1], C.TEXTBOOK[6][2]), (b1[1], b1[2])]).sanitize()       # cyclopentadienyl is not valid
    assert bad.valid.tolist() == [False, True] and bad.metrics()['validity'] == 0.5


def test_vina_types_tell_the_two_nitrogens_of_imidazole_apart(cuda):
    _, sym, p, _ = C.TEXTBOOK[5]                    # N0 takes no hydrogen (acceptor), N2 is the N-H (donor)
    mols = build(cuda, [(sym, p)] * 4)
    s = mols.sanitize()
    types = s.vina_types()
    assert types.tolist() == [4, -1, 2, -1, -1] * 4
    out = lambda a: torch.from_numpy((np.asarray(p[a]) * (1.0 + 3.0 / np.linalg.norm(p[a]))).astype(np.float32)).reshape(1, 3).to(cuda)
    pockets = [out(0), out(0), out(2), out(2)]      # a pocket atom 3 A outside N0 (twice) and outside N2 (twice) ...
    pocket_types = [[2], [4], [4], [2]]             # ... a donor, an acceptor, an acceptor, a donor
    sc = s.molecules.vina_score(pockets, [['N']] * 4, pocket_of=[0, 1, 2, 3], pocket_types=pocket_types, lig_types=types, radii={'B': 1.9})
    hb = sc.report[:, hip.VINA_REPORT.index('hbond')].tolist()
    assert hb[0] != 0.0 and hb[1] == 0.0 and hb[2] != 0.0 and hb[3] == 0.0
    plain = mols.vina_score(pockets, [['N']] * 4, pocket_of=[0, 1, 2, 3], pocket_types=pocket_types, radii={'B': 1.9})
    assert plain.report[0, hip.VINA_REPORT.index('hbond')].item() == 0.0      # without hydrogen counts both N are donors


def test_host_tensor_raises(cuda):
    _, sym, p, _ = C.TEXTBOOK[0]
    mols = build(cuda, [(sym, p)])
    mols.pos = mols.pos.cpu()
    with pytest.raises(hip.KpdError):
        mols.sanitize()
    with pytest.raises(hip.KpdError):
        hip.mol_sanitize(mols.pos, mols.lig_ptr, Z, ALLOWED, C.MASS, C.MASS_H,
                         dict(elem=mols.elem, frag=mols.frag, bonds=mols.bonds, order=mols.order, bond_ptr=mols.bond_ptr, status=mols.status))


def test_analyze_samples_keeps_its_keys_and_adds_the_sanitised_numbers(cuda):
    ligs = [(C.TEXTBOOK[k][1], C.TEXTBOOK[k][2]) for k in (0, 1, 6, 14)]      # two benzenes, cyclopentadienyl, phenol
    samples = [dict(positions=[torch.from_numpy(np.asarray(p, dtype=np.float32)) for _, p in ligs[:2]],
                    features=[torch.from_numpy(one_hot(sym)) for sym, _ in ligs[:2]]),
               dict(positions=[torch.from_numpy(np.asarray(p, dtype=np.float32)) for _, p in ligs[2:]],
                    features=[torch.from_numpy(one_hot(sym)) for sym, _ in ligs[2:]])]
    plain = molecule.analyze_samples(samples, ELEMENTS, device=cuda)
    assert plain == build(cuda, ligs).metrics() and sorted(plain) == ['atom_validity', 'avg_frag_frac', 'connectivity']
    out = molecule.analyze_samples(samples, ELEMENTS, device=cuda, sanitize=True)
    assert {k: out[k] for k in plain if k != 'connectivity'} == {k: plain[k] for k in plain if k != 'connectivity'}
    assert out['validity'] == 0.75 and out['connectivity'] == 1.0 and out['uniqueness'] == 2 / 3 and 'diversity' in out
    assert out['hbd_mean'] == 1 / 3 and out['lipinski4_mean'] == 4.0 and out['mw_std'] > 0.0
