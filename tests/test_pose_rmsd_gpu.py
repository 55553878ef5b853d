"""Symmetry-corrected RMSD between poses on the GPU (kpd_pose_rmsd and the methods on it) against the restatement of the rule in
include/kpd.h (tests/pose_rmsd_ref.py), bit for bit: every rmsd, plain, nodes, map and status.  The graphs are fed as
kpd_mol_perceive would have left them, so only the search is under test.  Every raw call runs with canary bytes behind each output
buffer and around the scratch, and checks that no input was written.  The restatement is computed once, for 65 poses and for
the pairs of 5: a ligand's result does not depend on K, so the smaller K are its first columns."""
import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import hip, molecule
from . import pose_rmsd_cases as PC
from . import pose_rmsd_ref as R
from .molecule_cases import ELEMENTS, one_hot
from .relax_cases import grow, make_pocket
from .test_molecule_gpu import CANARY, Guarded
from .util import guarded, intact
from .vina_cases import RADII

pytestmark = pytest.mark.gpu
K_MANY, K_PAIRS = 65, 5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def arrays(cases, cap_bonds=None):
    """Cases -> (ptr, mol) as kpd_mol_perceive would have left them, and the reference pose [N,3]."""
    ptr, elem, frag, bonds, bond_ptr = [0], [], [], [], [0]
    for c in cases:
        a0 = ptr[-1]
        elem += [PC.ELEMENTS_ALL.index(s) for s in c['sym']]
        frag += list(c['frag'])
        bonds += [(a0 + i, a0 + j) for i, j in c['bonds']]
        ptr.append(a0 + len(c['sym']))
        bond_ptr.append(len(bonds))
    cap = len(bonds) if cap_bonds is None else cap_bonds
    i64 = lambda x: np.asarray(x, dtype=np.int64)
    mol = dict(elem=i64(elem), frag=i64(frag), bonds=i64(bonds + [(0, 0)] * (cap - len(bonds))).reshape(-1, 2), bond_ptr=i64(bond_ptr),
               status=np.zeros(len(cases), dtype=np.int64))
    ref = np.concatenate([c['pos'] for c in cases]) if cases else np.zeros((0, 3), dtype=np.float32)
    return i64(ptr), mol, ref.astype(np.float32)


def stack(cases, K, seed=0):
    return np.concatenate([PC.poses(c, K, seed) for c in cases], axis=1) if cases else np.zeros((K, 0, 3), dtype=np.float32)


def rmsd_gpu(dev, ptr, mol, pos, ref=None, pairs=False, largest=False, skip_h=True, max_nodes=R.DEFAULT_MAX_NODES, bond_label=None,
             atom_label=None, want_map=True, z=PC.Z_ALL):
    """kpd_pose_rmsd through the C ABI; returns numpy arrays in the shapes of pose_rmsd_ref.pose_rmsd_batch."""
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.int32).to(dev)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    K, N, B, cap = pos.shape[0], pos.shape[1], len(ptr) - 1, len(mol['bonds'])
    ins = [i32(ptr), i32(mol['elem']), i32(np.asarray(z)), i32(mol['frag']), i32(np.asarray(mol['bonds']).reshape(-1)), i32(mol['bond_ptr']),
           i32(mol['status']), f32(pos)]
    opt = [None if x is None else (f32(x) if k == 2 else i32(x)) for k, x in enumerate((bond_label, atom_label, ref))]
    before = [x.clone() for x in ins] + [None if x is None else x.clone() for x in opt]
    per = K * K if pairs else K
    g = Guarded(dev)
    rmsd, plain, nodes, status = g.new(B * per, torch.float64), g.new(B * per, torch.float64), g.new(B * per, torch.int64), g.new(B)
    amap = g.new(K * N) if want_map and not pairs else None
    L = hip.lib()
    nb = int(L.kpd_pose_rmsd_scratch_bytes(N, K, int(pairs)))
    assert nb > 0
    scratch, p_scr = guarded(nb, torch.uint8, dev, CANARY)
    p = [x.data_ptr() for x in ins]
    q = [None if x is None else x.data_ptr() for x in opt]
    hip.check(L.kpd_pose_rmsd(p[0], N, B, p[1], len(z), p[2], p[3], p[4], p[5], cap, p[6], q[0], q[1], int(largest), int(skip_h), q[2],
                              p[7], K, int(pairs), int(max_nodes), rmsd.data_ptr(), plain.data_ptr(), None if amap is None else amap.data_ptr(),
                              nodes.data_ptr(), status.data_ptr(), p_scr, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    g.check()
    assert intact(scratch, nb, CANARY), f'kpd_pose_rmsd wrote outside its {nb} bytes of scratch'
    for x, y in zip(ins + opt, before):             # inputs are never written (compared as bits: a pose may hold a NaN)
        assert x is None or torch.equal(x.view(torch.int32), y.view(torch.int32))
    shape = (B, K, K) if pairs else (B, K)
    return dict(rmsd=rmsd[:B * per].cpu().numpy().reshape(shape), plain=plain[:B * per].cpu().numpy().reshape(shape),
                nodes=nodes[:B * per].cpu().numpy().reshape(shape), status=status[:B].cpu().numpy().astype(np.int64),
                map=None if amap is None else amap[:K * N].cpu().numpy().astype(np.int64).reshape(K, N))


def assert_same(got, ref, what='', poses=None):
    """Every bit of every output; `poses`: compare with the first columns of a reference computed for more poses."""
    sub = (lambda a: a) if poses is None else (lambda a: a[:, :poses, :poses] if a.ndim == 3 else a[:, :poses])
    assert got['status'].tolist() == ref['status'].tolist(), (what, 'status')
    for k in ('rmsd', 'plain'):
        assert np.array_equal(bits(got[k]), bits(sub(ref[k]))), (what, k, np.argwhere(bits(got[k]) != bits(sub(ref[k])))[:4])
    assert np.array_equal(got['nodes'], sub(ref['nodes'])), (what, 'nodes', np.argwhere(got['nodes'] != sub(ref['nodes']))[:4])
    if got['map'] is not None:
        want = ref['map'] if poses is None else ref['map'][:poses]
        assert np.array_equal(got['map'], want), (what, 'map', np.argwhere(got['map'] != want)[:4])


# ---- the cases and their restatement, computed once ----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def world():
    cases = PC.all_cases()
    ptr, mol, ref_pos = arrays(cases)
    many, five = stack(cases, K_MANY), stack(cases, K_PAIRS, seed=1)
    out = dict(cases=cases, ptr=ptr, mol=mol, ref_pos=ref_pos, many=many, five=five)
    for skip_h in (True, False):
        out['ref', skip_h] = R.pose_rmsd_batch(ptr, mol, PC.Z_ALL, many, ref_pos, skip_h=skip_h)
    out['pairs'] = R.pose_rmsd_batch(ptr, mol, PC.Z_ALL, five, pairs=True)
    return out


@pytest.mark.parametrize('K', [1, 3, K_MANY])
def test_every_bit_equals_the_restatement(cuda, world, K):
    for skip_h in (True, False):
        got = rmsd_gpu(cuda, world['ptr'], world['mol'], world['many'][:K], world['ref_pos'], skip_h=skip_h)
        assert_same(got, world['ref', skip_h], f'K={K} skip_h={skip_h}', poses=K)
        assert not got['status'].any() and (got['rmsd'] <= got['plain']).all() and (got['nodes'] >= 1).all()
    ref = world['ref', True]
    assert (ref['nodes'] < R.DEFAULT_MAX_NODES).all() and (ref['rmsd'] < ref['plain']).sum() > 40        # the symmetry shows


@pytest.mark.parametrize('K', [2, K_PAIRS])
def test_pairs_equal_the_restatement(cuda, world, K):
    got = rmsd_gpu(cuda, world['ptr'], world['mol'], world['five'][:K], pairs=True)
    assert_same(got, world['pairs'], f'pairs K={K}', poses=K)
    for k in ('rmsd', 'plain', 'nodes'):
        assert np.array_equal(got[k], got[k].transpose(0, 2, 1)) and not got[k][:, np.arange(K), np.arange(K)].any()
    one = rmsd_gpu(cuda, world['ptr'], world['mol'], world['five'][:1], pairs=True)                 # K = 1: nothing but the diagonal
    assert not one['status'].any() and not one['rmsd'].any() and not one['nodes'].any()


# ---- named behaviour -----------------------------------------------------------------------------------------------------------------
def named(name):
    return next(c for c in PC.named() if c['name'] == name)


def test_benzene_rotated_by_one_position(cuda):
    c = named('benzene')
    ptr, mol, ref = arrays([c])
    got = rmsd_gpu(cuda, ptr, mol, PC.permuted_rows(c['pos'], c['auto'])[None], ref)
    assert got['rmsd'][0, 0] == 0.0 and got['plain'][0, 0] > 1.0 and got['map'][0].tolist() == c['auto'] and got['status'][0] == 0


def test_fragments_and_hydrogens(cuda):
    two, methane, ethane = named('two ethanols and a chloride'), named('methane with hydrogens'), named('ethane with hydrogens')
    cases = [two, methane, ethane]
    ptr, mol, ref = arrays(cases)
    pos = np.concatenate([PC.permuted_rows(c['pos'], c['auto']) for c in cases])[None]
    for largest in (False, True):
        for skip_h in (True, False):
            got = rmsd_gpu(cuda, ptr, mol, pos, ref, largest=largest, skip_h=skip_h)
            assert_same(got, R.pose_rmsd_batch(ptr, mol, PC.Z_ALL, pos, ref, largest_only=largest, skip_h=skip_h), f'{largest} {skip_h}')
            # the swap of the two ethanols needs both in S; with the largest fragment alone the second is not there
            assert (got['rmsd'][0, 0] == 0.0) == (not largest) and got['plain'][0, 0] > 1.0
            assert got['map'][0, :7].tolist() == (two['auto'] if not largest else [0, 1, 2, -1, -1, -1, -1])
            # the carbons do not move: without the hydrogens both numbers are 0; with them the turn is found
            assert got['rmsd'][1, 0] == 0.0 and (got['plain'][1, 0] > 1.0) == (not skip_h)
            assert got['map'][0, 7:12].tolist() == ([0 + 7, -1, -1, -1, -1] if skip_h else [7 + v for v in methane['auto']])
            assert got['rmsd'][2, 0] == 0.0 and got['plain'][2, 0] > 1.0 and got['map'][0, 12:14].tolist() == [13, 12]


def test_sanitised_labels_do_not_depend_on_the_kekule_pattern(cuda):
    """Through perceive and sanitise.  The mirror of toluene passes through ring atoms and swaps the two Kekule patterns: the raw
    order_k as labels lose it, the labels of `Sanitized.pose_rmsd` (4 on an aromatic bond) keep it.  The mirror of o-xylene
    passes through two ring bonds and maps each pattern onto itself, so there even the raw orders keep it
    (tests/test_pose_rmsd_config.py shows both on the restatement)."""
    cases = [named('toluene'), PC.o_xylene()]
    pos = [torch.from_numpy(c['pos']).to(cuda) for c in cases]
    mols = molecule.build_molecules(pos, [torch.from_numpy(one_hot(c['sym'])).to(cuda) for c in cases], ELEMENTS)
    san = mols.sanitize()
    assert san.aromatic_bonds.sum().item() == 12
    mirrored = [torch.from_numpy(PC.permuted_rows(c['pos'], c['auto'])).to(cuda) for c in cases]
    by_default = san.pose_rmsd(mirrored)
    assert by_default.rmsd[:, 0].tolist() == [0.0, 0.0] and bool((by_default.plain[:, 0] > 1.0).all()) and by_default.status.tolist() == [0, 0]
    assert by_default.map[0].tolist() == cases[0]['auto'] + [7 + v for v in cases[1]['auto']]
    raw = san.molecules.pose_rmsd(mirrored, bond_label=san.molecules.order.clamp(1, 3))
    assert raw.rmsd[0, 0].item() == raw.plain[0, 0].item() > 1.0 and raw.rmsd[1, 0].item() == 0.0
    assert mols.pose_rmsd(mirrored).rmsd[:, 0].tolist() == [0.0, 0.0]                              # connectivity alone


def test_status_paths(cuda):
    benzene, ethanol = named('benzene'), named('ethanol')
    empty = dict(name='empty', sym=[], pos=np.zeros((0, 3), dtype=np.float32), bonds=[], frag=[], auto=None, group=None)
    cases = [benzene, empty, ethanol, benzene, ethanol, benzene]
    ptr, mol, ref = arrays(cases)
    mol['status'][2] = 8                            # left out by perception
    pos = stack(cases, 3)
    atom_label = np.zeros(len(ref), dtype=np.int64)
    atom_label[int(ptr[3]) + 2] = 2 ** 20           # out of range: ligand 3
    bond_label = np.ones(len(mol['bonds']), dtype=np.int64)
    bond_label[int(mol['bond_ptr'][4])] = 16        # out of range: ligand 4
    pos[1, int(ptr[5]) + 4, 1] = np.nan             # one pose of ligand 5
    got = rmsd_gpu(cuda, ptr, mol, pos, ref, bond_label=bond_label, atom_label=atom_label)
    assert_same(got, R.pose_rmsd_batch(ptr, mol, PC.Z_ALL, pos, ref, bond_label=bond_label, atom_label=atom_label), 'status paths')
    assert got['status'].tolist() == [0, 1, 1, 1, 1, 4]
    assert not got['rmsd'][1:5].any() and not got['nodes'][1:5].any() and (got['map'][:, int(ptr[1]):int(ptr[5])] == -1).all()
    assert got['rmsd'][5, 1] == 0.0 and got['nodes'][5].tolist()[1] == 0 and got['nodes'][5, 0] > 0 and got['nodes'][5, 2] > 0
    assert (got['map'][1, int(ptr[5]):] == -1).all() and (got['map'][0, int(ptr[5]):] >= 0).all()
    # a budget of 5 on benzene turned by one position: the bit, max_nodes + 1 nodes, and still an upper bound
    ptr, mol, ref = arrays([benzene])
    turned = PC.permuted_rows(benzene['pos'], benzene['auto'])[None]
    cut = rmsd_gpu(cuda, ptr, mol, turned, ref, max_nodes=5)
    assert_same(cut, R.pose_rmsd_batch(ptr, mol, PC.Z_ALL, turned, ref, max_nodes=5), 'max_nodes = 5')
    assert cut['status'].tolist() == [2] and cut['nodes'][0, 0] == 6 and cut['rmsd'][0, 0] == cut['plain'][0, 0] > 1.0
    # the same through the pairs, where a NaN pose spoils its row and its column only
    ptr, mol, ref = arrays([benzene, ethanol])
    pos = stack([benzene, ethanol], 4)
    pos[2, 3, 0] = np.inf
    got = rmsd_gpu(cuda, ptr, mol, pos, pairs=True)
    assert_same(got, R.pose_rmsd_batch(ptr, mol, PC.Z_ALL, pos, pairs=True), 'pairs with a non-finite pose')
    assert got['status'].tolist() == [4, 0] and not got['nodes'][0, 2].any() and not got['nodes'][0, :, 2].any() and got['nodes'][0, 0, 1] > 0


def test_refusals_and_an_empty_batch(cuda):
    ptr, mol, ref = arrays([])
    got = rmsd_gpu(cuda, ptr, mol, np.zeros((2, 0, 3), dtype=np.float32), ref)
    assert got['rmsd'].shape == (0, 2) and got['status'].shape == (0,)
    ptr, mol, ref = arrays([named('ethanol')])
    z = torch.tensor(PC.Z_ALL, dtype=torch.int32, device=cuda)
    d = torch.zeros(64, dtype=torch.int64, device=cuda)
    p = d.data_ptr()
    L = hip.lib()
    for K, pairs, max_nodes in ((0, 0, 10), (65, 1, 10), (2, 2, 10), (2, 0, 0)):
        assert L.kpd_pose_rmsd(p, 0, 0, p, len(PC.Z_ALL), z.data_ptr(), p, p, p, 0, p, None, None, 0, 1, p, p, K, pairs, max_nodes, p, p, None, p,
                               p, p, torch.cuda.current_stream().cuda_stream) != 0, (K, pairs, max_nodes)
    none = molecule.build_molecules([], [], ELEMENTS)
    r = none.pose_rmsd(torch.zeros(0, 3, device=cuda), ref=torch.zeros(0, 3, device=cuda))
    assert r.rmsd.shape == (0, 1) and r.map.shape == (1, 0) and r.table()['lig_idx'] == []
    assert none.pose_rmsd(torch.zeros(3, 0, 3, device=cuda), pairs=True).rmsd.shape == (0, 3, 3)


def test_alone_in_a_mixed_batch_with_spare_bond_rows_and_other_K(cuda, world):
    target = PC.generated(3)[2]
    others = (world['cases'][:16] + world['cases'][17:41])[:39]                 # without the 256-atom ring
    poses = PC.poses(target, 5, seed=9)
    ptr, mol, ref = arrays([target])
    alone = rmsd_gpu(cuda, ptr, mol, poses[:2], ref)
    assert alone['status'].tolist() == [0]
    for at in (0, 20, 39):
        cases = others[:at] + [target] + others[at:]
        assert len(cases) == 40
        n_atoms = sum(len(c['sym']) for c in cases)
        ptr, mol, ref = arrays(cases, cap_bonds=3 * n_atoms)
        pos = stack(cases, 5, seed=4)
        a0 = int(ptr[at])
        pos[:, a0:a0 + len(target['sym'])] = poses
        got = rmsd_gpu(cuda, ptr, mol, pos, ref)
        again = rmsd_gpu(cuda, ptr, mol, pos, ref)
        for k in ('rmsd', 'plain'):
            assert np.array_equal(bits(got[k][at, :2]), bits(alone[k][0])) and np.array_equal(bits(got[k]), bits(again[k]))
        assert np.array_equal(got['nodes'][at, :2], alone['nodes'][0]) and np.array_equal(got['nodes'], again['nodes'])
        assert np.array_equal(got['map'][:2, a0:a0 + len(target['sym'])] - a0, alone['map']) and np.array_equal(got['map'], again['map'])


# ---- the methods ---------------------------------------------------------------------------------------------------------------------
def test_relaxed_minimised_and_docked_poses(cuda):
    rng = np.random.default_rng(5)
    ligs = [grow(rng, n) for n in (8, 11, 5, 9, 14, 7)]
    pos = [torch.from_numpy(p).to(cuda) for _, p in ligs]
    feat = [torch.from_numpy(one_hot(s)).to(cuda) for s, _ in ligs]
    anchor = np.concatenate([p for _, p in ligs])
    pockets = [make_pocket(rng, 40, anchor, reach=4.0), make_pocket(rng, 60, anchor, reach=4.0)]
    ppos, psym = [torch.from_numpy(p).to(cuda) for _, p in pockets], [s for s, _ in pockets]
    mols = molecule.build_molecules(pos, feat, ELEMENTS)
    pof = [0, 0, 0, 1, 1, 1]
    # sym <= plain to the bit; plain and the report's column sum the same terms in another order (source order against index
    # order): at most n ulp apart, far inside 1e-12 relative
    r = mols.relax(ppos, psym, pocket_of=pof, max_iters=30)
    full = mols.pose_rmsd(r.molecules.pos)
    assert torch.equal(r.sym_rmsd(), full.rmsd[:, 0]) and bool((full.rmsd <= full.plain).all()) and full.status.tolist() == [0] * 6
    assert torch.allclose(full.plain[:, 0], r.report[:, 2], rtol=1e-12, atol=0.0) and bool((r.sym_rmsd() <= r.report[:, 2] * (1 + 1e-12)).all())
    assert r.table()['rmsd'] == r.report[:, 2].tolist()                                            # the report keeps its column
    m = mols.vina_minimize(ppos, psym, pocket_of=pof, radii=RADII, max_iters=10)
    assert m.sym_rmsd().shape == (6,) and bool((m.sym_rmsd() <= m.report[:, 8] * (1 + 1e-12)).all())
    d = mols.vina_dock(ppos, psym, pocket_of=pof, radii=RADII, n_chains=3, n_steps=2, seed=7, step_iters=5, max_iters=10)
    s, mm, found = d.sym_rmsd(), d.mode_rmsd(), d.n_found.tolist()
    assert s.shape == (6, 3) and mm.shape == (6, 3, 3) and torch.equal(mm, mm.transpose(1, 2)) and not bool(mm.diagonal(dim1=1, dim2=2).any())
    for b in range(6):
        assert not bool(s[b, found[b]:].any()) and not bool(mm[b, found[b]:].any()) and not bool(mm[b, :, found[b]:].any())
        assert bool((s[b, :found[b]] <= d.report[b, :found[b], 4] * (1 + 1e-12)).all())
    kept = d.distinct_modes()
    assert [k[0] for k in kept] == [0] * 6 and all(k == sorted(set(k)) and len(k) <= found[b] for b, k in enumerate(kept))
    t = full.table()
    assert list(t) == ['lig_idx', 'pose', 'rmsd', 'plain', 'nodes'] and t['lig_idx'] == list(range(6)) and t['rmsd'] == full.rmsd[:, 0].tolist()


def test_distinct_modes_drops_a_flipped_phenyl(cuda):
    """A hand-built stack of modes: biphenyl, the same with its second ring flipped (rows 7 <-> 11 and 8 <-> 10 exchanged), and
    a pose moved by 3 A.  The atom-by-atom rule of kpd_vina_dock keeps all three (the flip reads 1.4 A); with the symmetric
    matrix the flip is mode 0 again."""
    c = named('biphenyl')
    flip = list(range(6)) + [6, 11, 10, 9, 8, 7]
    ref = c['pos']
    modes = np.stack([ref, PC.permuted_rows(ref, flip), ref + np.array([3.0, 0.0, 0.0], dtype=np.float32)])
    mols = molecule.build_molecules([torch.from_numpy(ref).to(cuda)], [torch.from_numpy(one_hot(c['sym'])).to(cuda)], ELEMENTS)
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=cuda)
    out = dict(pos=torch.from_numpy(modes).to(cuda), n_found=torch.tensor([3], dtype=torch.int32, device=cuda), report=f64(1, 3, 8),
               chain_pos=torch.from_numpy(modes).to(cuda), chain_report=f64(1, 3, 10), status=torch.zeros(1, dtype=torch.int32, device=cuda))
    z3 = torch.zeros(1, 3, device=cuda)
    d = molecule.VinaDocked(mols, out, torch.zeros(0, dtype=torch.int32, device=cuda), (z3, z3))
    pr = mols.pose_rmsd(d._pos, pairs=True)
    assert pr.plain[0, 0, 1].item() > 1.0 and pr.rmsd[0, 0, 1].item() == 0.0                        # kept by the plain rule at 1 A
    assert torch.equal(d.mode_rmsd(), pr.rmsd) and d.distinct_modes() == [[0, 2]] and d.distinct_modes(min_rmsd=5.0) == [[0]]
    assert d.sym_rmsd()[0].tolist()[:2] == [0.0, 0.0] and abs(d.sym_rmsd()[0, 2].item() - 3.0) < 1e-6
    out['n_found'] = torch.tensor([2], dtype=torch.int32, device=cuda)
    two = molecule.VinaDocked(mols, out, torch.zeros(0, dtype=torch.int32, device=cuda), (z3, z3))
    assert two.distinct_modes() == [[0]] and not bool(two.mode_rmsd()[0, 2].any()) and two.sym_rmsd()[0, 2].item() == 0.0
    t = pr.table()
    assert list(t) == ['lig_idx', 'pose_i', 'pose_j', 'rmsd', 'plain', 'nodes'] and t['pose_i'] == [0, 0, 1] and t['pose_j'] == [1, 2, 2]
