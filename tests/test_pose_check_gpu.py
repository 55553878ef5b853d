"""Plausibility checks of poses on the GPU (kpd_pose_check and the methods on it) against the restatement of include/kpd.h
(tests/pose_check_ref.py), bit for bit: every fail, count, atom_fail and status, and every bit of report.  The graphs are fed as
kpd_mol_perceive and kpd_mol_sanitize would have left them, so only the checks are under test.  Every raw call runs with canary
bytes behind each output buffer and checks that no input was written.  The restatement of the shared batch is computed once,
for three poses: a pose's result does not depend on K, so K = 1 is its first column."""
import ctypes

import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import hip, molecule
from . import pose_check_cases as PC
from . import pose_check_ref as R
from . import sanitize_cases as SC
from .molecule_cases import ELEMENTS, one_hot
from .relax_cases import grow, make_pocket
from .test_molecule_gpu import Guarded
from .vina_cases import RADII

pytestmark = pytest.mark.gpu
NR, NC = len(R.REPORT), len(R.COUNTS)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def check_gpu(dev, ptr, mol, san, pos, lig_radius, pocket=None, largest=False, max_atoms=R.MOL_MAX, max_pocket=None, params=None, z=PC.Z_H):
    """kpd_pose_check through the C ABI; returns numpy arrays in the shapes of pose_check_ref.pose_check_batch."""
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.int32).to(dev)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    pos = np.asarray(pos, dtype=np.float32)
    K, N, B, cap = pos.shape[0], pos.shape[1], len(ptr) - 1, len(np.asarray(mol['bonds']).reshape(-1, 2))
    if pocket is None:
        pocket = dict(x=np.zeros((0, 3), np.float32), radius=np.zeros(0, np.float32), ptr=[0], of=[-1] * B)
    M, n_pockets = len(pocket['x']), len(pocket['ptr']) - 1
    ins = [i32(ptr), i32(mol['elem']), i32(np.asarray(z)), i32(mol['frag']), i32(np.asarray(mol['bonds']).reshape(-1)), i32(san['order_k']),
           i32(san['bond_flags']), i32(mol['bond_ptr']), i32(mol['status']), i32(san['status']), i32(san['atom_h']), i32(san['atom_flags']),
           f32(pos), f32(lig_radius), f32(pocket['x']), f32(pocket['radius']), i32(pocket['ptr']), i32(pocket['of'])]
    before = [x.clone() for x in ins]
    g = Guarded(dev)
    fail, report, counts = g.new(B * K), g.new(B * K * NR, torch.float64), g.new(B * K * NC)
    atom_fail, status = g.new(K * N), g.new(B * K)
    prm = None
    if params:
        prm = hip.pose_check_params(**params)
    p = [x.data_ptr() if x.numel() else None for x in ins]
    hip.check(hip.lib().kpd_pose_check(ins[0].data_ptr(), N, B, max_atoms, p[1], len(z), ins[2].data_ptr(), p[3], p[4], p[5], p[6],
                                       ins[7].data_ptr(), cap, p[8], p[9], p[10], p[11], int(largest), p[12], K, ins[13].data_ptr(), p[14],
                                       p[15], ins[16].data_ptr(), M, n_pockets, M if max_pocket is None else max_pocket, p[17],
                                       None if prm is None else ctypes.byref(prm), fail.data_ptr(), report.data_ptr(), counts.data_ptr(),
                                       atom_fail.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    g.check()
    for x, y in zip(ins, before):                   # inputs are never written (compared as bits: a pose may hold a NaN)
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    host = lambda t, n, shape: t[:n].cpu().numpy().reshape(shape)
    return dict(fail=host(fail, B * K, (B, K)).astype(np.int64), report=host(report, B * K * NR, (B, K, NR)),
                counts=host(counts, B * K * NC, (B, K, NC)).astype(np.int64), atom_fail=host(atom_fail, K * N, (K, N)).astype(np.int64),
                status=host(status, B * K, (B, K)).astype(np.int64))


def assert_same(got, ref, what='', poses=None):
    """Every bit of every output; `poses`: compare with the first poses of a reference computed for more."""
    sub = (lambda k, a: a) if poses is None else (lambda k, a: a[:poses] if k == 'atom_fail' else a[:, :poses])
    for k in ('status', 'fail', 'counts', 'atom_fail'):
        want = sub(k, ref[k])
        assert np.array_equal(got[k], want), (what, k, np.argwhere(got[k] != want)[:4], got[k][got[k] != want][:4], want[got[k] != want][:4])
    want = sub('report', ref['report'])
    assert np.array_equal(bits(got['report']), bits(want)), (what, 'report', np.argwhere(bits(got['report']) != bits(want))[:4])


def near_pocket(rng, pos, m, keep_out=2.2, reach=5.0):
    """m pocket carbons around the atoms `pos`: some of them close enough to clash, none closer than keep_out."""
    out = []
    while len(out) < m:
        q = pos[int(rng.integers(len(pos)))] + rng.standard_normal(3) * reach / 2
        if np.linalg.norm(pos - q, axis=1).min() >= keep_out:
            out.append(q)
    return PC.carbon_pocket(np.array(out))


# ---- the shared batch and its restatement, computed once -------------------------------------------------------------------------------
SHAPES = (1, 2, 63, 64, 65, 256, 257)


@pytest.fixture(scope='module')
def world():
    rng = np.random.default_rng(77)
    cases = PC.all_cases()
    for n in SHAPES:
        c = PC.chain_case(n)
        if n in (2, 65):                            # the lattice over more than one atom per lane; the long chains stay without a pocket
            c = PC.posed(c, c['name'] + ' in a pocket', c['pos'], 0, pocket=near_pocket(rng, c['pos'].astype(np.float64), 12))
        cases.append(c)
    cases.insert(3, PC.mol('empty', [], np.zeros((0, 3)), []))
    ptr, mol, san, pos, pocket = PC.arrays(cases, K=3)
    radius = PC.lig_radius()
    ref = R.pose_check_batch(ptr, mol, san, PC.Z_H, pos, radius, pocket)
    return dict(cases=cases, ptr=ptr, mol=mol, san=san, pos=pos, pocket=pocket, radius=radius, ref=ref)


@pytest.mark.parametrize('K', [1, 3])
def test_every_bit_equals_the_restatement(cuda, world, K):
    got = check_gpu(cuda, world['ptr'], world['mol'], world['san'], world['pos'][:K], world['radius'], world['pocket'])
    assert_same(got, world['ref'], f'K={K}', poses=K)
    names = [c['name'] for c in world['cases']]
    st = got['status'][:, 0]
    assert st[names.index('empty')] == R.NO_MOLECULE and st[names.index('chain 257')] == R.NO_MOLECULE and st[names.index('chain 256')] == 0
    for c in world['cases']:                        # the flags of the hand cases, now from the kernel
        if c['expect'] or c['name'] in ('benzene', 'propane', 'acetamide', 'hexane'):
            assert got['fail'][names.index(c['name']), 0] == c['expect'], c['name']
    lig = R.COUNTS.index('n_lig_points')
    assert got['counts'][names.index('chain 65 in a pocket'), 0, lig] > 2000 and got['counts'][names.index('chain 256'), 0, lig] == 0


def test_no_ligands_and_no_atoms(cuda):
    ptr, mol, san, pos, pocket = PC.arrays([], K=2)
    got = check_gpu(cuda, ptr, mol, san, pos, PC.lig_radius(), pocket)
    assert got['fail'].shape == (0, 2) and got['atom_fail'].shape == (2, 0)


# ---- named behaviour -------------------------------------------------------------------------------------------------------------------
def two_fragments():
    """Propane and, as a second fragment, a C-C pair stretched far beyond any bond length: only the scope decides whether it counts."""
    pr = PC.propane()
    pos = np.concatenate([pr['pos'], pr['pos'][:2] + np.float32(8.0)])
    pos[4] += np.float32(1.0)
    return PC.mol('two fragments', ['C'] * 5, pos, [(0, 1, 1), (1, 2, 1), (3, 4, 1)], h=[3, 2, 3, 3, 3])


def test_largest_only(cuda):
    c = two_fragments()
    ptr, mol, san, pos, pocket = PC.arrays([c])
    for largest in (False, True):
        ref = R.pose_check_batch(ptr, mol, san, PC.Z_H, pos, PC.lig_radius(), pocket, largest=largest)
        got = check_gpu(cuda, ptr, mol, san, pos, PC.lig_radius(), pocket, largest=largest)
        assert_same(got, ref, f'largest={largest}')
        assert got['fail'][0, 0] == (0 if largest else R.F_BOND) and got['counts'][0, 0, 0] == (2 if largest else 3)
        assert not got['atom_fail'][0, :3].any() and got['atom_fail'][0, 3:].tolist() == ([0, 0] if largest else [R.F_BOND] * 2)


def test_pockets_shared_staged_and_absent(cuda, world):
    rng = np.random.default_rng(5)
    a, b = PC.hexane(), PC.benzene()
    b = PC.posed(b, 'benzene next to hexane', b['pos'] + np.float32(3.5), 0)
    ptr, mol, san, pos, _ = PC.arrays([a, b, PC.propane()], K=2)
    shared = near_pocket(rng, pos[0, :12].astype(np.float64), 40)
    pocket = dict(x=shared['x'], radius=shared['radius'], ptr=[0, 40], of=[0, 0, -1])
    ref = R.pose_check_batch(ptr, mol, san, PC.Z_H, pos, PC.lig_radius(), pocket)
    full = check_gpu(cuda, ptr, mol, san, pos, PC.lig_radius(), pocket)
    assert_same(full, ref, 'two ligands in one pocket, one without')
    pk, lig = R.COUNTS.index('pocket_pairs'), R.COUNTS.index('n_lig_points')
    assert full['counts'][:, 0, pk].tolist() == [240, 240, 0] and full['counts'][2, 0, lig] == 0 and (full['counts'][:2, :, lig] > 300).all()
    for max_pocket in (0, 7, 39):                   # a pocket larger than the stage: the rest comes from global memory, to the bit
        assert_same(check_gpu(cuda, ptr, mol, san, pos, PC.lig_radius(), pocket, max_pocket=max_pocket), ref, f'max_pocket={max_pocket}')


def test_bad_coordinates_and_zero_radii(cuda):
    rng = np.random.default_rng(6)
    h = PC.hexane()
    with_pocket = PC.posed(h, 'hexane in a pocket', h['pos'], 0, pocket=near_pocket(rng, h['pos'].astype(np.float64), 10))
    cases = [with_pocket, PC.benzene(), PC.posed(h, 'hexane in another pocket', h['pos'], 0, pocket=with_pocket['pocket'])]
    ptr, mol, san, pos, pocket = PC.arrays(cases, K=3)
    pos[1, 8, 2] = np.nan                           # benzene's pose 1
    pos[2, 1, 0] = np.inf                           # the first hexane's pose 2
    pocket['x'][13, 1] = np.nan                     # the second pocket: every pose of its ligand
    pocket['radius'][2] = 0.0                       # the first pocket: an atom that takes no part
    ref = R.pose_check_batch(ptr, mol, san, PC.Z_H, pos, PC.lig_radius(), pocket)
    got = check_gpu(cuda, ptr, mol, san, pos, PC.lig_radius(), pocket)
    assert_same(got, ref, 'NaN and Inf')
    assert got['status'].tolist() == [[R.ATOM_OUT, R.ATOM_OUT, R.BAD_INPUT], [0, R.BAD_INPUT, 0], [R.BAD_INPUT] * 3]
    assert not got['report'][2].any() and not got['counts'][0, 2].any() and not got['atom_fail'][1, 6:12].any()
    assert got['counts'][0, 0, R.COUNTS.index('pocket_pairs')] == 9 * 6
    zero_n = PC.lig_radius(N=0.0)                   # a class without a radius: out of checks 3, 5 and 6, still in 1, 2 and 4
    ptr, mol, san, pos, pocket = PC.arrays([PC.posed(PC.acetamide(), 'acetamide in a pocket', PC.acetamide()['pos'], 0,
                                                     pocket=with_pocket['pocket'])])
    ref = R.pose_check_batch(ptr, mol, san, PC.Z_H, pos, zero_n, pocket)
    got = check_gpu(cuda, ptr, mol, san, pos, zero_n, pocket)
    assert_same(got, ref, 'zero radius')
    assert got['status'][0, 0] == R.ATOM_OUT and got['counts'][0, 0, R.COUNTS.index('pocket_pairs')] == 3 * 10 and got['counts'][0, 0, 0] == 3
    bad = PC.lig_radius(C=np.nan)
    assert check_gpu(cuda, ptr, mol, san, pos, bad, pocket)['status'][0, 0] == R.BAD_INPUT
    assert R.pose_check_batch(ptr, mol, san, PC.Z_H, pos, bad, pocket)['status'][0, 0] == R.BAD_INPUT


def test_hydrogens_take_part_on_request(cuda):
    e = PC.ethene()
    rng = np.random.default_rng(8)
    c = PC.posed(e, 'ethene in a pocket', e['pos'], 0, pocket=near_pocket(rng, e['pos'].astype(np.float64), 8, keep_out=2.6))
    ptr, mol, san, pos, pocket = PC.arrays([c])
    lig = R.COUNTS.index('n_lig_points')
    points = []
    for with_h in (False, True):
        radius = PC.lig_radius(with_h)
        ref = R.pose_check_batch(ptr, mol, san, PC.Z_H, pos, radius, pocket)
        got = check_gpu(cuda, ptr, mol, san, pos, radius, pocket)
        assert_same(got, ref, f'with_h={with_h}')
        assert got['status'][0, 0] == (0 if with_h else R.ATOM_OUT)
        assert got['counts'][0, 0, R.COUNTS.index('pocket_pairs')] == (6 if with_h else 2) * 8
        points.append(int(got['counts'][0, 0, lig]))
    assert points[1] > points[0] > 0


def test_thresholds_are_parameters(cuda):
    ptr, mol, san, pos, pocket = PC.arrays([PC.benzene(), PC.propane()])
    params = dict(bond_lo=0.99, angle_hi=1.03)
    ref = R.pose_check_batch(ptr, mol, san, PC.Z_H, pos, PC.lig_radius(), pocket, params=params)
    got = check_gpu(cuda, ptr, mol, san, pos, PC.lig_radius(), pocket, params=params)
    assert_same(got, ref, 'params')
    assert got['fail'][:, 0].tolist() == [R.F_BOND, R.F_ANGLE]


# ---- invariance ------------------------------------------------------------------------------------------------------------------------
def test_independent_of_the_batch_the_place_the_capacities_and_the_repeat(cuda, world):
    names = [c['name'] for c in world['cases']]
    target = world['cases'][names.index('benzene half-way into a slab')]
    ptr, mol, san, pos, pocket = PC.arrays([target], K=3)
    radius = world['radius']
    alone = check_gpu(cuda, ptr, mol, san, pos, radius, pocket)
    assert alone['status'].tolist() == [[0, 0, 0]] and alone['fail'][0, 0] == target['expect']
    tight = check_gpu(cuda, ptr, mol, san, pos[:2], radius, pocket, max_atoms=6, max_pocket=5)
    others = [c for c in world['cases'] if len(c['sym']) < 60 and c is not target]
    for at in (0, 7, len(others)):
        cases = others[:at] + [target] + others[at:]
        n_atoms = sum(len(c['sym']) for c in cases)
        ptr, mol, san, pos, pocket = PC.arrays(cases, K=3, cap_bonds=3 * n_atoms)
        got = check_gpu(cuda, ptr, mol, san, pos, radius, pocket)
        again = check_gpu(cuda, ptr, mol, san, pos, radius, pocket)
        a0 = int(ptr[at])
        for k in ('fail', 'counts', 'status'):
            assert np.array_equal(got[k][at], alone[k][0]) and np.array_equal(got[k], again[k]) and np.array_equal(tight[k][0], alone[k][0, :2])
        assert np.array_equal(bits(got['report'][at]), bits(alone['report'][0])) and np.array_equal(bits(got['report']), bits(again['report']))
        assert np.array_equal(bits(tight['report'][0]), bits(alone['report'][0, :2]))
        assert np.array_equal(got['atom_fail'][:, a0:a0 + 6], alone['atom_fail']) and np.array_equal(got['atom_fail'], again['atom_fail'])
        assert np.array_equal(tight['atom_fail'], alone['atom_fail'][:2])


# ---- the methods -----------------------------------------------------------------------------------------------------------------------
def host_arrays(san):
    """A `Sanitized` -> (ptr, mol, san, z) as numpy arrays in the layout of the C ABI."""
    m = san.molecules
    host = lambda t: t.cpu().numpy().astype(np.int64)
    mol = dict(elem=host(m.elem), frag=host(m.frag), bonds=host(m.bonds), bond_ptr=host(m.bond_ptr), status=host(m.status))
    sn = dict(order_k=host(m.order), bond_flags=host(san.bond_flags), atom_h=host(san.h), atom_flags=host(san.atom_flags), status=host(san.status))
    return host(m.lig_ptr), mol, sn, [molecule.ATOMIC_NUMBERS[e] for e in m.lig_elements]


def test_methods_equal_the_raw_call_on_generated_ligands(cuda):
    rng = np.random.default_rng(12)
    ligs = [(sym, pos) for sym, pos, _ in SC.generated(48)]
    pos = [torch.from_numpy(np.asarray(p, dtype=np.float32)).to(cuda) for _, p in ligs]
    feat = [torch.from_numpy(one_hot(s)).to(cuda) for s, _ in ligs]
    san = molecule.build_molecules(pos, feat, ELEMENTS).sanitize()
    m = san.molecules
    pockets = [near_pocket(rng, np.asarray(ligs[q][1], dtype=np.float64), 16) for q in range(2)]
    ppos, psym = [torch.from_numpy(p['x']).to(cuda) for p in pockets], [['C'] * 16] * 2
    pof = [0, 1, 0, 1, 0, 1] + [-1] * 42
    base = torch.cat(pos)
    stack = torch.stack([base, base + 0.15 * torch.randn(base.shape, generator=torch.Generator().manual_seed(3)).to(cuda)])
    pc = san.pose_check(stack, ppos, psym, pocket_of=pof)
    host = lambda t: t.cpu().numpy().astype(np.int64)
    _, mol, sn, z = host_arrays(san)
    radius = np.array(molecule.vdw_radius_table(ELEMENTS), dtype=np.float32)
    pocket = dict(x=np.concatenate([p['x'] for p in pockets]), radius=np.full(32, molecule.VDW_RADII['C'], dtype=np.float32), ptr=[0, 16, 32], of=pof)
    raw = check_gpu(cuda, host(m.lig_ptr), mol, sn, stack.cpu().numpy(), radius, pocket, z=z)
    got = dict(fail=host(pc.fail), report=pc.report.cpu().numpy(), counts=host(pc.counts), atom_fail=host(pc.atom_fail), status=host(pc.status))
    assert_same(got, raw, 'method against raw call')
    ref = R.pose_check_batch(host(m.lig_ptr), mol, sn, z, stack.cpu().numpy(), radius, pocket)
    assert_same(raw, ref, 'generated ligands')
    assert not (raw['status'] & 3).any() and (raw['counts'][:, :, R.COUNTS.index('rings')] > 0).sum() >= 2
    assert (raw['counts'][:6, :, R.COUNTS.index('n_lig_points')] > 0).all()
    assert torch.equal(pc.passed, (pc.fail == 0) & ((pc.status & 3) == 0) & san.valid[:, None])
    t = pc.table()
    assert list(t)[:3] == ['lig_idx', 'pose', 'passed'] and len(t['lig_idx']) == 96 and t['bond_ok'] == [not f & 1 for f in raw['fail'].reshape(-1)]
    own = san.pose_check()                          # the molecules' own pose, no pocket
    assert own.fail.shape == (48, 1) and torch.equal(own.fail[:, 0] & 63, pc.fail[:, 0] & 63)
    samples = [dict(positions=pos[:24], features=feat[:24]), dict(positions=pos[24:], features=feat[24:])]
    out = molecule.analyze_samples(samples, ELEMENTS, pose_check=True)
    assert 0.0 <= out['plausible'] <= 1.0 and 'plausible' not in molecule.analyze_samples(samples, ELEMENTS, sanitize=True)
    assert torch.equal(molecule.check_samples(pos, feat, ELEMENTS).fail, own.fail)


def test_hydrogenated_molecules_with_and_without_their_hydrogens(cuda):
    """The output of `add_hs`, sanitised again: the hydrogens are atoms of the graph, and `with_h` decides whether they take part in
    the clash and overlap checks; checks 1, 2 and 4 see them either way."""
    rng = np.random.default_rng(21)
    ligs = [(sym, pos) for sym, pos, _ in SC.generated(4)]
    pos = [torch.from_numpy(np.asarray(p, dtype=np.float32)).to(cuda) for _, p in ligs]
    feat = [torch.from_numpy(one_hot(s)).to(cuda) for s, _ in ligs]
    hyd = molecule.build_molecules(pos, feat, ELEMENTS).sanitize().add_hs()
    assert int(hyd.n_h.min()) > 0
    hs = hyd.molecules.sanitize()
    pk = near_pocket(rng, hyd.molecules.pos.cpu().numpy().astype(np.float64)[:int(hyd.molecules.lig_ptr[1])], 16, keep_out=2.4)
    ppos, psym, pof = [torch.from_numpy(pk['x']).to(cuda)], [['C'] * 16], [0, 0, -1, -1]
    ptr, mol, sn, z = host_arrays(hs)
    pocket = dict(x=pk['x'], radius=np.full(16, molecule.VDW_RADII['C'], dtype=np.float32), ptr=[0, 16], of=pof)
    got = {}
    for with_h in (False, True):
        pc = hs.pose_check(None, ppos, psym, pocket_of=pof, with_h=with_h)
        radius = np.array(molecule.vdw_radius_table(hs.molecules.lig_elements, with_h=with_h), dtype=np.float32)
        ref = R.pose_check_batch(ptr, mol, sn, z, hs.molecules.pos.cpu().numpy()[None], radius, pocket)
        host = lambda t: t.cpu().numpy().astype(np.int64)
        got[with_h] = dict(fail=host(pc.fail), report=pc.report.cpu().numpy(), counts=host(pc.counts), atom_fail=host(pc.atom_fail),
                           status=host(pc.status))
        assert_same(got[with_h], ref, f'hydrogenated, with_h={with_h}')
        assert got[with_h]['status'][:, 0].tolist() == [0 if with_h else R.ATOM_OUT] * 4
    off, on = got[False], got[True]
    for k in ('pocket_pairs', 'n_lig_points', 'pairs'):
        col = R.COUNTS.index(k)
        assert (on['counts'][:2, 0, col] > off['counts'][:2, 0, col]).all(), k
    same = R.F_BOND | R.F_ANGLE | R.F_RING | R.F_CENTRE | R.F_TWIST
    assert np.array_equal(on['fail'] & same, off['fail'] & same) and np.array_equal(on['counts'][:, :, :4], off['counts'][:, :, :4])
    n_bonds = (hs.molecules.bond_ptr[1:] - hs.molecules.bond_ptr[:-1]).cpu().numpy()
    assert np.array_equal(on['counts'][:, 0, 0], n_bonds)                            # every X-H bond has a rest length


def test_relaxed_minimised_and_docked_poses_in_one_call(cuda):
    rng = np.random.default_rng(5)
    ligs = [grow(rng, n) for n in (8, 11)]
    pos = [torch.from_numpy(p).to(cuda) for _, p in ligs]
    feat = [torch.from_numpy(one_hot(s)).to(cuda) for s, _ in ligs]
    anchor = np.concatenate([p for _, p in ligs])
    sym, pp = make_pocket(rng, 40, anchor, reach=4.0)
    ppos, psym = [torch.from_numpy(pp).to(cuda)], [sym]
    san = molecule.build_molecules(pos, feat, ELEMENTS).sanitize()
    mols = san.molecules
    d = mols.vina_dock(ppos, psym, radii=RADII, n_chains=3, n_steps=2, seed=7, step_iters=5, max_iters=10)
    pc = d.pose_check(san, ppos, psym)
    assert pc.fail.shape == (2, d.n_modes) and pc.atom_fail.shape == (d.n_modes, 19) and pc.status.shape == (2, d.n_modes)
    direct = san.pose_check(d._pos, ppos, psym)
    assert torch.equal(pc.fail, direct.fail) and torch.equal(pc.report.view(torch.int64), direct.report.view(torch.int64))
    assert not bool((pc.status & 3).any()) and bool((pc.counts[:, :, R.COUNTS.index('pocket_pairs')] > 0).all())
    r = mols.relax(ppos, psym, max_iters=30)
    rc = r.pose_check(san, ppos, psym)
    assert rc.fail.shape == (2, 1) and torch.equal(rc.fail, san.pose_check(r.molecules.pos, ppos, psym).fail)
    mn = mols.vina_minimize(ppos, psym, radii=RADII, max_iters=10)
    assert mn.pose_check(san, ppos, psym).fail.shape == (2, 1)
    with pytest.raises(hip.KpdError):
        other = molecule.build_molecules(pos, feat, ELEMENTS).sanitize()
        d.pose_check(other, ppos, psym)
