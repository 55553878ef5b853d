"""Explicit hydrogens on the GPU (kpd_mol_add_hs, Sanitized.add_hs) against the float64 restatement of the placement rule in
include/kpd.h (tests/hydrogens_ref.py).  Every comparison is exact equality: the integers, and the fp32 coordinates bit for bit.
The restatement runs on the graph the GPU perceived and sanitised, so only the hydrogen placement is under test here.
Every raw call runs with canary bytes behind each output buffer and around the scratch."""
import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import hip, molecule, utils
from . import hydrogens_cases as HC
from . import hydrogens_ref as HR
from . import sanitize_cases as SC
from . import sanitize_ref as SR
from .molecule_cases import ELEMENTS, one_hot
from .test_molecule_gpu import CANARY, Guarded, concat, perceive_gpu, random_batch
from .test_sanitize_gpu import mol_of, sanitize_gpu
from .util import guarded, intact

pytestmark = pytest.mark.gpu
ATOM_KEYS = ('elem', 'valence', 'frag', 'parent', 'source')
INT_KEYS = ('out_ptr', 'out_bond_ptr') + ATOM_KEYS + ('bonds', 'order', 'summary', 'n_h', 'status')


def add_hs_gpu(dev, pos, ptr, mol, san, largest=False, h_class=HC.H_CLASS, cap_atoms=None, cap_bonds=None, z=HC.Z_H, allowed=HC.ALLOWED_H):
    """kpd_mol_add_hs through the C ABI; returns numpy outputs in the layout of hydrogens_ref.add_hs_batch and the capacities."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.int32).to(dev)
    pos_d = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float32)).reshape(-1, 3).to(dev)
    ptr_d = t(np.asarray(ptr))
    N, B, cap_in = pos_d.shape[0], len(ptr) - 1, len(san['order_k'])
    extra = int(np.clip(np.asarray(san['atom_h']), 0, None).sum())
    ca = N + extra if cap_atoms is None else cap_atoms
    cb = cap_in + extra if cap_bonds is None else cap_bonds
    ins = [t(mol['elem']), t(mol['frag']), t(np.asarray(mol['bonds']).reshape(-1)), t(san['order_k']), t(mol['bond_ptr']), t(mol['status']),
           t(san['status']), t(san['valence_k']), t(san['atom_h']), t(san['atom_flags']), pos_d, ptr_d]
    before = [x.clone() for x in ins]
    zt, at = t(np.asarray(z)), t(np.asarray(allowed))
    g = Guarded(dev)
    sizes = dict(out_ptr=B + 1, pos=3 * ca, elem=ca, valence=ca, frag=ca, bonds=2 * cb, order=cb, out_bond_ptr=B + 1, summary=4 * B,
                 parent=ca, source=ca, n_h=B, status=B)
    o = {k: g.new(n, torch.float32 if k == 'pos' else torch.int32) for k, n in sizes.items()}
    L = hip.lib()
    nb = int(L.kpd_mol_add_hs_scratch_bytes(N, B))
    scratch, p_scr = guarded(nb, torch.uint8, dev, CANARY)
    hip.check(L.kpd_mol_add_hs(pos_d.data_ptr(), ptr_d.data_ptr(), N, B, ins[0].data_ptr(), len(z), zt.data_ptr(), at.data_ptr(),
                               ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), ins[4].data_ptr(), cap_in, ins[5].data_ptr(),
                               ins[6].data_ptr(), ins[7].data_ptr(), ins[8].data_ptr(), ins[9].data_ptr(), int(largest), h_class, ca, cb,
                               *[o[k].data_ptr() for k in sizes], p_scr, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    g.check()
    assert intact(scratch, nb, CANARY), f'kpd_mol_add_hs wrote outside its {nb} bytes of scratch'
    for x, y in zip(ins, before):                   # inputs are never written
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    out = {k: o[k][:n].cpu().numpy() for k, n in sizes.items()}
    out = {k: (v if k == 'pos' else v.astype(np.int64)) for k, v in out.items()}
    out['pos'], out['bonds'], out['summary'] = out['pos'].reshape(ca, 3), out['bonds'].reshape(cb, 2), out['summary'].reshape(B, 4)
    return out, ca, cb


def assert_same(got, ref, what=''):
    for k in INT_KEYS:
        bad = np.nonzero(np.asarray(got[k] != ref[k]).reshape(len(ref[k]), -1).any(axis=1))[0]
        assert bad.size == 0, (what, k, bad[:8], np.asarray(got[k])[bad[:4]], np.asarray(ref[k])[bad[:4]])
    diff = (got['pos'].view(np.int32) != ref['pos'].view(np.int32)).any(axis=1)
    print(f'{what}: {int(diff.sum())} of {len(diff)} coordinate rows differ from the restatement')
    assert not diff.any(), (what, 'pos', np.nonzero(diff)[0][:8])


def staged(dev, ligs, largest=False):
    """Perceive and sanitise on the GPU: pos, ptr, mol, san as numpy."""
    pos, feat, ptr = concat(ligs)
    perceived, _ = perceive_gpu(dev, pos, feat, ptr)
    mol = mol_of(perceived)
    return pos, ptr, mol, sanitize_gpu(dev, pos, ptr, mol, largest)


def run_both(dev, ligs, largest=False, edit=None, **caps):
    pos, ptr, mol, san = staged(dev, ligs, largest)
    if edit is not None:
        pos, ptr = edit(mol, san, pos, ptr) or (pos, ptr)
    got, ca, cb = add_hs_gpu(dev, pos, ptr, mol, san, largest, **caps)
    ref = HR.add_hs_batch(pos, ptr, mol, san, HC.Z_H, HC.ALLOWED_H, HC.H_CLASS, largest, cap_atoms=ca, cap_bonds=cb)
    return got, ref, mol, san, pos, ptr


SMALL = [(sym, p) for _, sym, p, _, _ in HC.SMALL]
TEXTBOOK = [(sym, p) for _, sym, p, _ in SC.TEXTBOOK]


# ---- 1. the kernel against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('largest', [False, True])
def test_small_textbook_and_generated_match(cuda, largest):
    ligs = SMALL + TEXTBOOK + [(sym, p) for sym, p, _ in SC.generated(48)]
    got, ref, _, _, _, _ = run_both(cuda, ligs, largest)
    assert_same(got, ref, f'molecules, largest_only={largest}')
    assert got['n_h'][:22].tolist() == [c[3] for c in HC.SMALL] and not got['status'][:22 + 18].any()


@pytest.mark.parametrize('largest', [False, True])
def test_random_clouds_match(cuda, largest):
    got, ref, _, _, _, _ = run_both(cuda, random_batch(), largest)
    assert_same(got, ref, f'clouds, largest_only={largest}')
    assert (got['status'] & HR.GENERAL).any() and (got['n_h'] > 0).sum() > 100       # the clouds reach the general rule


# ---- 2. edge inputs ----------------------------------------------------------------------------------------------------------------
def hand_written(pos, bonds, order_k, valence_k, atom_h):
    n = len(pos)
    mol = dict(elem=np.zeros(n, dtype=np.int64), frag=np.zeros(n, dtype=np.int64), bonds=np.array(bonds).reshape(-1, 2),
               order=np.array(order_k), bond_ptr=np.array([0, len(bonds)]), status=np.zeros(1, dtype=np.int64))
    san = dict(order_k=np.array(order_k), valence_k=np.array(valence_k), atom_h=np.array(atom_h), atom_flags=np.zeros(n, dtype=np.int64),
               status=np.zeros(1, dtype=np.int64))
    return np.asarray(pos, dtype=np.float32), np.array([0, n]), mol, san


def test_coincident_neighbour_sets_bit_3(cuda):
    pos, ptr, mol, san = hand_written([[0, 0, 0], [1.53, 0, 0], [0, 0, 0]], [[0, 1], [0, 2]], [1, 1], [2, 1, 1], [2, 3, 3])
    got, ca, cb = add_hs_gpu(cuda, pos, ptr, mol, san)
    ref = HR.add_hs_batch(pos, ptr, mol, san, HC.Z_H, HC.ALLOWED_H, HC.H_CLASS, cap_atoms=ca, cap_bonds=cb)
    assert_same(got, ref, 'coincident neighbour')
    assert got['status'].tolist() == [HR.GENERAL] and got['n_h'].tolist() == [8] and ref['mols'][0]['coincident'] == {0, 2}


def test_nan_coordinate_is_copied_through(cuda):
    def poison(mol, san, pos, ptr):
        pos = np.array(pos)
        pos[int(ptr[1]) + 1, 2] = np.nan
        pos[int(ptr[3]), 0] = np.inf
        return pos, ptr
    got, ref, _, _, _, ptr = run_both(cuda, TEXTBOOK[:5], edit=poison)
    assert got['status'].tolist() == [0, HR.NONFINITE, 0, HR.NONFINITE, 0] and got['n_h'].tolist() == [6, 0, 5, 0, 4]
    for k in INT_KEYS:
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got['pos'].view(np.int32), ref['pos'].view(np.int32))       # the NaN and the Inf are copied bit for bit


def test_atom_h_out_of_range_is_no_molecule(cuda):
    for value in (5, -1):
        def edit(mol, san, pos, ptr):
            san['atom_h'][int(ptr[1])] = value
        got, ref, _, _, _, _ = run_both(cuda, SMALL[13:16], edit=edit)
        assert_same(got, ref, f'atom_h = {value}')
        assert got['status'].tolist() == [0, HR.NO_MOLECULE, 0] and got['n_h'].tolist() == [8, 0, 6]


def test_empty_left_out_and_malformed_ligands(cuda):
    rng = np.random.default_rng(5)
    from .test_molecule_gpu import cloud
    ligs = [cloud(rng, n) for n in (1, 0, 64, 65, 257, 2)] + SMALL[5:8]
    got, ref, _, _, _, _ = run_both(cuda, ligs)
    assert_same(got, ref, 'sizes')
    assert got['status'][1] == HR.NO_MOLECULE and got['status'][4] == HR.NO_MOLECULE and got['n_h'][4] == 0
    assert got['out_ptr'][5] - got['out_ptr'][4] == 257                      # more than 256 atoms: the rows are copied, nothing else

    def bad_ptr(mol, san, pos, ptr):                # ligand 0 starts below 0, ligand 1 ends beyond the atoms, ligand 2 ends before it starts
        ptr = np.array(ptr)
        ptr[0], ptr[2] = -1, 100000
        return pos, ptr
    got, ref, _, _, _, _ = run_both(cuda, TEXTBOOK[:5], edit=bad_ptr)
    assert_same(got, ref, 'malformed lig_ptr')
    assert got['status'].tolist() == [HR.NO_MOLECULE] * 3 + [0, 0] and got['out_ptr'].tolist()[:4] == [0, 0, 0, 0]

    def graphs(mol, san, pos, ptr):                 # no output of perceive: rows out of order, order_k 0, a bond that leaves the ligand
        bp = mol['bond_ptr']
        mol['bonds'][[bp[0], bp[0] + 1]] = mol['bonds'][[bp[0] + 1, bp[0]]]
        san['order_k'][bp[1]] = 0
        mol['bonds'][bp[3]] = [ptr[3], ptr[4] + 1]
        mol['bond_ptr'][5] = 10 ** 6                # and a bond range beyond the list: no bonds are copied
    got, ref, _, _, _, _ = run_both(cuda, TEXTBOOK[:5], edit=graphs)
    assert_same(got, ref, 'hand-written graphs')
    assert got['status'].tolist() == [1, 1, 0, 1, 1] and got['summary'][4].tolist() == [0, 0, 0, 0]


def test_capacity_too_small_by_one(cuda):
    pos, ptr, mol, san = staged(cuda, SMALL[13:17])
    full, ca, cb = add_hs_gpu(cuda, pos, ptr, mol, san)
    need_a, need_b = int(full['out_ptr'][-1]), int(full['out_bond_ptr'][-1])
    assert not full['status'].any() and need_a <= ca and need_b <= cb
    for caps in (dict(cap_atoms=need_a - 1, cap_bonds=need_b), dict(cap_atoms=need_a, cap_bonds=need_b - 1)):
        got, ca, cb = add_hs_gpu(cuda, pos, ptr, mol, san, **caps)
        ref = HR.add_hs_batch(pos, ptr, mol, san, HC.Z_H, HC.ALLOWED_H, HC.H_CLASS, **caps)
        assert_same(got, ref, f'capacity {caps}')
        assert got['status'].tolist() == [0, 0, 0, HR.NO_ROOM] and got['out_ptr'][-1] == need_a and got['out_bond_ptr'][-1] == need_b
        assert (got['elem'][int(got['out_ptr'][3]):] == -1).all()            # the ligand that does not fit is not written
    for caps in (dict(cap_atoms=need_a + 1001, cap_bonds=need_b + 778), dict(cap_atoms=need_a + 2, cap_bonds=need_b),
                 dict(cap_atoms=3, cap_bonds=need_b + 5), dict(cap_atoms=1, cap_bonds=1)):
        got, ca, cb = add_hs_gpu(cuda, pos, ptr, mol, san, **caps)          # the rows behind the last ligand, and of every ligand that
        ref = HR.add_hs_batch(pos, ptr, mol, san, HC.Z_H, HC.ALLOWED_H, HC.H_CLASS, **caps)      # does not fit, read 0 / -1
        assert_same(got, ref, f'capacity {caps}')
        assert got['out_ptr'][-1] == need_a and got['out_bond_ptr'][-1] == need_b


def test_the_cap_of_256_atoms(cuda):
    got, ref, _, _, _, _ = run_both(cuda, [HC.carbon_chain(84), HC.carbon_chain(85)])
    assert_same(got, ref, 'chains')
    assert got['status'].tolist() == [0, HR.TOO_MANY_ATOMS] and got['n_h'].tolist() == [170, 0] and got['out_ptr'].tolist() == [0, 254, 339]


# ---- 3. independence of the batch and of the repeat ---------------------------------------------------------------------------------
def test_alone_in_a_batch_elsewhere_and_again(cuda):
    ligs = SMALL + TEXTBOOK
    pos, ptr, mol, san = staged(cuda, ligs)
    whole, _, _ = add_hs_gpu(cuda, pos, ptr, mol, san)
    again, _, _ = add_hs_gpu(cuda, pos, ptr, mol, san)
    for k in INT_KEYS:
        assert np.array_equal(whole[k], again[k]), k
    assert np.array_equal(whole['pos'].view(np.int32), again['pos'].view(np.int32))
    rev = list(reversed(ligs))
    turned, _, _ = add_hs_gpu(cuda, *staged(cuda, rev))
    B = len(ligs)
    for b in (0, 9, 18, 30, B - 1):
        alone, _, _ = add_hs_gpu(cuda, *staged(cuda, [ligs[b]]))
        w, a, t = HC.ligand(whole, b), HC.ligand(alone, 0), HC.ligand(turned, B - 1 - b)
        for k in ('elem', 'bonds', 'order', 'parent', 'frag', 'valence'):
            assert np.array_equal(w[k], a[k]) and np.array_equal(w[k], t[k]), (b, k)
        assert np.array_equal(w['pos'].view(np.int32), a['pos'].view(np.int32)) and np.array_equal(w['pos'].view(np.int32), t['pos'].view(np.int32)), b
        for k in ('summary', 'n_h', 'status'):
            assert np.array_equal(whole[k][b], alone[k][0]) and np.array_equal(whole[k][b], turned[k][B - 1 - b]), (b, k)


# ---- 4. the Python surface, and through the existing calls ------------------------------------------------------------------------------
def build(dev, ligs):
    return molecule.build_molecules([torch.from_numpy(np.asarray(p, dtype=np.float32)).to(dev) for _, p in ligs],
                                    [torch.from_numpy(one_hot(sym)).to(dev) for sym, _ in ligs], ELEMENTS)


@pytest.fixture(scope='module')
def hydrogenated(cuda):
    san = build(cuda, TEXTBOOK).sanitize()
    return san, san.add_hs()


def test_hydrogenated_surface_and_sdf(cuda, hydrogenated):
    san, hyd = hydrogenated
    m = hyd.molecules
    assert m.lig_elements == ELEMENTS + ['H'] and hyd.heavy is san.molecules and len(m) == len(TEXTBOOK) and not hyd.status.any()
    n_h = hyd.n_h.tolist()
    assert n_h == san.descriptors()['n_h'].tolist() and int(hyd.is_h.sum()) == sum(n_h)
    assert m._sizes == [len(sym) + h for (sym, _), h in zip(TEXTBOOK, n_h)] and m._max_atoms == max(m._sizes)
    assert torch.equal(m.pos[~hyd.is_h], san.molecules.pos) and torch.equal(hyd.source[~hyd.is_h], torch.arange(len(san.h), device=cuda, dtype=torch.int32))
    assert bool((~hyd.is_h[hyd.parent[hyd.is_h].long()]).all()) and m.valid is san.valid
    blocks = hyd.sdf()
    assert blocks == m.sdf()
    for (sym, _), h, block, nb in zip(TEXTBOOK, n_h, blocks, san.molecules.summary[:, 0].tolist()):
        lines = block.splitlines()
        n = len(sym) + h
        assert (int(lines[3][:3]), int(lines[3][3:6])) == (n, nb + h)
        assert [ln[31:34].strip() for ln in lines[4:4 + n]] == list(sym) + ['H'] * h
    # a second hydrogen class is not added, and the existing one is used
    again = hyd.molecules.sanitize().add_hs()
    assert again.molecules.lig_elements == ELEMENTS + ['H'] and not again.n_h.any()
    # a ligand that is copied through: the rows sized for its hydrogens are trimmed away
    mixed = build(cuda, [HC.carbon_chain(85), TEXTBOOK[0]]).sanitize().add_hs()
    assert mixed.status.tolist() == [hip.HS_TOO_MANY_ATOMS, 0] and mixed.n_h.tolist() == [0, 6]
    assert mixed.molecules.pos.shape[0] == 85 + 12 == int(mixed.molecules.lig_ptr[-1]) and int(mixed.is_h.sum()) == 6
    assert [int(b.splitlines()[3][:3]) for b in mixed.sdf()] == [85, 12]
    # the validity entry of the appended class is the caller's, if the caller's table has one
    ligs = TEXTBOOK[:1]
    own = molecule.build_molecules([torch.from_numpy(np.asarray(p, dtype=np.float32)).to(cuda) for _, p in ligs],
                                   [torch.from_numpy(one_hot(sym)).to(cuda) for sym, _ in ligs], ELEMENTS,
                                   allowed_bonds=dict(molecule.ALLOWED_BONDS, H=0)).sanitize().add_hs()
    assert own.molecules._allowed[-1] == 0 and own.molecules.summary[0].tolist() == [12, 1, 12, 6]       # every H counts as invalid
    assert m._allowed[-1] == molecule.ALLOWED_BONDS['H'] and m.summary[0].tolist() == [12, 1, 12, 0]
    empty = molecule.build_molecules([], [], ELEMENTS)
    empty.pos = torch.zeros(0, 3, device=cuda)
    e = empty.sanitize().add_hs()
    assert len(e.molecules) == 0 and e.n_h.numel() == 0 and e.molecules.sdf() == [] and e.is_h.numel() == 0


# Kekule structures that are not images of one another under the molecule's symmetry: kpd_mol_sanitize picks the lexicographically
# first optimum in bond rows, so the pattern, and with it the key WITH orders, may move under renumbering (sections 15, 16)
FUSED = ('naphthalene', 'anthracene', 'phenanthrene', 'pyrene', 'indole')


def test_keys_of_rotated_and_permuted_copies(cuda):
    rng = np.random.default_rng(3)
    turned = []
    for sym, p in TEXTBOOK:
        perm = rng.permutation(len(sym))
        A = np.linalg.qr(rng.standard_normal((3, 3)))[0]
        turned.append(([sym[i] for i in perm], (np.asarray(p)[perm] @ A.T + 2.0).astype(np.float32)))
    a, b = build(cuda, TEXTBOOK).sanitize().add_hs(), build(cuda, turned).sanitize().add_hs()
    assert a.n_h.tolist() == b.n_h.tolist() and not a.status.any() and not b.status.any()
    ka, kb, ha, hb = a.molecules.keys().tolist(), b.molecules.keys().tolist(), a.heavy.keys().tolist(), b.heavy.keys().tolist()
    single = [k for k, c in enumerate(SC.TEXTBOOK) if c[0] not in FUSED]
    assert len(single) == 13
    for k in single:                                # every Kekule structure is an image of the others: the default key (with orders) is equal
        assert ka[k] == kb[k], SC.TEXTBOOK[k][0]
    for k in range(len(TEXTBOOK)):                  # fused ones too: the hydrogens never split what the sanitiser's pattern left equal
        assert (ka[k] == kb[k]) == (ha[k] == hb[k]), SC.TEXTBOOK[k][0]
    print('keys with orders differ between the copies for', [SC.TEXTBOOK[k][0] for k in range(len(TEXTBOOK)) if ka[k] != kb[k]])
    assert torch.equal(a.molecules.keys(with_orders=False), b.molecules.keys(with_orders=False))      # all 18, the fused ones among them
    assert all(x != y for x, y in zip(ka, ha))      # and a hydrogenated molecule is another graph than its heavy atoms


def test_sanitising_the_hydrogenated_molecules_again(cuda, hydrogenated):
    san, hyd = hydrogenated
    again = hyd.molecules.sanitize()
    d0, d1 = san.descriptors(), again.descriptors()
    assert not again.h.any() and not again.status.any()
    for name in ('n_heavy', 'n_rot', 'n_rings', 'n_arom_rings', 'n_arom_atoms', 'n_cycles'):
        assert torch.equal(d0[name], d1[name]), name
    assert torch.equal(d0['mw'].view(torch.int64), d1['mw'].view(torch.int64))
    assert torch.equal(again.aromatic_atoms[~hyd.is_h], san.aromatic_atoms) and not again.aromatic_atoms[hyd.is_h].any()
    heavy_rows = ~hyd.is_h[hyd.molecules.bonds[:, 1].clamp(min=0).long()] & (hyd.molecules.bonds[:, 1] >= 0)
    total = int(san.molecules.bond_ptr[-1])
    assert torch.equal(again.molecules.order[heavy_rows], san.molecules.order[:total])
    assert bool((again.valid | ~san.valid).all())


def test_relax_keeps_the_x_h_lengths(cuda, hydrogenated):
    _, hyd = hydrogenated
    m = hyd.molecules
    far = torch.full((1, 3), 100.0, device=cuda)
    r = m.relax([far], [['C']], pocket_of=[-1] * len(m))
    assert not (r.status & (hip.RELAX_NO_MOLECULE | hip.RELAX_BAD_INPUT)).any()
    e0, e1 = r.report[:, hip.RELAX_REPORT.index('E_before')], r.report[:, hip.RELAX_REPORT.index('E_after')]
    assert bool((e1 <= e0).all())
    h_rows = hyd.is_h.nonzero().flatten()
    par = hyd.parent[h_rows].long()
    zt = torch.tensor(HC.Z_H, device=cuda)
    L = torch.tensor([HR.bond_length(int(zz)) for zz in zt[m.elem[par].long()].tolist()], dtype=torch.float64, device=cuda)
    for pos in (m.pos, r.molecules.pos):
        d = (pos[h_rows].double() - pos[par].double()).norm(dim=1)
        assert float((d - L).abs().max()) < (2e-6 if pos is m.pos else 0.05)


def test_vina_score_ignores_the_hydrogens(cuda, hydrogenated):
    san, hyd = hydrogenated
    rng = np.random.default_rng(9)
    centre = san.molecules.pos.mean(0).cpu().numpy()
    pocket = [torch.from_numpy((centre + rng.standard_normal((40, 3)) * 4.0).astype(np.float32)).to(cuda)]
    psym = [['C', 'N', 'O', 'S'][k % 4] for k in range(40)]
    kw = dict(pocket_of=[0] * len(TEXTBOOK), radii={'B': 1.9})
    heavy, full = san.molecules.vina_score(pocket, [psym], **kw), hyd.molecules.vina_score(pocket, [psym], **kw)
    assert torch.equal(full.lig_types[~hyd.is_h], heavy.lig_types) and bool((full.lig_types[hyd.is_h] == -1).all())
    n_rot = hip.VINA_REPORT.index('n_rot')
    assert torch.equal(full.report[:, n_rot], heavy.report[:, n_rot])
    terms = heavy.report[:, 2:7].abs().sum(1)
    for col in range(7):
        err = (full.report[:, col] - heavy.report[:, col]).abs()
        print(hip.VINA_REPORT[col], 'largest difference', float(err.max()))
        assert bool((err <= 1e-10 * terms).all()), hip.VINA_REPORT[col]


def samples_of(ligs):
    return [dict(positions=[torch.from_numpy(np.asarray(p, dtype=np.float32)) for _, p in ligs],
                 features=[torch.from_numpy(one_hot(sym)) for sym, _ in ligs])]


def test_keyword_paths_end_to_end(cuda, tmp_path):
    rng = np.random.default_rng(21)
    ligs = []
    while len(ligs) < 2:                            # two 12-atom samples of the seeded generator
        sym, pos, _ = SC.generate(int(rng.integers(0, 10 ** 6)))
        if len(sym) == 12:
            ligs.append((sym, pos))
    samples = samples_of(ligs)
    pocket = dict(positions=torch.from_numpy((np.asarray(ligs[0][1]).mean(0) + rng.standard_normal((30, 3)) * 6.0).astype(np.float32)),
                  elements=['C', 'N', 'O'] * 10)
    plain = molecule.relax_samples(samples, [pocket], ELEMENTS, device=cuda, max_iters=50)
    with_h = molecule.relax_samples(samples, [pocket], ELEMENTS, device=cuda, max_iters=50, add_hs=True)
    hyd = molecule.hydrogenate_samples(samples, ELEMENTS, device=cuda)
    assert plain.molecules.lig_elements == ELEMENTS and with_h.molecules.lig_elements == ELEMENTS + ['H']
    assert with_h._sizes == [12 + h for h in hyd.n_h.tolist()] and sum(hyd.n_h.tolist()) > 0
    assert not (with_h.status & (hip.RELAX_NO_MOLECULE | hip.RELAX_BAD_INPUT)).any()
    assert torch.equal(plain.molecules.pos, molecule.relax_samples(samples, [pocket], ELEMENTS, device=cuda, max_iters=50, add_hs=False).molecules.pos)
    pos, feat = [p.to(cuda) for p in samples[0]['positions']], [f.to(cuda) for f in samples[0]['features']]
    heavy_blocks = molecule.build_molecules(pos, feat, ELEMENTS).sdf()
    assert utils.sampled_ligands_sdf(pos, feat, ELEMENTS) == heavy_blocks == utils.sampled_ligands_sdf(pos, feat, ELEMENTS, add_hs=False)
    blocks = utils.sampled_ligands_sdf(pos, feat, ELEMENTS, add_hs=True)
    assert blocks == hyd.sdf() and all(int(b.splitlines()[3][:3]) == 12 + h for b, h in zip(blocks, hyd.n_h.tolist()))
    utils.write_sdf_file(tmp_path / 'h.sdf', pos, feat, ELEMENTS, add_hs=True)
    utils.write_sdf_file(tmp_path / 'heavy.sdf', pos, feat, ELEMENTS)
    assert (tmp_path / 'h.sdf').read_text() == ''.join(blocks) and (tmp_path / 'heavy.sdf').read_text() == ''.join(heavy_blocks)


def test_host_tensor_raises(cuda):
    san = build(cuda, TEXTBOOK[:1]).sanitize()
    m = san.molecules
    with pytest.raises(hip.KpdError):
        hip.mol_add_hs(m.pos.cpu(), m.lig_ptr, HC.Z_H, HC.ALLOWED_H, HC.H_CLASS,
                       dict(elem=m.elem, frag=m.frag, bonds=m.bonds, bond_ptr=m.bond_ptr, status=m.status), san._out)
    with pytest.raises(hip.KpdError):
        hip.mol_add_hs(m.pos, m.lig_ptr, HC.Z_H, HC.ALLOWED_H, 0,
                       dict(elem=m.elem, frag=m.frag, bonds=m.bonds, bond_ptr=m.bond_ptr, status=m.status), san._out)
    m.pos = m.pos.cpu()
    with pytest.raises(hip.KpdError):
        san.add_hs()
    with pytest.raises(hip.KpdError):
        molecule.hydrogenate_samples(samples_of(TEXTBOOK[:1]), ELEMENTS)
