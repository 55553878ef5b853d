"""The one check of molecule arguments in hip.py (`_mol_args`, lengths in hip.MOL_LENGTHS / hip.SAN_LENGTHS): every wrapper that
takes what `mol_perceive` / `mol_sanitize` returned accepts the real thing and refuses, with KpdError and before anything is
launched, each entry it names when that entry is one element short, int64 or a strided view.  The library cannot see a tensor's
length, so a short entry that got through would be read past its end by a kernel."""
from types import SimpleNamespace

import pytest
import torch

from keypoint_diffusion_amd import hip, molecule

pytestmark = pytest.mark.gpu

ELEMENTS = ['C', 'N', 'O']
Z = [6, 7, 8]
ALLOWED = [4, 3, 2]
MOL6 = ('elem', 'frag', 'bonds', 'order', 'bond_ptr', 'status')
MOL5 = ('elem', 'frag', 'bonds', 'bond_ptr', 'status')
SAN_HS = ('order_k', 'valence_k', 'atom_h', 'atom_flags', 'status')
SAN_FLAGS = ('order_k', 'bond_flags', 'atom_h', 'atom_flags', 'status')


@pytest.fixture(scope='module')
def batch(cuda):
    """B = 2 ligands, N = 4 atoms: the chain C-C-O and a lone C, perceived into a bond list of 3 N = 12 rows (2 used), sanitised;
    one pocket of two atoms; K = 2 poses."""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=cuda)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=cuda)
    a = SimpleNamespace(pos=f32([[0, 0, 0], [1.54, 0, 0], [2.14, 1.3, 0], [10, 0, 0]]), lig_ptr=i32([0, 3, 4]))
    feat = f32([[1, 0, 0], [1, 0, 0], [0, 0, 1], [1, 0, 0]])
    a.mol = hip.mol_perceive(a.pos, feat, a.lig_ptr, Z, ALLOWED)
    mass, mass_h = molecule.mass_table(ELEMENTS)
    a.san = hip.mol_sanitize(a.pos, a.lig_ptr, Z, ALLOWED, mass, mass_h, a.mol)
    a.stack = torch.stack([a.pos, a.pos + 0.05])
    a.pocket_x, a.pocket_ptr, a.pocket_of = f32([[0.5, 4, 0], [2.5, 4.5, 0.5]]), i32([0, 2]), i32([0, 0])
    a.pocket_type, _ = hip.vina_pocket_types(a.pocket_x, i32([6, 8]), a.pocket_ptr)
    a.lig_vdw, a.pocket_vdw = f32(molecule.vdw_table(ELEMENTS)), f32(molecule.vdw_table(['C', 'O']))
    a.xs, a.pocket_xs = f32(molecule.xs_radius_table(ELEMENTS)), f32(molecule.xs_radius_table(['C', 'O']))
    a.vdw_r, a.pocket_vdw_r = f32(molecule.vdw_radius_table(ELEMENTS)), f32(molecule.vdw_radius_table(['C', 'O']))
    a.box_lo, a.box_hi = f32([[-3, -3, -3], [7, -3, -3]]), f32([[5, 4, 3], [13, 3, 3]])
    torch.cuda.synchronize()
    assert a.mol['bonds'].shape == (12, 2) and a.mol['bond_ptr'].tolist() == [0, 2, 2] and a.mol['status'].tolist() == [0, 0]
    return a


def pockets(a, radius):
    return dict(pocket_x=a.pocket_x, pocket_radius=radius, pocket_ptr=a.pocket_ptr, pocket_of=a.pocket_of)


# wrapper -> (the call on a batch with `mol` and `san` replaced, the entries of mol it names, the entries of san it names)
CALLS = {
    'sdf_emit': (lambda a, mol, san: hip.sdf_emit(a.pos, a.lig_ptr, ELEMENTS, mol), MOL6, ()),
    'mol_keys': (lambda a, mol, san: hip.mol_keys(a.lig_ptr, Z, mol), MOL6, ()),
    'mol_sanitize': (lambda a, mol, san: hip.mol_sanitize(a.pos, a.lig_ptr, Z, ALLOWED, *molecule.mass_table(ELEMENTS), mol), MOL6, ()),
    'mol_add_hs': (lambda a, mol, san: hip.mol_add_hs(a.pos, a.lig_ptr, Z + [1], ALLOWED + [1], 3, mol, san), MOL5, SAN_HS),
    'mol_smiles': (lambda a, mol, san: hip.mol_smiles(a.lig_ptr, Z, ELEMENTS, mol, san), MOL5, SAN_FLAGS),
    'pose_rmsd': (lambda a, mol, san: hip.pose_rmsd(a.lig_ptr, Z, mol, a.stack, a.pos), MOL5, ()),
    'pose_check': (lambda a, mol, san: hip.pose_check(a.lig_ptr, Z, mol, san, a.stack, a.vdw_r, **pockets(a, a.pocket_vdw_r)), MOL5, SAN_FLAGS),
    'relax': (lambda a, mol, san: hip.relax(a.pos, a.lig_ptr, Z, a.lig_vdw, mol, a.pocket_x, a.pocket_vdw, a.pocket_ptr, a.pocket_of,
                                            max_iters=3), ('elem', 'bonds', 'bond_ptr', 'status'), ()),
    'vina_score': (lambda a, mol, san: hip.vina_score(a.pos, a.lig_ptr, Z, a.xs, mol, a.pocket_x, a.pocket_xs, a.pocket_type, a.pocket_ptr,
                                                      a.pocket_of), ('elem', 'bonds', 'order', 'bond_ptr', 'status'), ()),
    'vina_minimize': (lambda a, mol, san: hip.vina_minimize(a.pos, a.lig_ptr, Z, a.xs, mol, a.pocket_x, a.pocket_xs, a.pocket_type,
                                                            a.pocket_ptr, a.pocket_of, max_iters=3), MOL6, ()),
    'vina_dock': (lambda a, mol, san: hip.vina_dock(a.pos, a.lig_ptr, Z, a.xs, mol, a.pocket_x, a.pocket_xs, a.pocket_type, a.pocket_ptr,
                                                    a.pocket_of, a.box_lo, a.box_hi, n_chains=2, n_steps=2, max_iters=2, step_iters=2),
                  MOL6, ()),
}
BAD = {
    'one element short': lambda t: t.flatten()[:-1],
    'int64': lambda t: t.long(),
    'a strided view': lambda t: torch.stack([t.flatten(), t.flatten()], dim=1)[:, 0],      # as many elements, every other one of its storage
}


@pytest.mark.parametrize('wrapper', list(CALLS))
def test_the_real_arguments_are_accepted(batch, wrapper):
    CALLS[wrapper][0](batch, batch.mol, batch.san)
    torch.cuda.synchronize()


@pytest.mark.parametrize('wrapper', list(CALLS))
def test_every_named_entry_is_checked(batch, wrapper):
    call, fields, san_fields = CALLS[wrapper]
    for which, names in (('mol', fields), ('san', san_fields)):
        for name in names:
            for how, spoil in BAD.items():
                args = dict(mol=dict(batch.mol), san=dict(batch.san))
                args[which][name] = spoil(args[which][name])
                assert how != 'a strided view' or not args[which][name].is_contiguous()
                with pytest.raises(hip.KpdError):
                    call(batch, args['mol'], args['san'])
                    pytest.fail(f'{wrapper} accepted {which}[{name!r}] {how}')


@pytest.mark.parametrize('wrapper', ['pose_rmsd', 'relax'])
def test_an_odd_bond_list_is_refused(batch, wrapper):
    """One element too many: nothing would be read past its end, but the list no longer holds two atoms per row."""
    bonds = torch.cat([batch.mol['bonds'].flatten(), batch.mol['bonds'].new_zeros(1)])
    with pytest.raises(hip.KpdError):
        CALLS[wrapper][0](batch, dict(batch.mol, bonds=bonds), batch.san)


def test_pose_check_without_pockets_and_with_one_pose(batch):
    a = batch
    with_pockets = hip.pose_check(a.lig_ptr, Z, a.mol, a.san, a.stack, a.vdw_r, **pockets(a, a.pocket_vdw_r))
    without = hip.pose_check(a.lig_ptr, Z, a.mol, a.san, a.stack, a.vdw_r)
    one = hip.pose_check(a.lig_ptr, Z, a.mol, a.san, a.stack[:1], a.vdw_r, **pockets(a, a.pocket_vdw_r))
    flat = hip.pose_check(a.lig_ptr, Z, a.mol, a.san, a.pos, a.vdw_r, **pockets(a, a.pocket_vdw_r))
    torch.cuda.synchronize()
    col = hip.CHECK_COUNTS.index('pocket_pairs')
    assert with_pockets['fail'].shape == without['fail'].shape == (2, 2) and one['fail'].shape == (2, 1)
    assert int(with_pockets['counts'][0, 0, col]) > 0 and not without['counts'][:, :, col].any()
    assert (with_pockets['status'] == 0).all() and (without['status'] == 0).all()
    with pytest.raises(hip.KpdError):                           # the four pocket arguments come together
        hip.pose_check(a.lig_ptr, Z, a.mol, a.san, a.stack, a.vdw_r, pocket_ptr=a.pocket_ptr)
    assert set(flat) == set(one)
    for k in one:                                               # [N,3] is the one pose [1,N,3]: bit for bit
        assert flat[k].shape == one[k].shape and torch.equal(flat[k].contiguous().view(torch.uint8), one[k].contiguous().view(torch.uint8)), k
