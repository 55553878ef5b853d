"""Molecules from sampled ligands on the GPU (kpd_mol_perceive, kpd_sdf_emit, keypoint_diffusion_amd.molecule) against the
float64 restatement of the rule in include/kpd.h (tests/molecule_ref.py) and against chemistry written out by hand
(tests/molecule_cases.py).  Every comparison is exact equality of integers and bytes: the rule needs no tolerance.
Every raw call runs with canary bytes behind each output buffer."""
import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import hip, molecule, utils
from . import molecule_ref as R
from .molecule_cases import ALLOWED, ELEMENTS, TEXTBOOK, TWO_ETHANOLS_CL, Z, one_hot
from .util import guarded, intact

pytestmark = pytest.mark.gpu
PAD, CANARY = 64, 0x5A


# ---- raw calls with canaries ------------------------------------------------------------------------------------------
class Guarded:
    """Output buffers with PAD canary elements behind each; `check` asserts that none was touched."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def new(self, n, dtype=torch.int32):
        t = torch.empty(n + PAD, dtype=dtype, device=self.dev)
        t.view(torch.uint8).fill_(CANARY)
        self.bufs.append((t, n))
        return t

    def check(self):
        for t, n in self.bufs:
            tail = t[n:].view(torch.uint8)
            assert bool((tail == CANARY).all()), f'canary after a buffer of {n} x {t.dtype} overwritten'


def ptr_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def perceive_gpu(dev, pos, feat, ptr, z=Z, allowed=ALLOWED, cap_bonds=None):
    """kpd_mol_perceive through the C ABI.  Returns (numpy outputs, device tensors for kpd_sdf_emit)."""
    pos_d = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float32)).reshape(-1, 3).to(dev)
    feat_d = torch.from_numpy(np.ascontiguousarray(feat, dtype=np.float32)).to(dev)
    ptr_d = torch.tensor(np.asarray(ptr), dtype=torch.int32, device=dev)
    N, B, F = pos_d.shape[0], len(ptr) - 1, feat_d.shape[1]
    cap = 3 * N if cap_bonds is None else cap_bonds
    g = Guarded(dev)
    o = dict(elem=g.new(N), valence=g.new(N), frag=g.new(N), bonds=g.new(2 * cap), order=g.new(cap), bond_ptr=g.new(B + 1),
             summary=g.new(4 * B), status=g.new(B))
    L = hip.lib()
    nb = int(L.kpd_mol_scratch_bytes(N, B))
    scratch, p_scr = guarded(nb, torch.uint8, dev, CANARY)                 # the scratch has a band on either side
    zt, at = torch.tensor(z, dtype=torch.int32, device=dev), torch.tensor(allowed, dtype=torch.int32, device=dev)
    hip.check(L.kpd_mol_perceive(pos_d.data_ptr(), feat_d.data_ptr(), ptr_d.data_ptr(), N, B, F, zt.data_ptr(), at.data_ptr(), cap,
                                 *[o[k].data_ptr() for k in ('elem', 'valence', 'frag', 'bonds', 'order', 'bond_ptr', 'summary', 'status')],
                                 p_scr, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    g.check()
    assert intact(scratch, nb, CANARY), f'kpd_mol_perceive wrote outside its {nb} bytes of scratch'
    sizes = dict(elem=N, valence=N, frag=N, bonds=2 * cap, order=cap, bond_ptr=B + 1, summary=4 * B, status=B)
    dev_t = {k: o[k][:n] for k, n in sizes.items()}
    dev_t['bonds'] = dev_t['bonds'].reshape(cap, 2)
    out = {k: v.cpu().numpy().astype(np.int64) for k, v in dev_t.items()}
    out['summary'] = out['summary'].reshape(B, 4)
    dev_t.update(pos=pos_d, ptr=ptr_d, cap=cap)
    return out, dev_t


def sdf_gpu(dev, t, elements=ELEMENTS, largest=False, capacity=None):
    """kpd_sdf_emit through the C ABI on what perceive_gpu left on the device.  Returns (blocks, status, text_ptr)."""
    N, B = t['pos'].shape[0], t['ptr'].numel() - 1
    cap = 70 * N + 13 * t['cap'] + 77 * B if capacity is None else capacity
    g = Guarded(dev)
    text, tptr, status = g.new(cap, torch.uint8), g.new(B + 1, torch.int64), g.new(B)
    L = hip.lib()
    nb = int(L.kpd_sdf_scratch_bytes(N, B))
    scratch, p_scr = guarded(nb, torch.uint8, dev, CANARY)
    sym = hip._packed_symbols(elements, dev, 3)
    hip.check(L.kpd_sdf_emit(t['pos'].data_ptr(), t['ptr'].data_ptr(), N, B, t['elem'].data_ptr(), len(elements), sym.data_ptr(),
                             t['frag'].data_ptr(), t['bonds'].data_ptr(), t['order'].data_ptr(), t['bond_ptr'].data_ptr(), t['cap'],
                             t['status'].data_ptr(), int(largest), text.data_ptr(), cap, tptr.data_ptr(), status.data_ptr(),
                             p_scr, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    g.check()
    assert intact(scratch, nb, CANARY), f'kpd_sdf_emit wrote outside its {nb} bytes of scratch'
    p = tptr[:B + 1].cpu().tolist()
    raw = bytes(text[:cap].cpu().numpy())
    st = status[:B].cpu().tolist()
    blocks = [raw[p[b]:p[b + 1]].decode('ascii') if not st[b] else '' for b in range(B)]
    return blocks, st, p


def assert_equal(got, ref, what=''):
    for k in ('elem', 'valence', 'frag', 'bond_ptr', 'summary', 'status'):
        assert np.array_equal(got[k], ref[k]), (what, k, np.nonzero(np.asarray(got[k] != ref[k]).reshape(len(ref[k]), -1).any(axis=1))[0][:8])
    w = ref['written'][:len(got['order'])]
    assert np.array_equal(got['bonds'][w], ref['bonds'][:len(w)][w]), (what, 'bonds')
    assert np.array_equal(got['order'][w], ref['order'][:len(w)][w]), (what, 'order')


def concat(ligs):
    """[(symbols or features, pos)] -> pos, feat, ptr."""
    feats = [one_hot(f) if isinstance(f[0], str) else np.asarray(f, dtype=np.float32) for f, _ in ligs if len(f)]
    pos = [np.asarray(p, dtype=np.float32).reshape(-1, 3) for _, p in ligs]
    feat = np.concatenate(feats) if feats else np.zeros((0, len(ELEMENTS)), dtype=np.float32)
    return np.concatenate(pos), feat, ptr_of([len(p) for p in pos])


def cloud(rng, n, scale=1.6, pool=('C', 'C', 'C', 'N', 'O', 'S', 'Cl', 'F', 'P', 'Br')):
    """A normal cloud of n atoms, scale * (n / 20)^(1/3) A wide; one-hot features with a little noise under the maximum."""
    pos = (rng.standard_normal((n, 3)) * scale * (max(n, 1) / 20.0) ** (1.0 / 3.0)).astype(np.float32)
    sym = [pool[k] for k in rng.integers(0, len(pool), n)]
    feat = one_hot(sym) + (rng.random((n, len(ELEMENTS))) * 0.3).astype(np.float32) if n else np.zeros((0, len(ELEMENTS)), dtype=np.float32)
    return feat, pos


def random_batch(seed=2026, B=150):
    rng = np.random.default_rng(seed)
    return [cloud(rng, int(rng.integers(1, 61)), (1.0, 1.6, 2.2)[b % 3]) for b in range(B)]


@pytest.fixture(scope='module')
def parity():
    """The random batch and its restatement, computed once."""
    ligs = random_batch()
    pos, feat, ptr = concat(ligs)
    return dict(ligs=ligs, pos=pos, feat=feat, ptr=ptr, ref=R.perceive_batch(pos, feat, ptr, Z, ALLOWED))


# ---- 1. textbook fragments ----------------------------------------------------------------------------------------------
def test_textbook_fragments_by_hand(cuda):
    pos, feat, ptr = concat([(sym, p) for _, sym, p, _ in TEXTBOOK])
    got, _ = perceive_gpu(cuda, pos, feat, ptr)
    assert not got['status'].any()
    for b, (name, sym, p, bonds) in enumerate(TEXTBOOK):
        p0, p1, a0 = got['bond_ptr'][b], got['bond_ptr'][b + 1], ptr[b]
        found = {(int(i - a0), int(j - a0)): int(o) for (i, j), o in zip(got['bonds'][p0:p1], got['order'][p0:p1])}
        assert found == bonds, (name, found)
        assert list(got['bonds'][p0:p1].tolist()) == sorted(got['bonds'][p0:p1].tolist()), name
        val = np.zeros(len(sym), dtype=np.int64)
        for (i, j), o in bonds.items():
            val[i] += o
            val[j] += o
        assert np.array_equal(got['valence'][a0:a0 + len(sym)], val), name
        assert [ELEMENTS[e] for e in got['elem'][a0:a0 + len(sym)]] == sym, name
    by_name = {c[0]: b for b, c in enumerate(TEXTBOOK)}
    b = by_name['dimethyl sulfone']                        # S: valence 6, inside the rule's cap, above upstream's allowed 4
    assert got['valence'][ptr[b]] == 6 and got['summary'][b].tolist() == [4, 1, 5, 1]
    for name, lost in (('five neighbours, centre first', 4), ('five neighbours, centre last', 3)):
        b = by_name[name]                                   # the farthest neighbour ends isolated and invalid
        assert got['valence'][ptr[b] + lost] == 0 and got['summary'][b].tolist() == [4, 2, 5, 1], name
        assert got['frag'][ptr[b]:ptr[b + 1]].tolist() == ([0, 0, 0, 0, 1, 0] if lost == 4 else [0, 0, 0, 1, 0, 0]), name
    b = by_name['0.3 A apart']
    assert got['summary'][b].tolist() == [2, 1, 3, 0]
    assert got['summary'][by_name['ethanol']].tolist() == [2, 1, 3, 0]


def test_two_ethanols_and_a_chloride(cuda):
    sym, pos, bonds = TWO_ETHANOLS_CL
    got, _ = perceive_gpu(cuda, pos, one_hot(sym), ptr_of([7]))
    assert {(int(i), int(j)): int(o) for (i, j), o in zip(got['bonds'][:4], got['order'][:4])} == bonds
    assert got['bond_ptr'].tolist() == [0, 4] and got['frag'].tolist() == [0, 0, 0, 1, 1, 1, 2]
    assert got['summary'][0].tolist() == [4, 3, 3, 1] and got['status'].tolist() == [0]       # the lone Cl is the invalid atom
    m = molecule.build_molecules([torch.from_numpy(pos).to(cuda)], [torch.from_numpy(one_hot(sym)).to(cuda)], ELEMENTS)
    met = m.metrics()
    assert met['avg_frag_frac'] == 3 / 7 and met['connectivity'] == 0.0 and met['atom_validity'] == 1 - 1 / 7
    assert m.frag.tolist() == [0, 0, 0, 1, 1, 1, 2] and m.summary.tolist() == [[4, 3, 3, 1]]
    block = m.sdf(largest_frag=True)[0]
    assert block.splitlines()[3].startswith('  3  2') and block.count('\n') == 4 + 3 + 2 + 2


# ---- 2. random parity ---------------------------------------------------------------------------------------------------
def test_random_batch_exercises_every_rule_and_matches(cuda, parity):
    ref = parity['ref']
    orders = np.concatenate([m['order'] for m in ref['mols']])
    multi = sum(m['summary'][1] > 1 for m in ref['mols'])
    print('candidates', ref['stats']['candidates'], 'bonds', len(orders), 'pruned', ref['stats']['pruned'], 'double', int((orders == 2).sum()),
          'triple', int((orders == 3).sum()), 'demoted', ref['stats']['demoted'], 'ligands with several fragments', multi)
    # from the restatement alone: the batch exercised every rule
    assert ref['stats']['pruned'] >= 100 and ref['stats']['demoted'] >= 10
    assert (orders == 2).sum() >= 50 and (orders == 3).sum() >= 10 and multi >= 1
    got, _ = perceive_gpu(cuda, parity['pos'], parity['feat'], parity['ptr'])
    assert_equal(got, ref, 'random batch')


# ---- 3. shapes where it can go wrong ------------------------------------------------------------------------------------
def test_ligand_sizes_around_the_wave_and_the_limit(cuda):
    rng = np.random.default_rng(7)
    sizes = [0, 1, 2, 63, 64, 65, 255, 256, 257]
    pos, feat, ptr = concat([cloud(rng, n) for n in sizes])
    ref = R.perceive_batch(pos, feat, ptr, Z, ALLOWED)
    assert ref['status'].tolist()[0] == R.EMPTY and ref['status'].tolist()[-1] == R.BAD_SEGMENT and ref['stats']['pruned'] > 200
    got, t = perceive_gpu(cuda, pos, feat, ptr)
    assert_equal(got, ref, 'sizes')
    assert (got['elem'][ptr[-2]:] == -1).all() and got['summary'][-1].tolist() == [0, 0, 0, 0]       # 257 atoms: left out
    for largest in (False, True):
        blocks, st, _ = sdf_gpu(cuda, t, largest=largest)
        want, wst = R.sdf_batch(pos, ptr, ELEMENTS, ref, largest)
        assert st == wst and blocks == want, largest
        assert st[-1] == R.SDF_NO_MOLECULE and blocks[-1] == '' and blocks[0].splitlines()[3].startswith('  0  0')


def test_one_ligand_and_more_ligands_than_one_wave_of_workgroups(cuda):
    rng = np.random.default_rng(11)
    one = [cloud(rng, 23)]
    pos, feat, ptr = concat(one)
    got, _ = perceive_gpu(cuda, pos, feat, ptr)
    assert_equal(got, R.perceive_batch(pos, feat, ptr, Z, ALLOWED), 'B = 1')
    many = [cloud(rng, 1 + b % 5, 0.8) for b in range(6000)]          # 256 CUs hold at most a few thousand of these workgroups at once
    pos, feat, ptr = concat(many)
    ref = R.perceive_batch(pos, feat, ptr, Z, ALLOWED)
    assert ref['bond_ptr'][-1] > 3000
    got, t = perceive_gpu(cuda, pos, feat, ptr)
    assert_equal(got, ref, 'B = 6000')
    blocks, st, _ = sdf_gpu(cuda, t)
    want, wst = R.sdf_batch(pos, ptr, ELEMENTS, ref)
    assert st == wst and blocks == want
    # no ligands at all
    got, t = perceive_gpu(cuda, np.zeros((0, 3)), np.zeros((0, 10)), [0])
    assert got['bond_ptr'].tolist() == [0]
    assert sdf_gpu(cuda, t) == ([], [], [0])


def test_scratch_stays_inside_the_size_asked_for(cuda):
    """perceive_gpu / sdf_gpu put guard bands on both sides of exactly kpd_*_scratch_bytes and assert them untouched: a batch
    whose every scratch buffer is used to its last element (3 n bond rows are reserved, the ligand counts end the region)."""
    rng = np.random.default_rng(5)
    pos, feat, ptr = concat([cloud(rng, n) for n in (17, 1, 64, 30)])
    ref = R.perceive_batch(pos, feat, ptr, Z, ALLOWED)
    got, t = perceive_gpu(cuda, pos, feat, ptr)
    assert_equal(got, ref, 'guarded scratch')
    for largest in (False, True):
        blocks, st, _ = sdf_gpu(cuda, t, largest=largest)
        want, wst = R.sdf_batch(pos, ptr, ELEMENTS, ref, largest_only=largest)
        assert st == wst and blocks == want


def test_bond_capacity_too_small_for_the_middle_ligand_only(cuda):
    rng = np.random.default_rng(3)
    ligs = [(TEXTBOOK[0][1], TEXTBOOK[0][2]), cloud(rng, 20), (['Cl'], [[0.0, 0.0, 0.0]])]
    pos, feat, ptr = concat(ligs)
    full = R.perceive_batch(pos, feat, ptr, Z, ALLOWED)
    n_mid = int(full['summary'][1][0])
    assert n_mid > 5
    cap = 2 + n_mid - 1
    ref = R.perceive_batch(pos, feat, ptr, Z, ALLOWED, cap_bonds=cap)
    assert ref['status'].tolist() == [0, R.CAPACITY, 0] and ref['bond_ptr'][-1] == cap + 1
    got, t = perceive_gpu(cuda, pos, feat, ptr, cap_bonds=cap)
    assert_equal(got, ref, 'capacity')
    assert got['bond_ptr'][-1] == cap + 1                       # the size needed, beyond the capacity
    blocks, st, _ = sdf_gpu(cuda, t)
    want, wst = R.sdf_batch(pos, ptr, ELEMENTS, ref)
    assert st == wst == [0, R.SDF_NO_MOLECULE, 0] and blocks == want and blocks[1] == ''


def test_bad_coordinates_unknown_elements_and_nan_features(cuda):
    rng = np.random.default_rng(5)
    ligs = [cloud(rng, 12, 1.0) for _ in range(5)]
    ligs[1][1][3, 1] = np.nan
    ligs[2][1][0, 2] = np.inf
    ligs[2][1][7, 0] = -np.inf
    ligs[3][0][4, 6] = np.nan                                   # a NaN is the maximum of its feature row
    ligs[3][0][5, 0] = np.nan
    ligs[3][0][5, 3] = np.nan                                   # the first NaN wins
    pos, feat, ptr = concat(ligs)
    z = list(Z)
    z[1], z[2] = 0, 26                                          # nitrogen's class unknown, oxygen's class an element outside the table
    ref = R.perceive_batch(pos, feat, ptr, z, ALLOWED)
    assert ref['status'].tolist()[1] == R.BAD_ATOM and ref['status'].tolist()[2] == R.BAD_ATOM
    assert ref['elem'][ptr[3] + 4] == 6 and ref['elem'][ptr[3] + 5] == 0
    got, t = perceive_gpu(cuda, pos, feat, ptr, z=z)
    assert_equal(got, ref, 'bad atoms')
    assert got['valence'][ptr[1] + 3] == 0 and got['valence'][ptr[2]] == 0 and got['valence'][ptr[2] + 7] == 0
    unknown = np.isin(got['elem'], [1, 2])
    assert unknown.any() and (got['valence'][unknown] == 0).all()
    # the element decode is kpd_xyz_emit's
    elem, _, _ = hip.xyz_emit(t['pos'].nan_to_num(0.0, 0.0, 0.0), torch.from_numpy(feat).to(cuda), t['ptr'], ELEMENTS)
    assert np.array_equal(elem.cpu().numpy(), got['elem'])
    blocks, st, _ = sdf_gpu(cuda, t)
    want, wst = R.sdf_batch(pos, ptr, ELEMENTS, ref)
    assert st == wst and blocks == want and st[1] == st[2] == R.SDF_NONFINITE and st[0] == 0
    # the Python surface: a ligand without a block raises, or is the empty string on request
    z_all = molecule.build_molecules([torch.from_numpy(p).to(cuda) for _, p in ligs], [torch.from_numpy(f).to(cuda) for f, _ in ligs], ELEMENTS)
    with pytest.raises(hip.KpdError, match='ligand 1'):
        z_all.sdf()
    loose = z_all.sdf(strict=False)
    assert loose[1] == loose[2] == '' and loose[0].endswith('M  END\n$$$$\n') and z_all.status.tolist()[1] & hip.MOL_BAD_ATOM


@pytest.mark.parametrize('ptr', [[0, 5, 100000, 9, 12], [0, -3, 4, 12], [0, 5, 5, 13]])
def test_malformed_segments_are_left_out(cuda, ptr):
    rng = np.random.default_rng(9)
    feat, pos = cloud(rng, 12, 1.0)
    ref = R.perceive_batch(pos, feat, ptr, Z, ALLOWED)
    assert (ref['status'] & R.BAD_SEGMENT).any()
    got, t = perceive_gpu(cuda, pos, feat, ptr)
    assert_equal(got, ref, 'malformed')
    blocks, st, _ = sdf_gpu(cuda, t)
    want, wst = R.sdf_batch(pos, ptr, ELEMENTS, ref)
    assert st == wst and blocks == want


# ---- 4. batch invariance and determinism --------------------------------------------------------------------------------
def local_rows(got, ptr, b):
    a0, a1, p0, p1 = ptr[b], ptr[b + 1], got['bond_ptr'][b], got['bond_ptr'][b + 1]
    return (got['elem'][a0:a1].tolist(), got['valence'][a0:a1].tolist(), got['frag'][a0:a1].tolist(), (got['bonds'][p0:p1] - a0).tolist(),
            got['order'][p0:p1].tolist(), got['summary'][b].tolist(), int(got['status'][b]))


def test_batch_invariance_and_determinism(cuda, parity):
    ligs = parity['ligs'][:40]
    pos, feat, ptr = concat(ligs)
    got, t = perceive_gpu(cuda, pos, feat, ptr)
    again, t2 = perceive_gpu(cuda, pos, feat, ptr)
    for k in ('elem', 'valence', 'frag', 'order', 'bond_ptr', 'summary', 'status'):
        assert np.array_equal(got[k], again[k]), k
    n = got['bond_ptr'][-1]
    assert np.array_equal(got['bonds'][:n], again['bonds'][:n])
    assert sdf_gpu(cuda, t) == sdf_gpu(cuda, t2)
    perm = np.random.default_rng(1).permutation(len(ligs))
    ppos, pfeat, pptr = concat([ligs[k] for k in perm])
    shuffled, _ = perceive_gpu(cuda, ppos, pfeat, pptr)
    for at, b in enumerate(perm):
        assert local_rows(shuffled, pptr, at) == local_rows(got, ptr, b), b
    for b in (0, 7, 39):
        alone, _ = perceive_gpu(cuda, *concat([ligs[b]]))
        assert local_rows(alone, [0, len(ligs[b][1])], 0) == local_rows(got, ptr, b), b


# ---- 5. SDF bytes -----------------------------------------------------------------------------------------------------
def test_sdf_bytes(cuda, parity):
    pos, feat, ptr, ref = parity['pos'], parity['feat'], parity['ptr'], parity['ref']
    got, t = perceive_gpu(cuda, pos, feat, ptr)
    full = None
    for largest in (False, True):
        blocks, st, tp = sdf_gpu(cuda, t, largest=largest)
        want, wst = R.sdf_batch(pos, ptr, ELEMENTS, ref, largest)
        assert st == wst and not any(st)
        assert blocks == want, [b for b in range(len(want)) if blocks[b] != want[b]][:5]
        assert tp == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
        full = full or (blocks, tp)
    assert any(m['summary'][1] > 1 for m in ref['mols'])                        # largest_frag dropped something
    # capacity too small: offsets as in the full run, the ligands that fit are written, the others flagged
    blocks, tp = full
    cut = tp[3] + 10
    some, st, tp2 = sdf_gpu(cuda, t, capacity=cut)
    assert tp2 == tp and some[:3] == blocks[:3]
    assert st[:3] == [0, 0, 0] and all(s == R.SDF_CAPACITY for s in st[3:])
    none, st, tp3 = sdf_gpu(cuda, t, capacity=0)
    assert tp3 == tp and all(s == R.SDF_CAPACITY for s in st)


def test_sdf_coordinate_formatting(cuda):
    # odd / 32: the 4-decimal rounding is a tie in binary (312.5, 937.5, 1562.5, 2187.5 ten-thousandths): half to even
    ties = [0.03125, 0.09375, 0.15625, -0.21875, 5.03125, -1234.46875]
    small = [-0.0, 0.0, -1e-6, 4.9999e-5, 5.0001e-5, 1e-30, -1e-42]
    wide_ok = [99999.99, -9999.999, 12345.678, -0.5]
    ligs = [(['C', 'N', 'O'], np.array(ties, dtype=np.float32).reshape(2, 3).tolist() + [[1.0, 1.0, 1.0]]),
            (['Cl', 'Br'], [small[:3], small[3:6]]), (['S'], [[small[6], wide_ok[0], wide_ok[1]]]), (['P'], [wide_ok[1:]]),
            (['C', 'C'], [[0.0, 0.0, 0.0], [99999.9999, 0.0, 0.0]]),            # fp32: 100000.0, eleven characters
            (['C'], [[0.0, -10000.0, 0.0]]), (['I'], [[3e38, 0.0, 0.0]]), (['B'], [[1.5, 2.5, -3.5]])]
    pos, feat, ptr = concat(ligs)
    assert '%.4f' % float(np.float32(99999.99)) == '99999.9922' and '%.4f' % float(np.float32(99999.9999)) == '100000.0000'
    ref = R.perceive_batch(pos, feat, ptr, Z, ALLOWED)
    got, t = perceive_gpu(cuda, pos, feat, ptr)
    assert_equal(got, ref, 'formatting')
    blocks, st, _ = sdf_gpu(cuda, t)
    want, wst = R.sdf_batch(pos, ptr, ELEMENTS, ref)
    assert st == wst == [0, 0, 0, 0, R.SDF_WIDE, R.SDF_WIDE, R.SDF_WIDE, 0]
    assert blocks == want and blocks[4] == blocks[5] == blocks[6] == ''
    assert '    0.0312    0.0938    0.1562 C  ' in blocks[0] and '   -0.2188    5.0312-1234.4688 N  ' in blocks[0]
    assert '   -0.0000    0.0000   -0.0000 Cl ' in blocks[1] and '    0.0000    0.0001    0.0000 Br ' in blocks[1]
    assert '   -0.000099999.9922-9999.9990 S  ' in blocks[2]


# ---- 6. end to end --------------------------------------------------------------------------------------------------------
def test_sampling_to_molecules_end_to_end(cuda, tmp_path):
    from keypoint_diffusion_amd import synth
    from keypoint_diffusion_amd.ligand_diffuser import KeypointDiffusion
    from . import util
    cut = util.CUTOFFS_ALL_ATOM
    model = KeypointDiffusion(10, 10, None, n_timesteps=6, architecture='egnn', rec_encoder_type='fixed',
                              graph_config=dict(n_keypoints=20, graph_cutoffs=cut), dynamics_config=util.EGNN_C2, precision=1e-5)
    synth.fill_state_dict_(model, 13)
    model = model.eval().to(cuda)
    pocket = synth.synth_complexes([70], [1], 20, cut, seed=9)[0].to(cuda)
    pocket.remove_nodes(pocket.nodes('lig'), ntype='lig')
    pos, feat = model.sample_given_pocket(pocket, torch.tensor([8, 8, 8]))
    pos, feat = [p.to(cuda) for p in pos], [f.to(cuda) for f in feat]
    mols = molecule.build_molecules(pos, feat, ELEMENTS)
    assert len(mols) == 3 and mols.status.tolist() == [0, 0, 0] and mols.lig_ptr.tolist() == [0, 8, 16, 24]
    ref = R.perceive_batch(torch.cat(pos).cpu().numpy(), torch.cat(feat).cpu().numpy(), [0, 8, 16, 24], Z, ALLOWED)
    assert np.array_equal(mols.summary.cpu().numpy(), ref['summary']) and np.array_equal(mols.valence.cpu().numpy(), ref['valence'])
    blocks = mols.sdf()
    assert blocks == utils.sampled_ligands_sdf(pos, feat, ELEMENTS)
    bptr = mols.bond_ptr.tolist()
    for b, block in enumerate(blocks):                           # the block parses back to the tensors
        lines = block.split('\n')
        na, nb = int(lines[3][:3]), int(lines[3][3:6])
        assert na == 8 and nb == bptr[b + 1] - bptr[b] == int(mols.summary[b, 0])
        assert lines[1] == '  kpd_hip           3D' and lines[4 + na + nb:] == ['M  END', '$$$$', '']
        xyz = np.array([[float(lines[4 + a][10 * c:10 * c + 10]) for c in range(3)] for a in range(na)])
        assert np.abs(xyz - pos[b].cpu().numpy()).max() <= 0.5e-4 + 1e-9
        assert [lines[4 + a][31:34].strip() for a in range(na)] == [ELEMENTS[e] for e in mols.elem[8 * b:8 * b + 8].tolist()]
        rows = [[int(l[0:3]), int(l[3:6]), int(l[6:9])] for l in lines[4 + na:4 + na + nb]]
        bonds = (mols.bonds[bptr[b]:bptr[b + 1]] - 8 * b + 1).tolist()
        assert rows == [[i, j, o] for (i, j), o in zip(bonds, mols.order[bptr[b]:bptr[b + 1]].tolist())]
    utils.write_sdf_file(tmp_path / 'out.sdf', pos, feat, ELEMENTS, largest_frag=True)
    assert (tmp_path / 'out.sdf').read_text() == ''.join(mols.sdf(largest_frag=True))
    counts = torch.tensor([50, 12, 20, 2, 1, 3, 3, 1, 1, 1])
    met = mols.metrics(type_counts=counts)
    assert set(met) == {'atom_validity', 'avg_frag_frac', 'connectivity', 'atom_type_kldiv'}
    assert all(0.0 <= met[k] <= 1.0 for k in ('atom_validity', 'avg_frag_frac', 'connectivity')) and np.isfinite(met['atom_type_kldiv'])
    # the non-rdkit half of sample_and_analyze on what `_sample` returns
    samples = model._sample([pocket, pocket], [[8, 8], [8]])
    lig_pos = [p.to(cuda) for s in samples for p in s['positions']]
    lig_feat = [f.to(cuda) for s in samples for f in s['features']]
    assert molecule.analyze_samples(samples, ELEMENTS, type_counts=counts, device=cuda) == \
        molecule.build_molecules(lig_pos, lig_feat, ELEMENTS).metrics(type_counts=counts)
    with pytest.raises(hip.KpdError):
        molecule.analyze_samples(samples, ELEMENTS)              # `_sample` returns host tensors: no computing on the host
