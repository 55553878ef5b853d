"""Keys, fingerprints and Tanimoto diversity on the GPU (kpd_mol_keys, kpd_fp_diversity, Molecules.keys / fingerprints /
set_metrics) against the integer restatement of include/kpd.h (tests/molset_ref.py).  Keys, fingerprints, per-atom invariants,
pair counts and status words are compared by exact equality; div_sum, an fp64 sum whose order differs from the restatement's,
gets the bound of recursive summation, n_pairs * 2^-52 * div_sum (every term is >= 0, so the sum of magnitudes is the sum).
Every raw call runs with canary bytes behind each output buffer."""
import math
import random

import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import hip, molecule
from . import molecule_ref as R
from . import molset_ref as S
from .molecule_cases import ALLOWED, ELEMENTS, TEXTBOOK, TWO_ETHANOLS_CL, Z, one_hot
from .test_molecule_gpu import Guarded, cloud, concat, perceive_gpu, ptr_of

pytestmark = pytest.mark.gpu
CONFIGS = [dict(largest_only=True, with_orders=True, radius=2, nbits=2048), dict(largest_only=False, with_orders=False, radius=4, nbits=4096),
           dict(largest_only=True, with_orders=False, radius=0, nbits=64)]


# ---- bond graphs written down directly, in the layout kpd_mol_perceive leaves them in ------------------------------------
def graph(elem, bonds, order=None):
    return dict(elem=list(elem), bonds=[tuple(sorted(b)) for b in bonds], order=list(order) if order is not None else [1] * len(bonds))


def chain(n, rng):
    return graph([rng.choice([0, 0, 1, 2]) for _ in range(n)], [(a, a + 1) for a in range(n - 1)], [rng.choice([1, 1, 2]) for _ in range(n - 1)])


def branched(n, rng, max_deg=4, closures=0):
    """A random tree of n atoms with degree <= max_deg, plus some ring closures."""
    deg, bonds = [0] * n, set()
    for a in range(1, n):
        b = rng.choice([c for c in range(max(0, a - 12), a) if deg[c] < max_deg] or [c for c in range(a) if deg[c] < max_deg])
        bonds.add((b, a))
        deg[a] += 1
        deg[b] += 1
    for _ in range(closures if n > 2 else 0):
        i, j = sorted(rng.sample(range(n), 2))
        if (i, j) not in bonds and deg[i] < max_deg and deg[j] < max_deg:
            bonds.add((i, j))
            deg[i] += 1
            deg[j] += 1
    bonds = sorted(bonds)
    return graph([rng.choice([0, 0, 0, 1, 2, 3]) for _ in range(n)], bonds, [rng.choice([1, 1, 1, 2, 3]) for _ in bonds])


def union(*gs):
    """Several graphs as the fragments of one ligand."""
    elem, bonds, order, at = [], [], [], 0
    for g in gs:
        elem += g['elem']
        bonds += [(i + at, j + at) for i, j in g['bonds']]
        order += g['order']
        at += len(g['elem'])
    return graph(elem, bonds, order)


def renumbered(g, rng):
    n = len(g['elem'])
    p = list(range(n))
    rng.shuffle(p)
    elem = [0] * n
    for a in range(n):
        elem[p[a]] = g['elem'][a]
    rows = sorted((tuple(sorted((p[i], p[j]))), o) for (i, j), o in zip(g['bonds'], g['order']))
    return graph(elem, [r[0] for r in rows], [r[1] for r in rows])


def fragments(n, bonds):
    """frag of kpd_mol_perceive: the rank of every atom's component in order of first atom."""
    root = list(range(n))

    def find(a):
        while root[a] != a:
            root[a] = root[root[a]]
            a = root[a]
        return a
    for i, j in bonds:
        ri, rj = find(i), find(j)
        root[max(ri, rj)] = min(ri, rj)
    ranks = {}
    return [ranks.setdefault(find(a), len(ranks)) for a in range(n)]


def batch_of(specs):
    """specs: graph(...) dicts, 'empty', or ('left out', n).  Returns the arrays kpd_mol_perceive would have written and the
    structure molset_ref.keys_batch reads (that of molecule_ref.perceive_batch)."""
    ptr, elem, frag, bonds, order, bond_ptr, status, mols = [0], [], [], [], [], [0], [], []
    for s in specs:
        a0 = ptr[-1]
        if s == 'empty' or isinstance(s, tuple):
            n = 0 if s == 'empty' else s[1]
            elem += [-1] * n
            frag += [-1] * n
            status.append(hip.MOL_EMPTY if s == 'empty' else hip.MOL_BAD_SEGMENT)
            mols.append(None)
        else:
            n = len(s['elem'])
            rows = sorted(zip(s['bonds'], s['order']))
            f = fragments(n, s['bonds'])
            elem += s['elem']
            frag += f
            bonds += [(i + a0, j + a0) for (i, j), _ in rows]
            order += [o for _, o in rows]
            status.append(0)
            mols.append(dict(elem=np.array(s['elem']), frag=np.array(f), bonds=np.array([r[0] for r in rows]).reshape(-1, 2), order=np.array([r[1] for r in rows])))
        ptr.append(a0 + n)
        bond_ptr.append(len(order))
    arrays = dict(ptr=ptr, elem=elem, frag=frag, bonds=np.array(bonds, dtype=np.int64).reshape(-1, 2), order=order, bond_ptr=bond_ptr, status=status)
    return arrays, dict(elem=np.array(elem), status=np.array(status), mols=mols)


def to_device(arrays, dev):
    t = {k: torch.tensor(np.asarray(v), dtype=torch.int32, device=dev).contiguous() for k, v in arrays.items()}
    t['cap'] = t['order'].numel()
    return t


def keys_gpu(dev, t, z=Z, largest_only=True, with_orders=True, radius=2, nbits=2048, want_inv=True):
    """kpd_mol_keys through the C ABI on device tensors in kpd_mol_perceive's layout.  Returns numpy outputs (int64)."""
    N, B, W = t['elem'].numel(), t['ptr'].numel() - 1, nbits // 32
    g = Guarded(dev)
    key, fp, inv, status = g.new(B, torch.int64), g.new(B * W), g.new(N, torch.int64), g.new(B)
    zt = torch.tensor(z, dtype=torch.int32, device=dev)
    hip.check(hip.lib().kpd_mol_keys(t['ptr'].data_ptr(), N, B, t['elem'].data_ptr(), len(z), zt.data_ptr(), t['frag'].data_ptr(),
                                     t['bonds'].data_ptr(), t['order'].data_ptr(), t['bond_ptr'].data_ptr(), t['cap'], t['status'].data_ptr(),
                                     int(largest_only), int(with_orders), radius, nbits, key.data_ptr(), fp.data_ptr(),
                                     inv.data_ptr() if want_inv else None, status.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    g.check()
    if not want_inv:
        assert bool((inv.view(torch.uint8) == 0x5A).all())
    return dict(key=key[:B].cpu().numpy(), fp=fp[:B * W].cpu().numpy().view(np.uint32).astype(np.int64).reshape(B, W),
                atom_inv=inv[:N].cpu().numpy(), status=status[:B].cpu().numpy().astype(np.int64))


def assert_keys(got, want, what=''):
    for k in ('status', 'key', 'atom_inv', 'fp'):
        assert np.array_equal(got[k], want[k]), (what, k, np.nonzero(np.asarray(got[k] != want[k]).reshape(len(want[k]), -1).any(axis=1))[0][:8])


def div_gpu(dev, fp, use, group_ptr):
    """kpd_fp_diversity through the C ABI.  fp: [B, W] values of uint32 words.  Returns (div_sum, n_pairs, status) as numpy."""
    fp = np.asarray(fp, dtype=np.int64)
    B, W = fp.shape
    G = len(group_ptr) - 1
    fp_d = torch.from_numpy(fp.astype(np.uint32).view(np.int32).copy()).to(dev)
    use_d = torch.tensor(np.asarray(use, dtype=np.uint8), device=dev)
    gp = torch.tensor(np.asarray(group_ptr), dtype=torch.int32, device=dev)
    g = Guarded(dev)
    div, n_pairs, status = g.new(G, torch.float64), g.new(G, torch.int64), g.new(G)
    hip.check(hip.lib().kpd_fp_diversity(fp_d.data_ptr(), use_d.data_ptr(), B, W, gp.data_ptr(), G, div.data_ptr(), n_pairs.data_ptr(),
                                         status.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    g.check()
    return div[:G].cpu().numpy(), n_pairs[:G].cpu().numpy(), status[:G].cpu().numpy().astype(np.int64)


def assert_diversity(got, want, what=''):
    (d, n, st), (wd, wn, wst) = got, want
    assert np.array_equal(st, wst) and np.array_equal(n, wn), (what, st, n)
    for g in range(len(wd)):
        print(what, 'group', g, 'pairs', int(wn[g]), 'div_sum', d[g], 'restatement', wd[g], 'bound', wn[g] * 2.0 ** -52 * wd[g])
        assert abs(d[g] - wd[g]) <= wn[g] * 2.0 ** -52 * wd[g], (what, g)


# ---- 1. keys and fingerprints ------------------------------------------------------------------------------------------------
def test_ligand_sizes_around_the_lane_passes(cuda):
    rng = random.Random(3)
    specs = [chain(n, rng) for n in (1, 2, 63, 64, 65, 256)] + [branched(256, rng, closures=20)]
    arrays, ref = batch_of(specs)
    t = to_device(arrays, cuda)
    for cfg in CONFIGS[:2]:
        want = S.keys_batch(ref, arrays['ptr'], Z, **cfg)
        assert not want['status'].any() and len(set(want['key'].tolist())) == len(specs)
        assert_keys(keys_gpu(cuda, t, **cfg), want, cfg)
    one = keys_gpu(cuda, to_device(batch_of(specs[5:6])[0], cuda), **CONFIGS[0])           # B = 1: the 256-atom chain alone
    assert one['key'][0] == S.keys_batch(ref, arrays['ptr'], Z, **CONFIGS[0])['key'][5]


@pytest.fixture(scope='module')
def seventy():
    """70 ligands: random graphs up to degree 6, ligands of several fragments (one with a tie for the largest), renumbered
    copies, an empty ligand and one that was left out in the middle."""
    rng = random.Random(11)
    specs = [branched(rng.randint(1, 40), rng, max_deg=rng.choice([3, 4, 6]), closures=rng.randint(0, 4)) for _ in range(56)]
    specs[7] = graph([3] + [5] * 6, [(0, k) for k in range(1, 7)])                         # six neighbours: SF6
    specs[20] = 'empty'
    specs[33] = ('left out', 300)
    tie = union(specs[1], branched(5, rng), renumbered(specs[1], rng))                      # two largest fragments of one size
    specs += [union(specs[2], specs[3]), union(branched(3, rng), specs[4], branched(2, rng)), tie, union(chain(4, rng), chain(4, rng))]
    copies = [(b, len(specs) + k) for k, b in enumerate((0, 5, 7, 12, 30, 41, 50, 55, 56, 58))]
    specs += [renumbered(specs[b], rng) for b, _ in copies]
    assert len(specs) == 70
    arrays, ref = batch_of(specs)
    return dict(specs=specs, arrays=arrays, ref=ref, copies=copies, want=[S.keys_batch(ref, arrays['ptr'], Z, **cfg) for cfg in CONFIGS])


def test_seventy_ligands_match_under_every_setting(cuda, seventy):
    t = to_device(seventy['arrays'], cuda)
    for cfg, want in zip(CONFIGS, seventy['want']):
        assert want['status'].tolist() == [1 if b in (20, 33) else 0 for b in range(70)]
        got = keys_gpu(cuda, t, **cfg)
        assert_keys(got, want, cfg)
        assert got['key'][20] == got['key'][33] == 0 and not got['fp'][[20, 33]].any()
        for b, c in seventy['copies']:                                                      # renumbered copies inside one batch
            assert got['key'][b] == got['key'][c] and np.array_equal(got['fp'][b], got['fp'][c]), (cfg, b)
    full, largest = seventy['want'][1], seventy['want'][0]
    assert largest['key'][58] == largest['key'][1] and full['key'][58] != full['key'][1]    # the tie: the fragment of the lowest rank
    assert (largest['atom_inv'][seventy['arrays']['ptr'][58] + len(seventy['specs'][1]['elem']):seventy['arrays']['ptr'][59]] == 0).all()
    assert len(set(largest['key'].tolist())) >= 40
    no_inv = keys_gpu(cuda, t, want_inv=False, **CONFIGS[0])                                # atom_inv may be NULL
    assert np.array_equal(no_inv['key'], largest['key'])


def test_every_ligand_alone_gives_the_bits_it_gives_in_the_batch(cuda, seventy):
    ptr, want = seventy['arrays']['ptr'], seventy['want'][0]
    got = keys_gpu(cuda, to_device(seventy['arrays'], cuda), **CONFIGS[0])
    again = keys_gpu(cuda, to_device(seventy['arrays'], cuda), **CONFIGS[0])
    for k in got:
        assert np.array_equal(got[k], again[k]), k
    for b, spec in enumerate(seventy['specs']):
        alone = keys_gpu(cuda, to_device(batch_of([spec])[0], cuda), **CONFIGS[0])
        assert alone['key'][0] == got['key'][b] and alone['status'][0] == got['status'][b], b
        assert np.array_equal(alone['fp'][0], got['fp'][b]) and np.array_equal(alone['atom_inv'], got['atom_inv'][ptr[b]:ptr[b + 1]]), b


def test_inputs_that_perception_cannot_have_written_give_no_molecule(cuda):
    rng = random.Random(2)
    good = branched(9, rng)
    specs = [good, graph([0] * 8, [(0, k) for k in range(1, 8)]), good, graph([0, 0, 0], [(0, 1), (1, 2)]), good, graph([0, 0], [(0, 1)], [4])]
    arrays, ref = batch_of(specs)
    arrays['bonds'][arrays['bond_ptr'][3]] = [arrays['ptr'][3], arrays['ptr'][2]]           # a bond that leaves its ligand
    arrays['elem'][arrays['ptr'][4] + 1] = len(Z)                                           # an element class out of range
    got = keys_gpu(cuda, to_device(arrays, cuda), **CONFIGS[0])
    want = S.keys_batch(ref, arrays['ptr'], Z, **CONFIGS[0])
    assert got['status'].tolist() == [0, 1, 0, 1, 1, 1]
    for b in (0, 2):
        assert got['key'][b] == want['key'][b] and np.array_equal(got['fp'][b], want['fp'][b])
    assert not got['key'][[1, 3, 4, 5]].any() and not got['fp'][[1, 3, 4, 5]].any()
    assert not got['atom_inv'][arrays['ptr'][3]:arrays['ptr'][4]].any()


def test_perceived_ligands_textbook_and_left_out(cuda):
    rng = np.random.default_rng(21)
    ligs = [(sym, p) for _, sym, p, _ in TEXTBOOK] + [(TWO_ETHANOLS_CL[0], TWO_ETHANOLS_CL[1])]
    ligs += [cloud(rng, n, 1.3) for n in (30, 0, 257, 45)]
    pos, feat, ptr = concat(ligs)
    ref = R.perceive_batch(pos, feat, ptr, Z, ALLOWED)
    _, t = perceive_gpu(cuda, pos, feat, ptr)
    names = [c[0] for c in TEXTBOOK]
    nb = len(TEXTBOOK)
    assert max(m['summary'][1] for m in ref['mols'][nb + 1:] if m is not None) > 1           # a cloud with several fragments
    for cfg in CONFIGS:
        want = S.keys_batch(ref, ptr, Z, **cfg)
        assert want['status'].tolist() == [0] * (nb + 2) + [1, 1, 0]
        got = keys_gpu(cuda, t, **cfg)
        assert_keys(got, want, cfg)
        k = dict(zip(names, got['key'][:nb].tolist()))
        assert k['CO2'] == k['short CO2'] and k['five neighbours, centre first'] == k['five neighbours, centre last']
        assert (k['propene'] == k['propyne']) == (not cfg['with_orders']) and k['ethanol'] != k['acetamide']
        assert (got['key'][nb] == k['ethanol']) == cfg['largest_only']                      # two ethanols and a chloride
        # CO2 twice and the two stars; without orders propene, propyne and the bent C3 of '0.3 A apart' are one graph as well
        assert len(set(k.values())) == (nb - 2 if cfg['with_orders'] else nb - 4)


@pytest.mark.parametrize('ptr', [[0, 5, 100000, 9, 12], [0, -3, 4, 12]])
def test_malformed_segments_give_no_molecule(cuda, ptr):
    feat, pos = cloud(np.random.default_rng(9), 12, 1.0)
    ref = R.perceive_batch(pos, feat, ptr, Z, ALLOWED)
    _, t = perceive_gpu(cuda, pos, feat, ptr)
    want = S.keys_batch(ref, ptr, Z, **CONFIGS[0])
    assert want['status'].any() and not want['status'].all()
    assert_keys(keys_gpu(cuda, t, **CONFIGS[0]), want, 'malformed')


# ---- 2. diversity ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def prints():
    """Fingerprint rows of 64 words with a few dozen bits each, drawn from a small pool so that rows overlap; rows 4 and 5
    are all zero.  Groups of 0, 1, 2, 3 and 300 members, an empty group between full ones."""
    rng = np.random.default_rng(4)
    B, W = 330, 64
    fp = np.zeros((B, W), dtype=np.int64)
    for b in range(B):
        for bit in rng.choice(400, size=int(rng.integers(10, 60)), replace=False):
            fp[b, bit >> 5] |= 1 << (int(bit) & 31)
    fp[:, 63] |= (rng.random(B) < 0.5).astype(np.int64) << 31                              # the top bit of a word
    fp[4] = fp[5] = 0
    fp[2] |= fp[1]                                                                          # the two-member group overlaps for certain
    group_ptr = [0, 0, 1, 3, 3, 6, 306, 330]                                                # 0, 1, 2 (rows 1-2), 0, 3 (rows 3-5), 300, 24
    use = np.ones(B, dtype=np.uint8)
    return dict(fp=fp, group_ptr=group_ptr, use=use, want=S.diversity(fp, use, group_ptr))


def test_diversity_group_sizes(cuda, prints):
    fp, gp, use, want = prints['fp'], prints['group_ptr'], prints['use'], prints['want']
    assert want[1].tolist() == [0, 0, 1, 0, 3, 44850, 276] and want[0][5] > 30000
    got = div_gpu(cuda, fp, use, gp)
    assert_diversity(got, want, 'batch')
    assert got[0][0] == got[0][1] == got[0][3] == 0.0
    again = div_gpu(cuda, fp, use, gp)
    assert np.array_equal(got[0], again[0])
    for g in range(len(gp) - 1):                                                            # a group alone: the same bits
        alone = div_gpu(cuda, fp, use, gp[g:g + 2])
        assert alone[0][0] == got[0][g] and alone[1][0] == got[1][g] and alone[2][0] == 0, g
    # the three-member group pair by pair (rows 3, 4, 5; 4 and 5 are all zero: T = 1 when the union is empty)
    for i, j in ((3, 4), (3, 5), (4, 5)):
        mask = np.zeros_like(use)
        mask[[i, j]] = 1
        d, n, _ = div_gpu(cuda, fp, mask, gp)
        assert n[4] == 1 and d[4] == S.tanimoto_distance(fp[i], fp[j]) == (0.0 if i == 4 else 1.0), (i, j)
    d, n, _ = div_gpu(cuda, fp, use, [1, 3])
    assert d[0] == S.tanimoto_distance(fp[1], fp[2]) and 0.0 < d[0] < 1.0


def test_diversity_use_masks_and_malformed_segments(cuda, prints):
    fp, gp = prints['fp'], prints['group_ptr']
    rng = np.random.default_rng(8)
    use = (rng.random(len(fp)) < 0.6).astype(np.uint8)
    use[6:306:7] = 0
    use[1:3] = 0                                                                            # empties the two-member group
    use[306:] = 0
    use[310] = 1                                                                            # leaves one of 24
    want = S.diversity(fp, use, gp)
    assert want[1][2] == 0 and want[1][6] == 0 and 5000 < want[1][5] < 44850
    assert_diversity(div_gpu(cuda, fp, use, gp), want, 'masked')
    bad = [0, 3, 2, 400, 330, -1, 5]
    want = S.diversity(fp, prints['use'], bad)
    assert want[2].tolist() == [0, 1, 1, 1, 1, 1] and want[1].tolist() == [3, 0, 0, 0, 0, 0]
    got = div_gpu(cuda, fp, prints['use'], bad)
    assert_diversity(got, want, 'malformed')
    assert not got[0][1:].any()


@pytest.mark.parametrize('W', [2, 3, 128])
def test_diversity_row_widths(cuda, W):
    rng = np.random.default_rng(W)
    fp = rng.integers(0, 2 ** 32, size=(40, W), dtype=np.int64) & rng.integers(0, 2 ** 32, size=(40, W), dtype=np.int64)
    use = np.ones(40, dtype=np.uint8)
    assert_diversity(div_gpu(cuda, fp, use, [0, 17, 40]), S.diversity(fp, use, [0, 17, 40]), f'W = {W}')


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------
def test_set_metrics_by_hand(cuda):
    by_name = {c[0]: c for c in TEXTBOOK}
    eth, acn, prp = (by_name[k] for k in ('ethanol', 'acetonitrile', 'propene'))
    # ethanol again: atoms in the order O C C, turned a quarter about z and moved
    turned = np.stack([-eth[2][::-1, 1], eth[2][::-1, 0], eth[2][::-1, 2]], axis=1) + np.float32([3.0, -2.0, 5.0])
    ligs = [(eth[1], eth[2]), (eth[1][::-1], turned), (acn[1], acn[2]), (TWO_ETHANOLS_CL[0], TWO_ETHANOLS_CL[1]), (prp[1], prp[2])]
    dev_of = lambda ls: ([torch.from_numpy(np.asarray(p, dtype=np.float32)).to(cuda) for _, p in ls], [torch.from_numpy(one_hot(s)).to(cuda) for s, _ in ls])
    lig_pos, lig_feat = dev_of(ligs)
    train = molecule.training_keys(*dev_of([(prp[1], prp[2]), (eth[1], eth[2]), (eth[1][::-1], turned)]), ELEMENTS)
    assert train.dtype == torch.int64 and train.is_cuda and train.numel() == 2 and bool(train[0] < train[1])
    mols = molecule.build_molecules(lig_pos, lig_feat, ELEMENTS)
    keys = mols.keys()
    assert keys.dtype == torch.int64 and keys.shape == (5,)
    k = keys.tolist()
    assert k[0] == k[1] == k[3] and len({k[0], k[2], k[4]}) == 3                            # the largest fragment of ligand 3 is an ethanol
    assert len(set(mols.keys(largest_frag=False).tolist())) == 4
    # the restatement on the graphs written out by hand: C-C-O with two single bonds, C-C#N
    e = S.graph_key([6, 6, 8], [(0, 1), (1, 2)], [1, 1])
    a = S.graph_key([6, 6, 7], [(0, 1), (1, 2)], [1, 3])
    assert k[0] == S.signed(e['key']) and k[2] == S.signed(a['key'])
    fps = mols.fingerprints()
    assert fps.dtype == torch.int32 and fps.shape == (5, 64)
    assert (fps[0].cpu().numpy().view(np.uint32).tolist(), fps[2].cpu().numpy().view(np.uint32).tolist()) == (e['fp'], a['fp'])
    assert mols.fingerprints(radius=0, nbits=64).shape == (5, 2)
    # pocket 0 = ligands 0-3, pocket 1 = ligand 4.  Connected (largest fragment >= half the atoms): 0, 1, 2, 4; ligand 3 is 3 / 7.
    # Distinct keys among them: ethanol, acetonitrile, propene; the training set knows ethanol and propene.
    t = S.tanimoto_distance(e['fp'], a['fp'])
    assert 0.0 < t < 1.0
    m = mols.set_metrics(group_ptr=[0, 4, 5], train_keys=train)
    assert set(m) == {'uniqueness', 'novelty', 'diversity', 'diversity_std', 'diversity_per_group'}
    assert m['uniqueness'] == 3 / 4 and m['novelty'] == 1 / 3
    # diversity over the ligands that have a molecule, 3 of the 4 fingerprints of pocket 0 are ethanol's: 3 pairs at t, 3 at 0
    per_group = m['diversity_per_group'].tolist()
    assert abs(per_group[0] - 3 * t / 6) <= 6 * 2.0 ** -52 * (3 * t / 6) and per_group[1] == 0.0
    # mean and standard deviation: a dozen fp64 roundings of 2^-53 each on top of the sum's, far inside 1e-14
    assert m['diversity'] == pytest.approx(t / 4, rel=1e-14) and m['diversity_std'] == pytest.approx(float(np.std([t / 2, 0.0])), rel=1e-14)
    assert set(mols.set_metrics()) == {'uniqueness'} and mols.set_metrics(train_keys=train[:0])['novelty'] == 1.0
    assert mols.set_metrics(connectivity_thresh=3 / 7)['uniqueness'] == 3 / 5
    # analyze_samples: the groups are the pockets of `samples`
    cpu = lambda ts: [x.cpu() for x in ts]
    samples = [dict(positions=cpu(lig_pos[:4]), features=cpu(lig_feat[:4])), dict(positions=cpu(lig_pos[4:]), features=cpu(lig_feat[4:]))]
    both = molecule.analyze_samples(samples, ELEMENTS, device=cuda, train_keys=train, set_metrics=True)
    assert both.pop('diversity_per_group').tolist() == per_group
    assert both == {**mols.metrics(), **{k_: v for k_, v in m.items() if k_ != 'diversity_per_group'}}
    plain = molecule.analyze_samples(samples, ELEMENTS, device=cuda)
    assert plain == mols.metrics() and set(plain) == {'atom_validity', 'avg_frag_frac', 'connectivity'}
