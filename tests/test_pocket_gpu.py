"""Pocket extraction on the GPU (kpd_pocket_select, kpd_interface_points, keypoint_diffusion_amd.pocket) against the
reference's own outputs (tests/golden/pocket_XX.npz), bitwise; batch invariance; the residue-wise form against the
float64 restatement of test_pocket_config.py; the edges that must not fault; and raw arrays -> pockets -> dataset ->
sampling / a training step end to end."""
import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import hip
from keypoint_diffusion_amd import pocket as P

from . import util
from .test_pocket_config import load_cases, restate_points, restate_select
from .util import GUARD, guarded, intact

pytestmark = pytest.mark.gpu
EMPTY, CAPACITY, BAD_RES, BAD_SEGMENT = 1, 2, 4, 8


@pytest.fixture(scope='module')
def cases(cuda):
    cs = load_cases()
    for c in cs:
        for k in ('rec_pos', 'rec_res', 'lig_pos', 'other', 'rec_feat'):
            c[k + '_d'] = c[k].to(cuda)
    return cs


def ptr32(counts, dev):
    return torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32, device=dev)


def batch_of(cs, dev):
    cat = lambda k: torch.cat([c[k] for c in cs]).to(dev)
    return dict(pos=cat('rec_pos'), res=cat('rec_res'), other=cat('other'), feat=cat('rec_feat'), lig=cat('lig_pos'),
                rc=[c['rec_pos'].shape[0] for c in cs], lc=[c['lig_pos'].shape[0] for c in cs])


def run_batch(cs, dev, pad, cut, thr, excl, candidates):
    """hip-level batch run of complexes that share one parameter set; per-complex results on the host."""
    b = batch_of(cs, dev)
    rp, lp = ptr32(b['rc'], dev), ptr32(b['lc'], dev)
    keep = ~b['other']
    sel = hip.pocket_select(b['pos'], rp, b['res'], keep, keep, b['lig'], lp, max(b['rc']), pad, cut)
    cand = (sel['in_box'] & keep) if candidates == 'box' else sel['pocket_mask']
    ip = hip.interface_points(b['pos'], rp, cand, b['lig'], lp, thr, excl)
    out, off = [], 0
    for i in range(len(cs)):
        p0, p1, q0, q1 = sel['pocket_ptr'][i], sel['pocket_ptr'][i + 1], ip['ip_ptr'][i], ip['ip_ptr'][i + 1]
        out.append(dict(rows=(sel['rows'][p0:p1].long() - off).cpu(), pocket_res=sel['pocket_res'][p0:p1].long().cpu(),
                        mask=sel['pocket_mask'][off:off + b['rc'][i]].cpu(), in_box=sel['in_box'][off:off + b['rc'][i]].cpu(),
                        points=ip['points'][q0:q1].cpu(), n_cand=ip['n_cand'][i], status=(sel['status'][i], ip['status'][i])))
        off += b['rc'][i]
    return out


def check_against_reference(c, r, which):
    keep = ~c['other']
    assert r['status'] == (0, 0)
    assert torch.equal(r['mask'][keep], c['byres_mask'])
    assert torch.equal(r['rows'], torch.nonzero(keep)[:, 0][c['byres_mask']])
    assert torch.equal(c['rec_pos'][r['rows']], c['pocket_pos']) and torch.equal(c['rec_feat'][r['rows']], c['pocket_feat'])
    assert torch.equal(r['points'], c[which]), (r['points'].shape, c[which].shape)


# ---- 1. the reference's outputs, singly and batched ---------------------------------------------------------------
def test_single_complexes_match_the_reference_bitwise(cases):
    for c in cases:
        pad, cut, thr, excl = c['params']
        pos, feat, mask, ips = P.get_pocket_atoms(c['rec_pos_d'], c['rec_feat_d'], c['other_d'], c['rec_res_d'], c['lig_pos_d'], pad, cut, thr, excl)
        assert torch.equal(pos.cpu(), c['pocket_pos']) and torch.equal(feat.cpu(), c['pocket_feat'])
        assert torch.equal(mask.cpu(), c['byres_mask'])
        assert torch.equal(ips.cpu(), c['ip_box'])                                   # box candidate set
        ips2 = P.get_interface_points(c['lig_pos_d'], pos, dist_mat=None, distance_threshold=thr, exclusion_threshold=excl)
        assert torch.equal(ips2.cpu(), c['ip_pocket'])                               # pocket candidate set


def same_params(cases):
    groups = {}
    for c in cases:
        groups.setdefault(c['params'], []).append(c)
    return groups


def test_batches_match_the_reference_bitwise(cases, cuda):
    n = 0
    for params, cs in same_params(cases).items():
        for which, cand in (('ip_box', 'box'), ('ip_pocket', 'pocket')):
            for c, r in zip(cs, run_batch(cs, cuda, *params, cand)):
                check_against_reference(c, r, which)
                n += 1
    assert n == 2 * len(cases)
    # The entry points take one parameter set per batch, so the fixtures come in two groups of four that each ran as one batch
    # above.  All eight in ONE batch under the first group's parameters: that group must still equal the reference, the other
    # group the float64 restatement (same arithmetic as the kernels up to the last bit of an fp64 sum, i.e. ~1e-15 A).
    params = cases[0]['params']
    res = run_batch(cases, cuda, *params, 'box')
    for c, r in zip(cases, res):
        keep = ~c['other']
        in_box, mask, rows, pres, _ = restate_select(c['rec_pos'], c['rec_res'], keep, keep, c['lig_pos'], params[0], params[1])
        pts, nc = restate_points(c['lig_pos'], c['rec_pos'][in_box & keep], params[2], params[3])
        assert torch.equal(r['in_box'], in_box) and torch.equal(r['mask'], mask) and torch.equal(r['rows'], rows)
        assert torch.equal(r['pocket_res'], pres) and r['n_cand'] == nc and torch.equal(r['points'], pts)
        if c['params'] == params:
            check_against_reference(c, r, 'ip_box')


# ---- 2. batch composition and repeatability ----------------------------------------------------------------------
def test_permuted_batch_and_second_run_are_bitwise_equal(cases, cuda):
    params = cases[0]['params']
    a = run_batch(cases, cuda, *params, 'box')
    again = run_batch(cases, cuda, *params, 'box')
    perm = [5, 2, 7, 0, 3, 6, 1, 4][:len(cases)]
    b = run_batch([cases[i] for i in perm], cuda, *params, 'box')
    for i, j in enumerate(perm):
        for k in ('rows', 'pocket_res', 'mask', 'in_box', 'points'):
            assert torch.equal(a[j][k], b[i][k]), (j, k)
            assert torch.equal(a[j][k], again[j][k]), (j, k)
        assert a[j]['n_cand'] == b[i]['n_cand'] and a[j]['status'] == b[i]['status']


# ---- 3. residue-wise form -----------------------------------------------------------------------------------------
def test_residue_form(cases, cuda):
    for c in cases[:4]:
        pad, cut, thr, excl = c['params']
        n = c['rec_pos'].shape[0]
        hydrogen = c['rec_el'] == c['n_el'] - 1                                      # 'H' is the last listed element of the fixtures
        probe = torch.ones(n, dtype=torch.bool)                                      # every atom of the residue, hydrogens included
        emit = ~hydrogen & ~c['other']                                               # heavy atoms of supported elements
        rows, pres, pts = P.select_pocket_residues(c['rec_pos_d'], c['rec_res_d'], c['lig_pos_d'], cut, probe.to(cuda), emit.to(cuda),
                                                   interface_distance_threshold=thr, interface_exclusion_threshold=excl)
        _, mask, rrows, rres, _ = restate_select(c['rec_pos'], c['rec_res'], probe, emit, c['lig_pos'], None, cut)
        rpts, _ = restate_points(c['lig_pos'], c['rec_pos'][mask], thr, excl)
        assert torch.equal(rows.cpu(), rrows) and torch.equal(pres.cpu(), rres) and torch.equal(pts.cpu(), rpts)
        # with box_padding >= pocket_cutoff and probe == emit the box form (pinned to the reference above) selects the same atoms
        keep = (~c['other']).to(cuda)
        rp, lp = ptr32([n], cuda), ptr32([c['lig_pos'].shape[0]], cuda)
        nobox = hip.pocket_select(c['rec_pos_d'], rp, c['rec_res_d'], keep, keep, c['lig_pos_d'], lp, n, None, cut)
        box = hip.pocket_select(c['rec_pos_d'], rp, c['rec_res_d'], keep, keep, c['lig_pos_d'], lp, n, cut, cut)
        assert torch.equal(nobox['rows'], box['rows']) and torch.equal(nobox['pocket_res'], box['pocket_res'])
        assert nobox['rows'].numel() > 0 and bool(nobox['in_box'].all()) and not bool(box['in_box'].all())
        if pad >= cut:
            assert torch.equal(nobox['rows'].long().cpu(), torch.nonzero(~c['other'])[:, 0][c['byres_mask']])
        # ca_only: one atom per selected residue (here: the first atom of every residue stands for its C-alpha), no interface points
        first = torch.ones(n, dtype=torch.bool)
        first[1:] = c['rec_res'][1:] != c['rec_res'][:-1]
        rows_ca, pres_ca, pts_ca = P.select_pocket_residues(c['rec_pos_d'], c['rec_res_d'], c['lig_pos_d'], cut, probe.to(cuda), ca_only=True,
                                                            ca_mask=first.to(cuda))
        n_sel = int(torch.unique(c['rec_res'][restate_select(c['rec_pos'], c['rec_res'], probe, probe, c['lig_pos'], None, cut)[2]]).numel())
        assert rows_ca.numel() == n_sel and pres_ca.cpu().tolist() == list(range(n_sel)) and tuple(pts_ca.shape) == (0, 3)


# ---- 4. edges -------------------------------------------------------------------------------------------------
def small_complex(n_rec, n_lig, seed, spread=6.0):
    g = torch.Generator().manual_seed(seed)
    pos = torch.randn(n_rec, 3, generator=g) * spread + 25.0
    lig = torch.randn(n_lig, 3, generator=g) * 2.0 + 25.0
    res = (torch.arange(n_rec) // 7).to(torch.int32)
    return pos, res, lig


def run_one(pos, res, lig, dev, probe=None, emit=None, pad=6.0, cut=4.0, thr=5.0, excl=2.0):
    n = pos.shape[0]
    ones = torch.ones(n, dtype=torch.bool)
    probe, emit = ones if probe is None else probe, ones if emit is None else emit
    rp, lp = ptr32([n], dev), ptr32([lig.shape[0]], dev)
    sel = hip.pocket_select(pos.to(dev), rp, res.to(dev), probe.to(dev), emit.to(dev), lig.to(dev), lp, n, pad, cut)
    ip = P._points(pos.to(dev), rp, sel['pocket_mask'], lig.to(dev), lp, thr, excl)      # grows the candidate capacity when needed
    in_box, mask, rows, pres, bad = restate_select(pos, res, probe, emit, lig, pad, cut)
    pts, nc = restate_points(lig, pos[mask], thr, excl)
    assert torch.equal(sel['in_box'].cpu(), in_box) and torch.equal(sel['pocket_mask'].cpu(), mask)
    assert torch.equal(sel['rows'].long().cpu(), rows) and torch.equal(sel['pocket_res'].long().cpu(), pres)
    assert bool(sel['status'][0] & BAD_RES) == bad and bool(sel['status'][0] & EMPTY) == (rows.numel() == 0)
    assert ip['n_cand'][0] == nc and torch.equal(ip['points'].cpu(), pts) and bool(ip['status'][0] & EMPTY) == (nc == 0)
    return sel, ip


def test_far_ligand_is_skipped_and_neighbours_are_unaffected(cases, cuda):
    a, b = cases[0], cases[4]
    assert a['params'] == b['params']
    pad, cut, thr, excl = a['params']
    far = dict(a, lig_pos=a['lig_pos'] + 1000.0)
    res = run_batch([a, far, b], cuda, pad, cut, thr, excl, 'box')
    check_against_reference(a, res[0], 'ip_box')
    check_against_reference(b, res[2], 'ip_box')
    assert res[1]['status'] == (EMPTY, EMPTY) and res[1]['rows'].numel() == 0 and res[1]['points'].numel() == 0
    bt = batch_of([a, far, b], cuda)
    lig_feat = torch.zeros(bt['lig'].shape[0], 4, dtype=torch.bool, device=cuda)
    seg = lambda c: [0] + list(np.cumsum(c))
    data, skipped = P.extract_pockets(bt['pos'], bt['feat'], bt['res'], seg(bt['rc']), bt['lig'], lig_feat, seg(bt['lc']), pad, cut, thr, excl,
                                      other_atoms_mask=bt['other'], rec_files=['a', 'far', 'b'])
    assert skipped == [(1, 'no pocket atom')] and data['rec_files'] == ['a', 'b']
    n_a, n_b = a['pocket_pos'].shape[0], b['pocket_pos'].shape[0]
    assert data['rec_segments'].tolist() == [0, n_a, n_a + n_b]
    assert torch.equal(data['rec_pos'].cpu(), torch.cat([a['pocket_pos'], b['pocket_pos']]))
    assert torch.equal(data['rec_feat'].cpu(), torch.cat([a['pocket_feat'], b['pocket_feat']])) and data['rec_feat'].dtype == torch.bool
    assert torch.equal(data['interface_points'].cpu(), torch.cat([a['ip_box'], b['ip_box']]))
    assert data['ip_segments'].tolist() == [0, a['ip_box'].shape[0], a['ip_box'].shape[0] + b['ip_box'].shape[0]]
    assert torch.equal(data['lig_pos'].cpu(), torch.cat([a['lig_pos'], b['lig_pos']]))
    with pytest.raises(P.InterfacePointException):
        P.get_pocket_atoms(a['rec_pos_d'], a['rec_feat_d'], a['other_d'], a['rec_res_d'], far['lig_pos'].to(cuda), pad, cut, thr, excl)
    with pytest.raises(P.InterfacePointException):
        P.get_interface_points(far['lig_pos'].to(cuda), a['rec_pos_d'])
    with pytest.raises(ValueError):
        P.select_pocket_residues(a['rec_pos_d'], a['rec_res_d'], far['lig_pos'].to(cuda), cut)


def test_small_large_and_degenerate_inputs(cuda):
    # a one-atom receptor
    pos, res, lig = small_complex(1, 5, seed=1, spread=0.5)
    sel, ip = run_one(pos, res, lig, cuda)
    assert sel['rows'].tolist() == [0] and ip['points'].shape[0] >= 1
    # a 1024-atom ligand (the limit); one more is refused, at both levels, without touching memory
    pos, res, lig = small_complex(400, 1024, seed=2, spread=8.0)
    run_one(pos, res, lig, cuda, excl=1.0)
    big = torch.cat([lig, lig[:1]])
    with pytest.raises(hip.KpdError):
        P.get_interface_points(big.to(cuda), pos.to(cuda))
    sel = hip.pocket_select(pos.to(cuda), ptr32([400], cuda), res.to(cuda), torch.ones(400, dtype=torch.bool, device=cuda),
                            torch.ones(400, dtype=torch.bool, device=cuda), big.to(cuda), ptr32([1025], cuda), 400, 6.0, 4.0)
    assert sel['status'] == [BAD_SEGMENT] and sel['rows'].numel() == 0
    ip = hip.interface_points(pos.to(cuda), ptr32([400], cuda), torch.ones(400, dtype=torch.bool, device=cuda), big.to(cuda), ptr32([1025], cuda), 5.0, 2.0)
    assert ip['status'] == [BAD_SEGMENT] and ip['points'].numel() == 0
    # residue indices with gaps, atoms of a residue not adjacent
    pos, res, lig = small_complex(300, 12, seed=3)
    g = torch.Generator().manual_seed(4)
    shuffled = (res * 3 + 1)[torch.randperm(300, generator=g)]
    sel, _ = run_one(pos, shuffled, lig, cuda)
    assert sel['rows'].numel() > 20
    # residue indices outside [0, n): reported, those atoms are never selected, the others as usual
    bad = shuffled.clone()
    bad[5], bad[77], bad[200] = 300, -1, 2 ** 30
    sel, _ = run_one(pos, bad, lig, cuda)
    assert sel['status'][0] & BAD_RES
    # NaN coordinates: a receptor atom with one passes no test (alone in its residue it stays out; as part of a selected residue
    # it comes along, as with upstream's torch.isin); a ligand NaN poisons the box (torch.min) and nothing is selected
    near = int(torch.cdist(pos, lig).min(dim=1).values.argmin())
    own = res.clone()
    own[near] = 299
    sel, _ = run_one(pos, own, lig, cuda)
    assert near in sel['rows'].tolist()
    nan_pos = pos.clone()
    nan_pos[near, 1] = float('nan')
    sel, _ = run_one(nan_pos, own, lig, cuda)
    assert near not in sel['rows'].tolist()
    run_one(nan_pos, res, lig, cuda)
    nan_lig = lig.clone()
    nan_lig[3, 0] = float('nan')
    sel, _ = run_one(pos, res, nan_lig, cuda)
    assert sel['status'][0] & EMPTY
    run_one(pos, res, nan_lig, cuda, pad=None)                       # no box: the other ligand atoms still select
    # probe / emit all zero
    zeros = torch.zeros(300, dtype=torch.bool)
    sel, ip = run_one(pos, res, lig, cuda, probe=zeros)
    assert sel['status'][0] & EMPTY and ip['status'][0] & EMPTY
    sel, ip = run_one(pos, res, lig, cuda, emit=zeros)
    assert sel['status'][0] & EMPTY and sel['rows'].numel() == 0
    # an empty batch and an empty receptor
    hip.pocket_select(pos[:0].to(cuda), ptr32([], cuda), res[:0].to(cuda), zeros[:0].to(cuda), zeros[:0].to(cuda), lig[:0].to(cuda), ptr32([], cuda), 0, 6.0, 4.0)
    sel, ip = run_one(pos[:0], res[:0], lig, cuda)
    assert sel['status'] == [EMPTY]


# The offsets of both entry points come from the library's one scan kernel (csrc/scan_core.h): a single workgroup that takes
# SCAN_T counts per chunk and carries the running sum from chunk to chunk.
SCAN_T = 1024          # SCAN_THREADS of csrc/scan_core.h; test_scan_t_is_the_kernels_block_size holds the two together


def run_small(parts, dev):
    """Both entry points on a list of (pos, res, lig) with run_one's parameters; everything on the host."""
    cat = lambda k, dt: torch.cat([p[k] for p in parts]).to(dt).to(dev)
    rc, lc = [p[0].shape[0] for p in parts], [p[2].shape[0] for p in parts]
    pos, res, lig, rp, lp = cat(0, torch.float32), cat(1, torch.int32), cat(2, torch.float32), ptr32(rc, dev), ptr32(lc, dev)
    ones = torch.ones(sum(rc), dtype=torch.bool, device=dev)
    sel = hip.pocket_select(pos, rp, res, ones, ones, lig, lp, max(rc), 6.0, 4.0)
    ip = hip.interface_points(pos, rp, sel['pocket_mask'], lig, lp, 5.0, 2.0)
    return dict(rows=sel['rows'].long().cpu(), pocket_res=sel['pocket_res'].long().cpu(), pocket_ptr=sel['pocket_ptr'], status=sel['status'],
                points=ip['points'].cpu(), ip_ptr=ip['ip_ptr'], n_cand=ip['n_cand'], ip_status=ip['status'], n_rec=sum(rc))


@pytest.fixture(scope='module')
def many_small(cuda):
    """2 SCAN_T + 1 small complexes, a few without receptor atoms or with the ligand far away (zero counts mid-scan), and what
    slices of at most 64 of them give, per complex with rows counted from the complex's first atom."""
    g = torch.Generator().manual_seed(77)
    n = 2 * SCAN_T + 1
    nr, nl = torch.randint(8, 21, (n,), generator=g).tolist(), torch.randint(3, 7, (n,), generator=g).tolist()
    parts = []
    for i in range(n):
        pos, res, lig = small_complex(0 if i % 97 == 40 else nr[i], nl[i], seed=1000 + i)
        parts.append((pos, res, lig + 1000.0 if i % 101 == 5 else lig))
    per = []
    for lo in range(0, n, 64):
        r = run_small(parts[lo:lo + 64], cuda)
        off = 0
        for k, p in enumerate(parts[lo:lo + 64]):
            p0, p1, q0, q1 = r['pocket_ptr'][k], r['pocket_ptr'][k + 1], r['ip_ptr'][k], r['ip_ptr'][k + 1]
            per.append(dict(rows=r['rows'][p0:p1] - off, pocket_res=r['pocket_res'][p0:p1], points=r['points'][q0:q1], n_cand=r['n_cand'][k],
                            status=r['status'][k], ip_status=r['ip_status'][k]))
            off += p[0].shape[0]
    return parts, per


@pytest.mark.parametrize('B', [1, SCAN_T - 1, SCAN_T, SCAN_T + 1, 2 * SCAN_T + 1])
def test_offsets_across_the_chunks_of_the_scan(many_small, cuda, B):
    parts, per = many_small
    got = run_small(parts[:B], cuda)
    first = [0] + list(np.cumsum([p[0].shape[0] for p in parts[:B]]))
    want = per[:B]
    assert got['pocket_ptr'] == [0] + list(np.cumsum([w['rows'].numel() for w in want]))          # offsets shifted on the host
    assert got['ip_ptr'] == [0] + list(np.cumsum([w['points'].shape[0] for w in want]))
    assert torch.equal(got['rows'], torch.cat([w['rows'] + first[k] for k, w in enumerate(want)]))
    assert torch.equal(got['pocket_res'], torch.cat([w['pocket_res'] for w in want]))
    assert torch.equal(got['points'], torch.cat([w['points'] for w in want]))
    for k in ('n_cand', 'status', 'ip_status'):
        assert got[k] == [w[k] for w in want], k
    if B > 1:                                                   # the batch has complexes with nothing selected, and ones with something
        assert 0 < sum(st == EMPTY for st in got['status']) < B and got['pocket_ptr'][-1] > 0 and got['ip_ptr'][-1] > 0


def test_scan_t_is_the_kernels_block_size():
    import os
    import re
    src = open(os.path.join(os.path.dirname(hip.__file__), 'csrc', 'scan_core.h')).read()
    assert int(re.search(r'constexpr int SCAN_THREADS = (\d+);', src).group(1)) == SCAN_T
    assert 2 * SCAN_T < 1040 + 1000 + 30 < 3 * SCAN_T       # the source-CSR batch of test_recenc_train_gpu.py: three chunks, the last partial


def test_no_complexes_at_all(cuda):
    none = run_small([small_complex(0, 0, seed=1)], cuda)       # one complex without atoms: offsets [0, 0]
    assert none['pocket_ptr'] == [0, 0] and none['ip_ptr'] == [0, 0]
    z3, zi, zb, p0 = torch.zeros(0, 3, device=cuda), torch.zeros(0, dtype=torch.int32, device=cuda), torch.zeros(0, dtype=torch.bool, device=cuda), ptr32([], cuda)
    sel = hip.pocket_select(z3, p0, zi, zb, zb, z3, p0, 0, 6.0, 4.0)
    ip = hip.interface_points(z3, p0, zb, z3, p0, 5.0, 2.0)
    assert sel['pocket_ptr'] == [0] and sel['status'] == [] and ip['ip_ptr'] == [0] and ip['n_cand'] == [] and ip['status'] == []


def test_capacities_one_too_small(cases, cuda):
    cs = [cases[0], cases[4]]
    pad, cut, thr, excl = cs[0]['params']
    b = batch_of(cs, cuda)
    n_rec, n_lig, B = sum(b['rc']), sum(b['lc']), 2
    rp, lp, keep = ptr32(b['rc'], cuda), ptr32(b['lc'], cuda), (~b['other']).view(torch.uint8)
    full = run_batch(cs, cuda, pad, cut, thr, excl, 'box')
    need_rows = sum(r['rows'].numel() for r in full)
    L = hip.lib()

    def select(cap):
        rows, p_rows = guarded(cap, torch.int32, cuda, -7)
        pres, p_pres = guarded(cap, torch.int32, cuda, -7)
        in_box, mask = torch.empty(n_rec, dtype=torch.uint8, device=cuda), torch.empty(n_rec, dtype=torch.uint8, device=cuda)
        meta = torch.empty(2 * B + 1, dtype=torch.int32, device=cuda)
        nb = int(L.kpd_pocket_scratch_bytes(n_rec, B))
        scratch, p_scr = guarded(nb, torch.uint8, cuda, 0x5a)
        hip.check(L.kpd_pocket_select(b['pos'].data_ptr(), rp.data_ptr(), b['res'].data_ptr(), keep.data_ptr(), keep.data_ptr(), n_rec, max(b['rc']),
                                      b['lig'].data_ptr(), lp.data_ptr(), n_lig, B, pad, cut, cap, in_box.data_ptr(), mask.data_ptr(), p_rows, p_pres,
                                      meta.data_ptr(), meta.data_ptr() + 4 * (B + 1), p_scr, None))
        torch.cuda.synchronize()
        assert intact(rows, cap, -7) and intact(pres, cap, -7) and intact(scratch, nb, 0x5a)
        host = meta.cpu().tolist()
        return rows[GUARD:GUARD + cap], host[:B + 1], host[B + 1:], in_box

    rows, ptr, status, in_box = select(need_rows)
    assert status == [0, 0] and ptr[-1] == need_rows
    rows, ptr, status, _ = select(need_rows - 1)
    assert status == [0, CAPACITY] and ptr[-1] == need_rows                     # the exact size needed is reported
    n0 = full[0]['rows'].numel()
    assert torch.equal(rows[:n0].long().cpu(), full[0]['rows']) and bool((rows[n0:] == -7).all())   # nothing of the complex that does not fit

    cand = (in_box.bool() & keep.bool()).view(torch.uint8)
    n_cand = [r['n_cand'] for r in full]
    need_pts = sum(r['points'].shape[0] for r in full)

    def points(cap_cand, cap_pts):
        pts, p_pts = guarded(cap_pts * 3, torch.float32, cuda, -7.0)
        meta = torch.empty(3 * B + 1, dtype=torch.int32, device=cuda)
        nb = int(L.kpd_interface_points_scratch_bytes(n_rec, B, cap_cand))
        scratch, p_scr = guarded(nb, torch.uint8, cuda, 0x5a)
        base = meta.data_ptr()
        hip.check(L.kpd_interface_points(b['pos'].data_ptr(), rp.data_ptr(), cand.data_ptr(), n_rec, b['lig'].data_ptr(), lp.data_ptr(), n_lig, B, thr,
                                         excl, cap_cand, cap_pts, p_pts, base, base + 4 * (B + 1), base + 4 * (2 * B + 1), p_scr, None))
        torch.cuda.synchronize()
        assert intact(pts, cap_pts * 3, -7.0) and intact(scratch, nb, 0x5a)
        host = meta.cpu().tolist()
        return pts[GUARD:GUARD + cap_pts * 3].view(-1, 3), host[:B + 1], host[B + 1:2 * B + 1], host[2 * B + 1:]

    pts, ptr, nc, status = points(max(n_cand), need_pts)
    assert status == [0, 0] and nc == n_cand and ptr[-1] == need_pts
    assert torch.equal(pts.cpu(), torch.cat([r['points'] for r in full]))
    pts, ptr, nc, status = points(max(n_cand), need_pts - 1)
    assert status == [0, CAPACITY] and ptr[-1] == need_pts and nc == n_cand
    k0 = full[0]['points'].shape[0]
    assert torch.equal(pts[:k0].cpu(), full[0]['points']) and bool((pts[k0:] == -7.0).all())
    big = int(np.argmax(n_cand))
    pts, ptr, nc, status = points(max(n_cand) - 1, need_pts)
    assert nc == n_cand and status[big] == CAPACITY and status[1 - big] == 0     # the exact candidate count is reported
    q0, q1 = ptr[1 - big], ptr[1 - big + 1]
    assert torch.equal(pts[q0:q1].cpu(), full[1 - big]['points'])               # the neighbour is untouched by the overflow
    # the Python layer grows the candidate capacity itself
    ip = P._points(b['pos'], rp, cand, b['lig'], lp, thr, excl)
    assert ip['status'] == [0, 0]


# ---- 5. end to end ------------------------------------------------------------------------------------------------
REC_EL = ['C', 'N', 'O', 'S', 'P', 'F', 'Cl', 'Br', 'I', 'B']


def synthetic_structures(n_res_list, n_lig_list, seed):
    """Whole receptors (globules of residues, a few "other" atoms) with a ligand inside, as flat arrays + segment tables."""
    g = torch.Generator().manual_seed(seed)
    pos, el, res, lig, lig_el = [], [], [], [], []
    for n_res, n_lig in zip(n_res_list, n_lig_list):
        per = torch.randint(4, 10, (n_res,), generator=g)
        n = int(per.sum())
        R = (3 * n / 0.05 / (4 * np.pi)) ** (1 / 3)
        c = torch.randn(n_res, 3, generator=g)
        c = c / c.norm(dim=1, keepdim=True) * R * torch.rand(n_res, 1, generator=g) ** (1 / 3)
        pos.append(torch.repeat_interleave(c, per, dim=0) + torch.randn(n, 3, generator=g) * 1.5 + torch.tensor([30.0, -20.0, 10.0]))
        res.append(torch.repeat_interleave(torch.arange(n_res), per).to(torch.int32))
        e = torch.randint(0, 4, (n,), generator=g)
        e[torch.rand(n, generator=g) < 0.02] = len(REC_EL)                            # "other"
        el.append(e)
        steps = torch.randn(n_lig, 3, generator=g)
        lig.append(torch.cumsum(1.5 * steps / steps.norm(dim=1, keepdim=True), dim=0) + torch.tensor([30.0, -20.0, 10.0]))
        lig_el.append(torch.randint(0, 10, (n_lig,), generator=g))
    el = torch.cat(el)
    seg = lambda parts: [0] + list(np.cumsum([p.shape[0] for p in parts]))
    return dict(rec_pos=torch.cat(pos), rec_feat=torch.nn.functional.one_hot(el, len(REC_EL) + 1)[:, :-1].bool(), other=el == len(REC_EL),
                rec_res=torch.cat(res), rec_seg=seg(pos), lig_pos=torch.cat(lig), lig_feat=torch.nn.functional.one_hot(torch.cat(lig_el), 10).bool(),
                lig_seg=seg(lig))


def test_raw_structures_to_sampling_and_a_training_step(cuda):
    from keypoint_diffusion_amd import dataset as kdata, optim, synth, utils as kutils
    from keypoint_diffusion_amd.ligand_diffuser import KeypointDiffusion
    s = synthetic_structures([260, 300, 220], [12, 18, 9], seed=5)
    d = {k: (v.to(cuda) if isinstance(v, torch.Tensor) else v) for k, v in s.items()}
    data, skipped = P.extract_pockets(d['rec_pos'], d['rec_feat'], d['rec_res'], d['rec_seg'], d['lig_pos'], d['lig_feat'], d['lig_seg'],
                                      lig_box_padding=6, pocket_cutoff=5, interface_distance_threshold=5, interface_exclusion_threshold=2,
                                      other_atoms_mask=d['other'], lig_files=['a.sdf', 'b.sdf', 'c.sdf'])
    assert skipped == [] and data['lig_files'] == ['a.sdf', 'b.sdf', 'c.sdf']
    sizes = (data['rec_segments'][1:] - data['rec_segments'][:-1]).tolist()
    n_ip = (data['ip_segments'][1:] - data['ip_segments'][:-1]).tolist()
    print('pocket atoms', sizes, 'interface points', n_ip)
    assert min(sizes) >= 20 and max(sizes) <= 2048 and min(n_ip) >= 2
    cut = dict(util.CUTOFFS_ALL_ATOM, kl=8, ll=5)
    ds = kdata.ProteinLigandDataset('byop', data, REC_EL, REC_EL, n_keypoints=8, graph_cutoffs=cut)
    assert len(ds) == 3
    # (a) byop.py:254-334: sample into a pocket cut here, write XYZ
    model = KeypointDiffusion(10, 10, None, n_timesteps=4, architecture='egnn', rec_encoder_type='fixed',
                              graph_config=dict(n_keypoints=8, graph_cutoffs=cut), dynamics_config=dict(util.EGNN_C2, n_layers=2),
                              rec_encoder_config={'vector_size': 16}, precision=1e-5)
    synth.fill_state_dict_(model, 13)
    model = model.eval().cuda()
    g1, _ = ds[1]
    pos, feat = model.sample_given_pocket(g1, torch.tensor([9, 11]))
    blocks = kutils.sampled_ligands_xyz([p.cuda() for p in pos], [f.cuda() for f in feat], REC_EL)
    assert [blk[1].split('\n')[0] for blk in blocks] == ['9', '11'] and all(torch.isfinite(p).all() for p in pos)
    # (b) train.py:524: one optimizer step of a learned-encoder model whose encoder loss targets the interface points
    rec_cfg = dict(coords_range=10, fix_pos=False, hidden_n_node_feat=64, k_closest=4, kp_feat_scale=1.0, kp_rad=0.0, message_norm=0.0,
                   n_convs=2, n_kk_convs=0, n_kk_heads=4, no_cg=False, norm=True, out_n_node_feat=64, use_sameres_feat=True, use_tanh=True,
                   in_n_node_feat=10)
    learned = KeypointDiffusion(10, 64, None, n_timesteps=50, architecture='egnn', rec_encoder_type='learned',
                                graph_config=dict(n_keypoints=8, graph_cutoffs=cut), dynamics_config=dict(util.EGNN_C2, n_layers=2, message_norm=0.0),
                                rec_encoder_config=rec_cfg, rec_encoder_loss_config=dict(loss_type='optimal_transport', use_interface_points=True),
                                precision=1e-5)
    synth.fill_state_dict_(learned, 3)
    learned = learned.to(cuda).train()
    opt = optim.Adam(learned.parameters(), lr=1e-4)
    torch.manual_seed(0)
    g, ips = ds.get_batch([0, 1, 2])
    assert [int(p.shape[0]) for p in ips] == n_ip
    out = learned(g, ips)
    total = out['l2'] + 0.1 * out['rec_encoder']
    opt.zero_grad(set_to_none=True)
    total.backward()
    opt.step()
    vals = {k: float(v.detach()) for k, v in out.items() if v is not None}
    print('losses', vals)
    assert all(np.isfinite(v) for v in vals.values()) and vals['rec_encoder'] > 0
    assert all(torch.isfinite(p).all() for p in learned.parameters())
