"""Pocket extraction without a GPU: the entry points exist and agree between header, library and binding, the wrappers
refuse CPU tensors, and a float64 torch restatement of upstream's selection (written here, used by test_pocket_gpu.py
as well) reproduces every fixture the reference's own get_pocket_atoms / get_interface_points produced
(tests/golden/pocket_XX.npz, make_pocket_golden.py), inside the margins that make a selection test meaningful."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from keypoint_diffusion_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ['kpd_pocket_scratch_bytes', 'kpd_pocket_select', 'kpd_interface_points_scratch_bytes', 'kpd_interface_points']
MARGIN = 1e-4       # the band of the graph builders: ~100 x the fp32 rounding of a direct difference at 8 A


# ---- fixtures -----------------------------------------------------------------------------------------------------
def load_cases():
    files = sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', 'pocket_[0-9][0-9].npz')))
    cases = []
    for f in files:
        z = np.load(f)
        c = {k: torch.from_numpy(z[k]) for k in ('rec_pos', 'rec_res', 'lig_pos', 'byres_mask', 'pocket_pos', 'pocket_feat', 'ip_box', 'ip_pocket')}
        c['n_el'] = len(z['elements'])
        c['rec_el'] = torch.from_numpy(z['rec_el'].astype(np.int64))
        c['other'] = c['rec_el'] == c['n_el']
        c['rec_feat'] = torch.nn.functional.one_hot(c['rec_el'], c['n_el'] + 1)[:, :-1].bool()       # rec_atom_featurizer :161-168
        c['params'] = tuple(float(v) for v in z['params'])                # box_padding, pocket_cutoff, dist_thr, excl_thr
        c['margins'], c['n_rejected'], c['name'] = z['margins'], int(z['n_rejected']), os.path.basename(f)
        cases.append(c)
    return cases


# ---- float64 restatement ------------------------------------------------------------------------------------------
def d2_matrix(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Squared distances from direct differences, float64 on the fp32 coordinates (the differences are exact)."""
    return (a.double()[:, None, :] - b.double()[None, :, :]).square().sum(-1)


def restate_select(pos, res, probe, emit, lig, box_padding, cutoff):
    """pdbbind_processing.py:92-138 / process_bindingmoad.py:124-161 on arrays.  Returns in_box, pocket mask (over the input
    rows), rows, pocket_res (rank of the residue among the selected ones, by first appearance), bad_res."""
    n = pos.shape[0]
    if box_padding is None:
        in_box = torch.ones(n, dtype=torch.bool)
    else:
        lo = lig.min(dim=0).values - box_padding                         # fp32, as upstream (:92-97)
        hi = lig.max(dim=0).values + box_padding
        in_box = (pos >= lo).all(dim=1) & (pos <= hi).all(dim=1)          # :114-117
    valid = (res >= 0) & (res < n)
    near = torch.zeros(n, dtype=torch.bool)
    idx = torch.nonzero(in_box & probe.bool() & valid).flatten()
    if idx.numel() and lig.shape[0]:
        near[idx] = (d2_matrix(pos[idx], lig) < float(cutoff) ** 2).any(dim=1)       # min d < cutoff (:127-128)
    flag = torch.zeros(max(n, 1), dtype=torch.bool)
    flag[res[near].long()] = True
    mask = emit.bool() & valid & flag[res.clamp(0, max(n - 1, 0)).long()]             # torch.isin (:134)
    rows = torch.nonzero(mask).flatten()
    seen = {}
    pocket_res = torch.tensor([seen.setdefault(int(r), len(seen)) for r in res[rows]], dtype=torch.long)
    return in_box, mask, rows, pocket_res, bool((~valid).any())


def restate_points(lig, rec, dist_thr, excl_thr, margins=None):
    """pdbbind_processing.py:306-323: candidate pairs in torch.where order, fp32 midpoints, greedy thinning in float64.
    Returns (points, n_candidates); `margins` (a list) receives the distance of the closest exclusion decision to its threshold."""
    d2 = d2_matrix(lig, rec)
    li, ri = torch.where(d2 < float(dist_thr) ** 2)
    mid = (lig[li] + rec[ri]) / 2
    if not mid.shape[0]:
        return mid, 0
    m64 = mid.double()
    sel = [0]
    for i in range(1, mid.shape[0]):
        dmin = (m64[sel] - m64[i]).square().sum(-1).min()
        if margins is not None:
            margins.append(abs(float(dmin.sqrt()) - excl_thr))
        if dmin >= float(excl_thr) ** 2:
            sel.append(i)
    return mid[sel], mid.shape[0]


# ---- tests --------------------------------------------------------------------------------------------------------
def test_entry_points_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'kpd.h')).read()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for s in SYMBOLS:
        assert s + '(' in header and s in hip.EXPORTS and hasattr(lib, s), s
    L = hip.lib()
    assert L.kpd_pocket_scratch_bytes(1000, 4) > 0 and L.kpd_pocket_scratch_bytes(-1, 4) == -1
    assert L.kpd_interface_points_scratch_bytes(1000, 4, 2048) >= 4 * 2048 * 12 and L.kpd_interface_points_scratch_bytes(1, 1, -1) == -1
    from keypoint_diffusion_amd import pocket
    for name in ('get_interface_points', 'get_pocket_atoms', 'select_pocket_residues', 'extract_pockets', 'InterfacePointException'):
        assert hasattr(pocket, name), name
    e = pocket.InterfacePointException(IndexError('x'))
    assert isinstance(e.original_exception, IndexError)


def test_wrappers_refuse_cpu_tensors():
    from keypoint_diffusion_amd import pocket
    pos, lig = torch.randn(12, 3), torch.randn(4, 3)
    res, ones = torch.arange(12, dtype=torch.int32) // 3, torch.ones(12, dtype=torch.bool)
    ptr, lptr = torch.tensor([0, 12], dtype=torch.int32), torch.tensor([0, 4], dtype=torch.int32)
    feat = torch.zeros(12, 5, dtype=torch.bool)
    with pytest.raises(hip.KpdError):
        hip.pocket_select(pos, ptr, res, ones, ones, lig, lptr, 12, 6.0, 4.0)
    with pytest.raises(hip.KpdError):
        hip.interface_points(pos, ptr, ones, lig, lptr, 5.0, 2.0)
    with pytest.raises(hip.KpdError):
        pocket.get_interface_points(lig, pos)
    with pytest.raises(hip.KpdError):
        pocket.get_pocket_atoms(pos, feat, ~ones, res, lig, 6, 4, 5, 2)
    with pytest.raises(hip.KpdError):
        pocket.select_pocket_residues(pos, res, lig, 4)
    with pytest.raises(hip.KpdError):
        pocket.extract_pockets(pos, feat, res, [0, 12], lig, torch.zeros(4, 5, dtype=torch.bool), [0, 4])


def test_fixture_set():
    cases = load_cases()
    assert len(cases) >= 8
    assert sum(c['n_rejected'] for c in cases) <= len(cases), 'more than half of the draws were rejected when the fixtures were made'
    for c in cases:
        n = c['rec_pos'].shape[0]
        assert c['rec_pos'].dtype == torch.float32 and c['rec_res'].dtype == torch.int32 and 3000 < n < 14000
        assert int(c['other'].sum()) > 0 and c['ip_box'].shape[0] > 0 and c['ip_pocket'].shape[0] > 0
        assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', c['name'])) < 1_000_000


@pytest.mark.parametrize('k', range(8))
def test_restatement_reproduces_the_reference_inside_the_margins(k):
    c = load_cases()[k]
    pad, cut, thr, excl = c['params']
    keep = ~c['other']
    in_box, mask, rows, _, bad = restate_select(c['rec_pos'], c['rec_res'], keep, keep, c['lig_pos'], pad, cut)
    assert not bad
    assert torch.equal(mask[keep], c['byres_mask'])                       # indexed over the non-"other" atoms, as upstream
    assert torch.equal(c['rec_pos'][rows], c['pocket_pos']) and torch.equal(c['rec_feat'][rows], c['pocket_feat'])
    m_box, m_pocket = [], []
    pts, _ = restate_points(c['lig_pos'], c['rec_pos'][in_box & keep], thr, excl, m_box)
    assert torch.equal(pts, c['ip_box'])                                  # float64 dist_mat path, box candidate set
    pts, _ = restate_points(c['lig_pos'], c['pocket_pos'], thr, excl, m_pocket)
    assert torch.equal(pts, c['ip_pocket'])                               # fp32 torch.cdist path, pocket candidate set
    # margin condition, float64: no decision of the reference closer than 1e-4 A to its threshold
    d = d2_matrix(c['lig_pos'], c['rec_pos']).sqrt()
    m_thr = float((d - thr).abs().min())
    box = in_box & keep
    m_cut = float((d[:, box].min(dim=0).values - cut).abs().min())
    got = np.array([m_thr, m_cut, min(m_box), min(m_pocket)])
    print(c['name'], 'margins', got)
    assert (got >= MARGIN).all(), got
    assert np.allclose(got, c['margins'], rtol=1e-6, atol=1e-9)          # the generator measured the same thing
