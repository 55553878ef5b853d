"""The segmented distance hinge (kpd_dist_hinge, csrc/dist_hinge.hip) behind `DistanceHingeLoss` / `segmented_dist_hinge`: against
upstream's own module evaluated in float64 (tests/golden/dist_hinge.npz, make_hinge_golden.py), the subgradient edge cases exactly,
and bitwise batch invariance and run-to-run reproducibility of the segmented launch."""
import json
import os

import numpy as np
import pytest
import torch

from keypoint_diffusion_amd.dist_hinge_loss import DistanceHingeLoss, segmented_dist_hinge

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-5


def _golden():
    z = np.load(os.path.join(HERE, 'golden', 'dist_hinge.npz'))
    return z, [str(n) for n in z['names']]


def _ptr(counts, dev):
    return torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32, device=dev)


def test_module_matches_upstream_fixture(cuda):
    z, names = _golden()
    assert len(names) >= 12
    for name in names:
        a = torch.from_numpy(z[f'{name}/a']).to(cuda).requires_grad_(True)
        b = torch.from_numpy(z[f'{name}/b']).to(cuda).requires_grad_(True) if f'{name}/b' in z else None
        loss = DistanceHingeLoss(float(z[f'{name}/thr']))(a, b)
        loss.backward()
        ref = float(z[f'{name}/loss'])
        got = float(loss.detach())
        assert abs(got - ref) <= TOL * max(abs(ref), 1.0), (name, got, ref)
        for t, key in ((a, 'ga'), (b, 'gb')):
            if t is None:
                continue
            g_ref = torch.from_numpy(z[f'{name}/{key}'])
            err = float((t.grad.double().cpu() - g_ref).abs().max()) if g_ref.numel() else 0.0
            assert err <= TOL * max(float(g_ref.abs().max()) if g_ref.numel() else 0.0, 1.0), (name, key, err)


def test_subgradient_edge_cases_are_exact(cuda):
    thr = 2.0
    a = torch.tensor([[0.0, 0.0, 0.0]], device=cuda, requires_grad=True)
    b = torch.tensor([[2.0, 0.0, 0.0]], device=cuda, requires_grad=True)
    loss = DistanceHingeLoss(thr)(a, b)
    loss.backward()
    assert float(loss.detach()) == 0.0
    assert a.grad.tolist() == [[0.5, 0.0, 0.0]] and b.grad.tolist() == [[-0.5, 0.0, 0.0]]      # d == thr: torch.max splits it
    # d == 0: the pair adds thr to the loss and nothing to the gradient (no NaN)
    a = torch.tensor([[1.0, 2.0, 3.0]], device=cuda, requires_grad=True)
    b = torch.tensor([[1.0, 2.0, 3.0]], device=cuda, requires_grad=True)
    loss = DistanceHingeLoss(thr)(a, b)
    (3.0 * loss).backward()
    assert float(loss.detach()) == thr
    assert a.grad.tolist() == [[0.0, 0.0, 0.0]] and b.grad.tolist() == [[0.0, 0.0, 0.0]]
    # backward scales by the incoming gradient
    z, _ = _golden()
    a = torch.from_numpy(z['cross_7x13/a']).to(cuda).requires_grad_(True)
    b = torch.from_numpy(z['cross_7x13/b']).to(cuda)
    (-2.5 * DistanceHingeLoss(float(z['cross_7x13/thr']))(a, b)).backward()
    g_ref = -2.5 * torch.from_numpy(z['cross_7x13/ga'])
    assert float((a.grad.double().cpu() - g_ref).abs().max()) <= TOL * float(g_ref.abs().max())


def _ragged(cuda, n, seed):
    pairs = json.load(open(os.path.join(HERE, 'golden', 'size_pairs.json')))['all_atom']['pairs'][:n]
    gen = torch.Generator().manual_seed(seed)
    rec = [(torch.rand(r, 3, generator=gen) * 14.0) for r, _ in pairs]
    lig = [(torch.rand(l, 3, generator=gen) * 5.0 + 4.5) for _, l in pairs]
    return lig, rec


def test_segmented_is_batch_invariant_and_reproducible(cuda):
    lig, rec = _ragged(cuda, 64, 5)
    lig[3], rec[5] = lig[3][:0], rec[5][:0]                          # an empty ligand and an empty receptor segment
    thr = 3.5
    a = torch.cat(lig).to(cuda).requires_grad_(True)
    b = torch.cat(rec).to(cuda).requires_grad_(True)
    a_ptr, b_ptr = _ptr([len(x) for x in lig], cuda), _ptr([len(x) for x in rec], cuda)
    total, seg = segmented_dist_hinge(a, a_ptr, b, b_ptr, thr)
    total.backward()
    ga, gb = a.grad.clone(), b.grad.clone()
    active = sum(int((torch.cdist(l.double(), r.double()) < thr).sum()) for l, r in zip(lig, rec))
    assert active > 2000 and float(seg[3]) == 0.0 and float(seg[5]) == 0.0

    # a second run: identical bits
    a.grad = b.grad = None
    total2, seg2 = segmented_dist_hinge(a, a_ptr, b, b_ptr, thr)
    total2.backward()
    assert torch.equal(total, total2) and torch.equal(seg, seg2) and torch.equal(ga, a.grad) and torch.equal(gb, b.grad)

    # each complex alone (one launch per complex, the upstream loop): identical bits for its loss and its gradient rows
    ao, bo = 0, 0
    for s, (l, r) in enumerate(zip(lig, rec)):
        la = l.to(cuda).requires_grad_(True)
        rb = r.to(cuda).requires_grad_(True)
        one = DistanceHingeLoss(thr)(la, rb)
        one.backward()
        assert torch.equal(one.detach().reshape(1), seg[s:s + 1]), s
        assert torch.equal(la.grad, ga[ao:ao + len(l)]) and torch.equal(rb.grad, gb[bo:bo + len(r)]), s
        ao, bo = ao + len(l), bo + len(r)
    # and inside a different batch (reordered, half of it): the same bits again
    order = list(range(0, 64, 2))[::-1]
    a3 = torch.cat([lig[i] for i in order]).to(cuda)
    b3 = torch.cat([rec[i] for i in order]).to(cuda)
    _, seg3 = segmented_dist_hinge(a3, _ptr([len(lig[i]) for i in order], cuda), b3, _ptr([len(rec[i]) for i in order], cuda), thr)
    assert torch.equal(seg3, seg[order])

    # the total against a float64 restatement
    ref = sum(float((thr - torch.cdist(l.double(), r.double(), compute_mode='donot_use_mm_for_euclid_dist')).clamp(min=0).sum())
              for l, r in zip(lig, rec))
    assert abs(float(total.detach()) - ref) <= TOL * ref


def test_self_mode_matches_triu_restatement(cuda):
    gen = torch.Generator().manual_seed(8)
    x = torch.rand(5000, 3, generator=gen) * 45.0
    thr = 2.0
    xd = x.to(cuda).requires_grad_(True)
    loss = DistanceHingeLoss(thr)(xd)
    loss.backward()
    x64 = x.double().requires_grad_(True)
    d = torch.cdist(x64, x64, compute_mode='donot_use_mm_for_euclid_dist')
    iu = torch.triu_indices(5000, 5000, offset=1)
    ref = (thr - d[iu[0], iu[1]]).clamp(min=0).sum()
    ref.backward()
    assert int((d[iu[0], iu[1]] < thr).sum()) > 1000
    assert abs(float(loss.detach()) - float(ref.detach())) <= TOL * float(ref.detach())
    err = float((xd.grad.double().cpu() - x64.grad).abs().max())
    assert err <= TOL * float(x64.grad.abs().max()), err


def test_empty_batch_and_loud_errors(cuda):
    e = torch.zeros(0, 3, device=cuda)
    p = torch.zeros(1, dtype=torch.int32, device=cuda)
    total, seg = segmented_dist_hinge(e, p, e, p, 2.0)                # S = 0
    assert seg.numel() == 0 and float(total) == 0.0
    from keypoint_diffusion_amd import hip
    with pytest.raises(hip.KpdError):
        DistanceHingeLoss(2.0)(torch.zeros(3, 3, device=cuda, dtype=torch.float64))
    with pytest.raises(hip.KpdError):
        segmented_dist_hinge(torch.zeros(3, 3, device=cuda), p.long(), None, None, 2.0)
