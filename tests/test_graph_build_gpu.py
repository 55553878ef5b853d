"""GPU: the graph builders of csrc/graph_build.hip against the fp64 oracle on the cases of graph_cases.py, exactly: same
edges in the same order, same row pointers and counts, nothing written past the edge count.  test_graph_cases.py shows on the
CPU that these cases reach the neighbour caps, pairs on the cutoff, kNN ties, more than 1024 complexes, the launch-geometry
switches and the size limits."""
import functools

import pytest
import torch

from keypoint_diffusion_amd import hip
from oracle import graph_ops as og

from . import graph_cases as gc

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _lig_on_device(name, dev):
    lig_x, nl, kp_x, nk = gc.lig_case(name)
    empty = torch.zeros(0, dtype=torch.long)
    return hip.PreparedBatch(nl, nk, empty, empty, dev), lig_x.to(dev), kp_x.to(dev)


@functools.lru_cache(maxsize=None)
def _rec_on_device(name, dev):
    x, counts, res = gc.rec_case(name)
    return x.to(dev), og.counts_to_ptr(counts).int().to(dev), (None if res is None else res.to(dev))


def _same_list(what, label, got, ref, owner):
    """got / ref: (src, dst) long CPU tensors; owner[e] = complex of reference edge e's dst."""
    n = min(got[0].numel(), ref[0].numel())
    diff = torch.nonzero((got[0][:n] != ref[0][:n]) | (got[1][:n] != ref[1][:n])).flatten()
    if diff.numel() == 0 and got[0].numel() == ref[0].numel():
        return
    if diff.numel():
        e = int(diff[0])
        detail = f'first differs at edge {e} (complex {int(owner[e])}): got ({int(got[0][e])} -> {int(got[1][e])}), ' \
                 f'expected ({int(ref[0][e])} -> {int(ref[1][e])}); {diff.numel()} of {n} differ'
    else:
        detail = f'first {n} edges agree'
    pytest.fail(f'{what}: {label}: {got[0].numel()} edges, expected {ref[0].numel()}; {detail}')


def _inside(what, label, idx, n, bidx):
    assert idx.numel() == 0 or (int(idx.min()) >= 0 and int(idx.max()) < n), f'{what}: {label} index outside 0..{n - 1}'
    return bidx[idx]


@pytest.mark.parametrize('name,ll_k,kl_k', gc.LIG_RUNS)
def test_lig_graph(cuda, name, ll_k, kl_k):
    what = f'{name} (ll_k={ll_k}, kl_k={kl_k})'
    c = gc.LIG_CASES[name]
    pb, lig_x, kp_x = _lig_on_device(name, cuda)
    out = hip.build_lig_graph(pb, lig_x, kp_x, c.ll_cut, kl_k, ll_k=ll_k, kl_cutoff=c.kl_cut)
    torch.cuda.synchronize()
    out = {k: v.long().cpu() for k, v in out.items()}
    ref = gc.lig_reference(name, ll_k, kl_k)
    _, nl, _, nk = gc.lig_case(name)
    lig_b, kp_b = og.counts_to_batch_idx(nl), og.counts_to_batch_idx(nk)
    E_ll, E_kl = ref['ll_src'].numel(), ref['lk_src'].numel()

    assert out['counts'][0] == E_ll and out['counts'][1] == E_kl, f'{what}: counts {out["counts"][:2].tolist()}, expected {[E_ll, E_kl]}'
    assert not out['counts'][2:].any(), f'{what}: counts[2:] written'
    pg = torch.nonzero(out['ll_per_graph'] != ref['ll_per_graph']).flatten()
    assert pg.numel() == 0, f'{what}: ll_per_graph differs first at complex {int(pg[0])}: {int(out["ll_per_graph"][pg[0]])}, ' \
                            f'expected {int(ref["ll_per_graph"][pg[0]])}'
    for lst, n_src, src_b, n_dst, dst_b, E in (('ll', pb.n_lig, lig_b, pb.n_lig, lig_b, E_ll), ('lk', pb.n_lig, lig_b, pb.n_kp, kp_b, E_kl),
                                               ('kl', pb.n_kp, kp_b, pb.n_lig, lig_b, E_kl)):
        src, dst = out[f'{lst}_src'], out[f'{lst}_dst']
        _same_list(what, lst, (src[:E], dst[:E]), (ref[f'{lst}_src'], ref[f'{lst}_dst']), dst_b[ref[f'{lst}_dst']])
        assert not src[E:].any() and not dst[E:].any(), f'{what}: {lst} wrote past its {E} edges'
        own_s, own_d = _inside(what, f'{lst}_src', src[:E], n_src, src_b), _inside(what, f'{lst}_dst', dst[:E], n_dst, dst_b)
        assert torch.equal(own_s, own_d), f'{what}: {lst} edge across complexes'
        rp = torch.nonzero(out[f'{lst}_rowptr'] != ref[f'{lst}_rowptr']).flatten()
        assert out[f'{lst}_rowptr'].numel() == n_dst + 1 and rp.numel() == 0, \
            f'{what}: {lst}_rowptr differs first at row {int(rp[0])} of {n_dst}: {int(out[f"{lst}_rowptr"][rp[0]])}, ' \
            f'expected {int(ref[f"{lst}_rowptr"][rp[0]])}'
    assert bool((out['ll_src'][:E_ll] != out['ll_dst'][:E_ll]).all()), f'{what}: ll self loop'


@pytest.mark.parametrize('max_lig,max_kp,message', [
    (1024, 1057, r'knn needs 155664 B of LDS \(max_x=1024, max_y=1057\)'),
    (1025, 1056, r'max_lig=1025 outside 1\.\.1024'),
])
def test_lig_graph_refuses_past_the_limits(cuda, max_lig, max_kp, message):
    lig_x, nl, kp_x, nk = gc.limits(max_lig, max_kp)
    empty = torch.zeros(0, dtype=torch.long)
    pb = hip.PreparedBatch(nl, nk, empty, empty, cuda)
    with pytest.raises(hip.KpdError, match=message):
        hip.build_lig_graph(pb, lig_x.to(cuda), kp_x.to(cuda), 2.5, 5)
    torch.cuda.synchronize()


@pytest.mark.parametrize('name', list(gc.REC_CASES))
def test_rec_graph(cuda, name):
    x, ptr, res = _rec_on_device(name, cuda)
    _, counts, _ = gc.rec_case(name)
    n_rec, bidx = int(counts.sum()), og.counts_to_batch_idx(counts)
    src, dst, per_graph, same, rowptr = hip.build_rec_graph(x, ptr, int(counts.max()), gc.REC_R, res, max_nn=gc.REC_CASES[name].max_nn,
                                                            return_rowptr=True)
    torch.cuda.synchronize()
    src, dst, per_graph, rowptr = src.long().cpu(), dst.long().cpu(), per_graph.long().cpu(), rowptr.long().cpu()
    ref = gc.rec_reference(name)
    _same_list(name, 'rr', (src, dst), (ref['src'], ref['dst']), bidx[ref['dst']])
    assert torch.equal(_inside(name, 'src', src, n_rec, bidx), _inside(name, 'dst', dst, n_rec, bidx)), f'{name}: edge across pockets'
    assert bool((src != dst).all()) and bool((dst[1:] >= dst[:-1]).all()), f'{name}: self loop or not dst-major'
    pg = torch.nonzero(per_graph != ref['per_graph']).flatten()
    assert pg.numel() == 0, f'{name}: per_graph differs first at pocket {int(pg[0])}'
    rp = torch.nonzero(rowptr != ref['rowptr']).flatten()
    assert rowptr.numel() == n_rec + 1 and rp.numel() == 0, f'{name}: rowptr differs first at row {int(rp[0])} of {n_rec}'
    if res is None:
        assert same is None
    else:
        assert same.dtype == torch.bool and torch.equal(same.cpu(), ref['same_res']), f'{name}: same_res differs'
        assert bool(ref['same_res'].any()) and not bool(ref['same_res'].all())
    assert len(hip.build_rec_graph(x, ptr, int(counts.max()), gc.REC_R, res, max_nn=gc.REC_CASES[name].max_nn)) == 4     # default return


def test_rec_graph_scratch_guard_bands(cuda):
    """kpd_build_rec_graph through the C ABI with guard bands on both sides of exactly kpd_rec_graph_scratch_bytes."""
    from .util import guarded, intact
    name = 'rec_sizes'                                   # pockets of 1, 2 and 2048 atoms
    x, ptr, res = _rec_on_device(name, cuda)
    _, counts, _ = gc.rec_case(name)
    ref = gc.rec_reference(name)
    n_rec, B, E = int(counts.sum()), counts.numel(), ref['src'].numel()
    L = hip.lib()
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=cuda)
    src, dst, rowptr, per_graph, cnt = i32(E), i32(E), i32(n_rec + 1), i32(B), i32(2)
    same = torch.empty(E, dtype=torch.uint8, device=cuda)
    nb = int(L.kpd_rec_graph_scratch_bytes(n_rec, B))
    scratch, p_scr = guarded(nb, torch.uint8, cuda, 0x5a)
    hip.check(L.kpd_build_rec_graph(x.data_ptr(), ptr.data_ptr(), B, n_rec, int(counts.max()), gc.REC_R, gc.REC_CASES[name].max_nn,
                                    res.data_ptr(), E, src.data_ptr(), dst.data_ptr(), rowptr.data_ptr(), per_graph.data_ptr(),
                                    same.data_ptr(), cnt.data_ptr(), p_scr, None))
    torch.cuda.synchronize()
    assert intact(scratch, nb, 0x5a), f'{name}: wrote outside the {nb} bytes of scratch'
    assert cnt.tolist() == [E, 0]
    _same_list(name, 'rr', (src.long().cpu(), dst.long().cpu()), (ref['src'], ref['dst']), og.counts_to_batch_idx(counts)[ref['dst']])
    assert torch.equal(rowptr.long().cpu(), ref['rowptr']) and torch.equal(per_graph.long().cpu(), ref['per_graph'])
    assert torch.equal(same.bool().cpu(), ref['same_res'])


def test_rec_graph_refuses_past_the_limit(cuda):
    x, counts, _ = gc.rec_over_limit()
    with pytest.raises(hip.KpdError, match=r'radius graph: 2049 nodes per graph \(max 2048\)'):
        hip.build_rec_graph(x.to(cuda), og.counts_to_ptr(counts).int().to(cuda), 2049, gc.REC_R)
    torch.cuda.synchronize()
