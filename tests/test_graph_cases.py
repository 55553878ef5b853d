"""CPU: every case of graph_cases.py reaches the path of csrc/graph_build.hip it is named for, shown with the oracle alone.
Without this the GPU comparisons of test_graph_build_gpu.py could pass on inputs that never meet a cap, a boundary or a tie."""
import pytest
import torch

from oracle import graph_ops as og

from . import graph_cases as gc

KL_KMAX = 16


def _complexes(name):
    lig_x, nl, kp_x, nk = gc.lig_case(name)
    lp, kp = og.counts_to_ptr(nl), og.counts_to_ptr(nk)
    for b in range(nl.numel()):
        yield b, lig_x[lp[b]:lp[b + 1]], kp_x[kp[b]:kp[b + 1]], int(lp[b]), int(kp[b])


def _offdiag(d2):
    return d2.masked_fill(torch.eye(d2.shape[0], dtype=torch.bool), float('inf'))


@pytest.mark.parametrize('name', gc.LATTICE_LIG)
def test_lig_lattice_property(name):
    lig_x, nl, kp_x, nk = gc.lig_case(name)
    for x, n in ((lig_x, nl), (kp_x, nk)):
        assert x.dtype == torch.float32 and x.shape == (int(n.sum()), 3)
        assert torch.equal(x * 2, (x * 2).round()) and float(x.abs().max()) <= 32.0
    c = gc.LIG_CASES[name]
    for r in (c.ll_cut, c.kl_cut):                                        # r2 exact in fp32
        assert float(torch.tensor(r, dtype=torch.float32) ** 2) == r * r and (r * r * 4).is_integer()


@pytest.mark.parametrize('name', sorted(set(gc.REC_CASES) | {'over_limit'}))
def test_rec_lattice_property(name):
    x, counts, _ = gc.rec_over_limit() if name == 'over_limit' else gc.rec_case(name)
    assert x.dtype == torch.float32 and x.shape == (int(counts.sum()), 3)
    assert torch.equal(x * 2, (x * 2).round()) and float(x.abs().max()) <= 32.0


@pytest.mark.parametrize('name,seed', list(zip(gc.GENERAL_LIG, gc.GENERAL_SEEDS)))
def test_general_margins(name, seed):
    lig_x, nl, kp_x, nk = gc.lig_case(name)                               # the builder asserts the same
    assert nl.tolist() == [37, 4, 25] and nk.tolist() == [20, 40, 7]
    m_r, m_k = gc.general_margins(lig_x, nl, kp_x, nk, *gc.GENERAL_CUTS)
    print(f'{name} (seed {seed}): smallest cutoff margin {m_r:.3e}, smallest kNN margin {m_k:.3e}')
    assert m_r > gc.MARGIN and m_k > gc.MARGIN
    ref = gc.lig_reference(name, 0, 0)                                    # ordinary data: both sides of both cutoffs occur
    n_pairs_ll = int((nl * (nl - 1)).sum())
    assert 0 < ref['ll_src'].numel() < n_pairs_ll and 0 < ref['lk_src'].numel() < int((nl * nk).sum())


def test_caps_ll_kl_reaches_both_caps():
    over_ll = at_ll = over_kl = at_kl = 0
    ref = gc.lig_reference('caps_ll_kl', 0, 0)
    ll_deg = ref['ll_rowptr'][1:] - ref['ll_rowptr'][:-1]
    lk_deg = ref['lk_rowptr'][1:] - ref['lk_rowptr'][:-1]
    for b, l, k, lo, klo in _complexes('caps_ll_kl'):
        cand_ll = (_offdiag(gc.pair_d2(l, l)) < 36.0).sum(1)
        cand_kl = (gc.pair_d2(l, k) < 36.0).sum(1)
        assert bool((cand_ll == l.shape[0] - 1).all()) and bool((cand_kl == l.shape[0]).all())     # the whole block is in range
        over_ll += int((cand_ll > gc.LL_MAX_NN).sum())
        at_ll += int((cand_ll == gc.LL_MAX_NN).sum())
        over_kl += int((cand_kl > gc.KL_MAX_NN).sum())
        at_kl += int((cand_kl == gc.KL_MAX_NN).sum())
        assert torch.equal(ll_deg[lo:lo + l.shape[0]], cand_ll.clamp(max=gc.LL_MAX_NN))
        assert torch.equal(lk_deg[klo:klo + k.shape[0]], cand_kl.clamp(max=gc.KL_MAX_NN))
    assert over_ll == 216 + 202 and at_ll == 201 and over_kl == 10 and at_kl == 2


@pytest.mark.parametrize('name', ['rec_block_nn1', 'rec_block_nn3', 'rec_block_nn100', 'rec_sizes'])
def test_rec_reaches_cap(name):
    x, counts, _ = gc.rec_case(name)
    max_nn, ptr = gc.REC_CASES[name].max_nn, og.counts_to_ptr(counts)
    cand = torch.cat([(_offdiag(gc.pair_d2(x[ptr[b]:ptr[b + 1]], x[ptr[b]:ptr[b + 1]])) < gc.REC_R ** 2).sum(1) for b in range(counts.numel())])
    assert int((cand > max_nn).sum()) > 0
    if name != 'rec_sizes':
        assert int((cand == max_nn).sum()) > 0 and int((cand == 0).sum()) == 1        # exactly at the cap; the lone atom
    ref = gc.rec_reference(name)
    assert torch.equal(ref['rowptr'][1:] - ref['rowptr'][:-1], cand.clamp(max=max_nn))
    assert bool((ref['src'] != ref['dst']).all())


@pytest.mark.parametrize('name,r,max_nn', [('caps_ll_kl', 6.0, 200), ('limits', 2.5, 200)])
def test_oracle_radius_graph_is_the_rule_lig(name, r, max_nn):
    """oracle.graph_ops.radius_graph gets there through radius(max + 1) and a second truncation; pin it to the rule."""
    lig_x, nl, _, _ = gc.lig_case(name)
    src, dst = gc.direct_radius_graph(lig_x, r, nl, max_nn)
    ref = gc.lig_reference(name, 0, gc.LIG_CASES[name].k_pairs[0][1])
    assert torch.equal(ref['ll_src'], src) and torch.equal(ref['ll_dst'], dst)


@pytest.mark.parametrize('name', ['rec_block_nn1', 'rec_block_nn3', 'rec_block_nn100'])
def test_oracle_radius_graph_is_the_rule_rec(name):
    x, counts, _ = gc.rec_case(name)
    src, dst = gc.direct_radius_graph(x, gc.REC_R, counts, gc.REC_CASES[name].max_nn)
    ref = gc.rec_reference(name)
    assert torch.equal(ref['src'], src) and torch.equal(ref['dst'], dst)


def test_boundary_pairs_exist_and_are_no_edges():
    ref = gc.lig_reference('boundary_ties', 0, 0)
    ll, lk = set(zip(ref['ll_src'].tolist(), ref['ll_dst'].tolist())), set(zip(ref['lk_src'].tolist(), ref['lk_dst'].tolist()))
    n_ll = n_kl = 0
    for b, l, k, lo, klo in _complexes('boundary_ties'):
        for i, j in torch.nonzero(gc.pair_d2(l, l) == 6.25).tolist():      # [centre, neighbour]
            assert (lo + j, lo + i) not in ll
            n_ll += 1
        for p, j in torch.nonzero(gc.pair_d2(l, k) == 6.25).tolist():      # [kp, lig]
            assert (lo + j, klo + p) not in lk
            n_kl += 1
    assert n_ll > 0 and n_kl > 0
    x, counts, _ = gc.rec_case('rec_block_nn100')
    on = torch.nonzero(gc.pair_d2(x, x) == 6.25).tolist()
    rr = set(zip(*[t.tolist() for t in (gc.rec_reference('rec_block_nn100')['src'], gc.rec_reference('rec_block_nn100')['dst'])]))
    assert len(on) > 0 and all((j, i) not in rr for i, j in on)


def test_coincident_atoms():
    zero_ll = zero_kl = 0
    for b, l, k, lo, klo in _complexes('boundary_ties'):
        zero_ll += int((_offdiag(gc.pair_d2(l, l)) == 0).sum())
        zero_kl += int((gc.pair_d2(l, k) == 0).sum())
        assert float(gc.pair_d2(l[:1], k[:1])) == 0.0
    assert zero_ll >= 2 * 5 and zero_kl >= 7


@pytest.mark.parametrize('ll_k,kl_k', [(1, 1), (3, 5), (16, 16)])
def test_knn_ties_at_the_kth_rank(ll_k, kl_k):
    """Some query has its k-th and (k+1)-th candidate at one distance (so the index decides who stays), and some query has a
    strictly nearer candidate of a higher index than two tied ones it keeps (so a kept tie has to move down in order)."""
    tie_ll = tie_kl = shove_ll = shove_kl = 0
    for b, l, k, lo, klo in _complexes('boundary_ties'):
        for d2, kk, which in ((_offdiag(gc.pair_d2(l, l)), ll_k, 'll'), (gc.pair_d2(l, k), kl_k, 'kl')):
            if d2.shape[1] - (which == 'll') <= kk:
                continue                                                   # fewer candidates than k: nothing is cut
            val, idx = torch.sort(d2, dim=1, stable=True)
            ties = int((val[:, kk - 1] == val[:, kk]).sum())
            shove = 0
            if kk >= 2:
                for q in range(d2.shape[0]):
                    for j in range(1, kk):
                        if val[q, j] == val[q, j - 1] and bool(((val[q, :j - 1] < val[q, j]) & (idx[q, :j - 1] > idx[q, j])).any()):
                            shove += 1
            if which == 'll':
                tie_ll, shove_ll = tie_ll + ties, shove_ll + shove
            else:
                tie_kl, shove_kl = tie_kl + ties, shove_kl + shove
    assert tie_ll > 0 and tie_kl > 0
    if min(ll_k, kl_k) >= 3:
        assert shove_ll > 0 and shove_kl > 0


def test_small_complexes_and_mask_words():
    _, nl, _, nk = gc.lig_case('boundary_ties')
    assert nl.tolist() == [1, 2, 3, 16, 17, 64, 65] and nk.tolist() == [1, 31, 32, 33, 64, 65, 2]
    assert int(nl.min()) < 3 < 5 < KL_KMAX                                # k > n and k > n - 1 at (3, 5) and (16, 16)
    assert {16, 17} <= set(nl.tolist())                                   # n - 1 < KL_KMAX, n - 1 == KL_KMAX
    assert {32, 33, 64, 65} <= set(nk.tolist())                           # one, two and three mask words
    ref = gc.lig_reference('boundary_ties', 16, 16)
    assert torch.equal(ref['ll_per_graph'], nl * torch.clamp(nl - 1, max=16))
    assert ref['lk_src'].numel() == int((nk * torch.clamp(nl, max=16)).sum())


@pytest.mark.parametrize('name,B', [('many_complexes_1024', 1024), ('many_complexes_1025', 1025), ('many_complexes_2049', 2049)])
def test_many_complexes_cross_a_scan_chunk(name, B):
    _, nl, _, nk = gc.lig_case(name)
    assert nl.numel() == nk.numel() == B and B >= 1024
    assert nl[:6].tolist() == [1, 2, 3, 1, 2, 3] and nk[:4].tolist() == [1, 2, 1, 2]
    for ll_k, kl_k in gc.LIG_CASES[name].k_pairs:
        ref = gc.lig_reference(name, ll_k, kl_k)
        pg = ref['ll_per_graph']
        assert pg.unique().numel() >= 3                                    # the scan adds unequal terms
        if B > 1024:
            assert int(pg[1024:].sum()) > 0 and int(pg[:1024].sum()) > 0   # a carry, and something after it
    x, counts, _ = gc.rec_case('rec_many')
    assert counts.numel() == 1025 and int(gc.rec_reference('rec_many')['per_graph'][1024:].sum()) > 0


def test_thread_switch_sizes():
    threads = lambda max_y: 256 if max_y <= 256 else (320 if max_y <= 320 else 512)       # launch_knn_bipartite
    got = []
    for m in (256, 257, 320, 321):
        _, nl, _, nk = gc.lig_case(f'thread_switch_{m}')
        assert nl.tolist() == [8, 20] and int(nk.max()) == m and gc.LIG_CASES[f'thread_switch_{m}'].k_pairs == ((0, 5),)
        got.append(threads(int(nk.max())))
    assert got == [256, 320, 320, 512]


def test_limits_sizes():
    lds = lambda max_x, max_y: max_x * (12 + 4 * ((max_y + 31) // 32) + 4) + 16             # launch_knn_bipartite
    _, nl, _, nk = gc.lig_case('limits')
    assert int(nl.max()) == 1024 and int(nk.max()) == 1056 and gc.LIG_CASES['limits'].k_pairs[0][1] > 0
    assert lds(1024, 1056) == 151568 <= 150 * 1024 < lds(1024, 1057)
    ref = gc.lig_reference('limits', 0, 5)
    deg = ref['ll_rowptr'][1:] - ref['ll_rowptr'][:-1]
    assert int(deg.max()) == gc.LL_MAX_NN                                 # the 1024-atom complex meets the ll cap as well
    x, counts, _ = gc.rec_over_limit()
    assert counts.tolist() == [2049]
    _, counts, res = gc.rec_case('rec_sizes')
    assert counts.tolist() == [1, 2, 2048] and bool((res[1:] >= res[:-1]).all()) and bool((res[1:] == res[:-1]).any())
    assert gc.rec_case('rec_sizes_nores')[2] is None
