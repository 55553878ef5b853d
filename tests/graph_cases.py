"""Inputs for the graph builders of csrc/graph_build.hip, shared by test_graph_cases.py (CPU: every case reaches the path it
is named for) and test_graph_build_gpu.py (the kernels against the fp64 oracle).  No synth pockets: plain coordinate arrays.

Two families.
  * exact lattice: every coordinate is a multiple of 0.5 with |x| <= 32 and every cutoff has an exactly representable square
    (2.5 -> 6.25, 6.0 -> 36), so every dx*dx + dy*dy + dz*dz is exact in fp32 with or without FMA contraction (a multiple of 0.25
    below 2^14).  Kernel and fp64 oracle then have to agree bit for bit: this family carries the ties, the pairs that sit on the
    cutoff and the neighbour caps.  Atom order inside a complex is a seeded permutation of the lattice sites, so index order and
    distance order differ.
  * general position: seeded fp32 Gaussian clouds.  The builder asserts that no pair's d2 lies within a relative MARGIN of r2 and
    that every two consecutive candidates of every kNN query differ by more than a relative MARGIN, so an fp32 three-term sum (a
    few ulps of error, MARGIN is about 100) orders and cuts them as fp64 does.
"""
import functools
from typing import NamedTuple, Optional

import numpy as np
import torch

from oracle import graph_ops as og

MARGIN = 1e-5
LL_MAX_NN, KL_MAX_NN = 200, 100                 # launch_lig_graph: caps of the ll and the kl radius graph
K_PAIRS = [(0, 0), (1, 1), (3, 5), (16, 16)]    # (ll_k, kl_k); 0 = radius graph, 16 = KL_KMAX


# ---- lattice helpers ------------------------------------------------------------------------------------------------------
def block_sites(nx, ny, nz):
    """All sites of an nx x ny x nz block of spacing 0.5 with its corner at the origin, raster order, float64."""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing='ij'), -1).reshape(-1, 3)
    return g.astype(np.float64) * 0.5


def pick(rng, sites, n):
    """n distinct sites in a seeded random order."""
    assert n <= len(sites)
    return sites[rng.permutation(len(sites))[:n]]


def origin(rng, extent=6.0):
    """A lattice vector that keeps a block of the given extent inside |x| <= 32."""
    return rng.integers(-64, int((32 - extent) * 2) + 1, 3).astype(np.float64) * 0.5


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))


def _counts(c):
    return torch.tensor(list(c), dtype=torch.long)


def _lattice_lig(rng, block, lig_counts, kp_counts, coincident=False):
    sites = block_sites(*block)
    extent = 0.5 * (max(block) - 1)
    lig, kp = [], []
    for nl, nk in zip(lig_counts, kp_counts):
        o = origin(rng, extent)
        l, k = pick(rng, sites, nl), pick(rng, sites, nk)
        if coincident:
            if nl >= 3:
                l[-1] = l[0]                      # two ligand atoms on one site
            k[0] = l[0]                           # a keypoint on a ligand atom
        lig.append(l + o)
        kp.append(k + o)
    return _t(np.concatenate(lig)), _counts(lig_counts), _t(np.concatenate(kp)), _counts(kp_counts)


# ---- ligand-graph cases: functions returning (lig_x, lig_counts, kp_x, kp_counts) ------------------------------------------------
def caps_ll_kl():
    """Every atom of a complex inside one 6x6x6 block (diameter 4.33 < 6): a centre of an n-atom complex has n - 1 ll candidates
    (215, 201, 200 against the cap of 200) and a keypoint has n kl candidates (102, 101, 100 against the cap of 100)."""
    return _lattice_lig(np.random.default_rng(101), (6, 6, 6), [216, 202, 201, 102, 101, 100, 3], [2] * 7)


def boundary_ties():
    """6x5x4 block, cutoff 2.5: index offsets (5,0,0) and (3,4,0) sit on d2 == 6.25; a lattice ties everywhere."""
    return _lattice_lig(np.random.default_rng(102), (6, 5, 4), [1, 2, 3, 16, 17, 64, 65], [1, 31, 32, 33, 64, 65, 2], coincident=True)


def many_complexes(B):
    return _lattice_lig(np.random.default_rng(103), (6, 5, 4), [1 + b % 3 for b in range(B)], [1 + b % 2 for b in range(B)])


def thread_switch(max_kp):
    return _lattice_lig(np.random.default_rng(104), (8, 8, 8), [8, 20], [3, max_kp], coincident=True)


def limits(max_lig=1024, max_kp=1056):
    return _lattice_lig(np.random.default_rng(105), (11, 11, 11), [5, max_lig], [max_kp, 4])


GENERAL_SEEDS = (8, 2)                          # smallest margins (cutoff, kNN): seed 8: 2.99e-4, 9.97e-5; seed 2: 9.25e-4, 8.63e-5
GENERAL_SIGMA = 3.0
GENERAL_CUTS = (5.0, 6.0)                       # (ll, kl)


def _rel_gap(a, b):
    return (a - b).abs() / torch.maximum(a.abs(), b.abs())


def general_margins(lig_x, lig_counts, kp_x, kp_counts, ll_cut, kl_cut):
    """Smallest relative distance of any pair's d2 to its r2, and smallest relative gap between two consecutive candidates of any
    kNN query (all ranks, ll and kl), in fp64."""
    lp, kp = og.counts_to_ptr(lig_counts), og.counts_to_ptr(kp_counts)
    m_r, m_k = float('inf'), float('inf')
    for b in range(lig_counts.numel()):
        l, k = lig_x[lp[b]:lp[b + 1]].double(), kp_x[kp[b]:kp[b + 1]].double()
        ll = ((l[:, None] - l[None]) ** 2).sum(-1)
        kl = ((k[:, None] - l[None]) ** 2).sum(-1)
        off = ~torch.eye(l.shape[0], dtype=torch.bool)
        for d2, r in ((ll[off], ll_cut), (kl.flatten(), kl_cut)):
            if d2.numel():
                m_r = min(m_r, float((d2 / (r * r) - 1).abs().min()))
        for d2 in (ll.masked_fill(~off, float('inf')).sort(1).values[:, :-1], kl.sort(1).values):
            if d2.shape[1] >= 2:
                m_k = min(m_k, float(_rel_gap(d2[:, 1:], d2[:, :-1]).min()))
    return m_r, m_k


def general(seed):
    g = torch.Generator().manual_seed(seed)
    lig_counts, kp_counts = _counts([37, 4, 25]), _counts([20, 40, 7])
    centres = torch.randn(3, 3, generator=g) * 10.0
    lig_x = torch.cat([centres[b] + GENERAL_SIGMA * torch.randn(int(n), 3, generator=g) for b, n in enumerate(lig_counts)]).float()
    kp_x = torch.cat([centres[b] + GENERAL_SIGMA * torch.randn(int(n), 3, generator=g) for b, n in enumerate(kp_counts)]).float()
    m_r, m_k = general_margins(lig_x, lig_counts, kp_x, kp_counts, GENERAL_CUTS[0], GENERAL_CUTS[1])
    assert m_r > MARGIN and m_k > MARGIN, f'seed {seed}: cutoff margin {m_r:.3g}, kNN margin {m_k:.3g}; pick another seed'
    return lig_x, lig_counts, kp_x, kp_counts


class LigCase(NamedTuple):
    name: str
    build: object          # () -> (lig_x, lig_counts, kp_x, kp_counts)
    ll_cut: float
    kl_cut: float
    k_pairs: tuple         # the (ll_k, kl_k) the case runs with


LIG_CASES = {c.name: c for c in [
    LigCase('caps_ll_kl', caps_ll_kl, 6.0, 6.0, ((0, 0),)),
    LigCase('boundary_ties', boundary_ties, 2.5, 2.5, tuple(K_PAIRS)),
    LigCase('many_complexes_1024', functools.partial(many_complexes, 1024), 2.5, 2.5, ((0, 0), (2, 1))),
    LigCase('many_complexes_1025', functools.partial(many_complexes, 1025), 2.5, 2.5, ((0, 0), (2, 1))),
    LigCase('many_complexes_2049', functools.partial(many_complexes, 2049), 2.5, 2.5, ((0, 0), (2, 1))),
    LigCase('thread_switch_256', functools.partial(thread_switch, 256), 2.5, 2.5, ((0, 5),)),
    LigCase('thread_switch_257', functools.partial(thread_switch, 257), 2.5, 2.5, ((0, 5),)),
    LigCase('thread_switch_320', functools.partial(thread_switch, 320), 2.5, 2.5, ((0, 5),)),
    LigCase('thread_switch_321', functools.partial(thread_switch, 321), 2.5, 2.5, ((0, 5),)),
    LigCase('limits', limits, 2.5, 2.5, ((0, 5),)),
    LigCase('general', functools.partial(general, GENERAL_SEEDS[0]), GENERAL_CUTS[0], GENERAL_CUTS[1], tuple(K_PAIRS)),
    LigCase('general_2', functools.partial(general, GENERAL_SEEDS[1]), GENERAL_CUTS[0], GENERAL_CUTS[1], tuple(K_PAIRS)),
]}
GENERAL_LIG = ['general', 'general_2']
LATTICE_LIG = [n for n in LIG_CASES if n not in GENERAL_LIG]
LIG_RUNS = [(c.name, ll_k, kl_k) for c in LIG_CASES.values() for ll_k, kl_k in c.k_pairs]


@functools.lru_cache(maxsize=None)
def lig_case(name):
    return LIG_CASES[name].build()


def _rowptr(dst, n):
    return og.counts_to_ptr(torch.bincount(dst, minlength=n))


@functools.lru_cache(maxsize=None)
def lig_reference(name, ll_k, kl_k):
    """The oracle's graph of a case on fp64 inputs, in the layout of hip.build_lig_graph: ll dst-major; lk kp-major; kl the same
    pairs sorted by (lig, kp); CSR row pointers; edges per complex.  Computed once per (case, ll_k, kl_k); do not modify."""
    c = LIG_CASES[name]
    lig_x, nl, kp_x, nk = lig_case(name)
    lx, kx = lig_x.double(), kp_x.double()
    n_lig, n_kp = int(nl.sum()), int(nk.sum())
    ll_src, ll_dst = og.knn_graph(lx, ll_k, nl) if ll_k > 0 else og.radius_graph(lx, c.ll_cut, nl, LL_MAX_NN)
    kp_idx, lig_idx = og.knn(lx, kx, kl_k, nl, nk) if kl_k > 0 else og.radius(lx, kx, c.kl_cut, nl, nk, KL_MAX_NN)
    order = torch.argsort(lig_idx * n_kp + kp_idx)
    return dict(ll_src=ll_src, ll_dst=ll_dst, ll_rowptr=_rowptr(ll_dst, n_lig), ll_per_graph=og.edges_per_graph(ll_dst, nl),
                lk_src=lig_idx, lk_dst=kp_idx, lk_rowptr=_rowptr(kp_idx, n_kp),
                kl_src=kp_idx[order], kl_dst=lig_idx[order], kl_rowptr=_rowptr(lig_idx, n_lig))


# ---- receptor-graph cases: functions returning (rec_x, rec_counts, res_idx) ------------------------------------------------------
REC_R = 2.5
REC_BLOCK_SEED = 3


def _runs(n, rng):
    """Sorted residue numbers with runs of 1..4 atoms."""
    out, r = [], 0
    while len(out) < n:
        out += [r] * int(rng.integers(1, 5))
        r += int(rng.integers(1, 3))
    return torch.tensor(out[:n], dtype=torch.int32)


def rec_block():
    """One pocket of 150 atoms in four parts more than 2.5 apart, in one seeded order: 143 sites of a 7x6x6 block (up to 142
    candidates; the seed is chosen so that one centre has exactly 100), four mutually adjacent sites (3 candidates each), a pair
    (1 each) and a lone atom (none)."""
    rng = np.random.default_rng(REC_BLOCK_SEED)
    dense = pick(rng, block_sites(7, 6, 6), 143)
    clique = np.array([[0, 0, 0], [.5, 0, 0], [0, .5, 0], [0, 0, .5]]) + [10.0, 0, 0]
    pair = np.array([[0, 0, 0], [0, 2.0, 0]]) + [16.0, 0, 0]
    lone = np.array([[22.0, 0, 0]])
    x = np.concatenate([dense, clique, pair, lone])
    x = x[rng.permutation(len(x))] + origin(rng, 22.0)
    return _t(x), _counts([150]), _runs(150, rng)


def rec_sizes():
    """Pockets of 1, 2 and 2048 atoms (the largest the builder takes); the 2048 fill most of a 13x13x13 block."""
    rng = np.random.default_rng(202)
    xs = [pick(rng, block_sites(13, 13, 13), n) + origin(rng) for n in (1, 2, 2048)]
    return _t(np.concatenate(xs)), _counts([1, 2, 2048]), _runs(2051, rng)


def rec_many(B=1025):
    rng = np.random.default_rng(203)
    counts = [1 + b % 3 for b in range(B)]
    xs = [pick(rng, block_sites(6, 5, 4), n) + origin(rng) for n in counts]
    return _t(np.concatenate(xs)), _counts(counts), _runs(sum(counts), rng)


def rec_over_limit():
    rng = np.random.default_rng(204)
    return _t(pick(rng, block_sites(13, 13, 13), 2049) + origin(rng)), _counts([2049]), None


class RecCase(NamedTuple):
    name: str
    build: object          # () -> (rec_x, rec_counts, res_idx)
    max_nn: int
    with_res: bool


REC_CASES = {c.name: c for c in [
    RecCase('rec_block_nn1', rec_block, 1, True),
    RecCase('rec_block_nn3', rec_block, 3, False),
    RecCase('rec_block_nn100', rec_block, 100, True),
    RecCase('rec_sizes', rec_sizes, 100, True),
    RecCase('rec_sizes_nores', rec_sizes, 100, False),
    RecCase('rec_many', rec_many, 100, True),
]}


@functools.lru_cache(maxsize=None)
def rec_case(name):
    x, counts, res = REC_CASES[name].build()
    return x, counts, (res if REC_CASES[name].with_res else None)


@functools.lru_cache(maxsize=None)
def rec_reference(name):
    x, counts, res = rec_case(name)
    src, dst = og.radius_graph(x.double(), REC_R, counts, REC_CASES[name].max_nn)
    same: Optional[torch.Tensor] = None if res is None else res[src] == res[dst]
    return dict(src=src, dst=dst, rowptr=_rowptr(dst, int(counts.sum())), per_graph=og.edges_per_graph(dst, counts), same_res=same)


# ---- what a case reaches, from the oracle's side ----------------------------------------------------------------------------
def pair_d2(x, y):
    return ((y.double()[:, None] - x.double()[None]) ** 2).sum(-1)


def direct_radius_graph(x, r, counts, max_nn):
    """The rule itself: for every centre i the neighbours j != i of its graph with d2 < r2, the first max_nn by index."""
    ptr = og.counts_to_ptr(counts)
    src, dst = [], []
    for b in range(counts.numel()):
        lo, hi = int(ptr[b]), int(ptr[b + 1])
        ok = pair_d2(x[lo:hi], x[lo:hi]) < r * r
        ok.fill_diagonal_(False)
        for i in range(hi - lo):
            nb = torch.nonzero(ok[i]).flatten()[:max_nn]
            src.append(nb + lo)
            dst.append(torch.full_like(nb, lo + i))
    return torch.cat(src), torch.cat(dst)
