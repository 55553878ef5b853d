"""Batched heterogeneous complex graph: the carrier the denoiser boundary works on.

The reference passes a batched DGL heterograph (node types rec / kp / lig, edge types
rr, rk, kk, kl, ll, lk; data_processing/pdbbind_processing.py:236-274) through
`KeypointDiffusion` -> `rec_encoder(g, batch_idxs)` -> `dynamics(g, t, batch_idxs)`.  DGL is
not available on ROCm here, so this container re-expresses the slice of the DGL API those
callers touch (utils.py:81-170, models/ligand_diffuser.py:185-203, 254-267, 342-469) on
plain torch tensors.  It is host plumbing only: the per-step edge lists are never stored
here, the HIP path builds them in preallocated CSR buffers every step.
"""
from contextlib import contextmanager
from typing import Dict, List, Optional, Tuple

import torch

NTYPES = ['rec', 'kp', 'lig']
CANONICAL_ETYPES = [
    ('rec', 'rr', 'rec'), ('rec', 'rk', 'kp'), ('kp', 'kk', 'kp'),
    ('kp', 'kl', 'lig'), ('lig', 'll', 'lig'), ('lig', 'lk', 'kp'),
]
_ET = {c[1]: c for c in CANONICAL_ETYPES}


def _et_name(etype) -> str:
    return etype[1] if isinstance(etype, tuple) else etype


class _DataView:
    def __init__(self, store: dict):
        self.data = store


class _NodeSpace:
    def __init__(self, g):
        self._g = g

    def __getitem__(self, ntype):
        return _DataView(self._g._ndata[ntype])

    def __call__(self, ntype):
        return torch.arange(self._g._num_nodes[ntype], device=self._g.device)


class _EdgeSpace:
    def __init__(self, g):
        self._g = g

    def __getitem__(self, etype):
        return _DataView(self._g._edata[_et_name(etype)])

    def __call__(self, form='uv', etype=None):
        src, dst = self._g._edges[_et_name(etype)]
        if form == 'uv':
            return src, dst
        if form == 'eid':
            return torch.arange(src.shape[0], device=src.device)
        if form == 'all':
            return src, dst, torch.arange(src.shape[0], device=src.device)
        raise ValueError(f'unsupported form {form!r}')


class HeteroBatch:
    """A batch of B complexes stored flat, graph-major (all nodes of complex 0, then 1 ...)."""

    ntypes = NTYPES
    canonical_etypes = CANONICAL_ETYPES
    etypes = [c[1] for c in CANONICAL_ETYPES]

    def __init__(self, num_nodes: Dict[str, int], device='cpu'):
        self.device = torch.device(device)
        self._num_nodes = {nt: int(num_nodes.get(nt, 0)) for nt in NTYPES}
        self._ndata: Dict[str, Dict[str, torch.Tensor]] = {nt: {} for nt in NTYPES}
        z = lambda: torch.zeros(0, dtype=torch.long, device=self.device)
        self._edges: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {et: (z(), z()) for et in self.etypes}
        self._edata: Dict[str, Dict[str, torch.Tensor]] = {et: {} for et in self.etypes}
        self._bnn = {nt: torch.tensor([self._num_nodes[nt]], dtype=torch.long, device=self.device) for nt in NTYPES}
        self._bne = {et: torch.zeros(1, dtype=torch.long, device=self.device) for et in self.etypes}
        self.nodes = _NodeSpace(self)
        self.edges = _EdgeSpace(self)

    # ---- sizes -------------------------------------------------------------------------
    @property
    def batch_size(self) -> int:
        return int(self._bnn['lig'].shape[0])

    def num_nodes(self, ntype=None) -> int:
        if ntype is None:
            return sum(self._num_nodes.values())
        return self._num_nodes[ntype]

    def num_edges(self, etype=None) -> int:
        if etype is None:
            return sum(int(s.shape[0]) for s, _ in self._edges.values())
        return int(self._edges[_et_name(etype)][0].shape[0])

    def batch_num_nodes(self, ntype) -> torch.Tensor:
        return self._bnn[ntype]

    def batch_num_edges(self, etype) -> torch.Tensor:
        return self._bne[_et_name(etype)]

    def set_batch_num_nodes(self, val: Dict[str, torch.Tensor]):
        for nt, t in val.items():
            self._bnn[nt] = t.to(self.device).long()

    def set_batch_num_edges(self, val: Dict):
        for et, t in val.items():
            self._bne[_et_name(et)] = t.to(self.device).long()

    # ---- mutation ----------------------------------------------------------------------
    def add_edges(self, src, dst, data: Optional[dict] = None, etype=None):
        et = _et_name(etype)
        s0, d0 = self._edges[et]
        src = torch.as_tensor(src, dtype=torch.long, device=self.device)
        dst = torch.as_tensor(dst, dtype=torch.long, device=self.device)
        self._edges[et] = (torch.cat([s0, src]), torch.cat([d0, dst]))
        for k, t in self._edata[et].items():
            pad = torch.zeros((src.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=self.device)
            self._edata[et][k] = torch.cat([t, pad])
        if data:
            for k, t in data.items():
                self._edata[et][k] = t
        if self.batch_size == 1:
            self._bne[et] = torch.tensor([self._edges[et][0].shape[0]], device=self.device)

    def remove_edges(self, eids, etype=None):
        et = _et_name(etype)
        s, d = self._edges[et]
        keep = torch.ones(s.shape[0], dtype=torch.bool, device=self.device)
        keep[torch.as_tensor(eids, dtype=torch.long, device=self.device)] = False
        self._edges[et] = (s[keep], d[keep])
        for k in list(self._edata[et]):
            self._edata[et][k] = self._edata[et][k][keep]
        if self.batch_size == 1:
            self._bne[et] = torch.tensor([self._edges[et][0].shape[0]], device=self.device)

    def add_nodes(self, num: int, data: Optional[dict] = None, ntype=None):
        old = self._num_nodes[ntype]
        self._num_nodes[ntype] = old + int(num)
        for k, t in list(self._ndata[ntype].items()):
            if data is not None and k in data:
                self._ndata[ntype][k] = torch.cat([t, data[k].to(self.device)])
            else:
                pad = torch.zeros((int(num),) + tuple(t.shape[1:]), dtype=t.dtype, device=self.device)
                self._ndata[ntype][k] = torch.cat([t, pad])
        if data:
            for k, t in data.items():
                if k not in self._ndata[ntype]:
                    assert old == 0, 'new feature on a non-empty node set'
                    self._ndata[ntype][k] = t.to(self.device)
        if self.batch_size == 1:
            self._bnn[ntype] = torch.tensor([self._num_nodes[ntype]], device=self.device)

    def remove_nodes(self, nids, ntype=None):
        nids = torch.as_tensor(nids, dtype=torch.long, device=self.device)
        n = self._num_nodes[ntype]
        keep = torch.ones(n, dtype=torch.bool, device=self.device)
        keep[nids] = False
        remap = torch.cumsum(keep.long(), 0) - 1
        for k in list(self._ndata[ntype]):
            self._ndata[ntype][k] = self._ndata[ntype][k][keep]
        self._num_nodes[ntype] = int(keep.sum())
        for (s_nt, et, d_nt) in CANONICAL_ETYPES:
            if ntype not in (s_nt, d_nt):
                continue
            s, d = self._edges[et]
            ek = torch.ones(s.shape[0], dtype=torch.bool, device=self.device)
            if s_nt == ntype:
                ek &= keep[s]
            if d_nt == ntype:
                ek &= keep[d]
            s, d = s[ek], d[ek]
            if s_nt == ntype:
                s = remap[s]
            if d_nt == ntype:
                d = remap[d]
            self._edges[et] = (s, d)
            for k in list(self._edata[et]):
                self._edata[et][k] = self._edata[et][k][ek]
        if self.batch_size == 1:
            self._bnn[ntype] = torch.tensor([self._num_nodes[ntype]], device=self.device)

    # ---- misc --------------------------------------------------------------------------
    @contextmanager
    def local_scope(self):
        saved_n = {nt: dict(d) for nt, d in self._ndata.items()}
        saved_e = {et: dict(d) for et, d in self._edata.items()}
        try:
            yield
        finally:
            self._ndata.clear()
            self._ndata.update(saved_n)
            self._edata.clear()
            self._edata.update(saved_e)

    def to(self, device) -> 'HeteroBatch':
        device = torch.device(device)
        g = HeteroBatch(self._num_nodes, device=device)
        g._ndata = {nt: {k: t.to(device) for k, t in d.items()} for nt, d in self._ndata.items()}
        g._edges = {et: (s.to(device), d.to(device)) for et, (s, d) in self._edges.items()}
        g._edata = {et: {k: t.to(device) for k, t in d.items()} for et, d in self._edata.items()}
        g._bnn = {nt: t.to(device) for nt, t in self._bnn.items()}
        g._bne = {et: t.to(device) for et, t in self._bne.items()}
        return g

    def prepared(self):
        """Device-side int32 view of the static batch structure (per-complex offsets, dst-sorted kk
        CSR) consumed by the HIP engines; cached until node counts or kk edges change."""
        from . import hip
        kk_s, kk_d = self._edges['kk']
        # The key identifies the tensors by storage and version counter, never by value: reading the per-complex
        # counts back (.tolist()) would synchronise with the GPU on every reverse step and drain the launch queue.
        # The cache entry keeps the keyed tensors alive, so a data_ptr cannot be recycled by another tensor.
        bl, bk = self._bnn['lig'], self._bnn['kp']
        key = (bl.data_ptr(), bl._version, int(bl.shape[0]), bk.data_ptr(), bk._version, kk_s.data_ptr(), kk_s._version,
               int(kk_s.shape[0]), str(self.device))
        cache = getattr(self, '_prepared', None)
        if cache is None or cache[0] != key:
            self._prepared = (key, hip.PreparedBatch(bl, bk, kk_s, kk_d, self.device), (bl, bk, kk_s, kk_d))
        return self._prepared[1]

    def node_ptr(self, ntype) -> torch.Tensor:
        """int64 [B+1] offsets of each complex's nodes in the flat node array."""
        ptr = torch.zeros(self.batch_size + 1, dtype=torch.long, device=self.device)
        ptr[1:] = torch.cumsum(self._bnn[ntype], 0)
        return ptr

    def __repr__(self):
        return (f'HeteroBatch(B={self.batch_size}, nodes={self._num_nodes}, '
                f'edges={ {et: int(s.shape[0]) for et, (s, _) in self._edges.items()} })')


def heterograph(data_dict: Dict, num_nodes_dict: Dict[str, int], device='cpu') -> HeteroBatch:
    """dgl.heterograph(data_dict, num_nodes_dict=..., device=...) for the six edge types."""
    g = HeteroBatch(num_nodes_dict, device=device)
    for et, (src, dst) in data_dict.items():
        src = torch.as_tensor(src, dtype=torch.long, device=g.device)
        dst = torch.as_tensor(dst, dtype=torch.long, device=g.device)
        name = _et_name(et)
        g._edges[name] = (src, dst)
        g._bne[name] = torch.tensor([src.shape[0]], dtype=torch.long, device=g.device)
    return g


def batch(graphs: List[HeteroBatch]) -> HeteroBatch:
    """dgl.batch: concatenate complexes, offsetting edge endpoints."""
    dev = graphs[0].device
    tot = {nt: sum(g._num_nodes[nt] for g in graphs) for nt in NTYPES}
    out = HeteroBatch(tot, device=dev)
    for nt in NTYPES:
        keys = set().union(*[g._ndata[nt].keys() for g in graphs])
        for k in keys:
            parts = [g._ndata[nt][k] for g in graphs if k in g._ndata[nt]]
            out._ndata[nt][k] = torch.cat(parts) if parts else None
        out._bnn[nt] = torch.cat([g._bnn[nt] for g in graphs])
    off = {nt: 0 for nt in NTYPES}
    srcs = {et: [] for et in out.etypes}
    dsts = {et: [] for et in out.etypes}
    for g in graphs:
        for (s_nt, et, d_nt) in CANONICAL_ETYPES:
            s, d = g._edges[et]
            srcs[et].append(s + off[s_nt])
            dsts[et].append(d + off[d_nt])
        for nt in NTYPES:
            off[nt] += g._num_nodes[nt]
    for et in out.etypes:
        out._edges[et] = (torch.cat(srcs[et]), torch.cat(dsts[et]))
        out._bne[et] = torch.cat([g._bne[et] for g in graphs])
        keys = set().union(*[g._edata[et].keys() for g in graphs])
        for k in keys:
            out._edata[et][k] = torch.cat([g._edata[et][k] for g in graphs if k in g._edata[et]])
    return out


def unbatch(g: HeteroBatch) -> List[HeteroBatch]:
    """dgl.unbatch: split back into single complexes (edges must be graph-major)."""
    B = g.batch_size
    nptr = {nt: g.node_ptr(nt).tolist() for nt in NTYPES}
    eptr = {}
    for et in g.etypes:
        p = [0]
        for c in g._bne[et].tolist():
            p.append(p[-1] + c)
        eptr[et] = p
    out = []
    for b in range(B):
        nn = {nt: nptr[nt][b + 1] - nptr[nt][b] for nt in NTYPES}
        h = HeteroBatch(nn, device=g.device)
        for nt in NTYPES:
            for k, t in g._ndata[nt].items():
                h._ndata[nt][k] = t[nptr[nt][b]:nptr[nt][b + 1]]
        for (s_nt, et, d_nt) in CANONICAL_ETYPES:
            s, d = g._edges[et]
            lo, hi = eptr[et][b], eptr[et][b + 1]
            h._edges[et] = (s[lo:hi] - nptr[s_nt][b], d[lo:hi] - nptr[d_nt][b])
            h._bne[et] = torch.tensor([hi - lo], dtype=torch.long, device=g.device)
            for k, t in g._edata[et].items():
                h._edata[et][k] = t[lo:hi]
        out.append(h)
    return out


def segment_sum_ordered(x: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
    """[B, D] sums of the rows of x [N, D] per segment (`counts` [B] int64), added in a fixed order: every segment is padded with
    zeros to a power of two and its rows are added pairwise, neighbours first.  index_add_ accumulates floats with atomics, so its
    bits change from call to call; here they do not, and (x + 0 is exact, a row's place in the tree is its index in the segment)
    they do not depend on the other segments either.  log2(longest segment) small launches: for set-up code, not for a step."""
    B, (N, D) = counts.shape[0], x.shape
    longest = int(counts.max()) if B else 0
    P = 1 << max(longest - 1, 0).bit_length()
    seg = torch.arange(B, device=x.device).repeat_interleave(counts)
    pos = torch.arange(N, device=x.device) - (torch.cumsum(counts, 0) - counts)[seg]
    pad = x.new_zeros(B, P, D)
    pad[seg, pos] = x
    while P > 1:
        pad = pad[:, 0::2] + pad[:, 1::2]
        P >>= 1
    return pad[:, 0]


def readout_nodes(g: HeteroBatch, feat: str, op: str = 'mean', ntype: str = None, ordered: bool = False) -> torch.Tensor:
    """dgl.readout_nodes: per-complex reduction of a node feature ([B, ...]).  `ordered`: sum in a fixed order
    (`segment_sum_ordered`), for callers that promise the same bits for the same inputs."""
    x = g._ndata[ntype][feat]
    counts = g._bnn[ntype]
    if ordered:
        flat = x.flatten(1) if x.dim() > 1 else x[:, None]
        out = segment_sum_ordered(flat, counts).reshape((g.batch_size,) + tuple(x.shape[1:]))
        if op == 'sum':
            return out
        if op == 'mean':
            return out / counts.clamp(min=1).to(x.dtype).view((-1,) + (1,) * (x.dim() - 1))
        raise ValueError(f'unsupported readout op {op!r}')
    bidx = torch.arange(g.batch_size, device=g.device).repeat_interleave(counts)
    out = torch.zeros((g.batch_size,) + tuple(x.shape[1:]), dtype=x.dtype, device=g.device)
    out.index_add_(0, bidx, x)
    if op == 'sum':
        return out
    if op == 'mean':
        shape = (-1,) + (1,) * (x.dim() - 1)
        return out / counts.clamp(min=1).to(x.dtype).view(shape)
    raise ValueError(f'unsupported readout op {op!r}')


def get_batch_info(g: HeteroBatch):
    """utils.py:81-90."""
    return ({nt: g.batch_num_nodes(nt) for nt in g.ntypes},
            {et: g.batch_num_edges(et) for et in g.canonical_etypes})


def get_batch_idxs(g: HeteroBatch) -> Dict[str, torch.Tensor]:
    """utils.py:159-169: complex index of every node, per node type."""
    ar = torch.arange(g.batch_size, device=g.device)
    return {nt: ar.repeat_interleave(g.batch_num_nodes(nt)) for nt in g.ntypes}


def get_edges_per_batch(edge_node_idxs: torch.Tensor, batch_size: int, node_batch_idxs: torch.Tensor):
    """utils.py:92-98."""
    out = torch.zeros(batch_size, dtype=torch.long, device=edge_node_idxs.device)
    if edge_node_idxs.numel():
        out.index_add_(0, node_batch_idxs[edge_node_idxs], torch.ones_like(edge_node_idxs))
    return out


def copy_graph(g: HeteroBatch, n_copies: int, lig_atoms_per_copy=None, batched_graph=False) -> List[HeteroBatch]:
    """utils.py:103-157: replicate one encoded pocket, optionally resizing the ligand."""
    copies = []
    for i in range(n_copies):
        nn = dict(g._num_nodes)
        if lig_atoms_per_copy is not None:
            nn['lig'] = int(lig_atoms_per_copy[i])
        c = HeteroBatch(nn, device=g.device)
        for et in g.etypes:
            s, d = g._edges[et]
            c._edges[et] = (s.clone(), d.clone())
            c._bne[et] = g._bne[et].clone() if batched_graph else torch.tensor([s.shape[0]], device=g.device)
            for k, t in g._edata[et].items():
                c._edata[et][k] = t.detach().clone()
        if batched_graph:
            c._bnn = {nt: t.clone() for nt, t in g._bnn.items()}
        for nt in NTYPES:
            for k, t in g._ndata[nt].items():
                if nt == 'lig' and lig_atoms_per_copy is not None:
                    c._ndata[nt][k] = torch.zeros((nn['lig'],) + tuple(t.shape[1:]), device=g.device)
                else:
                    c._ndata[nt][k] = t.detach().clone()
        copies.append(c)
    return copies
