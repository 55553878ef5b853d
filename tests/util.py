"""Shared helpers for the test-suite: batch construction and product <-> oracle conversion."""
import contextlib

import torch

from keypoint_diffusion_amd import graph as G
from keypoint_diffusion_amd import synth
from oracle.batch import OBatch

CUTOFFS_ALL_ATOM = {'kk': 8, 'kl': 6, 'll': 6, 'rk': 100, 'rr': 3.5}

EGNN_C2 = dict(n_layers=6, hidden_nf=256, use_tanh=True, message_norm=0, update_kp_feat=True, norm=True,
               ll_k=0, kl_k=5, no_cg=False)
EGNN_DEV = dict(n_layers=6, hidden_nf=256, use_tanh=True, message_norm=0, update_kp_feat=False, norm=True,
                ll_k=0, kl_k=5)


def to_obatch(g: G.HeteroBatch) -> OBatch:
    """Product graph container -> oracle batch (CPU copies)."""
    cpu = lambda t: t.detach().cpu()
    ob = OBatch(n={nt: cpu(g.batch_num_nodes(nt)) for nt in g.ntypes}, x={}, h={}, v={}, edges={})
    for nt in g.ntypes:
        d = g.nodes[nt].data
        if 'x_0' in d:
            ob.x[nt] = cpu(d['x_0']).float()
        if 'h_0' in d:
            ob.h[nt] = cpu(d['h_0']).float()
        if 'v_0' in d:
            ob.v[nt] = cpu(d['v_0']).float()
    for et in g.etypes:
        s, d = g.edges(etype=et)
        ob.edges[et] = (cpu(s), cpu(d))
    return ob


def to_obatch64(g: G.HeteroBatch) -> OBatch:
    """`to_obatch` with positions, scalars and vectors in float64: the input of a float64 oracle run."""
    ob = to_obatch(g)
    for d in (ob.x, ob.h, ob.v):
        for nt in d:
            d[nt] = d[nt].double()
    return ob


@contextlib.contextmanager
def float64_oracle():
    """The oracle makes its own constants (zero vectors, the rbf centres) in torch's default dtype: float64 while it runs in float64,
    so that nothing in a high-precision reference is rounded to fp32 on the way."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def tile_spans(dst: torch.Tensor, n_dst: int, tile: int = 64) -> torch.Tensor:
    """[n_dst] how many `tile`-edge tiles the run of in-edges of each destination touches when the edges of one type are stored
    destination-major (0 for a destination without in-edge): a run [lo, hi) touches tiles lo / tile .. (hi - 1) / tile."""
    deg = torch.bincount(dst, minlength=n_dst)
    hi = torch.cumsum(deg, 0)
    lo = hi - deg
    return torch.where(deg > 0, (hi - 1) // tile - lo // tile + 1, torch.zeros_like(deg))


def fixed_encode(g: G.HeteroBatch, n_vec=None) -> G.HeteroBatch:
    """What FixedReceptorEncoder does (kp := rec, kk := rr), on the container, without the module."""
    from keypoint_diffusion_amd.receptor_encoder_fixed import FixedReceptorEncoder
    return FixedReceptorEncoder(n_vec)(g, G.get_batch_idxs(g))


def make_batch(n_rec, n_lig, cutoffs=CUTOFFS_ALL_ATOM, seed=1234, n_rec_feat=10, n_keypoints=20,
               density=synth.ATOM_DENSITY) -> G.HeteroBatch:
    gs = synth.synth_complexes(n_rec, n_lig, n_keypoints, cutoffs, seed=seed, n_rec_feat=n_rec_feat, density=density)
    return G.batch(gs)


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    """max |a-b| / max |b| -- the 'within 1e-4 rel fp32' measure of BASELINE.json."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def per_complex_rel_err(a: torch.Tensor, b: torch.Tensor, counts) -> float:
    """max over complexes of (max |a - b| / max |b|) taken INSIDE each complex: a small complex (a single-atom ligand, a
    quiet pocket) is judged on its own scale instead of hiding under the largest entry of the batch."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    worst, off = 0.0, 0
    for n in [int(c) for c in counts]:
        if n:
            ref = b[off:off + n].abs().max().clamp(min=1e-30)
            worst = max(worst, float((a[off:off + n] - b[off:off + n]).abs().max() / ref))
        off += n
    assert off == a.shape[0], (off, a.shape)
    return worst


def elementwise_excess(a: torch.Tensor, b: torch.Tensor, rtol: float = 1e-4, atol_rel: float = 1e-6) -> float:
    """allclose(a, b, rtol, atol = atol_rel * max |b|) as a number: max of |a - b| / (atol + rtol |b|); <= 1 passes."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    atol = atol_rel * float(b.abs().max().clamp(min=1e-30))
    return float(((a - b).abs() / (atol + rtol * b.abs())).max())


def assert_parity(got: torch.Tensor, ref: torch.Tensor, counts=None, tol: float = 1e-4, what: str = '', atol_rel: float = 1e-6,
                  max_excess: float = 1.0):
    """The three parity measures of the denoiser tests: whole-tensor relative error (BASELINE.json's '1e-4 rel fp32'),
    the same per complex, and an elementwise allclose(rtol = tol, atol = atol_rel * max |ref|).  `max_excess` above 1 loosens the
    elementwise measure alone, for a case whose caller has measured that fp32 itself needs it."""
    e = rel_err(got, ref)
    assert e < tol, f'{what}: rel err {e:.3e} >= {tol}'
    if counts is not None:
        pc = per_complex_rel_err(got, ref, counts)
        assert pc < tol, f'{what}: per-complex rel err {pc:.3e} >= {tol}'
    ex = elementwise_excess(got, ref, rtol=tol, atol_rel=atol_rel)
    assert ex <= max_excess, f'{what}: allclose(rtol={tol}, atol={atol_rel} max|ref|) violated by a factor {ex:.2f}'


def assert_param_grads(model, ref_grads: dict, tol: float, min_checked: int = 10, tol_of: dict = None):
    """Every parameter gradient of `model` against `ref_grads` (name -> float64 gradient or None, from autograd through an oracle):
    max |g - ref| <= tol * max |ref| per tensor (`tol_of`: name -> another bound for single tensors).  A parameter the oracle never
    applies (gradient None or all zero) must have none here either; a lone bias is judged on the scale of its weight's gradient (a
    cancelling sum over all edges)."""
    worst, checked = [], 0
    for n, p in model.named_parameters():
        if p.numel() == 0:                                            # GVPDropout's dummy_param: nothing to compare
            continue
        r = ref_grads[n]
        if r is None or float(r.abs().max()) < 1e-10:               # fc_dst: built, never applied (:190-191); a saturated tanh head
            assert p.grad is None or float(p.grad.abs().max()) <= 1e-9, n
            continue
        assert p.grad is not None, n
        scale = r.abs().max().item()
        if r.numel() == 1 and n.endswith('.bias'):                    # lone attention bias: a cancelling sum over all edges
            scale = max(scale, ref_grads[n[:-4] + 'weight'].abs().max().item())
        worst.append(((p.grad.cpu().double() - r).abs().max().item() / scale / (tol_of or {}).get(n, tol), n))
        checked += 1
    worst.sort(reverse=True)
    assert checked > min_checked and worst[0][0] < 1.0, [(e * (tol_of or {}).get(n, tol), n) for e, n in worst[:8]]


def _pair_dist(x, y, n_x, n_y):
    """float64 distance matrices [n_y[b], n_x[b]] of every complex."""
    x, y, ox, oy = x.detach().double(), y.detach().double(), 0, 0
    for nx, ny in zip([int(c) for c in n_x], [int(c) for c in n_y]):
        yield torch.cdist(y[oy:oy + ny], x[ox:ox + nx])
        ox, oy = ox + nx, oy + ny


def knn_rel_gap(x, y, k, n_x, n_y) -> float:
    """How far a kNN edge list (k nearest x of every y, nearest first) is from changing: the smallest (d_j+1 - d_j) / d_j+1 over
    consecutive entries of each query's k + 1 smallest distances -- membership (k-th against (k+1)-th) and order alike."""
    gap = float('inf')
    for d in _pair_dist(x, y, n_x, n_y):
        d = torch.sort(d, dim=1).values[:, :k + 1]
        if d.shape[1] > 1:
            gap = min(gap, float(((d[:, 1:] - d[:, :-1]) / d[:, 1:].clamp(min=1e-30)).min()))
    return gap


def radius_rel_gap(x, y, r, n_x, n_y) -> float:
    """How far a radius edge list (x within r of y) is from changing: the smallest |d - r| / r over all pairs of a complex."""
    return min(float(((d - r).abs() / r).min()) for d in _pair_dist(x, y, n_x, n_y))


def run_threaded_world(world: int, fn, timeout: float = 600.0):
    """`fn(rank)` on `world` ranks that are THREADS of this process, joined by torch's in-process 'threaded' process group
    (torch.testing._internal.distributed.multi_threaded_pg: every collective of torch.distributed works, each thread sees its
    own rank / world size).  This is how more ranks than the GPU box admits GPU-holding processes (6, the test runner
    included) are rehearsed on one card.  Returns [fn(0), ..., fn(world - 1)]; re-raises the first rank failure."""
    import threading
    import torch.distributed as dist
    from torch.testing._internal.distributed import multi_threaded_pg as mt
    mt._install_threaded_pg()
    torch._C._distributed_c10d._set_thread_isolation_mode(True)
    store = dist.HashStore()
    results, errors = [None] * world, []

    def worker(rank):
        try:
            dist.init_process_group(backend='threaded', rank=rank, world_size=world, store=store)
            try:
                results[rank] = fn(rank)
                dist.barrier()
            finally:
                dist.destroy_process_group()
        except BaseException as ex:                                   # noqa: B036 -- wake the other ranks, report below
            errors.append((rank, ex))
            mt.ProcessLocalGroup.exception_handle(ex)

    threads = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(world)]
    try:
        for th in threads:
            th.start()
        for th in threads:
            th.join(timeout)
            assert not th.is_alive(), 'a thread rank did not finish'
    finally:
        torch._C._distributed_c10d._set_thread_isolation_mode(False)
        mt.ProcessLocalGroup.reset()
        mt._uninstall_threaded_pg()
    if errors:
        raise errors[0][1]
    return results


GUARD = 64


def guarded(n, dtype, dev, value):
    """A buffer of n elements between two bands of GUARD elements, all set to `value`: (the whole buffer, the address of element 0)."""
    buf = torch.full((n + 2 * GUARD,), value, dtype=dtype, device=dev)
    return buf, buf.data_ptr() + GUARD * buf.element_size()


def intact(buf, n, value):
    return bool((buf[:GUARD] == value).all()) and bool((buf[GUARD + n:] == value).all())
