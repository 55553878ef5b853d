"""Timing of kpd_vina_dock next to kpd_vina_minimize, measured in the same run on the same ligands (profiles/vina_dock.md).
    python profiles/tools/vina_dock_bench.py      HIP events around the raw C calls (buffers preallocated, no host sync inside)
The inputs are the self-avoiding chains of profiles/tools/vina_min_bench.py (one fragment and n - 3 rotors per ligand) in pockets
of 300 atoms: 640 ligands of 25 atoms, 10 per pocket, in 64 pockets, and 64 ligands of 60 atoms in one pocket; the search runs at
its defaults (8 chains, 50 steps, step_iters 20, refinement max_iters 200) inside every ligand's own bounding box widened by 4 A.
The yardstick is kpd_vina_minimize's time per ligand-evaluation: the evaluation code is the same."""
import sys, os, ctypes
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from keypoint_diffusion_amd import hip, molecule

dev = torch.device('cuda:0')
L = hip.lib()
ELEMENTS = ['C', 'N', 'O', 'S', 'P', 'F', 'Cl', 'Br', 'I', 'B']
POOL = [0, 0, 0, 1, 2, 3, 6, 5, 4, 7]
POCKET_ELEMENTS = ['C', 'C', 'C', 'N', 'O', 'S']
M = 300
N_CHAINS, N_STEPS, N_MODES = 8, 50, 8
MCOL = {k: c for c, k in enumerate(hip.VINA_MIN_REPORT)}
CCOL = {k: c for c, k in enumerate(hip.VINA_DOCK_CHAIN_REPORT)}


def chains(B, n, seed):
    """B self-avoiding chains of n atoms, as in vina_min_bench.py: 1.5 A bonds, 111 degree angles, staggered dihedrals with 15
    degrees of noise; a new atom stays 2.6 A from every atom but its two predecessors."""
    rng = np.random.default_rng(seed)
    out = np.zeros((B, n, 3))
    ca, sa = np.cos(np.deg2rad(111.0)), np.sin(np.deg2rad(111.0))
    for b in range(B):
        p = [np.zeros(3), np.array([1.5, 0.0, 0.0]), np.array([1.5 - 1.5 * ca, 1.5 * sa, 0.0])]
        while len(p) < n:
            a, bb, c = p[-3], p[-2], p[-1]
            bc = (c - bb) / np.linalg.norm(c - bb)
            nrm = np.cross(bb - a, bc)
            nrm /= np.linalg.norm(nrm)
            m = np.cross(nrm, bc)
            for _ in range(40):
                phi = np.deg2rad(rng.choice([60.0, 180.0, 300.0]) + 15.0 * rng.standard_normal())
                q = c + 1.5 * (-ca * bc + sa * np.cos(phi) * m + sa * np.sin(phi) * nrm)
                if len(p) < 3 or np.linalg.norm(np.array(p[:-2]) - q, axis=1).min() >= 2.6:
                    break
            else:
                p = p[:max(3, len(p) - 4)]               # a dead end: step back
                continue
            p.append(q)
        out[b] = np.array(p) - np.mean(p, axis=0)
    return torch.tensor(out.reshape(B * n, 3), dtype=torch.float32)


def setup(B, n, group):
    g = torch.Generator().manual_seed(B * 1000 + n)
    N, P = B * n, B // group
    pos = chains(B, n, B * 1000 + n).to(dev)
    cls = torch.tensor(POOL)[torch.randint(0, len(POOL), (N,), generator=g)]
    cls = torch.where(cls == 1, cls, torch.zeros_like(cls))          # C and N only: a halogen in mid-chain would cut it
    feat = torch.nn.functional.one_hot(cls, len(ELEMENTS)).float().to(dev)
    r = (4.5 ** 3 + (11.0 ** 3 - 4.5 ** 3) * torch.rand(P * M, generator=g)) ** (1.0 / 3.0)
    d = torch.randn(P * M, 3, generator=g)
    px = (d / d.norm(dim=1, keepdim=True) * r[:, None]).to(dev)
    pel = [POCKET_ELEMENTS[k] for k in torch.randint(0, len(POCKET_ELEMENTS), (P * M,), generator=g).tolist()]
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
    z, allowed = molecule._class_tables(ELEMENTS, None)
    per = pos.reshape(B, n, 3)
    o = dict(B=B, N=N, n=n, P=P, pos=pos, feat=feat, ptr=(torch.arange(B + 1, dtype=torch.int32) * n).to(dev),
             z=torch.tensor(z, dtype=torch.int32, device=dev), allowed=torch.tensor(allowed, dtype=torch.int32, device=dev), elem=i32(N),
             valence=i32(N), frag=i32(N), bonds=i32(3 * N, 2), order=i32(3 * N), bond_ptr=i32(B + 1), summary=i32(B, 4), status=i32(B),
             lig_radius=torch.tensor(molecule.xs_radius_table(ELEMENTS, {'B': 2.0}), dtype=torch.float32, device=dev), px=px,
             pz=torch.tensor([molecule.ATOMIC_NUMBERS[e] for e in pel], dtype=torch.int32, device=dev),
             prad=torch.tensor(molecule.xs_radius_table(pel), dtype=torch.float32, device=dev), ptype=i32(P * M), pstatus=i32(P),
             pptr=(torch.arange(P + 1, dtype=torch.int32) * M).to(dev), pof=(torch.arange(B, dtype=torch.int32) // group).to(dev),
             pos_out=torch.empty_like(pos), mreport=f64(B, 16), mstatus=i32(B), lo=(per.amin(dim=1) - 4.0).contiguous(),
             hi=(per.amax(dim=1) + 4.0).contiguous(), modes=torch.empty(N_MODES, N, 3, device=dev), n_found=i32(B), dreport=f64(B, N_MODES, 8),
             chain_pos=torch.empty(N_CHAINS, N, 3, device=dev), creport=f64(B, N_CHAINS, len(CCOL)), dstatus=i32(B))
    o['s1'] = torch.empty(int(L.kpd_mol_scratch_bytes(N, B)), dtype=torch.uint8, device=dev)
    hip.check(L.kpd_mol_perceive(o['pos'].data_ptr(), o['feat'].data_ptr(), o['ptr'].data_ptr(), N, B, len(ELEMENTS), o['z'].data_ptr(),
              o['allowed'].data_ptr(), 3 * N, o['elem'].data_ptr(), o['valence'].data_ptr(), o['frag'].data_ptr(), o['bonds'].data_ptr(),
              o['order'].data_ptr(), o['bond_ptr'].data_ptr(), o['summary'].data_ptr(), o['status'].data_ptr(), o['s1'].data_ptr(), None))
    hip.check(L.kpd_vina_pocket_types(o['px'].data_ptr(), o['pz'].data_ptr(), o['pptr'].data_ptr(), P * M, P, o['ptype'].data_ptr(),
              o['pstatus'].data_ptr(), None))
    return o


def ligand_args(o):
    return (o['pos'].data_ptr(), o['ptr'].data_ptr(), o['N'], o['B'], o['n'], o['elem'].data_ptr(), len(ELEMENTS), o['z'].data_ptr(),
            o['lig_radius'].data_ptr(), o['frag'].data_ptr(), o['bonds'].data_ptr(), o['order'].data_ptr(), o['bond_ptr'].data_ptr(),
            3 * o['N'], o['status'].data_ptr(), None, o['px'].data_ptr(), o['prad'].data_ptr(), o['ptype'].data_ptr(), o['pptr'].data_ptr(),
            o['P'] * M, o['P'], M, o['pof'].data_ptr(), 64)


def minimize(o, **params):
    p = hip.vina_min_params(**params)
    hip.check(L.kpd_vina_minimize(*ligand_args(o), ctypes.byref(p), o['pos_out'].data_ptr(), o['mreport'].data_ptr(), o['mstatus'].data_ptr(),
                                  None))


def dock(o, n_steps=N_STEPS, **params):
    p = hip.vina_dock_params(**params)
    hip.check(L.kpd_vina_dock(*ligand_args(o), o['lo'].data_ptr(), o['hi'].data_ptr(), None, 1, N_CHAINS, n_steps, N_MODES, ctypes.byref(p),
                              o['modes'].data_ptr(), o['n_found'].data_ptr(), o['dreport'].data_ptr(), o['chain_pos'].data_ptr(),
                              o['creport'].data_ptr(), o['dstatus'].data_ptr(), None))


def timed(fn, reps, warm):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize(); ts.append(a.elapsed_time(b) * 1e3)
    return np.array(ts)


def show(ts):
    return f'median {np.median(ts) / 1e3:.2f} ms, min {ts.min() / 1e3:.2f}, max {ts.max() / 1e3:.2f} ({len(ts)} runs)'


for B, n, group in ((640, 25, 10), (64, 60, 64)):
    o = setup(B, n, group)
    minimize(o); dock(o); torch.cuda.synchronize()
    ran = (o['mstatus'] & (1 | 2 | 32)) == 0
    m_evals = float(o['mreport'][ran, MCOL['evaluations']].sum())
    cr, st = o['creport'], o['dstatus']
    d_evals = float(cr[:, :, CCOL['evaluations']].sum())
    print(f'B={B} x {n} atoms in {o["P"]} pockets of {M}: dock status bits {[int((st & b).ne(0).sum()) for b in (1, 2, 4, 16, 32, 128, 256, 512)]} '
          f'(1, 2, 4, 16, 32, 128, 256, 512); chains that found a pose {int(cr[:, :, CCOL["found"]].sum())} of {B * N_CHAINS}, mean modes '
          f'{float(o["n_found"].float().mean()):.2f}, accepted steps per chain {float(cr[:, :, CCOL["accepted"]].mean()):.1f}, box rejections '
          f'{float(cr[:, :, CCOL["box_rejected"]].mean()):.1f}, evaluations per chain {d_evals / (B * N_CHAINS):.0f}; mean score: input '
          f'{float(o["mreport"][ran, MCOL["score_before"]].mean()):.3f}, minimised {float(o["mreport"][ran, MCOL["score_after"]].mean()):.3f}, '
          f'docked mode 0 {float(o["dreport"][:, 0, 0].mean()):.3f}')
    tm = timed(lambda: minimize(o), 5, 1)
    td = timed(lambda: dock(o), 3, 1)
    per_min, per_dock = np.median(tm) / max(m_evals, 1.0), np.median(td) / max(d_evals, 1.0)
    print('  kpd_vina_minimize, defaults (max_iters 200)', show(tm), f'-> {m_evals:.0f} evaluations, {per_min * 1e3:.1f} ns per ligand-evaluation')
    print(f'  kpd_vina_dock, defaults ({N_CHAINS} chains x {N_STEPS} steps)', show(td),
          f'-> {d_evals:.0f} evaluations, {per_dock * 1e3:.1f} ns per ligand-evaluation, {np.median(td) / B / 1e3:.3f} ms per ligand')
    print(f'  ratio of the two times per ligand-evaluation (dock / minimise): {per_dock / per_min:.3f}; workgroups {B * N_CHAINS} against {B}')
