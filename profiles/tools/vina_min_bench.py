"""Timing of kpd_vina_minimize next to kpd_vina_score, measured in the same run (profiles/vina_min.md).
    python profiles/tools/vina_min_bench.py      HIP events around the raw C calls (buffers preallocated, no host sync inside)
The inputs are those of profiles/tools/vina_bench.py: seeded normal clouds of 1.6 A x (n / 20)^(1/3), one-hot features over ten
element classes; 6 400 ligands of 25 atoms, 100 per pocket, in 64 pockets of 300 atoms, and 64 ligands of 60 atoms in one pocket
of 300.  The clouds fall into many fragments (a ligand of more than 8 is left out), so both shapes are run a second time with
self-avoiding chains in place of the clouds: one fragment and n - 3 rotors per ligand.  The yardstick is k_vina_score's time per
ligand: it has the same pair loop, and one evaluation here adds the intramolecular pass, the projection on the pose coordinates
and the move."""
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
COL = {k: c for c, k in enumerate(hip.VINA_MIN_REPORT)}

def chains(B, n, seed):
    """B self-avoiding chains of n atoms: 1.5 A bonds, 111 degree angles, staggered dihedrals with 15 degrees of noise; a new atom
    stays 2.6 A from every atom but its two predecessors, so the bond rule finds the chain and nothing else.  One fragment and
    n - 3 rotors per ligand, centred where the clouds sit (the longer chains reach into the pocket's shell and past it)."""
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


def setup(B, n, group, chain=False):
    g = torch.Generator().manual_seed(B * 1000 + n)
    N, P = B * n, B // group
    pos = (torch.randn(N, 3, generator=g) * 1.6 * (n / 20.0) ** (1.0 / 3.0)).to(dev)
    if chain:
        pos = chains(B, n, B * 1000 + n).to(dev)
    cls = torch.tensor(POOL)[torch.randint(0, len(POOL), (N,), generator=g)]
    if chain:
        cls = torch.where(cls == 1, cls, torch.zeros_like(cls))      # C and N only: a halogen in mid-chain would cut it
    feat = torch.nn.functional.one_hot(cls, len(ELEMENTS)).float().to(dev)
    r = (4.5 ** 3 + (11.0 ** 3 - 4.5 ** 3) * torch.rand(P * M, generator=g)) ** (1.0 / 3.0)
    d = torch.randn(P * M, 3, generator=g)
    px = (d / d.norm(dim=1, keepdim=True) * r[:, None]).to(dev)
    pel = [POCKET_ELEMENTS[k] for k in torch.randint(0, len(POCKET_ELEMENTS), (P * M,), generator=g).tolist()]
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
    z, allowed = molecule._class_tables(ELEMENTS, None)
    o = dict(B=B, N=N, n=n, P=P, pos=pos, feat=feat, ptr=(torch.arange(B + 1, dtype=torch.int32) * n).to(dev),
             z=torch.tensor(z, dtype=torch.int32, device=dev), allowed=torch.tensor(allowed, dtype=torch.int32, device=dev), elem=i32(N),
             valence=i32(N), frag=i32(N), bonds=i32(3 * N, 2), order=i32(3 * N), bond_ptr=i32(B + 1), summary=i32(B, 4), status=i32(B),
             lig_radius=torch.tensor(molecule.xs_radius_table(ELEMENTS, {'B': 2.0}), dtype=torch.float32, device=dev), px=px,
             pz=torch.tensor([molecule.ATOMIC_NUMBERS[e] for e in pel], dtype=torch.int32, device=dev),
             prad=torch.tensor(molecule.xs_radius_table(pel), dtype=torch.float32, device=dev), ptype=i32(P * M), pstatus=i32(P),
             pptr=(torch.arange(P + 1, dtype=torch.int32) * M).to(dev), pof=(torch.arange(B, dtype=torch.int32) // group).to(dev),
             report=f64(B, 8), vstatus=i32(B), pos_out=torch.empty_like(pos), mreport=f64(B, 16), mstatus=i32(B))
    o['s1'] = torch.empty(int(L.kpd_mol_scratch_bytes(N, B)), dtype=torch.uint8, device=dev)
    return o

def perceive(o):
    hip.check(L.kpd_mol_perceive(o['pos'].data_ptr(), o['feat'].data_ptr(), o['ptr'].data_ptr(), o['N'], o['B'], len(ELEMENTS), o['z'].data_ptr(),
              o['allowed'].data_ptr(), 3 * o['N'], o['elem'].data_ptr(), o['valence'].data_ptr(), o['frag'].data_ptr(), o['bonds'].data_ptr(),
              o['order'].data_ptr(), o['bond_ptr'].data_ptr(), o['summary'].data_ptr(), o['status'].data_ptr(), o['s1'].data_ptr(), None))

def pocket_types(o):
    hip.check(L.kpd_vina_pocket_types(o['px'].data_ptr(), o['pz'].data_ptr(), o['pptr'].data_ptr(), o['P'] * M, o['P'], o['ptype'].data_ptr(),
              o['pstatus'].data_ptr(), None))

def score(o):
    p = hip.vina_params()
    hip.check(L.kpd_vina_score(o['pos'].data_ptr(), o['ptr'].data_ptr(), o['N'], o['B'], o['n'], o['elem'].data_ptr(), len(ELEMENTS),
              o['z'].data_ptr(), o['lig_radius'].data_ptr(), o['bonds'].data_ptr(), o['order'].data_ptr(), o['bond_ptr'].data_ptr(), 3 * o['N'],
              o['status'].data_ptr(), None, o['px'].data_ptr(), o['prad'].data_ptr(), o['ptype'].data_ptr(), o['pptr'].data_ptr(), o['P'] * M,
              o['P'], M, o['pof'].data_ptr(), ctypes.byref(p), o['report'].data_ptr(), None, None, None, o['vstatus'].data_ptr(), None))

def minimize(o, **params):
    p = hip.vina_min_params(**params)
    hip.check(L.kpd_vina_minimize(o['pos'].data_ptr(), o['ptr'].data_ptr(), o['N'], o['B'], o['n'], o['elem'].data_ptr(), len(ELEMENTS),
              o['z'].data_ptr(), o['lig_radius'].data_ptr(), o['frag'].data_ptr(), o['bonds'].data_ptr(), o['order'].data_ptr(),
              o['bond_ptr'].data_ptr(), 3 * o['N'], o['status'].data_ptr(), None, o['px'].data_ptr(), o['prad'].data_ptr(),
              o['ptype'].data_ptr(), o['pptr'].data_ptr(), o['P'] * M, o['P'], M, o['pof'].data_ptr(), 64, ctypes.byref(p),
              o['pos_out'].data_ptr(), o['mreport'].data_ptr(), o['mstatus'].data_ptr(), None))

def timed(fn, reps, warm):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize(); ts.append(a.elapsed_time(b) * 1e3)
    return np.array(ts)

def show(ts):
    return f'median {np.median(ts):.1f} us, min {ts.min():.1f}, max {ts.max():.1f} ({len(ts)} runs)'

for B, n, group, chain in ((6400, 25, 100, False), (64, 60, 64, False), (6400, 25, 100, True), (64, 60, 64, True)):
    o = setup(B, n, group, chain)
    perceive(o); pocket_types(o); score(o); minimize(o); torch.cuda.synchronize()
    rep, st = o['mreport'], o['mstatus']
    ran = (st & (1 | 2 | 32)) == 0
    k = int(ran.sum())
    evals, iters = float(rep[ran, COL['evaluations']].sum()), float(rep[ran, COL['iterations']].sum())
    print(f'B={B} x {n} atoms ({"chains" if chain else "clouds"}) in {o["P"]} pockets of {M}: status bits {[int((st & b).ne(0).sum()) for b in (1, 2, 4, 8, 16, 32, 64)]} '
          f'(1 .. 64), {k} ligands minimised; mean iterations {iters / max(k, 1):.1f}, mean evaluations {evals / max(k, 1):.1f}, mean N_rot '
          f'{float(rep[ran, COL["n_rot"]].mean()):.2f}, mean fragments {float(rep[ran, COL["n_frag"]].mean()):.2f}, mean score '
          f'{float(rep[ran, COL["score_before"]].mean()):.3f} -> {float(rep[ran, COL["score_after"]].mean()):.3f}, mean E '
          f'{float(rep[ran, COL["E_before"]].mean()):.3f} -> {float(rep[ran, COL["E_after"]].mean()):.3f}, mean rmsd '
          f'{float(rep[ran, COL["rmsd"]].mean()):.3f}')
    ts = timed(lambda: score(o), 20, 3)
    t1 = timed(lambda: minimize(o, max_iters=0), 20, 3)
    tm = timed(lambda: minimize(o), 5, 1)
    per_score = np.median(ts) / B
    per_eval = np.median(tm) / max(evals, 1.0)
    print('  kpd_vina_score, report only                ', show(ts), f'-> {per_score * 1e3:.1f} ns per ligand')
    print('  kpd_vina_minimize, max_iters 0 (1 eval)    ', show(t1), f'-> {np.median(t1) / B * 1e3:.1f} ns per ligand')
    print('  kpd_vina_minimize, defaults (max_iters 200)', show(tm), f'-> {per_eval * 1e3:.1f} ns per ligand-evaluation')
    print(f'  ratio ligand-evaluation / k_vina_score ligand: {per_eval / per_score:.2f}; one-evaluation call / k_vina_score call: '
          f'{np.median(t1) / np.median(ts):.2f}')
