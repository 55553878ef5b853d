"""Timing of kpd_vina_pocket_types and kpd_vina_score next to kpd_mol_perceive (profiles/vina.md).
    python profiles/tools/vina_bench.py      HIP events around the raw C calls (buffers preallocated, no host sync inside)
The inputs are those of profiles/tools/relax_bench.py: seeded normal clouds of 1.6 A x (n / 20)^(1/3), one-hot features over ten
element classes; 6 400 ligands of 25 atoms, 100 per pocket, in 64 pockets of 300 atoms, and 64 ligands of 60 atoms in one pocket
of 300.  A pocket is 300 atoms drawn uniformly from the shell 4.5 .. 11 A around the origin, where the clouds sit."""
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

def setup(B, n, group):
    g = torch.Generator().manual_seed(B * 1000 + n)
    N, P = B * n, B // group
    pos = (torch.randn(N, 3, generator=g) * 1.6 * (n / 20.0) ** (1.0 / 3.0)).to(dev)
    cls = torch.tensor(POOL)[torch.randint(0, len(POOL), (N,), generator=g)]
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
             report=f64(B, 8), grad=f64(N, 3), atom=f64(N), ltype=i32(N), vstatus=i32(B))
    o['s1'] = torch.empty(int(L.kpd_mol_scratch_bytes(N, B)), dtype=torch.uint8, device=dev)
    return o

def perceive(o):
    hip.check(L.kpd_mol_perceive(o['pos'].data_ptr(), o['feat'].data_ptr(), o['ptr'].data_ptr(), o['N'], o['B'], len(ELEMENTS), o['z'].data_ptr(),
              o['allowed'].data_ptr(), 3 * o['N'], o['elem'].data_ptr(), o['valence'].data_ptr(), o['frag'].data_ptr(), o['bonds'].data_ptr(),
              o['order'].data_ptr(), o['bond_ptr'].data_ptr(), o['summary'].data_ptr(), o['status'].data_ptr(), o['s1'].data_ptr(), None))

def pocket_types(o):
    hip.check(L.kpd_vina_pocket_types(o['px'].data_ptr(), o['pz'].data_ptr(), o['pptr'].data_ptr(), o['P'] * M, o['P'], o['ptype'].data_ptr(),
              o['pstatus'].data_ptr(), None))

def score(o, outputs=True):
    p = hip.vina_params()
    opt = lambda k: o[k].data_ptr() if outputs else None
    hip.check(L.kpd_vina_score(o['pos'].data_ptr(), o['ptr'].data_ptr(), o['N'], o['B'], o['n'], o['elem'].data_ptr(), len(ELEMENTS),
              o['z'].data_ptr(), o['lig_radius'].data_ptr(), o['bonds'].data_ptr(), o['order'].data_ptr(), o['bond_ptr'].data_ptr(), 3 * o['N'],
              o['status'].data_ptr(), None, o['px'].data_ptr(), o['prad'].data_ptr(), o['ptype'].data_ptr(), o['pptr'].data_ptr(), o['P'] * M,
              o['P'], M, o['pof'].data_ptr(), ctypes.byref(p), o['report'].data_ptr(), opt('grad'), opt('atom'), opt('ltype'),
              o['vstatus'].data_ptr(), None))

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

for B, n, group in ((6400, 25, 100), (64, 60, 64)):
    o = setup(B, n, group)
    perceive(o); pocket_types(o); score(o); torch.cuda.synchronize()
    rep, st = o['report'], o['vstatus']
    pairs = B * n * M
    print(f'B={B} x {n} atoms in {o["P"]} pockets of {M}: status bits {[int((st & b).ne(0).sum()) for b in (1, 2, 4)]}, pocket status '
          f'{int(o["pstatus"].ne(0).sum())}, pocket types {torch.bincount(o["ptype"] + 1, minlength=9).tolist()} (-1 .. 7), ligand types '
          f'{torch.bincount(o["ltype"] + 1, minlength=9).tolist()}, mean score {float(rep[:, 0].mean()):.3f}, mean terms '
          f'{[round(float(v), 3) for v in rep[:, 2:7].mean(dim=0)]}, mean N_rot {float(rep[:, 7].mean()):.2f}')
    tp = timed(lambda: perceive(o), 50, 5)
    tt = timed(lambda: pocket_types(o), 50, 5)
    ts = timed(lambda: score(o), 50, 5)
    tl = timed(lambda: score(o, False), 50, 5)
    print('  kpd_mol_perceive                          ', show(tp))
    print('  kpd_vina_pocket_types                     ', show(tt))
    print('  kpd_vina_score, grad + atom_score + types ', show(ts))
    print('  kpd_vina_score, report only               ', show(tl))
    print(f'  {pairs / (np.median(ts) * 1e-6) / 1e9:.1f} G pair visits/s ({pairs} ligand x pocket pairs per call)')
