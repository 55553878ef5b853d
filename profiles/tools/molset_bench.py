"""Timing of the set-level molecule entry points next to kpd_mol_perceive (profiles/molset.md).
    python profiles/tools/molset_bench.py      HIP events around the raw C calls (buffers preallocated, no host sync inside)
The ligands are those of profiles/tools/molecule_bench.py: seeded normal clouds of 1.6 A x (n / 20)^(1/3), one-hot features over
ten element classes; 6 400 ligands of 25 atoms in 64 groups of 100, and 64 ligands of 60 atoms in one group."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from keypoint_diffusion_amd import hip, molecule

dev = torch.device('cuda:0')
L = hip.lib()
ELEMENTS = ['C', 'N', 'O', 'S', 'P', 'F', 'Cl', 'Br', 'I', 'B']
POOL = [0, 0, 0, 1, 2, 3, 6, 5, 4, 7]
NBITS = 2048

def setup(B, n, group):
    g = torch.Generator().manual_seed(B * 1000 + n)
    N = B * n
    pos = (torch.randn(N, 3, generator=g) * 1.6 * (n / 20.0) ** (1.0 / 3.0)).to(dev)
    cls = torch.tensor(POOL)[torch.randint(0, len(POOL), (N,), generator=g)]
    feat = torch.nn.functional.one_hot(cls, len(ELEMENTS)).float().to(dev)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    z, allowed = molecule._class_tables(ELEMENTS, None)
    o = dict(B=B, N=N, G=B // group, pos=pos, feat=feat, ptr=(torch.arange(B + 1, dtype=torch.int32) * n).to(dev),
             z=torch.tensor(z, dtype=torch.int32, device=dev), allowed=torch.tensor(allowed, dtype=torch.int32, device=dev), elem=i32(N),
             valence=i32(N), frag=i32(N), bonds=i32(3 * N, 2), order=i32(3 * N), bond_ptr=i32(B + 1), summary=i32(B, 4), status=i32(B),
             key=torch.empty(B, dtype=torch.int64, device=dev), fp=i32(B, NBITS // 32), atom_inv=torch.empty(N, dtype=torch.int64, device=dev),
             key_status=i32(B), group_ptr=(torch.arange(B // group + 1, dtype=torch.int32) * group).to(dev),
             div=torch.empty(B // group, dtype=torch.float64, device=dev), pairs=torch.empty(B // group, dtype=torch.int64, device=dev),
             div_status=i32(B // group))
    o['s1'] = torch.empty(int(L.kpd_mol_scratch_bytes(N, B)), dtype=torch.uint8, device=dev)
    return o

def perceive(o):
    hip.check(L.kpd_mol_perceive(o['pos'].data_ptr(), o['feat'].data_ptr(), o['ptr'].data_ptr(), o['N'], o['B'], len(ELEMENTS), o['z'].data_ptr(),
              o['allowed'].data_ptr(), 3 * o['N'], o['elem'].data_ptr(), o['valence'].data_ptr(), o['frag'].data_ptr(), o['bonds'].data_ptr(),
              o['order'].data_ptr(), o['bond_ptr'].data_ptr(), o['summary'].data_ptr(), o['status'].data_ptr(), o['s1'].data_ptr(), None))

def keys(o, largest=1, inv=True):
    hip.check(L.kpd_mol_keys(o['ptr'].data_ptr(), o['N'], o['B'], o['elem'].data_ptr(), len(ELEMENTS), o['z'].data_ptr(), o['frag'].data_ptr(),
              o['bonds'].data_ptr(), o['order'].data_ptr(), o['bond_ptr'].data_ptr(), 3 * o['N'], o['status'].data_ptr(), largest, 1, 2, NBITS,
              o['key'].data_ptr(), o['fp'].data_ptr(), o['atom_inv'].data_ptr() if inv else None, o['key_status'].data_ptr(), None))

def diversity(o):
    use = o['use']
    hip.check(L.kpd_fp_diversity(o['fp'].data_ptr(), use.data_ptr(), o['B'], NBITS // 32, o['group_ptr'].data_ptr(), o['G'], o['div'].data_ptr(),
              o['pairs'].data_ptr(), o['div_status'].data_ptr(), None))

def timed(fn, reps=50):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize(); ts.append(a.elapsed_time(b) * 1e3)
    ts = np.array(ts)
    return f'median {np.median(ts):.1f} us, min {ts.min():.1f}, max {ts.max():.1f} ({reps} runs)'

for B, n, group in ((6400, 25, 100), (64, 60, 64)):
    o = setup(B, n, group)
    perceive(o); keys(o)
    o['use'] = (o['key_status'] == 0).to(torch.uint8)
    diversity(o); torch.cuda.synchronize()
    s = o['summary'].sum(0).tolist()
    print(f'B={B} x {n} atoms in {o["G"]} groups of {group}: {o["N"]} atoms, {s[0]} bonds, {s[1]} fragments, {s[2]} atoms in largest fragments, '
          f'{int(torch.unique(o["key"]).numel())} distinct keys, {int(o["pairs"].sum())} pairs, mean diversity '
          f'{float((o["div"] / o["pairs"]).mean()):.4f}, mean bits per row {float(sum(((o["fp"] >> k) & 1).sum() for k in range(32))) / B:.1f}, status',
          int(o['status'].max()), int(o['key_status'].max()), int(o['div_status'].max()))
    print('  kpd_mol_perceive                 ', timed(lambda: perceive(o)))
    print('  kpd_mol_keys, largest fragment   ', timed(lambda: keys(o)))
    print('  kpd_mol_keys, every atom         ', timed(lambda: keys(o, 0)))
    print('  kpd_mol_keys, without atom_inv   ', timed(lambda: keys(o, 1, False)))
    print('  kpd_fp_diversity                 ', timed(lambda: diversity(o)))
