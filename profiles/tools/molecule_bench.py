"""Timing of the molecule entry points (profiles/molecule.md).
    python profiles/tools/molecule_bench.py time      HIP events around the raw C calls (buffers preallocated, no host sync inside)
    rocprofv3 --kernel-trace --stats --output-format csv -- python profiles/tools/molecule_bench.py trace
                                                      ten calls of each entry point at both sizes
Ligands are normal clouds of 1.6 A x (n / 20)^(1/3) with one-hot features over ten element classes (seeded)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from keypoint_diffusion_amd import hip, molecule

dev = torch.device('cuda:0')
mode = sys.argv[1]
L = hip.lib()
ELEMENTS = ['C', 'N', 'O', 'S', 'P', 'F', 'Cl', 'Br', 'I', 'B']
POOL = [0, 0, 0, 1, 2, 3, 6, 5, 4, 7]

def setup(B, n):
    g = torch.Generator().manual_seed(B * 1000 + n)
    N = B * n
    pos = (torch.randn(N, 3, generator=g) * 1.6 * (n / 20.0) ** (1.0 / 3.0)).to(dev)
    cls = torch.tensor(POOL)[torch.randint(0, len(POOL), (N,), generator=g)]
    feat = torch.nn.functional.one_hot(cls, len(ELEMENTS)).float().to(dev)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    z, allowed = molecule._class_tables(ELEMENTS, None)
    o = dict(B=B, N=N, pos=pos, feat=feat, ptr=(torch.arange(B + 1, dtype=torch.int32) * n).to(dev), z=torch.tensor(z, dtype=torch.int32, device=dev),
             allowed=torch.tensor(allowed, dtype=torch.int32, device=dev), elem=i32(N), valence=i32(N), frag=i32(N), bonds=i32(3 * N, 2), order=i32(3 * N),
             bond_ptr=i32(B + 1), summary=i32(B, 4), status=i32(B), sdf_status=i32(B), text_ptr=torch.empty(B + 1, dtype=torch.int64, device=dev))
    o['cap_text'] = 70 * N + 13 * 3 * N + 77 * B
    o['text'] = torch.empty(o['cap_text'], dtype=torch.uint8, device=dev)
    o['s1'] = torch.empty(int(L.kpd_mol_scratch_bytes(N, B)), dtype=torch.uint8, device=dev)
    o['s2'] = torch.empty(int(L.kpd_sdf_scratch_bytes(N, B)), dtype=torch.uint8, device=dev)
    o['sym'] = hip._packed_symbols(ELEMENTS, dev, 3)
    return o

def perceive(o):
    hip.check(L.kpd_mol_perceive(o['pos'].data_ptr(), o['feat'].data_ptr(), o['ptr'].data_ptr(), o['N'], o['B'], len(ELEMENTS), o['z'].data_ptr(),
              o['allowed'].data_ptr(), 3 * o['N'], o['elem'].data_ptr(), o['valence'].data_ptr(), o['frag'].data_ptr(), o['bonds'].data_ptr(),
              o['order'].data_ptr(), o['bond_ptr'].data_ptr(), o['summary'].data_ptr(), o['status'].data_ptr(), o['s1'].data_ptr(), None))

def sdf(o, largest=0):
    hip.check(L.kpd_sdf_emit(o['pos'].data_ptr(), o['ptr'].data_ptr(), o['N'], o['B'], o['elem'].data_ptr(), len(ELEMENTS), o['sym'].data_ptr(),
              o['frag'].data_ptr(), o['bonds'].data_ptr(), o['order'].data_ptr(), o['bond_ptr'].data_ptr(), 3 * o['N'], o['status'].data_ptr(), largest,
              o['text'].data_ptr(), o['cap_text'], o['text_ptr'].data_ptr(), o['sdf_status'].data_ptr(), o['s2'].data_ptr(), None))

def timed(fn, reps=50):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize(); ts.append(a.elapsed_time(b) * 1e3)
    ts = np.array(ts)
    return f'median {np.median(ts):.1f} us, min {ts.min():.1f}, max {ts.max():.1f} ({reps} runs)'

for B, n in ((6400, 25), (64, 60)):
    o = setup(B, n)
    perceive(o); sdf(o); torch.cuda.synchronize()
    if mode == 'time':
        s = o['summary'].sum(0).tolist()
        print(f'B={B} x {n} atoms: {o["N"]} atoms, {s[0]} bonds, {s[1]} fragments, {s[3]} invalid atoms, {int(o["text_ptr"][B])} bytes of SDF, status',
              int(o['status'].max()), int(o['sdf_status'].max()))
        print('  kpd_mol_perceive              ', timed(lambda: perceive(o)))
        print('  kpd_sdf_emit                  ', timed(lambda: sdf(o)))
        print('  kpd_sdf_emit, largest fragment', timed(lambda: sdf(o, 1)))
    else:
        for _ in range(10):
            perceive(o); sdf(o)
        torch.cuda.synchronize()
        print('done', B, n)
