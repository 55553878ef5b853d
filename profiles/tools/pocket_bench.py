"""Timing of the pocket entry points on the fixture complexes (profiles/pocket.md).
    python profiles/tools/pocket_bench.py time        HIP events around the raw C calls (buffers preallocated, no host sync inside),
                                                      then the interface-point call with its phases cut off one at a time
    rocprofv3 --kernel-trace --stats --output-format csv -- python profiles/tools/pocket_bench.py B
                                                      ten calls of each entry point at batch size B (1 = the 13.5 k-atom receptor)
"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from keypoint_diffusion_amd import hip
from tests.test_pocket_config import load_cases

dev = torch.device('cuda:0')
cases = load_cases()
mode = sys.argv[1]
L = hip.lib()

def setup(cs):
    pos = torch.cat([c['rec_pos'] for c in cs]).to(dev); res = torch.cat([c['rec_res'] for c in cs]).to(dev)
    keep = (~torch.cat([c['other'] for c in cs])).to(dev).view(torch.uint8); lig = torch.cat([c['lig_pos'] for c in cs]).to(dev)
    rc = [c['rec_pos'].shape[0] for c in cs]; lc = [c['lig_pos'].shape[0] for c in cs]
    p32 = lambda v: torch.tensor([0] + list(np.cumsum(v)), dtype=torch.int32, device=dev)
    B, n_rec, n_lig = len(cs), sum(rc), sum(lc)
    o = dict(pos=pos, res=res, keep=keep, lig=lig, rp=p32(rc), lp=p32(lc), B=B, n_rec=n_rec, n_lig=n_lig, max_rec=max(rc))
    o['in_box'] = torch.empty(n_rec, dtype=torch.uint8, device=dev); o['mask'] = torch.empty(n_rec, dtype=torch.uint8, device=dev)
    o['rows'] = torch.empty(n_rec, dtype=torch.int32, device=dev); o['pres'] = torch.empty(n_rec, dtype=torch.int32, device=dev)
    o['meta'] = torch.empty(2 * B + 1, dtype=torch.int32, device=dev); o['meta2'] = torch.empty(3 * B + 1, dtype=torch.int32, device=dev)
    o['s1'] = torch.empty(int(L.kpd_pocket_scratch_bytes(n_rec, B)), dtype=torch.uint8, device=dev)
    o['s2'] = torch.empty(int(L.kpd_interface_points_scratch_bytes(n_rec, B, 2048)), dtype=torch.uint8, device=dev)
    o['pts'] = torch.empty(B * 2048, 3, device=dev)
    return o

def select(o, pad=8.0, cut=8.0):
    m = o['meta'].data_ptr()
    hip.check(L.kpd_pocket_select(o['pos'].data_ptr(), o['rp'].data_ptr(), o['res'].data_ptr(), o['keep'].data_ptr(), o['keep'].data_ptr(), o['n_rec'], o['max_rec'],
              o['lig'].data_ptr(), o['lp'].data_ptr(), o['n_lig'], o['B'], pad, cut, o['n_rec'], o['in_box'].data_ptr(), o['mask'].data_ptr(), o['rows'].data_ptr(),
              o['pres'].data_ptr(), m, m + 4 * (o['B'] + 1), o['s1'].data_ptr(), None))

def points(o, cand, thr=5.0, excl=2.0):
    m = o['meta2'].data_ptr(); B = o['B']
    hip.check(L.kpd_interface_points(o['pos'].data_ptr(), o['rp'].data_ptr(), cand.data_ptr(), o['n_rec'], o['lig'].data_ptr(), o['lp'].data_ptr(), o['n_lig'], B,
              thr, excl, 2048, B * 2048, o['pts'].data_ptr(), m, m + 4 * (B + 1), m + 4 * (2 * B + 1), o['s2'].data_ptr(), None))

def timed(fn, reps=50):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize(); ts.append(a.elapsed_time(b) * 1e3)
    ts = np.array(ts)
    return f'median {np.median(ts):.1f} us, min {ts.min():.1f}, max {ts.max():.1f} ({reps} runs)'

if mode == 'time':
    for name, cs in (('B=64 (8 fixtures x 8)', cases * 8), ('B=1, 13.5k-atom receptor', [cases[7]]), ('B=8 fixtures', cases)):
        o = setup(cs)
        select(o); torch.cuda.synchronize()
        cand_box = (o['in_box'] & o['keep']).contiguous(); cand_pocket = o['mask'].clone()
        print(name, 'n_rec', o['n_rec'], 'pocket atoms', int(o['meta'][o['B']]))
        print('  kpd_pocket_select            ', timed(lambda: select(o)))
        print('  kpd_interface_points (box)   ', timed(lambda: points(o, cand_box)), 'points', int(o['meta2'][o['B']]))
        print('  kpd_interface_points (pocket)', timed(lambda: points(o, cand_pocket)), 'points', int(o['meta2'][o['B']]))
else:
    B = int(mode)
    o = setup((cases * 8)[:B] if B > 1 else [cases[7]])
    select(o); torch.cuda.synchronize()
    cand = (o['in_box'] & o['keep']).contiguous()
    for _ in range(10):
        select(o); points(o, cand)
    torch.cuda.synchronize()
    print('done', B)
if mode == 'time':
    for name, cs in (('B=64', cases * 8), ('B=1 13.5k', [cases[7]])):
        o = setup(cs)
        select(o); torch.cuda.synchronize()
        cand = (o['in_box'] & o['keep']).contiguous()
        print(name, 'phase attribution of kpd_interface_points (box set)')
        print('  full (thr 5, excl 2)              ', timed(lambda: points(o, cand)))
        print('  thinning cut (excl 1e9: 1 point)  ', timed(lambda: points(o, cand, 5.0, 1e9)))
        print('  no candidate pair (thr 0)         ', timed(lambda: points(o, cand, 0.0, 2.0)))
        print('  no candidate atom (mask all zero) ', timed(lambda: points(o, torch.zeros_like(cand))))
