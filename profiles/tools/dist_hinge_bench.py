"""The receptor-ligand hinge kernel (kpd_dist_hinge) at the C2 shape (B = 64 x 300 / 25) and at ragged B = 512 (size_pairs.json), and one
training step (forward, backward, Adam) of egnn_40kp_train and egnn_train with and without the rl_hinge term.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python profiles/tools/dist_hinge_bench.py` (k_hinge_rows, k_hinge_total); it prints wall times."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
import bench
from keypoint_diffusion_amd import optim
from keypoint_diffusion_amd.dist_hinge_loss import segmented_dist_hinge

dev = torch.device('cuda:0')


def timed(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


def hinge_case(tag, pairs):
    gen = torch.Generator().manual_seed(1)
    rec = [torch.rand(r, 3, generator=gen) * 14 for r, _ in pairs]
    lig = [torch.rand(l, 3, generator=gen) * 5 + 4.5 for _, l in pairs]
    a = torch.cat(lig).to(dev).requires_grad_(True)
    b = torch.cat(rec).to(dev)
    ptr = lambda xs: torch.tensor([0] + torch.tensor([len(x) for x in xs]).cumsum(0).tolist(), dtype=torch.int32, device=dev)
    ap, bp = ptr(lig), ptr(rec)
    n_pairs = sum(len(l) * len(r) for l, r in zip(lig, rec))
    ms = timed(lambda: segmented_dist_hinge(a, ap, b, bp, 3.5), 50)
    print(json.dumps(dict(case=tag, B=len(pairs), pairs=n_pairs, ms_per_call_wall=ms)))


pairs512 = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'size_pairs.json')))['all_atom']['pairs'][:512]
hinge_case('c2_64x300x25', [(300, 25)] * 64)
hinge_case('ragged_512', pairs512)

for wl in ('egnn_40kp_train', 'egnn_train'):
    model = bench.build_model(dev, wl).train()
    opt = optim.Adam(model.parameters(), lr=1e-4)
    template = bench.raw_batch(64, 300, 25, 1234, dev, wl).to(dev)
    for thr in (0, 3.5):
        model.rl_dist_threshold = thr

        def step():
            out = model(template.to(dev), None)
            loss = out['l2'] + (out['rl_hinge'] if thr > 0 else 0)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        ms = timed(step, 10)
        print(json.dumps(dict(workload=wl, rl_dist_threshold=thr, ms_per_step=ms)))
