"""Cost of the inpainting step (profiles/inpaint.md): the fused update kernels and the extra noise draws at the contract shape
(B = 64 x 300-atom pocket x 25-atom ligand, 10 features), and one inpainting step of the contract model next to one plain step.

    python profiles/tools/inpaint_timing.py [--parent-lib PATH] [--out FILE]

--parent-lib: libkpd_hip.so of the parent commit; its kpd_sample_update is timed on the same inputs next to this commit's.
Protocol: HIP events around N back-to-back launches on one stream (kernels: N = 500, steps: N = 50) after 50 / 10 warm-up calls (a step window starts from the
same saved state each time, so the per-step graphs are comparable);
every variant is timed ROUNDS times, the variants alternating inside each round; the table gives the median and the range of the
per-call times over the rounds.  Back-to-back launches overlap launch overhead with execution, so the kernel figures are
throughput per call, the number that matters inside a step that is a queue of dependent launches."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from keypoint_diffusion_amd import graph as G  # noqa: E402
from keypoint_diffusion_amd import hip  # noqa: E402
from keypoint_diffusion_amd.ligand_diffuser import InpaintContext  # noqa: E402

ROUNDS = 7


def timed(fn, n, warm, reset=None):
    if reset is not None:
        reset()
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n           # us per call


def alternate(variants, n, warm, reset=None):
    times = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            times[k].append(timed(fn, n, warm, reset))
    return {k: dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib')
    ap.add_argument('--out')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    B, n_rec, n_lig, F = 64, 300, 25, 10
    model = bench.build_model(dev)
    g = bench.build_batch(model, B, n_rec, n_lig, 0, dev)
    pb, bidx = g.prepared(), G.get_batch_idxs(g)
    lig, kp = g.nodes['lig'].data, g.nodes['kp'].data
    lig['x_0'], lig['h_0'], kp['x_0'] = lig['x_0'].float().contiguous(), lig['h_0'].float().contiguous(), kp['x_0'].float().contiguous()
    saved = [t.clone() for t in (lig['x_0'], lig['h_0'], kp['x_0'])]
    N = B * n_lig
    r = lambda w: torch.randn(N, w, device=dev)
    eps_x, eps_h, nx, nh, kx, kh = r(3), r(F), r(3), r(F), r(3), r(F)
    T = model.n_timesteps
    s, t = torch.full((B,), 0.5, device=dev), torch.full((B,), 0.5 + 1.0 / T, device=dev)
    coef3, coef6 = model.step_coefficients(s, t), model.inpaint_coefficients(s, t)
    fixed = (torch.arange(N, device=dev) % 2 == 0)
    ctx = InpaintContext(fixed, lig['x_0'].clone(), lig['h_0'].clone(), G.readout_nodes(g, 'x_0', op='mean', ntype='kp'))
    ids = torch.arange(B, device=dev)
    # alpha_t|s ~ 1 at the middle of the schedule: the state stays bounded over the repeated in-place calls
    state = (lig['x_0'], lig['h_0'], kp['x_0'])
    kernels = {
        'kpd_sample_update (this commit)': lambda: hip.sample_update(pb, F, *state, eps_x, eps_h, nx, nh, coef3),
        'kpd_sample_update_inpaint, half the atoms fixed': lambda: hip.sample_update_inpaint(pb, F, *state, eps_x, eps_h, nx, nh, coef6, ctx.fixed,
                                                                                            ctx.x, ctx.h, ctx.kp_com0, kx, kh),
        'kpd_sample_renoise': lambda: hip.sample_renoise(pb, F, *state, nx, nh, coef6),
        'kpd_step_coefficients': lambda: hip.step_coefficients(model.gamma.gamma, s, t),
        'kpd_inpaint_coefficients': lambda: hip.inpaint_coefficients(model.gamma.gamma, s, t),
        'two torch.randn draws (known x, known h)': lambda: (torch.randn(N, 3, device=dev), torch.randn(N, F, device=dev)),
        'two kpd_complex_noise draws (known x, known h)': lambda: (hip.complex_noise(pb, 3, ids, 7, 3, 2), hip.complex_noise(pb, F, ids, 7, 3, 3)),
    }
    # The wrappers above cost ~9 us of host time per call, more than these kernels run: back to back they measure the host.  The
    # library entry points called directly (pointers taken once) measure the launches, and put both commits on the same footing.
    L = hip.lib()
    head = (pb.B, pb.lig_ptr.data_ptr(), pb.kp_ptr.data_ptr(), F)
    ptrs = [a.data_ptr() for a in (*state, eps_x, eps_h, nx, nh, coef3)]
    ptrs6 = [a.data_ptr() for a in (*state, eps_x, eps_h, nx, nh, coef6, ctx.fixed, ctx.x, ctx.h, ctx.kp_com0, kx, kh)]
    ptrs_r = [a.data_ptr() for a in (*state, nx, nh, coef6)]
    stream = torch.cuda.current_stream().cuda_stream

    def raw(fn, p):
        def call():
            assert fn(*head, *p, pb.max_lig, stream) == 0
        return call
    kernels = {'kpd_sample_update (this commit), direct call': raw(L.kpd_sample_update, ptrs),
               'kpd_sample_update_inpaint, half the atoms fixed, direct call': raw(L.kpd_sample_update_inpaint, ptrs6),
               'kpd_sample_renoise, direct call': raw(L.kpd_sample_renoise, ptrs_r),
               **{k + (', through hip.py' if k.startswith('kpd_') else ''): v for k, v in kernels.items()}}
    if args.parent_lib:
        P = C.CDLL(os.path.abspath(args.parent_lib))
        P.kpd_sample_update.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 8 + [C.c_int32, C.c_void_p]
        parent = raw(P.kpd_sample_update, ptrs)
        # same inputs, same bits
        parent()
        a = [x.clone() for x in state]
        for x, c in zip(state, saved):
            x.copy_(c)
        kernels['kpd_sample_update (this commit), direct call']()
        same = all(torch.equal(x, y) for x, y in zip(state, a))
        kernels = {'kpd_sample_update (parent commit), direct call': parent, **kernels}
    else:
        same = None
    out = {'shape': dict(B=B, n_rec=n_rec, n_lig=n_lig, atom_nf=F), 'gpu': torch.cuda.get_device_name(0),
           'parent_and_this_commit_same_bits': same, 'kernels': alternate(kernels, 500, 50)}
    def reset():                                 # every timed window starts from the same state: the step's cost depends on its graph
        for x, c in zip(state, saved):
            x.copy_(c)

    free = InpaintContext(torch.zeros_like(fixed), ctx.x, ctx.h, ctx.kp_com0)
    with torch.no_grad():
        steps = {
            'plain step (sample_p_zs_given_zt)': lambda: model.sample_p_zs_given_zt(s, t, g, bidx),
            'inpainting step, no atom fixed (the same dynamics as the plain step)': lambda: model.sample_p_zs_given_zt(s, t, g, bidx, inpaint=free),
            'inpainting step, half the atoms fixed': lambda: model.sample_p_zs_given_zt(s, t, g, bidx, inpaint=ctx),
        }
        out['steps'] = alternate(steps, 50, 10, reset)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
