"""Cost and effect of clash guidance (profiles/guidance.md) at the contract shape: B = 64 x (300-atom pocket, 25-atom ligand),
10 features, the contract model (`bench.py` `egnn_all_atom`, fixed encoder: the 300 pocket atoms are the keypoints), the 300
pocket atoms as wall, threshold 3 A.

    python profiles/tools/guidance_timing.py [--parent-lib PATH] [--effect] [--out FILE]

--parent-lib: libkpd_hip.so of the parent commit; its kpd_sample_update is timed on the same inputs next to this commit's.
--effect: also run the whole reverse loop with scale 0, 0.5 and 1 over the same seeds and report `clash_score` of the final samples
(seeded random weights: what the numbers say about a trained model's chemistry is nothing).
On a commit without the guidance entry points (the parent) the tool times the plain step only, so the same file gives the
parent's step for the comparison.
Protocol, as profiles/tools/inpaint_timing.py: HIP events around N back-to-back calls on one stream (kernels: N = 500 after 50
warm-up calls, steps: N = 50 after 10, every step window from the same saved state); every variant is timed ROUNDS times, the
variants alternating inside each round; the table gives the median and the range of the per-call times over the rounds."""
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

try:
    from keypoint_diffusion_amd.ligand_diffuser import ClashGuidance, GuidanceContext
except ImportError:                              # the parent commit: plain step only
    ClashGuidance = GuidanceContext = None

ROUNDS = 7
THRESHOLD = 3.0


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


def effect(model, dev, B, n_rec, n_lig, seeds=(1, 2)):
    """`clash_score` of the final samples against the pocket atoms, scale 0 / 0.5 / 1, the same seeds and complex ids."""
    out = {}
    ids = torch.arange(B)
    unguided = {}
    for wall_kind in ('pocket atoms', 'unguided ligands of the same seed'):
        for scale in (0.0, 0.5, 1.0):
            energy, pairs, dmin, clean = [], [], [], []
            for seed in seeds:
                model.use_complex_noise(seed)
                g = bench.build_batch(model, B, n_rec, n_lig, 0, dev)
                if wall_kind == 'pocket atoms':
                    walls, wall = [w.cpu() for w in g.nodes['kp'].data['x_0'].split(g.batch_num_nodes('kp').tolist())], None
                else:                                # an obstacle where this model puts its ligands: the wall is met whatever the weights
                    walls = unguided[seed]
                    wall = (torch.cat(walls).to(dev), torch.tensor([0] + [w.shape[0] for w in walls]).cumsum(0))
                with torch.no_grad():
                    pos, _ = model.sample_from_encoded_receptors(g, complex_ids=ids, guidance=ClashGuidance(THRESHOLD, scale=scale, wall=wall))
                if wall_kind == 'pocket atoms' and scale == 0.0:
                    unguided[seed] = pos
                sc = model.clash_score(pos, walls, THRESHOLD)
                energy.append(float(sc[:, 0].mean())), pairs.append(float(sc[:, 1].mean()))
                dmin.append(float(sc[:, 2][torch.isfinite(sc[:, 2])].min()) if bool(torch.isfinite(sc[:, 2]).any()) else None)
                clean.append(int((sc[:, 1] == 0).sum()))
            out[f'wall = {wall_kind}, scale {scale}'] = dict(mean_energy_per_ligand=[round(e, 3) for e in energy],
                                                             mean_pairs_per_ligand=[round(p, 2) for p in pairs], smallest_distance=dmin,
                                                             ligands_without_a_pair=clean, seeds=list(seeds))
    model.use_complex_noise(None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib')
    ap.add_argument('--effect', action='store_true')
    ap.add_argument('--out')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    B, n_rec, n_lig, F = 64, 300, 25, 10
    model = bench.build_model(dev)
    g = bench.build_batch(model, B, n_rec, n_lig, 0, dev)
    pb, bidx = g.prepared(), G.get_batch_idxs(g)
    lig, kp = g.nodes['lig'].data, g.nodes['kp'].data
    lig['x_0'], lig['h_0'], kp['x_0'] = lig['x_0'].float().contiguous(), lig['h_0'].float().contiguous(), kp['x_0'].float().contiguous()
    state = (lig['x_0'], lig['h_0'], kp['x_0'])
    saved = [t.clone() for t in state]
    N = B * n_lig
    r = lambda w: torch.randn(N, w, device=dev)
    eps_x, eps_h, nx, nh = r(3), r(F), r(3), r(F)
    T = model.n_timesteps
    s, t = torch.full((B,), 0.5, device=dev), torch.full((B,), 0.5 + 1.0 / T, device=dev)
    out = {'shape': dict(B=B, n_rec=n_rec, n_lig=n_lig, atom_nf=F, wall_atoms_per_complex=n_rec, threshold=THRESHOLD),
           'gpu': torch.cuda.get_device_name(0), 'guidance_available': ClashGuidance is not None}

    def reset():                                 # every timed window starts from the same state: the step's cost depends on its graph
        for x, c in zip(state, saved):
            x.copy_(c)

    steps = {'plain step (sample_p_zs_given_zt)': lambda: model.sample_p_zs_given_zt(s, t, g, bidx)}
    if ClashGuidance is not None:
        ctx = GuidanceContext(*model.resolve_wall(g), G.readout_nodes(g, 'x_0', op='mean', ntype='kp', ordered=True), THRESHOLD)
        coef3, coef9 = model.step_coefficients(s, t), model.guided_coefficients(s, t, 1.0, 1.0)
        L = hip.lib()
        head = (pb.B, pb.lig_ptr.data_ptr(), pb.kp_ptr.data_ptr(), F)
        ptrs = [a.data_ptr() for a in (*state, eps_x, eps_h, nx, nh, coef3)]
        ptrs9 = [a.data_ptr() for a in (*state, eps_x, eps_h, nx, nh, coef9)] + [None, None, None, ctx.kp_com0.data_ptr(), None, None,
                                                                                ctx.wall_ptr.data_ptr(), ctx.wall_x.data_ptr()]
        stream = torch.cuda.current_stream().cuda_stream

        def raw(fn, p, *tail):
            def call():
                assert fn(*head, *p, *tail, pb.max_lig, stream) == 0
            return call
        score_out = torch.empty(B, 3, device=dev)
        kernels = {
            'kpd_sample_update (this commit), direct call': raw(L.kpd_sample_update, ptrs),
            'kpd_sample_update_guided, 300 wall atoms per complex, direct call': raw(L.kpd_sample_update_guided, ptrs9, THRESHOLD),
            'kpd_clash_score, direct call': lambda: L.kpd_clash_score(B, pb.lig_ptr.data_ptr(), state[0].data_ptr(), ctx.wall_ptr.data_ptr(),
                                                                      ctx.wall_x.data_ptr(), THRESHOLD, score_out.data_ptr(), stream),
            'kpd_sample_update_guided, through hip.py': lambda: hip.sample_update_guided(pb, F, *state, eps_x, eps_h, nx, nh, coef9, ctx.wall_x,
                                                                                        ctx.wall_ptr, ctx.kp_com0, THRESHOLD),
            'kpd_step_coefficients, through hip.py': lambda: hip.step_coefficients(model.gamma.gamma, s, t),
            'kpd_guided_coefficients, through hip.py': lambda: hip.guided_coefficients(model.gamma.gamma, s, t, 1.0, 1.0),
        }
        same = None
        if args.parent_lib:
            P = C.CDLL(os.path.abspath(args.parent_lib))
            P.kpd_sample_update.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 8 + [C.c_int32, C.c_void_p]
            parent = raw(P.kpd_sample_update, ptrs)
            parent()                                 # same inputs, same bits
            a = [x.clone() for x in state]
            reset()
            kernels['kpd_sample_update (this commit), direct call']()
            same = all(torch.equal(x, y) for x, y in zip(state, a))
            reset()
            kernels = {'kpd_sample_update (parent commit), direct call': parent, **kernels}
        out['parent_and_this_commit_same_bits'] = same
        out['kernels'] = alternate(kernels, 500, 50, reset)
        off = GuidanceContext(ctx.wall_x, ctx.wall_ptr, ctx.kp_com0, THRESHOLD, scale=0.0)
        steps['guided step, 300 wall atoms per complex'] = lambda: model.sample_p_zs_given_zt(s, t, g, bidx, guidance=ctx)
        steps['guided step, scale = 0 (the pair loop is skipped)'] = lambda: model.sample_p_zs_given_zt(s, t, g, bidx, guidance=off)
    with torch.no_grad():
        out['steps'] = alternate(steps, 50, 10, reset)
        if args.effect and ClashGuidance is not None:
            out['effect'] = effect(model, dev, B, n_rec, n_lig)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
