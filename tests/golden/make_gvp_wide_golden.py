#!/usr/bin/env python
"""Generate tests/golden/gvp_wide.npz: upstream's own LigRecDynamicsGVP sub-modules (the encoders, GVPMultiEdgeConv's message GVPs,
GVPLayerNorms and update GVPs, the NoisePredictionBlock) composed as in models/dynamics_gvp.py:149-199 (make_golden.py::gvp_composed),
at n_hidden_scalars 320 and 512, on a ragged 3-complex batch -- the fixture of tests/test_gvp_wide_gpu.py::test_upstream_fixture_parity.
Two cases per width: update_kp with 2 convs and message_norm 10, and update_kp off, 1 conv, 'mean'.

Run in the build container only (it imports the reference, which never travels to the GPU box):
    python tests/golden/make_gvp_wide_golden.py
No weights are stored: each case stores the seed from which synth.fill_state_dict_ rebuilds them (upstream's state-dict layout equals
this library's, checked here).  The reference runs in float64 on the float32 inputs; inputs, edge lists and outputs are stored."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden import make_golden as mg                                  # noqa: E402  (imports the reference modules)

BASE = dict(vector_size=16, n_message_gvps=3, n_update_gvps=2, n_noise_gvps=4, ll_k=0, kl_k=7, dropout=0.0)
CASES = [('s320_kp', 320, dict(n_convs=2, update_kp=True, message_norm=10.0), 41),
         ('s320_mean', 320, dict(n_convs=1, update_kp=False, message_norm='mean'), 42),
         ('s512_kp', 512, dict(n_convs=2, update_kp=True, message_norm=10.0), 43),
         ('s512_mean', 512, dict(n_convs=1, update_kp=False, message_norm='mean'), 44)]
N_REC, N_LIG, BATCH_SEED, V_SEED = [60, 23, 41], [11, 3, 7], 9, 5


def main():
    g, ob = mg.small_batch(N_REC, N_LIG, seed=BATCH_SEED, v=16)
    gen = torch.Generator().manual_seed(V_SEED)
    ob.v['kp'] = 0.5 * torch.randn(ob.x['kp'].shape[0], 16, 3, generator=gen)
    t = torch.linspace(0.2, 0.9, len(N_REC))
    out = dict(n_rec=np.array(N_REC), n_lig=np.array(N_LIG), batch_seed=BATCH_SEED, t=t.numpy(), kp_v=ob.v['kp'].numpy(),
               lig_x=ob.x['lig'].numpy(), lig_h=ob.h['lig'].numpy(), kp_x=ob.x['kp'].numpy(), kp_h=ob.h['kp'].numpy(),
               kk_src=ob.edges['kk'][0].numpy(), kk_dst=ob.edges['kk'][1].numpy(), names=np.array([c[0] for c in CASES]))
    for tag, S, over, seed in CASES:
        kw = dict(BASE, n_hidden_scalars=S, graph_cutoffs=mg.CUT, **over)
        ref, mine = mg.RefGVPDyn(10, 10, **kw), mg.LigRecDynamicsGVP(10, 10, **kw)
        a = {k: list(v.shape) for k, v in ref.state_dict().items()}
        b = {k: list(v.shape) for k, v in mine.state_dict().items()}
        assert a == b, f'{tag}: state-dict layout differs: {set(a) ^ set(b)}'
        mg.synth.fill_state_dict_(ref, seed)
        edges = mg.oegnn.lig_edges(ob, kw)
        edges['kk'] = ob.edges['kk']
        o64 = type(ob)(n=ob.n, x={k: v.double() for k, v in ob.x.items()}, h={k: v.double() for k, v in ob.h.items()},
                       v={k: v.double() for k, v in ob.v.items()}, edges=ob.edges)
        torch.set_default_dtype(torch.float64)            # (gvp_composed's zero-initialised sums and node vectors)
        try:
            with torch.no_grad():
                eps_h, eps_x = mg.gvp_composed(ref.double().eval(), kw, o64, t.double(), edges)
        finally:
            torch.set_default_dtype(torch.float32)
        out[f'{tag}_seed'] = seed
        out[f'{tag}_eps_h'] = eps_h.numpy()
        out[f'{tag}_eps_x'] = eps_x.numpy()
        for et in ('ll', 'kl'):
            out[f'{tag}_{et}_src'] = edges[et][0].numpy()
            out[f'{tag}_{et}_dst'] = edges[et][1].numpy()
    path = os.path.join(HERE, 'gvp_wide.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB')


if __name__ == '__main__':
    main()
