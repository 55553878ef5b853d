#!/usr/bin/env python
"""Generate tests/golden/egnn_wide.npz: upstream's own LigRecDynamics sub-modules (LigRecConv's edge / coordinate / attention / node
MLPs and LayerNorms, the encoders and the decoder) composed as in models/dynamics.py:342-385 (make_golden.py::egnn_composed), at
hidden_nf 257 and 512, 2 layers, update_kp_feat on and off, on a ragged 3-complex batch -- the fixture of
tests/test_egnn_wide_gpu.py::test_upstream_fixture_parity.

Run in the build container only (it imports the reference, which never travels to the GPU box):
    python tests/golden/make_egnn_wide_golden.py
No weights are stored: each case stores the seed from which synth.fill_state_dict_ rebuilds them (upstream's state-dict layout equals
this library's, checked here).  The reference runs in float64 on the float32 inputs; inputs, edge lists and outputs are stored."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden import make_golden as mg                                  # noqa: E402  (imports the reference modules)

CASES = [('h257_kp', 257, True, 31), ('h257_nokp', 257, False, 32), ('h512_kp', 512, True, 33), ('h512_nokp', 512, False, 34)]
N_REC, N_LIG, BATCH_SEED = [70, 23, 41], [12, 3, 8], 7


def main():
    g, ob = mg.small_batch(N_REC, N_LIG, seed=BATCH_SEED)
    t = torch.linspace(0.2, 0.9, len(N_REC))
    out = dict(n_rec=np.array(N_REC), n_lig=np.array(N_LIG), batch_seed=BATCH_SEED, t=t.numpy(),
               lig_x=ob.x['lig'].numpy(), lig_h=ob.h['lig'].numpy(), kp_x=ob.x['kp'].numpy(), kp_h=ob.h['kp'].numpy(),
               kk_src=ob.edges['kk'][0].numpy(), kk_dst=ob.edges['kk'][1].numpy(), names=np.array([c[0] for c in CASES]))
    for tag, H, upd, seed in CASES:
        cfg = dict(mg.util.EGNN_C2, hidden_nf=H, n_layers=2, update_kp_feat=upd)
        kw = dict(cfg, graph_cutoffs=mg.CUT)
        ref, mine = mg.RefEGNN(10, 10, **kw), mg.LigRecDynamics(10, 10, **kw)
        a = {k: list(v.shape) for k, v in ref.state_dict().items()}
        b = {k: list(v.shape) for k, v in mine.state_dict().items()}
        assert a == b, f'{tag}: state-dict layout differs: {set(a) ^ set(b)}'
        mg.synth.fill_state_dict_(ref, seed)
        edges = mg.oegnn.lig_edges(ob, kw)
        edges['kk'] = ob.edges['kk']
        o64 = type(ob)(n=ob.n, x={k: v.double() for k, v in ob.x.items()}, h={k: v.double() for k, v in ob.h.items()}, v={},
                       edges=ob.edges)
        with torch.no_grad():
            eps_h, eps_x = mg.egnn_composed(ref.double().eval(), kw, o64, t.double(), edges)
        out[f'{tag}_seed'] = seed
        out[f'{tag}_eps_h'] = eps_h.numpy()
        out[f'{tag}_eps_x'] = eps_x.numpy()
        for et in ('ll', 'kl'):
            out[f'{tag}_{et}_src'] = edges[et][0].numpy()
            out[f'{tag}_{et}_dst'] = edges[et][1].numpy()
    path = os.path.join(HERE, 'egnn_wide.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB')


if __name__ == '__main__':
    main()
