#!/usr/bin/env python
"""Generate tests/golden/dist_hinge.npz: upstream's own DistanceHingeLoss (losses/dist_hinge_loss.py, plain torch) evaluated in
float64 under autograd, the fixture of tests/test_dist_hinge_gpu.py.

Run in the build container only (it imports the reference file, which never travels to the GPU box):
    python tests/golden/make_hinge_golden.py
Inputs are drawn in float32 and stored as float32 (the GPU test feeds exactly these values); the loss and both gradients are
computed from them in float64.  Cases: cross mode (pos_a vs pos_b) and self mode (pos_b = None), sizes from 1 x 1 to 60 x 661 and
5 000 points, empty sides, and the two edge cases that fix the subgradients: d == thr (torch.max splits the gradient, 0.5 each
way) and d == 0 (the pair adds thr to the loss, torch.cdist gives it no gradient).  Edge cases are kept at <= 25 rows, where
torch.cdist computes the exact difference form (larger sets go through |a|^2 + |b|^2 - 2ab, which cannot hit d == 0 or d == thr)."""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference/losses/dist_hinge_loss.py'


def _upstream():
    spec = importlib.util.spec_from_file_location('ref_dist_hinge_loss', REF)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.DistanceHingeLoss


def _cloud(gen, n, side):
    return (torch.rand(n, 3, generator=gen) * side).float()


def main():
    DistanceHingeLoss = _upstream()
    gen = torch.Generator().manual_seed(2026)
    cases = []          # (name, a fp32, b fp32 or None, thr)
    cases.append(('cross_1x1', torch.tensor([[0.3, -0.2, 0.1]]), torch.tensor([[1.1, 0.4, -0.5]]), 3.0))
    cases.append(('cross_7x13', _cloud(gen, 7, 4.0), _cloud(gen, 13, 4.0), 2.5))
    cases.append(('cross_25x300', _cloud(gen, 25, 6.0) + 5.0, _cloud(gen, 300, 16.0), 4.0))
    cases.append(('cross_60x661', _cloud(gen, 60, 8.0) + 6.0, _cloud(gen, 661, 20.0), 3.5))
    cases.append(('cross_0x10', torch.zeros(0, 3), _cloud(gen, 10, 3.0), 2.0))
    cases.append(('cross_10x0', _cloud(gen, 10, 3.0), torch.zeros(0, 3), 2.0))
    cases.append(('cross_tie', torch.tensor([[0.0, 0.0, 0.0]]), torch.tensor([[2.0, 0.0, 0.0]]), 2.0))
    b = _cloud(gen, 9, 3.0)
    a = torch.cat([b[2:3], _cloud(gen, 4, 3.0), b[7:8]])             # rows 0 and 5 coincide with receptor points: d == 0
    cases.append(('cross_zero', a, b, 1.5))
    cases.append(('self_1', _cloud(gen, 1, 2.0), None, 2.0))
    cases.append(('self_0', torch.zeros(0, 3), None, 2.0))
    cases.append(('self_40', _cloud(gen, 40, 6.0), None, 2.0))
    cases.append(('self_tie', torch.tensor([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 0.0, 5.0]]), None, 2.0))
    s = _cloud(gen, 6, 3.0)
    cases.append(('self_zero', torch.cat([s, s[1:2]]), None, 1.5))   # rows 1 and 6 coincide: d == 0
    cases.append(('self_5000', _cloud(gen, 5000, 40.0), None, 2.0))

    out = {'names': np.array([c[0] for c in cases])}
    for name, a, b, thr in cases:
        a64 = a.double().requires_grad_(True)
        b64 = None if b is None else b.double().requires_grad_(True)
        loss = DistanceHingeLoss(thr)(a64, b64)
        ins = [a64] + ([] if b64 is None else [b64])
        grads = torch.autograd.grad(loss, ins, allow_unused=True) if loss.requires_grad else [None] * len(ins)
        grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, ins)]
        out[f'{name}/a'] = a.numpy()
        out[f'{name}/thr'] = np.float64(thr)
        out[f'{name}/loss'] = np.float64(loss.detach())
        out[f'{name}/ga'] = grads[0].numpy()
        if b is not None:
            out[f'{name}/b'] = b.numpy()
            out[f'{name}/gb'] = grads[1].numpy()
        print(f'{name}: loss {float(loss.detach()):.6f}')
    np.savez_compressed(os.path.join(HERE, 'dist_hinge.npz'), **out)


if __name__ == '__main__':
    main()
