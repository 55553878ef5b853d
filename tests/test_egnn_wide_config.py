"""CPU side of the wide EGNN denoiser: a config with dynamics.hidden_nf = 512 builds the model with upstream's parameter shapes, and
hidden_nf = 1025 is refused when the model is constructed (no GPU needed)."""
import os

import pytest
import yaml

from keypoint_diffusion_amd.model_setup import model_from_config

CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'configs', 'egnn_all_atom_like.yml')


def _upstream_shapes(H, atom_nf, rec_nf, n_layers, update_kp):
    """models/dynamics.py: LigRecDynamics.__init__ (:300-340) and LigRecConv (:9-87) with in = hidden = out = H + 1."""
    W = H + 1
    s = {'lig_encoder.0.weight': (64, atom_nf), 'lig_encoder.0.bias': (64,), 'lig_encoder.2.weight': (H, 64), 'lig_encoder.2.bias': (H,),
         'lig_decoder.0.weight': (2 * atom_nf, H), 'lig_decoder.0.bias': (2 * atom_nf,),
         'lig_decoder.2.weight': (atom_nf, 2 * atom_nf), 'lig_decoder.2.bias': (atom_nf,)}
    if rec_nf != H:
        s.update({'rec_encoder.0.weight': (2 * rec_nf, rec_nf), 'rec_encoder.0.bias': (2 * rec_nf,),
                  'rec_encoder.2.weight': (H, 2 * rec_nf), 'rec_encoder.2.bias': (H,)})
    ets = ['ll', 'kl', 'lk', 'kk'] if update_kp else ['ll', 'kl']
    nts = ['lig', 'kp'] if update_kp else ['lig']
    for i in range(n_layers):
        p = f'egnn.conv_layers.{i}.'
        for et in ets:
            for blk in ('edge_mlp', 'coord_mlp'):
                s.update({f'{p}{blk}.{et}.0.weight': (W, 2 * W + 1), f'{p}{blk}.{et}.0.bias': (W,),
                          f'{p}{blk}.{et}.2.weight': (W, W), f'{p}{blk}.{et}.2.bias': (W,)})
            s[f'{p}coord_mlp.{et}.4.weight'] = (1, W)
            s.update({f'{p}soft_attention.{et}.0.weight': (1, W), f'{p}soft_attention.{et}.0.bias': (1,)})
        for nt in nts:
            s.update({f'{p}node_mlp.{nt}.0.weight': (W, 2 * W), f'{p}node_mlp.{nt}.0.bias': (W,),
                      f'{p}node_mlp.{nt}.2.weight': (W, W), f'{p}node_mlp.{nt}.2.bias': (W,)})
    return s


def test_hidden_nf_512_builds_with_upstream_shapes():
    cfg = yaml.safe_load(open(CFG))
    cfg['dynamics']['hidden_nf'] = 512
    m = model_from_config(cfg, require_dataset_dir=False)
    dyn = m.dynamics
    assert dyn.hidden_nf == 512
    got = {k: tuple(v.shape) for k, v in dyn.state_dict().items()}
    want = _upstream_shapes(512, dyn.atom_nf, dyn.rec_nf, dyn.n_layers, dyn.update_kp_feat)
    if dyn.norm:
        for i in range(dyn.n_layers):
            for nt in (['lig', 'kp'] if dyn.update_kp_feat else ['lig']):
                want[f'egnn.conv_layers.{i}.layer_norm.{nt}.weight'] = (513,)
                want[f'egnn.conv_layers.{i}.layer_norm.{nt}.bias'] = (513,)
    assert got == want


def test_hidden_nf_1025_is_refused():
    cfg = yaml.safe_load(open(CFG))
    cfg['dynamics']['hidden_nf'] = 1025
    with pytest.raises(ValueError, match='1 .. 1024'):
        model_from_config(cfg, require_dataset_dir=False)
