"""CPU side of the inference widths below 256: the three train-then-sample models of test_infer_widths_gpu.py build from a config
through model_from_config with upstream's parameter shapes (no GPU needed)."""
import os

import yaml

from keypoint_diffusion_amd.model_setup import model_from_config

CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'configs', 'egnn_all_atom_like.yml')


def _build(architecture, over):
    cfg = yaml.safe_load(open(CFG))
    cfg['diffusion']['architecture'] = architecture
    cfg['diffusion']['rec_encoder_type'] = 'learned'
    cfg['rec_encoder']['k_closest'] = 5                 # the learned EGNN encoder needs one of k_closest / kp_rad
    for (sec, key), v in over.items():
        cfg[sec][key] = v
    return model_from_config(cfg, require_dataset_dir=False)


def _shapes(module):
    return {k: tuple(v.shape) for k, v in module.state_dict().items()}


def test_gvp_learned_encoder_out_scalar_size_64():
    m = _build('gvp', {('rec_encoder_gvp', 'out_scalar_size'): 64})
    s = _shapes(m.rec_encoder)
    assert s['scalar_embed.0.weight'] == (64, 10) and s['scalar_embed.2.weight'] == (64, 64) and s['scalar_norm.weight'] == (64,)
    assert s['keypoint_initializer.src_net.weight'] == (64, 64) and s['keypoint_initializer.dst_net.weight'] == (64, 64)
    assert s['keypoint_initializer.keypoint_embedding.0.weight'] == (64 * 20, 64)          # (k d): 20 keypoints of 64
    assert s['keypoint_initializer.keypoint_embedding.2.weight'] == (64 * 20,)
    assert m.dynamics.n_kp_scalars == 64
    assert _shapes(m.dynamics)['kp_encoder.0.weight'][1] == 65          # n_kp_scalars + the timestep


def test_egnn_learned_encoder_out_n_node_feat_192():
    m = _build('egnn', {('rec_encoder', 'out_n_node_feat'): 192})
    s = _shapes(m.dynamics)
    H = m.dynamics.hidden_nf
    assert m.dynamics.rec_nf == 192 and H == 256
    assert s['rec_encoder.0.weight'] == (384, 192) and s['rec_encoder.2.weight'] == (H, 384)


def test_egnn_identity_keypoint_encoder_at_hidden_nf_100():
    m = _build('egnn', {('rec_encoder', 'out_n_node_feat'): 100, ('dynamics', 'hidden_nf'): 100})
    s = _shapes(m.dynamics)
    assert m.dynamics.rec_nf == m.dynamics.hidden_nf == 100
    assert not any(k.startswith('rec_encoder.') for k in s)               # nn.Identity: no parameters
    assert s['lig_encoder.2.weight'] == (100, 64) and s['egnn.conv_layers.0.node_mlp.lig.0.weight'] == (101, 202)
