"""CPU side of the receptor-ligand hinge term: a config with rl_dist_threshold > 0 builds the model (upstream train.py:37, 217-218
sets diffusion.rl_dist_threshold), and the hinge refuses CPU tensors instead of computing without the GPU kernel."""
import os

import pytest
import torch
import yaml

from keypoint_diffusion_amd import hip
from keypoint_diffusion_amd.dist_hinge_loss import DistanceHingeLoss, segmented_dist_hinge
from keypoint_diffusion_amd.model_setup import model_from_config

CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'configs', 'egnn_all_atom_like.yml')


def test_config_with_rl_dist_threshold_builds_the_model(tmp_path):
    cfg = yaml.safe_load(open(CFG))
    cfg['diffusion']['rl_dist_threshold'] = 2.0
    f = tmp_path / 'config.yml'
    f.write_text(yaml.safe_dump(cfg))
    m = model_from_config(yaml.safe_load(f.read_text()), require_dataset_dir=False)
    assert m.rl_dist_threshold == 2.0
    assert len(m.state_dict()) == 349                      # the term has no parameters of its own
    cfg['diffusion']['architecture'], cfg['diffusion']['rec_encoder_type'] = 'gvp', 'learned'
    assert model_from_config(cfg, require_dataset_dir=False).rl_dist_threshold == 2.0


def test_hinge_has_no_cpu_path():
    a, b = torch.zeros(4, 3, requires_grad=True), torch.ones(5, 3)
    with pytest.raises((hip.KpdError, RuntimeError)):
        DistanceHingeLoss(2.0)(a, b)
    with pytest.raises((hip.KpdError, RuntimeError)):
        DistanceHingeLoss(2.0)(a)
    ptr = torch.tensor([0, 4], dtype=torch.int32)
    with pytest.raises((hip.KpdError, RuntimeError)):
        segmented_dist_hinge(a, ptr, b, torch.tensor([0, 5], dtype=torch.int32), 2.0)
