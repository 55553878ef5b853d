"""`KeypointDiffusion`: the diffusion wrapper around the denoiser, with the reference's public
surface (models/ligand_diffuser.py:24-538) on the HIP hot path.

Host code (this file) is tensor plumbing and the noise schedule; every per-timestep tensor
operation -- denoiser forward, z_s update, COM removal -- is a call into libkpd_hip.so.
`LigandDiffuser` is kept as an alias (BASELINE.json names the class that way).
"""
import pickle
from math import ceil
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import graph as G
from . import hip
from .dynamics import LigRecDynamics
from .dist_hinge_loss import segmented_dist_hinge
from .dynamics_gvp import LigRecDynamicsGVP
from .receptor_encoder_fixed import FixedReceptorEncoder
from .receptor_encoder import ReceptorEncoder
from .receptor_encoder_gvp import ReceptorEncoderGVP
from .rec_encoder_loss import ReceptorEncoderLoss


class LigandSizeDistribution:
    """P(n_lig | n_rec) from the shipped joint histogram (models/n_nodes_dist.py:7-59)."""

    def __init__(self, processed_dataset_dir: Path):
        f = Path(processed_dataset_dir) / 'train_n_node_joint_dist.pkl'
        if not f.exists():
            raise ValueError(f'Joint distribution file {f} does not exist')
        with open(f, 'rb') as fh:
            hist, self.rec_bounds, self.lig_bounds = pickle.load(fh)
        self.joint_histogram = torch.from_numpy(hist)
        self.rec_idx_to_size = torch.arange(self.rec_bounds[0], self.rec_bounds[1] + 1)
        self.lig_idx_to_size = torch.arange(self.lig_bounds[0], self.lig_bounds[1] + 1)

    def sample(self, n_nodes_rec: torch.Tensor, n_replicates: int) -> torch.Tensor:
        lo, hi = self.rec_bounds
        clipped = n_nodes_rec.clamp(min=lo, max=hi)
        for a, b in zip(n_nodes_rec.tolist(), clipped.tolist()):
            if a != b:
                print(f'WARNING: Number of receptor nodes {a} is not in the range {self.rec_bounds} from the '
                      f'training set; conditioning on {b} nodes')
        rows = self.joint_histogram[(clipped - lo).long()]
        idx = torch.multinomial(rows, n_replicates, replacement=True)
        return self.lig_idx_to_size[idx]


def polynomial_schedule(timesteps: int, s: float = 1e-4, power: float = 3.0) -> np.ndarray:
    """alpha^2 of the clipped polynomial schedule (ligand_diffuser.py:620-650)."""
    steps = timesteps + 1
    t = np.linspace(0, steps, steps)
    a2 = np.concatenate([np.ones(1), (1 - np.power(t / steps, power)) ** 2])
    a2 = np.cumprod(np.clip(a2[1:] / a2[:-1], a_min=0.001, a_max=1.0))
    return (1 - 2 * s) * a2 + s


class PredefinedNoiseSchedule(nn.Module):
    """Lookup table gamma[0..T] = -(log alpha^2 - log sigma^2) (ligand_diffuser.py:654-690)."""

    def __init__(self, noise_schedule: str, timesteps: int, precision: float):
        super().__init__()
        self.timesteps = timesteps
        if not noise_schedule.startswith('polynomial_'):
            raise ValueError(noise_schedule)
        a2 = polynomial_schedule(timesteps, s=precision, power=float(noise_schedule.split('_')[1]))
        gamma = -(np.log(a2) - np.log(1 - a2))
        self.gamma = nn.Parameter(torch.from_numpy(gamma).float(), requires_grad=False)

    def forward(self, t: torch.Tensor) -> torch.Tensor:
        return self.gamma[torch.round(t * self.timesteps).long()]


class InpaintContext:
    """What an inpainting step needs besides the state (include/kpd.h, "Inpainting"): `fixed` [n_lig] bool / uint8 (1 = this atom
    is given), `x` [n_lig,3] known positions in the input (receptor) frame, `h` [n_lig,atom_nf] known features already divided
    by `lig_feat_norm_constant` (both read on the fixed rows only), `kp_com0` [B,3] keypoint mean in the input frame."""

    def __init__(self, fixed: torch.Tensor, x: torch.Tensor, h: torch.Tensor, kp_com0: torch.Tensor):
        if not (isinstance(fixed, torch.Tensor) and fixed.dtype in (torch.bool, torch.uint8) and fixed.dim() == 1):
            raise ValueError(f'fixed must be a 1-D bool or uint8 tensor with one entry per ligand atom (got '
                             f'{getattr(fixed, "dtype", type(fixed))} {tuple(getattr(fixed, "shape", ()))})')
        if x.shape != (fixed.shape[0], 3) or h.dim() != 2 or h.shape[0] != fixed.shape[0] or kp_com0.dim() != 2 or kp_com0.shape[1] != 3:
            raise ValueError(f'inpaint: x {tuple(x.shape)}, h {tuple(h.shape)}, kp_com0 {tuple(kp_com0.shape)} do not fit '
                             f'{fixed.shape[0]} ligand atoms')
        self.fixed = (fixed.view(torch.uint8) if fixed.dtype == torch.bool else fixed).contiguous()
        self.x, self.h, self.kp_com0 = x.float().contiguous(), h.float().contiguous(), kp_com0.float().contiguous()


class ClashGuidance:
    """Clash guidance as the caller asks for it (include/kpd.h, "Clash guidance"): push the denoised ligand positions out of the
    `threshold` Angstrom spheres around the wall atoms at every reverse step with t <= `t_max`, `scale` = 1 moving a single contact
    exactly onto its sphere.  `wall`: None, or the atoms to stay away from in the form the entry point documents -- one [m_i,3]
    tensor per pocket for `_sample` and its callers (None: each pocket's receptor atoms as given), `(wall_x [n_wall,3],
    wall_ptr [B+1])` for `sample_from_encoded_receptors` / `inpaint_from_encoded_receptors` (None: the `rec` rows of the batch when
    it has any, else its keypoints).  A C-alpha model sees one atom per residue: hand it the full-atom pocket explicitly."""

    def __init__(self, threshold: float, scale: float = 1.0, t_max: float = 1.0, wall=None):
        for name, v in (('threshold', threshold), ('scale', scale), ('t_max', t_max)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v in (float('inf'), float('-inf')):
                raise ValueError(f'{name} must be a finite number (got {v!r})')
        if not threshold > 0:
            raise ValueError(f'threshold must be positive, in Angstrom (got {threshold!r})')
        if not scale >= 0:
            raise ValueError(f'scale must be >= 0 (got {scale!r})')
        if not 0 < t_max <= 1:
            raise ValueError(f't_max must lie in (0, 1] (got {t_max!r})')
        self.threshold, self.scale, self.t_max, self.wall = float(threshold), float(scale), float(t_max), wall

    def with_wall(self, wall) -> 'ClashGuidance':
        return ClashGuidance(self.threshold, self.scale, self.t_max, wall)


class GuidanceContext:
    """What a guided step needs besides the state: `wall_x` [n_wall,3] in the input (receptor) frame, `wall_ptr` [B+1] offsets
    per complex (0 first, ascending, n_wall last: read once here, the kernel trusts it), `kp_com0` [B,3] keypoint mean in the
    input frame, and the numbers of a `ClashGuidance`."""

    def __init__(self, wall_x: torch.Tensor, wall_ptr: torch.Tensor, kp_com0: torch.Tensor, threshold: float, scale: float = 1.0,
                 t_max: float = 1.0):
        c = ClashGuidance(threshold, scale, t_max)
        self.threshold, self.scale, self.t_max = c.threshold, c.scale, c.t_max
        if not (isinstance(kp_com0, torch.Tensor) and kp_com0.dim() == 2 and kp_com0.shape[1] == 3):
            raise ValueError(f'guidance: kp_com0 must be [B, 3] (got {tuple(getattr(kp_com0, "shape", ()))})')
        hip.check_wall(wall_x, wall_ptr, kp_com0.shape[0], 'guidance')
        self.wall_x, self.wall_ptr = wall_x.float().contiguous(), wall_ptr.int().contiguous()
        self.kp_com0 = kp_com0.float().contiguous()


class StepGraph:
    """A captured reverse step.  `step(s, t)` writes the two scalars into static device buffers and replays the graph;
    the graph holds the denoiser forward (graph build included), the noise draw and the in-place z_s update."""

    def __init__(self, model: 'KeypointDiffusion', g, bidx=None, noise=None, inpaint=None, guidance=None):
        dev, B = g.device, g.batch_size
        if dev.type != 'cuda':
            raise hip.KpdError('a step graph needs the batch on the GPU')
        self.s, self.t = torch.zeros(B, device=dev), torch.ones(B, device=dev)
        lig, kp = g.nodes['lig'].data, g.nodes['kp'].data
        state = [lig['x_0'], lig['h_0'], kp['x_0']]
        for i, t in enumerate(state):
            if not (t.is_contiguous() and t.dtype == torch.float32):
                raise hip.KpdError('graph capture needs contiguous fp32 state tensors (they are updated in place)')
        saved = [t.clone() for t in state]
        T = model.n_timesteps
        self.s.fill_((T - 1) / T)
        kw = {} if inpaint is None else {'inpaint': inpaint}          # the plain step is called exactly as before
        if guidance is not None:
            kw['guidance'] = guidance
        # warm-up outside capture (workspace reservation, first-use initialisation), on a side stream as capture requires
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(2):
                model.sample_p_zs_given_zt(self.s, self.t, g, bidx, noise=noise, **kw)
        torch.cuda.current_stream(dev).wait_stream(side)
        for t, c in zip(state, saved):
            t.copy_(c)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            model.sample_p_zs_given_zt(self.s, self.t, g, bidx, noise=noise, **kw)
        self._keep = (g, noise, inpaint, guidance)
        # The captured kernels hold raw pointers into the engine's workspace arena and packed weights.  Holding the engine
        # object keeps both allocations alive even if the module builds a new engine; the pin records what must not have
        # changed for a replay to mean "one reverse step of this model": the arena (a larger batch re-reserves it, which
        # frees the captured one) and the weights the engine was packed from.
        self._model = model
        self._engine = model.dynamics.engine()
        self._pin = (self._engine._reserved, model.dynamics._weights_key())
        ps = list(model.dynamics.parameters())
        self._sentinels = [ps[i] for i in sorted({0, len(ps) // 2, len(ps) - 1})] if ps else []
        self._sentinel_key = [(p.data_ptr(), p._version) for p in self._sentinels]

    def _check_pin(self):
        """Every replay: the engine object and its arena are the captured ones (two attribute reads) and three sentinel parameters
        (first, middle, last) still have the captured storage and version counter -- whatever rewrites the weights as a whole
        (an optimizer step, load_state_dict, an EMA swap, .to()) moves every one of them, so such a change raises on the NEXT
        replay, not up to 15 replays later.  Every 16th replay, starting with the first: all weights are the captured ones (a walk
        over all parameters -- host time the graph exists to avoid), which also catches a change to a single tensor."""
        dyn = self._model.dynamics
        self._replays = getattr(self, '_replays', -1) + 1
        if dyn._engine is not self._engine or self._engine._reserved != self._pin[0]:
            raise hip.KpdError('stale step graph: the denoiser engine was rebuilt or its workspace re-reserved (a larger batch ran) '
                               'after capture; the captured kernels point into freed memory -- capture the step again')
        if ([(p.data_ptr(), p._version) for p in self._sentinels] != self._sentinel_key or
                (self._replays % 16 == 0 and dyn._weights_key() != self._pin[1])):
            raise hip.KpdError('stale step graph: the model weights changed after capture (the graph replays the weights packed at '
                               'capture time) -- capture the step again')

    def step(self, s: float, t: float):
        self._check_pin()
        self.s.fill_(s)
        self.t.fill_(t)
        self.graph.replay()


class KeypointDiffusion(nn.Module):

    def __init__(self, atom_nf, rec_nf, processed_dataset_dir: Optional[Path], n_timesteps: int = 1000,
                 keypoint_centered=False, architecture: str = 'egnn', rec_encoder_type: str = 'learned',
                 graph_config={}, dynamics_config={}, rec_encoder_config={}, rec_encoder_loss_config={},
                 precision=1e-4, lig_feat_norm_constant=1, rl_dist_threshold=0, use_fake_atoms=False):
        super().__init__()
        if architecture not in ('egnn', 'gvp'):
            raise ValueError(f'Unsupported architecture: {architecture}')
        if rec_encoder_type not in ('learned', 'fixed'):
            raise ValueError(f'Receptor encoder type must be either "learned" or "fixed". Got {rec_encoder_type=} instead.')
        self.n_lig_features, self.n_kp_feat, self.n_timesteps = atom_nf, rec_nf, n_timesteps
        self.lig_feat_norm_constant = lig_feat_norm_constant
        self.use_fake_atoms, self.rec_encoder_type, self.architecture = use_fake_atoms, rec_encoder_type, architecture
        self.rl_dist_threshold = rl_dist_threshold
        if use_fake_atoms:
            raise NotImplementedError('fake atoms are unused by every shipped config (max_fake_atom_frac: 0.0) and '
                                      'the reference implementation of their removal cannot run (ligand_diffuser.py:559)')
        # the ligand-size prior is host-side and optional here: synthetic benches have no dataset directory
        self.lig_size_dist = LigandSizeDistribution(processed_dataset_dir) if processed_dataset_dir is not None else None
        self.gamma = PredefinedNoiseSchedule('polynomial_2', timesteps=n_timesteps, precision=precision)

        dynamics_config = dict(dynamics_config)
        if 'no_cg' in rec_encoder_config:
            dynamics_config['no_cg'] = rec_encoder_config['no_cg']
        dyn_cls = LigRecDynamics if architecture == 'egnn' else LigRecDynamicsGVP
        self.dynamics = dyn_cls(atom_nf, rec_nf, **graph_config, **dynamics_config)

        if rec_encoder_type == 'learned':
            enc_cls = ReceptorEncoder if architecture == 'egnn' else ReceptorEncoderGVP      # ligand_diffuser.py:62-67
            self.rec_encoder = enc_cls(**graph_config, **rec_encoder_config)
        else:
            self.rec_encoder = FixedReceptorEncoder(
                n_vec_feats=rec_encoder_config['vector_size'] if architecture == 'gvp' else None)
        rec_encoder_loss_config = dict(rec_encoder_loss_config)
        if rec_encoder_type == 'fixed':
            rec_encoder_loss_config['loss_type'] = 'none'                                      # ligand_diffuser.py:85-87
        self.rec_encoder_loss_fn = ReceptorEncoderLoss(**rec_encoder_loss_config)

    # ---- training entry point ----------------------------------------------------------
    def forward(self, complex_graphs, interface_points):
        """Losses of one batch (ligand_diffuser.py:89-175): {'l2', 'pos', 'feat', 'rec_encoder'}, and 'rl_hinge' when
        rl_dist_threshold > 0 (the receptor-ligand clash penalty of :137-156, `_rl_hinge`; a training loop adds it with its
        weight, train.py:340-341).

        Trainable end to end in all eight shipped configurations and dev_config: the noise prediction is differentiated by the HIP
        backward passes of the denoisers (kpd_egnn_trainer_* / kpd_gvp_trainer_*, with respect to the keypoint positions, features
        and vectors too), the learned keypoints by the backward passes of their encoder (kpd_recenc_trainer_* for gvp_20kp /
        gvp_40kp, kpd_recegnn_trainer_* for egnn_20kp / egnn_40kp), and the optimal-transport encoder loss (rec_encoder_loss.py)
        adds its gradient at the keypoint positions.  With a fixed encoder there are no encoder parameters and that loss is the
        constant 0 (:85-87)."""
        losses = {}
        g = self.normalize(complex_graphs)
        batch_size, device = g.batch_size, g.device
        batch_idxs = G.get_batch_idxs(g)
        g = self.rec_encoder(g, batch_idxs)
        if self.rec_encoder_type == 'fixed':
            batch_idxs = G.get_batch_idxs(g)                  # :106-107: keypoints = receptor atoms now
        apply_rl_hinge = self.rl_dist_threshold > 0
        if apply_rl_hinge:
            init_kp_com = self._kp_mean(g, batch_idxs['kp'])  # :111-112, before any COM removal
        # :115; the exact transport plans are solved on host threads while the denoiser's forward is launched below
        losses['rec_encoder'] = None
        pending = self.rec_encoder_loss_fn.begin(g, interface_points=interface_points)
        try:
            g = self.remove_com(g, batch_idxs['lig'], batch_idxs['kp'], com='ligand')
            t = torch.randint(0, self.n_timesteps, size=(batch_size,), device=device).float() / self.n_timesteps
            eps = {'h': torch.randn(g.nodes['lig'].data['h_0'].shape, device=device),
                   'x': torch.randn(g.nodes['lig'].data['x_0'].shape, device=device)}
            gamma_t = self.gamma(t).to(device=device)
            g = self.noised_representation(g, batch_idxs['lig'], batch_idxs['kp'], eps, gamma_t)
            eps_h_pred, eps_x_pred = self.dynamics(g, t, batch_idxs)
        except BaseException:
            pending.abandon()                # the denoiser raised: do not leave the solver thread running behind the exception
            raise
        losses['rec_encoder'] = pending.finish()
        if apply_rl_hinge:
            losses['rl_hinge'] = self._rl_hinge(g, batch_idxs, eps_x_pred, gamma_t, init_kp_com)
        x_loss = (eps['x'] - eps_x_pred).square().sum()
        n_x_loss_terms = eps['x'].numel()
        h_loss = (eps['h'] - eps_h_pred).square().sum()
        losses['l2'] = (x_loss + h_loss) / (n_x_loss_terms + eps['h'].numel())
        losses['pos'] = x_loss / n_x_loss_terms
        losses['feat'] = h_loss / eps['h'].numel()
        return losses

    def noised_representation(self, g, lig_batch_idx, kp_batch_idx, eps, gamma_t):
        """z_t = alpha_t z_0 + sigma_t eps, then ligand-COM removal (ligand_diffuser.py:205-219)."""
        alpha_t = self.alpha(gamma_t)[lig_batch_idx][:, None]
        sigma_t = self.sigma(gamma_t)[lig_batch_idx][:, None]
        g.nodes['lig'].data['x_0'] = alpha_t * g.nodes['lig'].data['x_0'] + sigma_t * eps['x']
        g.nodes['lig'].data['h_0'] = alpha_t * g.nodes['lig'].data['h_0'] + sigma_t * eps['h']
        return self.remove_com(g, lig_batch_idx, kp_batch_idx, com='ligand')

    def _kp_mean(self, g, kp_batch_idx):
        """Per-complex mean keypoint position [B,3] (dgl.readout_nodes(..., 'kp', 'mean') without reading the counts back to the host).
        Detached: the hinge term's keypoint dependence cancels exactly (see `_rl_hinge`)."""
        x = g.nodes['kp'].data['x_0'].detach()
        s = torch.zeros(g.batch_size, 3, dtype=x.dtype, device=x.device).index_add_(0, kp_batch_idx, x)
        return s / g.batch_num_nodes('kp').clamp(min=1).to(x.dtype)[:, None]

    def _rl_hinge(self, g, batch_idxs, eps_x_pred, gamma_t, init_kp_com):
        """sum_b sum_{i,j} max(thr - ||x_hat_i - r_j||, 0) over the ligand atoms i and receptor atoms j of every complex
        (ligand_diffuser.py:137-156), as one segmented kernel launch (kpd_dist_hinge) instead of a loop over dgl.unbatch.
        x_hat = (z - sigma_t eps_x_pred) / alpha_t is the denoised ligand (denoised_representation, :221-230), moved back into the
        receptor's frame the way upstream does it: minus the current keypoint mean, plus the keypoint mean before COM removal.  Both
        means are shifts by the ligand COMs removed before and after noising, so the term reaches the parameters only through
        eps_x_pred; the keypoint means are detached (their autograd contributions cancel exactly upstream too).  The graph is not
        modified.  With a fixed encoder the receptor nodes are gone (receptor_encoder_fixed.py) and the term is a differentiable 0."""
        lig_b, kp_b = batch_idxs['lig'], batch_idxs['kp']
        alpha_t = self.alpha(gamma_t)[lig_b][:, None]
        sigma_t = self.sigma(gamma_t)[lig_b][:, None]
        x_hat = (g.nodes['lig'].data['x_0'] - sigma_t * eps_x_pred) / alpha_t
        x_hat = x_hat - self._kp_mean(g, kp_b)[lig_b] + init_kp_com[lig_b]
        rec_x = g.nodes['rec'].data.get('x_0')
        if rec_x is None:
            rec_x = torch.zeros(0, 3, device=x_hat.device)
        total, _ = segmented_dist_hinge(x_hat.float().contiguous(), g.node_ptr('lig').int(), rec_x.detach().float().contiguous(),
                                        g.node_ptr('rec').int(), self.rl_dist_threshold)
        return total

    def denoised_representation(self, g, lig_batch_idx, kp_batch_idx, eps_x_pred, eps_h_pred, gamma_t):
        """ligand_diffuser.py:221-230."""
        alpha_t = self.alpha(gamma_t)[lig_batch_idx][:, None]
        sigma_t = self.sigma(gamma_t)[lig_batch_idx][:, None]
        g.nodes['lig'].data['x_0'] = (g.nodes['lig'].data['x_0'] - sigma_t * eps_x_pred) / alpha_t
        g.nodes['lig'].data['h_0'] = (g.nodes['lig'].data['h_0'] - sigma_t * eps_h_pred) / alpha_t
        return g

    # ---- small host helpers ------------------------------------------------------------
    def normalize(self, g):
        g.nodes['lig'].data['h_0'] = g.nodes['lig'].data['h_0'] / self.lig_feat_norm_constant
        return g

    def unnormalize(self, g):
        g.nodes['lig'].data['h_0'] = g.nodes['lig'].data['h_0'] * self.lig_feat_norm_constant
        return g

    def remove_com(self, g, lig_batch_idx, kp_batch_idx, com: str = None, ordered: bool = False):
        if com is None:
            raise NotImplementedError('removing COM of receptor/ligand complex not implemented')
        if com not in ('ligand', 'receptor'):
            raise ValueError(f'invalid value for com: {com=}')
        c = G.readout_nodes(g, feat='x_0', ntype='lig' if com == 'ligand' else 'kp', op='mean', ordered=ordered)
        g.nodes['lig'].data['x_0'] = g.nodes['lig'].data['x_0'] - c[lig_batch_idx]
        g.nodes['kp'].data['x_0'] = g.nodes['kp'].data['x_0'] - c[kp_batch_idx]
        return g

    def sigma(self, gamma):
        return torch.sqrt(torch.sigmoid(gamma))

    def alpha(self, gamma):
        return torch.sqrt(torch.sigmoid(-gamma))

    def sigma_and_alpha_t_given_s(self, gamma_t, gamma_s):
        sigma2 = -torch.expm1(F.softplus(gamma_s) - F.softplus(gamma_t))
        log_alpha2 = F.logsigmoid(-gamma_t) - F.logsigmoid(-gamma_s)
        return sigma2, torch.sqrt(sigma2), torch.exp(0.5 * log_alpha2)

    # ---- sampling ----------------------------------------------------------------------
    def encode_receptors(self, g):
        return self.rec_encoder(g, G.get_batch_idxs(g))

    def step_coefficients(self, s: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        """[B,3] = (alpha_t|s, sigma^2_t|s / alpha_t|s / sigma_t, sigma_t|s sigma_s / sigma_t)
        (ligand_diffuser.py:505-526).  On the GPU this is one kernel (kpd_step_coefficients); host tensors take
        the same arithmetic through the torch mirror below (schedule inspection, tests)."""
        if s.is_cuda:
            return hip.step_coefficients(self.gamma.gamma, s, t)
        g_s, g_t = self.gamma(s), self.gamma(t)
        sigma2_ts, sigma_ts, alpha_ts = self.sigma_and_alpha_t_given_s(g_t, g_s)
        sig_s, sig_t = self.sigma(g_s), self.sigma(g_t)
        return torch.stack([alpha_ts, sigma2_ts / alpha_ts / sig_t, sigma_ts * sig_s / sig_t], dim=1).contiguous()

    def inpaint_coefficients(self, s: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        """[B,6] = the three columns of `step_coefficients`, bit for bit, then (alpha_s, sigma_s, sigma_t|s): what an inpainting
        step needs to noise the known part to level s and to move the state back from s to t (include/kpd.h).  One kernel on
        the GPU (kpd_inpaint_coefficients), the torch mirror on host tensors."""
        if s.is_cuda:
            return hip.inpaint_coefficients(self.gamma.gamma, s, t)
        g_s, g_t = self.gamma(s), self.gamma(t)
        _, sigma_ts, _ = self.sigma_and_alpha_t_given_s(g_t, g_s)
        return torch.cat([self.step_coefficients(s, t), torch.stack([self.alpha(g_s), self.sigma(g_s), sigma_ts], dim=1)],
                         dim=1).contiguous()

    def guided_coefficients(self, s: torch.Tensor, t: torch.Tensor, scale: float = 1.0, t_max: float = 1.0) -> torch.Tensor:
        """[B,9] = the six columns of `inpaint_coefficients`, bit for bit, then alpha_t, sigma_t and the guidance weight
        w = scale alpha_s sigma^2_t|s / sigma_t^2 for round(t T) <= round(t_max T), 0 above (include/kpd.h, "Clash guidance").  One
        kernel on the GPU (kpd_guided_coefficients), the torch mirror on host tensors."""
        c = ClashGuidance(1.0, scale, t_max)
        if s.is_cuda:
            return hip.guided_coefficients(self.gamma.gamma, s, t, c.scale, c.t_max)
        g_s, g_t = self.gamma(s), self.gamma(t)
        sigma2_ts, _, _ = self.sigma_and_alpha_t_given_s(g_t, g_s)
        T = self.n_timesteps
        on = torch.round(t * T) <= torch.round(torch.tensor(c.t_max, dtype=t.dtype) * T)
        w = torch.where(on, c.scale * self.alpha(g_s) * sigma2_ts / torch.sigmoid(g_t), torch.zeros_like(g_t))
        return torch.cat([self.inpaint_coefficients(s, t), torch.stack([self.alpha(g_t), self.sigma(g_t), w], dim=1)], dim=1).contiguous()

    def use_complex_noise(self, seed):
        """Opt in to sharding-invariant noise: every draw of the sampler becomes a function of (seed, complex id, timestep,
        position in the complex) (kpd_complex_noise), so a run split over ranks reproduces the single-process run.
        `seed=None` returns to the reference behaviour (one global torch.randn per draw)."""
        self._noise_seed = None if seed is None else int(seed)
        return self

    def _draw(self, g, width, complex_ids, step, tag):
        if getattr(self, '_noise_seed', None) is None or complex_ids is None:
            return torch.randn(g.num_nodes('lig'), width, device=g.device)
        return hip.complex_noise(g.prepared(), width, complex_ids, self._noise_seed, step, tag)

    def sample_p_zs_given_zt(self, s, t, g, batch_idxs=None, noise=None, complex_ids=None, step=0, inpaint=None, repetition=0,
                             guidance=None):
        """One reverse step (ligand_diffuser.py:497-538).  `noise` = (pos_noise, feat_noise) may be
        injected for reproducible parity tests; by default it is drawn with torch.randn as upstream
        (or per complex, `use_complex_noise`, when `complex_ids` [B] int64 and the integer `step` are given).
        `inpaint` (an `InpaintContext`): the step around fixed atoms (kpd_sample_update_inpaint); `noise` may then be the 4-tuple
        (pos_noise, feat_noise, known_pos_noise, known_feat_noise), and `repetition` u selects the tags 6u .. 6u + 3 of the
        per-complex streams.  With `inpaint=None` nothing differs from the plain step.
        `guidance` (a `GuidanceContext`: the prepared wall and `kp_com0`): the step with the clash shift (kpd_sample_update_guided),
        alone or together with `inpaint`; it draws what the step without it draws.  With `guidance=None` nothing differs."""
        lig, kp = g.nodes['lig'].data, g.nodes['kp'].data
        for d, k in ((lig, 'x_0'), (lig, 'h_0'), (kp, 'x_0')):
            if not (d[k].is_contiguous() and d[k].dtype == torch.float32):
                d[k] = d[k].contiguous().float()
        if guidance is not None:
            return self._guided_step(s, t, g, batch_idxs, noise, complex_ids, step, inpaint, repetition, guidance)
        if inpaint is not None:
            return self._inpaint_step(s, t, g, batch_idxs, noise, complex_ids, step, inpaint, repetition)
        coef = self.step_coefficients(s, t)
        eps_h, eps_x = self.dynamics(g, t, batch_idxs)
        if noise is None:
            noise = (self._draw(g, 3, complex_ids, step, 0), self._draw(g, lig['h_0'].shape[1], complex_ids, step, 1))
        hip.sample_update(g.prepared(), self.n_lig_features, lig['x_0'], lig['h_0'], kp['x_0'], eps_x, eps_h,
                          noise[0], noise[1], coef)
        return g

    def _inpaint_step(self, s, t, g, batch_idxs, noise, complex_ids, step, inpaint, repetition):
        lig, kp = g.nodes['lig'].data, g.nodes['kp'].data
        coef = self.inpaint_coefficients(s, t)
        eps_h, eps_x = self.dynamics(g, t, batch_idxs)
        noise = tuple(noise) if noise is not None else ()
        if len(noise) not in (0, 2, 4):
            raise ValueError('noise must be (pos, feat) or (pos, feat, known_pos, known_feat)')
        F = lig['h_0'].shape[1]
        for tag in range(len(noise), 4):             # draw order: step x, step h, known x, known h
            noise += (self._draw(g, 3 if tag % 2 == 0 else F, complex_ids, step, 6 * repetition + tag),)
        hip.sample_update_inpaint(g.prepared(), self.n_lig_features, lig['x_0'], lig['h_0'], kp['x_0'], eps_x, eps_h, noise[0],
                                  noise[1], coef, inpaint.fixed, inpaint.x, inpaint.h, inpaint.kp_com0, noise[2], noise[3])
        return g

    def _guided_step(self, s, t, g, batch_idxs, noise, complex_ids, step, inpaint, repetition, guidance):
        if not isinstance(guidance, GuidanceContext):
            raise ValueError(f'guidance must be a GuidanceContext (the prepared wall and kp_com0), got {type(guidance).__name__}')
        if g.device.type != 'cuda':
            raise hip.KpdError(f'a guided step needs the batch on the GPU (got {g.device}); there is no CPU implementation')
        lig, kp = g.nodes['lig'].data, g.nodes['kp'].data
        coef = self.guided_coefficients(s, t, guidance.scale, guidance.t_max)
        eps_h, eps_x = self.dynamics(g, t, batch_idxs)
        noise = tuple(noise) if noise is not None else ()
        F = lig['h_0'].shape[1]
        if inpaint is None:                          # the draws of the plain step: tags 0 and 1
            if len(noise) not in (0, 2):
                raise ValueError('noise must be (pos, feat)')
            if not noise:
                noise = (self._draw(g, 3, complex_ids, step, 0), self._draw(g, F, complex_ids, step, 1))
            known = {}
        else:                                        # the draws of the inpainting step
            if len(noise) not in (0, 2, 4):
                raise ValueError('noise must be (pos, feat) or (pos, feat, known_pos, known_feat)')
            for tag in range(len(noise), 4):
                noise += (self._draw(g, 3 if tag % 2 == 0 else F, complex_ids, step, 6 * repetition + tag),)
            known = dict(fixed=inpaint.fixed, known_x=inpaint.x, known_h=inpaint.h, known_noise_x=noise[2], known_noise_h=noise[3])
        hip.sample_update_guided(g.prepared(), self.n_lig_features, lig['x_0'], lig['h_0'], kp['x_0'], eps_x, eps_h, noise[0], noise[1],
                                 coef, guidance.wall_x, guidance.wall_ptr, guidance.kp_com0, guidance.threshold, **known)
        return g

    def resolve_wall(self, g, wall=None):
        """(wall_x [n_wall,3] fp32, wall_ptr [B+1] int32) on g's device for a batch of encoded pockets, before the loop moves it.
        `wall=None`: the `rec` rows of `g` when it has any (for the fixed encoder these are the atoms the keypoints were taken
        from), else its `kp` rows; otherwise `wall` is `(wall_x, wall_ptr)` in the input frame and is checked against the batch."""
        B = g.batch_size
        if wall is None:
            nt = 'rec' if g.num_nodes('rec') > 0 else 'kp'
            wall_x, wall_ptr = g.nodes[nt].data['x_0'].float().clone(), g.node_ptr(nt)
        else:
            if not (isinstance(wall, (tuple, list)) and len(wall) == 2):
                raise ValueError('guidance.wall must be None or (wall_x [n_wall,3], wall_ptr [B+1]) for a batch of encoded pockets')
            wall_x, wall_ptr = torch.as_tensor(wall[0]), torch.as_tensor(wall[1])
            hip.check_wall(wall_x, wall_ptr, B, 'guidance.wall')
        return wall_x.float().to(g.device).contiguous(), wall_ptr.to(g.device).int().contiguous()

    def resolve_pocket_walls(self, ref_graphs, wall=None):
        """One [m_i,3] fp32 tensor per pocket, in that pocket's frame: `wall=None` takes each pocket's receptor atoms as given
        (`rec` `x_0` of `ref_graphs[i]`, before encoding); otherwise `wall` is one tensor per pocket."""
        if wall is None:
            return [r.nodes['rec'].data['x_0'].float() for r in ref_graphs]
        if not isinstance(wall, (list, tuple)) or len(wall) != len(ref_graphs):
            raise ValueError(f'guidance.wall must have one [m,3] tensor per pocket ({len(ref_graphs)}), got '
                             f'{len(wall) if isinstance(wall, (list, tuple)) else type(wall).__name__}')
        wall = [torch.as_tensor(w).float() for w in wall]
        for i, w in enumerate(wall):
            if w.dim() != 2 or w.shape[1] != 3:
                raise ValueError(f'guidance.wall[{i}] must be [m, 3] (got {tuple(w.shape)})')
        return wall

    def clash_score(self, positions, wall, threshold: float) -> torch.Tensor:
        """[n,3] = per ligand {1/2 sum (threshold - d)+^2, pairs with d < threshold, smallest such d or +inf} (kpd_clash_score):
        `positions` is a list of [n_i,3] tensors as the samplers return them, `wall` one [m,3] tensor for all of them or a list
        with one per ligand, in the same frame.  Runs on the GPU the model lives on; the result comes back on the host."""
        positions = [torch.as_tensor(p).float() for p in positions]
        wall = [torch.as_tensor(wall).float()] * len(positions) if isinstance(wall, torch.Tensor) else [torch.as_tensor(w).float() for w in wall]
        if len(wall) != len(positions) or not positions:
            raise ValueError(f'clash_score: {len(positions)} ligands but {len(wall)} walls')
        for name, ts in (('positions', positions), ('wall', wall)):
            for i, p in enumerate(ts):
                if p.dim() != 2 or p.shape[1] != 3:
                    raise ValueError(f'clash_score: {name}[{i}] must be [n, 3] (got {tuple(p.shape)})')
        dev = next(self.parameters()).device
        if dev.type != 'cuda':
            raise hip.KpdError(f'clash_score runs on the GPU (the model lives on {dev}); there is no CPU implementation')
        ptr = lambda ts: torch.tensor([0] + [p.shape[0] for p in ts]).cumsum(0).int().to(dev)
        return hip.clash_score(torch.cat(positions).to(dev).contiguous(), ptr(positions), torch.cat(wall).to(dev).contiguous(), ptr(wall),
                               ClashGuidance(threshold).threshold).cpu()

    def renoise_zt_given_zs(self, s, t, g, noise=None, complex_ids=None, step=0, repetition=0):
        """The forward move between two repetitions of a resampled inpainting step: z_t = alpha_t|s z_s + sigma_t|s n for the
        ligand positions and features, then ligand-COM removal (kpd_sample_renoise).  Tags 6u + 4, 6u + 5 of the per-complex
        streams."""
        lig, kp = g.nodes['lig'].data, g.nodes['kp'].data
        if noise is None:
            noise = (self._draw(g, 3, complex_ids, step, 6 * repetition + 4),
                     self._draw(g, lig['h_0'].shape[1], complex_ids, step, 6 * repetition + 5))
        hip.sample_renoise(g.prepared(), self.n_lig_features, lig['x_0'], lig['h_0'], kp['x_0'], noise[0], noise[1],
                           self.inpaint_coefficients(s, t))
        return g

    @torch.no_grad()
    def capture_step(self, g, bidx=None, noise=None, inpaint=None, guidance=None) -> 'StepGraph':
        """One reverse step (`sample_p_zs_given_zt`) captured as a HIP graph for this batch: replaying it costs one
        launch instead of ~30.  The step's kernels take shapes from host-known capacities and counts from device memory,
        so the same graph serves every timestep.  Measured gain is small (B = 1: 0.99 -> 0.96 ms/step, B = 64: 8.32 ->
        8.29): the step is bound by its chain of dependent kernels, not by launch overhead."""
        if guidance is None:
            return StepGraph(self, g, bidx, noise, inpaint)
        return StepGraph(self, g, bidx, noise, inpaint, guidance)

    @torch.no_grad()
    def sample_from_encoded_receptors(self, g, visualize=False, init_lig_pos: torch.Tensor = None, complex_ids=None,
                                      use_graph: Optional[bool] = None, guidance: Optional[ClashGuidance] = None):
        """Full reverse loop for a batch of encoded pockets (ligand_diffuser.py:342-469).  `complex_ids` [B] int64
        (global index of every complex in the job) selects the per-complex noise streams of `use_complex_noise`.
        `use_graph=True`: replay the reverse step as a captured HIP graph (not with the per-complex noise streams, which
        take the timestep as a launch argument); the default is the eager step, the measured difference is ≤ 3 %.
        `guidance` (a `ClashGuidance`): every step pushes the denoised positions out of the wall atoms (`resolve_wall` says
        which); GPU batches only.  With `guidance=None` the loop is call for call what it was."""
        if guidance is None:
            return self._reverse_loop(g, visualize, init_lig_pos, complex_ids, use_graph)
        return self._reverse_loop(g, visualize, init_lig_pos, complex_ids, use_graph, guidance=self._checked_guidance(g, guidance))

    @staticmethod
    def _checked_guidance(g, guidance):
        if not isinstance(guidance, ClashGuidance):
            raise ValueError(f'guidance must be a ClashGuidance (got {type(guidance).__name__})')
        if g.device.type != 'cuda':
            raise hip.KpdError(f'guided sampling needs the batch on the GPU (got {g.device}); there is no CPU implementation')
        return guidance

    @torch.no_grad()
    def inpaint_from_encoded_receptors(self, g, fixed: torch.Tensor, resamplings: int = 1, visualize=False,
                                       init_lig_pos: torch.Tensor = None, complex_ids=None, use_graph: Optional[bool] = None,
                                       overwrite_fixed: bool = True, guidance: Optional[ClashGuidance] = None):
        """The reverse loop around fixed atoms (RePaint-style replacement conditioning; include/kpd.h, "Inpainting").  `fixed`
        [n_lig] bool / uint8 marks the given ligand atoms; their known positions (input frame) and features are the ligand rows
        of `g`, the other rows are generated.  Every timestep is run `resamplings` times with a forward move back to t in between
        (r T denoiser forwards in all).  `overwrite_fixed`: return the fixed rows as the caller's values bit for bit; otherwise
        they come back as the loop leaves them, X + (alpha_0 - 1) k0 + sigma_0 n'.  Without `init_lig_pos` a complex with fixed
        atoms starts in the frame of the mean of its known positions.  `use_graph=True` is available for `resamplings == 1` with
        the global noise.  `guidance` (a `ClashGuidance`): the free atoms are also pushed out of the wall atoms; the fixed atoms
        are neither pushed nor part of the wall.  Returns what `sample_from_encoded_receptors` returns."""
        n_lig = g.num_nodes('lig')
        if not (isinstance(fixed, torch.Tensor) and fixed.dtype in (torch.bool, torch.uint8)):
            raise ValueError(f'fixed must be a bool or uint8 tensor (got {getattr(fixed, "dtype", type(fixed).__name__)})')
        if fixed.dim() != 1 or fixed.shape[0] != n_lig:
            raise ValueError(f'fixed must have one entry per ligand atom: expected [{n_lig}], got {list(fixed.shape)}')
        if isinstance(resamplings, bool) or not isinstance(resamplings, int) or resamplings < 1:
            raise ValueError(f'resamplings must be an integer >= 1 (got {resamplings!r})')
        width = g.nodes['lig'].data['h_0'].shape[1] if g.nodes['lig'].data['h_0'].dim() == 2 else -1
        if width != self.n_lig_features:
            raise ValueError(f"the ligand features of g (h_0) must have atom_nf = {self.n_lig_features} columns (got {width})")
        if g.device.type != 'cuda':
            raise hip.KpdError(f'inpaint_from_encoded_receptors: g must live on the GPU (got {g.device}); there is no CPU implementation')
        kw = {} if guidance is None else {'guidance': self._checked_guidance(g, guidance)}
        return self._reverse_loop(g, visualize, init_lig_pos, complex_ids, use_graph, fixed=fixed.to(g.device),
                                  resamplings=resamplings, overwrite_fixed=overwrite_fixed, **kw)

    def _reverse_loop(self, g, visualize, init_lig_pos, complex_ids, use_graph, fixed=None, resamplings=1, overwrite_fixed=True,
                      guidance=None):
        """The loop behind `sample_from_encoded_receptors` (fixed is None: the plain sampler, call for call as upstream) and
        `inpaint_from_encoded_receptors`.  The per-complex means of the set-up and of the frame restoration are summed in a fixed
        order (`G.segment_sum_ordered`): with the per-complex noise streams a run is then a function of its inputs and the seed,
        bit for bit, as the step kernels already are."""
        device, B = g.device, g.batch_size
        init_kp_com = G.readout_nodes(g, feat='x_0', op='mean', ntype='kp', ordered=True)
        bidx = G.get_batch_idxs(g)
        lig_b, kp_b = bidx['lig'], bidx['kp']
        ctx, gkw = None, {}
        if guidance is not None:         # the wall in the input frame, before anything moves; every call below gets it as a keyword
            gkw = {'guidance': GuidanceContext(*self.resolve_wall(g, guidance.wall), init_kp_com, guidance.threshold, guidance.scale,
                                               guidance.t_max)}
        if fixed is not None:
            fixed = fixed.bool()
            known_x, known_h = g.nodes['lig'].data['x_0'].float().clone(), g.nodes['lig'].data['h_0'].float().clone()
            ctx = InpaintContext(fixed, known_x, known_h / self.lig_feat_norm_constant, init_kp_com)
        if init_lig_pos is not None:
            assert init_lig_pos.shape == (B, 3)
            frame = init_lig_pos
        else:
            frame = G.readout_nodes(g, feat='x_0', op='mean', ntype='rec', ordered=True)
            if ctx is not None:          # a complex with fixed atoms starts around them
                w = fixed.to(known_x.dtype)[:, None]
                n_lig_atoms = g.batch_num_nodes('lig')
                n_fixed = G.segment_sum_ordered(w, n_lig_atoms)
                known_com = G.segment_sum_ordered(known_x * w, n_lig_atoms) / n_fixed.clamp(min=1)
                frame = torch.where(n_fixed > 0, known_com, frame)
        g.nodes['kp'].data['x_0'] = g.nodes['kp'].data['x_0'] - frame[kp_b]
        if complex_ids is not None:
            complex_ids = complex_ids.to(device).long()
        for tag, feat in enumerate(('x_0', 'h_0')):
            g.nodes['lig'].data[feat] = self._draw(g, g.nodes['lig'].data[feat].shape[1], complex_ids, self.n_timesteps, tag)
        g = self.remove_com(g, lig_b, kp_b, com='ligand', ordered=True)

        def snapshot():
            f = G.copy_graph(g, n_copies=1, batched_graph=True)[0]
            f = self.unnormalize(f)
            delta = init_kp_com - G.readout_nodes(f, feat='x_0', ntype='kp', op='mean', ordered=True)
            f.nodes['lig'].data['x_0'] = f.nodes['lig'].data['x_0'] + delta[lig_b]
            parts = G.unbatch(f.to('cpu'))
            return [p.nodes['lig'].data['x_0'] for p in parts], [p.nodes['lig'].data['h_0'] for p in parts]

        frames_x, frames_h = [], []
        if visualize:
            fx, fh = snapshot()
            frames_x.append(fx), frames_h.append(fh)
        ones = torch.ones(B, device=device)
        per_complex = getattr(self, '_noise_seed', None) is not None and complex_ids is not None
        if use_graph and per_complex:
            raise ValueError('use_graph=True cannot be combined with per-complex noise streams (the timestep is a launch argument)')
        if use_graph and resamplings != 1:
            raise ValueError('use_graph=True needs resamplings == 1 (the forward move between repetitions is not part of the captured step)')
        if ctx is None:
            step_graph = self.capture_step(g, bidx, **gkw) if use_graph else None
        else:
            step_graph = self.capture_step(g, bidx, inpaint=ctx, **gkw) if use_graph else None
        for s in reversed(range(self.n_timesteps)):
            if step_graph is not None:
                step_graph.step(s / self.n_timesteps, (s + 1) / self.n_timesteps)
            elif ctx is None:
                g = self.sample_p_zs_given_zt(ones * (s / self.n_timesteps), ones * ((s + 1) / self.n_timesteps), g, bidx,
                                              complex_ids=complex_ids, step=s, **gkw)
            else:
                s_, t_ = ones * (s / self.n_timesteps), ones * ((s + 1) / self.n_timesteps)
                for u in range(resamplings):
                    g = self.sample_p_zs_given_zt(s_, t_, g, bidx, complex_ids=complex_ids, step=s, inpaint=ctx, repetition=u, **gkw)
                    if u + 1 < resamplings:
                        g = self.renoise_zt_given_zs(s_, t_, g, complex_ids=complex_ids, step=s, repetition=u)
            if visualize:
                fx, fh = snapshot()
                frames_x.append(fx), frames_h.append(fh)

        g = self.remove_com(g, lig_b, kp_b, com='receptor', ordered=True)
        for nt in ('lig', 'kp'):
            g.nodes[nt].data['x_0'] = g.nodes[nt].data['x_0'] + init_kp_com[bidx[nt]]
        g = self.unnormalize(g)
        if ctx is not None and overwrite_fixed:
            g.nodes['lig'].data['x_0'] = torch.where(fixed[:, None], known_x, g.nodes['lig'].data['x_0'])
            g.nodes['lig'].data['h_0'] = torch.where(fixed[:, None], known_h, g.nodes['lig'].data['h_0'])
        if visualize and not (ctx is not None and overwrite_fixed):
            return list(zip(*frames_x)), list(zip(*frames_h))
        parts = G.unbatch(g.to('cpu'))
        pos, feat = [p.nodes['lig'].data['x_0'] for p in parts], [p.nodes['lig'].data['h_0'] for p in parts]
        if visualize:                                        # the last frame is the result: it carries the overwritten rows
            frames_x[-1], frames_h[-1] = pos, feat
            return list(zip(*frames_x)), list(zip(*frames_h))
        return pos, feat

    @torch.no_grad()
    def _sample(self, ref_graphs: List[G.HeteroBatch], n_lig_atoms: List[List[int]], rec_enc_batch_size: int = 32,
                diff_batch_size: int = 32, visualize=False, use_ref_lig_com: bool = False, group=None, known=None,
                resamplings: int = 1, guidance: Optional[ClashGuidance] = None):
        """Several pockets x several ligands per pocket (ligand_diffuser.py:271-340).

        `known` (inpainting): one entry per pocket, None or (pos [m_i,3] in the pocket's frame, feat [m_i,atom_nf]); these atoms
        are rows 0 .. m_i - 1 of every ligand generated for pocket i and are held fixed, the other rows are generated
        (`inpaint_from_encoded_receptors`, with `resamplings`).

        `guidance` (a `ClashGuidance`): clash guidance in every reverse step; its `wall` is None (each pocket's receptor atoms as
        given in `ref_graphs[i]`, before encoding) or one [m_i,3] tensor per pocket in that pocket's frame.  A C-alpha model
        should be handed the full-atom pocket here.  Every complex carries its pocket's wall, so sharding changes nothing.

        The flat list of (pocket, replicate) complexes it builds (:292-313) is the unit of multi-GPU work:
        when a `torch.distributed` process group with more than one rank is initialised, every rank calls this with the SAME
        arguments, takes a contiguous, edge-count-balanced shard of that list (`dist.shard_complexes`), encodes only the pockets
        its shard touches, runs the reverse loop on its shard in `diff_batch_size` batches, and one all-gather of the ligand
        tensors (`dist.gather_ligand_lists`, RCCL over xGMI) returns ALL ligands, in input order, on every rank.  Noise then comes
        from the per-complex Philox streams keyed by the global complex index (`use_complex_noise`; switched on with a seed
        all ranks agree on if the caller did not choose one), so the sharded run reproduces the single-process run of the same
        seed up to fp32 summation order.  The pockets are encoded `rec_enc_batch_size` at a time."""
        from . import dist as D
        sharded = D.sharding_active(group)
        if sharded and visualize:
            raise ValueError('visualize=True returns whole trajectories and is a single-process feature')
        # the flat complex list: (pocket index, number of ligand atoms), in input order
        flat = [(i, int(n)) for i, sizes in enumerate(n_lig_atoms) for n in sizes]
        device = ref_graphs[0].device
        if isinstance(resamplings, bool) or not isinstance(resamplings, int) or resamplings < 1:
            raise ValueError(f'resamplings must be an integer >= 1 (got {resamplings!r})')
        walls = None
        if guidance is not None:
            walls = [w.to(device) for w in self.resolve_pocket_walls(ref_graphs, self._checked_guidance(ref_graphs[0], guidance).wall)]
        if known is not None:
            if len(known) != len(ref_graphs):
                raise ValueError(f'known must have one entry per pocket ({len(ref_graphs)}), got {len(known)}')
            known = [None if k is None else (torch.as_tensor(k[0]).float(), torch.as_tensor(k[1]).float()) for k in known]
            for i, k in enumerate(known):
                if k is None:
                    continue
                if k[0].dim() != 2 or k[0].shape[1] != 3 or k[1].dim() != 2 or k[1].shape[0] != k[0].shape[0]:
                    raise ValueError(f'known[{i}] must be (pos [m,3], feat [m,atom_nf]); got {tuple(k[0].shape)}, {tuple(k[1].shape)}')
                if k[1].shape[1] != self.n_lig_features:
                    raise ValueError(f'known[{i}]: the known features must have atom_nf = {self.n_lig_features} columns '
                                     f'(got {k[1].shape[1]})')
                small = [n for n in n_lig_atoms[i] if int(n) < k[0].shape[0]]
                if small:
                    raise ValueError(f'n_lig_atoms[{i}] asks for {int(small[0])} atoms, fewer than the {k[0].shape[0]} known atoms '
                                     f'of known[{i}]')

        def run(mine):
            """Ligands of the complexes `mine` (a range into `flat`)."""
            pockets = sorted({flat[c][0] for c in mine})
            encoded = {}
            for lo in range(0, len(pockets), max(1, rec_enc_batch_size)):
                chunk = pockets[lo:lo + max(1, rec_enc_batch_size)]
                enc = self.encode_receptors(G.batch([ref_graphs[i] for i in chunk]))
                encoded.update(zip(chunk, G.unbatch(enc)))
            graphs = []
            for c in mine:           # one copy_graph call per (pocket, run of replicates) keeps the reference's copy semantics
                i, n = flat[c]
                graphs.extend(G.copy_graph(encoded[i], n_copies=1, lig_atoms_per_copy=torch.tensor([n])))
                if known is not None:
                    m = 0 if known[i] is None else known[i][0].shape[0]
                    d = graphs[-1].nodes['lig'].data
                    if m:
                        d['x_0'][:m], d['h_0'][:m] = known[i][0].to(device), known[i][1].to(device)
                    d['_fixed'] = torch.arange(n, device=device) < m
            pos, feat = [], []
            for lo in range(0, len(graphs), diff_batch_size):
                bg = G.batch(graphs[lo:lo + diff_batch_size])
                init = G.readout_nodes(bg, feat='x_0', op='mean', ntype='lig') if use_ref_lig_com else None
                ids = torch.arange(mine[lo], mine[lo] + bg.batch_size, dtype=torch.long)
                gkw = {}
                if walls is not None:
                    ws = [walls[flat[c][0]] for c in mine[lo:lo + bg.batch_size]]
                    wptr = torch.tensor([0] + [w.shape[0] for w in ws]).cumsum(0)
                    gkw = {'guidance': guidance.with_wall((torch.cat(ws), wptr))}
                if known is None:
                    p, f = self.sample_from_encoded_receptors(bg, visualize=visualize, init_lig_pos=init, complex_ids=ids, **gkw)
                else:
                    fixed = bg.nodes['lig'].data.pop('_fixed')
                    p, f = self.inpaint_from_encoded_receptors(bg, fixed, resamplings=resamplings, visualize=visualize,
                                                               init_lig_pos=init, complex_ids=ids, **gkw)
                pos.extend(p), feat.extend(f)
            return pos, feat

        if sharded:
            restore = getattr(self, '_noise_seed', None)
            if restore is None:
                self.use_complex_noise(D.common_seed(group))
            try:
                # cost of a complex ~ its edges per layer: kk + kl/lk grow with the pocket, ll with the ligand
                costs = [600.0 + 22.7 * ref_graphs[i].num_nodes('rec') + n * n for i, n in flat]
                lig_pos, lig_feat = D.sharded_map(costs, run, group=group, device=device)
            finally:
                self._noise_seed = restore
        else:
            lig_pos, lig_feat = run(range(len(flat)))
        samples, end = [], 0
        for i in range(len(ref_graphs)):
            start, end = end, end + len(n_lig_atoms[i])
            samples.append({'positions': lig_pos[start:end], 'features': lig_feat[start:end]})
        return samples

    @torch.no_grad()
    def sample_given_pocket(self, rec_graph, n_lig_atoms: torch.Tensor, rec_enc_batch_size: int = 32,
                            diff_batch_size: int = 32, visualize=False, guidance: Optional[ClashGuidance] = None):
        """`guidance.wall`: None (the pocket's receptor atoms) or one [m,3] tensor in the pocket's frame."""
        kw = {} if guidance is None else {'guidance': self._one_pocket(guidance)}
        s = self._sample([rec_graph], n_lig_atoms=[n_lig_atoms.tolist()], rec_enc_batch_size=rec_enc_batch_size,
                         diff_batch_size=diff_batch_size, visualize=visualize, **kw)
        return s[0]['positions'], s[0]['features']

    @torch.no_grad()
    def inpaint_given_pocket(self, rec_graph, known_pos: torch.Tensor, known_feat: torch.Tensor, n_lig_atoms: torch.Tensor,
                             rec_enc_batch_size: int = 32, diff_batch_size: int = 32, resamplings: int = 1, visualize=False,
                             guidance: Optional[ClashGuidance] = None):
        """Ligands of the sizes `n_lig_atoms` for one pocket, grown around the known atoms: `known_pos` [m,3] (the pocket's
        frame) and `known_feat` [m,atom_nf] come back as rows 0 .. m - 1 of every ligand.  `guidance` as in `sample_given_pocket`."""
        known_pos, known_feat = torch.as_tensor(known_pos), torch.as_tensor(known_feat)
        if known_pos.dim() != 2 or known_pos.shape[1] != 3:
            raise ValueError(f'known_pos must be [m, 3] (got {tuple(known_pos.shape)})')
        if known_feat.dim() != 2 or known_feat.shape[0] != known_pos.shape[0] or known_feat.shape[1] != self.n_lig_features:
            raise ValueError(f'known_feat must be [{known_pos.shape[0]}, atom_nf = {self.n_lig_features}] (got {tuple(known_feat.shape)})')
        s = self._sample([rec_graph], n_lig_atoms=[torch.as_tensor(n_lig_atoms).tolist()], rec_enc_batch_size=rec_enc_batch_size,
                         diff_batch_size=diff_batch_size, visualize=visualize, known=[(known_pos, known_feat)],
                         resamplings=resamplings, **({} if guidance is None else {'guidance': self._one_pocket(guidance)}))
        return s[0]['positions'], s[0]['features']

    @staticmethod
    def _one_pocket(guidance):
        """The single-pocket entry points take the wall as one tensor; `_sample` takes one per pocket."""
        if not isinstance(guidance, ClashGuidance):
            raise ValueError(f'guidance must be a ClashGuidance (got {type(guidance).__name__})')
        return guidance if guidance.wall is None else guidance.with_wall([guidance.wall])

    @torch.no_grad()
    def sample_random_sizes(self, ref_graphs, n_replicates: int = 10, rec_enc_batch_size: int = 32,
                            diff_batch_size: int = 32, guidance: Optional[ClashGuidance] = None):
        if self.lig_size_dist is None:
            raise ValueError('no processed_dataset_dir was given: the ligand-size prior is unavailable')
        n_rec = torch.tensor([g.num_nodes('rec') for g in ref_graphs])
        n_lig = self.lig_size_dist.sample(n_rec, n_replicates)
        return self._sample(ref_graphs, n_lig_atoms=n_lig.tolist(), rec_enc_batch_size=rec_enc_batch_size,
                            diff_batch_size=diff_batch_size, **({} if guidance is None else {'guidance': guidance}))


LigandDiffuser = KeypointDiffusion
