#!/usr/bin/env python
"""Headline benchmark: denoising steps/sec of the reverse-diffusion hot path on MI355X.

A *step* is one reverse-diffusion step (`KeypointDiffusion.sample_p_zs_given_zt`:
denoiser forward + z_s update + COM removal) over one batch of B synthetic complexes that
is already resident in HBM.  Contract workload = BASELINE.json configs[1]:
egnn_all_atom dynamics, B = 64 synthetic 300-atom pockets / 25-atom ligands, T = 500.

    python bench.py --gpus N --steps K --warmup W [--full]

N > 1: one rank per GPU over RCCL.  Either the caller starts the ranks (torch.distributed.run: RANK /
WORLD_SIZE / MASTER_* in the environment) or -- when WORLD_SIZE is absent -- this script starts N fresh
rank processes itself, BEFORE anything touches the GPU, and relays rank 0's JSON line.  Every rank owns
its own batch of B complexes (weak scaling, no data-path collective); one all-gather of the ligand
tensors sits at the end of each timed region (the exchange the sharded sampler performs after the last
step).  W warm-up steps, then `--repeats` regions of EXACTLY K steps, each bracketed by barrier +
synchronize on both sides and reduced with MAX over ranks; `value` is the MEDIAN region, the spread is
reported beside it.  Rank 0 prints ONE JSON line.

A plain run does only what that line needs: set up, warm up, time the regions, write `--dump-outputs`,
print.  `--full` (off by default) adds, at N = 1, everything that takes runs of its own: the CPU baseline
of the oracle with its parity check of the measured path, and for the contract workload BASELINE.json
configs[0] on the GPU, configs[2] (gvp_40kp, B = 64) and the configs[4] shape (gvp_all_atom, ragged
150-600 / 15-35 atoms), B = 512 and the f16x2 mode (nested under `secondary`, each with its own roofline
and CPU baseline), and full sampling runs end to end (`end_to_end`: receptor encoding + T reverse steps +
host copy -> measured ligands/min).
"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CUTOFFS = {'kk': 8, 'kl': 6, 'll': 6, 'rk': 100, 'rr': 3.5}      # trained_models/egnn_all_atom/config.yml
DYNAMICS = dict(hidden_nf=256, kl_k=5, ll_k=0, message_norm=0, n_layers=6, no_cg=False, norm=True,
                update_kp_feat=True, use_tanh=True)
PEAK_F32_MATRIX_TFLOPS = 157.3      # MI355X_MICROARCH.md: dense fp32 MFMA peak (= the fp32 vector peak)
PEAK_HBM_GBS = 8000.0
# What back-to-back fp32 MFMAs deliver on all CUs of this part at once, measured WITH a clock trace in round 3
# (profiles/tools/mfma_clock_trace.hip -> profiles/r03_mfma_clock_trace.txt: 64.0 cycles per v_mfma_f32_32x32x2_f32, 2.37 GHz held
# over 2 s of continuous MFMA issue at ~697 W => 155.5 TFLOP/s).  Round 2's "132 sustained" came from single 0.7-ms launches out of
# idle, i.e. from the clock ramp (the first launches of the trace run at 0.96 - 2.2 GHz); it is withdrawn.  Context for `frac`, not the peak.
MEASURED_F32_MFMA_TFLOPS = 155.5
# f16x2 mode (opt-in, --gemm f16x2 / KPD_GEMM=f16x2): every fp32 product of the EGNN GEMMs (edge, projection and node-update kernels) and of
# the 256 x 256 products of the GVP message / update chains is three f16 MFMA products of hi / lo operand planes with fp32 accumulation, so the bound for USEFUL flops is the dense f16 MFMA peak (MI355X_MICROARCH.md: ~2.5 PFLOP/s) / 3
PEAK_F16_MATRIX_TFLOPS = 2500.0
# FLOPs the fused EGNN edge kernel executes per edge per layer: the two 257x257 second Linears of edge_mlp /
# coord_mlp plus the attention and coordinate heads (the first Linears run per NODE, k_proj_ws)
EDGE_KERNEL_FLOP_PER_EDGE = 2 * (2 * 257 * 257) + 2 * (2 * 257)
# reference formulation of the same edge work: both Linears of both MLPs
EDGE_ALGO_FLOP_PER_EDGE = 2 * (515 * 257 + 257 * 257) * 2 + 4 * 257
EDGE_ALGO_BYTES_PER_EDGE = 4 * 257 + 16          # gathered row + coords + index
GVP_ALGO_FLOP_PER_EDGE = 460.9e3                 # 3 chained message GVPs, reference formulation
GVP_ALGO_BYTES_PER_EDGE = 4 * 304 + 16           # 256 scalars + 48 vector floats + coords + index


def gvp_chain_flop_per_edge(S=256, V=16, n_msg=3, rbf=16):
    """FLOPs k_gvp_chain executes per edge: the message chain of GVPMultiEdgeConv.message (models/gvp.py:545-549) with the
    h_src block of the first to_feats_out applied per node (k_gvp_proj_chain).  Unpadded matrix shapes; the MFMA instruction
    count of the kernel (PMC) gives 1 % more (padding of the 17-channel hidden tile)."""
    vi, h0 = V + 1, max(V + 1, V)                                           # [x_diff | v_src] -> hidden max(vi, vo)
    head = 2 * (3 * vi * h0 + (rbf + h0) * S + S * V + 3 * h0 * V)         # vec1, [rbf | sh] block, gates, vec2
    rest = 2 * (3 * V * V + (S + V) * S + S * V + 3 * V * V)
    return head + (n_msg - 1) * rest


# secondary workloads (BASELINE.json configs[2] and configs[4]); the JSON contract line is always configs[1]
GVP_DYN = dict(vector_size=16, n_convs=6, n_hidden_scalars=256, message_norm=10.0, update_kp=True, ll_k=0, kl_k=7,
               n_message_gvps=3, n_update_gvps=2, n_noise_gvps=4, dropout=0.1)
GVP_ENC = dict(out_scalar_size=128, n_message_gvps=3, n_update_gvps=2, vector_size=16, n_rr_convs=4, n_rk_convs=2,
               message_norm=10.0, k_closest=5, kp_rad=0, dropout=0.1)
EGNN_ENC = dict(coords_range=10, fix_pos=False, hidden_n_node_feat=128, k_closest=5, kp_feat_scale=1.0, kp_rad=0.0,
                message_norm=0.0, n_convs=4, n_kk_convs=0, n_kk_heads=4, no_cg=False, norm=True, out_n_node_feat=128,
                use_sameres_feat=True, use_tanh=True)                      # trained_models/egnn_40kp/config.yml:59-75
WORKLOADS = {
    'egnn_all_atom': dict(arch='egnn', enc='fixed', dyn=DYNAMICS, n_kp=20, cutoffs=CUTOFFS, T=500),
    'egnn_40kp': dict(arch='egnn', enc='learned', dyn=dict(DYNAMICS, message_norm=0.0), n_kp=40,
                      cutoffs=dict(CUTOFFS, kl=8, ll=5), T=500),
    'gvp_40kp': dict(arch='gvp', enc='learned', dyn=GVP_DYN, n_kp=40, cutoffs=dict(CUTOFFS, kl=8, ll=6.0), T=500),
    'gvp_all_atom': dict(arch='gvp', enc='fixed', dyn=dict(GVP_DYN, message_norm='mean'), n_kp=20, cutoffs=CUTOFFS, T=1000),
    # one optimisation step of train.py's inner loop (loss of KeypointDiffusion.forward, backward, clip, Adam) on the
    # egnn_all_atom model: the backward pass of csrc/egnn_train.hip
    'egnn_train': dict(arch='egnn', enc='fixed', dyn=DYNAMICS, n_kp=20, cutoffs=CUTOFFS, T=500),
    # same for the gvp_all_atom model in training mode (GVPDropout 0.1): the backward pass of csrc/gvp_train.hip
    'gvp_train': dict(arch='gvp', enc='fixed', dyn=dict(GVP_DYN, message_norm='mean'), n_kp=20, cutoffs=CUTOFFS, T=1000),
    # the same for the keypoint models (learned receptor encoder -> 40 keypoints -> denoiser; encoder + denoiser backward passes and the
    # optimal-transport encoder loss): trained_models/gvp_40kp, egnn_40kp
    'gvp_40kp_train': dict(arch='gvp', enc='learned', dyn=GVP_DYN, n_kp=40, cutoffs=dict(CUTOFFS, kl=8, ll=6.0), T=500),
    'egnn_40kp_train': dict(arch='egnn', enc='learned', dyn=dict(DYNAMICS, message_norm=0.0), n_kp=40, cutoffs=dict(CUTOFFS, kl=8, ll=5), T=500),
}
TRAFFIC_FILES = ('r05_traffic.json', 'r04_traffic.json', 'r03_traffic.json', 'r02_traffic.json', 'r01_traffic.json')      # per-launch HBM bytes of the dominant kernels (PMC passes)


# ---------------------------------------------------------------------------------------------------
# what the line attests about the process that produced it
# ---------------------------------------------------------------------------------------------------
# KPD_* variables that do not change what the kernels compute or how fast (launcher rehearsal switches of this script)
HARMLESS_ENV = ('KPD_BENCH_SPAWN_ECHO', 'KPD_BENCH_SHARE_GPU', 'KPD_BENCH_DIST_AT_1')


class BenchRefused(SystemExit):
    """bench.py will not print a line it cannot stand behind (exit code 2)."""

    def __init__(self, why):
        print(f'bench.py: refused -- {why}', file=sys.stderr, flush=True)
        super().__init__(2)


def attest_environment(environ, build_flags, allow_tools=False):
    """Every KPD_* variable other than this script's own rehearsal switches selects a different kernel path (KPD_GEMM), a memory mode
    (KPD_TRAIN_STORE), NaN poisoning (KPD_POISON), another library (KPD_LIB) or -- in the TOOLS build of the library only -- an A/B or
    ablation switch (KPD_EDGE_ABLATE can tell the contract kernel to skip its GEMM).  A run with any of them set, or on a library whose
    kpd_build_flags() is not 0, is refused unless `--tools` marks it as a diagnostic run; either way the line lists what was set.
    Pure function (tests/test_bench_line.py)."""
    seen = sorted(k for k in environ if k.startswith('KPD_'))
    altering = [k for k in seen if k not in HARMLESS_ENV]
    if not allow_tools:
        if altering:
            raise BenchRefused(f'performance-altering variables are set: {", ".join(altering)} (use the flags of this script, e.g. --gemm; '
                               f'--tools marks a diagnostic run)')
        if build_flags != 0:
            raise BenchRefused(f'libkpd_hip.so is not the product build (kpd_build_flags() = {build_flags}: TOOLS build)')
    return {'env': seen, 'build': 'product' if build_flags == 0 else 'tools', 'attested': not altering and build_flags == 0}


def check_record(out):
    """A roofline fraction outside (0, 1] means the accounting or the run is wrong (work skipped, wrong peak, a kernel that did not
    run): refuse to print it.  Applies to the contract line and to every secondary."""
    def one(name, r):
        rf = (r or {}).get('roofline')
        if rf is None:
            return
        frac = rf.get('frac')
        if frac is None or not (0.0 < frac <= 1.0):
            raise BenchRefused(f'roofline.frac of {name} is {frac}: outside (0, 1]')
        hb = (rf.get('hbm') or {}).get('frac')
        if hb is not None and not (0.0 <= hb <= 1.0):
            raise BenchRefused(f'roofline.hbm.frac of {name} is {hb}: outside [0, 1]')
    one('the contract workload', out)
    for name, r in (out.get('secondary') or {}).items():
        one(name, r)
    for name, r in (out.get('hbm_kernels') or {}).get('kernels', {}).items():
        if not (0.0 <= r.get('frac', 0.0) <= 1.0):
            raise BenchRefused(f'hbm_kernels[{name}].frac is {r.get("frac")}: outside [0, 1]')


# ---------------------------------------------------------------------------------------------------
# rank launcher: `python bench.py --gpus N` without a launcher starts the N ranks itself
# ---------------------------------------------------------------------------------------------------
def spawn_ranks(n: int) -> int:
    """Start n fresh rank processes of this script (one per GPU, RCCL rendezvous on 127.0.0.1) and wait for them.
    Runs before this process has imported torch or touched the GPU: the children are ordinary new processes,
    nothing is exec'ed over a process that holds a GPU context."""
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    try:
        pending = list(procs)
        while pending:
            for p in list(pending):
                code = p.poll()
                if code is None:
                    continue
                pending.remove(p)
                if code != 0 and rc == 0:
                    rc = code
                    for q in pending:            # a rank died: the others would wait in a collective forever
                        q.terminate()
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return rc


# ---------------------------------------------------------------------------------------------------
# models, batches
# ---------------------------------------------------------------------------------------------------
def build_model(device, workload='egnn_all_atom'):
    import torch  # noqa: F401
    from keypoint_diffusion_amd import synth
    from keypoint_diffusion_amd.ligand_diffuser import KeypointDiffusion
    w = WORKLOADS[workload]
    rec_cfg = dict(GVP_ENC) if w['arch'] == 'gvp' else (dict(EGNN_ENC) if w['enc'] == 'learned' else {})
    if w['enc'] == 'learned':
        rec_cfg['in_scalar_size' if w['arch'] == 'gvp' else 'in_n_node_feat'] = 10
    model = KeypointDiffusion(10, 128 if w['enc'] == 'learned' else 10, None, n_timesteps=w['T'],
                              architecture=w['arch'], rec_encoder_type=w['enc'],
                              graph_config=dict(n_keypoints=w['n_kp'], graph_cutoffs=w['cutoffs']),
                              dynamics_config=w['dyn'], rec_encoder_config=rec_cfg, precision=1e-5)
    synth.fill_state_dict_(model, seed=0)
    return model.eval().to(device)


def raw_batch(B, n_rec, n_lig, seed, device, workload='egnn_all_atom'):
    """The un-encoded batch (pocket graphs + t = T ligands), on `device` when the encoder is learned."""
    from keypoint_diffusion_amd import graph as G
    from keypoint_diffusion_amd import synth
    w = WORKLOADS[workload]
    if isinstance(n_rec, int):
        n_rec, n_lig = [n_rec] * B, [n_lig] * B
    g = G.batch(synth.synth_complexes(n_rec, n_lig, w['n_kp'], w['cutoffs'], seed=seed))
    if w['enc'] == 'learned':
        if w['arch'] == 'egnn':                      # synthetic rr `same_res` column (the dataset's bool edge feature)
            s_, d_ = g.edges(etype='rr')
            g.edges['rr'].data['same_res'] = ((s_ // 8) == (d_ // 8)).view(-1, 1)
        g = g.to(device)                             # the learned encoders run on the GPU (once per pocket)
    return g


def build_batch(model, B, n_rec, n_lig, seed, device, workload='egnn_all_atom'):
    import torch
    g = raw_batch(B, n_rec, n_lig, seed, device, workload)
    with torch.no_grad():
        g = model.encode_receptors(g)                # fixed encoder: kp := rec, kk := rr
    return g.to(device)


def ragged_sizes(B, rank):
    import torch
    gen = torch.Generator().manual_seed(77 + rank)
    return (torch.randint(150, 601, (B,), generator=gen).tolist(), torch.randint(15, 36, (B,), generator=gen).tolist())


# ---------------------------------------------------------------------------------------------------
# CPU baselines (the oracle = plain-PyTorch CPU restatement of the reference path; test infrastructure, imported here only)
# ---------------------------------------------------------------------------------------------------
def host_cpu():
    """Cores this process may actually use: physical cores, capped by the affinity mask and the cgroup CPU quota (a GPU box
    hands one-GPU jobs a share of the host, and oversubscribing it is what made round 2's baseline swing by 2.4x)."""
    import math
    import torch
    try:
        import psutil
        phys = psutil.cpu_count(logical=False) or os.cpu_count() or 1
    except Exception:                                                # noqa: BLE001
        phys = os.cpu_count() or 1
    usable = min(phys, len(os.sched_getaffinity(0)))
    quota = None
    try:
        q, per = open('/sys/fs/cgroup/cpu.max').read().split()
        if q != 'max':
            quota = float(q) / float(per)
    except Exception:                                                # noqa: BLE001
        try:
            q = int(open('/sys/fs/cgroup/cpu/cpu.cfs_quota_us').read())
            per = int(open('/sys/fs/cgroup/cpu/cpu.cfs_period_us').read())
            if q > 0:
                quota = q / per
        except Exception:                                            # noqa: BLE001
            pass
    if quota:
        usable = max(1, min(usable, int(math.floor(quota))))
    model = 'unknown'
    try:
        for ln in open('/proc/cpuinfo'):
            if ln.startswith('model name'):
                model = ln.split(':', 1)[1].strip()
                break
    except Exception:                                                # noqa: BLE001
        pass
    return {'cpu_model': model, 'physical_cores': phys, 'logical_cpus': os.cpu_count(), 'affinity': len(os.sched_getaffinity(0)),
            'cgroup_quota_cpus': quota, 'threads_used': usable, 'torch': torch.__version__}


def rank_cpu_threads(usable_cores, local_world):
    """CPU threads one rank of `local_world` ranks on this host may use (at least one)."""
    return max(1, int(usable_cores) // max(1, int(local_world)))


def _cpu_time_steps(fwd, sd, cfg, ob, T, n_warm, n_timed):
    """Per-step wall times (s) of oracle reverse steps, every step taken from the same t = T state (as the GPU line does)."""
    import torch
    from oracle import diffusion as odiff
    table = odiff.gamma_table(T, 1e-5)
    gen = torch.Generator().manual_seed(5)
    B = int(ob.n['lig'].numel())
    times = []
    with torch.no_grad():
        for i in range(n_warm + n_timed):
            si = T - 1 - (i % T)
            s, t = torch.full((B,), si / T), torch.full((B,), (si + 1) / T)
            work = ob.clone()
            nx, nh = torch.randn(work.x['lig'].shape, generator=gen), torch.randn(work.h['lig'].shape, generator=gen)
            t0 = time.perf_counter()
            eh, ex = fwd(sd, cfg, work, t)
            odiff.sample_step(work, eh, ex, s, t, table, T, nx, nh)
            times.append(time.perf_counter() - t0)
    return times[n_warm:]


def _stats(times, B):
    med = statistics.median(times)
    q = statistics.quantiles(times, n=4) if len(times) >= 4 else [min(times), med, max(times)]
    # spread = interquartile range over the median (one preempted step out of fifteen no longer sets it); the full range beside it
    return {'B': B, 'timed_steps': len(times), 's_per_step_median': med, 'spread_pct': 100.0 * (q[2] - q[0]) / med, 'spread_statistic': 'IQR / median',
            'range_pct': 100.0 * (max(times) - min(times)) / med, 'complex_steps_per_s': B / med}


PARITY_TOL = 1e-4          # BASELINE.json north_star: "within 1e-4 rel fp32" (max |a - b| / max |b|, tests/util.py rel_err)


def product_vs_oracle(model, fwd, sd, cfg, g_cpu, tol=PARITY_TOL):
    """The oracle as the checker of the thing being measured: one denoiser forward of the product (HIP path, cuda:0, exact fp32 mode) on the
    B = 8 sample the baseline was just timed on, at t = 1, against the oracle's output for the same inputs.  A line whose kernels do not
    compute the reference's function is refused (round 5: a missed hardware hazard in a hand-scheduled SiLU gave wrong, run-to-run
    different outputs at an unchanged speed -- the bench line looked fine)."""
    import torch
    from keypoint_diffusion_amd import graph as G
    from tests.util import rel_err, to_obatch
    ob = to_obatch(g_cpu)
    t = torch.ones(int(ob.n['lig'].numel()))
    with torch.no_grad():
        ref_h, ref_x = fwd(sd, cfg, ob, t)
        m = model.to('cuda')
        m.dynamics.gemm_mode = 'f32'                   # this model instance belongs to the baseline leg; the timed one is untouched
        gd = g_cpu.to('cuda')
        eps_h, eps_x = m.dynamics(gd, t.to('cuda'), G.get_batch_idxs(gd))
        torch.cuda.synchronize()
    eh, ex = rel_err(eps_h, ref_h), rel_err(eps_x, ref_x)
    rec = {'vs': 'oracle', 'what': 'denoiser forward at t = 1 on the B = 8 baseline sample, exact fp32 mode', 'rel_err_h': eh, 'rel_err_x': ex,
           'tol': tol, 'ok': bool(eh < tol and ex < tol)}
    if not rec['ok']:
        raise BenchRefused(f'the product path disagrees with the oracle on the baseline sample: rel err {eh:.3g} (h), {ex:.3g} (x) > {tol:g}')
    return rec


def cpu_baseline(workload='egnn_all_atom', ragged=False, B_scale=64, n_timed=15, with_c1=False):
    """the oracle (plain PyTorch fp32 CPU restatement of the reference path) on this box's host cores --
    `torch.set_num_threads(cores this process may use)`, the workload's shape at B = 1 and B = 8, 2 warm-up steps then `n_timed`
    timed steps each, median; `value` is the B = 8 median scaled to the B_scale batch.  `with_c1`: BASELINE configs[0] in full
    (dev_config: 60-node C-alpha pocket, 20-atom ligand, all 100 reverse steps) is timed as well.  The keypoints of the
    learned-encoder workloads come from the product encoder (run once on the GPU, outside the timed region): the baseline times
    the per-step denoiser path only, like `value`."""
    import torch
    from oracle import egnn as oegnn
    from oracle import gvp as ogvp
    from tests.util import to_obatch
    cpu = host_cpu()
    prev_threads = torch.get_num_threads()
    torch.set_num_threads(cpu['threads_used'])
    try:
        w = WORKLOADS[workload]
        T = w['T']
        enc_dev = 'cuda' if w['enc'] == 'learned' else 'cpu'
        model = build_model(enc_dev, workload)
        sd = {k[len('dynamics.'):]: v.detach().cpu() for k, v in model.state_dict().items() if k.startswith('dynamics.')}
        cfg = dict(w['dyn'], graph_cutoffs=w['cutoffs'])
        fwd = oegnn.egnn_dynamics_forward if w['arch'] == 'egnn' else ogvp.gvp_dynamics_forward
        cases = {}
        for B in (1, 8):
            n_rec, n_lig = (300, 25)
            if ragged:
                n_rec, n_lig = ragged_sizes(64, 0)
                n_rec, n_lig = n_rec[:B], n_lig[:B]
            g = build_batch(model, B, n_rec, n_lig, seed=99, device=enc_dev, workload=workload).to('cpu')
            cases[f'B{B}'] = _stats(_cpu_time_steps(fwd, sd, cfg, to_obatch(g), T, 2, n_timed), B)
            if B == 8:
                parity = product_vs_oracle(model, fwd, sd, cfg, g)
        out = {'value': cases['B8']['complex_steps_per_s'] / B_scale, 'unit': 'steps/s', 'cores': cpu['threads_used'], 'kind': 'port',
               'complex_steps_per_s': cases['B8']['complex_steps_per_s'], 'cases': cases, 'host': cpu,
               'cpu_seconds': sum(c['s_per_step_median'] * (c['timed_steps'] + 2) for c in cases.values()), 'parity': parity,
               'sample': f'oracle (plain PyTorch fp32 CPU restatement of the {workload} denoiser + update) at the '
                         f'{"ragged 150-600 / 15-35 atom" if ragged else "300 / 25 atom"} shape, B = 1 and B = 8, 2 warm-up + {n_timed} timed '
                         f'reverse steps each from the t = T state, median; value = the B = 8 rate scaled to the B = {B_scale} batch '
                         f'(BASELINE.md section 2)'}
        if with_c1:
            from keypoint_diffusion_amd import synth
            from keypoint_diffusion_amd import graph as G
            from keypoint_diffusion_amd.ligand_diffuser import KeypointDiffusion
            from tests import util
            cut = {'rr': 3.5, 'rk': 100, 'kk': 8, 'kl': 8, 'll': 9}                # configs/dev_config.yml:35
            m1 = KeypointDiffusion(10, 20, None, n_timesteps=100, architecture='egnn', rec_encoder_type='fixed',
                                   graph_config=dict(n_keypoints=20, graph_cutoffs=cut), dynamics_config=util.EGNN_DEV, precision=1e-5)
            synth.fill_state_dict_(m1, 0)
            g1 = m1.encode_receptors(G.batch(synth.synth_complexes([60], [20], 20, cut, seed=7, n_rec_feat=20, density=synth.CA_DENSITY)))
            sd1 = {k[len('dynamics.'):]: v.detach() for k, v in m1.state_dict().items() if k.startswith('dynamics.')}
            ts = _cpu_time_steps(oegnn.egnn_dynamics_forward, sd1, dict(util.EGNN_DEV, graph_cutoffs=cut), to_obatch(g1), 100, 2, 100)
            out['c1_dev_config'] = dict(_stats(ts, 1), total_s_100_steps=sum(ts),
                                        note='configs[0]: dev_config egnn (no keypoint update), 60-node C-alpha pocket, 20-atom ligand, all 100 reverse steps')
        return out
    finally:
        torch.set_num_threads(prev_threads)


def train_cpu_baseline(workload, B_sample=2):
    """Loss + torch autograd through the CPU oracle for B_sample complexes of the same shape (one step after a warm-up)."""
    import torch
    from oracle import egnn as oegnn
    from oracle import gvp as ogvp
    from tests.util import to_obatch
    w = WORKLOADS[workload]
    model = build_model('cpu', workload)
    g = build_batch(model, B_sample, 300, 25, seed=99, device='cpu', workload=workload)
    ob = to_obatch(g)
    sd = {k[len('dynamics.'):]: v.clone().requires_grad_(v.numel() > 0) for k, v in model.state_dict().items()
          if k.startswith('dynamics.')}
    cfg = dict(w['dyn'], graph_cutoffs=w['cutoffs'])
    fwd = oegnn.egnn_dynamics_forward if w['arch'] == 'egnn' else ogvp.gvp_dynamics_forward

    def one():
        eh, ex = fwd(sd, cfg, ob, torch.full((B_sample,), 0.5))
        (eh.square().sum() + ex.square().sum()).backward()

    one()
    t0 = time.perf_counter()
    one()
    dt = time.perf_counter() - t0
    return {'value': B_sample / dt / 64.0, 'unit': 'steps/s', 'cores': torch.get_num_threads(), 'kind': 'port',
            'complex_steps_per_s': B_sample / dt,
            'sample': f'oracle forward + torch autograd backward on {B_sample} complexes of the same 300/25 shape, 1 step after '
                      f'1 warm-up, scaled to the B=64 batch (no optimizer step on the CPU side)'}


# ---------------------------------------------------------------------------------------------------
# timed regions
# ---------------------------------------------------------------------------------------------------
def timed_regions(step, n_warmup, n_steps, repeats, dist, sync_tail=None, info=None):
    """W warm-up steps, then `repeats` regions of exactly `n_steps` steps, each bracketed by barrier + synchronize on
    both sides; returns the per-region wall times (seconds), MAX over ranks.  `info` (a dict) receives what a SCALE record
    needs to show the collective library saw every rank: `ranks_seen` (an all-reduce of ones over the process group) and
    `per_rank_ms_per_step` (each rank's own median region, all-gathered)."""
    import torch
    it = 0
    for _ in range(n_warmup):
        step(it)
        it += 1
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_steps):
            step(it)
            it += 1
        if sync_tail is not None:
            sync_tail()
        torch.cuda.synchronize()
        t_local = time.perf_counter() - t0
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0, t_local))
    local = [b for _, b in out]
    out = [a for a, _ in out]
    if dist is not None:
        backend_dev = 'cpu' if dist.get_backend() == 'gloo' else 'cuda'
        t = torch.tensor(out, device=backend_dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        out = t.cpu().tolist()
        if info is not None:
            ones = torch.ones(1, device=backend_dev, dtype=torch.float64)
            dist.all_reduce(ones)
            mine = torch.tensor([1e3 * statistics.median(local) / n_steps], device=backend_dev, dtype=torch.float64)
            every = [torch.zeros_like(mine) for _ in range(dist.get_world_size())]
            dist.all_gather(every, mine)
            info['ranks_seen'] = int(round(float(ones.item())))
            info['per_rank_ms_per_step'] = [float(e.item()) for e in every]
            info['backend'] = dist.get_backend()
    elif info is not None:
        info['ranks_seen'] = 1
        info['per_rank_ms_per_step'] = [1e3 * statistics.median(local) / n_steps]
        info['backend'] = None
    return out


def load_traffic(workload):
    for name in TRAFFIC_FILES:
        f = os.path.join(ROOT, 'profiles', name)
        if not os.path.exists(f):
            continue
        d = json.load(open(f))
        if workload in d:
            return d[workload].get('hbm_bytes_per_launch'), f'profiles/{name}[{workload}]'
        if workload == 'egnn_all_atom' and 'hbm_bytes_per_launch' in d:
            return d['hbm_bytes_per_launch'], f'profiles/{name}'
    return None, None


KERNEL_STATS_ROUNDS = ('r05', 'r04')      # profiles/<round>_kernel_stats_<workload>.csv: rocprofv3 --kernel-trace --stats of `bench.py --workload ...`


def load_kernel_stats(tag):
    """{kernel name up to '(': (calls, average ns)} from the newest committed rocprofv3 statistics of this workload, and the file's name."""
    import csv
    for rnd in KERNEL_STATS_ROUNDS:
        f = os.path.join(ROOT, 'profiles', f'{rnd}_kernel_stats_{tag}.csv')
        if os.path.exists(f):
            rows = {}
            for r in csv.DictReader(open(f)):
                name = r['Name'].split('(')[0].replace('void ', '').strip()
                rows[name] = (int(r['Calls']), float(r['AverageNs']))
            return rows, f'profiles/{rnd}_kernel_stats_{tag}.csv'
    return None, None


def hbm_kernel_report(arch, dyn, tag, B, NL, NK, counts, rec_nf):
    """the genuinely bandwidth-bound kernels of a reverse step -- graph build, embed / decode, sampler update -- each
    with its ALGORITHMIC bytes per launch (every array it must read or write, once; live sizes of this run), the rocprofv3 average
    duration of the committed statistics of the same command, achieved GB/s and the fraction of the 8 TB/s HBM peak.  They move a few
    MB per launch at most, so all of them are bounded by launch + memory LATENCY (a launch of 5 us cannot exceed bytes / 5 us), not by
    bandwidth: `regime` says so per kernel.  Together they are ~2 % of a step."""
    stats, src = load_kernel_stats(tag)
    if stats is None:
        return None
    F = 10
    E_ll, E_kl = counts['E_ll'], counts['E_kl']
    i4 = 4
    if arch == 'egnn':
        W = 264                                    # row stride of the 257-wide state
        emb_w_lig = (F * 64 + 64 + 64 * 256 + 256) * 4
        emb_w_kp = 0 if rec_nf == 256 else (rec_nf * 2 * rec_nf + 2 * rec_nf + 2 * rec_nf * 256 + 256) * 4
        table = [
            ('k_node_graph_index', 2, i4 * (NL + NK) / 2 + i4 * (B + 1)),
            ('k_ll_count', 1, 12 * NL + i4 * (B + 1) + i4 * NL + i4 * B),
            ('k_scan_graph_counts', 1, 3 * i4 * B),
            ('k_ll_fill', 1, 12 * NL + 2 * i4 * NL + i4 * (B + 1) + 2 * i4 * E_ll + i4 * (NL + 1)),
            ('k_kl_offsets', 1, 3 * i4 * (B + 1)),
            ('k_kl_build', 1, 12 * (NL + NK) + 2 * i4 * (B + 1) + 4 * i4 * E_kl + i4 * (NL + NK + 2)),
            ('k_egnn_meta', 1, 8 * i4 * B),
            ('k_embed', 2, (4 * F * NL + emb_w_lig + 4 * W * NL + 4 * rec_nf * NK + emb_w_kp + 4 * W * NK) / 2),
            ('k_decode', 1, 4 * W * NL + 24 * NL + (256 * 20 + 20 + 20 * F + F) * 4 + 4 * (F + 3) * NL),
            ('k_step_coef', 1, 3 * i4 * B + 4 * 8 * B),
            ('k_sample_update', 1, 4 * (3 + F) * NL * 4 + 2 * 12 * NK),
        ]
    else:
        S = dyn['n_hidden_scalars']
        table = [
            ('k_node_graph_index', 2, i4 * (NL + NK) / 2 + i4 * (B + 1)),
            ('k_ll_count', 1, 12 * NL + i4 * (B + 1) + i4 * NL + i4 * B),
            ('k_scan_graph_counts', 1, 3 * i4 * B),
            ('k_ll_fill', 1, 12 * NL + 2 * i4 * NL + i4 * (B + 1) + 2 * i4 * E_ll + i4 * (NL + 1)),
            ('k_kl_offsets', 1, 3 * i4 * (B + 1)),
            ('k_kl_build', 1, 12 * (NL + NK) + 2 * i4 * (B + 1) + 4 * i4 * E_kl + i4 * (NL + NK + 2)),
            ('k_egnn_meta', 1, 8 * i4 * B),
            ('k_gvp_embed', 2, (4 * F * NL + 4 * rec_nf * NK + ((F + 1) * S + (rec_nf + 1) * S + 6 * S) * 4 + 4 * S * (NL + NK)) / 2),
            ('k_step_coef', 1, 3 * i4 * B + 4 * 8 * B),
            ('k_sample_update', 1, 4 * (3 + F) * NL * 4 + 2 * 12 * NK),
        ]
    kernels, tot_b, tot_ns = {}, 0.0, 0.0
    for name, per_step, nbytes in table:
        hit = [v for k, v in stats.items() if k.split('::')[-1] == name]
        if not hit:
            continue
        ns = hit[0][1]
        gbs = nbytes / ns                                  # bytes / ns = GB/s
        kernels[name] = {'bytes': nbytes, 'avg_us': ns / 1e3, 'per_step': per_step, 'gb_s': gbs, 'frac': gbs / PEAK_HBM_GBS,
                         'regime': 'latency (a %.1f-us launch moving %.2f MB)' % (ns / 1e3, nbytes / 1e6) if gbs / PEAK_HBM_GBS < 0.10 else 'bandwidth'}
        tot_b += per_step * nbytes
        tot_ns += per_step * ns
    if not kernels:
        return None
    return {'kernels': kernels, 'bytes_per_step': tot_b, 'us_per_step': tot_ns / 1e3, 'gb_s': tot_b / tot_ns, 'frac': tot_b / tot_ns / PEAK_HBM_GBS,
            'peak': PEAK_HBM_GBS, 'unit': 'GB/s', 'durations_from': src, 'durations_measured_in_this_run': False,
            'note': 'algorithmic bytes per launch (live sizes) / rocprofv3 AverageNs of the committed statistics of the same command'}


def run_sampling(args, workload, device, rank, world, dist, B, n_rec, n_lig, ragged, gemm='f32', dump=None):
    """Steps/s of one sampling workload + the roofline of its dominant kernel.  Returns the result dict (rank 0) .
    `dump` (a directory): rank 0 writes the outputs of the last timed step there (dump_outputs)."""
    import torch
    from keypoint_diffusion_amd import graph as G
    w = WORKLOADS[workload]
    T = w['T']
    model = build_model(device, workload)
    g = build_batch(model, B, n_rec, n_lig, seed=1234 + rank * B, device=device, workload=workload)
    bidx = G.get_batch_idxs(g)
    model.dynamics.gemm_mode = gemm                    # explicit attribute: survives every engine rebuild (dynamics.engine())
    eng = model.dynamics.engine()
    assert eng.gemm_mode() == gemm, (eng.gemm_mode(), gemm)
    ones = torch.ones(B, device=device)
    # Random-init weights do not denoise: left to itself the chain drives the ligand atoms apart and
    # the lig-lig radius graph empties within ~20 steps, which would shrink the measured work.  Every
    # step therefore starts from the t = T state (x_0, h_0 ~ N(0, I), ligand COM removed: the complete
    # 600-edge lig-lig graph of SURVEY.md 8(d)); restoring it is three small device copies.
    lig, kp = g.nodes['lig'].data, g.nodes['kp'].data
    init = (lig['x_0'].clone(), lig['h_0'].clone(), kp['x_0'].clone())
    step_graph = None
    if args.graph:
        with torch.no_grad():
            step_graph = model.capture_step(g, bidx)
    # dump: what the last timed step hands its caller (the updated ligand coordinates / features and keypoint coordinates),
    # copied before the t = T state is restored
    last_timed = args.steps * args.repeats - 1 if dump else None
    timing, outputs = [False], {}

    def step(i):
        si = T - 1 - (i % T)
        if step_graph is not None:
            step_graph.step(si / T, (si + 1) / T)
        else:
            model.sample_p_zs_given_zt(ones * (si / T), ones * ((si + 1) / T), g, bidx)
        if timing[0] and i == last_timed:
            outputs.update(lig_x=lig['x_0'].clone(), lig_h=lig['h_0'].clone(), kp_x=kp['x_0'].clone())
        lig['x_0'].copy_(init[0]), lig['h_0'].copy_(init[1]), kp['x_0'].copy_(init[2])

    def tail():
        if dist is not None:
            from keypoint_diffusion_amd.dist import all_gather_ligands
            all_gather_ligands(g)

    with torch.no_grad():
        for i in range(args.warmup):
            step(i)
        torch.cuda.synchronize()
        eng.profile(True)
        rank_info = {}
        timing[0] = True
        regions = timed_regions(step, 0, args.steps, args.repeats, dist, tail, info=rank_info)
        timing[0] = False
        kern_ms, launches = eng.profile_read()
        eng.profile(False)
        counts = eng.last_counts()
    if rank != 0:
        return None
    if dump:
        dump_outputs(dump, outputs)
    med = statistics.median(regions)
    steps_per_s = world * args.steps / med
    # the event-timed dominant kernel must fit inside the wall time it is part of
    total_wall_ms = 1e3 * sum(regions)
    assert kern_ms <= total_wall_ms * 1.001, (kern_ms, total_wall_ms)
    e_all = counts['E_ll'] + counts['E_kl'] + counts['E_lk'] + counts['E_kk']
    n_launch_step = w['dyn']['n_layers'] if w['arch'] == 'egnn' else w['dyn']['n_convs']
    edges_per_step = (n_launch_step - 1) * e_all + counts['E_last']
    edges_per_launch = edges_per_step / n_launch_step
    avg_s = kern_ms / max(launches, 1) * 1e-3
    peak, bound = PEAK_F32_MATRIX_TFLOPS, 'mfma'
    if w['arch'] == 'egnn':
        kernel, f_exec, f_algo, b_algo = 'k_egnn_edge', EDGE_KERNEL_FLOP_PER_EDGE, EDGE_ALGO_FLOP_PER_EDGE, EDGE_ALGO_BYTES_PER_EDGE
        if gemm == 'f16x2':
            kernel, peak = 'k_egnn_edge_h', PEAK_F16_MATRIX_TFLOPS / 3.0
    else:
        kernel, f_exec, f_algo, b_algo = ('k_gvp_chain', gvp_chain_flop_per_edge(w['dyn']['n_hidden_scalars']), GVP_ALGO_FLOP_PER_EDGE,
                                          GVP_ALGO_BYTES_PER_EDGE)
        if gemm == 'f16x2':
            # the 256 x 256 products of the non-head message GVPs run split (3 f16 products each); heads, gates and vector parts stay fp32:
            # price the whole kernel against the f16 / 3 peak as for the EGNN edge kernel (a lower bound on the fraction)
            kernel, peak = 'k_gvp_chain<16, 1, 0>', PEAK_F16_MATRIX_TFLOPS / 3.0
    achieved = edges_per_launch * f_exec / avg_s / 1e12 if avg_s > 0 else 0.0
    hbm_gbs = edges_per_launch * b_algo / avg_s / 1e9 if avg_s > 0 else 0.0
    traffic, tsrc = load_traffic(workload + ('_ragged' if ragged else '') + ('_f16x2' if gemm != 'f32' else '')) if (B == 64 and (ragged or n_rec == 300)) else (None, None)
    shape = ('150-600', '15-35') if ragged else (n_rec, n_lig)
    desc = {'egnn_all_atom': 'egnn_all_atom dynamics (6 EGNN layers, hidden 256, update_kp_feat; fixed receptor encoder)',
            'egnn_40kp': 'egnn_40kp (learned EGNN receptor encoder -> 40 keypoints -> EGNN dynamics)',
            'gvp_40kp': 'gvp_40kp (learned GVP receptor encoder -> 40 keypoints -> GVP dynamics, 6 convs, 256 scalars / 16 vectors)',
            'gvp_all_atom': 'gvp_all_atom dynamics (6 GVP convs, 256 scalars / 16 vectors, message_norm mean; fixed receptor encoder)'}
    out = {
        'metric': 'denoising steps/sec', 'value': steps_per_s, 'unit': 'steps/s', 'n_gpus': world,
        'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': 1e3 * med / args.steps,
        'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
        'dtype': 'f32' if gemm == 'f32' else ('f32 via f16x2 split in the EGNN GEMMs (edge, projection, node update): 3 f16 MFMA products of '
                                              'hi/lo planes per fp32 product, f32 accumulate; everything else f32' if w['arch'] == 'egnn' else
                                              'f32 via f16x2 split in the 256 x 256 products of the message and update chains (k_gvp_chain, k_gvp_node_chain): 3 f16 MFMA products '
                                              'of hi/lo planes per fp32 product, f32 accumulate; everything else f32'),
        'data': 'synthetic',
        'config': {'workload': f'{desc[workload]}, batch of {B} synthetic {shape[0]}-atom pockets / {shape[1]}-atom ligands per GPU, '
                               f'T={T}, seeded random-init weights, every step taken from the t=T ligand state',
                   'batch_per_gpu': B, 'n_rec': 'U{150..600}' if ragged else n_rec, 'n_lig': 'U{15..35}' if ragged else n_lig,
                   'parallelism': f'dp{world}'},
        'repeats': {'n': args.repeats, 'ms_per_step': [1e3 * r / args.steps for r in regions], 'statistic': 'median',
                    'spread_pct': 100.0 * (max(regions) - min(regions)) / med},
        'ranks_seen': rank_info.get('ranks_seen'), 'per_rank_ms_per_step': rank_info.get('per_rank_ms_per_step'),
        'collective_backend': rank_info.get('backend'),
        'complex_steps_per_s': steps_per_s * B,
        'ligands_per_min_derived': steps_per_s * B * 60.0 / T,
        'edges_per_launch': {**counts, 'E_full_layer': e_all, 'launches_per_step': n_launch_step,
                             'mean_edges_per_launch': edges_per_launch},
        'roofline': {'kernel': kernel, 'bound': bound, 'achieved': achieved, 'peak': peak,
                     'unit': 'TFLOP/s', 'frac': achieved / peak,
                     'peak_note': 'dense fp32 MFMA peak' if gemm == 'f32' else 'dense f16 MFMA peak / 3 (three f16 products per useful fp32 product); '
                                  'achieved counts USEFUL flops (the same 265 kFLOP/edge as the exact kernel)',
                     'peak_measured': {'value': MEASURED_F32_MFMA_TFLOPS, 'unit': 'TFLOP/s', 'frac_of_it': achieved / MEASURED_F32_MFMA_TFLOPS,
                                       'source': 'profiles/r03_mfma_clock_trace.txt: bare fp32 MFMA loop on every CU, 64.0 cycles per MFMA at the 2.37 GHz '
                                                 'the part holds for seconds under that load (round 2 quoted 132 from launches inside the clock ramp: withdrawn)'},
                     'traffic': traffic,
                     'traffic_source': tsrc,
                     'traffic_unit': 'HBM bytes per launch (rocprofv3 PMC, 2 x FETCH_SIZE + WRITE_SIZE, separate passes; committed '
                                     'figure, not re-measured in this run)',
                     'avg_launch_ms': avg_s * 1e3, 'launches': launches, 'kernel_ms_total': kern_ms, 'wall_ms_total': total_wall_ms,
                     'flop_per_edge_executed': f_exec, 'flop_per_launch': edges_per_launch * f_exec,
                     'reference_formulation_tflops': edges_per_launch * f_algo / avg_s / 1e12 if avg_s > 0 else 0.0,
                     'hbm': {'achieved': hbm_gbs, 'peak': PEAK_HBM_GBS, 'unit': 'GB/s', 'frac': hbm_gbs / PEAK_HBM_GBS,
                             'bytes_per_launch': edges_per_launch * b_algo}},
    }
    if gemm == 'f32' and B == 64 and (ragged or n_rec == 300):
        rep = hbm_kernel_report(w['arch'], w['dyn'], workload + ('_ragged' if ragged else ''), B, int(g.num_nodes('lig')), int(g.num_nodes('kp')),
                                counts, int(g.nodes['kp'].data['h_0'].shape[1]))
        if rep:
            out['hbm_kernels'] = rep
    del model, g, eng
    torch.cuda.empty_cache()
    return out


def run_end_to_end(device, workload='egnn_all_atom', B=64, n_rec=300, n_lig=25, gemm='f32', ragged=False):
    """One full sampling run as test.py times it (reference test.py:149, 215-232): receptor encoding + T reverse steps of the
    whole batch + the copy of the sampled ligands to the host.  The receptor encoder is timed on its own as well (SURVEY.md
    8(d): "encoder timed separately"): `encoder_ms` is `encode_receptors` alone, synchronised on both sides.  With random-init
    weights the chain does not denoise (the ligand spreads and the lig-lig graph thins out), so this is a functional
    wall-clock figure, not the steady-state rate."""
    import gc
    import torch
    w = WORKLOADS[workload]
    model = build_model(device, workload)
    model.dynamics.gemm_mode = gemm
    assert model.dynamics.engine().gemm_mode() == gemm
    if ragged:
        n_rec, n_lig = ragged_sizes(B, 0)
    runs = []
    with torch.no_grad():
        for it in range(4):         # first pass = warm-up (workspace reservation, first-use initialisation); the MEDIAN of the other three counts
            g = raw_batch(B, n_rec, n_lig, 4321, device, workload)          # (a host hiccup -- allocator, collector -- once put 80 ms into a 1.5-ms encoder)
            if w['enc'] != 'learned':
                g = g.to(device)                   # resident before the clock starts, like `value`'s batch (raw_batch uploads the learned-encoder case itself)
            gc.collect()                           # (the previous pass's graphs and ligand lists: a collection of them inside the encoder's few ms read as 80 ms)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            enc = model.encode_receptors(g).to(device)
            torch.cuda.synchronize()
            t_enc = time.perf_counter() - t0
            pos, feat = model.sample_from_encoded_receptors(enc)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if it:
                runs.append((dt, t_enc))
    # median of the three timed passes for both figures (the contract `value` and the CPU baseline are medians too); the spread says
    # when a host hiccup sat in one of them
    dt = statistics.median(r[0] for r in runs)
    t_enc = statistics.median(r[1] for r in runs)
    spread = 100.0 * (max(r[0] for r in runs) - min(r[0] for r in runs)) / dt
    assert len(pos) == B and all(p.device.type == 'cpu' for p in pos)
    del model
    torch.cuda.empty_cache()
    return {'workload': workload + ('_ragged' if ragged else ''), 'gemm': gemm, 'ligands_per_min': 60.0 * B / dt, 'wall_s': dt,
            'encoder_ms': 1e3 * t_enc, 'reverse_loop_and_copy_s': dt - t_enc, 'steps_per_s_in_loop': w['T'] / (dt - t_enc),
            'n_ligands': B, 'n_timesteps': w['T'], 'runs_wall_s': [r[0] for r in runs], 'runs_encoder_ms': [1e3 * r[1] for r in runs],
            'statistic': 'median of 3 timed passes', 'spread_pct': spread,
            'includes': 'receptor encoding + all reverse steps (per-step graph rebuild, fresh noise) + final frame shift + '
                        'device->host copy of the ligands; model build and synthetic-data generation excluded',
            'note': 'random-init weights do not denoise: the ligand spreads over the loop and the lig-lig graph thins, so late '
                    'steps are cheaper than the t=T step the contract line times'}


# ---------------------------------------------------------------------------------------------------
# the ONE line the driver parses: contract fields + roofline + cpu_baseline, everything else as bare numbers
# ---------------------------------------------------------------------------------------------------
FULL_RECORD = os.path.join('gpurun_out', 'bench_full_record.json')      # relative to the repo root
ATTEST = {}                                                                # filled by main() (attest_environment)
COMPACT_LIMIT = 4096                                                       # bytes; the driver lost a 26.7 KB line in round 3


def _r(x, nd=5):
    """Round to `nd` significant digits (keeps the line short; the side file has full precision)."""
    if isinstance(x, bool) or x is None or isinstance(x, (int, str)):
        return x
    if isinstance(x, float):
        return float(f'{x:.{nd}g}')
    if isinstance(x, (list, tuple)):
        return [_r(v, nd) for v in x]
    return x


def compact_line(out, full_path=None):
    """The single JSON line bench.py prints: every contract field, `config`, `roofline` and `cpu_baseline` as the contract
    defines them, the secondary workloads reduced to `[steps_per_s, ms_per_step, roofline_frac]`, the end-to-end runs to
    `[ligands_per_min, encoder_ms]`.  Prose and per-case detail live in the side file `full_path`.  Pure function of the
    record (tests/test_bench_line.py feeds it a synthetic full record and bounds the length)."""
    cfg = out.get('config', {})
    line = {k: _r(out.get(k)) for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better',
                                        'scaling', 'vs_baseline')}
    dtype = str(out.get('dtype', 'f32'))
    line['dtype'] = dtype if len(dtype) <= 16 else dtype.split(' ', 1)[0] + ('+f16x2' if 'f16x2' in dtype else '')
    line['data'] = out.get('data', 'synthetic')
    wl = str(cfg.get('workload', ''))
    line['config'] = {'workload': wl if len(wl) <= 260 else wl[:257] + '...',
                      **{k: cfg[k] for k in ('batch_per_gpu', 'n_rec', 'n_lig', 'parallelism') if k in cfg}}
    rf = out.get('roofline')
    if rf:
        line['roofline'] = {k: _r(rf.get(k), 9 if k == 'traffic' else 5) for k in ('kernel', 'bound', 'achieved', 'peak', 'unit', 'frac', 'traffic',
                                                                                   'avg_launch_ms', 'launches', 'kernel_ms_total', 'wall_ms_total')}
        if 'hbm' in rf:
            line['roofline']['hbm_frac'] = _r(rf['hbm'].get('frac'))
        if 'edge_kernels' in rf:             # training lines: the two per-layer edge kernels by their own HIP events
            line['roofline']['edge_kernels'] = {k: [_r(v.get('avg_launch_ms')), _r(v.get('frac'), 4)] for k, v in rf['edge_kernels'].items()}
            line['roofline']['edge_kernels_fields'] = ['avg_launch_ms', 'frac']
    cb = out.get('cpu_baseline')
    if cb:
        host = cb.get('host', {})
        line['cpu_baseline'] = {'value': _r(cb.get('value')), 'unit': cb.get('unit'), 'cores': cb.get('cores'), 'kind': cb.get('kind'),
                                'sample': 'oracle reverse steps at the same shape, B=1 and B=8, 2 warm-up + %d timed each, median (spread = IQR/median); '
                                          'value = B=8 rate scaled to the batch' % max([c.get('timed_steps', 0) for c in cb['cases'].values()] + [0])
                                          if 'cases' in cb else str(cb.get('sample', ''))[:160],
                                'cpu_model': host.get('cpu_model'),
                                'cases': {k: _r(v.get('complex_steps_per_s')) for k, v in cb.get('cases', {}).items()},
                                'spread_pct': {k: _r(v.get('spread_pct'), 3) for k, v in cb.get('cases', {}).items()}}
        if cb.get('parity'):                 # the oracle as the checker of the measured path (product_vs_oracle): [rel err h, rel err x, tolerance]
            line['parity_vs_oracle'] = [_r(cb['parity'].get('rel_err_h'), 3), _r(cb['parity'].get('rel_err_x'), 3), cb['parity'].get('tol')]
        if 'c1_dev_config' in cb:
            line['cpu_baseline']['c1_total_s_100_steps'] = _r(cb['c1_dev_config'].get('total_s_100_steps'))
    if rf:
        line['roofline']['traffic_measured'] = bool(rf.get('traffic_measured', False))      # false: `traffic` is the committed PMC figure
    att = out.get('attest') or {}
    line['env'] = att.get('env', [])
    line['build'] = att.get('build', 'product')
    if not att.get('attested', True):
        line['attested'] = False                 # a --tools diagnostic run: never a contract line
    for k in ('gpu_over_cpu', 'complex_steps_per_s', 'ranks_seen', 'per_rank_ms_per_step', 'collective_backend'):
        if out.get(k) is not None:
            line[k] = _r(out[k])
    rep = out.get('repeats')
    if rep:
        line['repeats'] = {'n': rep.get('n'), 'spread_pct': _r(rep.get('spread_pct'), 3)}
    sec = out.get('secondary')
    if sec:
        line['secondary'] = {name: [_r(r.get('value')), _r(r.get('ms_per_step')), _r(r.get('roofline', {}).get('frac'), 4)]
                             for name, r in sec.items()}
        line['secondary_fields'] = ['steps_per_s', 'ms_per_step', 'roofline_frac']
    e2e = {}
    if out.get('end_to_end'):
        e2e[out['end_to_end'].get('workload', 'egnn_all_atom')] = out['end_to_end']
    for name, r in (out.get('end_to_end_more') or {}).items():
        e2e[name] = r
    if e2e:
        line['end_to_end'] = {name: [_r(r.get('ligands_per_min')), _r(r.get('encoder_ms')), r.get('n_timesteps'), _r(r.get('spread_pct'), 3)]
                              for name, r in e2e.items()}
        line['end_to_end_fields'] = ['ligands_per_min (median of 3)', 'encoder_ms', 'T', 'spread_pct']
    hk = out.get('hbm_kernels')
    if hk:
        # graph build + embed / decode + sampler update together, algorithmic bytes over rocprof time, fraction of 8 TB/s
        line['hbm_kernels_frac'] = _r(hk.get('frac'), 3)
        line['hbm_kernels_us_per_step'] = _r(hk.get('us_per_step'), 4)
    if out.get('ligands_per_min') is not None:
        line['ligands_per_min'] = _r(out['ligands_per_min'])
    if out.get('c1_gpu'):
        line['c1_gpu_s_100_steps'] = _r(out['c1_gpu'].get('total_s_100_steps'))
    if full_path:
        line['full_record'] = full_path
    return line


# ---------------------------------------------------------------------------------------------------
# --dump-outputs DIR: what the timed path computed in its last step, for comparing two builds output by output
# ---------------------------------------------------------------------------------------------------
DUMP_LIMIT = 64 << 20          # bytes of array data over all files of one dump


def dump_outputs(path, arrays, limit=DUMP_LIMIT):
    """Write `arrays` (name -> tensor or ndarray) as `path/<name>.npy`: float64 stays float64, everything else becomes float32.
    When the arrays together exceed `limit` bytes, every array keeps the same fraction of its elements, chosen by a generator
    seeded with 0 (flat indices, ascending): the same shapes give the same sample in every run.  Returns the files written."""
    import numpy as np
    host = {}
    for name, a in arrays.items():
        a = np.asarray(a.detach().cpu() if hasattr(a, 'detach') else a)
        host[name] = a if a.dtype == np.float64 else a.astype(np.float32)
    total = sum(a.nbytes for a in host.values())
    os.makedirs(path, exist_ok=True)
    files = []
    for name, a in host.items():
        if total > limit:
            keep = a.size * limit // total
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, keep, replace=False))]
        f = os.path.join(path, f'{name}.npy')
        np.save(f, a)
        files.append(f)
    print(f'bench.py: outputs of the last timed step -> {", ".join(files)}' + (f' (sampled to {limit} bytes of {total})' if total > limit else ''),
          file=sys.stderr, flush=True)
    return files


def emit(out):
    """Write the full record to the side file (best effort: a read-only tree must not lose the line) and print the compact line."""
    path = None
    out.setdefault('attest', dict(ATTEST))
    check_record(out)
    try:
        os.makedirs(os.path.join(ROOT, os.path.dirname(FULL_RECORD)), exist_ok=True)
        with open(os.path.join(ROOT, FULL_RECORD), 'w') as f:
            json.dump(out, f, indent=1)
        path = FULL_RECORD
    except OSError as e:
        print(f'bench.py: full record not written ({e})', file=sys.stderr)
    text = json.dumps(compact_line(out, path), separators=(',', ':'))
    if len(text) > COMPACT_LIMIT:                         # never again hand the driver a line it cannot take
        slim = compact_line({k: v for k, v in out.items() if k not in ('secondary', 'end_to_end_more')}, path)
        slim['dropped'] = 'secondary (line over %d bytes): see full_record' % COMPACT_LIMIT
        text = json.dumps(slim, separators=(',', ':'))
    sys.stdout.flush()
    print(text, flush=True)


def run_c1_gpu(device):
    """BASELINE.json configs[0] on the GPU: configs/dev_config.yml egnn dynamics (no keypoint update, kl_k 5, ll r 9), one synthetic C-alpha
    pocket of 60 nodes + a 20-atom ligand, all 100 reverse steps of one sampling run (encode + loop + host copy).  The CPU oracle's time for
    the same 100 steps is `cpu_baseline.c1_dev_config`.  B = 1: a latency figure, not a throughput one."""
    import torch
    from keypoint_diffusion_amd import graph as G
    from keypoint_diffusion_amd import synth
    from keypoint_diffusion_amd.ligand_diffuser import KeypointDiffusion
    from tests import util
    cut = {'rr': 3.5, 'rk': 100, 'kk': 8, 'kl': 8, 'll': 9}                # configs/dev_config.yml:35
    m1 = KeypointDiffusion(10, 20, None, n_timesteps=100, architecture='egnn', rec_encoder_type='fixed',
                           graph_config=dict(n_keypoints=20, graph_cutoffs=cut), dynamics_config=util.EGNN_DEV, precision=1e-5)
    synth.fill_state_dict_(m1, 0)
    m1 = m1.eval().to(device)
    times = []
    with torch.no_grad():
        for _ in range(3):          # first pass = warm-up
            g = G.batch(synth.synth_complexes([60], [20], 20, cut, seed=7, n_rec_feat=20, density=synth.CA_DENSITY))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pos, _ = m1.sample_from_encoded_receptors(m1.encode_receptors(g).to(device))
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
    assert len(pos) == 1 and tuple(pos[0].shape) == (20, 3)
    del m1
    torch.cuda.empty_cache()
    return {'total_s_100_steps': min(times[1:]), 'ms_per_step': 10.0 * min(times[1:]), 'runs_s': times,
            'note': 'configs[0] on the GPU: one 60-node C-alpha pocket, one 20-atom ligand, 100 reverse steps end to end (B = 1: latency-bound)'}


def run_train(args, device, rank, world, dist):
    """Secondary workloads: training steps/sec of the EGNN / GVP denoiser (fixed receptor encoder) on synthetic complexes."""
    import torch
    from keypoint_diffusion_amd import graph as G
    from keypoint_diffusion_amd import synth
    from keypoint_diffusion_amd.dist import allreduce_gradients
    w = WORKLOADS[args.workload]
    model = build_model(device, args.workload).train()
    # train.py:430 builds a plain torch.optim.Adam and :541-543 clips and steps; the product's drop-ins for the two calls (optim.py: one launch
    # each, same arithmetic -- tests/test_optim_gpu.py) are the default, --torch-optimizer keeps torch's, --fused-optimizer torch's fused=True
    from keypoint_diffusion_amd import optim as kpd_optim
    native_opt = not (args.torch_optimizer or args.fused_optimizer)
    if native_opt:
        opt, clip_grads = kpd_optim.Adam(model.parameters(), lr=1e-4), kpd_optim.clip_grad_value_
    else:
        opt = torch.optim.Adam(model.parameters(), lr=1e-4, fused=True) if args.fused_optimizer else torch.optim.Adam(model.parameters(), lr=1e-4)
        clip_grads = torch.nn.utils.clip_grad_value_
    B = args.batch
    template = raw_batch(B, args.n_rec, args.n_lig, 1234 + rank * B, device, args.workload).to(device)
    last = [None]
    enc_weight = 0.1 if w['enc'] == 'learned' else 0.0      # train.py adds the encoder loss with its configured weight

    def step(i):
        g = template.to(device)             # fresh container over the same device tensors (forward re-binds node data)
        losses = model(g, None)
        opt.zero_grad(set_to_none=True)
        (losses['l2'] + enc_weight * losses['rec_encoder'] if enc_weight else losses['l2']).backward()
        if dist is not None:
            allreduce_gradients(list(model.parameters()))
        clip_grads(model.parameters(), 1.0)
        opt.step()
        last[0] = losses

    rank_info = {}
    for i in range(args.warmup):
        step(i)
    torch.cuda.synchronize()
    trainer = model.dynamics._trainer()[0] if hasattr(model.dynamics, '_trainer') else None
    egnn_prof = w['arch'] == 'egnn' and trainer is not None and hasattr(trainer, 'profile')
    if egnn_prof:
        trainer.profile(True)
    regions = timed_regions(step, 0, args.steps, args.repeats, dist, info=rank_info)
    if rank == 0 and args.dump_outputs:
        # what the last timed step hands its caller: the loss terms of KeypointDiffusion.forward and the parameters after the Adam update
        losses = {f'loss_{k}': v for k, v in last[0].items() if v is not None}
        dump_outputs(args.dump_outputs, dict(losses, parameters=torch.cat([p.detach().reshape(-1) for p in model.parameters()])))
    if rank == 0:
        med = statistics.median(regions)
        n_steps_total = args.steps * args.repeats
        out = {'metric': 'training steps/sec', 'value': world * args.steps / med, 'unit': 'steps/s', 'n_gpus': world,
               'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': 1e3 * med / args.steps, 'higher_is_better': True,
               'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
               'config': {'workload': f'{args.workload}: loss + backward + clip + Adam on {w["arch"]}_{"40kp (learned encoder, encoder + optimal-transport loss included)" if w["enc"] == "learned" else "all_atom"} (6 layers, hidden 256, '
                                      f'training mode), batch of {B} '
                                      f'synthetic {args.n_rec}-atom pockets / {args.n_lig}-atom ligands per GPU, one bucketed gradient all-reduce per step when N > 1',
                          'batch_per_gpu': B, 'parallelism': f'dp{world}',
                          'optimizer': 'keypoint_diffusion_amd.optim.Adam + clip_grad_value_ (kpd_adam_step)' if native_opt else
                                       f'torch.optim.Adam{"(fused=True)" if args.fused_optimizer else ""} + torch.nn.utils.clip_grad_value_'},
               'repeats': {'n': args.repeats, 'ms_per_step': [1e3 * r / args.steps for r in regions], 'statistic': 'median',
                           'spread_pct': 100.0 * (max(regions) - min(regions)) / med},
               'complex_steps_per_s': world * args.steps / med * B, 'final_l2': float(last[0]['l2'].detach()),
               'ranks_seen': rank_info.get('ranks_seen'), 'per_rank_ms_per_step': rank_info.get('per_rank_ms_per_step')}
        # ---- roofline of the step: executed FLOPs of the denoiser's forward (the same accounting as the sampling lines: first Linears per
        # node) x 3 (backward = one product for the input gradient and one for the weight gradient per forward product) over the step time,
        # against the dense fp32 MFMA peak; beside it the two per-layer edge kernels of the EGNN trainer by their own HIP events
        NL, NK = int(template.num_nodes('lig')), int(template.num_nodes('rec')) if w['enc'] == 'fixed' else B * w['n_kp']      # fixed encoder: kp := rec
        L = w['dyn']['n_layers'] if w['arch'] == 'egnn' else w['dyn']['n_convs']
        if w['arch'] == 'egnn':
            prof = trainer.profile_read() if egnn_prof else None
            if egnn_prof:
                trainer.profile(False)
            edges_step = prof['fwd'][2] / max(n_steps_total, 1) if prof else 0.0
            f_edge = edges_step * EDGE_KERNEL_FLOP_PER_EDGE
            f_proj = 2 * 257 * 257 * ((L - 1) * 8 * (NL + NK) + 6 * NL + 2 * NK)
            f_node = 2 * (514 * 257 + 257 * 257) * ((L - 1) * (NL + NK) + NL)
            f_fwd = f_edge + f_proj + f_node
        else:
            c = trainer.last_counts() if hasattr(trainer, 'last_counts') else dict(E_ll=0, E_kl=0, E_lk=0, E_kk=0)
            S = w['dyn']['n_hidden_scalars']
            e_all, e_last = c['E_ll'] + c['E_kl'] + c['E_lk'] + c['E_kk'], c['E_ll'] + c['E_kl']
            edges_step = (L - 1) * e_all + e_last
            f_edge = edges_step * gvp_chain_flop_per_edge(S)
            f_proj = 2 * S * S * ((L - 1) * 2 * (NL + NK) + NL + NK)          # h_src block of the first message Linear, per source node and edge type
            f_node = 301.2e3 * ((L - 1) * (NL + NK) + NL)                      # two update GVPs per destination node
            f_fwd = f_edge + f_proj + f_node
        f_step = 3.0 * f_fwd
        t_step = med / args.steps
        ach = f_step / t_step / 1e12
        rf = {'kernel': 'whole training step (forward + backward + clip + Adam)', 'bound': 'mfma', 'achieved': ach, 'peak': PEAK_F32_MATRIX_TFLOPS,
              'unit': 'TFLOP/s', 'frac': ach / PEAK_F32_MATRIX_TFLOPS, 'traffic': None, 'traffic_measured': False,
              'flop_per_step_executed': f_step, 'flop_forward_executed': f_fwd, 'flop_forward_parts': {'edge': f_edge, 'projections': f_proj, 'node': f_node},
              'edges_per_step': edges_step, 'avg_launch_ms': 1e3 * t_step, 'launches': n_steps_total, 'kernel_ms_total': 1e3 * sum(regions),
              'wall_ms_total': 1e3 * sum(regions),
              'note': 'executed FLOPs = 3 x the forward (first Linears counted per node, as the kernels compute them); optimizer, loss and the '
                      'encoder of the keypoint models are in the time but not in the FLOPs, so frac is a lower bound'}
        if w['arch'] == 'egnn' and egnn_prof and prof['fwd'][1] and prof['bwd'][1]:
            kern = {}
            for tag, name in (('fwd', 'k_egnn_edge_train'), ('bwd', 'k_egnn_edge_bwd')):
                ms, n_l, edges = prof[tag]
                a_k = edges * EDGE_KERNEL_FLOP_PER_EDGE / (ms * 1e-3) / 1e12          # both kernels run the 257 x 257 products of both branches once
                kern[name] = {'avg_launch_ms': ms / n_l, 'launches': n_l, 'achieved': a_k, 'frac': a_k / PEAK_F32_MATRIX_TFLOPS,
                              'ms_per_step': ms / n_steps_total}
            rf['edge_kernels'] = kern
            assert sum(k['ms_per_step'] for k in kern.values()) <= 1e3 * t_step * 1.001
        out['roofline'] = rf
        if world == 1 and args.full and not args.no_cpu_baseline and w['enc'] == 'fixed':
            out['cpu_baseline'] = train_cpu_baseline(args.workload)
        emit(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=None, help='timed steps per region (default 200; 20 for the training workloads)')
    ap.add_argument('--warmup', type=int, default=None, help='untimed warm-up steps (default 20; 3 for the training workloads)')
    ap.add_argument('--repeats', type=int, default=3, help='timed regions of --steps steps each; the median is reported')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--n-rec', type=int, default=300)
    ap.add_argument('--n-lig', type=int, default=25)
    ap.add_argument('--full', action='store_true', help='at N = 1, also measure what takes runs of its own: the CPU baseline with its '
                                                        'parity check and, for the contract workload, the secondary workloads and the '
                                                        'end-to-end runs (off: only the timed steps of the line)')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the CPU baseline and its parity check')
    ap.add_argument('--fused-optimizer', action='store_true', help='training workloads: torch.optim.Adam(fused=True)')
    ap.add_argument('--torch-optimizer', action='store_true', help='training workloads: torch.optim.Adam + torch.nn.utils.clip_grad_value_ instead '
                                                                   'of keypoint_diffusion_amd.optim (one launch each)')
    ap.add_argument('--no-secondary', action='store_true', help='with --full: skip the configs[0] / configs[2] / configs[4]-shape / end-to-end '
                                                                'measurements')
    ap.add_argument('--workload', default='egnn_all_atom', choices=list(WORKLOADS),
                    help='egnn_all_atom = BASELINE.json configs[1] (the contract line); the others are secondary')
    ap.add_argument('--gemm', default='f32', choices=['f32', 'f16x2'],
                    help='f32 = exact fp32 MFMA everywhere (the contract line); f16x2 = opt-in split-f16 products in the EGNN GEMMs')
    ap.add_argument('--graph', action='store_true', help='replay the reverse step as a captured HIP graph (StepGraph)')
    ap.add_argument('--ragged', action='store_true', help='pockets 150-600 atoms, ligands 15-35 atoms (configs[4] shape)')
    ap.add_argument('--tools', action='store_true', help='diagnostic run (profiles/tools): KPD_* switches and the TOOLS build of the library are '
                                                         'allowed; the line then carries "attested": false and is not a contract line')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32 / float64, '
                         'at most 64 MB; rank 0): ligand coordinates and features and keypoint coordinates of a sampling workload, '
                         'the loss terms and updated parameters of a training workload')
    args = ap.parse_args()
    training = args.workload.endswith('_train')
    if args.steps is None:
        args.steps = 20 if training else 200
    if args.warmup is None:
        args.warmup = 3 if training else 20

    # N ranks without a launcher: start them here, before anything in this process touches the GPU
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        sys.exit(spawn_ranks(args.gpus))

    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if os.environ.get('KPD_BENCH_SPAWN_ECHO') == '1':        # launcher self-test (tests/test_bench_launch.py): no GPU, no torch
        print(json.dumps({'rank': rank, 'local_rank': local_rank, 'world': world, 'gpus': args.gpus,
                          'master': os.environ.get('MASTER_ADDR'), 'port': os.environ.get('MASTER_PORT')}), flush=True)
        return
    import torch
    if world != args.gpus:
        raise SystemExit(f'bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks')
    if world > 1:
        # N ranks share one host: each takes its share of the cores for the synthetic-batch generation and the torch-side
        # setup, instead of N x all-cores thread pools oversubscribing the box while the others wait in the first barrier
        torch.set_num_threads(rank_cpu_threads(host_cpu()['threads_used'], int(os.environ.get('LOCAL_WORLD_SIZE', world))))
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs a GPU: the hot path has no CPU implementation')
    # KPD_BENCH_SHARE_GPU=1 (functional rehearsal on a one-GPU box only): every rank uses cuda:0 and the
    # process group runs over gloo, because RCCL refuses two ranks on one device
    share = os.environ.get('KPD_BENCH_SHARE_GPU') == '1'
    if share:
        local_rank = 0
    elif local_rank >= torch.cuda.device_count():
        raise SystemExit(f'bench.py: rank {rank} needs cuda:{local_rank} but only {torch.cuda.device_count()} device(s) are visible '
                         f'(KPD_BENCH_SHARE_GPU=1 rehearses N ranks on one GPU over gloo)')
    torch.cuda.set_device(local_rank)
    device = torch.device('cuda', local_rank)
    dist = None
    # KPD_BENCH_DIST_AT_1=1: a ONE-rank job still initialises RCCL and takes the distributed branch (tests/test_nccl_gpu.py)
    if world > 1 or os.environ.get('KPD_BENCH_DIST_AT_1') == '1':
        import torch.distributed as dist
        if share:
            dist.init_process_group('gloo')
        else:
            dist.init_process_group('nccl', device_id=device)
        assert dist.get_world_size() == args.gpus

    from keypoint_diffusion_amd import hip
    ATTEST.update(attest_environment(os.environ, int(hip.lib().kpd_build_flags()), allow_tools=args.tools))
    torch.manual_seed(1000 + rank)
    if training:
        run_train(args, device, rank, world, dist)
        if dist is not None:
            dist.destroy_process_group()
        return

    n_rec, n_lig = args.n_rec, args.n_lig
    if args.ragged:
        n_rec, n_lig = ragged_sizes(args.batch, rank)
    out = run_sampling(args, args.workload, device, rank, world, dist, args.batch, n_rec, n_lig, args.ragged, gemm=args.gemm,
                       dump=args.dump_outputs)
    if rank == 0:
        default_line = args.workload == 'egnn_all_atom' and not args.ragged and not args.graph and args.gemm == 'f32'
        if world == 1 and args.full and not args.no_cpu_baseline:
            out['cpu_baseline'] = cpu_baseline(args.workload, ragged=args.ragged, B_scale=args.batch, with_c1=default_line)
            out['gpu_over_cpu'] = out['value'] / out['cpu_baseline']['value']
        if world == 1 and args.full and default_line and not args.no_secondary:
            # BASELINE.json configs[2] and the configs[4] shape, same method (shorter regions), each with its roofline
            sec_args = argparse.Namespace(**vars(args))
            sec_args.steps, sec_args.warmup = max(20, args.steps // 2), max(5, args.warmup // 2)
            sec = {}
            for name, wl, ragged in (('gvp_40kp', 'gvp_40kp', False), ('gvp_all_atom_ragged', 'gvp_all_atom', True)):
                nr, nl = ragged_sizes(64, 0) if ragged else (300, 25)
                r = run_sampling(sec_args, wl, device, 0, 1, None, 64, nr, nl, ragged)
                if not args.no_cpu_baseline:
                    r['cpu_baseline'] = cpu_baseline(wl, ragged=ragged)
                    r['gpu_over_cpu'] = r['value'] / r['cpu_baseline']['value']
                sec[name] = r
            # configs[3] / configs[4] at their stated batch of 512 on this ONE GPU (the 8-GPU jobs shard it 64 per rank): per-complex
            # cost beside the B = 64 lines above (flat from 64 up means the 8-way shard loses nothing to small batches)
            big_args = argparse.Namespace(**vars(sec_args))
            big_args.steps, big_args.warmup = max(10, args.steps // 8), 3
            r = run_sampling(big_args, 'egnn_all_atom', device, 0, 1, None, 512, 300, 25, False)
            r['per_complex_us'] = 1e3 * r['ms_per_step'] / 512
            r['per_complex_us_at_B64'] = 1e3 * out['ms_per_step'] / 64
            sec['egnn_all_atom_b512'] = r
            nr, nl = ragged_sizes(512, 0)
            r = run_sampling(big_args, 'gvp_all_atom', device, 0, 1, None, 512, nr, nl, True)
            r['per_complex_us'] = 1e3 * r['ms_per_step'] / 512
            r['per_complex_us_at_B64'] = 1e3 * sec['gvp_all_atom_ragged']['ms_per_step'] / 64
            sec['gvp_all_atom_ragged_b512'] = r
            # the contract workload once more in the opt-in f16x2 mode (separately judged; parity suite runs in both modes)
            r = run_sampling(sec_args, 'egnn_all_atom', device, 0, 1, None, 64, 300, 25, False, gemm='f16x2')
            if 'cpu_baseline' in out:
                r['cpu_baseline'] = out['cpu_baseline']
                r['gpu_over_cpu'] = r['value'] / out['cpu_baseline']['value']
            r['end_to_end'] = run_end_to_end(device, gemm='f16x2')
            sec['egnn_all_atom_f16x2'] = r
            for name, wl, ragged in (('gvp_40kp_f16x2', 'gvp_40kp', False), ('gvp_all_atom_ragged_f16x2', 'gvp_all_atom', True)):
                nr, nl = ragged_sizes(64, 0) if ragged else (300, 25)
                r = run_sampling(sec_args, wl, device, 0, 1, None, 64, nr, nl, ragged, gemm='f16x2')
                base = sec[name[:-len('_f16x2')]]
                if 'cpu_baseline' in base:
                    r['cpu_baseline'] = base['cpu_baseline']
                    r['gpu_over_cpu'] = r['value'] / base['cpu_baseline']['value']
                sec[name] = r
            out['secondary'] = sec
            out['end_to_end'] = run_end_to_end(device)
            out['ligands_per_min'] = out['end_to_end']['ligands_per_min']
            # configs[2] (learned encoder timed on its own) and the configs[4] shape at its own T = 1000, exact mode
            out['c1_gpu'] = run_c1_gpu(device)
            out['end_to_end_more'] = {'gvp_40kp': run_end_to_end(device, 'gvp_40kp'),
                                      'gvp_all_atom_ragged': run_end_to_end(device, 'gvp_all_atom', ragged=True)}
        emit(out)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
