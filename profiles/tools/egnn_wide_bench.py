"""The wide EGNN denoiser (csrc/egnn_wide.hip) at B = 64 x (300-atom pocket, 25-atom ligand), egnn_all_atom graph settings (fixed
encoder, ll radius 6, kl kNN 5, update_kp_feat, 6 layers), hidden_nf 384 and 512: forward time from device events (3 warm-up forwards,
then `--reps` timed ones: mean / min / max), executed GEMM FLOPs per forward from the shapes and the live edge counts, the fraction of
the 157.3 TFLOP/s fp32 MFMA bound, the bytes the gather / head / aggregation kernels move, and the reserved workspace.  Kernel table:
`rocprofv3 --kernel-trace --stats -- python profiles/tools/egnn_wide_bench.py` in a run of its own.  One JSON line per width."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from keypoint_diffusion_amd import synth
from keypoint_diffusion_amd.dynamics import LigRecDynamics
from tests import util

PEAK = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--widths', default='384,512')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--B', type=int, default=64)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    B, n_rec, n_lig = a.B, 300, 25
    g = util.fixed_encode(util.make_batch([n_rec] * B, [n_lig] * B)).to(dev)
    t = torch.rand(B, device=dev)
    for H in [int(w) for w in a.widths.split(',')]:
        cfg = dict(util.EGNN_C2, hidden_nf=H)
        model = synth.fill_state_dict_(LigRecDynamics(10, 10, graph_cutoffs=util.CUTOFFS_ALL_ATOM, **cfg), 3).eval().to(dev)
        with torch.no_grad():
            for _ in range(3):
                model(g, t, None)
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                model(g, t, None)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
        eng = model.engine()
        c = eng.last_counts()
        ws = float(eng.debug('ws_bytes', 1)[0])
        L, W, LDW = cfg['n_layers'], H + 1, (H + 4) & ~3
        n_l, n_k = B * n_lig, B * n_rec
        E = [c['E_ll'], c['E_kl'], c['E_lk'], c['E_kk']]
        flops = byts = 0
        for li in range(L):
            last = li == L - 1
            ets = [0, 1] if last else [0, 1, 2, 3]
            slots_l, slots_k = (6, 2) if last else (8, 8)
            flops += 2 * (n_l * slots_l + n_k * slots_k) * LDW * LDW                        # projections
            for et in ets:
                flops += 2 * 2 * E[et] * LDW * LDW                                          # second Linear, both branches
                byts += 2 * E[et] * LDW * 4 * (2 + 1)                                       # gather: P_src + P_dst rows read, A1 written
                byts += 2 * E[et] * LDW * 4                                                 # heads: A2 read
                byts += E[et] * LDW * 4                                                     # aggregation: A2 (edge branch) read
            for n in ([n_l] if last else [n_l, n_k]):
                flops += 2 * n * (2 * LDW * LDW + LDW * LDW)                                # node MLP
        mean = sum(ms) / len(ms)
        print(json.dumps(dict(hidden_nf=H, B=B, ms_mean=round(mean, 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3),
                              forwards_per_s=round(1e3 / mean, 2), tflop_per_step=round(flops / 1e12, 3),
                              frac_mfma_bound=round(flops / (mean * 1e-3) / PEAK, 3), edge_kernel_gb=round(byts / 1e9, 2),
                              ws_bytes=int(ws), edges=dict(zip(['ll', 'kl', 'lk', 'kk'], E)))), flush=True)
        del model, eng
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
