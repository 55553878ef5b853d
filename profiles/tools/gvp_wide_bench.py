"""The wide GVP denoiser (csrc/gvp_wide.hip) at B = 64 x (300-atom pocket, 25-atom ligand), the gvp_all_atom settings of bench.py (fixed
encoder, 6 convs, message_norm 'mean', ll radius 6, kl kNN 7, update_kp, 3 / 2 / 4 message / update / noise GVPs, 16 vector channels),
n_hidden_scalars 384 and 512: forward time from device events (3 warm-up forwards, then `--reps` timed ones: mean / min / max),
executed GEMM FLOPs per forward from the shapes and the live edge counts, the fraction of the 157.3 TFLOP/s fp32 MFMA bound, the bytes
the gather / vector-channel / aggregation kernels move, and the reserved workspace.  Kernel table:
`rocprofv3 --kernel-trace --stats -- python profiles/tools/gvp_wide_bench.py` in a run of its own.  One JSON line per width."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from keypoint_diffusion_amd import synth
from keypoint_diffusion_amd.dynamics_gvp import LigRecDynamicsGVP
from tests import util

PEAK = 157.3e12
GVP_ALL_ATOM = dict(vector_size=16, n_convs=6, message_norm='mean', update_kp=True, ll_k=0, kl_k=7, n_message_gvps=3, n_update_gvps=2,
                    n_noise_gvps=4, dropout=0.0)


def gvp_cost(M, si, so, vi, vo):
    """GEMM FLOPs of one GVP over M rows (scalar products: [s | |Vh|] -> so and the gate so -> vo), and the bytes its vector-channel
    kernels move (v_in read; Vh, Vu, |Vh| written; gate product read; V written)."""
    h = max(vi, vo)
    flops = 2 * M * so * (si + h) + 2 * M * vo * so
    byts = 4 * M * (3 * vi + 3 * h + 3 * vo + h) + 4 * M * (vo + 3 * vo + 3 * vo)
    return flops, byts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--widths', default='384,512')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--B', type=int, default=64)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    B, n_rec, n_lig, V = a.B, 300, 25, 16
    g = util.fixed_encode(util.make_batch([n_rec] * B, [n_lig] * B), n_vec=V).to(dev)
    t = torch.rand(B, device=dev)
    for S in [int(w) for w in a.widths.split(',')]:
        cfg = dict(GVP_ALL_ATOM, n_hidden_scalars=S)
        model = synth.fill_state_dict_(LigRecDynamicsGVP(10, 10, graph_cutoffs=util.CUTOFFS_ALL_ATOM, **cfg), 3).eval().to(dev)
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
        Sw = (S + 3) & ~3
        n = [B * n_lig, B * n_rec]
        E = [c['E_ll'], c['E_kl'], c['E_lk'], c['E_kk']]
        src, dst = [0, 1, 0, 1], [0, 0, 1, 1]
        flops = 2 * (n[0] * 12 + n[1] * 12) * Sw                                        # encoders ([h | t] padded to 12 columns)
        gather = vec = agg = 0
        for ci in range(cfg['n_convs']):
            last = ci == cfg['n_convs'] - 1
            ets = [0, 1] if last else [0, 1, 2, 3]
            for et in ets:
                flops += 2 * n[src[et]] * Sw * Sw                                         # s_src block, once per source node
                gather += 4 * E[et] * (2 * Sw + 3 * (V + 1))                              # P row read, pre row and vin written
                f, b = gvp_cost(E[et], 0, Sw, V + 1, V)                                   # head: |Vh| block + gate
                flops += f; vec += b
                for _ in range(cfg['n_message_gvps'] - 1):
                    f, b = gvp_cost(E[et], Sw, Sw, V, V)
                    flops += f; vec += b
                agg += 4 * E[et] * (Sw + 3 * V)                                           # the message rows, read once
            for nt in ([0] if last else [0, 1]):
                for _ in range(cfg['n_update_gvps']):
                    f, b = gvp_cost(n[nt], Sw, Sw, V, V)
                    flops += f; vec += b
        for j in range(cfg['n_noise_gvps']):
            lastg = j == cfg['n_noise_gvps'] - 1
            f, b = gvp_cost(n[0], Sw, 64 if lastg else Sw, V, 1 if lastg else V)
            flops += f; vec += b
        mean = sum(ms) / len(ms)
        print(json.dumps(dict(n_hidden_scalars=S, B=B, ms_mean=round(mean, 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3),
                              forwards_per_s=round(1e3 / mean, 2), tflop_per_step=round(flops / 1e12, 3),
                              frac_mfma_bound=round(flops / (mean * 1e-3) / PEAK, 3), gather_gb=round(gather / 1e9, 2),
                              vector_kernel_gb=round(vec / 1e9, 2), agg_gb=round(agg / 1e9, 2), ws_bytes=int(ws),
                              edges=dict(zip(['ll', 'kl', 'lk', 'kk'], E)))), flush=True)
        del model, eng
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
