"""Timing of the kernel mean embedding kernel (include/bsig_kme.h, csrc/kme.h) for profiles/kme_NOTES.md, by the
method of tools/signature_ex_timing.py: HIP events, a warm-up, median and range of REPS repeats, the kernels of a
comparison alternating in one process, N = 32 000 trajectories, n_feat 256.
  (i)  kernel time in fp32 and in double for Pendulum (3, 1, T 21), Ant (60, 8, T 50 and T 200) and ShadowHand
       (211, 20, T 50), each next to two yardsticks on the same trajectories: the UNFUSED composition of kernels
       the project had before -- the rows written out (bsig_kme_rows), bsig_rff_project on [N M, d], a mean over
       t (torch), in slices of trajectories whose projected rows take SLICE_BYTES at most -- and copy_rows moving
       the fused kernel's algorithmic bytes (trajectories in, rows out), the HBM bound.  No read-back in any of
       them (check_finite=False).
  (ii) --fit: pairs per second of BayesSim.fit (wall clock around the whole call, summaries included) on
       FIT_PAIRS Ant-shaped synthetic pairs with summary_kme (256 inputs), summary_xcorr (K 0, 600 inputs) and
       summary_corrdiff (11 802 inputs), alternating, and what bsig_fit_is_persistent answers for each plan.
  (iii) --pmc TASK fp32|fp64: the fused launch of one shape of (i) alone, five times, for a counter pass
       (tools/pmc_pass.sh runs it once per counter)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import bayes_sim_ig_amd as B
from tools.csrc_hash import csrc_hash
from tools.signature_ex_timing import DEV, REPS, timed

N = 32000
N_FEAT = 256
FIT_PAIRS = 32000
FIT_REPS = 3
SLICE_BYTES = 1 << 30
SHAPES = (('Pendulum', 3, 1, 21), ('Ant', 60, 8, 50), ('Ant200', 60, 8, 200), ('ShadowHand', 211, 20, 50))


def inputs(sd, ad, length, dtype):
    gen = torch.Generator().manual_seed(0)
    states = torch.randn(N, length, sd, generator=gen).to(DEV).to(dtype)
    actions = torch.rand(N, length, ad, generator=gen).to(DEV).to(dtype)
    emb = B.KernelMeanEmbedding(sd, ad, n_feat=N_FEAT, device=DEV).fit_scale(states, actions, dtype=dtype)
    return states, actions, emb


def unfused(emb, states, actions, out, prec, ws):
    """The same rows from the kernels the project had before: rows out, projection, mean over t, in slices."""
    lib, _lib = B._lib.load(), B._lib
    n, length, _ = states.shape
    steps, m, d = length - 1, emb.n_feat // 2, emb.row_dim
    coeff = emb.coefficients(prec.dtype)
    per = max(1, min(n, SLICE_BYTES // (steps * emb.n_feat * prec.itemsize)))
    for lo in range(0, n, per):
        hi = min(n, lo + per)
        x = emb.rows(states[lo:hi], actions[lo:hi], dtype=prec.dtype)
        feats = torch.empty(((hi - lo) * steps, emb.n_feat), dtype=prec.dtype, device=x.device)
        if prec.itemsize == 4:
            _lib.check(lib.bsig_rff_project(_lib.ptr(x), x.stride(0), None, _lib.ptr(coeff), coeff.stride(0), None,
                                            _lib.ptr(feats), emb.n_feat, x.shape[0], d, m, float(np.sqrt(1.0 / m)),
                                            0, _lib.ptr(ws), ws.numel() * 4, _lib.stream()))
        else:
            _lib.check(lib.bsig_rff_project_f64(_lib.ptr(x), x.stride(0), None, _lib.ptr(coeff), coeff.stride(0),
                                                None, _lib.ptr(feats), emb.n_feat, x.shape[0], d, m,
                                                float(np.sqrt(1.0 / m)), 0, _lib.stream()))
        torch.mean(feats.view(hi - lo, steps, emb.n_feat), dim=1, out=out[lo:hi, :emb.n_feat])


def kernel_times():
    lib = B._lib.load()
    print('(i) N = %d, n_feat %d; us: median (min .. max) of %d repeats; bytes: trajectories in + rows out'
          % (N, N_FEAT, REPS))
    for task, sd, ad, length in SHAPES:
        for dtype in (torch.float32, torch.float64):
            prec = B._lib.F64 if dtype == torch.float64 else B._lib.F32
            if prec.itemsize == 8 and task == 'Ant200':
                continue                                   # (3 GB of double trajectories: the fp32 figure is the point)
            states, actions, emb = inputs(sd, ad, length, dtype)
            quad = 16 // prec.itemsize
            out = torch.empty(N, B._lib.round_up(N_FEAT, quad), dtype=dtype, device=DEV)
            out_u = torch.empty_like(out)
            steps, d = length - 1, emb.row_dim
            per = max(1, min(N, SLICE_BYTES // (steps * N_FEAT * prec.itemsize)))
            ws = torch.empty(max(int(lib.bsig_gemm_workspace_bytes(per * steps, N_FEAT // 2, d)) // 4 + 1, 1),
                             dtype=torch.float32, device=DEV)
            elems = length * (sd + ad) + N_FEAT
            half = B._lib.round_up((elems + 1) // 2, quad)
            src = torch.randn(N, half, device=DEV).to(dtype)
            dst = torch.empty_like(src)
            fns = {
                'fused': lambda: emb(states, actions, out=out, check_finite=False, dtype=dtype),
                'unfused': lambda: unfused(emb, states, actions, out_u, prec, ws),
                'copy': lambda: prec.copy_rows(B._lib.ptr(src), half, None, B._lib.ptr(dst), half, N, half,
                                               B._lib.stream()),
            }
            res = timed(fns, reps=REPS if task != 'Ant200' else 5)
            gap = float((out[:, :N_FEAT] - out_u[:, :N_FEAT]).abs().max())
            nbytes = float(elems) * prec.itemsize * N
            flops = 2.0 * N * steps * d * N_FEAT / 2
            group = lib.bsig_kme_group(length, length, sd, ad, N_FEAT // 2, 1, 0, prec.itemsize)
            print('  %s T %d %s: d %d, %d a workgroup, %.1f MB, %.2f GFLOP of z: fused %.0f (%.0f .. %.0f) = %.2f TB/s, '
                  '%.1f TFLOP/s; unfused (slices of %d) %.0f (%.0f .. %.0f); copy_rows %.0f (%.0f .. %.0f); '
                  'fused / unfused = %.3f, fused / copy = %.1f; largest |fused - unfused| %.2g'
                  % ((task, length, 'fp64' if prec.itemsize == 8 else 'fp32', d, group, nbytes / 1e6, flops / 1e9) +
                     res['fused'] + (nbytes / res['fused'][0] / 1e6, flops / res['fused'][0] / 1e6, per) +
                     res['unfused'] + res['copy'] +
                     (res['fused'][0] / res['unfused'][0], res['fused'][0] / res['copy'][0], gap)), flush=True)
            del states, actions, emb, out, out_u, src, dst, ws
            torch.cuda.empty_cache()


def one_shape(task, precision):
    sd, ad, length = {name: (sd, ad, length) for name, sd, ad, length in SHAPES}[task]
    dtype = torch.float64 if precision == 'fp64' else torch.float32
    states, actions, emb = inputs(sd, ad, length, dtype)
    out = torch.empty(N, N_FEAT, dtype=dtype, device=DEV)
    for _ in range(5):
        emb(states, actions, out=out, check_finite=False, dtype=dtype)
    torch.cuda.synchronize()


def fit_throughput():
    sd, ad, length = 60, 8, 50
    gen = torch.Generator().manual_seed(1)
    theta = (0.01 + 1.99 * torch.rand(FIT_PAIRS, 2, generator=gen)).to(DEV)
    states = (torch.randn(FIT_PAIRS, length, sd, generator=gen) * theta[:, :1].cpu().view(-1, 1, 1)).to(DEV)
    actions = torch.rand(FIT_PAIRS, length, ad, generator=gen).to(DEV)
    B.MDNN.VERBOSE = False
    models = {}
    for name in ('summary_kme', 'summary_xcorr', 'summary_corrdiff'):
        cfg = {'modelClass': 'MDNN', 'summarizerFxn': name, 'trainTrajLen': length, 'components': 5,
               'hiddenLayers': (128, 128), 'lr': 1e-3}
        torch.manual_seed(11)
        models[name] = B.BayesSim(model_cfg=cfg, obs_dim=sd, act_dim=ad, params_dim=2,
                                  params_lows=np.array([0.01, 0.01]), params_highs=np.array([2.0, 2.0]),
                                  prior=None, device=DEV)
    times = {name: [] for name in models}
    for rep in range(FIT_REPS + 1):                    # the first round warms up (plans, graphs, the scale)
        for name, bs in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            logs = bs.fit(theta, states, actions)
            torch.cuda.synchronize()
            if rep:
                times[name].append(FIT_PAIRS / (time.perf_counter() - t0))
            assert np.isfinite(logs[-1]['train_loss']).all()
    print('(ii) BayesSim.fit on %d Ant-shaped synthetic pairs (sd 60, ad 8, T 50), MDNN (128, 128), 5 components: '
          'pairs per second, median and range of %d fits, alternating' % (FIT_PAIRS, FIT_REPS))
    for name, bs in models.items():
        model = bs.model
        code = int(model._plan_prec.is_persistent(model._plan)) if model._plan is not None else -1
        v = times[name]
        print('  %s, %d inputs: %.0f pairs/s (%.0f .. %.0f); bsig_fit_is_persistent: %d'
              % (name, model.input_dim, float(np.median(v)), min(v), max(v), code))
    med = {k: float(np.median(v)) for k, v in times.items()}
    print('  kme / xcorr = %.2f, kme / corrdiff = %.2f' % (med['summary_kme'] / med['summary_xcorr'],
                                                         med['summary_kme'] / med['summary_corrdiff']))


def main(argv):
    print('# csrc: %s' % csrc_hash())
    print('# %s' % torch.cuda.get_device_name(0))
    if '--pmc' in argv:
        task, precision = argv[argv.index('--pmc') + 1:][:2]
        one_shape(task, precision)
    elif '--fit' in argv:
        fit_throughput()
    else:
        kernel_times()


if __name__ == '__main__':
    main(sys.argv[1:])
