"""Timing of the split-bf16 matmul precision next to the fp32 route (profiles/split_bf16_NOTES.md), the two
modes alternating in one process, HIP events, warm-up, median and range of REPS repeats:
  1. the RFF projection at the fit's block shape, 32 000 x 2310 -> 2048 frequencies (cfg5), and at the
     per-chunk shape 800 x 2310 -> 2048 (bsig_rff_project_ex);
  2. the head forward product 8192 x 260 x 4096 (rows gathered, bias epilogue) and the head gradient
     dW = dO^T X[ids], 260 x 4096 x 8192, of the same update (bsig_gemm_f32_ex; dO at the pitch ceil16(260)) --
     with BSIG_SPLIT_BF16_EVERYWHERE=1: gemm_run leaves this class of shapes on the fp32 kernels because of
     what is measured here;
  3. one scaled-batch update end to end: cfg5-shaped MDRFF (I = 2310, 4096 features, D = 32, K = 4),
     20 000 pairs as one chunk, minibatch 8192 -- the difference of a 12-update and a 4-update
     run_training call over 8 (the calls share the staging, the feature cache and the evaluations' count
     differs by one: a rough per-update figure) -- twice: as a user gets it (the rule active: projection on
     the split kernel, the two head products on the fp32 kernels) and with BSIG_SPLIT_BF16_EVERYWHERE=1
     (the split kernel in both head products);
  4. 100 updates of the per-phase path on the cfg4 shape (MDNN [128, 128], I = 232, D = 32, K = 4,
     minibatch 100, 1000 pairs): the small products.
TFLOP/s are fp32-equivalent: 2 m n k over the time, whatever the kernel multiplies."""
import ctypes as C
import os
import sys

os.environ['BSIG_NO_PERSISTENT'] = '1'      # the per-phase kernels: the persistent ones are not touched by the mode
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import bayes_sim_ig_amd as B
from bayes_sim_ig_amd import _lib

DEV = 'cuda:0'
REPS = 21
MODES = ('float32', 'split_bf16')


def timed_pair(fns, reps=REPS, warm=3):
    """{mode: (median, min, max)} in us; the modes alternate inside every repeat"""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t[k].append(a.elapsed_time(b) * 1e3)
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in t.items()}


def report(name, res, flops=None, path=None):
    f32, spl = res['float32'], res['split_bf16']
    line = '%s: fp32 %.1f us (%.1f .. %.1f), split_bf16 %.1f us (%.1f .. %.1f), split / fp32 = %.3f' % (
        (name,) + f32 + spl + (spl[0] / f32[0],))
    if flops:
        line += '; %.1f -> %.1f TFLOP/s fp32-equivalent' % (flops / f32[0] / 1e6, flops / spl[0] / 1e6)
    if path:
        line += '; split kernel: tile %d, %d K slices of %d, %d workgroups' % (path[1], path[3], path[4], path[5])
    print(line, flush=True)


def gemm_path(m, n, k, akm, bkm, gathered, epi, ws_bytes):
    out = (C.c_int32 * 8)()
    _lib.check(_lib.load().bsig_debug_gemm_path(m, n, k, akm, bkm, gathered, epi, ws_bytes, 1, out))
    assert out[0] == _lib.GEMM_PATH_SPLIT_BF16, list(out)
    return list(out)


def projection(rows, d=2310, mf=2048):
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(rows, d, generator=g) * 0.3).to(DEV)
    coeff = torch.zeros(mf, _lib.round_up(d, 4))
    coeff[:, :d] = torch.randn(mf, d, generator=g) / 4.0
    coeff = coeff.to(DEV)
    feats = torch.empty(rows, 2 * mf, device=DEV)
    ws_bytes = int(lib.bsig_gemm_workspace_bytes(rows, mf, d))
    ws = torch.empty(ws_bytes // 4 + 1, device=DEV)

    def run(matmul):
        _lib.check(lib.bsig_rff_project_ex(_lib.ptr(x), x.stride(0), None, _lib.ptr(coeff), coeff.stride(0), None,
                                           _lib.ptr(feats), feats.stride(0), rows, d, mf, 0.02, 0, _lib.ptr(ws),
                                           ws_bytes, _lib.stream(), matmul))
    res = timed_pair({'float32': lambda: run(0), 'split_bf16': lambda: run(1)})
    report('RFF projection %d x %d -> %d' % (rows, d, mf), res, 2.0 * rows * d * mf,
           gemm_path(rows, mf, d, 0, 0, 0, _lib.EPI_COS_SIN, ws_bytes))


def head_products(batch=8192, nh=260, f=4096, pool=40000):
    lib = _lib.load()
    x = torch.randn(pool, f, device=DEV)
    ids = torch.randint(0, pool, (batch,), device=DEV, dtype=torch.int32)
    w, bias = torch.randn(nh, f, device=DEV), torch.randn(nh, device=DEV)
    ld_o = _lib.round_up(nh, 16)
    o = torch.empty(batch, ld_o, device=DEV)
    d_o = torch.randn(batch, ld_o, device=DEV)
    dw = torch.empty(nh, f, device=DEV)
    ws_bytes = max(int(lib.bsig_gemm_workspace_bytes(batch, nh, f)), int(lib.bsig_gemm_workspace_bytes(nh, f, batch)))
    ws = torch.empty(ws_bytes // 4 + 1, device=DEV)

    def fwd(matmul):
        _lib.check(lib.bsig_gemm_f32_ex(_lib.ptr(x), f, 0, _lib.ptr(ids), _lib.ptr(w), f, 0, None, _lib.ptr(o), ld_o,
                                        batch, nh, f, _lib.EPI_BIAS, 0, _lib.ptr(bias), None, 0, 1.0, _lib.ptr(ws),
                                        ws_bytes, _lib.stream(), matmul))

    def grad(matmul):
        _lib.check(lib.bsig_gemm_f32_ex(_lib.ptr(d_o), ld_o, 1, None, _lib.ptr(x), f, 1, _lib.ptr(ids), _lib.ptr(dw), f,
                                        nh, f, batch, _lib.EPI_NONE, 0, None, None, 0, 1.0, _lib.ptr(ws), ws_bytes,
                                        _lib.stream(), matmul))
    flops = 2.0 * batch * nh * f
    report('head forward %d x %d x %d (gathered rows, bias)' % (batch, nh, f),
           timed_pair({'float32': lambda: fwd(0), 'split_bf16': lambda: fwd(1)}), flops,
           gemm_path(batch, nh, f, 0, 0, 1, _lib.EPI_BIAS, ws_bytes))
    report('head gradient %d x %d x %d (gathered contraction rows)' % (nh, f, batch),
           timed_pair({'float32': lambda: grad(0), 'split_bf16': lambda: grad(1)}), flops,
           gemm_path(nh, f, batch, 1, 1, 1, _lib.EPI_NONE, ws_bytes))


def model(cls, i, d, k, precision, **kw):
    args = dict(input_dim=i, output_dim=d, output_lows=np.zeros(d), output_highs=np.ones(d), n_gaussians=k,
                full_covariance=False, lr=1e-3, activation=torch.nn.Tanh, device=DEV)
    torch.manual_seed(0)
    np.random.seed(0)
    m = B.MDRFF(**args, **kw) if cls == 'MDRFF' else B.MDNN(**args, **kw)
    return m.set_matmul_precision(precision)


def scaled_update(label, n=20000, batch=8192, i=2310, d=32, k=4, reps=REPS):
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(n, i, generator=g) * 0.3).to(DEV)
    y = torch.rand(n, d, generator=g).to(DEV)
    models = {p: model('MDRFF', i, d, k, p, n_feat=4096, sigma=4.0) for p in MODES}
    ids = {nu: np.random.RandomState(2).randint(0, int(n * 0.8), (nu, batch)) for nu in (4, 12)}
    res = {}
    for nu in (4, 12):
        res[nu] = timed_pair({p: (lambda p=p, nu=nu: models[p].run_training(x, y, nu, batch, ids_table=ids[nu], _defer=True))
                              for p in MODES}, reps=reps, warm=2)
        assert all(not m._may_time_out() for m in models.values())
    per = {p: tuple((res[12][p][j] - res[4][p][0]) / 8 for j in range(3)) for p in MODES}
    report('scaled-batch update, %s (cfg5 shape, minibatch %d), (12-update call - median 4-update call) / 8'
           % (label, batch), per)
    for nu in (4, 12):
        report('  the %d-update run_training call as a whole' % nu, res[nu])


def small_updates(n=1000, nu=100, batch=100, i=232, d=32, k=4):
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(n, i, generator=g) * 0.3).to(DEV)
    y = torch.rand(n, d, generator=g).to(DEV)
    ids = np.random.RandomState(2).randint(0, 800, (nu, batch))
    models = {p: model('MDNN', i, d, k, p, hidden_layers=(128, 128)) for p in MODES}
    res = timed_pair({p: (lambda p=p: models[p].run_training(x, y, nu, batch, ids_table=ids, _defer=True)) for p in MODES})
    assert all(not m._may_time_out() for m in models.values())
    report('%d per-phase updates, cfg4 shape (MDNN [128, 128], I = %d, minibatch %d), the run_training call' % (nu, i, batch), res)


def main():
    _lib.require_gpu()
    B.MDNN.VERBOSE = False
    what = sys.argv[1:] or ['projection', 'head', 'scaled', 'small']
    if 'projection' in what:
        projection(32000)
        projection(800)
    if 'head' in what:
        # the class of shapes gemm_run leaves on the fp32 kernels: measured with the rule switched off
        os.environ['BSIG_SPLIT_BF16_EVERYWHERE'] = '1'
        head_products()
        del os.environ['BSIG_SPLIT_BF16_EVERYWHERE']
    if 'scaled' in what:
        scaled_update('head products on the fp32 kernels (the rule, what a user gets)')
        os.environ['BSIG_SPLIT_BF16_EVERYWHERE'] = '1'
        scaled_update('split kernel in both head products (rule off)')
        del os.environ['BSIG_SPLIT_BF16_EVERYWHERE']
    if 'small' in what:
        small_updates()


if __name__ == '__main__':
    main()
