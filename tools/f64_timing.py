"""Timing of the fp64 mode next to the fp32 per-phase path (profiles/f64_NOTES.md): one cfg2-shaped chunk
(MDRFF, I = 302, D = 13, K = 10, 1024 features) and one cfg4-shaped chunk (MDNN [128, 128], I = 232, D = 32,
K = 4), 1000 pairs, 100 updates of minibatch 100.  HIP events bracket the whole run_training call as enqueued:
the per-call staging (widening / copying x and y on the device, the id upload, begin), the 100 updates and the 6
held-out evaluations -- so "us / update" is the call's time over 100, not kernel time alone, and host enqueue
time shows where the host is the slower side.  Median, minimum and maximum of 9 calls after a warm-up call.
The GEMM share of the fp64 call is the time of its updates' products alone (same shapes, operand forms and
gathers, replayed through bsig_gemm_f64 on scratch operands) over the call's: a rough figure."""
import ctypes as C
import os
import sys

os.environ['BSIG_NO_PERSISTENT'] = '1'      # the fp32 side: its per-phase kernels
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import bayes_sim_ig_amd as B
from bayes_sim_ig_amd import _lib

DEV = 'cuda:0'
SHAPES = {
    'cfg2-shaped': dict(cls='MDRFF', i=302, d=13, k=10, n_feat=1024),
    'cfg4-shaped': dict(cls='MDNN', i=232, d=32, k=4, hidden=(128, 128)),
}
N, NU, BATCH = 1000, 100, 100


def timed(fn, reps=9):
    """(median, min, max) in us"""
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b) * 1e3)
    return float(np.median(t)), min(t), max(t)


def model(sh, dtype):
    kw = dict(input_dim=sh['i'], output_dim=sh['d'], output_lows=np.zeros(sh['d']), output_highs=np.ones(sh['d']),
              n_gaussians=sh['k'], full_covariance=False, lr=1e-3, activation=torch.nn.Tanh, device=DEV)
    torch.manual_seed(0)
    np.random.seed(0)
    if sh['cls'] == 'MDRFF':
        m = B.MDRFF(n_feat=sh['n_feat'], sigma=4.0, **kw)
    else:
        m = B.MDNN(hidden_layers=sh['hidden'], **kw)
    return m.double() if dtype == 'float64' else m


def gemm_set(sh):
    """The products of one fp64 update (forward, backward) as bsig_gemm_f64 calls on scratch operands."""
    lib = _lib.load()
    nh = sh['k'] * (1 + 2 * sh['d'])
    r = lambda *s: torch.randn(*s, dtype=torch.float64, device=DEV)
    ids = torch.randint(0, 800, (BATCH,), dtype=torch.int32, device=DEV)
    calls = []

    def add(a, a_km, a_rows, b, b_km, b_rows, m, n, k):
        c = torch.empty(m, n, dtype=torch.float64, device=DEV)
        calls.append((a, a_km, a_rows, b, b_km, b_rows, c, m, n, k))
    if sh['cls'] == 'MDRFF':
        f = sh['n_feat']
        feats, w, d_o = r(N, f), r(nh, f), r(BATCH, nh)
        add(feats, 0, ids, w, 0, None, BATCH, nh, f)
        add(d_o, 1, None, feats, 1, ids, nh, f, BATCH)
    else:
        i, h = sh['i'], 128
        x, w1, w2, wh = r(N, i), r(h, i), r(h, h), r(nh, h)
        h1, h2, d_o, dz = r(BATCH, h), r(BATCH, h), r(BATCH, nh), r(BATCH, h)
        add(x, 0, ids, w1, 0, None, BATCH, h, i)
        add(h1, 0, None, w2, 0, None, BATCH, h, h)
        add(h2, 0, None, wh, 0, None, BATCH, nh, h)
        add(d_o, 0, None, wh, 1, None, BATCH, h, nh)
        add(d_o, 1, None, h2, 1, None, nh, h, BATCH)
        add(dz, 0, None, w2, 1, None, BATCH, h, h)
        add(dz, 1, None, h1, 1, None, h, h, BATCH)
        add(dz, 1, None, x, 1, ids, h, i, BATCH)

    def run():
        st = _lib.stream()
        for _ in range(NU):
            for a, a_km, a_rows, b, b_km, b_rows, c, m, n, k in calls:
                _lib.check(lib.bsig_gemm_f64(_lib.ptr(a), a.stride(0), a_km, _lib.ptr(a_rows), _lib.ptr(b),
                                             b.stride(0), b_km, _lib.ptr(b_rows), _lib.ptr(c), n, m, n, k, 0, 0,
                                             None, None, 0, 1.0, st))
    return run


def main():
    _lib.require_gpu()
    B.MDNN.VERBOSE = False
    for name, sh in SHAPES.items():
        g = torch.Generator().manual_seed(1)
        x = (torch.randn(N, sh['i'], generator=g) * 0.3).to(DEV)
        y = torch.rand(N, sh['d'], generator=g).to(DEV)
        ids = np.random.RandomState(2).randint(0, 800, (NU, BATCH))
        out = {}
        for dtype in ('float32', 'float64'):
            m = model(sh, dtype)
            assert not m._may_time_out()
            out[dtype] = timed(lambda: m.run_training(x, y, NU, BATCH, ids_table=ids, _defer=True))
        gemm = timed(gemm_set(sh))
        fmt = lambda t: '%.1f (%.1f .. %.1f)' % tuple(v / NU for v in t)
        print('%s, us/update median (min .. max): fp32 per-phase %s, fp64 %s (x%.1f), fp64 GEMMs of the updates '
              '%s = %.0f %% of the fp64 call' % (name, fmt(out['float32']), fmt(out['float64']),
                                                 out['float64'][0] / out['float32'][0], fmt(gemm),
                                                 100 * gemm[0] / out['float64'][0]))


if __name__ == '__main__':
    main()
