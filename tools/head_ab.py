#!/usr/bin/env python3
"""A/B of two builds of the library (BSIG_LIB_PATH) over the mixture-density head's thread-per-component rows
(csrc/mdn_row.h: mdn_nll_kernel<FULL>, full_row of the persistent MDNN kernel, mdn_nll_f64_kernel<FULL>) and the
forward() tuple kernel.  Two builds that print the same lines compute the same bits.

default (MI355X): one line per case with a sha256 over the bytes of loss, d_out and the flag word.
  fp32: every row of tests/head_cases.py CASES at eps 0, at 1e-5 with injected noise and at 1e-5 with Philox draws; a
        dominant logit (softmax outputs under MIN_WEIGHT) with a small ll_limit and a large min_weight;
        bsig_mdn_head_outputs and bsig_mdn_nll_from_tuple on the thread-per-component rows; loss and every gradient
        (the head bias column sums among them) of MDNN.loss_and_grad on a full-covariance model.
  persist: one full-covariance chunk of the persistent MDNN kernel at the shape of
        tests/test_gpu_persistent_mdnn.py::test_full_covariance_chunk_matches_oracle: logs and final flat weights.
  fp64: HEAD_CASES of tests/test_gpu_f64.py with the same variants, outputs, tuple loss and loss_and_grad.
--dump FILE (MI355X): the fp64 losses and d_out arrays at eps = 0, and the persistent chunk's logs and final weights,
  into an .npz.
cmp A.npz B.npz: two dumps.  fp64: the diagonal d mu / d pre columns may differ by at most 5 ulp (the two builds may
  associate g_lp z / sigma differently: two roundings of one real value each), everything else -- losses, logit
  gradients, full covariance -- by nothing; asserts.  The persistent chunk's differences are printed.
--time (MI355X): HIP events, 9 repetitions after a warm-up, every repetition in us: the `full` and `diag` rows of
  head_cases.py at batch 1025 through bsig_mdn_head_nll, and the full-covariance persistent chunk.
usage: [BSIG_LIB_PATH=...] python tools/head_ab.py [--dump FILE | --time] | cmp A.npz B.npz"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
DEV = 'cuda:0'
SEED, STREAM = 0x5EED1234ABCD, 77
# (batch, D, K, full, a thread-per-component row); HEAD_CASES of tests/test_gpu_f64.py
F64_CASES = [c + (True,) for c in [(9, 3, 4, False), (7, 2, 10, False), (5, 1, 1, False), (9, 4, 3, True), (9, 5, 3, True),
                                   (33, 13, 10, False), (7, 49, 10, False), (7, 32, 10, True), (5, 8, 64, False)]]
PERSIST = (6, 5, 'summary_corrdiff', 7, 3, 12)      # (d, k, summarizer, sd, ad, t)


def cmp(pa, pb):
    a, b = np.load(pa), np.load(pb)
    worst = 0
    for key in a.files:
        if key.startswith('persist_'):      # reported, not asserted: the chunk test's tolerance is its bound
            scale = np.abs(a[key]).max()
            print('%-22s max |a - b| / max |a| = %.3g (%d of %d values differ)'
                  % (key, np.abs(a[key] - b[key]).max() / scale, int((a[key] != b[key]).sum()), a[key].size))
            continue
        d, k, full = [int(v) for v in key.split('_')[1:4]]
        x, y = a[key].view(np.int64), b[key].view(np.int64)
        ulp = np.abs(x - y)
        loose = np.zeros(x.shape[-1], bool)
        if key.startswith('dout_') and not full:
            loose[k:k + 2 * d * k] = True                 # d mu, d pre of the diagonal rows
        worst = max(worst, int(ulp.max()))
        print('%-22s max ulp %d (diagonal d mu / d pre), %d elsewhere'
              % (key, ulp[..., loose].max() if loose.any() else 0, ulp[..., ~loose].max()))
        assert ulp[..., ~loose].max() == 0 and (not loose.any() or ulp[..., loose].max() <= 5), key
    print('cmp ok: largest difference %d ulp' % worst)


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


class Head:
    """the C entry points of one precision on device tensors"""

    def __init__(self, B, torch, f64):
        self.B, self.torch, self.f64, self.L, self.lib = B, torch, f64, B._lib, B._lib.load()
        self.dt = torch.float64 if f64 else torch.float32

    def dims(self, d, k, full, eps, min_w=1e-5, ll=1e5):
        hd = self.L.HeadDims()
        hd.out_dim, hd.n_comp, hd.full_cov = d, k, int(full)
        hd.eps_noise, hd.min_weight, hd.ll_limit = eps, min_w, ll
        self.hy = self.L.F64Hyper(1e-3, 0.9, 0.999, 1e-8, eps, min_w, ll, 0.0)
        return hd

    def ws(self, hd, b):
        fn = self.lib.bsig_head_workspace_bytes_f64 if self.f64 else self.lib.bsig_head_workspace_bytes
        return self.torch.empty(int(fn(C.byref(hd), b)) // 4 + 64, device=DEV)

    def pre(self, hd):
        return (C.byref(hd), C.byref(self.hy)) if self.f64 else (C.byref(hd),)

    def data(self, b, d, k, full, seed=0):
        torch = self.torch
        nh = k + 2 * d * k + (d * (d - 1) // 2 if full else 0) * k
        gen = torch.Generator().manual_seed(b * 7 + d * 131 + k + seed)
        o = torch.randn(b, nh, generator=gen, dtype=torch.float64) * 0.5
        o[:, :k] *= 6.0
        y = torch.rand(b, d, generator=gen, dtype=torch.float64)
        noise = torch.rand(b, d, k, generator=gen, dtype=torch.float64)
        return [t.to(self.dt).to(DEV) for t in (o, y, noise)]

    def nll(self, hd, o, y, noise, seed=0, sid=0):
        torch, L = self.torch, self.L
        b, nh = o.shape
        loss = torch.full((1,), float('nan'), dtype=self.dt, device=DEV)
        d_o = torch.full((b, nh), float('nan'), dtype=self.dt, device=DEV)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        ws = self.ws(hd, b)
        fn = self.lib.bsig_mdn_head_nll_f64 if self.f64 else self.lib.bsig_mdn_head_nll
        L.check(fn(*self.pre(hd), L.ptr(o), nh, L.ptr(y), y.shape[1], None, b, b, L.ptr(noise), seed, sid, L.ptr(loss),
                   L.ptr(d_o), L.ptr(flag), L.ptr(ws), ws.numel() * 4, L.stream()))
        torch.cuda.synchronize()
        return loss, d_o, flag

    def outputs_and_tuple(self, hd, o, y, noise, d, k, full):
        torch, L = self.torch, self.L
        b = o.shape[0]
        ls = d * (d - 1) // 2 if full else 0
        outs = [torch.full((b, n), float('nan'), dtype=self.dt, device=DEV) for n in (k, d * k, d * k, max(ls * k, 1))]
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        loss = torch.full((1,), float('nan'), dtype=self.dt, device=DEV)
        ws = self.ws(hd, b)
        fn = self.lib.bsig_mdn_head_outputs_f64 if self.f64 else self.lib.bsig_mdn_head_outputs
        L.check(fn(*self.pre(hd), L.ptr(o), o.shape[1], b, L.ptr(noise), SEED, STREAM, L.ptr(outs[0]), L.ptr(outs[1]),
                   L.ptr(outs[2]), L.ptr(outs[3]) if full else None, L.ptr(flag), L.ptr(ws), ws.numel() * 4, L.stream()))
        fn = self.lib.bsig_mdn_nll_from_tuple_f64 if self.f64 else self.lib.bsig_mdn_nll_from_tuple
        L.check(fn(*self.pre(hd), L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(outs[2]), L.ptr(outs[3]) if full else None,
                   L.ptr(y), d, b, L.ptr(loss), L.ptr(flag), L.ptr(ws), ws.numel() * 4, L.stream()))
        torch.cuda.synchronize()
        return outs + [loss, flag]

    def model_grads(self):
        """loss and every gradient of a small full-covariance MDNN (head bias gradients: the finish kernel's sums)"""
        torch, B = self.torch, self.B
        d, k, inp, b = 4, 3, 12, 37
        torch.manual_seed(5)
        m = B.MDNN(device=DEV, input_dim=inp, output_dim=d, n_gaussians=k, full_covariance=True, hidden_layers=(16,),
                   lr=1e-3, output_lows=np.zeros(d), output_highs=np.ones(d), activation=torch.nn.Tanh)
        if self.f64:
            m = m.double()
        gen = torch.Generator().manual_seed(6)
        x, y = torch.randn(b, inp, generator=gen, dtype=torch.float64), torch.rand(b, d, generator=gen, dtype=torch.float64)
        noise = torch.rand(b, d, k, generator=gen, dtype=torch.float64)
        B.MDNN.EPS_NOISE = 1e-5
        loss = m.loss_and_grad(x.to(self.dt).to(DEV), y.to(self.dt).to(DEV), noise=noise.to(self.dt).to(DEV))
        torch.cuda.synchronize()
        return [loss] + [p.grad for _, p in m.named_parameters()]


def head_lines(B, torch, f64, cases, dump=None):
    H = Head(B, torch, f64)
    tag = 'fp64' if f64 else 'fp32'
    for b, d, k, full, _ in cases:
        name = '%s b%d_d%d_k%d_%s' % (tag, b, d, k, 'full' if full else 'diag')
        o, y, noise = H.data(b, d, k, full)
        cols = []
        for what, eps, nz, seed in (('eps0', 0.0, None, 0), ('noise', 1e-5, noise, 0), ('philox', 1e-5, None, SEED)):
            res = H.nll(H.dims(d, k, full, eps), o, y, nz, seed, STREAM if seed else 0)
            cols.append('%s %s' % (what, sha(*res)))
            if dump is not None and what == 'eps0':
                dump['dout_%d_%d_%d_b%d' % (d, k, int(full), b)] = res[1].cpu().numpy()
                dump['loss_%d_%d_%d_b%d' % (d, k, int(full), b)] = res[0].cpu().numpy()
        if k > 1:
            oc = o.clone()
            oc[:, 0] += 25.0
            cols.append('dominant %s' % sha(*H.nll(H.dims(d, k, full, 1e-5), oc, y, noise)))
            cols.append('clamps %s' % sha(*H.nll(H.dims(d, k, full, 1e-5, 0.05, 5.0), oc, y, noise)))
        print('%-26s %s' % (name, '  '.join(cols)), flush=True)
    for b, d, k, full, per_component in cases:
        if not per_component:
            continue
        o, y, noise = H.data(b, d, k, full, seed=5)
        for what, nz in (('noise', noise), ('philox', None)):
            res = H.outputs_and_tuple(H.dims(d, k, full, 0.25), o, y, nz, d, k, full)
            print('%-26s outputs+tuple %s %s' % ('%s b%d_d%d_k%d_%s' % (tag, b, d, k, 'full' if full else 'diag'), what,
                                                 sha(*res)), flush=True)
    print('%-26s loss_and_grad %s' % (tag + ' mdnn_full', sha(*H.model_grads())), flush=True)


def persist_chunk(B, torch, n_updates=40):
    import bench
    d, k, summarizer, sd, ad, t = PERSIST
    cfg = dict(task='synthetic', model='MDNN', summarizer=summarizer, t=t, sd=sd, ad=ad, d=d, k=k, hidden=[128, 128],
               n_feat=0, pairs=1000, full=True)
    os.environ.pop('BSIG_NO_PERSISTENT', None)
    B.MDNN.EPS_NOISE = 0.0
    theta, states, actions = bench.synth_pairs(cfg, 1000, 3, DEV)
    bs = bench.build_gpu_model(B, cfg, DEV, 77)
    ids = np.random.RandomState(5).randint(0, 800, (n_updates, 100))
    summ = bs._summarize(states, actions)
    run = lambda: bs.model.run_training(summ, theta, n_updates, 100, ids_table=ids)
    logs = run()
    assert B._lib.load().bsig_fit_is_persistent(bs.model._plan) == 2
    return logs, bs.model._flat.clone(), run


def timed(torch, fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    reps = []
    for _ in range(9):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        reps.append(e0.elapsed_time(e1) * 1e3)
    return 'median %.1f us  slowest %.1f  fastest %.1f  all %s' % (sorted(reps)[4], max(reps), min(reps),
                                                                 ' '.join('%.1f' % r for r in reps))


def timing(B, torch):
    import head_cases as HC
    H = Head(B, torch, False)
    for _, d, k, full, path, _, _ in HC.CASES:
        if path not in (HC.PATH_DIAG, HC.PATH_FULL):
            continue
        b = 1025
        o, y, noise = H.data(b, d, k, full)
        hd = H.dims(d, k, full, 1e-5)
        L, lib = H.L, H.lib
        loss, d_o = torch.zeros(1, device=DEV), torch.zeros_like(o)
        flag, ws = torch.zeros(1, dtype=torch.int32, device=DEV), H.ws(hd, b)
        fn = lambda: L.check(lib.bsig_mdn_head_nll(C.byref(hd), L.ptr(o), o.shape[1], L.ptr(y), d, None, b, b,
                                                   L.ptr(noise), 0, 0, L.ptr(loss), L.ptr(d_o), L.ptr(flag), L.ptr(ws),
                                                   ws.numel() * 4, L.stream()))
        print('head_nll b%d d%d k%d %s  %s' % (b, d, k, 'full' if full else 'diag', timed(torch, fn)), flush=True)
    run = persist_chunk(B, torch)[2]
    print('persistent full-covariance chunk (40 updates)  %s' % timed(torch, run), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == 'cmp':
        return cmp(sys.argv[2], sys.argv[3])
    import torch
    import bayes_sim_ig_amd as B
    import head_cases as HC
    B._lib.require_gpu()
    B.MDNN.VERBOSE = False
    if '--time' in sys.argv:
        return timing(B, torch)
    if '--dump' in sys.argv:
        dump = {}
        head_lines(B, torch, True, F64_CASES, dump)
        logs, flat, _ = persist_chunk(B, torch)
        dump['persist_logs'] = np.array(logs['train_loss'] + logs['test_loss'], np.float64)
        dump['persist_weights'] = flat.cpu().numpy()
        np.savez(sys.argv[sys.argv.index('--dump') + 1], **dump)
        return
    head_lines(B, torch, False, [c[:4] + (c[4] in (HC.PATH_DIAG, HC.PATH_FULL),) for c in HC.CASES])
    logs, flat, _ = persist_chunk(B, torch)
    print('persist full d%d_k%d          logs %s  weights %s' % (PERSIST[0], PERSIST[1], hashlib.sha256(
        repr(sorted(logs.items())).encode()).hexdigest()[:16], sha(flat)), flush=True)
    head_lines(B, torch, True, F64_CASES)


if __name__ == '__main__':
    main()
