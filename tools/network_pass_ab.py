#!/usr/bin/env python3
"""A/B of two builds of the library (BSIG_LIB_PATH) over the estimator's per-phase network pass
(csrc/network_pass.h).  Two builds that print the same hashes lay out parameters and workspaces alike and
compute the same bits.

--host (no GPU, no torch): one sha256 over a grid of cfgs of bsig_mdn_param_count, bsig_mdn_param_offsets,
bsig_mdn_workspace_bytes and bsig_mdn_workspace_bytes_f64 -- and, for the cfgs the layout refuses, of the
return code and the bsig_last_error text.

default (MI355X): per case and precision one line with a sha256 of the _head_forward output, of the loss and
flat gradient buffer of loss_and_grad, and of the trained weights and logs of a 20-update teacher-forced
run_training on the per-phase kernels (BSIG_NO_PERSISTENT=1; fp32: the update graph with fused Adam, then once
more bound with the split-Adam flag: gradient graph + flat Adam).
usage: [BSIG_LIB_PATH=...] python tools/network_pass_ab.py [--host] [--only SUBSTRING]"""
import ctypes as C
import hashlib
import itertools
import os
import struct
import sys

os.environ['BSIG_NO_PERSISTENT'] = '1'      # (read when a fit plan is created)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayes_sim_ig_amd import _lib     # noqa: E402

TRUNKS = ((), (5,), (128, 128), (24, 7, 130), (3, 9, 33, 64), (16, 12, 8, 4, 2), (7,) * 6, (33, 1, 2, 3, 5, 8, 13),
          (12,) * 8)
# (out_dim, n_comp): Nh = 243 / 270 / 297 around the whole-width kernels' 257..272 (gemm_wide_covers), small heads
HEADS = ((13, 9), (13, 10), (13, 11), (2, 10), (5, 3), (1, 1))
BATCHES = (1, 50, 100, 2047, 2048, 8192)


def _cfg(input_dim=10, hidden=(), rff=0, cos_only=0, d=3, k=3, full=0):
    cfg = _lib.MdnCfg()
    cfg.input_dim, cfg.n_hidden = input_dim, len(hidden)
    for i, h in enumerate(hidden[:_lib.MAX_HIDDEN]):
        cfg.hidden[i] = h
    cfg.activation, cfg.rff_feats, cfg.rff_cos_only, cfg.rff_scale = 0, rff, cos_only, 0.125
    cfg.head.out_dim, cfg.head.n_comp, cfg.head.full_cov = d, k, full
    cfg.head.eps_noise, cfg.head.min_weight, cfg.head.ll_limit = 1e-5, 1e-5, 1e5
    cfg.lr, cfg.beta1, cfg.beta2, cfg.adam_eps = 1e-3, 0.9, 0.999, 1e-8
    return cfg


def host():
    lib = _lib.load()
    digest, count = hashlib.sha256(), 0
    offs = (C.c_int64 * (2 * (_lib.MAX_HIDDEN + 4)))()

    def record(cfg, batches):
        nonlocal count
        ref = None if cfg is None else C.byref(cfg)
        rec = [struct.pack('<q', lib.bsig_mdn_param_count(ref)), lib.bsig_last_error()]
        for i in range(len(offs)):
            offs[i] = -7
        rc = lib.bsig_mdn_param_offsets(ref, offs, len(offs))
        rec += [struct.pack('<i%dq' % len(offs), rc, *offs), lib.bsig_last_error() if rc else b'']
        for b in batches:
            rec.append(struct.pack('<2Q', lib.bsig_mdn_workspace_bytes(ref, b), lib.bsig_mdn_workspace_bytes_f64(ref, b)))
        digest.update(b'|'.join(rec))
        count += 1

    for hidden, (d, k), full, input_dim in itertools.product(TRUNKS, HEADS, (0, 1), (1, 10, 302)):
        record(_cfg(input_dim, hidden, d=d, k=k, full=full), BATCHES)
    for rff, cos_only, (d, k), full in itertools.product((2, 64, 500, 63, 1), (0, 1), HEADS, (0, 1)):
        if cos_only or rff % 2 == 0:
            record(_cfg(302, rff=rff, cos_only=cos_only, d=d, k=k, full=full), BATCHES)
    # what make_layout refuses, one cfg per requirement (and too few offset slots)
    record(None, (100,))
    bad_depth = _cfg()
    for n_hidden in (-1, _lib.MAX_HIDDEN + 1):
        bad_depth.n_hidden = n_hidden
        record(bad_depth, (100,))
    for cfg in (_cfg(input_dim=0), _cfg(hidden=(8,), rff=64), _cfg(rff=63), _cfg(rff=-2), _cfg(hidden=(8, 0)),
                _cfg(d=0), _cfg(k=0)):
        record(cfg, (100,))
    rc = lib.bsig_mdn_param_offsets(C.byref(_cfg(hidden=(8, 8))), offs, 11)
    digest.update(struct.pack('<i', rc) + lib.bsig_last_error())
    print('host: %d cfgs  sha256 %s' % (count + 1, digest.hexdigest()))


# name: (class, hidden, activation, full_cov, batch, (out_dim, n_comp), eps_noise, rows)
CASES = {}
for depth, hidden in enumerate(((), (16,), (16, 12), (16, 12, 8))):
    CASES['mdnn_depth%d' % depth] = ('MDNN', hidden, 'Tanh', False, 64, (3, 3), 1e-5, False)
for act in ('ReLU', 'LeakyReLU', 'Sigmoid', 'Identity'):          # (Tanh at depth 2: mdnn_depth2)
    CASES['mdnn_' + act.lower()] = ('MDNN', (16, 12), act, False, 64, (3, 3), 1e-5, False)
CASES['mdnn_full'] = ('MDNN', (16, 12, 8), 'Tanh', True, 64, (3, 3), 1e-5, False)
CASES['mdnn_rows_eps0'] = ('MDNN', (16, 12, 8), 'ReLU', True, 64, (3, 3), 0.0, True)
CASES['mdnn_depth0_rows'] = ('MDNN', (), 'Tanh', False, 64, (3, 3), 0.0, True)
CASES['mdnn_wide_b2048'] = ('MDNN', (24,), 'Tanh', False, 2048, (13, 10), 1e-5, False)
CASES['mdrff'] = ('MDRFF', (), 'Tanh', False, 64, (3, 3), 1e-5, False)
CASES['mdrff_full_rows_eps0'] = ('MDRFF', (), 'Tanh', True, 64, (3, 3), 0.0, True)
CASES['mdrff_wide_b2048'] = ('MDRFF', (), 'Tanh', False, 2048, (13, 10), 1e-5, True)


def _sha(*arrays):
    import numpy as np
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def device(only):
    import numpy as np
    import torch
    import bayes_sim_ig_amd as B
    _lib.require_gpu()
    B.MDNN.VERBOSE = False
    dev, n_updates, input_dim = 'cuda:0', 20, 10
    for name, (cls, hidden, act, full, batch, (d, k), eps, use_rows) in CASES.items():
        if only and only not in name:
            continue
        B.MDNN.EPS_NOISE = eps
        kw = dict(input_dim=input_dim, output_dim=d, output_lows=np.zeros(d), output_highs=np.ones(d), n_gaussians=k,
                  full_covariance=full, activation=getattr(torch.nn, act), lr=1e-3)
        kw.update(dict(hidden_layers=hidden) if cls == 'MDNN' else dict(n_feat=64, sigma=2.0))
        n_tot = batch * 5 // 4
        gen = torch.Generator().manual_seed(21)
        x, y = torch.randn(n_tot, input_dim, generator=gen).to(dev), torch.rand(n_tot, d, generator=gen).to(dev)
        noise = torch.rand(batch, d, k, generator=gen).to(dev)
        rng = np.random.RandomState(22)
        rows = rng.randint(0, n_tot, batch) if use_rows else None
        ids = rng.randint(0, batch, (n_updates, batch))       # (the first `batch` rows are the training split)
        for dtype, splits in (('fp32', (False, True)), ('fp64', (False,))):
            torch.manual_seed(23)
            np.random.seed(24)
            m = getattr(B, cls)(device=dev, **kw)
            if dtype == 'fp64':
                m.double()
            w0 = m._flat.detach().clone()
            fwd = _sha(m._head_forward(x)[1].cpu().numpy())
            loss = m.loss_and_grad(x if use_rows else x[:batch], y, rows=rows, noise=noise)
            grad = _sha(loss.cpu().numpy(), m._flat_grad.cpu().numpy())
            fits = []
            for split in splits:
                with torch.no_grad():
                    m._flat.copy_(w0)
                if split:      # bound as a data-parallel rank binds it: gradients to the flat buffer, then the flat Adam kernel
                    m._drop_plan()
                    m._bind_flags = lambda m=m: B.MDNN._bind_flags(m) | _lib.FIT_SPLIT_ADAM
                torch.manual_seed(25)
                logs = m.run_training(x, y, n_updates, batch, ids_table=ids)
                fits.append(_sha(m._flat.cpu().numpy(), np.asarray(logs['train_loss'] + logs['test_loss'], np.float64)))
            torch.cuda.synchronize()
            print('%-22s %s  forward %s  loss_grad %s  fit %s' % (name, dtype, fwd, grad, '  split-Adam '.join(fits)),
                  flush=True)


if __name__ == '__main__':
    if '--host' in sys.argv:
        host()
    else:
        device(sys.argv[sys.argv.index('--only') + 1] if '--only' in sys.argv else None)
