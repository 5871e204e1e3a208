#!/usr/bin/env python3
"""Update times across a chunk boundary of a block launch (bsig_fit_run_block) from the persistent kernel's
wall-clock stamps: a cfg5-shaped fit of 2000 pairs (two chunks in one launch), updates BSIG_PROF_T0 ..
BSIG_PROF_T0 + 8 of the launch (default 96: the boundary lies between updates 99 and 100)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

os.environ.setdefault('BSIG_PROF_T0', '96')
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                     # noqa: E402
import bayes_sim_ig_amd as B     # noqa: E402

B.MDNN.VERBOSE = False
dev = 'cuda:0'
lib = B._lib.require_gpu()
cfg = dict(bench.CONFIGS[sys.argv[1] if len(sys.argv) > 1 else 'cfg5'])
theta, states, actions = bench.synth_pairs(cfg, 2000, 3, dev)
bs = bench.build_gpu_model(B, cfg, dev, 77)
bs.fit(theta, states, actions)                        # warm-up (plan)
buf = torch.zeros(2 * 256 * 8 * 16, dtype=torch.int64, device=dev)
lib.bsig_debug_persist_profile(buf.data_ptr())
bs.fit(theta, states, actions)
torch.cuda.synchronize()
lib.bsig_debug_persist_profile(None)
st = buf.cpu().numpy().reshape(2, 256, 8, 16)[0].astype(np.float64) / 100.0   # 100 MHz -> us
t0 = int(os.environ['BSIG_PROF_T0'])
tiles = [g for g in range(256) if st[g, 1, 3] > 0]
print('block launches so far: %d; %d tile workgroups; update u of the launch: start of u+1 minus start of u, '
      'first / last tile workgroup to start' % (getattr(bs.model, '_block_launches', 0), len(tiles)))
for u in range(7):
    a = np.array([st[g, u, 0] for g in tiles]); b = np.array([st[g, u + 1, 0] for g in tiles])
    print('    update %3d: %6.2f us (min start), %6.2f us (max start)' % (t0 + u, b.min() - a.min(), b.max() - a.max()))
