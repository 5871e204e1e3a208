"""Timing of the general signature kernel (include/bsig_signature.h, csrc/signature_ex.h) for
profiles/signature_ex_NOTES.md: HIP events, a warm-up, median and range of REPS repeats, the kernels of a
comparison alternating in one process.
  (i)  cfg4b's shape, N = 100 000, L = 11, sd = 17, ad = 4 (d = 22), depth 3: the general kernel (reached with
       the identity channel list) next to the tuned signature3_kernel (channels=None);
  (ii) what only the general kernel does: depth 4 at sd = 4, ad = 1 (d = 6, 1554 terms) and depth 5 at sd = 3,
       ad = 1 (d = 5, 3905 terms), L = 21, N = 100 000.
Bytes/s are over the algorithmic 4 (L d + width) bytes per trajectory: the channels read once, the row written once."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import bayes_sim_ig_amd as B
from tools.csrc_hash import csrc_hash

DEV = 'cuda:0'
REPS = 11
N = 100000


def timed(fns, reps=REPS, warm=2):
    """{name: (median, min, max)} in us; the kernels alternate inside every repeat"""
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


def shape(length, sd, ad, depth):
    gen = torch.Generator().manual_seed(0)
    states = torch.randn(N, length, sd, generator=gen).to(DEV)
    actions = torch.rand(N, length, ad, generator=gen).to(DEV)
    d = 1 + sd + ad
    width = B.summarizers.signature_dim(d, depth)
    out = torch.empty(N, B._lib.round_up(width, 4), device=DEV)
    return states, actions, out, 4.0 * (length * d + width) * N


def line(name, res, nbytes):
    med, lo, hi = res
    return '%s: %.0f us (%.0f .. %.0f), %.2f TB/s of algorithmic bytes' % (name, med, lo, hi, nbytes / med / 1e6)


def main():
    print('# csrc: %s' % csrc_hash())
    print('# %s, N = %d, %d repeats' % (torch.cuda.get_device_name(0), N, REPS))
    states, actions, out, nbytes = shape(11, 17, 4, 3)
    ident = list(range(21))
    res = timed({'tuned': lambda: B.summary_signatory(states, actions, depth=3, out=out),
                 'general': lambda: B.summary_signatory(states, actions, depth=3, channels=ident, out=out)})
    print('(i) depth 3, L = 11, d = 22 (cfg4b), %.1f KB per trajectory' % (nbytes / N / 1e3))
    print('  ' + line('signature3_kernel (channels=None)', res['tuned'], nbytes))
    print('  ' + line('signature_ex_kernel (identity list)', res['general'], nbytes))
    print('  general / tuned = %.2f' % (res['general'][0] / res['tuned'][0]))
    del states, actions, out
    print('(ii) the general kernel beyond depth 3, L = 21')
    for sd, ad, depth in ((4, 1, 4), (3, 1, 5)):
        states, actions, out, nbytes = shape(21, sd, ad, depth)
        res = timed({'general': lambda: B.summary_signatory(states, actions, depth=depth, out=out)})
        print('  ' + line('depth %d, d = %d, %.1f KB per trajectory' % (depth, 1 + sd + ad, nbytes / N / 1e3),
                          res['general'], nbytes))
        del states, actions, out


if __name__ == '__main__':
    main()
