#!/usr/bin/env python3
"""What bsig_debug_gemm_path and bsig_gemm_workspace_bytes answer over a fixed grid of shapes, layouts,
epilogues, workspaces, matmul precisions and environment switches: one sha256 of the whole dump and the
point count.  Host arithmetic only (no GPU, no torch).  Two builds of the library that print the same
hash route every point of the grid alike.
usage: [BSIG_LIB_PATH=...] python tools/gemm_route_dump.py [--out FILE] [--skip-k0]
--skip-k0 leaves k = 0 out: a build from before the fp32 kernels refused an empty contraction divides by zero
on the host there, and can only be compared on the rest of the grid."""
import ctypes
import hashlib
import itertools
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayes_sim_ig_amd import _lib     # noqa: E402

M = (1, 33, 100, 128, 129, 300, 512, 2048, 2090, 4096, 8192)
N = (1, 32, 64, 65, 96, 97, 128, 192, 257, 260, 272, 288, 510, 512, 1024, 4096)
K = (0, 1, 31, 32, 64, 130, 302, 500, 530, 859, 1024, 1056, 2048, 2080, 4096)
LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))
EPILOGUES = (0, 1, 2, 3, 5, 100)      # NONE, BIAS, BIAS_ACT, COS_SIN, MUL_DACT, the fused Adam step
SWITCHES = ('BSIG_GEMM_LEAN', 'BSIG_GEMM_WIDE', 'BSIG_GEMM_NO_LARGE_PLAN', 'BSIG_GEMM_NO_UNALIGNED',
            'BSIG_DEBUG_F64_ACC_MIN_K', 'BSIG_SPLIT_BF16_EVERYWHERE', 'BSIG_GEMM_TILE', 'BSIG_GEMM_SPLITS',
            'BSIG_GEMM_WIDE_TILE', 'BSIG_GEMM_WIDE_WGS', 'BSIG_GEMM_NO_COMBINE')
ENVS = [{}, {'BSIG_GEMM_LEAN': '0'}, {'BSIG_GEMM_WIDE': '0'}, {'BSIG_GEMM_NO_LARGE_PLAN': '1'},
        {'BSIG_GEMM_NO_UNALIGNED': '1'}, {'BSIG_DEBUG_F64_ACC_MIN_K': '1'}, {'BSIG_SPLIT_BF16_EVERYWHERE': '1'}]
ENVS += [{'BSIG_GEMM_TILE': str(t), 'BSIG_GEMM_SPLITS': str(s)} for t in range(6) for s in (1, 3)]
# every point without switches; under a switch every STRIDE-th point of the cross product (5 is coprime to the
# lengths of the inner axes: every value of every axis still appears)
STRIDE = 5


def main():
    args = sys.argv[1:]
    lib = _lib.load()
    out_file = open(args[args.index('--out') + 1], 'wb') if '--out' in args else None
    ks = K[1:] if '--skip-k0' in args else K
    digest, count, out = hashlib.sha256(), 0, (ctypes.c_int32 * 8)()
    inner = list(itertools.product(LAYOUTS, (0, 1), EPILOGUES, range(3), (0, 1)))
    for env in ENVS:
        for key in SWITCHES:
            os.environ.pop(key, None)
        os.environ.update(env)
        stride, i = (STRIDE if env else 1), 0
        for (m, n, k) in itertools.product(M, N, ks):
            need = int(lib.bsig_gemm_workspace_bytes(m, n, k))
            rec = [struct.pack('<q', need)]
            for ((akm, bkm), gathered, epi, ws_kind, matmul) in inner:
                i += 1
                if i % stride:
                    continue
                rc = lib.bsig_debug_gemm_path(m, n, k, akm, bkm, gathered, epi, (0, 4 * m * n, need)[ws_kind], matmul, out)
                rec.append(struct.pack('<9i', rc, *out))
                count += 1
            rec = b''.join(rec)
            digest.update(rec)
            if out_file:
                out_file.write(rec)
    print('%d points  sha256 %s' % (count, digest.hexdigest()))


if __name__ == '__main__':
    main()
