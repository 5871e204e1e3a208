"""Shared pieces of the summarizer path tests (tests/test_host_logic.py,
tests/test_gpu_summary_paths.py): the path ids bsig_debug_summary_path reports,
the output layout of a case (pitch, base offset) and the table of shapes with
the device path each must take."""
from collections import namedtuple

# kinds (bsig_summary_dim)
START, CORR, CORRDIFF, SIG = 0, 1, 2, 3

# out[0]: kernel
K_START = 0         # summary_start_kernel<10>
K_WAVE = 1          # crosscorr_wave_kernel: one wavefront per trajectory (S A <= 2048)
K_QUADS = 2         # crosscorr_quads_kernel: line-aligned quad stores, rstep rows per sweep
K_CC = 3            # crosscorr_kernel: one workgroup per trajectory
K_SIG3 = 4          # signature3_kernel<DMAX>
K_SIG12 = 5         # signature12_kernel (depth 1 or 2)
KERNEL_NAMES = {K_START: 'start', K_WAVE: 'wave', K_QUADS: 'quads', K_CC: 'cc', K_SIG3: 'sig3',
                K_SIG12: 'sig12'}

# out[1]: store loop
ST_ELEM = 0         # one float per lane / thread
ST_QUAD = 1         # a quad of action features per thread, walking down the state features
ST_VEC4 = 2         # generic float4 loop
ST_VEC4_TAIL = 3    # generic float4 loop + scalar tail (S A % 4 != 0)
ST_LINE = 4         # signature: head, line-aligned quads, tail
ST_FACTORS = 5      # factor rows only
STORE_NAMES = {ST_ELEM: 'elem', ST_QUAD: 'quad', ST_VEC4: 'vec4', ST_VEC4_TAIL: 'vec4tail',
               ST_LINE: 'line', ST_FACTORS: 'fac'}

PATH_FIELDS = ['kernel', 'store', 'prefetch', 'threads', 'lds', 'grid', 'rstep', 'dmax', 'steps',
               'depth', 'ex_x', 'ex_y']

GRID_CAP = 256 * 64           # grid_for: workgroups of the grid-striding kernels
N_PF = GRID_CAP + 37          # every workgroup of a grid_for launch handles a second trajectory
N_WAVE = 4 * 65536 + 5        # ... and of the wave kernel (4 trajectories per workgroup, 65536 cap)

Case = namedtuple('Case', 'name kind n t ta sd ad kernel store prefetch want depth max_t pad off '
                          'factors')


def C(name, kind, n, t, ta, sd, ad, kernel, store, prefetch, want=None, depth=0, max_t=10,
      pad=None, off=0, factors=False):
    """pad: output pitch = width + pad (None: the 16-byte aligned pitch + 4 floats); off: floats
    between the buffer's (aligned) base and row 0; want: other out[] fields to pin."""
    return Case(name, kind, n, t, ta, sd, ad, kernel, store, prefetch, want or {}, depth, max_t,
                pad, off, factors)


def window(t, sd):
    """crosscorr_window: summarizers.py:96-99"""
    w = 5 if sd > 50 else 10
    return t if t <= w else w


def sig_depth(c):
    d = 1 + c.sd + c.ad
    if c.depth:
        return c.depth
    return next(k for k in (3, 2, 1, 0) if d ** k <= 110 ** 2)


def dims(c):
    """(S, A) of a cross-correlation case"""
    w = window(c.t, c.sd)
    return w * (c.sd - 1), w * c.ad


def width(c):
    """floats per row the call writes: the summary, or the factor row's S + A + 3"""
    if c.kind == START:
        return c.max_t * (c.sd + c.ad)
    if c.kind == SIG:
        d = 1 + c.sd + c.ad
        return sum(d ** k for k in range(1, sig_depth(c) + 1))
    s, a = dims(c)
    return s + a + 3 if c.factors else s * a + 2


def pitch(c):
    w = width(c)
    return w + c.pad if c.pad is not None else -(-w // 4) * 4 + 4


def query_args(c, n=None):
    """bsig_debug_summary_path's arguments for the case's launch"""
    return (c.kind, c.n if n is None else n, c.t, c.ta, c.sd, c.ad, c.depth, c.max_t, pitch(c),
            1 if c.off % 4 == 0 else 0, 1 if c.factors else 0)


CASES = [
    # --- summary_start: 64 / 128 / 256 threads at per-step widths 95 / 96, 191 / 192
    C('start_w95', START, 9, 12, 12, 90, 5, K_START, ST_ELEM, 0, {'threads': 64}),
    C('start_w96', START, 9, 4, 15, 90, 6, K_START, ST_ELEM, 0, {'threads': 128}, max_t=13),
    C('start_w191', START, 5, 30, 7, 180, 11, K_START, ST_ELEM, 0, {'threads': 128}, max_t=7),
    C('start_w192', START, 5, 3, 25, 180, 12, K_START, ST_ELEM, 0, {'threads': 256}, max_t=25),
    C('start_cfg5', START, 3, 11, 11, 211, 20, K_START, ST_ELEM, 0, {'threads': 256}),
    C('start_pendulum', START, 7, 21, 20, 3, 1, K_START, ST_ELEM, 0, {'threads': 64}, max_t=1, pad=3),
    C('start_big', START, N_PF, 12, 9, 3, 1, K_START, ST_ELEM, 0, {'grid': GRID_CAP, 'threads': 64}),
    # --- one wavefront per trajectory (S A <= 2048)
    C('wave_cartpole', CORRDIFF, 7, 21, 21, 4, 1, K_WAVE, ST_ELEM, 0, {'grid': 2, 'lds': 40 * 16}),
    C('wave_cartpole_corr', CORR, 6, 21, 19, 4, 1, K_WAVE, ST_ELEM, 0, pad=1),
    C('wave_2048_t4', CORRDIFF, 5, 4, 4, 129, 1, K_WAVE, ST_ELEM, 0),        # S A = 512 x 4
    C('wave_2048_t8', CORR, 5, 8, 8, 33, 1, K_WAVE, ST_ELEM, 0, off=1),      # S A = 256 x 8
    C('wave_short', CORRDIFF, 9, 6, 6, 5, 2, K_WAVE, ST_ELEM, 0),            # T < W
    C('wave_big', CORRDIFF, N_WAVE, 21, 21, 4, 1, K_WAVE, ST_ELEM, 0, {'grid': 65536}),
    C('wave_fac', CORRDIFF, 7, 21, 21, 4, 1, K_WAVE, ST_FACTORS, 0, factors=True),
    C('wave_fac_big', CORR, N_WAVE, 21, 21, 4, 1, K_WAVE, ST_FACTORS, 0, factors=True),
    # --- crosscorr_quads_kernel: rstep 256, 128, 24, 8, 1
    C('quads_r256', CORRDIFF, 5, 4, 4, 130, 1, K_QUADS, ST_QUAD, 1, {'rstep': 256}),   # S A = 2064
    C('quads_r128', CORR, 5, 8, 8, 34, 1, K_QUADS, ST_QUAD, 1, {'rstep': 128}),        # S A = 2112
    C('quads_ant', CORRDIFF, 5, 51, 51, 60, 8, K_QUADS, ST_QUAD, 1, {'rstep': 24}),
    C('quads_anymal', CORRDIFF, 5, 21, 21, 48, 12, K_QUADS, ST_QUAD, 1, {'rstep': 8}),
    C('quads_shadow_more', CORRDIFF, 3, 51, 51, 211, 20, K_QUADS, ST_QUAD, 1, {'rstep': 8}),
    C('quads_r1', CORR, 5, 8, 8, 3, 68, K_QUADS, ST_QUAD, 1, {'rstep': 1}),
    C('quads_sd257', CORRDIFF, 4, 6, 6, 257, 4, K_QUADS, ST_QUAD, 1, {'rstep': 48}),   # sd - 1 = 256
    C('quads_ad256', CORRDIFF, 4, 3, 3, 3, 256, K_QUADS, ST_QUAD, 1, {'rstep': 1}),
    C('quads_big', CORRDIFF, N_PF, 4, 4, 130, 1, K_QUADS, ST_QUAD, 1, {'rstep': 256, 'grid': GRID_CAP}),
    # --- crosscorr_kernel, quad per thread (A % 4 == 0, the quads kernel's rstep is 0)
    C('cc_quad_a140', CORRDIFF, 5, 21, 21, 8, 14, K_CC, ST_QUAD, 1, {'rstep': 7}),
    C('cc_quad_a140_w5', CORRDIFF, 3, 51, 51, 60, 28, K_CC, ST_QUAD, 1, {'rstep': 7}),
    C('cc_quad_a600', CORR, 5, 21, 21, 3, 60, K_CC, ST_QUAD, 1, {'rstep': 1}),
    C('cc_quad_big', CORRDIFF, N_PF, 6, 6, 4, 22, K_CC, ST_QUAD, 1, {'rstep': 7}),
    # --- crosscorr_kernel, generic float4 loop, with and without the scalar tail
    C('cc_vec4', CORRDIFF, 5, 21, 21, 25, 1, K_CC, ST_VEC4, 1),
    C('cc_vec4_tail', CORRDIFF, 5, 5, 5, 52, 3, K_CC, ST_VEC4_TAIL, 1),
    C('cc_vec4_a1100', CORRDIFF, 3, 21, 21, 20, 110, K_CC, ST_VEC4, 1),      # A % 4 == 0, A > 1024
    C('cc_vec4_big', CORR, N_PF, 21, 21, 25, 1, K_CC, ST_VEC4, 1),
    C('cc_vec4_tail_big', CORRDIFF, N_PF, 5, 5, 52, 3, K_CC, ST_VEC4_TAIL, 1),
    # --- crosscorr_kernel, scalar store (pitch not a multiple of 4, or a misaligned base)
    C('cc_scalar_pitch', CORRDIFF, 5, 21, 21, 25, 1, K_CC, ST_ELEM, 1, pad=1),
    C('cc_scalar_ant_pitch', CORR, 3, 51, 51, 60, 8, K_CC, ST_ELEM, 1, pad=1),
    C('cc_scalar_ant_offset', CORRDIFF, 4, 51, 51, 60, 8, K_CC, ST_ELEM, 1, off=1),
    C('cc_scalar_big', CORRDIFF, N_PF, 21, 21, 25, 1, K_CC, ST_ELEM, 1, pad=3),
    # --- crosscorr_kernel, features fetched in place (sd - 1 > 256 or ad > 256)
    C('cc_inplace_sd300', CORRDIFF, 3, 11, 11, 300, 2, K_CC, ST_VEC4_TAIL, 0),
    C('cc_inplace_sd258', CORRDIFF, 4, 6, 6, 258, 4, K_CC, ST_QUAD, 0, {'rstep': 51}),
    C('cc_inplace_ad300', CORR, 4, 3, 3, 3, 300, K_CC, ST_QUAD, 0, {'rstep': 1}),
    C('cc_inplace_ad257', CORRDIFF, 4, 3, 3, 3, 257, K_CC, ST_VEC4_TAIL, 0),
    C('cc_inplace_big', CORRDIFF, N_PF, 3, 3, 3, 257, K_CC, ST_VEC4_TAIL, 0),
    C('cc_inplace_quad_big', CORR, N_PF, 2, 2, 3, 260, K_CC, ST_QUAD, 0, {'rstep': 1}),
    C('cc_lds_edge', CORRDIFF, 2, 4, 4, 9598, 1, K_CC, ST_QUAD, 0, {'lds': 150 * 1024, 'rstep': 256}),
    # --- crosscorr_kernel, factor rows
    C('cc_fac_ant', CORRDIFF, 5, 51, 51, 60, 8, K_CC, ST_FACTORS, 1, factors=True),
    C('cc_fac_shadow_more', CORRDIFF, 3, 51, 51, 211, 20, K_CC, ST_FACTORS, 1, {'ex_x': 64},
      factors=True),
    C('cc_fac_a1100', CORRDIFF, 3, 21, 21, 20, 110, K_CC, ST_FACTORS, 1, {'ex_x': 64}, factors=True),
    C('cc_fac_inplace', CORRDIFF, 3, 11, 11, 300, 2, K_CC, ST_FACTORS, 0, factors=True, pad=1),
    C('cc_fac_big', CORRDIFF, N_PF, 21, 21, 25, 1, K_CC, ST_FACTORS, 1,
      {'ex_y': GRID_CAP, 'ex_x': 10}, factors=True),
    C('cc_fac_inplace_big', CORR, N_PF, 3, 3, 3, 257, K_CC, ST_FACTORS, 0, factors=True),
    # --- signature3_kernel<DMAX> at d = 8/9, 16/17, 24/25, 32
    C('sig_d8', SIG, 5, 11, 11, 5, 2, K_SIG3, ST_LINE, 1, {'dmax': 8, 'threads': 64}),
    C('sig_d9', SIG, 5, 11, 11, 6, 2, K_SIG3, ST_LINE, 1, {'dmax': 16, 'threads': 128}),
    C('sig_d16', SIG, 5, 11, 11, 12, 3, K_SIG3, ST_LINE, 1, {'dmax': 16, 'threads': 256}),
    C('sig_d17', SIG, 5, 11, 11, 13, 3, K_SIG3, ST_LINE, 1, {'dmax': 24, 'threads': 320}),
    C('sig_d24', SIG, 4, 11, 11, 20, 3, K_SIG3, ST_LINE, 1, {'dmax': 24, 'threads': 576}, depth=3),
    C('sig_d25', SIG, 4, 11, 11, 20, 4, K_SIG3, ST_LINE, 1, {'dmax': 32, 'threads': 640}, depth=3),
    C('sig_d32', SIG, 3, 11, 11, 27, 4, K_SIG3, ST_LINE, 1, {'dmax': 32, 'threads': 1024}, depth=3),
    # L sd at the thread count (prefetch) and one above (fetched in place)
    C('sig_d8_lsd64', SIG, 5, 16, 16, 4, 3, K_SIG3, ST_LINE, 1, {'dmax': 8}),
    C('sig_d8_lsd65', SIG, 5, 13, 13, 5, 2, K_SIG3, ST_LINE, 0, {'dmax': 8}),
    C('sig_d16_lsd264', SIG, 5, 22, 22, 12, 3, K_SIG3, ST_LINE, 0, {'dmax': 16}),
    C('sig_d32_lsd1024', SIG, 2, 64, 64, 16, 15, K_SIG3, ST_LINE, 1, {'dmax': 32}, depth=3),
    C('sig_d32_lsd1025', SIG, 2, 41, 41, 25, 6, K_SIG3, ST_LINE, 0, {'dmax': 32}, depth=3),
    C('sig_d32_lds_edge', SIG, 2, 88, 88, 27, 4, K_SIG3, ST_LINE, 0, {'dmax': 32, 'lds': 153488},
      depth=3),
    # plain store: pitch not a multiple of 4, misaligned base
    C('sig_d9_pitch', SIG, 5, 11, 11, 6, 2, K_SIG3, ST_ELEM, 1, {'dmax': 16}, pad=2),
    C('sig_d17_offset', SIG, 4, 11, 11, 13, 3, K_SIG3, ST_ELEM, 1, {'dmax': 24}, off=1),
    C('sig_d24_offset', SIG, 3, 9, 9, 16, 7, K_SIG3, ST_ELEM, 1, {'dmax': 24}, depth=3, off=2),
    C('sig_d8_big', SIG, N_PF, 11, 11, 5, 2, K_SIG3, ST_LINE, 1, {'dmax': 8, 'grid': GRID_CAP}),
    C('sig_d9_pitch_big', SIG, N_PF, 11, 11, 6, 2, K_SIG3, ST_ELEM, 1, {'dmax': 16}, pad=2),
    C('sig_d8_inplace_big', SIG, N_PF, 13, 13, 5, 2, K_SIG3, ST_LINE, 0, {'dmax': 8}),
    # --- signature12_kernel
    C('sig12_cfg4', SIG, 2, 11, 11, 211, 20, K_SIG12, ST_ELEM, 0, {'depth': 1, 'lds': 0}),
    C('sig12_d2', SIG, 4, 9, 9, 30, 2, K_SIG12, ST_ELEM, 0, {'depth': 2}),
    C('sig12_d2_d23', SIG, 3, 7, 7, 18, 4, K_SIG12, ST_ELEM, 0, {'depth': 2}),  # 23^3 > 110^2
    C('sig12_d2_explicit', SIG, 3, 21, 21, 60, 8, K_SIG12, ST_ELEM, 0, {'depth': 2}, depth=2, pad=1),
    C('sig12_d1_big', SIG, N_PF, 5, 5, 60, 60, K_SIG12, ST_ELEM, 0, {'depth': 1}),
]

# shapes every launch refuses with BSIG_EUNSUPPORTED: (name, kind, t, sd, ad, depth, factors)
REFUSED = [
    ('cc_lds', CORRDIFF, 4, 9599, 1, 0, False),         # (S + A + 8) 4 B = 150 KB + 16 B
    ('cc_lds_fac', CORR, 4, 9599, 1, 0, True),
    ('cc_lds_w3', CORRDIFF, 3, 12798, 1, 0, False),
    ('sig3_d33', SIG, 11, 28, 4, 3, False),              # depth 3 needs d <= 32
    ('sig3_lds', SIG, 89, 27, 4, 3, False),             # d = 32: 150 KB + 144 B at L = 89
    ('sig2_lds', SIG, 193, 150, 49, 2, False),          # L d 4 B > 150 KB
]


def case_id(c):
    return c.name
