"""The shared cases of the least-squares dynamics summary (include/bsig_sysid.h), its definition restated in
numpy in double, the kernel's own form restated in numpy in fp32, and the error bound: what
tests/test_sysid_host.py and tests/test_gpu_sysid.py compare with.  Nothing here touches the library or the GPU.

The definition.  states [N, Ts, sd], actions [N, Ta, ad]; M = Ts - 1, p = 1 + sd + ad.
  a_t = actions[min(t, Ta - 1)];  phi_t = [1 | s_t | a_t],  y_t = s_(t+1) - s_t,  t = 0..M-1;
  G = Phi^T Phi / M,  B = Phi^T Y / M,  rho = ridge trace(G) / p,  W = (G + rho I)^-1 B  (``numpy.linalg.solve``
  on the primal system, then two steps of refinement with the residual B - (G + rho I) W in long double, so that
  the reference's own error is a few u64 ||W_:j|| whatever the condition number: the ``4 U64 ||.||`` below);
  r_j = sqrt(1/M sum_t (y_tj - phi_t . W_:j)^2);  row = [W row-major | r].

The bound of ``bounds``: per output column j, on the 2-norm of the error of W_:j and on |r_j - r^_j|, for the form
the kernel solves (csrc/sysid.h): the primal p x p system for p <= M, else the dual M x M system
alpha = (K + rho I)^-1 Y, K = Phi Phi^T / M, W = Phi^T alpha / M, e_t = rho alpha_t.  u is the unit roundoff of the
output precision, gamma(n) = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.,
Lemma 3.1); an fma is one rounding, so every count below that takes it for two holds as well.  The inputs are
exactly representable in the precision the kernel computes in.  A is the k x k matrix it factorises, x_j the
solution column (W_:j or alpha_:j), b_j its right-hand side, L the length of a Gram chain (M primal, p dual).
  1. The products (ch. 3, (3.5): an inner product of n terms, then the reciprocal's rounding and its multiply):
       |K^ - K| <= gamma(L + 2) |Phi|^T |Phi| / M   (dual: |Phi| |Phi|^T / M)  =: gamma(L + 2) Kabs;
       primal b^_j: y^_t is one more rounding:   ||b^_j - b_j||_2 <= gamma(M + 3) || |Phi|^T |y_j| / M ||_2;
       dual   b^_j = y^_j:                       ||b^_j - b_j||_2 <= u ||y_j||_2.
  2. rho^ = fl(fl(ridge^ trace^) / p): the diagonal's chains, k - 1 adds, the rounding of ridge to the precision,
     a multiply, a divide:  |rho^ - rho| <= gamma(L + k + 4) rho.
  3. The Cholesky solve (Theorem 10.4): (A^ + dA) x^_j = b^_j with |dA| <= gamma(3 k + 1) |R^|^T |R^|.  Normwise,
     || |R^|^T |R^| ||_2 <= ||R^||_F^2 = trace(R^^T R^), and by Theorem 10.3 each diagonal entry of R^^T R^ is at
     most A^_ii / (1 - gamma(k + 1)), so with 1. and 2. on the trace
       ||dA||_2 <= gamma(3 k + 1) trace(A) (1 + gamma(L + k + 4)) / (1 - gamma(k + 1)).
  4. Together  E = (K^ - K) + (rho^ - rho) I + dA,
       ||E||_2 <= gamma(L + 2) ||Kabs||_2 + gamma(L + k + 4) rho + 3.,
     and from (A + E) x^_j = b_j + db_j, with ainv = ||A^-1||_2 and ainv ||E||_2 < 1 (asserted):
       ||x^_j - x_j||_2 <= ainv (||db_j||_2 + ||E||_2 ||x_j||_2) / (1 - ainv ||E||_2)  =: dx_j.
     Primal: that is the bound on W_:j.  Dual: W^_cj is one more chain of M terms over alpha^, a reciprocal and
     its multiply:
       ||W^_:j - W_:j||_2 <= ||Phi||_2 dx_j / M + gamma(M + 2) ||Phi||_F (||alpha_j||_2 + dx_j) / M.
  5. r.  Primal: e^_t = fl(y^_t - fl(phi_t . W^_:j)), a chain of p terms:
       ||e^ - e||_2 <= De = (1 + u) (u ||y_j||_2 + ||Phi||_2 dW_j + gamma(p) ||Phi||_F (||W_:j||_2 + dW_j)) + u ||e||_2.
     Dual: e^_t = fl(rho^ alpha^_t):
       De = (1 + u) (rho (1 + g) dx_j + g rho ||alpha_j||_2) + u rho ||alpha_j||_2,  g = gamma(L + k + 4).
     The sum of squares is at most 2 M + 2 roundings of partial sums (runs of steps, the runs added up, the
     reciprocal and its multiply), the root halves that and adds one:
       |r^_j - r_j| <= (1 + gamma(2 M + 3)) De / sqrt(M) + gamma(2 M + 3) r_j.
Every norm is evaluated from the fp64 reference; no constant was fitted to what a kernel gave.  The comparisons add
4 U64 ||W_:j||_2 (and 4 U64 (r_j + |y| terms) for r) for the reference's own rounding.
"""
import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53
DEFAULT_RIDGE = 1e-3
WIDE_RIDGE = 1e-1

# name -> (n, Ts, Ta, sd, ad, ridge, in double too).  n = None: the row counts around the trajectories per
# workgroup, G, that the library answers for the shape (test_gpu_sysid.py asks bsig_sysid_group).
CASES = {
    'pendulum': (None, 21, 21, 3, 1, DEFAULT_RIDGE, True),
    'm1': (19, 2, 2, 3, 1, DEFAULT_RIDGE, True),                      # M = 1: a 1 x 1 dual system
    'boundary_m4': (13, 5, 5, 3, 1, DEFAULT_RIDGE, True),             # M = p - 1: dual
    'boundary_m5': (13, 6, 6, 3, 1, DEFAULT_RIDGE, True),             # M = p: primal
    'boundary_m6': (13, 7, 7, 3, 1, DEFAULT_RIDGE, True),
    'tile_16': (5, 17, 17, 12, 3, WIDE_RIDGE, True),                  # k = 16: the 16-wide tile of threads, full
    'tile_17': (5, 18, 18, 13, 3, WIDE_RIDGE, True),                  # one beyond it
    'tile_32': (5, 33, 33, 27, 4, WIDE_RIDGE, True),
    'odd': (7, 12, 12, 7, 3, WIDE_RIDGE, True),                       # p = M = 11, 84 outputs
    'ant_t50': (5, 50, 50, 60, 8, WIDE_RIDGE, True),                  # dual, k = 49
    'ant_t100': (3, 100, 100, 60, 8, WIDE_RIDGE, True),               # primal, k = 69
    'shadowhand': (3, 50, 50, 211, 20, WIDE_RIDGE, False),            # dual, k = 49; fp32 only (LDS)
    'ta_t_minus_1': (21, 21, 20, 3, 1, DEFAULT_RIDGE, True),
    # a constant action is collinear with the intercept: G is singular, the condition number IS 1 + p / ridge, and
    # at the default ridge the fp32 bound is 1.5e-2 of ||W_:j||: above the 1e-2 a case must stay under, so 1e-2
    'ta_1': (21, 21, 1, 3, 1, 1e-2, True),
    'ta_above_t': (21, 21, 24, 3, 1, DEFAULT_RIDGE, True),
}
# ill-conditioned, double only: kappa up to 1 + 69 / 1e-6
ILL = {'ant_t50_ridge_1e-6': (5, 50, 50, 60, 8, 1e-6), 'ant_t100_ridge_1e-6': (3, 100, 100, 60, 8, 1e-6)}


def group_counts(g):
    """Row counts around G trajectories a workgroup: 1, G - 1, G, G + 1, 3 G + 2."""
    return sorted({1, max(g - 1, 1), g, g + 1, 3 * g + 2})


def width(sd, ad):
    return (1 + sd + ad) * sd + sd


def trajectories(n, ts, ta, sd, ad, seed=0):
    """Seeded fp32-representable trajectories as float32 numpy arrays.  The regressors of a trajectory are 0.8
    of a design whose Gram matrix is a multiple of the identity (orthogonal columns, all orthogonal to the
    intercept, where M > sd + ad; orthogonal rows otherwise) plus 0.2 of white noise, shifted by 0.25: a system
    whose conditioning is set by the shape and the ridge, not by the draw.  Actions the kernel pads (Ta < M) or
    ignores (Ta > M) are what they are."""
    rng = np.random.RandomState(1000003 * seed + 7919 * n + 101 * ts + 13 * sd + ad)
    m, d = ts - 1, sd + ad
    states = np.empty((n, ts, sd))
    actions = np.empty((n, ta, ad))
    for i in range(n):
        z = rng.standard_normal((m, d))
        if m > d:
            q, _ = np.linalg.qr(np.concatenate([np.ones((m, 1)), z], axis=1))
            design = q[:, 1:] * np.sqrt(m)
        else:
            q, _ = np.linalg.qr(z.T)
            design = q.T * np.sqrt(d)
        mix = 0.8 * design + 0.2 * rng.standard_normal((m, d)) + 0.25
        states[i, :m] = mix[:, :sd]
        states[i, m] = mix[m - 1, :sd] + 0.5 * rng.standard_normal(sd)
        own = min(ta, m)
        actions[i, :own] = mix[:own, sd:]
        actions[i, own:] = rng.standard_normal((ta - own, ad))
    return states.astype(np.float32), actions.astype(np.float32)


def regressors(states, actions, dtype=np.float64):
    """(Phi [N, M, p], Y [N, M, sd]) in ``dtype``; Y by the one subtraction the kernel does."""
    s, a = np.asarray(states, dtype=dtype), np.asarray(actions, dtype=dtype)
    n, ts, sd = s.shape
    m, ta = ts - 1, a.shape[1]
    assert m >= 1
    phi = np.concatenate([np.ones((n, m, 1), dtype=dtype), s[:, :m], a[:, np.minimum(np.arange(m), ta - 1)]],
                         axis=2)
    return phi, s[:, 1:] - s[:, :-1]


def reference(states, actions, ridge=DEFAULT_RIDGE):
    """The rows of the definition, [N, width] in double."""
    phi, y = regressors(states, actions)
    n, m, p = phi.shape
    ext = np.longdouble
    rows = []
    for i in range(n):
        f, fe, ye = phi[i], phi[i].astype(ext), y[i].astype(ext)
        gram, cross = np.dot(fe.T, fe) / m, np.dot(fe.T, ye) / m
        a_ext = gram + (ext(ridge) * np.trace(gram) / p) * np.eye(p, dtype=ext)
        a = a_ext.astype(np.float64)
        w = np.linalg.solve(a, cross.astype(np.float64))
        for _ in range(2):
            w = w + np.linalg.solve(a, (cross - np.dot(a_ext, w.astype(ext))).astype(np.float64))
        e = (ye - np.dot(fe, w.astype(ext))).astype(np.float64)
        rows.append(np.concatenate([w.reshape(-1), np.sqrt((e * e).sum(axis=0) / m)]))
    return np.stack(rows)


def _gamma(k, u):
    assert k * u < 0.01
    return k * u / (1.0 - k * u)


def bounds(states, actions, ridge, u):
    """(dW [N, sd], dr [N, sd]): the module docstring's bounds on ||W^_:j - W_:j||_2 and |r^_j - r_j| for the
    form the kernel solves, plus the reference's own 4 U64 terms."""
    phi, y = regressors(states, actions)
    n, m, p = phi.shape
    sd = y.shape[2]
    dual = m < p
    k, chain = (m, p) if dual else (p, m)
    g_rho = _gamma(chain + k + 4, u)
    d_w, d_r = np.empty((n, sd)), np.empty((n, sd))
    for i in range(n):
        f, yy = phi[i], y[i]
        fa = np.abs(f)
        gram = f.T @ f / m
        rho = ridge * np.trace(gram) / p
        if dual:
            a = f @ f.T / m + rho * np.eye(m)
            k_abs = fa @ fa.T / m
            x = np.linalg.solve(a, yy)                                        # alpha
            db = u * np.linalg.norm(yy, axis=0)
        else:
            a = gram + rho * np.eye(p)
            k_abs = fa.T @ fa / m
            x = np.linalg.solve(a, f.T @ yy / m)                              # W
            db = _gamma(m + 3, u) * np.linalg.norm(fa.T @ np.abs(yy) / m, axis=0)
        ainv = np.linalg.norm(np.linalg.inv(a), 2)
        err = (_gamma(chain + 2, u) * np.linalg.norm(k_abs, 2) + g_rho * rho
               + _gamma(3 * k + 1, u) * np.trace(a) * (1.0 + g_rho) / (1.0 - _gamma(k + 1, u)))
        assert ainv * err < 0.5, (ainv, err)
        xn = np.linalg.norm(x, axis=0)
        dx = ainv * (db + err * xn) / (1.0 - ainv * err)
        f2, ff = np.linalg.norm(f, 2), np.linalg.norm(f, 'fro')
        yn = np.linalg.norm(yy, axis=0)
        if dual:
            w = f.T @ x / m
            dw = f2 * dx / m + _gamma(m + 2, u) * ff * (xn + dx) / m
            de = (1.0 + u) * (rho * (1.0 + g_rho) * dx + g_rho * rho * xn) + u * rho * xn
        else:
            w, dw = x, dx
            e_norm = np.linalg.norm(yy - f @ w, axis=0)
            de = (1.0 + u) * (u * yn + f2 * dw + _gamma(p, u) * ff * (np.linalg.norm(w, axis=0) + dw)) + u * e_norm
        r = np.linalg.norm(yy - f @ w, axis=0) / np.sqrt(m)
        g_sum = _gamma(2 * m + 3, u)
        wn = np.linalg.norm(w, axis=0)
        d_w[i] = dw + 4.0 * U64 * wn
        d_r[i] = (1.0 + g_sum) * de / np.sqrt(m) + g_sum * r + 4.0 * U64 * (r + (yn + ff * wn) / np.sqrt(m))
    return d_w, d_r


def split(rows, sd, ad):
    """(W [N, p, sd], r [N, sd]) of rows [N, width]."""
    p = 1 + sd + ad
    rows = np.asarray(rows)
    return rows[:, :p * sd].reshape(-1, p, sd), rows[:, p * sd:]


def ratios(got, ref, d_w, d_r, sd, ad):
    """(worst ||W^_:j - W_:j||_2 / dW_j, worst |r^_j - r_j| / dr_j); a zero bound asks for a zero error."""
    w_got, r_got = split(np.asarray(got, dtype=np.float64), sd, ad)
    w_ref, r_ref = split(ref, sd, ad)
    e_w = np.linalg.norm(w_got - w_ref, axis=1)
    e_r = np.abs(r_got - r_ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        q_w = np.where(d_w > 0, e_w / d_w, np.where(e_w == 0, 0.0, np.inf))
        q_r = np.where(d_r > 0, e_r / d_r, np.where(e_r == 0, 0.0, np.inf))
    return float(q_w.max()), float(q_r.max())


# ---------------------------------------------------------------- the kernel's form, in numpy
def plan(ts, sd, ad, itemsize):
    """(dual, k, trajectories a workgroup, runs of steps of the primal's residual sums): csrc/sysid.h's plan."""
    m, p = ts - 1, 1 + sd + ad
    dual = m < p
    k = m if dual else p

    def r16(b):
        return (b + 15) // 16 * 16

    def slot(per_traj):
        nseg = 0 if dual else max(1, min(per_traj // sd, m))
        return 16 + r16(ts * (p | 1) * itemsize) + r16(k * (k | 1) * itemsize) + r16(k * sd * itemsize) \
            + r16(nseg * sd * itemsize)
    if slot(256) > 160 * 1024:
        return None
    per_traj = 16
    while per_traj < 256 and 2 * per_traj <= width(sd, ad):
        per_traj *= 2
    group = 256 // per_traj
    while group > 1 and group * slot(256 // group) > 64 * 1024:
        group //= 2
    per_traj = 256 // group
    return dual, k, group, (0 if dual else max(1, min(per_traj // sd, m)))


def kernel_form(states, actions, ridge, dtype=np.float32):
    """The rows as csrc/sysid.h forms them -- the system it picks, its chains in its order, an fma as the exactly
    formed product added in double and rounded once more to ``dtype`` (a double rounding apart from the
    hardware's, which the bound's counts cover) -- vectorised over the trajectories, [N, width] in ``dtype``."""
    t = dtype
    phi, y = regressors(states, actions, dtype=t)
    n, m, p = phi.shape
    sd = y.shape[2]
    dual, k, _, nseg = plan(m + 1, sd, p - 1 - sd, np.dtype(t).itemsize)

    def fma(a, b, c):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(t)
    rcp_m = t(1) / t(m)
    mat = np.zeros((n, k, k), dtype=t)
    lead = phi if dual else np.swapaxes(phi, 1, 2)          # [n, k, chain]
    for q in range(lead.shape[2]):
        mat = fma(lead[:, :, None, q], lead[:, None, :, q], mat)
    mat = mat * rcp_m
    if dual:
        rhs = y.copy()
    else:
        rhs = np.zeros((n, p, sd), dtype=t)
        for s in range(m):
            rhs = fma(phi[:, s, :, None], y[:, s, None, :], rhs)
        rhs = rhs * rcp_m
    trace = np.zeros(n, dtype=t)
    for i in range(k):
        trace = trace + mat[:, i, i]
    rho = (t(ridge) * trace) / t(p)
    for i in range(k):
        mat[:, i, i] = mat[:, i, i] + rho
    for j in range(k):
        ljj = np.sqrt(mat[:, j, j])
        mat[:, j + 1:, j] = mat[:, j + 1:, j] / ljj[:, None]
        col = mat[:, j + 1:, j]
        mat[:, j + 1:, j + 1:] = fma(-col[:, :, None], col[:, None, :], mat[:, j + 1:, j + 1:])
    for i in range(k):
        mat[:, i, i] = np.sqrt(mat[:, i, i])
    for i in range(k):
        acc = rhs[:, i]
        for c in range(i):
            acc = fma(-mat[:, i, c, None], rhs[:, c], acc)
        rhs[:, i] = acc / mat[:, i, i, None]
    for i in range(k - 1, -1, -1):
        acc = rhs[:, i]
        for c in range(i + 1, k):
            acc = fma(-mat[:, c, i, None], rhs[:, c], acc)
        rhs[:, i] = acc / mat[:, i, i, None]
    if dual:
        w = np.zeros((n, p, sd), dtype=t)
        for s in range(m):
            w = fma(phi[:, s, :, None], rhs[:, s, None, :], w)
        w = w * rcp_m
        acc = np.zeros((n, sd), dtype=t)
        for s in range(m):
            e = rho[:, None] * rhs[:, s]
            acc = fma(e, e, acc)
    else:
        w = rhs
        seg_len = -(-m // nseg)
        acc = np.zeros((n, sd), dtype=t)
        for seg in range(nseg):
            part = np.zeros((n, sd), dtype=t)
            for s in range(min(seg * seg_len, m), min((seg + 1) * seg_len, m)):
                fit = np.zeros((n, sd), dtype=t)
                for c in range(p):
                    fit = fma(phi[:, s, c, None], w[:, c], fit)
                e = y[:, s] - fit
                part = fma(e, e, part)
            acc = acc + part
    r = np.sqrt(acc * rcp_m)
    return np.concatenate([w.reshape(n, -1), r], axis=1)
