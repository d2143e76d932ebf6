"""The initial guess from the last solutions (keyword guessProjection K) as a NumPy walk composed from
the oracle's pieces -- oracle.spmv_adv (the prologue's residual product), DistMatrix.apply (the in-loop product),
oracle.dot / norm1.  Every product, difference, quotient and root of the small solve is one Python float operation,
rounded once; every vector step one NumPy float64 operation; under helpers.blocked the sums run in the device's tree.
Shared by tests/test_guess_projection_walk.py (CPU) and tests/test_gpu_guess_projection.py, together with the time-step
sequence both run."""
import math

import numpy as np

from ogl_amd import synthetic

K_MAX = 8
TAU = 2.0 ** -32


class Walk:
    pass


def small_solve(G, g):
    """Cholesky with dropping of the lower triangle of G (k x k floats), then the two triangular solves: (alpha, kept
    flags).  A dropped column has alpha +0.0; one alpha that is not finite zeroes them all (and nothing counts as kept)."""
    k = len(g)
    L = [[0.0] * k for _ in range(k)]
    kept = [False] * k
    for j in range(k):
        gjj = float(G[j][j])
        s = gjj
        for m in range(j):
            if kept[m]:
                s = s - L[j][m] * L[j][m]
        kept[j] = bool(s > TAU * gjj)
        if not kept[j]:
            continue
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, k):
            t = float(G[i][j])
            for m in range(j):
                if kept[m]:
                    t = t - L[i][m] * L[j][m]
            L[i][j] = _div(t, L[j][j])
    y = [0.0] * k
    for j in range(k):
        if kept[j]:
            t = float(g[j])
            for m in range(j):
                if kept[m]:
                    t = t - L[j][m] * y[m]
            y[j] = _div(t, L[j][j])
    alpha = [0.0] * k
    for j in range(k - 1, -1, -1):
        if kept[j]:
            t = y[j]
            for m in range(j + 1, k):
                if kept[m]:
                    t = t - L[m][j] * alpha[m]
            alpha[j] = _div(t, L[j][j])
    if not all(math.isfinite(a) for a in alpha):
        return [0.0] * k, [False] * k
    return alpha, kept


def _div(a, b):
    """IEEE quotient of two Python floats (b is a root of a positive number here, never zero; a may be inf or NaN)."""
    return float(np.float64(a) / np.float64(b))


def gram(oracle, rp, cols, vals, b, x0, ring):
    """(r0, S0, W, g, G): step 2 to 4 of the pre-step.  G: its lower triangle, G[i][j] for i >= j."""
    rp32, cols32 = np.asarray(rp, np.int32), np.asarray(cols, np.int32)
    A = oracle.DistMatrix(rp32, cols32, vals)
    r0 = oracle.spmv_adv(rp32, cols32, vals, -1.0, x0, 1.0, b)
    W = [A.apply(d) for d in ring]
    g = [oracle.dot(w, r0) for w in W]
    G = [[oracle.dot(W[i], W[j]) if j <= i else 0.0 for j in range(len(W))] for i in range(len(W))]
    return r0, oracle.norm1(r0), W, g, G


def project(oracle, rp, cols, vals, b, x0, ring):
    """The pre-step on a ring (a list of vectors, oldest first): a Walk with x (the projected guess; x0 itself, the same
    bits, for an empty ring), alpha, kept (columns the projection kept), norm_before (S0; 0.0 for an empty ring) and the
    sums g, G."""
    w = Walk()
    x0 = np.array(x0, np.float64, copy=True)
    w.offered = len(ring)
    if not ring:
        w.x, w.alpha, w.kept, w.norm_before, w.g, w.G, w.W, w.r0 = x0, [], 0, 0.0, [], [], [], None
        return w
    with np.errstate(all="ignore"):
        w.r0, w.norm_before, w.W, w.g, w.G = gram(oracle, rp, cols, vals, b, x0, ring)
        w.alpha, flags = small_solve(w.G, w.g)
        w.flags = flags
        w.kept = sum(flags)
        t = x0
        for a, d in zip(w.alpha, ring):   # row i: t = x_i, then t = t - h_j d_ji with h_j = -alpha_j, j ascending
            t = t - (-a) * np.asarray(d, np.float64)
        w.x = t
    return w


class Ring:
    """The stored steps of one field, oldest first."""

    def __init__(self, K):
        assert 0 <= K <= K_MAX
        self.K, self.vectors = K, []

    def store(self, d):
        if self.K == 0:
            return
        self.vectors.append(np.array(d, np.float64, copy=True))
        del self.vectors[:-self.K]


def step(oracle, ring, rp, cols, vals, b, x0, solve, turned):
    """One solve of a field with the keyword: the pre-step, solve(guess) -> a result with .x, the post-step.
    turned(result): whether a turn ran.  Returns (projection, result)."""
    p = project(oracle, rp, cols, vals, b, x0, ring.vectors if ring.K else [])
    res = solve(p.x)
    if ring.K and (p.kept >= 1 or turned(res)):
        ring.store(res.x - x0)           # the whole step x_final - x0, one rounded difference per row
    p.stored = len(ring.vectors)
    return p, res


# ---- the time-step sequence of the tests: 10 x 9 x 7, coefficients varied per step, x*(t) in four fixed modes ----

SEQ_SHAPE = (10, 9, 7)
SEQ_DT = 0.1
SEQ_CRITERION = dict(tolerance=1e-9, rel_tol=0.0)
_modes = []


def sequence_case(n):
    """The system of step n: the 7-point pattern with every face coefficient and the diagonal shift moving with n."""
    nx, ny, nz = SEQ_SHAPE
    lower_addr, upper_addr = synthetic.box_faces(nx, ny, nz)
    N, F = nx * ny * nz, lower_addr.size
    upper = -(1.0 + 0.3 * np.sin(0.4 * n + 0.05 * np.arange(F)))
    diag = np.zeros(N)
    np.add.at(diag, lower_addr, -upper)
    np.add.at(diag, upper_addr, -upper)
    diag += 0.02 * (1.0 + 0.2 * math.sin(n))
    return synthetic.LduCase(N, lower_addr, upper_addr, diag, upper, None)


def sequence_x_star(t):
    nx, ny, nz = SEQ_SHAPE
    if not _modes:
        rng = np.random.default_rng(3)
        zc, yc, xc = np.meshgrid(np.linspace(0, 1, nz), np.linspace(0, 1, ny), np.linspace(0, 1, nx), indexing="ij")
        for i in range(4):
            u = np.sin(np.pi * (i + 1) * xc) * np.cos(np.pi * i * yc) * (1 + zc * i)
            _modes.append(u.ravel() + 0.01 * rng.standard_normal(u.size))
    U = _modes
    return U[0] + t * U[1] + t * t * U[2] + math.sin(3 * t) * U[3]


def sequence_rhs(case, n):
    return synthetic.apply_case(case, sequence_x_star(SEQ_DT * n))


def run_sequence(oracle, K, steps, csr_of):
    """The loop with the oracle's Jacobi-CG from each projected guess, the first guess zero and every later one the previous
    solution.  csr_of(case) -> (rp, cols, vals).  Returns a list of (projection, result, ring as a list of vectors)."""
    ring, out = Ring(K), []
    x = np.zeros(SEQ_SHAPE[0] * SEQ_SHAPE[1] * SEQ_SHAPE[2])
    for n in range(steps):
        case = sequence_case(n)
        rp, cols, vals = csr_of(case)
        b = sequence_rhs(case, n)
        A = oracle.DistMatrix(rp, cols, vals)
        inv = oracle.jacobi_generate_scalar(rp, cols, vals)
        p, res = step(oracle, ring, rp, cols, vals, b, x,
                      lambda guess: oracle.cg(A, b, guess, inv, max_iter=1000, **SEQ_CRITERION),
                      lambda r: r.n_iterations >= 2)
        out.append((p, res, [v.copy() for v in ring.vectors]))
        x = res.x
    return out
