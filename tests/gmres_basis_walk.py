"""The GKOGMRES loop as a NumPy walk with a selectable precision of the STORED Krylov basis:
tests/gmres_ortho_walk.gmres_walk restated with a `basis` argument.  With basis "double" it is that walk bit for bit
(tests/test_gmres_basis_walk.py pins it); with "single" every store into the basis is rounded once to binary32
(nearest-even) and every operation on the basis sees the exact widening of what was stored -- the contract of the property
basisPrecision.  The Gram-Schmidt steps and the criterion are the ones of gmres_ortho_walk and mixed_walk, imported, not
restated.  Shared by tests/test_gmres_basis_walk.py (CPU) and tests/test_gpu_gmres_basis.py."""
import math

import numpy as np

from gmres_ortho_walk import ORTHO, Walk, verdict

BASIS_CODE = {"double": 0, "single": 1}
FLT_MIN = 2.0 ** -126  # the smallest normal binary32: a store in (0, FLT_MIN) is not pinned (flushed or not)


def gmres_walk(oracle, rp, cols, vals, b, x0, precond=None, ortho="mgs", basis="double", tolerance=1e-6, rel_tol=1e-6,
               min_iter=0, max_iter=1000, krylov_dim=0):
    """Call under helpers.blocked for the device's bits.  precond: an oracle.Precond or None.  Evaluation frequency 1.
    Beyond gmres_ortho_walk's result: w.basis (the stored vectors of the last cycle, in their stored type) and
    w.subnormal_stores (stores into the basis whose value lies in (0, 2^-126): 0 wherever the bits are to be compared)."""
    step = ORTHO[ortho]
    single = bool(BASIS_CODE[basis])
    rp32, cols32 = np.asarray(rp, np.int32), np.asarray(cols, np.int32)
    vals, b = np.asarray(vals, np.float64), np.asarray(b, np.float64)
    A = oracle.DistMatrix(rp32, cols32, vals)
    apply_m = (lambda v: v.copy()) if precond is None else precond.apply
    n, m = b.size, (krylov_dim if krylov_dim > 0 else 100)
    x = np.array(x0, np.float64, copy=True)
    stored = [None] * (m + 1)   # what memory holds: float32 arrays with basis "single"
    V = [None] * (m + 1)        # wide(stored): what every operation on the basis sees
    H = np.zeros((m + 1, m))
    gs, gc, rnc, y = np.zeros(m), np.zeros(m), np.zeros(m + 1), np.zeros(m)
    history = np.zeros(max(max_iter, min_iter) + 5)
    columns = []
    state = dict(r=None, S=0.0, subnormal=0)

    def store(j, v):
        """V_j = v (double) or fl32(v): one rounding to binary32, then the exact widening."""
        if single:
            a = np.abs(v)
            state["subnormal"] += int(np.count_nonzero((a > 0.0) & (a < FLT_MIN)))
            stored[j] = v.astype(np.float32)
            V[j] = stored[j].astype(np.float64)
        else:
            stored[j] = V[j] = v

    def restart():
        r = oracle.spmv_adv(rp32, cols32, vals, -1.0, x, 1.0, b)
        rn = math.sqrt(oracle.dot(r, r))
        rnc[0] = rn
        store(0, r / rn)
        state["r"], state["S"] = r, oracle.norm1(r)

    def update_x(cols_done):
        for i in range(cols_done - 1, -1, -1):            # solve_upper_triangular
            t = rnc[i]
            for j in range(i + 1, cols_done):
                t -= H[i, j] * y[j]
            y[i] = t / H[i, i]
        s = np.zeros(n)
        for j in range(cols_done):                        # calculate_qy
            s = s + V[j] * y[j]
        return x + apply_m(s)

    restart()
    norm_factor = oracle.compute_normfactor(A, state["r"], x, b)
    it = checks = n_evals = 0
    init_res = res = 0.0
    while True:
        evaluated, n_evals, init_res, res_k, stop = verdict(tolerance, rel_tol, min_iter, max_iter, checks, n_evals,
                                                            init_res, norm_factor, state["S"])
        if evaluated:
            history[checks] = res = res_k
        checks += 1
        if stop:
            break
        if it == m:
            x = update_x(m)
            restart()
            it = 0
        nx = A.apply(apply_m(V[it]))
        h, nx = step(oracle, nx, V[:it + 1])
        hn = math.sqrt(oracle.dot(nx, nx))
        H[:it + 1, it] = h
        H[it + 1, it] = hn
        columns.append((it, [float(v) for v in h] + [hn]))
        store(it + 1, nx / hn)
        for j in range(it):                               # givens_rotation: the previous rotations
            t = gc[j] * H[j, it] + gs[j] * H[j + 1, it]
            H[j + 1, it] = -gs[j] * H[j, it] + gc[j] * H[j + 1, it]
            H[j, it] = t
        if H[it, it] == 0.0:
            gc[it], gs[it] = 0.0, 1.0
        else:
            scale = abs(H[it, it]) + abs(H[it + 1, it])
            a0, a1 = H[it, it] / scale, H[it + 1, it] / scale
            hyp = scale * math.sqrt(a0 * a0 + a1 * a1)
            gc[it], gs[it] = H[it, it] / hyp, H[it + 1, it] / hyp
        H[it, it] = gc[it] * H[it, it] + gs[it] * H[it + 1, it]
        H[it + 1, it] = 0.0
        rnc[it + 1] = -gs[it] * rnc[it]
        rnc[it] = gc[it] * rnc[it]
        it += 1
    if it > 0:
        x = update_x(it)
    w = Walk()
    w.x, w.n_iterations, w.n_evals, w.history, w.columns = x, checks, n_evals, history[:checks].copy(), columns
    w.initial_residual, w.final_residual, w.norm_factor = init_res, res, norm_factor
    w.basis = [v for v in stored if v is not None]
    w.subnormal_stores = state["subnormal"]
    return w
