"""The GKOGMRES loop as a NumPy walk with a selectable Gram-Schmidt step: restarted,
right-preconditioned GMRES composed from the oracle's pieces -- oracle.dot / norm1, DistMatrix.apply, Precond.apply,
oracle.compute_normfactor -- and the criterion as tests/mixed_walk.py states it.  Every product, sum, difference and
quotient of a vector step is one NumPy float64 operation, rounded once; under helpers.blocked the sums run in the
device's tree.  With ortho "mgs" the walk is oracle.gmres restated (tests/test_gmres_ortho_walk.py pins that bit for bit);
"cgs" and "cgs2" are the contract of the property orthoMethod.  Shared by tests/test_gmres_ortho_walk.py (CPU) and
tests/test_gpu_gmres_ortho.py."""
import math

import numpy as np

from mixed_walk import verdict

ORTHO_CODE = {"mgs": 0, "cgs": 1, "cgs2": 2}


class Walk:
    pass


def ortho_mgs(oracle, w, V):
    """finish_arnoldi as oracle.gmres has it: one link after another, each dot product on the w the link before left."""
    h = []
    for v in V:
        hj = oracle.dot(w, v)
        h.append(hj)
        w = w - hj * v
    return h, w


def _cgs_round(oracle, w, V):
    h = [oracle.dot(w, v) for v in V]   # all on the same unmodified w
    t = w
    for hj, v in zip(h, V):             # row i: t = w_i, then t = t - h_j v_ji for j ascending
        t = t - hj * v
    return h, t


def ortho_cgs(oracle, w, V):
    return _cgs_round(oracle, w, V)


def ortho_cgs2(oracle, w, V):
    h, w = _cgs_round(oracle, w, V)
    g, w = _cgs_round(oracle, w, V)
    return [hj + gj for hj, gj in zip(h, g)], w   # H(j, it) = h_j + g_j, one rounded sum


ORTHO = {"mgs": ortho_mgs, "cgs": ortho_cgs, "cgs2": ortho_cgs2}


def gmres_walk(oracle, rp, cols, vals, b, x0, precond=None, ortho="mgs", tolerance=1e-6, rel_tol=1e-6, min_iter=0,
               max_iter=1000, krylov_dim=0):
    """Call under helpers.blocked for the device's bits.  precond: an oracle.Precond or None.  Evaluation frequency 1."""
    step = ORTHO[ortho]
    rp32, cols32 = np.asarray(rp, np.int32), np.asarray(cols, np.int32)
    vals, b = np.asarray(vals, np.float64), np.asarray(b, np.float64)
    A = oracle.DistMatrix(rp32, cols32, vals)
    apply_m = (lambda v: v.copy()) if precond is None else precond.apply
    n, m = b.size, (krylov_dim if krylov_dim > 0 else 100)
    x = np.array(x0, np.float64, copy=True)
    V = [None] * (m + 1)
    H = np.zeros((m + 1, m))
    gs, gc, rnc, y = np.zeros(m), np.zeros(m), np.zeros(m + 1), np.zeros(m)
    history = np.zeros(max(max_iter, min_iter) + 5)
    columns = []          # (it, [H(0, it) .. H(it, it), H(it + 1, it)]) of every turn, before the rotations
    state = dict(r=None, S=0.0)

    def restart():
        r = oracle.spmv_adv(rp32, cols32, vals, -1.0, x, 1.0, b)
        rn = math.sqrt(oracle.dot(r, r))
        rnc[0] = rn
        V[0] = r / rn
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
        V[it + 1] = nx / hn
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
    return w


def true_residual(oracle, rp, cols, vals, b, x, norm_factor):
    """sum |b - A x| / norm_factor with the oracle's SpMV and norm1, as mixed_walk.true_residual forms it."""
    r = oracle.spmv_adv(np.asarray(rp, np.int32), np.asarray(cols, np.int32), vals, -1.0, x, 1.0, b)
    return oracle.norm1(r) / norm_factor
