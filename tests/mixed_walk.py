"""The contract of the mixed-precision mode as a NumPy walk: fp32 inner CG on A32 = fl32(A)
under an fp64 iterative refinement.  Every fp32 product and sum is one NumPy float32 operation (rounded once), every
quotient is formed in float64 and rounded once, the wide sums are the oracle's reductions on the float64 casts -- under
helpers.blocked they run in the device's tree.  Shared by tests/test_mixed_walk.py (CPU) and
tests/test_gpu_mixed_precision.py."""
import numpy as np

F32, F64 = np.float32, np.float64
TINY32 = 2.0 ** -126  # smallest normal binary32 magnitude

STOP_CRITERION, STOP_MAX_ITER, STOP_NO_PROGRESS, STOP_BREAKDOWN = 0, 1, 2, 3


def spmv32(rp, cols, a32, x32, track=None):
    """y = A32 x: every row summed from 0.0f in ascending stored column order, fp32 products and sums.  track: a Tracker
    that sees every product and every partial sum."""
    rp = np.asarray(rp, np.int64)
    n = rp.size - 1
    lens = np.diff(rp)
    y = np.zeros(n, F32)
    x32 = np.asarray(x32, F32)
    for s in range(int(lens.max()) if n else 0):
        rows = np.nonzero(lens > s)[0]
        k = rp[rows] + s
        prod = a32[k] * x32[cols[k]]
        y[rows] = y[rows] + prod
        if track is not None:
            track(prod)
            track(y[rows])
    return y


class Tracker:  # (defined before its first use at call time)
    """Smallest nonzero magnitude of every fp32 intermediate that passes through it."""

    def __init__(self):
        self.smallest = np.inf

    def __call__(self, v):
        a = np.abs(np.asarray(v, F64))
        a = a[a > 0]
        if a.size:
            self.smallest = min(self.smallest, float(a.min()))
        return v


class Walk:
    pass


def verdict(tolerance, rel_tol, min_iter, max_iter, it, n_evals, init_res, norm_factor, norm):
    """criterion_verdict (device_common.hpp) with frequency 1: (evaluated, n_evals, init_res, res, stop)."""
    if 0 < it < min_iter:
        return False, n_evals, init_res, 0.0, False
    res = norm / norm_factor
    if it == 0:
        init_res = res
    stop = it >= max_iter or res < tolerance or (rel_tol > 0 and res < rel_tol * init_res)
    return True, n_evals + 1, init_res, res, stop


def mixed_walk(oracle, rp, cols, vals, b, x0, inv_d=None, tolerance=1e-6, rel_tol=1e-6, min_iter=0, max_iter=1000,
               inner_rel_tol=1e-4, inner_max_iter=1000):
    """Call under helpers.blocked for the device's bits.  inv_d: the fp64 inverse diagonal (BJ, maxBlockSize 1) or None."""
    track = Tracker()
    rp, cols = np.asarray(rp, np.int64), np.asarray(cols, np.int64)
    vals, b = np.asarray(vals, F64), np.asarray(b, F64)
    a32 = track(vals.astype(F32))
    d32 = None if inv_d is None else track(np.asarray(inv_d, F64).astype(F32))
    assert np.all(np.isfinite(a32)) and (d32 is None or np.all(np.isfinite(d32)))
    wide = lambda u, v: oracle.dot(u.astype(F64), v.astype(F64))
    wide1 = lambda u: oracle.norm1(u.astype(F64))
    A = oracle.DistMatrix(rp.astype(np.int32), cols.astype(np.int32), vals)
    x = np.array(x0, F64, copy=True)
    residual = lambda: oracle.spmv_adv(rp.astype(np.int32), cols.astype(np.int32), vals, -1.0, x, 1.0, b)
    # O0
    r = residual()
    norm_factor = oracle.compute_normfactor(A, r, x, b)
    S = oracle.norm1(r)
    T = k = n_evals = 0
    init_res = res = 0.0
    history, t_prev, S_prev, reason, step_turns = [], None, None, None, []
    w = Walk()
    while True:
        # O1
        evaluated, n_evals, init_res, res_k, stop = verdict(tolerance, rel_tol, min_iter, max_iter, T, n_evals, init_res,
                                                            norm_factor, S)
        if evaluated:
            history.append(res_k)
            res = res_k
        if stop:
            met = res_k < tolerance or (rel_tol > 0 and res_k < rel_tol * init_res)
            reason = STOP_CRITERION if met else STOP_MAX_ITER
        elif k >= 1:
            if t_prev == 0:
                reason = STOP_BREAKDOWN
            elif S >= S_prev or not np.isfinite(S):
                reason = STOP_NO_PROGRESS
            elif S == 0.0:
                reason = STOP_CRITERION
        if reason is not None:
            break
        # O2
        res_now = S / norm_factor
        want_abs, want_rel = tolerance, rel_tol * init_res
        nu = (want_abs if want_abs > want_rel else want_rel) / res_now
        half_nu = 0.5 * nu
        theta = inner_rel_tol if inner_rel_tol > half_nu else half_nu
        L = min(inner_max_iter, max_iter - T)
        k += 1
        # O3
        rt = track((r / S).astype(F32))
        # O4: the inner solve
        u = np.zeros_like(rt)
        z = rt if d32 is None else track(rt * d32)
        rho, tau0 = wide(rt, z), wide1(rt)
        rho_prev, p, t, nonfinite = 0.0, None, 0, not (np.isfinite(rho) and np.isfinite(tau0))
        for j in range(1, (0 if nonfinite else L) + 1):
            if j == 1 or rho_prev == 0.0:
                p = z.copy()
            else:
                p = track(z + track(F32(rho / rho_prev) * p))
            q = spmv32(rp, cols, a32, p, track)
            pi = wide(p, q)
            if pi == 0.0:
                break
            t = j
            if not np.isfinite(pi):
                nonfinite = True
                break
            a = F32(rho / pi)
            track(a)
            u = track(u + track(a * p))
            rt = track(rt - track(a * q))
            z = rt if d32 is None else track(rt * d32)
            rho_prev, rho, tau = rho, wide(rt, z), wide1(rt)
            if not (np.isfinite(rho) and np.isfinite(tau)):
                nonfinite = True
                break
            if tau <= theta * tau0:
                break
        T += t
        t_prev = t
        step_turns.append(t)
        # O5
        if not nonfinite:
            x = x + S * u.astype(F64)
        # O6
        r = residual()
        S_prev, S = S, oracle.norm1(r)
    w.x, w.n_iterations, w.n_evals, w.outer_steps, w.inner_turns, w.stop_reason = x, T + 1, n_evals, k, T, reason
    w.history = np.array(history, F64)
    w.step_turns = step_turns
    w.initial_residual, w.final_residual, w.norm_factor = init_res, res, norm_factor
    w.smallest_fp32 = track.smallest
    return w


def true_residual(oracle, rp, cols, vals, b, x, norm_factor):
    """sum |b - A x| / norm_factor in float64, sequential sums."""
    r = oracle.spmv_adv(np.asarray(rp, np.int32), np.asarray(cols, np.int32), vals, -1.0, x, 1.0, b)
    return float(np.sum(np.abs(r))) / norm_factor


def meets_criterion(res, init_res, tolerance, rel_tol):
    return res < tolerance or (rel_tol > 0 and res < rel_tol * init_res)
