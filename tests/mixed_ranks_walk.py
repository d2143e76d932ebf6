"""The contract of the mixed-precision mode on several ranks ("several ranks") as a NumPy walk per
rank: tests/mixed_walk.py's steps with the halo exchange and the all-reduce passed in.  The inner product is spmv32 on the
rank's rows, then, for boundary rows, acc = q_i; acc = acc + a32nl_k * recv32[col_k] over the row's non-local entries in
stored order (fp32 products and sums, rounded once each); every wide sum is the rank's sum in the oracle's tree, then summed
over the ranks by `allreduce`; the norm factor and the fp64 residual are the distributed oracle's.  Every scalar a
decision reads comes out of an all-reduce, so every rank takes every branch alike.  Shared by
tests/test_mixed_ranks_walk.py (CPU) and tests/mixed_ranks_worker.py."""
import numpy as np

from mixed_walk import (F32, F64, STOP_BREAKDOWN, STOP_CRITERION, STOP_MAX_ITER, STOP_NO_PROGRESS, Tracker, Walk, spmv32,
                        verdict)


def non_local32(nl_rp, nl_cols, a32nl, recv32, y, track=None):
    """y_i = y_i + a32nl_k * recv32[col_k] over row i's non-local entries in stored order."""
    nl_rp = np.asarray(nl_rp, np.int64)
    lens = np.diff(nl_rp)
    y = np.array(y, F32, copy=True)
    for s in range(int(lens.max()) if lens.size else 0):
        rows = np.nonzero(lens > s)[0]
        k = nl_rp[rows] + s
        prod = a32nl[k] * recv32[nl_cols[k]]
        y[rows] = y[rows] + prod
        if track is not None:
            track(prod)
            track(y[rows])
    return y


class RankSystem:
    """One rank's share: the local CSR, the non-local triplets (row-sorted), the send list, and the two collectives.
    exchange(send) -> recv over this rank's neighbours (float64 on the wire: binary32 values pass exactly);
    allreduce(a) -> a summed over the ranks.  Either may be None on one rank without interfaces."""

    def __init__(self, oracle, rp, cols, vals, nl_rows=None, nl_cols=None, nl_vals=None, send_idxs=None, exchange=None,
                 allreduce=None, global_n=None):
        self.rp, self.cols, self.vals = np.asarray(rp, np.int32), np.asarray(cols, np.int32), np.asarray(vals, F64)
        self.n = self.rp.size - 1
        empty = np.zeros(0, np.int32)
        self.nl_rows = empty if nl_rows is None else np.asarray(nl_rows, np.int32)
        self.nl_cols = empty if nl_cols is None else np.asarray(nl_cols, np.int32)
        self.nl_vals = np.zeros(0, F64) if nl_vals is None else np.asarray(nl_vals, F64)
        self.send_idxs = empty if send_idxs is None else np.asarray(send_idxs, np.int32)
        self.nl_rp = np.asarray(oracle.rowptr_from_rows(self.n, self.nl_rows), np.int32)
        self.exchange = exchange
        self.allreduce = allreduce if allreduce is not None else (lambda a: np.array(a, F64, copy=True))
        kw = {}
        if self.nl_rows.size:
            kw = dict(nl_rowptr=self.nl_rp, nl_cols=self.nl_cols, nl_vals=self.nl_vals, send_idxs=self.send_idxs,
                      n_halo=self.nl_rows.size, exchange=exchange)
        self.A = oracle.DistMatrix(self.rp, self.cols, self.vals, allreduce=allreduce, global_n=global_n, **kw)
        self.oracle = oracle

    def halo(self, x):
        return self.exchange(np.asarray(x, F64)[self.send_idxs]) if self.nl_rows.size else np.zeros(0, F64)

    def residual(self, b, x):
        """r = b - A x as the double path computes it: the local part, then the non-local part onto it."""
        o = self.oracle
        r = o.spmv_adv(self.rp, self.cols, self.vals, -1.0, x, 1.0, b)
        if self.nl_rows.size:
            r = o.spmv_adv(self.nl_rp, self.nl_cols, self.nl_vals, -1.0, self.halo(x), 1.0, r)
        return r

    def total(self, *values):
        """The ranks' sums of up to two values (one all-reduce)."""
        return self.allreduce(np.array(values, F64))


def product32(sys, a32, a32nl, p, track=None):
    """q = A32 p on this rank: collective (the halo of p travels as binary32 values)."""
    q = spmv32(sys.rp, sys.cols, a32, p, track)
    if sys.nl_rows.size:
        recv32 = sys.halo(p.astype(F64)).astype(F32)
        q = non_local32(sys.nl_rp, sys.nl_cols, a32nl, recv32, q, track)
    return q


def mixed_ranks_walk(sys, b, x0, inv_d=None, tolerance=1e-6, rel_tol=1e-6, min_iter=0, max_iter=1000, inner_rel_tol=1e-4,
                     inner_max_iter=1000):
    """Call under helpers.blocked for the device's bits, on every rank at once.  inv_d: the rank's own fp64 inverse diagonal
    (BJ, maxBlockSize 1) or None."""
    oracle, track = sys.oracle, Tracker()
    b = np.asarray(b, F64)
    a32, a32nl = track(sys.vals.astype(F32)), track(sys.nl_vals.astype(F32))
    d32 = None if inv_d is None else track(np.asarray(inv_d, F64).astype(F32))
    assert np.all(np.isfinite(a32)) and np.all(np.isfinite(a32nl)) and (d32 is None or np.all(np.isfinite(d32)))
    wide = lambda u, v: oracle.dot(u.astype(F64), v.astype(F64))
    wide1 = lambda u: oracle.norm1(u.astype(F64))
    x = np.array(x0, F64, copy=True)
    # O0: the double path's distributed prologue
    r = sys.residual(b, x)
    norm_factor = oracle.compute_normfactor(sys.A, r, x, b)
    S = sys.total(oracle.norm1(r), 0.0)[0]  # (next to S: the overflow count, 0 here)
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
        # O3: the global S, the rank's own inverse diagonal
        rt = track((r / S).astype(F32))
        # O4: the inner solve
        u = np.zeros_like(rt)
        z = rt if d32 is None else track(rt * d32)
        rho, tau0 = sys.total(wide(rt, z), wide1(rt))
        rho_prev, p, t, nonfinite = 0.0, None, 0, not (np.isfinite(rho) and np.isfinite(tau0))
        for j in range(1, (0 if nonfinite else L) + 1):
            if j == 1 or rho_prev == 0.0:
                p = z.copy()
            else:
                p = track(z + track(F32(rho / rho_prev) * p))
            q = product32(sys, a32, a32nl, p, track)
            pi = sys.total(wide(p, q))[0]
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
            rho_prev = rho
            rho, tau = sys.total(wide(rt, z), wide1(rt))
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
        r = sys.residual(b, x)
        S_prev, S = S, sys.total(oracle.norm1(r), 0.0)[0]
    w.x, w.n_iterations, w.n_evals, w.outer_steps, w.inner_turns, w.stop_reason = x, T + 1, n_evals, k, T, reason
    w.history = np.array(history, F64)
    w.step_turns = step_turns
    w.initial_residual, w.final_residual, w.norm_factor = init_res, res, norm_factor
    w.smallest_fp32 = track.smallest
    return w
