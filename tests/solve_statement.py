"""Independent float64 statement of ONE linearisation of the reference-parity solve: the normal matrix JᵀJ = A ⊗ I₃,
the right-hand side g = -Jᵀr, every row's column set and a per-entry error budget, plus the statement's own solution of
A x = g.  Written from the reference, not from dynfu_amd/csrc/solve_*.hip or oracle/solve_oracle_body.inc:

* data term (energy.t:50-55): per vertex v with k-NN nodes n_0..n_{k-1} of its canonical position,
  r_v = sqrt(tau_v) (live_v - canon_v - sum_i w_vi t_{n_i}), w_vi the RBF weight exp(-|canon_v - dg_v|^2 / (2 dg_w^2))
  (energy.t:15-16, node.cpp:35);
* regulariser (energy.t:75-78): per node n and each of its k nearest nodes m, r_nm = w_reg ((dg_v_m - t_n) - (dg_v_m - t_m))
  = w_reg (t_m - t_n); the self edge m = n is empty (zero residual, zero Jacobian);
* w_reg = sqrt(lambda / (D k)) (opt_solver.cpp:30);
* graphs (opt_solver.cpp:56-105): the data graph is the k-NN of each canonical vertex among the nodes, the
  regularisation graph the k-NN of each node among the nodes (itself first); a slot of -1 (fewer than k nodes) is empty.

A row with tau = 0 contributes nothing (no value, no column).  Accumulation is vectorised: every slot pair (i, j) of
every row is an addend keyed by a * D + b, summed with a sort and reduceat, never a Python loop over rows.
"""
import numpy as np

U32 = 2.0 ** -24  # unit round-off of float32


def rbf_weights(node_pos, node_w, canon, idx):
    """exp(-|v - g|^2 / (2 w^2)) in float64 (node.cpp:35, energy.t:15-16); 0 at an empty slot"""
    p = np.asarray(node_pos, np.float64)
    nw = np.asarray(node_w, np.float64)
    v = np.asarray(canon, np.float64)
    ii = np.where(idx >= 0, idx, 0)
    d2 = ((v[:, None, :] - p[ii]) ** 2).sum(-1)
    w = np.exp(-d2 / (2.0 * nw[ii] ** 2))
    return np.where(idx >= 0, w, 0.0)


def knn_graph(node_pos, query, k):
    """brute-force k-NN of each query among the nodes in float64, ties to the lower index, -1 past D"""
    p = np.asarray(node_pos, np.float64)
    q = np.asarray(query, np.float64)
    D = len(p)
    out = np.full((len(q), k), -1, np.int32)
    kk = min(k, D)
    for s in range(0, len(q), 4096):
        d2 = ((q[s:s + 4096, None, :] - p[None, :, :]) ** 2).sum(-1)
        order = np.lexsort((np.broadcast_to(np.arange(D), d2.shape), d2), axis=-1)[:, :kk]
        out[s:s + 4096, :kk] = order
    return out


class Statement:
    """One linearisation.  Attributes:
    rows, cols, vals   -- A in COO form, sorted by (row, col); JᵀJ = A ⊗ I₃
    n_add, abs_sum     -- per entry: number of addends and sum of their magnitudes
    reg_add            -- per entry: number of regularisation addends (their tau w_reg^2 is rounded on the device)
    g                  -- (D, 3) right-hand side -Jᵀr at t
    g_abs, g_err       -- (D, 3) sum of |addend| of g and a first-order bound on float32 evaluation of each addend
    amax               -- the largest tau (max_j |w_j|)^2 of any row, in float32 (the device's fixed-point bound)
    list_len           -- (D,) rows that name each node (data and regularisation, any tau)
    cost               -- sum of squared residuals at t
    """

    def __init__(self, node_pos, node_w, k, canon, live, data_idx, tau, lam, t=None, rbf=None, reg_idx=None):
        D = len(node_pos)
        N = len(canon)
        self.D, self.k = D, k
        data_idx = np.asarray(data_idx, np.int64).reshape(N, k)
        tau = np.asarray(tau, np.float64).reshape(N)
        w = rbf_weights(node_pos, node_w, canon, data_idx) if rbf is None else np.where(data_idx >= 0, np.asarray(rbf, np.float64), 0.0)
        if reg_idx is None:
            reg_idx = knn_graph(node_pos, node_pos, k)
        reg_idx = np.asarray(reg_idx, np.int64).reshape(D, k)
        t = np.zeros((D, 3)) if t is None else np.asarray(t, np.float64).reshape(D, 3)
        tau_reg = lam / (D * k)  # w_reg^2 (opt_solver.cpp:30)

        # regularisation rows (energy.t:75-78): ids (m, n), weights (-1, +1) so that sum_j w_j t_j = t_n - t_m
        n_of = np.repeat(np.arange(D), k)
        m_of = reg_idx.reshape(-1)
        keep = (m_of >= 0) & (m_of != n_of)
        rid = np.stack([m_of[keep], n_of[keep]], 1)
        rw = np.tile(np.array([-1.0, 1.0]), (len(rid), 1))

        # every row in one padded table: ids (-1 = empty), weights, right-hand side b, tau
        kk = max(k, 2)
        ids = np.full((N + len(rid), kk), -1, np.int64)
        ws = np.zeros((N + len(rid), kk))
        ids[:N, :k], ws[:N, :k] = data_idx, w
        ids[N:, :2], ws[N:, :2] = rid, rw
        b = np.zeros((N + len(rid), 3))
        b[:N] = np.asarray(live, np.float64) - np.asarray(canon, np.float64)
        taus = np.concatenate([tau, np.full(len(rid), tau_reg)])
        is_reg = np.arange(len(taus)) >= N
        valid = ids >= 0
        ws = np.where(valid, ws, 0.0)

        self.list_len = np.bincount(ids[valid], minlength=D)
        wm = np.where(valid, np.abs(ws), 0.0).max(1).astype(np.float32)
        self.amax = float((taus.astype(np.float32) * wm * wm).max()) if len(taus) else 0.0

        # residual e = b - sum_j w_j t_j (the data residual / sqrt(tau), energy.t:55), the gradient and the cost
        tg = t[np.where(valid, ids, 0)]
        wt = ws[..., None] * tg
        e = b - wt.sum(1)
        self.cost = float((taus * (e * e).sum(1)).sum())
        live_rows = taus != 0.0
        ga, gabs, gerr = (np.zeros((D, 3)) for _ in range(3))
        # first-order bound on a float32 addend fl(fl(tau w_a) e): b rounded once, sum_j w_j t_j in k steps, e rounded,
        # tau w_a and the product rounded (tau itself is exact: the device's own when it is given, w_reg^2 within 3 u)
        e_err = U32 * np.abs(b) + (k + 1) * U32 * np.abs(wt).sum(1) + U32 * np.abs(e)
        for j in range(kk):
            sel = valid[:, j] & live_rows
            a = ids[sel, j]
            tw = taus[sel] * ws[sel, j]
            add = tw[:, None] * e[sel]
            err = np.abs(tw)[:, None] * (e_err[sel] + 2 * U32 * np.abs(e[sel]) + np.where(is_reg[sel], 3 * U32, 0.0)[:, None] * np.abs(e[sel]))
            for c in range(3):
                ga[:, c] += np.bincount(a, add[:, c], minlength=D)
                gabs[:, c] += np.bincount(a, np.abs(add[:, c]), minlength=D)
                gerr[:, c] += np.bincount(a, err[:, c], minlength=D)
        self.g, self.g_abs, self.g_err = ga, gabs, gerr

        # A: every slot pair (i, j) of every row with tau != 0, keyed by a * D + b
        keys, vals, regs = [], [], []
        for i in range(kk):
            for j in range(kk):
                sel = valid[:, i] & valid[:, j] & live_rows
                keys.append(ids[sel, i] * D + ids[sel, j])
                vals.append(taus[sel] * ws[sel, i] * ws[sel, j])
                regs.append(is_reg[sel])
        keys = np.concatenate(keys) if keys else np.zeros(0, np.int64)
        vals = np.concatenate(vals) if vals else np.zeros(0)
        regs = np.concatenate(regs) if regs else np.zeros(0, bool)
        order = np.argsort(keys, kind="stable")
        keys, vals, regs = keys[order], vals[order], regs[order]
        starts = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]]) if len(keys) else np.zeros(0, np.int64)
        uk = keys[starts]
        self.n_add = np.diff(np.r_[starts, len(keys)])
        self.vals = np.add.reduceat(vals, starts) if len(keys) else np.zeros(0)
        self.abs_sum = np.add.reduceat(np.abs(vals), starts) if len(keys) else np.zeros(0)
        self.reg_add = np.add.reduceat(regs.astype(np.int64), starts) if len(keys) else np.zeros(0, np.int64)
        self.rows, self.cols = uk // D, uk % D
        # a diagonal whose sum is 0 (every addend 0) is not an entry
        drop = (self.rows == self.cols) & (self.vals == 0.0)
        if drop.any():
            for name in ("rows", "cols", "vals", "n_add", "abs_sum", "reg_add"):
                setattr(self, name, getattr(self, name)[~drop])
        self.row_ptr = np.searchsorted(self.rows, np.arange(D + 1))

    # ------------------------------------------------------------------ views
    def row_lengths(self):
        return np.diff(self.row_ptr)

    def columns(self, a):
        return self.cols[self.row_ptr[a]:self.row_ptr[a + 1]]

    def dense(self):
        M = np.zeros((self.D, self.D))
        M[self.rows, self.cols] = self.vals
        return M

    def matvec(self, x):
        """A x for x of shape (D,) or (D, 3)"""
        x = np.asarray(x, np.float64)
        if x.ndim == 1:
            return np.bincount(self.rows, self.vals * x[self.cols], minlength=self.D)
        return np.stack([np.bincount(self.rows, self.vals * x[self.cols, c], minlength=self.D) for c in range(x.shape[1])], 1)

    def fixed_quantum(self, extra_bits=0):
        """one unit of the device's fixed-point grid per node: 2^(e - 40 + extra), amax < 2^e, extra = the bits a list of
        more than 2^22 rows gives up (one per doubling)"""
        _, e = np.frexp(np.float32(max(self.amax, 1e-30)))
        e = int(np.clip(e, -80, 100))
        extra = np.array([int(n >> 22).bit_length() for n in self.list_len]) + extra_bits
        return np.ldexp(1.0, e - 40 + extra)

    def budget(self, deterministic=False):
        """per-entry bound on |A_device - A| when the device is given the same tau and RBF weights (float32):
        * each addend fl(fl(tau w_a) w_b): 2 u |addend| (+ 3 u for a regularisation addend, whose w_reg^2 is rounded);
        * off-diagonal: one grid quantum per addend (truncation to 2^(e - 40 + extra));
        * diagonal: summed in float32 registers — a thread's ceil(n / 256) addends, a 64-lane wave reduction (6 levels),
          four wave partials — gamma_(ceil(n/256) + 8) sum|addend|; the default path adds the four partials on the grid
          (4 quanta), the order-stable one in float32;
        * the final conversion to float32: u |A|; float64 of the statement itself: 1e-15 sum|addend|."""
        q = self.fixed_quantum()[self.rows]
        diag = self.rows == self.cols
        b = 2 * U32 * self.abs_sum + 3 * U32 * self.reg_add * (self.abs_sum / np.maximum(self.n_add, 1))
        b = b + np.where(diag, 0.0, self.n_add * q)
        m = np.ceil(self.n_add / 256.0) + 8
        b = b + np.where(diag, m * U32 * self.abs_sum + (0.0 if deterministic else 4.0) * q, 0.0)
        return b + U32 * np.abs(self.vals) + 1e-15 * self.abs_sum

    def grid_share(self, deterministic=False):
        """the part of budget() that the fixed-point grid contributes"""
        q = self.fixed_quantum()[self.rows]
        diag = self.rows == self.cols
        return np.where(diag, 0.0 if deterministic else 4.0 * q, self.n_add * q)

    def g_budget(self):
        """bound on |g_device - g|: each float32 addend (g_err) plus the float32 sum of a node's list, gamma_(m + 8)"""
        m = np.ceil(self.list_len / 256.0)[:, None] + 8
        return self.g_err + m * U32 * self.g_abs + 1e-15 * self.g_abs

    # ------------------------------------------------------------------ solving the statement's own system
    def solve(self, rhs=None, tol=1e-13, max_iter=20000):
        """x with A x = g per coordinate: dense solve up to 4 096 nodes, float64 CG to 1e-13 beyond"""
        g = self.g if rhs is None else np.asarray(rhs, np.float64)
        if self.D <= 4096:
            return np.linalg.solve(self.dense(), g)
        x = np.zeros_like(g)
        r = g.copy()
        p = r.copy()
        rr = (r * r).sum(0)
        rr0 = rr.copy()
        for _ in range(max_iter):
            if (rr <= tol * tol * rr0).all():
                break
            Ap = self.matvec(p)
            alpha = rr / np.maximum((p * Ap).sum(0), 1e-300)
            x += alpha * p
            r -= alpha * Ap
            rr_new = (r * r).sum(0)
            p = r + (rr_new / np.maximum(rr, 1e-300)) * p
            rr = rr_new
        return x

    def lambda_min(self):
        """smallest eigenvalue of A (dense, float64)"""
        return float(np.linalg.eigvalsh(self.dense())[0])
