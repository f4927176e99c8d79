"""PoissonSolverAMR::solve (main.cpp:14404-14616) restated in plain NumPy, from the reference's text alone: the pipelined, preconditioned
BiCGSTAB with its every-50th true-residual refresh, its breakdown restart, its x_opt bookkeeping and its stopping rule.

  init(b, x0, A, Minv)          14408-14446 (zero_corner: 14404-14407)
  iteration(state, k, A, Minv)  one pass of the loop body 14450-14603
  solve(...)                    the loop 14449-14604 and 14605

A (= _lhs, with whatever mean-constraint row ComputeLHS 9282-9326 adds) and Minv (= _preconditioner) are callables the caller passes in:
array -> new array of the same shape.  Every elementwise update is written in the reference's association and evaluated in float64, one
rounding per operation, so with a bit-exact A and Minv the vectors are the reference's bit for bit.  Dot products (`dots`):
  "sequential"  float64, left to right -- the reference's order on one OpenMP thread (np.cumsum accumulates strictly in order)
  "longdouble"  products and sum in long double, rounded to float64 once

State: a dict of the 17 work vectors of VECTORS, x_opt, and the scalars alpha, beta, omega, r0r_prev, norm, init_norm, min_norm, restarts,
useXopt.  iteration() returns a NEW dict (its input is left alone) with three more entries for whoever compares against it: `totals`
(q.y, y.y, the seven of 14546 and, after a restart, the two of 14578-14581), `restarted` and `done` (the stopping rule 14601).

`given` lets a caller replace what the iteration would total itself by values from elsewhere (a device's own omega, its seven totals, its
restart totals): the vector updates are then judged with exactly the scalars the other side used.
`mutation` selects one deliberately wrong iteration of MUTATIONS (tests/test_bicgstab_restatement.py shows that each is visible)."""
import numpy as np

f64 = np.float64
EPS = f64(1e-100)
VECTORS = ("phat", "rhat", "shat", "what", "zhat", "qhat", "s", "w", "z", "t", "v", "q", "r", "y", "x", "r0", "b")
SCALARS = ("alpha", "beta", "omega", "r0r_prev", "norm", "init_norm", "min_norm", "restarts", "useXopt")
MUTATIONS = ("omega_for_alpha_in_rhat", "shat_from_new_zhat", "z_from_stale_t", "x_with_q", "r0s_against_r", "x_opt_not_snapshotted",
             "w_without_alpha_v", "q_from_old_s")


def dot(a, b, dots="sequential"):
    if dots == "sequential":
        return f64(np.cumsum((a * b).ravel())[-1])
    if dots == "longdouble":
        return f64(np.sum(a.ravel().astype(np.longdouble) * b.ravel().astype(np.longdouble)))
    raise ValueError(dots)


def init(b, x0, A, Minv, dots="sequential", zero_corner=None):
    """14408-14446.  zero_corner: flat index of cell (0,0,0) of the block with index (0,0,0) where bMeanConstraint is 1 or > 2 (14404-14407)."""
    b = np.array(b, dtype=np.float64)
    if zero_corner is not None:
        b.ravel()[zero_corner] = 0.0
    st = {n: np.zeros_like(b) for n in VECTORS}
    st["b"] = b
    r = b.copy()                                     # 14413
    x = np.array(x0, dtype=np.float64)               # 14414
    r0 = r - A(x)                                    # 14417-14420
    r = r0.copy()                                    # 14421
    rhat = Minv(r0)                                  # 14423
    w = A(rhat)
    what = Minv(w)
    t = A(what)                                      # 14426
    temp0, temp1 = dot(r0, r0, dots), dot(r0, w, dots)
    st.update(r=r, x=x, r0=r0, rhat=rhat, w=w, what=what, t=t, x_opt=np.zeros_like(b))
    st.update(alpha=temp0 / (temp1 + EPS), beta=f64(0), omega=f64(0), r0r_prev=temp0, norm=np.sqrt(temp0), init_norm=np.sqrt(temp0),
              min_norm=f64(1e50), restarts=0, useXopt=False, totals={"r0r0": temp0, "r0w": temp1}, restarted=False, done=False)
    return st


def iteration(st, k, A, Minv, dots="sequential", max_restarts=100, tol=0.0, tol_rel=0.0, given=None, mutation=None):
    given = given or {}
    assert mutation is None or mutation in MUTATIONS, mutation
    n = dict(st)  # every vector below is rebound to a new array, never edited in place
    alpha, beta, omega = f64(st["alpha"]), f64(st["beta"]), f64(st["omega"])
    rhat, w, what, t, r, r0, b = st["rhat"], st["w"], st["what"], st["t"], st["r"], st["r0"], st["b"]
    if k % 50 != 0:                                                              # 14454-14464
        phat = rhat + beta * (st["phat"] - omega * st["shat"])
        s = w + beta * (st["s"] - omega * st["z"])
        z = t + beta * (st["z"] - omega * st["v"])
        zhat_used = Minv(z) if mutation == "shat_from_new_zhat" else st["zhat"]
        shat = what + beta * (st["shat"] - omega * zhat_used)
    else:                                                                        # 14466-14472
        phat = rhat + beta * (st["phat"] - omega * st["shat"])
        s = A(phat)
        shat = Minv(s)
        z = A(shat)
    q = r - alpha * (st["s"] if mutation == "q_from_old_s" else s)               # 14459-14461 / 14475-14477
    qhat = rhat - alpha * shat
    y = w - alpha * z
    qy, yy = dot(q, y, dots), dot(y, y, dots)
    zhat = Minv(z)                                                               # 14488
    v = A(zhat)                                                                  # 14489
    omega = f64(given["omega"]) if "omega" in given else qy / (yy + EPS)         # 14493
    x = st["x"] + alpha * phat + omega * (q if mutation == "x_with_q" else qhat)  # 14504 / 14519
    if k % 50 != 0:                                                              # 14505-14507
        r = q - omega * y
        rhat = qhat - omega * (what - (omega if mutation == "omega_for_alpha_in_rhat" else alpha) * zhat)
        w = y - omega * (t if mutation == "w_without_alpha_v" else t - alpha * v)
    else:                                                                        # 14521-14527
        r = b - A(x)
        rhat = Minv(r)
        w = A(rhat)
    seven = (dot(r0, r, dots), dot(r0, w, dots), dot(r if mutation == "r0s_against_r" else r0, s, dots), dot(r0, z, dots),
             dot(r, r, dots), dot(r0, r0, dots), dot(r, r, dots))                # 14508-14514 / 14530-14536
    totals = {"qy": qy, "yy": yy, "seven": seven}
    r0r, r0w, r0s, r0z, norm_1, norm_2, nn = (f64(u) for u in given.get("seven", seven))
    what = Minv(w)                                                               # 14548
    t = st["t"] if mutation == "z_from_stale_t" else A(what)                     # 14549: left stale, the next z is built from the old t
    norm = np.sqrt(nn)
    with np.errstate(all="ignore"):
        beta = alpha / (omega + EPS) * r0r / (f64(st["r0r_prev"]) + EPS)         # 14558
        alpha = r0r / (r0w + beta * r0s - beta * omega * r0z)                    # 14559
        alphat = f64(1.0) / (omega + EPS) + r0w / (r0r + EPS) - beta * omega * r0z / (r0r + EPS)
        alphat = f64(1.0) / (alphat + EPS)
    if np.abs(alphat) < f64(10) * np.abs(alpha):                                 # 14563-14564
        alpha = alphat
    r0r_prev = r0r
    restarts, restarted = st["restarts"], False
    if r0r * r0r < f64(1e-16) * norm_1 * norm_2 and restarts < max_restarts:     # 14566-14593
        restarts += 1
        restarted = True
        r0 = r.copy()
        rhat = Minv(r0)
        w = A(rhat)
        temp = (dot(r0, r0, dots), dot(r0, w, dots))
        totals["restart"] = temp
        temp0, temp1 = (f64(u) for u in given.get("restart", temp))
        what = Minv(w)
        t = A(what)
        alpha = temp0 / (temp1 + EPS)
        r0r_prev = temp0
        beta = f64(0)
        omega = f64(0)
    min_norm, useXopt, x_opt = f64(st["min_norm"]), st["useXopt"], st["x_opt"]
    if norm < min_norm:                                                          # 14594-14600
        useXopt = True
        min_norm = norm
        if mutation != "x_opt_not_snapshotted":
            x_opt = x.copy()
    done = bool(norm < tol or norm / (f64(st["init_norm"]) + EPS) < tol_rel)     # 14601
    n.update(phat=phat, s=s, shat=shat, z=z, q=q, qhat=qhat, y=y, zhat=zhat, v=v, x=x, r=r, rhat=rhat, w=w, what=what, t=t, r0=r0, x_opt=x_opt,
             alpha=alpha, beta=beta, omega=omega, r0r_prev=r0r_prev, norm=norm, min_norm=min_norm, restarts=restarts, useXopt=useXopt,
             totals=totals, restarted=restarted, done=done)
    return n


def solve(b, x0, A, Minv, dots="sequential", zero_corner=None, tol=1e-6, tol_rel=1e-4, max_iter=1000, max_restarts=100, mutation=None):
    """14404-14616: returns (solution, iterations, state); the solution is x_opt where one was recorded (14605)."""
    st = init(b, x0, A, Minv, dots, zero_corner)
    k = 0
    while k < max_iter:
        st = iteration(st, k, A, Minv, dots, max_restarts, tol, tol_rel, mutation=mutation)
        k += 1
        if st["done"]:
            break
    return (st["x_opt"] if st["useXopt"] else st["x"]), k, st
