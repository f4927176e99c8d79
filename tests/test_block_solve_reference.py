"""The exact block solve of tests/block_solve_exact.py and the bounds it derives, checked on the CPU (no GPU): the helper against a dense
solve of the assembled 512 x 512 operator, and the reference's block CG (the oracle's orc_precond_block_coef, pinned to the compiled
reference by test_oracle_vs_ref.py) inside those bounds on the whole edge catalogue.  test_gpu_block_preconditioner.py holds the device's
block solvers to the same bounds."""
import numpy as np
import pytest

import block_solve_exact as X
import oracle_lib as O

# Poisson and two Helmholtz shifts h^2 / (nu dt)
CENTRES = [-6.0, -6.0 - 0.01, -6.0 - 100.0]


@pytest.mark.parametrize("centre", CENTRES)
def test_exact_solve_against_a_dense_solve(centre):
    """Random blocks and all 512 unit impulses: the sine-transform solve equals np.linalg.solve of the Kronecker-sum matrix to double
    rounding, and its residual, evaluated in long double, is <= 1e-15 relative (before and after rounding z to double)."""
    rng = np.random.default_rng(11)
    h = 0.125
    rhs = np.concatenate([rng.uniform(-1, 1, (24, 8, 8, 8)), np.eye(512).reshape(512, 8, 8, 8)])
    A = X.dense_block_operator(centre)
    zd = np.linalg.solve(A, (rhs.reshape(len(rhs), -1) / h).T).T.reshape(rhs.shape)
    z = X.exact_block_solve(rhs, h, centre)
    assert z.dtype == np.float64
    d = np.abs(z - zd).reshape(len(z), -1).max(axis=1) / np.abs(zd).reshape(len(z), -1).max(axis=1)
    assert d.max() <= 1e-14, d.max()            # np.linalg.solve's own error: ~ kappa * eps
    for zz in (X.exact_block_solve_ld(rhs, h, centre), z):
        rn, bn = X.block_residual(zz, rhs, h, centre)
        assert (rn / bn).max() <= 1e-15, (rn / bn).max()
    # the inverse is symmetric (the operator is)
    G = X.exact_block_solve(np.eye(512).reshape(512, 8, 8, 8), 1.0, centre).reshape(512, 512)
    assert np.abs(G - G.T).max() <= 1e-15 * np.abs(G).max()


def test_exact_solve_of_eigenmodes_and_operator_norms():
    """An eigenvector Q_kz x Q_ky x Q_kx is returned divided by h (lam_kz + lam_ky + lam_kx + c + 6); kappa = 32.16 for Poisson."""
    for c in CENTRES:
        for k in [(0, 0, 0), (7, 7, 7), (3, 1, 5), (0, 7, 2)]:
            m = X.eigenmode(*k)
            lam = float(X.LAM[k[0]] + X.LAM[k[1]] + X.LAM[k[2]]) + c + 6
            z = X.exact_block_solve(m[None], 0.5, c)[0]
            assert np.abs(z - m / (0.5 * lam)).max() <= 1e-15 * np.abs(m / (0.5 * lam)).max()
    nrm, inv = X.operator_norms(-6.0)
    assert abs(nrm * inv - 32.16) < 0.01
    nrm2, inv2 = X.operator_norms(-6.0 - 1.0)
    assert nrm2 * inv2 < nrm * inv
    # the matrix agrees with the helper's operator
    rng = np.random.default_rng(2)
    v = rng.uniform(-1, 1, (3, 8, 8, 8))
    for c in CENTRES:
        dense = (X.dense_block_operator(c) @ v.reshape(3, -1).T).T.reshape(v.shape)
        assert np.abs(X.apply_block_operator(v, c).astype(np.float64) - dense).max() <= 1e-15 * np.abs(dense).max()


@pytest.mark.parametrize("centre", CENTRES + [-7.0])
def test_reference_block_cg_meets_the_stopping_rule_bounds(centre):
    """The reference's block CG on 900 blocks of the edge catalogue, uniform h and per-block h: true residual and error inside
    cg_bounds(), skipped blocks exact zeros, no NaN.  Records its iteration counts per kind (the device's are held to these +-1 in
    test_gpu_block_preconditioner.py)."""
    rng = np.random.default_rng(17)
    kinds, blocks = X.edge_grid(rng, 900, 1.0)
    for h in (0.1, rng.choice([0.2, 0.1, 0.05], len(blocks))):
        hb = np.broadcast_to(h, len(blocks))
        c = centre if centre == -6.0 else -6.0 - (hb / 0.1) ** 2 * (-6.0 - centre)   # Helmholtz: the shift follows h^2
        rhs = np.ascontiguousarray([b * hh for b, hh in zip(blocks, hb)])          # thresholds of the catalogue are per unit h
        z, its = O.precond_blocks(rhs, hb, c)
        assert np.isfinite(z).all()
        sk = X.skipped(rhs, hb)
        assert np.array_equal(sk, np.isin(kinds, ["zero", "below_skip"]))
        assert (z[sk] == 0).all() and (its[sk] == 0).all()
        rb, eb, bn = X.cg_bounds(rhs, hb, c)
        rn, _ = X.block_residual(z, rhs, hb, c)
        err = np.linalg.norm((z - X.exact_block_solve(rhs, hb, c)).reshape(len(z), -1), axis=1)
        print(f"centre {centre}: residual / bound max {(rn / rb)[~sk].max():.4f}, error / bound max {(err / eb)[~sk].max():.4f}; "
              "iterations " + ", ".join(f"{k} {its[kinds == k].min()}-{its[kinds == k].max()}" for k in X.EDGE_KINDS))
        assert (rn[~sk] <= rb[~sk]).all(), (rn / rb)[~sk].max()
        assert (err[~sk] <= eb[~sk]).all(), (err / eb)[~sk].max()
        # one CG iteration solves an eigenvector; every other solved block takes more than one and far fewer than the cap of 100
        assert (its[np.isin(kinds, ["lowest_mode", "highest_mode", "above_skip"])] == 1).all()
        assert (its[np.isin(kinds, ["random", "constant", "spike"])] >= 2).all() and its.max() < 60
        if centre == -6.0:
            assert (its[kinds == "random"] >= 20).all() and (its[kinds == "random"] <= 35).all()


def test_reference_block_cg_at_falling_scales():
    """The same block scaled down: the relative criterion ends the CG until the absolute one (||r||^2 / 512^2 < 1e-32) takes over,
    the counts fall, and below 1e-32 on entry the block is exactly 0."""
    rng = np.random.default_rng(5)
    b = rng.uniform(-1, 1, (1, 8, 8, 8))
    counts = []
    for s in (1.0, 1e-12, 1e-13, 1e-14, 1e-15):
        z, its = O.precond_blocks(b * s, 1.0)
        counts.append(int(its[0]))
        rb, eb, _ = X.cg_bounds(b * s, 1.0)
        rn, _ = X.block_residual(z, b * s, 1.0)
        if s >= 1e-14:
            assert rn[0] <= rb[0]
        else:
            assert (z == 0).all() and its[0] == 0
    print("iterations at scales 1, 1e-12 ... 1e-15:", counts)
    assert counts == sorted(counts, reverse=True) and counts[0] >= 20 and counts[-1] == 0 and counts[-2] >= 1
