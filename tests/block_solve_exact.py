"""The block preconditioner's operator solved exactly, in extended precision (test helper, no GPU).

M^-1 (getZImplParallel, main.cpp:14704-14745; the Helmholtz form 10534-10579) solves, on ONE 8^3 block with zero ghosts,
    sum6(z) + c z = r / h,      c = -6 (Poisson) or -6 - h^2 / (nu dt) (Helmholtz).
The 1-D Dirichlet operator tridiag(1, -2, 1) has the sine eigenvectors Q[k][j] = sqrt(2/9) sin(pi (j+1)(k+1) / 9) (Q = Q^T = Q^-1) and
eigenvalues lam_k = 2 cos(pi (k+1) / 9) - 2, so
    z = (Q x Q x Q) diag(1 / (lam_i + lam_j + lam_k + c + 6)) (Q x Q x Q) (r / h).
Here Q and lam are evaluated in np.longdouble from a longdouble pi, and so is the whole transform: the result is the exact solve to
well below double rounding.  The reference's block CG stops at ||r_k||^2 / 512^2 < max(1e-14 ||r_0||^2 / 512^2, 1e-32) and leaves a block
at 0 when ||r_0||^2 / 512^2 < 1e-32; cg_bounds() turns that rule into bounds on the true residual and on the error of any block CG.
"""
import numpy as np

LD = np.longdouble
PI = 4 * np.arctan(LD(1))
_K = np.arange(1, 9, dtype=LD)
Q = np.sqrt(LD(2) / LD(9)) * np.sin(PI * np.outer(_K, _K) / LD(9))   # [k][j], symmetric and orthogonal
LAM = 2 * np.cos(PI * _K / LD(9)) - 2                                 # 1-D eigenvalues, -0.12 ... -3.88
LAM3 = LAM[:, None, None] + LAM[None, :, None] + LAM[None, None, :]    # eigenvalues of sum6 - 6 on the block, [kz][ky][kx]

BLOCK_REL, BLOCK_ABS = 1e-7, 1e-16   # kSqrNorm{Rel,Abs}Criterion (main.cpp:14619-14624), as norms
SKIP_BELOW = 1e-32                   # ||r_0||^2 / 512^2 below this: the block stays 0 (14735-14736)


def _per_block(v, n):
    return np.broadcast_to(np.asarray(v, dtype=LD), (n,)).reshape(n, 1, 1, 1)


def _transform(v):
    """(Q x Q x Q) v over the three cell axes of v[n, 8, 8, 8]."""
    v = np.einsum("kj,nzyj->nzyk", Q, v)
    v = np.einsum("kj,nzjx->nzkx", Q, v)
    return np.einsum("kj,njyx->nkyx", Q, v)


def exact_block_solve_ld(rhs_blocks, h, centre=-6.0):
    """exact_block_solve in np.longdouble (not rounded to double)."""
    r = np.asarray(rhs_blocks, dtype=LD)
    n = len(r)
    b = r / _per_block(h, n)
    return _transform(_transform(b) / (LAM3[None] + _per_block(centre, n) + 6))


def exact_block_solve(rhs_blocks, h, centre=-6.0):
    """z = M^-1 r block by block, exactly: rhs_blocks [n, 8, 8, 8] (z, y, x), h and centre scalars or one per block; float64 out."""
    return exact_block_solve_ld(rhs_blocks, h, centre).astype(np.float64)


def apply_block_operator(z, centre=-6.0):
    """sum6(z) + c z on each block with zero ghosts, in np.longdouble."""
    z = np.asarray(z, dtype=LD)
    p = np.zeros((len(z), 10, 10, 10), dtype=LD)
    p[:, 1:9, 1:9, 1:9] = z
    s = (p[:, :-2, 1:-1, 1:-1] + p[:, 2:, 1:-1, 1:-1] + p[:, 1:-1, :-2, 1:-1] + p[:, 1:-1, 2:, 1:-1] + p[:, 1:-1, 1:-1, :-2]
         + p[:, 1:-1, 1:-1, 2:])
    return s + _per_block(centre, len(z)) * z


def block_residual(z, rhs, h, centre=-6.0):
    """Per block ||A z - r/h||_2 and ||r/h||_2, accumulated in np.longdouble (returned as float64)."""
    n = len(z)
    b = np.asarray(rhs, dtype=LD) / _per_block(h, n)
    res = apply_block_operator(z, centre) - b
    rn = np.sqrt((res.reshape(n, -1) ** 2).sum(axis=1))
    bn = np.sqrt((b.reshape(n, -1) ** 2).sum(axis=1))
    return rn.astype(np.float64), bn.astype(np.float64)


def operator_norms(centre=-6.0):
    """(||A||_2, ||A^-1||_2) of the block operator with centre coefficient c (scalar or per block): A is symmetric negative definite
    for c <= -6, its eigenvalues lam_i + lam_j + lam_k + c + 6.  Condition number 32.16 for Poisson, smaller with a Helmholtz shift."""
    c = np.asarray(centre, dtype=LD) + 6
    lo, hi = np.abs(LAM3.max() + c), np.abs(LAM3.min() + c)
    return hi.astype(np.float64), (1 / lo).astype(np.float64)


def skipped(rhs, h):
    """Blocks the reference leaves at 0: ||r/h||^2 / 512^2 < 1e-32."""
    n = len(rhs)
    b = np.asarray(rhs, dtype=LD) / _per_block(h, n)
    return ((b.reshape(n, -1) ** 2).sum(axis=1) / 512 ** 2 < SKIP_BELOW)


def cg_bounds(rhs, h, centre=-6.0):
    """What the reference's stopping rule guarantees for ANY block CG that obeys it, per block:
        residual  ||A z - r/h||_2 <= 1.0001 max(1e-7 ||r/h||_2, 512 * 1e-16)   (the rule on ||r_k||^2 / 512^2; 1e-4 relative slack for the
                  recursive residual's drift from the true one);
        error     ||z - z_exact||_2 <= ||A^-1||_2 * residual bound, i.e. kappa 1.0001e-7 ||z_exact||_2 while the relative criterion
                  ends the CG (||r/h|| <= ||A|| ||z_exact||) -- no fitted tolerance.
    Returns (residual bound, error bound, ||r/h||_2)."""
    n = len(rhs)
    b = np.asarray(rhs, dtype=LD) / _per_block(h, n)
    bn = np.sqrt((b.reshape(n, -1) ** 2).sum(axis=1)).astype(np.float64)
    res = 1.0001 * np.maximum(BLOCK_REL * bn, 512 * BLOCK_ABS)
    _, inv = operator_norms(centre)
    return res, inv * res, bn


def eigenmode(kz, ky, kx):
    """The block eigenvector Q[kz] x Q[ky] x Q[kx] (float64); M^-1 of it is itself / (h (lam_kz + lam_ky + lam_kx + c + 6))."""
    return np.einsum("z,y,x->zyx", Q[kz], Q[ky], Q[kx]).astype(np.float64)


def _scaled_to(v, h, sqr_norm0):
    """v scaled so that ||v/h||^2 / 512^2 = sqr_norm0."""
    return v * (512 * h * np.sqrt(sqr_norm0) / np.linalg.norm(v))


EDGE_KINDS = ("zero", "below_skip", "above_skip", "absolute", "random", "lowest_mode", "highest_mode", "constant", "spike")


def edge_blocks(rng, h=1.0, kinds=EDGE_KINDS):
    """One block of each kind (list of (kind, block [8, 8, 8])), where block CGs go wrong:
        zero          -> exact 0;
        below_skip    ||r/h||^2/512^2 = 1/4 of 1e-32 -> left at exact 0;  above_skip: 4 x 1e-32 -> solved, the absolute criterion ends it;
        absolute      ||r/h||^2/512^2 ~ 1e-29: the absolute criterion (1e-32) ends the CG after a few iterations;
        random        uniform in [-1, 1], amplitude 10^U(-2, 2);
        lowest_mode / highest_mode  an eigenvector of the block operator: one CG iteration is exact;
        constant      one value in every cell (the slowest-converging smooth content);
        spike         1e6 at one cell on 1e-6 noise: 12 decades inside one block."""
    out = []
    for k in kinds:
        if k == "zero":
            b = np.zeros((8, 8, 8))
        elif k == "below_skip":
            b = _scaled_to(rng.uniform(-1, 1, (8, 8, 8)), h, 0.25e-32)
        elif k == "above_skip":
            b = _scaled_to(rng.uniform(-1, 1, (8, 8, 8)), h, 4e-32)
        elif k == "absolute":
            b = _scaled_to(rng.uniform(-1, 1, (8, 8, 8)), h, 1e-29 * rng.uniform(0.5, 2))
        elif k == "random":
            b = rng.uniform(-1, 1, (8, 8, 8)) * 10 ** rng.uniform(-2, 2)
        elif k == "lowest_mode":
            b = eigenmode(0, 0, 0) * rng.uniform(0.5, 2)
        elif k == "highest_mode":
            b = eigenmode(7, 7, 7) * rng.uniform(0.5, 2)
        elif k == "constant":
            b = np.full((8, 8, 8), rng.uniform(-3, 3))
        elif k == "spike":
            b = 1e-6 * rng.uniform(-1, 1, (8, 8, 8))
            b[tuple(rng.integers(0, 8, 3))] = 1e6
        else:
            raise ValueError(k)
        out.append((k, b))
    return out


def edge_grid(rng, nblocks, h=1.0):
    """nblocks blocks cycling through the edge catalogue (neighbouring blocks converge at very different speeds): (kinds, blocks)."""
    kinds, blocks = [], []
    while len(blocks) < nblocks:
        for k, b in edge_blocks(rng, h):
            if len(blocks) < nblocks:
                kinds.append(k)
                blocks.append(b)
    return np.array(kinds), np.ascontiguousarray(blocks)


def dense_block_operator(centre=-6.0):
    """The 512 x 512 Kronecker sum T x I x I + I x T x I + I x I x T + (c + 6) I (cells in (z, y, x) order, float64)."""
    T = np.diag(np.full(8, -2.0)) + np.diag(np.ones(7), 1) + np.diag(np.ones(7), -1)
    I = np.eye(8)
    return np.kron(np.kron(T, I), I) + np.kron(np.kron(I, T), I) + np.kron(np.kron(I, I), T) + (centre + 6) * np.eye(512)
