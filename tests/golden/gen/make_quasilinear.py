"""Writes tests/golden/quasilinear_twin.npz: for each equation kind of Quasilinear2d the final iterate of the LONG-DOUBLE twin of the
float64 numpy pipeline (tests/_quasilinear_reference.py) on the class test's configuration -- N_d = 150, N_b = 40 points of
_quasilinear_reference.points, Gaussian kernel sigma = 0.3, adaptive nugget 1e-8, 8 Gauss-Newton steps from zero, the manufactured
solutions of main_Quasilinear2d.py.  Everything is long double here: Theta, its Cholesky factor, F, A, the solves, the normal equations
(H solved in float64 and refined in long double).  Minutes on a CPU, which is why the result is a fixture; tests/test_gpu_quasilinear.py
compares the device's and the float64 pipeline's iterates with it.
    python tests/golden/gen/make_quasilinear.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'nonlinpdes-gpsolver_amd')]

import _gn_reference as R                       # noqa: E402
import _quasilinear_reference as Q              # noqa: E402

LD = Q.LD
ND, NB, SIGMA, NUGGET, STEPS, AMPLITUDE = 150, 40, 0.3, 1e-8, 8, 0.5


def cholesky_ld(T):
    n = T.shape[0]
    L = np.zeros_like(T)
    for j in range(n):
        d = T[j, j] - L[j, :j] @ L[j, :j]
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (T[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_lower_ld(L, B):
    X = np.array(B, dtype=LD)
    for i in range(L.shape[0]):
        if i:
            X[i] -= L[i, :i] @ X[:i]
        X[i] /= L[i, i]
    return X


def twin(kind, prm, L, f, g, steps):
    Nd = f.size
    prm = tuple(LD(v) for v in prm)
    f, g = f.astype(LD), g.astype(LD)
    z = np.zeros(5 * Nd, dtype=LD)
    i = np.arange(Nd)
    for _ in range(steps):
        v = Q.split(z, Nd)
        A = np.zeros((6 * Nd + g.size, 5 * Nd), dtype=LD)
        for k in range(4):
            A[k * Nd + i, (k + 1) * Nd + i] = 1
        for k, d in enumerate(Q.dG(kind, prm, f, *v)):
            A[4 * Nd + i, k * Nd + i] = d
        A[5 * Nd + i, i] = 1
        Fv = np.concatenate([v[1], v[2], v[3], v[4], Q.G(kind, prm, f, *v), v[0], g])
        Sb = solve_lower_ld(L, np.concatenate([A, Fv[:, None]], axis=1))
        S, w = Sb[:, :-1], Sb[:, -1]
        H, gr = S.T @ S, S.T @ w
        delta = R.refine(lambda r: np.linalg.solve(H.astype(np.float64), r), lambda d: gr - H @ d, gr.astype(np.float64))
        z = z - delta
    return z


def main():
    import main_Quasilinear2d as drv
    from src.quasilinear import QuasilinearEquation
    Xd, Xb = Q.points(ND, NB)
    T = Q.theta_nugget('Gaussian', SIGMA, Xd, Xb, NUGGET)
    L = cholesky_ld(T)
    out = {}
    for kind in Q.KINDS:
        eq = QuasilinearEquation.make((kind,) + tuple(Q.PRM[kind][:2 if kind == 'p_laplace' else 1]))
        u, f = drv.manufactured(eq, AMPLITUDE)
        z = twin(kind, eq.params, L, f(*Xd.T), u(*Xb.T), STEPS)
        out[kind] = z.astype(np.float64)
        print(kind, 'L2 error of the twin', float(np.sqrt(np.mean((out[kind][:ND] - u(*Xd.T)) ** 2))), flush=True)
    np.savez_compressed(os.path.join(ROOT, 'tests', 'golden', 'quasilinear_twin.npz'), **out)


if __name__ == '__main__':
    main()
