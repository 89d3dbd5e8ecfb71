"""g2o's Levenberg-Marquardt loop driven through the step-wise C ABI (test infrastructure, not a test file).

optimization_algorithm_levenberg.cpp:61-189 on the host, the way adapters/block_solver_hip.h lets g2o's own OptimizationAlgorithmLevenberg
drive a cs_ba handle: per iteration the estimates are uploaded (cs_ba_set_estimates), computeActiveErrors (cs_ba_compute_errors),
buildSystem (cs_ba_build_system), in the first iteration lambda_0 = 1e-5 * max |H_jj| over the vertices' diagonal blocks
(cs_ba_get_vertex_hessians, :166-180); per trial push / setLambda + solve / update / chi2 and, for a rejected trial, pop.  g2o keeps the
estimates on its side between iterations, so the state makes a host round trip per iteration.
"""
import numpy as np


def max_diagonal(hc, ho, hp):
    """max |H_jj| over the diagonal blocks of every vertex class (an empty class counts as 0)."""
    return max([np.abs(np.einsum("kii->ki", h)).max() for h in (hc, ho, hp) if len(h)] + [0.0])


def run(A, iterations, start, max_trials=10):
    """`iterations` LM iterations on the handle A from the state start = (cams, cuboids, points).
    -> dict(chi2, lam, trials: one entry per iteration done; first_hessians: vertex_hessians() of the first linearisation).
    The final state is A.state()."""
    cams, cubs, pts = (np.asarray(a, float).copy() for a in start)
    lam, ni, n_bad = -1.0, 2.0, 0
    chis, lams, trials = [], [], []
    first = None
    for it in range(iterations):
        A.set_estimates(cams, cubs, pts)                 # adapter: upload_estimates() in buildSystem()
        cur = A.compute_errors()
        ini = tmp = cur
        A.build_system()
        if it == 0:
            first = tuple(h.copy() for h in A.vertex_hessians())
            lam = 1e-5 * max_diagonal(*first)
        rho, q = 0.0, 0
        while True:
            A.push()
            ok, _ = A.solve(lam)
            b, x = A.system_vectors()
            A.update()
            tmp = A.compute_errors()
            if not ok:
                tmp = np.finfo(float).max
            scale = float(np.dot(x, lam * x + b)) + 1e-3
            rho = (cur - tmp) / scale
            if rho > 0 and np.isfinite(tmp):
                lam *= max(1.0 / 3.0, min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0))
                ni = 2.0
                cur = tmp
            else:
                lam *= ni
                ni *= 2
                A.pop()
            q += 1
            if not (rho < 0 and q < max_trials):
                break
        cams, cubs, pts = A.state()                      # g2o keeps the estimates on its side between iterations
        chis.append(cur); lams.append(lam); trials.append(q)
        if q == max_trials or rho == 0:
            break
        n_bad = n_bad + 1 if (ini - cur) * 1e3 < ini else 0
        if n_bad >= 3:
            break
    return dict(chi2=chis, lam=lams, trials=trials, first_hessians=first)
