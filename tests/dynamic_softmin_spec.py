"""Mode D's softmin (MPPI) rounds, restated from what already exists (nothing new is specified here):

    round r's candidates   = tests/dynamic_sampled_spec.py candidates() round that round's centre with the spread
                             sigma shrink^r (the product in float64, as acmpc_optimize forms it), global indices 0 .. N - 1;
    round 0                  samples round the caller's centre, the caller's u_ref (or none) as candidate 1;
    after every round but    the softmin mean of ITS candidates (oracle softmin_mean: weights exp(-(cost - min) / lambda)
    the last                 in float32, the sums in float64, one rounding to float32; the plain mean when no cost is
                             finite) is the next round's centre - its candidate 0 - and the round's winner its candidate 1;
    the record             = the LAST round's argmin winner.  No mean is taken after the last round.

The previous winner is always a candidate, so the winner's cost never rises from round to round."""
import numpy as np

import dynamic_ensemble_spec as es
import dynamic_sampled_spec as dss

T = np.float32


def softmin_mean(orc, cost, U, lam):
    """[n, 2] float32: oracle softmin_mean of the candidates U [N, n, 2], uniform weights when no cost is finite."""
    if not np.isfinite(cost).any():
        return U.astype(np.float64).mean(axis=0).astype(T)
    return orc.softmin_mean(cost, U, lam).astype(T)


def round_sigmas(sigma, shrink, rounds):
    """The spread of every round as acmpc_optimize forms it: sigma * scale in float64, scale *= shrink per round."""
    out, scale = [], 1.0
    for _ in range(rounds):
        out.append((float(sigma[0]) * scale, float(sigma[1]) * scale))
        scale *= float(shrink)
    return out


def solve(orc, dp, coef, vehicles, centre, u_ref, n_candidates, rounds, sigma, shrink, seed, lam, problem=0,
          reduce=es.MEAN, weights=None, nn_window=None, **kwargs):
    """One softmin solve of problem number `problem`: a list with one dict per round - centre, u_ref (candidate 1, or
    None), sigma, U [N, n, 2], cost, violation, best (the argmin) and mean (None after the last round).  `kwargs`:
    rollout_dynamic's settings, u_prev and obstacles."""
    out = []
    c, ref = np.asarray(centre, dtype=T), None if u_ref is None else np.asarray(u_ref, dtype=T)
    for r, sig in enumerate(round_sigmas(sigma, shrink, rounds)):
        U = dss.candidates(orc, dp, c, ref, n_candidates, 0, problem, r, seed, sig)
        cost, V = dss.costs(orc, dp, coef, vehicles, U, reduce, weights, nn_window, **kwargs)[:2]
        best = orc.pick_best(cost)[0]
        mean = softmin_mean(orc, cost, U, lam) if r + 1 < rounds else None
        out.append(dict(centre=c, u_ref=ref, sigma=sig, U=U, cost=cost, violation=V, best=best, mean=mean))
        if mean is not None:
            c, ref = mean, U[best].copy()
    return out
