"""Mode D's sampled call forms, restated from what already exists (nothing new is specified here):

    candidate c of a launch  = oracle sample_candidates() at global index index_offset + c - Philox counter
                               (uint32(index_offset + c), problem, round, draw), key = seed; sigma = (sigma_delta,
                               sigma_pedal); the input box on (delta, pedal); global candidate 0 = the centre, global
                               candidate 1 = u_ref when given, NO candidate 2 (mode D has no LQ plan);
    its cost and violation   = tests/dynamic_spec.py under one vehicle, tests/dynamic_ensemble_spec.py under K;
    its key                  = pack_key(cost, uint32(index_offset + c)); the winner = the smallest key (the first minimum,
                               non-finite costs last); the record = the winner's cost, violation, controls and states.

What acmpc_sample_device writes into a matrix and acmpc_rollout_sampled_device draws inside its kernel are both this."""
import numpy as np

import dynamic_ensemble_spec as es
import dynamic_spec as ds

T = np.float32


def candidates(orc, dp, centre, u_ref, n_candidates, index_offset, problem, round_, seed, sigma):
    """U [N, n, 2] float32: the (delta, pedal) sequences of global candidates index_offset .. index_offset + N - 1 of
    problem number `problem`, round `round_`, drawn round `centre` [n, 2] inside the box of `dp` (make_dynamic_problem)."""
    kw = dp["kw"]
    return orc.sample_candidates(centre, u_ref, n_candidates, index_offset, problem, round_, seed, sigma, kw["u_min"],
                                 kw["u_max"], u_extra=None)


def costs(orc, dp, coef, vehicles, U, reduce=es.MEAN, weights=None, nn_window=None, return_states=False, **kwargs):
    """(cost [N], violation [N][, states [N, n + 1, 3]]) of the candidates U under the vehicle blocks `vehicles` (one block:
    dynamic_spec; several: the ensemble's combine); `kwargs`: rollout_dynamic's settings, u_prev and obstacles."""
    if len(vehicles) == 1:
        return ds.spec_costs(orc, dp, coef, vehicles[0], nn_window=nn_window, U=U, return_states=return_states, **kwargs)
    return es.spec_ensemble(orc, dp, coef, vehicles, reduce=reduce, weights=weights, nn_window=nn_window, U=U,
                            return_states=return_states, **kwargs)


def rollout_sampled(orc, dp, coef, vehicles, centre, u_ref, n_candidates, index_offset, problem, round_, seed, sigma,
                    reduce=es.MEAN, weights=None, nn_window=None, return_states=False, **kwargs):
    """One shard's launch: dict(U, cost, violation, key, n_feasible[, x]) - `key` is the shard's smallest packed key as a
    Python int, over GLOBAL indices.  `kwargs`: rollout_dynamic's settings, u_prev and obstacles."""
    U = candidates(orc, dp, centre, u_ref, n_candidates, index_offset, problem, round_, seed, sigma)
    out = costs(orc, dp, coef, vehicles, U, reduce, weights, nn_window, return_states, **kwargs)
    cost, V = out[0], out[1]
    best = orc.pick_best(cost)[0]
    res = dict(U=U, cost=cost, violation=V, best=best, key=pack_key(cost[best], index_offset + best),
               n_feasible=int(np.count_nonzero(V == 0)))
    if return_states:
        res["x"] = out[2]
    return res


def pack_key(cost, index):
    """acmpc_pack_key: (ordered int32 of the cost, non-finite -> +inf) << 32 | uint32(index), as a signed 64-bit value."""
    bits = int(np.asarray(cost, dtype=T).view(np.uint32))
    if (bits & 0x7f800000) == 0x7f800000:
        bits = 0x7f800000
    hi = bits if bits < 0x80000000 else (bits - (1 << 32)) ^ 0x7fffffff
    return (hi << 32) | (int(index) & 0xffffffff)
