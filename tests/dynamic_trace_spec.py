"""Mode D's plan trace restated in NumPy ("Mode D, plan trace"): the rollout of
tests/dynamic_obstacles_spec.py - its lines, the step through dynamic_spec.dynamic_step, the rate and slip lines through
dynamic_terms_spec.step_terms, the discs through dynamic_obstacles_spec.step_obstacles - keeping what every control step saw:
the six states and the 22 floats of a `terms` row (include/acmpc.h, acmpc_trace_plans).  Bit-identical to
trace_dynamic_kernel (csrc/acmpc_dynamic_trace.hip).  A helper of the tests, not a test file.

Cost, V and (X, Y, yaw) come out of the very lines the composed restatements of the scoring kernels run, so they are theirs by
construction.  The hinges of slots 5 .. 19 are RESTATED beside those lines (as the kernel restates them beside the shared cost
functions); `replay()` squares them back into V, which is what holds the restatements to the lines that score.

`tracing()` swaps dynamic_obstacles_spec.rollout_dynamic - where every restatement composed under
dynamic_obstacles_spec.setting() ends - for the duration of a `with` block; `restatement()` composes every setting of a handle
under it, the downforce's block (dynamic_aero_spec.setting: the load transfer's and the coupling's with aero = None) in the load
transfer's place."""
from __future__ import annotations

import contextlib
from types import SimpleNamespace

import numpy as np

import dynamic_aero_spec as das
import dynamic_integration_spec as dis
import dynamic_objective_spec as dos
import dynamic_obstacles_spec as dobs
import dynamic_spec as ds
import dynamic_terms_spec as dts
from acmpc_oracle import fma32, wrap_spec

T = np.float32
TERM_FLOATS = 22
J, EY, EPSI, DV, DK, BOX, CORRIDOR, RATE, SLIP, CEILING, DISCS, V_SLOT, E_SLOT = 0, 1, 2, 3, 4, 5, 7, 8, 10, 11, 12, 20, 21
HINGES = slice(5, 20)
MAX_OBSTACLES = 8


def rollout_trace(obstacles, objective, terms, u_prev, x0, wp, U, vehicle, Q, R, QN, u_lo, u_hi, w_bound, dt, wheelbase,
                  nn_window=None, return_states=False):
    """dynamic_obstacles_spec.rollout_dynamic - the same lines - that also returns dict(states [N, n + 1, 6], terms
    [N, n, 22]): ((cost, V[, X_out]), traced)."""
    pos, radii, weight, margin = obstacles
    K = 0 if pos is None else int(np.asarray(pos).shape[1])
    ob = dobs.constants(weight, margin)
    soft = ob.soft and K > 0
    if K > 0:
        pos = np.asarray(pos, dtype=T)
        radii = np.asarray(radii, dtype=T)
    o = dos.constants(*objective)
    c = dts.constants(dt, *terms)
    k = ds.derived_constants(vehicle)
    U = np.asarray(U, dtype=T)
    wp = np.asarray(wp, dtype=T)
    N, n, _ = U.shape
    Q, R, QN = (np.asarray(a, dtype=T) for a in (Q, R, QN))
    lo, hi = np.asarray(u_lo, dtype=T), np.asarray(u_hi, dtype=T)
    half, zero, wb, dtT = T(0.5), T(0.0), T(w_bound), T(dt)
    hQ, hR, hQN = half * Q, half * R, half * QN
    ox, oy = wp[0, 0], wp[0, 1]
    wx, wy = wp[:, 0] - ox, wp[:, 1] - oy
    key_a, key_b = T(-2.0) * wx, T(-2.0) * wy
    key_c = fma32(wy, wy, wx * wx)
    row_k = fma32(wp[:, 3], wx, -(wp[:, 2] * wy))
    row_ns = -wp[:, 3]
    delta_ref = ds.atan_spec(T(wheelbase) * wp[:, 5])
    q = dos.progress_table(wp)
    x0 = np.asarray(x0, dtype=T)
    st = [np.full(N, x0[0] - ox, dtype=T), np.full(N, x0[1] - oy, dtype=T)] + [np.full(N, x0[m], dtype=T) for m in range(2, 6)]
    S0, S1, S2, S3, V, E = (np.zeros(N, dtype=T) for _ in range(6))
    ey = np.zeros(N, dtype=T)
    ep = np.zeros(N, dtype=T)
    j_prev = np.zeros(N, dtype=np.int64)
    rows = np.arange(N)
    pd = pp = None
    if c.rate and u_prev is not None:
        prev = np.asarray(u_prev, dtype=T)
        pd, pp = np.full(N, prev[0], dtype=T), np.full(N, prev[1], dtype=T)
    X_out = np.zeros((N, n + 1, 3), dtype=T)
    X_out[:, 0] = np.stack([st[0] + ox, st[1] + oy, st[2]], axis=1)
    states = np.zeros((N, n + 1, 6), dtype=T)
    out = np.zeros((N, n, TERM_FLOATS), dtype=T)
    states[:, 0] = np.stack([st[0] + ox, st[1] + oy] + st[2:], axis=1)
    for i in range(n):
        d, p = U[:, i, 0], U[:, i, 1]
        st = list(ds.dynamic_step(st, d, p, k, dtT))
        X, Y, psi, vx = st[0], st[1], st[2], st[3]
        if nn_window is None:
            w = np.broadcast_to(np.arange(n), (N, n))
        else:
            back, ahead = nn_window
            width = back + ahead + 1
            lo_w = np.maximum(np.minimum(j_prev - back, n - width), 0)
            hi_w = np.minimum(lo_w + width, n) - 1
            w = np.minimum(lo_w[:, None] + np.arange(width)[None, :], hi_w[:, None])
        best = np.full(N, np.inf, dtype=T)
        j = w[:, 0].copy()
        for b in range(0, w.shape[1], ds.SCAN_BLOCK):
            block = w[:, b:b + ds.SCAN_BLOCK]
            dd = fma32(Y[:, None], key_b[block], fma32(X[:, None], key_a[block], key_c[block]))
            first = np.argmin(np.where(np.isnan(dd), T(np.inf), dd), axis=1)
            dd = dd[rows, first]
            better = dd < best
            best = np.where(better, dd, best)
            j = np.where(better, block[rows, first], j)
        j_prev = j
        g = wp[j]
        row = out[:, i]
        with np.errstate(all="ignore"):
            ey = fma32(g[:, 2], Y, fma32(row_ns[j], X, row_k[j]))
            ep = wrap_spec(psi - g[:, 4], T)
            dv = vx - g[:, 6]
            dk = d - delta_ref[j]
            S0 = fma32(ey, ey, S0)
            S1 = fma32(ep, ep, S1)
            S2 = fma32(dv, dv, S2)
            S3 = fma32(dk, dk, S3)
            hd = d - np.fmin(np.fmax(d, lo[0]), hi[0])
            V = fma32(hd, hd, V)
            hp = p - np.fmin(np.fmax(p, lo[1]), hi[1])
            V = fma32(hp, hp, V)
            hc = np.fmax(np.abs(ey) - g[:, 7], zero)
            V = fma32(hc, hc, V)
        row[:, J], row[:, EY], row[:, EPSI], row[:, DV], row[:, DK] = j.astype(T), ey, ep, dv, dk
        row[:, BOX], row[:, BOX + 1], row[:, CORRIDOR] = hd, hp, hc
        if i == 0 and pd is None:
            pd, pp = d, p
        # the hinges dynamic_terms_spec.step_terms is about to square, restated
        with np.errstate(all="ignore"):
            if c.rate:
                row[:, RATE] = np.fmax(np.abs((d - pd) * c.inv_dt) - c.rd_max, zero)
                row[:, RATE + 1] = np.fmax(np.abs((p - pp) * c.inv_dt) - c.rp_max, zero)
            if c.slip:
                row[:, SLIP] = np.fmax(np.abs((st[5] * k["lr"] - st[4]) / (vx + T(ds.VX_EPS))) - c.b_max, zero)
        E, V = dts.step_terms(c, k, st, d, p, pd, pp, E, V)
        pd, pp = d, p
        if o.ceiling:
            with np.errstate(all="ignore"):
                cap = fma32(o.cs, g[:, 6], o.co)
                h = np.fmax(np.asarray(vx - cap, dtype=T), zero)
                V = np.asarray(fma32(h, h, V), dtype=T)
            row[:, CEILING] = h
        if K > 0:
            with np.errstate(all="ignore"):
                for m in range(K):   # dynamic_obstacles_spec.step_obstacles' depth, restated
                    dx, dy = X - T(pos[i, m, 0] - ox), Y - T(pos[i, m, 1] - oy)
                    row[:, DISCS + m] = np.fmax(radii[m] - np.sqrt(np.asarray(fma32(dy, dy, dx * dx), dtype=T)), zero)
            E, V = dobs.step_obstacles(ob, soft, pos[i], radii, ox, oy, X, Y, E, V)
        row[:, V_SLOT], row[:, E_SLOT] = V, E
        X_out[:, i + 1] = np.stack([X + ox, Y + oy, psi], axis=1)
        states[:, i + 1] = np.stack([X + ox, Y + oy] + st[2:], axis=1)
    with np.errstate(all="ignore"):
        tN = T(n) * dtT
        Jc = hQ[0] * S0
        Jc = fma32(hQ[1], S1, Jc)
        Jc = fma32(hR[0], S2, Jc)
        Jc = fma32(hR[1], S3, Jc)
        if c.rate or c.slip or soft:
            Jc = Jc + E
        s = (hQN[0] * ey) * ey
        s = fma32(hQN[1] * ep, ep, s)
        s = fma32(hQN[2] * tN, tN, s)
        Jc = Jc + s
        if o.progress:
            g = wp[j_prev]
            prog = np.asarray(fma32(g[:, 3], st[1], fma32(g[:, 2], st[0], q[j_prev])), dtype=T)
            Jc = fma32(o.nwp, prog, Jc)
        cost = fma32(wb, V, Jc)
    cost = np.asarray(cost, dtype=T)
    V = np.asarray(V, dtype=T)
    traced = dict(states=states, terms=out, totals=np.stack([cost, V], axis=1))
    return ((cost, V, X_out) if return_states else (cost, V)), traced


@contextlib.contextmanager
def tracing():
    """Inside the block every restatement that ends in dynamic_obstacles_spec.rollout_dynamic leaves its trace in the
    handle's `out`: dict(states, terms, totals) of the last rollout."""
    handle = SimpleNamespace(out=None)
    saved = dobs.rollout_dynamic

    def traced(obstacles, objective, terms, u_prev, *args, **kwargs):
        kwargs.pop("trace", None)
        result, handle.out = rollout_trace(obstacles, objective, terms, u_prev, *args, **kwargs)
        return result

    dobs.rollout_dynamic = traced
    try:
        yield handle
    finally:
        dobs.rollout_dynamic = saved


NO_TERMS = dict(rate_weight=(0.0, 0.0), rate_max=None, slip_weight=0.0, slip_max=None)
NO_OBJECTIVE = dict(progress_weight=0.0, speed_ceiling=None)


def settings(**over):
    """A handle's mode D settings as one dict; the defaults are a handle nothing was set on."""
    s = dict(M=1, blend=None, terms=dict(NO_TERMS), objective=dict(NO_OBJECTIVE), ratio=None, load=None, aero=None,
             clearance=(0.0, 0.0))
    s.update(over)
    return s


def from_case(c):
    """The settings of a dynamic_fuzz_cases case."""
    return settings(M=c["M"], blend=c["blend"], terms=c["terms"], objective=c["objective"], ratio=c["ratio"], load=c["load"])


@contextlib.contextmanager
def restatement(s, u_prev=None, obstacles=None):
    """Every setting of `s` composed under tracing(), with ONE problem's previous control and obstacles = (positions
    [n, K, 2], radii [K]) or None."""
    pos, radii = (None, None) if obstacles is None else obstacles
    with tracing() as handle:
        with dobs.setting(pos, radii, *s["clearance"]):
            with das.setting(s["ratio"], s["load"], s["aero"]):
                with dos.setting(**s["objective"]):
                    with dts.setting(u_prev=u_prev, **s["terms"]):
                        with dis.setting(s["M"], s["blend"]):
                            yield handle


def trace_plans(dp, coef, U, vehicles, s, nn_window=None, u_prev=None, obstacles=None):
    """What Engine.trace_plans must give for ONE problem `dp` (dynamic_spec.make_dynamic_problem) on the packed rows `coef`
    [n, 8]: dict(states [M, K, n + 1, 6], totals [M, K, 2], terms [M, K, n, 22]) for the plans U [M, n, 2] under the vehicle
    blocks `vehicles`."""
    kw = dp["kw"]
    per = []
    for block in vehicles:
        with restatement(s, u_prev, obstacles) as handle:
            ds.rollout_dynamic(dp["x0"], coef, U, block, kw["step_cost"], kw["r_term"], kw["final_cost"], kw["u_min"],
                               kw["u_max"], kw["w_bound"], kw["dt"], kw["wheelbase"], nn_window=nn_window)
            per.append(handle.out)
    return {name: np.stack([t[name] for t in per], axis=1) for name in ("states", "totals", "terms")}


def replay(terms):
    """V of every step from the hinges alone: V = fma(h, h, V) over slots 5 .. 19 in order, from the previous step's slot 20
    (+0 at step 0).  terms [..., n, 22] -> [..., n] float32."""
    terms = np.asarray(terms, dtype=T)
    out = np.empty(terms.shape[:-1], dtype=T)
    for i in range(terms.shape[-2]):
        V = np.zeros(terms.shape[:-2], dtype=T) if i == 0 else terms[..., i - 1, V_SLOT]
        for slot in range(HINGES.start, HINGES.stop):
            h = terms[..., i, slot]
            V = np.asarray(fma32(h, h, V), dtype=T)
        out[..., i] = V
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=T).view(np.uint32)
