"""Cases and the reference of the tick prologue's tables (csrc/acmpc_prologue.hip: `prologue_kernel`), shared by
tests/test_prologue_cases.py (CPU: the case list's own conditions, the library's host statements) and
tests/test_gpu_prologue_tables.py (the kernel, by every input route).  Plain module: NumPy and oracle/acmpc_oracle.py only,
nothing of the library.

The kernel gives a lane one waypoint up to n = 64 and two beyond, takes the path out of its arguments up to H = 64 points and
from pinned memory beyond, and is accepted up to n = 128: the horizons below sit on both sides of each of those numbers.  The
paths turn through more than pi (a left arc's heading runs from pi/2 across +-pi), start next to +-pi (the rotated s-bends:
neighbouring headings of opposite sign from the first pair on) and wiggle; the settings cycle through the localised ceiling
and a profile without an end velocity.

`check_tables` is the one statement of what is asserted about a set of tables, whoever made them:
  x, y, ds, width   bit-equal to `orc.construct_waypoints` (IEEE + - * sqrt only);
  psi               within `psi_ulps` ulp(pi) of the heading evaluated in long double on the same float64 differences;
  kappa             within the bound that follows from `psi_ulps` (kappa_bound), kappa[0] == kappa[1], |turn| <= pi;
  v                 bit-equal to `orc.speed_profile_exact` on the NumPy ceiling (`velocity_ceiling`) of THESE kappa and ds;
  x0, coef, u_ref   from THESE tables in float64: copied columns bit-equal as float32, computed ones within one float32 ulp.
"""
import math
from types import SimpleNamespace

import numpy as np

import acmpc_oracle as orc
from test_support import RACING

HORIZONS = (3, 4, 50, 64, 65, 66, 128, 129)
SPACING = 2.45
RADII = (15.0, 25.0, 40.0)
CONS = dict(RACING["monza"]["speed_profile_constraints"], v_max=28.0)
LIMITS = orc.vehicle_limits(2.65, 1.94, 0.30, CONS["v_min"], CONS["v_max"])
BOX = orc.input_box(LIMITS)
ULP_PI = float(np.spacing(np.pi))
# The host statement's atan2 is the C library's: glibc's double atan2 is within 1 ulp of the result (its manual's table of
# known errors), and a heading's own ulp is at most ulp(pi).
PSI_ULPS_HOST = 1.0
MODES = {"S": (0, None), "T": (1, None), "Tw": (1, (2, 5))}   # label -> (engine mode, nearest-waypoint window)


def widths(H):
    return np.linspace(10.0, 6.0, H)


def from_headings(theta):
    """H x 3 path whose segment i has length SPACING and heading theta[i], from the origin."""
    theta = np.asarray(theta, dtype=np.float64)
    H = theta.shape[0] + 1
    xy = np.zeros((H, 2))
    xy[1:, 0] = np.cumsum(SPACING * np.cos(theta))
    xy[1:, 1] = np.cumsum(SPACING * np.sin(theta))
    return np.column_stack([xy, widths(H)])


def arc(H, radius, sign, lead):
    """Straight along +y for `lead` points, then a circle of `radius` to the left (sign +1) or the right (-1)."""
    s = SPACING * np.arange(H)
    turned = np.maximum(s - s[lead - 1], 0.0) / radius
    x = -sign * radius * (1.0 - np.cos(turned))
    y = np.minimum(s, s[lead - 1]) + radius * np.sin(turned)
    return np.column_stack([x, y, widths(H)])


def s_bend(H, sign):
    """Along +y with the heading swinging 0.04 rad to either side, period six segments; segment 0 heads at pi/2 exactly and
    segment 1 0.035 rad to the left of it (sign +1) or the right (-1)."""
    i = np.arange(H - 1)
    return from_headings(math.pi / 2.0 + sign * 0.04 * np.sin(2.0 * math.pi * i / 6.0))


def rotated(path, heading):
    """`path` turned about its first point so that its first segment heads at `heading`."""
    d = path[1, :2] - path[0, :2]
    turn = heading - math.atan2(d[1], d[0])
    c, s = math.cos(turn), math.sin(turn)
    rel = path[:, :2] - path[0, :2]
    out = path.copy()
    out[:, 0] = path[0, 0] + c * rel[:, 0] - s * rel[:, 1]
    out[:, 1] = path[0, 1] + s * rel[:, 0] + c * rel[:, 1]
    return out


def wiggly(H, trial):
    """The family of test_the_exact_profile_on_the_device_at_other_horizons, seeded per H; the second one starts off the
    origin, so that the start state's lateral offset takes the waypoint's coordinates."""
    rng = np.random.default_rng(1000 * H + trial)
    y = SPACING * np.arange(H)
    x = rng.uniform(2.0, 12.0) * np.sin(y / rng.uniform(8.0, 40.0)) + 0.002 * rng.uniform(-1, 1) * y ** 2
    shift = (3.5, -7.25) if trial else (0.0, 0.0)
    return np.column_stack([x - x[0] + shift[0], y + shift[1], widths(H)])


def _cases_at(H):
    lead = 5 if H >= 33 else 1
    paths = [("arc_r%d_%s" % (r, "left" if sign > 0 else "right"), "arc", arc(H, r, sign, lead))
             for r in RADII for sign in (+1, -1)]
    paths.append(("rotated_to_plus_pi", "rotated", rotated(s_bend(H, +1), math.pi - 0.01)))
    paths.append(("rotated_to_minus_pi", "rotated", rotated(s_bend(H, -1), -math.pi + 0.01)))
    paths.append(("wiggly_0", "wiggly", wiggly(H, 0)))
    paths.append(("wiggly_1", "wiggly", wiggly(H, 1)))
    out = []
    for i, (name, family, coords) in enumerate(paths):
        out.append(SimpleNamespace(name="H%d_%s" % (H, name), H=H, n=H - 1, family=family, index=i,
                                   coords=np.ascontiguousarray(coords, dtype=np.float64),
                                   localised=int(i in (3, 8)), has_end_velocity=int(i % 2 == 0),
                                   offset=(1.0 if i % 2 == 0 else -1.0) * (0.1 + 0.03 * i)))
    return out


CASES = [case for H in HORIZONS for case in _cases_at(H)]


def cases_at(H):
    return [c for c in CASES if c.H == H]


# ---- the reference --------------------------------------------------------------------------------------------------------
def long_double_headings(coords):
    """atan2 of the float64 coordinate differences the table is made of (forward segments 0 .. n - 1, then the segment that
    closes the loop from the last point to point 0), evaluated in long double."""
    xy = np.asarray(coords, dtype=np.float64)[:, :2]
    ahead = np.concatenate([xy[1:] - xy[:-1], xy[:1] - xy[-1:]], axis=0)   # float64 differences, as every statement takes them
    wide = ahead.astype(np.longdouble)
    return np.arctan2(wide[:, 1], wide[:, 0])


def wrap_long_double(angle):
    """np.mod(a + pi, 2 pi) - pi with the float64 constant, in long double."""
    pi = np.longdouble(math.pi)
    return np.mod(angle + pi, 2 * pi) - pi


def long_double_kappa(coords, ds):
    seg = long_double_headings(coords)
    n = seg.shape[0] - 1
    behind = np.concatenate([seg[n:], seg[:n - 1]])
    kappa = wrap_long_double(seg[:n] - behind) / (ds.astype(np.longdouble) + orc.EPS) + orc.EPS
    kappa[0] = kappa[1]
    return kappa


def kappa_bound(psi_ulps, ds, kappa):
    """|kappa - long_double_kappa| allowed when every heading is within `psi_ulps` ulp(pi).  The turn wrap(psi[i] - psi[i-1])
    carries the two heading errors; its float64 evaluation rounds the difference (|.| < 2 pi: half an ulp(4) = 1 ulp(pi)), the
    sum with pi (|.| < 3 pi: half an ulp(8) = 2 ulp(pi)) and the final difference (|.| <= pi: 0.5 ulp(pi)); fmod is exact.
    That is divided by ds + eps; four relative 2^-53 cover the rounding of ds + eps, of the quotient and of the + eps."""
    turn = (2.0 * psi_ulps + 4.0) * ULP_PI
    return turn / (ds + orc.EPS) + 4.0 * 2.0 ** -53 * np.abs(kappa)


def velocity_ceiling(kappa, cons, localised, has_end_velocity):
    """speed_profile.py:26-43 (localised: 131-150) in NumPy, every form: the localised ceiling is v_max everywhere and takes
    no end velocity; without an end velocity the last ceiling is the curvature's."""
    n = kappa.shape[0]
    if localised:
        return np.full(n, float(cons["v_max"]))
    curvature = np.abs(kappa)
    c = np.sqrt(cons["ay_max"] / (curvature + 1e-12))
    c = np.where(curvature < cons["ki_min"], cons["v_max"], c)
    c = np.maximum(cons["v_min"], np.minimum(c, cons["v_max"])) + 2.0
    if has_end_velocity:
        c[n - 1] = cons["end_velocity"]
    return c


def reference_profile(case, kappa, ds):
    """(ceiling, profile or None) of `case` on the given curvatures and spacings."""
    ceiling = velocity_ceiling(kappa, CONS, case.localised, case.has_end_velocity)
    return ceiling, orc.speed_profile_exact(ceiling, ds, CONS["a_min"], CONS["a_max"], CONS["v_min"])


def reference_table(case):
    """The 7 x n table from the oracle and NumPy alone (float64 headings from long double, rounded once)."""
    table = orc.construct_waypoints(case.coords)
    table[orc.ROW_PSI] = long_double_headings(case.coords)[:case.n].astype(np.float64)
    table[orc.ROW_KAPPA] = long_double_kappa(case.coords, table[orc.ROW_DS]).astype(np.float64)
    ceiling, profile = reference_profile(case, table[orc.ROW_KAPPA], table[orc.ROW_DS])
    return table, ceiling, profile


def heading_jump(case):
    """The largest |psi[i + 1] - psi[i]| between neighbours."""
    psi = long_double_headings(case.coords)[:case.n].astype(np.float64)
    return float(np.abs(np.diff(psi)).max())


def heading_error(coords, psi):
    """The largest |psi - long double heading| in ulp(pi)."""
    exact = long_double_headings(coords)[:psi.shape[0]]
    return float(np.max(np.abs(psi.astype(np.longdouble) - exact))) / ULP_PI


def heading_error_in_own_ulps(coords, psi):
    """The same error in units of each heading's own last place (half an ulp(pi) below 2 rad, a quarter below 1)."""
    exact = long_double_headings(coords)[:psi.shape[0]]
    return float(np.max(np.abs(psi.astype(np.longdouble) - exact) / np.spacing(np.abs(exact.astype(np.float64)))))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(_bits(got), _bits(want)), "%s: %s != %s" % (what, got.ravel()[:6], want.ravel()[:6])


def assert_within_one_ulp32(got, want64, what):
    """`got` float32 against the float64 value: equal to its rounding or to a neighbour of it."""
    want = np.asarray(want64, dtype=np.float64).astype(np.float32)
    assert got.dtype == np.float32 and got.shape == want.shape, what
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp), what


def clip32(centre, box=BOX):
    """What the sampler makes of candidate 0 (orc.sample_candidates: fmin(fmax(., lo), hi) in float32)."""
    lo, hi = (np.asarray(b, dtype=np.float32) for b in box)
    return np.fmin(np.fmax(np.asarray(centre, dtype=np.float32), lo), hi)


def check_tables(case, mode, table, psi_ulps, coef=None, x0=None, u_ref=None, info=None, coords=None, what=""):
    """Everything the module docstring lists, for tables made from `coords` (default: the case's) with the case's settings
    by a handle of LIMITS / BOX.  `mode` is a key of MODES.  Returns the largest heading error in ulp(pi)."""
    what = "%s %s %s" % (case.name, mode, what)
    coords = case.coords if coords is None else coords
    n = coords.shape[0] - 1
    assert table.shape == (7, n) and table.dtype == np.float64, what
    want = orc.construct_waypoints(coords)
    for row, name in ((orc.ROW_X, "x"), (orc.ROW_Y, "y"), (orc.ROW_DS, "ds"), (orc.ROW_WIDTH, "width")):
        assert_bits(table[row], want[row], what + " " + name)
    assert_bits(table[orc.ROW_WIDTH], np.ascontiguousarray(coords[1:, 2]), what + " width is the next point's")
    psi, kappa, ds, v = table[orc.ROW_PSI], table[orc.ROW_KAPPA], table[orc.ROW_DS], table[orc.ROW_V]
    # psi
    error = heading_error(coords, psi)
    assert error <= psi_ulps, "%s psi: %.3f ulp(pi) > %.3f" % (what, error, psi_ulps)
    # kappa
    exact_kappa = long_double_kappa(coords, ds)
    off = np.abs(kappa.astype(np.longdouble) - exact_kappa).astype(np.float64)
    bound = kappa_bound(psi_ulps, ds, kappa)
    assert np.all(off <= bound), "%s kappa: %s over the bound at %s" % (what, (off / bound).max(), int(np.argmax(off / bound)))
    assert_bits(kappa[:1], kappa[1:2], what + " kappa[0] == kappa[1]")
    turn = (kappa - orc.EPS) * (ds + orc.EPS)                   # the wrapped heading difference itself: in [-pi, pi)
    assert np.all(np.abs(turn) <= math.pi * (1.0 + 1e-12)), what + " turn outside [-pi, pi)"
    # speed profile
    ceiling, profile = reference_profile(case, kappa, ds)
    assert profile is not None, what + " no feasible profile"
    assert_bits(v, profile, what + " speed profile")
    if case.localised:
        assert np.all(v == CONS["v_max"]), what
    elif not case.has_end_velocity:
        curvature_only = velocity_ceiling(kappa, CONS, 0, 0)
        assert ceiling[n - 1] == curvature_only[n - 1] and v[n - 1] <= curvature_only[n - 1], what
    if info is not None:
        assert info[4] == 0 and info[5] == 0, "%s status %s iterations %s" % (what, info[4], info[5])
    temporal = MODES[mode][0] == 1
    # x0
    if x0 is not None:
        assert x0.dtype == np.float32 and x0.shape == (3,), what
        if temporal:
            assert_bits(x0, np.array([case.offset, 0.0, math.pi / 2.0]).astype(np.float32), what + " pose")
        else:
            start = orc.t2s(table[:3, 0], (case.offset, 0.0, math.pi / 2.0))
            assert_within_one_ulp32(x0, start, what + " start state")
            assert x0[2] == 0.0 and -math.pi <= float(x0[1]) < math.pi, what + " e_psi outside [-pi, pi)"
    # coef
    if coef is not None:
        assert coef.dtype == np.float32, what
        if temporal:
            assert coef.shape == (n, orc.COEF_STRIDE_T), what
            rows = orc.coefficients_temporal(table, LIMITS.margin)
            copied = [orc.CT_X, orc.CT_Y, orc.CT_PSI, orc.CT_KREF, orc.CT_VREF, orc.CT_HALF]
            computed = {orc.CT_COS: np.cos(psi), orc.CT_SIN: np.sin(psi)}
        else:
            assert coef.shape == (n, orc.COEF_STRIDE_S), what
            rows = orc.coefficients_spatial(table, LIMITS.margin)
            copied = [orc.CS_DS, orc.CS_VREF, orc.CS_KREF, orc.CS_EYLO, orc.CS_EYHI, 9, 10, 11]
            f, A, B = orc.linearise(table)
            computed = {orc.CS_A21: A[:, 1, 0], orc.CS_A31: A[:, 2, 0], orc.CS_B31: B[:, 2, 0], orc.CS_F3: f[:, 2]}
        assert sorted(copied + list(computed)) == list(range(coef.shape[1])), what
        for column in copied:
            assert_bits(coef[:, column], np.ascontiguousarray(rows[:, column]), "%s coef column %d" % (what, column))
        for column, value in computed.items():
            assert_within_one_ulp32(np.ascontiguousarray(coef[:, column]), value, "%s coef column %d" % (what, column))
    # u_ref
    if u_ref is not None:
        want_u = np.stack([np.clip(v, BOX[0][0], BOX[1][0]), np.clip(kappa, BOX[0][1], BOX[1][1])], axis=1).astype(np.float32)
        assert_bits(u_ref, want_u, what + " u_ref")
    return error
