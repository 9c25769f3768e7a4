"""The sampler's normals and candidate sets in plain float64, written from the definitions ("The
sampler") - NOT from the kernel's operation order: library log / sqrt / cos / sin, the knot positions as fractions, plain
sums and products.  tests/test_sampler_float64.py holds the oracle's bit-for-bit restatement (oracle.log_spec,
box_muller_spec, candidate_normals, sample_segments, sample_candidates) to it, tests/test_gpu_sampler_float64.py the
kernels.  A helper of the tests, not a test file.

Two things are taken as given because they are the specification and not an accuracy choice: Philox4x32-10 (integer
arithmetic, held to Random123's known answers in tests/test_capi_host.py), and the uniform, which IS a float32 value -
the float32 nearest (k + 1/2) 2^-24 - widened to float64 here.  The centre, u_ref, the box and sigma are float32 data too.

Nothing here calls oracle.log_spec, box_muller_spec, uniform_open, candidate_normals, sample_segments or
sample_candidates.  Philox is bound at import, so a test that plants a defect in the oracle's does not reach this file.

The statistics at the end (moments, Kolmogorov-Smirnov, correlations) are what both test files hold a set of normals to."""
from __future__ import annotations

import numpy as np
from scipy.special import ndtr

from acmpc_oracle import philox4x32_10 as _philox

KNOTS = 8
Z_MAX = float(np.sqrt(50.0 * np.log(2.0)))   # sqrt(-2 ln 2^-25) = 5.8871: the smallest uniform gives the largest radius


def uniforms64(words):
    """32 random bits -> the float32 nearest (k + 1/2) 2^-24 with k the top 24 bits, as float64.  In (0, 1]: the product
    is exact in float64, and only k = 2^24 - 1 (1 - 2^-25, a tie between 1 - 2^-24 and 1) rounds to 1."""
    k = (np.asarray(words, dtype=np.uint32) >> 8).astype(np.float64)
    return ((k + 0.5) * 2.0 ** -24).astype(np.float32).astype(np.float64)


def box_muller64(u1, u2):
    """z = sqrt(-2 ln u1) (cos 2 pi u2, sin 2 pi u2) for float32 uniforms widened to float64."""
    u1 = np.asarray(u1, dtype=np.float32).astype(np.float64)
    u2 = np.asarray(u2, dtype=np.float32).astype(np.float64)
    radius = np.sqrt(-2.0 * np.log(u1))
    return radius * np.cos(2.0 * np.pi * u2), radius * np.sin(2.0 * np.pi * u2)


def block_uniforms(n_candidates, index_offset, problem, round_, seed):
    """The Philox words of every candidate as uniforms [N, 4 draws, 4 words] (float64 values of float32s) and the global
    indices: counter (uint32(index_offset + c), problem, round, q), key (seed's low word, seed's high word)."""
    gidx = (int(index_offset) + np.arange(n_candidates, dtype=np.int64)) % (1 << 32)
    ctr = np.empty((n_candidates, KNOTS // 2, 4), dtype=np.uint32)
    ctr[..., 0] = gidx[:, None]
    ctr[..., 1] = problem
    ctr[..., 2] = round_
    ctr[..., 3] = np.arange(KNOTS // 2)[None, :]
    key = np.array([int(seed) % (1 << 32), (int(seed) >> 32) % (1 << 32)], dtype=np.uint32)
    return gidx, uniforms64(_philox(ctr, np.broadcast_to(key, ctr.shape[:-1] + (2,))))


def normals64(n_candidates, index_offset, problem, round_, seed):
    """(global indices [N], z [N, 8 knots, 2 controls] float64): words 0 and 1 of draw q give knot 2q, words 2 and 3 knot
    2q + 1; the cosine is the first control's normal and the sine the second's."""
    gidx, u = block_uniforms(n_candidates, index_offset, problem, round_, seed)
    z = np.empty((n_candidates, KNOTS, 2))
    z[:, 0::2, 0], z[:, 0::2, 1] = box_muller64(u[..., 0], u[..., 1])
    z[:, 1::2, 0], z[:, 1::2, 1] = box_muller64(u[..., 2], u[..., 3])
    return gidx, z


def knots64(n):
    """Per step i of n: (left knot k_i, weight w0_i of the left knot); knot k_i + 1 gets 1 - w0_i.  pos_i = 7 i / (n - 1)
    (0 at n = 1), k_i = min(floor pos_i, 6), w0_i = (1 + cos pi (pos_i - k_i)) / 2.  The position is taken as an exact
    fraction, so the floor and the remainder carry no rounding."""
    i = np.arange(n, dtype=np.int64)
    den = max(n - 1, 1)
    num = (KNOTS - 1) * i if n > 1 else np.zeros(n, dtype=np.int64)
    k = np.minimum(num // den, KNOTS - 2)
    frac = (num - k * den) / den
    return k, 0.5 * (1.0 + np.cos(np.pi * frac))


def amplitude64(gidx):
    """((g & 7) + 1) / 8; global candidate 0 has none."""
    gidx = np.asarray(gidx, dtype=np.int64)
    return np.where(gidx == 0, 0.0, ((gidx & 7) + 1) / 8.0)


def spread_factor(n):
    """sqrt(w0^2 + w1^2) per step: a step's noise w0 z_k + w1 z_{k+1} of two independent standard normals has this standard
    deviation - 1 on a knot, sqrt(1/2) = 0.71 midway between two."""
    _, w0 = knots64(n)
    return np.sqrt(w0 * w0 + (1.0 - w0) * (1.0 - w0))


def candidates64(centre, u_ref, n_candidates, index_offset, problem, round_, seed, sigma, u_lo, u_hi, u_extra=None):
    """U [N, n, 2] float64 = clip(base + sigma amp (w0 z_k + (1 - w0) z_{k+1}), lo, hi): base the centre, amp as
    amplitude64 - but global candidate 1 is `u_ref` and global candidate 2 `u_extra`, each where given, with no noise.
    sigma and the box are the float32 of the doubles passed (what the handle keeps)."""
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)   # noqa: E731
    centre = f32(centre)
    n = centre.shape[0]
    gidx, z = normals64(n_candidates, index_offset, problem, round_, seed)
    k, w0 = knots64(n)
    amp = amplitude64(gidx)
    base = np.broadcast_to(centre, (n_candidates, n, 2)).copy()
    for index, given in ((1, u_ref), (2, u_extra)):
        if given is not None:
            base[gidx == index] = f32(given)
            amp[gidx == index] = 0.0
    noise = w0[None, :, None] * z[:, k, :] + (1.0 - w0)[None, :, None] * z[:, k + 1, :]
    U = base + f32(sigma)[None, None, :] * amp[:, None, None] * noise
    return np.clip(U, f32(u_lo), f32(u_hi))


# ---- statistics of a set of would-be standard normals ---------------------------------------------------------------------
def moment_figures(z):
    """Mean, variance, skewness and excess kurtosis of the flattened set, each in ITS standard errors under the hypothesis
    (1 / sqrt M, sqrt(2 / M), sqrt(6 / M), sqrt(24 / M)), and the largest |z|."""
    z = np.asarray(z, dtype=np.float64).ravel()
    M = z.size
    mean = z.mean()
    d = z - mean
    var = np.mean(d * d)
    skew = np.mean(d ** 3) / var ** 1.5
    kurt = np.mean(d ** 4) / var ** 2 - 3.0
    return dict(M=M, mean=mean * np.sqrt(M), variance=(var - 1.0) / np.sqrt(2.0 / M), skewness=skew / np.sqrt(6.0 / M),
                kurtosis=kurt / np.sqrt(24.0 / M), largest=float(np.abs(z).max()))


def ks_figure(z):
    """Kolmogorov-Smirnov against the standard normal distribution: D sqrt M."""
    z = np.sort(np.asarray(z, dtype=np.float64).ravel())
    M = z.size
    F = ndtr(z)
    i = np.arange(M)
    D = max(np.max((i + 1) / M - F), np.max(F - i / M))
    return float(D * np.sqrt(M))


def correlation_figure(a, b):
    """|rho| sqrt M of two sets taken element by element (standard error 1 / sqrt M when they are independent)."""
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    a = a - a.mean()
    b = b - b.mean()
    rho = np.dot(a, b) / np.sqrt(np.dot(a, a) * np.dot(b, b))
    return float(abs(rho) * np.sqrt(a.size))


def within_candidate_figures(z):
    """The pairings inside one candidate of z [M, 8, 2], each as |rho| sqrt(samples): the two outputs of a Box-Muller pair
    (= the two control components of a knot) and their squares, the two pairs of a Philox block, every pair of knots
    (neighbours first) in either component, and a knot's first component with another knot's second."""
    z = np.asarray(z, dtype=np.float64)
    out = dict(pair=correlation_figure(z[:, :, 0], z[:, :, 1]),
               pair_squares=correlation_figure(z[:, :, 0] ** 2, z[:, :, 1] ** 2),
               block=max(correlation_figure(z[:, 0::2, a], z[:, 1::2, b]) for a in (0, 1) for b in (0, 1)),
               neighbours=max(correlation_figure(z[:, :-1, a], z[:, 1:, b]) for a in (0, 1) for b in (0, 1)))
    out["knots"] = max(correlation_figure(z[:, i, a], z[:, j, b])
                       for i in range(KNOTS) for j in range(i + 1, KNOTS) for a in (0, 1) for b in (0, 1))
    return out
