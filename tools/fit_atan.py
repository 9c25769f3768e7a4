#!/usr/bin/env python3
"""The odd polynomial of mode D's arctangent (csrc/acmpc_dynamic.h: atan_spec; tests/dynamic_spec.py: atan_spec).

    atan t = t + t^3 P(t^2),  t in [0, 1],  P of degree K - 1 in t^2

fitted by Lawson-weighted least squares (iteratively re-weighted towards the minimax error), the coefficients rounded to
float32, then the float32 evaluation - Horner in t^2 with every multiply-add ONE fused multiply-add, exactly as the kernel
runs it - checked on a dense sweep of [0, 1] against float64 arctan, and on the whole real line through the reduction
atan x = pi/2 - atan(1/x) (|x| > 1).  Prints the coefficients and the errors.  NumPy only.

usage: python3 tools/fit_atan.py [terms]      (default 8)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from acmpc_oracle import fma32  # noqa: E402


def lawson_fit(terms, iterations=200):
    t = np.linspace(1e-4, 1.0, 20001)
    target = (np.arctan(t) - t) / t ** 3              # P(t^2) in the relative sense of the t^3 term
    basis = np.stack([(t * t) ** k for k in range(terms)], axis=1)
    scale = t ** 3                                    # absolute error of atan = t^3 * error of P
    weight = np.ones_like(t)
    coef = None
    for _ in range(iterations):
        sw = np.sqrt(weight) * scale
        coef, *_ = np.linalg.lstsq(basis * sw[:, None], target * sw, rcond=None)
        err = np.abs((basis @ coef - target) * scale)
        weight = weight * (err + 1e-30)
        weight /= weight.sum()
    return coef


def evaluate32(t, coef32):
    """The kernel's sequence: p = c_{K-1}; p = fma(t2, p, c_k) down to c_0; atan = fma(t t2, p, t)."""
    t = np.asarray(t, dtype=np.float32)
    t2 = t * t
    p = np.full_like(t, coef32[-1])
    for c in coef32[-2::-1]:
        p = fma32(t2, p, np.float32(c))
    return fma32(t * t2, p, t)


def main():
    terms = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    coef32 = lawson_fit(terms).astype(np.float32)
    t = np.linspace(0.0, 1.0, 2000001, dtype=np.float32)
    err = np.abs(evaluate32(t, coef32).astype(np.float64) - np.arctan(t.astype(np.float64)))
    print("terms %d: max |error| on [0, 1] (float32 evaluation) %.3g" % (terms, err.max()))
    print("coefficients:", ", ".join(repr(float(c)) for c in coef32))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dynamic_spec
    x = np.concatenate([np.linspace(-40.0, 40.0, 2000001, dtype=np.float32),
                        np.geomspace(1e-30, 3e38, 200001).astype(np.float32)])
    full = np.abs(dynamic_spec.atan_spec(x).astype(np.float64) - np.arctan(x.astype(np.float64)))
    print("atan_spec over the real line: max |error| %.3g (bound %.1g)" % (full.max(), dynamic_spec.ATAN_ERROR_BOUND))


if __name__ == "__main__":
    main()
