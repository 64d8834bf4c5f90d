"""Restatements of guided distillation for the host and the GPU tests, on top of distill_helpers.

1. ``cfg_np``: the guided combination ``e = out_u + w (out_c - out_u)`` of common.h's cfg_eps - subtraction, product,
   sum, one rounding each, in the dtype of its inputs.
2. ``guided_kernels_np``: the two-step pair - ``distill_helpers.kernels_np`` on the combined outputs, which is all the
   guided kernels change; ``guidance_target_np``: the same-timestep kernel.  fp32 is what the device must produce bit
   for bit, fp64 on the same fp32 table what the forward-error bound is measured against.
3. The bounds, by the rule of distill_helpers (3.): a chain of n roundings from exact inputs is off by at most
   ``((1 + u)^n - 1) S``, S the sum of the absolute products of the expanded expression; the n stated here is the
   count along the longest path plus one, which covers the terms of second order in u ((1 + u)^k - 1 <= (k + 1) u for
   every k counted here).  The combination adds 3 roundings (subtraction, product, sum) in front of whatever consumes
   the teacher's output, and a path passes through ONE teacher output:
       z_mid  = A1 (p1 z + q1 e1) + B1 z          3 + product, sum, product, sum                    =  7, n =  8
       target = G (W2 (p2 z_mid + q2 e2) + W1 x1c) + H z     7 for z_mid, then 6 (through e2: 3 + 6) = 13, n = 14
       same-timestep target = G (p z + q e) + H z  product, sum, product, sum: unguided 4, n = 5; guided 7, n = 8
   i.e. ``distill_helpers.N_ZMID + 3`` and ``N_TARGET + 3``.  In S the combination's magnitude is
   ``|out_u| + |w| (|out_c| + |out_u|)``.  w is an input, exact in fp32 for every value tested."""
import numpy as np

import distill_helpers as H
from distill_helpers import U, bits, forward_process  # noqa: F401  (re-exported)

N_CFG = 3
N_ZMID_G, N_TARGET_G = H.N_ZMID + N_CFG, H.N_TARGET + N_CFG
N_SAME, N_SAME_G = 5, 5 + N_CFG
WS = (0.0, 1.0, 3.5, -0.5)


def cfg_np(oc, ou, w):
    """out_u + w (out_c - out_u), one operation per rounding, in the arrays' dtype."""
    dt = oc.dtype
    d = oc - ou
    m = dt.type(w) * d
    e = ou + m
    assert e.dtype == dt
    return e


def cfg_mag(oc, ou, w):
    oc, ou = (np.abs(np.asarray(v, dtype=np.float64)) for v in (oc, ou))
    return ou + abs(float(w)) * (oc + ou)


def guided_kernels_np(rows, t, z, o1, o2, w, lo, hi):
    """The guided two-step pair; ``o1`` / ``o2`` are (2, B, ...): the outputs under the condition, then under the null
    condition.  The dict of ``distill_helpers.kernels_np`` plus the two combinations."""
    e1, e2 = cfg_np(o1[0], o1[1], w), cfg_np(o2[0], o2[1], w)
    out = H.kernels_np(rows, t, z, e1, e2, lo, hi)
    out.update(e1=e1, e2=e2)
    return out


def guided_magnitudes(rows, t, z, o1, o2, w):
    """(S_zmid, S_target, S_x1) of the guided pair in fp64."""
    return H.magnitudes(rows, t, z, cfg_mag(o1[0], o1[1], w), cfg_mag(o2[0], o2[1], w))


def _cols4(rows_t, ndim):
    return [rows_t[:, i].reshape((-1,) + (1,) * (ndim - 1)) for i in range(4)]


def guidance_target_np(rows4, t, z, e, lo, hi):
    """The same-timestep kernel on the (combined) output e: a dict of x0c and target, in the arrays' dtype."""
    dt = z.dtype
    p, q, G, Hh = _cols4(np.asarray(rows4)[np.asarray(t)].astype(dt), z.ndim)
    lo, hi = dt.type(lo), dt.type(hi)
    a = p * z
    b = q * e
    x0c = np.minimum(np.maximum(a + b, lo), hi)
    a = G * x0c
    b = Hh * z
    target = a + b
    assert x0c.dtype == dt and target.dtype == dt
    return {"x0c": x0c, "target": target}


def guidance_magnitude(rows4, t, z, e_mag):
    """S of the same-timestep target in fp64; ``e_mag``: |out|, or ``cfg_mag`` under guidance."""
    z = np.abs(np.asarray(z, dtype=np.float64))
    p, q, G, Hh = (np.abs(c) for c in _cols4(np.asarray(rows4)[np.asarray(t)].astype(np.float64), z.ndim))
    return G * (p * z + q * np.asarray(e_mag, dtype=np.float64)) + Hh * z


def guided_case(rng, rows32, t, shape, w):
    """Random (z, o1, o2) fp32 with o1, o2 of shape (2, B, ...), scaled per sample as ``distill_helpers.clamp_case``
    does and once more by the combination's gain, so that the implied x0 straddles the bounds (-1, 1) at every w."""
    gain = float(np.sqrt((1.0 - w) ** 2 + w ** 2))
    z, c1, c2 = H.clamp_case(rng, rows32, t, shape)
    _, u1, u2 = H.clamp_case(rng, rows32, t, shape)
    o1 = (np.stack([c1, u1]) / gain).astype(np.float32)
    o2 = (np.stack([c2, u2]) / gain).astype(np.float32)
    return z, o1, o2
