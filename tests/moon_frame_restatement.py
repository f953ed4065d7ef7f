"""The moon-centred frame of include/nexoclom_hip.h ("Moon-centred frame"), restated in NumPy fp64
from the definition.  The only source of expected values of the moon-frame tests: nothing here
calls the package.

Moon of radius ``rad`` and orbit radius ``a`` [R], rate ``omega`` [rad/s], phase ``phi`` at
t_remaining = 0:

    M = a (-sin phi, cos phi, 0)          U = a omega (-cos phi, -sin phi, 0)          k = 1/rad

and a row (t, x, y, z, vx, vy, vz) becomes, with theta = omega t,

    p' = (R_z(theta) p - M) k             v' = (R_z(theta) v - U) k

R_z(theta) (x, y) = (c x - s y, s x + c y).  Float32 rows are widened, computed in fp64 and rounded
once.
"""
from collections import namedtuple

import numpy as np

Frame = namedtuple('Frame', 'omega M U scale')
IDENTITY = Frame(0.0, np.zeros(3), np.zeros(3), 1.0)


def moon_frame(rad, a, omega, phi):
    """The frame of a moon from its orbit, all in fp64."""
    M = np.array([-a*np.sin(phi), a*np.cos(phi), 0.0])
    U = np.array([-a*omega*np.cos(phi), -a*omega*np.sin(phi), 0.0])
    return Frame(float(omega), M, U, 1.0/rad)


def moon_at(a, omega, phi, t):
    """Position and velocity of the moon at t_remaining = t (phase phi - omega t; time runs
    against t_remaining), shape (..., 3)."""
    ang = phi - omega*np.asarray(t, dtype=np.float64)
    zero = np.zeros_like(ang)
    return (np.stack([-a*np.sin(ang), a*np.cos(ang), zero], -1),
            np.stack([-a*omega*np.cos(ang), -a*omega*np.sin(ang), zero], -1))


def move_rows(frame, t, x, y, z, vx, vy, vz):
    """(6, n) x', y', z', vx', vy', vz' of the rows, in the dtype of ``x`` (float32 rows are
    rounded once, at the end)."""
    out_type = np.asarray(x).dtype
    t, x, y, z, vx, vy, vz = (np.asarray(c, dtype=np.float64) for c in (t, x, y, z, vx, vy, vz))
    theta = frame.omega*t
    s, c = np.sin(theta), np.cos(theta)
    k = frame.scale
    moved = [((c*x - s*y) - frame.M[0])*k, ((s*x + c*y) - frame.M[1])*k, (z - frame.M[2])*k,
             ((c*vx - s*vy) - frame.U[0])*k, ((s*vx + c*vy) - frame.U[1])*k,
             (vz - frame.U[2])*k]
    return np.stack(moved).astype(out_type)


def bounds(frame, x, y, vx, vy):
    """(position bound, velocity bound) per row of |got - want| for x' and y' computed in fp64:
    8 * 2^-52 * (|x| + |y| + |M_x| + |M_y|) * k, and the same with U for the velocities -- two
    products with a sine and cosine good to 2 ulp, one subtraction, one scaling: at most 6 ulp of
    the largest term; 8 covers an fma contraction on either side."""
    x, y, vx, vy = (np.abs(np.asarray(c, dtype=np.float64)) for c in (x, y, vx, vy))
    eps = 8*2.0**-52
    return (eps*(x + y + abs(frame.M[0]) + abs(frame.M[1]))*frame.scale,
            eps*(vx + vy + abs(frame.U[0]) + abs(frame.U[1]))*frame.scale)


def f32_ulp(want):
    """One float32 ulp of ``want`` (the spacing at |want|), as float64."""
    return np.spacing(np.abs(np.asarray(want, dtype=np.float32))).astype(np.float64)


def corotating_rows(a, omega, phi, rad, d, u, t):
    """Rows of a point that stands still in the moon's frame at ``d`` [moon radii] with the
    velocity ``u`` [moon radii / s] there: p_j = R_z(-omega t_j)(M + d rad), v_j = R_z(-omega t_j)
    (U + u rad).  Returns (t, x, y, z, vx, vy, vz)."""
    frame = moon_frame(rad, a, omega, phi)
    t = np.asarray(t, dtype=np.float64)
    P = frame.M + np.asarray(d, dtype=np.float64)*rad
    W = frame.U + np.asarray(u, dtype=np.float64)*rad
    s, c = np.sin(-omega*t), np.cos(-omega*t)
    ones = np.ones_like(t)
    return (t, c*P[0] - s*P[1], s*P[0] + c*P[1], P[2]*ones,
            c*W[0] - s*W[1], s*W[0] + c*W[1], W[2]*ones)
