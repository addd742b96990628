"""Plain numpy float64 restatement of what 'bpf-a2c' and the Fisher analysis add to the particle filter of tests/_bpf_ref.py
(algos/test_environment/eval/test_policy.py:109-156, 361-371, 403-405, 432-436; FIC.particle_FIM, eval/core.py:686-694) for ONE
(env, agent) pair: the particles' 3 x 3 Fisher information matrix with the magnitude sum its summation bound is taken from, the
initial bound from the prior's particles, the controller's table of moves, and the observation the actor sees.  Particles are rows
[NP, 3] = (intensity, x, y) as in the reference; the kernels keep them [3, NP].

The allowance on every entry of the matrix is the one tests/_bpf_ref.py's controller uses for J_fish: (NP + 16) * 2^-52 times the sum
of the magnitudes of the entry's terms -- a float64 sum of NP terms taken in another order, with 16 ulps for the handful of operations
inside a term that may round differently (the column scale of the initial bound is 1e10 / 900 here, 1e10 * (1 / 900) there)."""
import numpy as np

ACTION = np.array([(-100, 0), (-71, 71), (0, 100), (71, 71), (100, 0), (71, -71), (0, -100), (-71, -71)], dtype=np.float64)   # test_policy.py:18-27
SCALE = np.array([1e10, 1.0, 1.0])                                 # the diagonal of scale_mat (test_policy.py:362)


def fim(xp, w, det, bkg, c=SCALE):
    """particle_FIM (core.py:686-694) with scale = diag(c) at the detector position det (x, y).  Returns (F [3, 3], the sum of the
    magnitudes of every entry's terms [3, 3])."""
    pred = xp.copy()
    pred[:, 0] = pred[:, 0] * 1e4
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        denom = np.sum(np.square(det - pred[:, 1:]), axis=1)
        grad_xy = (2 * (det - pred[:, 1:])) * (pred[:, 0] / np.square(denom))[:, None]
        grad = np.hstack(((1 / denom)[:, None], grad_xy))
        J = np.einsum('ij,ikl->ijk', grad, grad[:, :, None]) * (1 / (pred[:, 0] / denom + bkg))[:, None, None]
        Js = (J @ np.diag(np.asarray(c, dtype=np.float64))) * w[:, None, None]
        return Js.sum(axis=0), np.abs(Js).sum(axis=0)


def prior_scale(intensity, coord):
    """the diagonal of scale_mat @ uni_probs (test_policy.py:362-365) for the prior box intensity x coord x coord"""
    return np.array([1e10 / (intensity[1] - intensity[0]), 1 / (coord[1] - coord[0]), 1 / (coord[1] - coord[0])])


def prior_particles(prior_u, intensity, coord):
    """the prior's particles [NP, 3] from its uniforms [NP, 3] (core.py:556-557)"""
    xp = np.empty_like(prior_u)
    xp[:, 0] = intensity[0] + (intensity[1] - intensity[0]) * prior_u[:, 0]
    xp[:, 1:] = coord[0] + (coord[1] - coord[0]) * prior_u[:, 1:]
    return xp


def fim_prior(xp_init, det, bkg, intensity, coord):
    """the initial bound (test_policy.py:127-135): the matrix of the prior's particles with weights 1 / NP and scale @ uni_probs"""
    NP = xp_init.shape[0]
    return fim(xp_init, np.full(NP, 1 / NP), det, bkg, prior_scale(intensity, coord))


def tol(NP, mag):
    """the summation bound of an entry whose terms' magnitudes add up to mag"""
    return (NP + 16) * 2.0 ** -52 * mag


def trace(F):
    return (F[..., 0, 0] + F[..., 1, 1]) + F[..., 2, 2]


def standardise(reading, mean, std):
    """(float32)(((float64)reading - mean) / std), clipped to [-8, 8] (test_policy.py:400, 422)"""
    return np.clip(((np.asarray(reading, dtype=np.float32).astype(np.float64) - mean) / std).astype(np.float32), np.float32(-8), np.float32(8))


def pcrb(F0, R, noise_params):
    """the bound's recursion (test_policy.py:368-371, 435) for one lane: F0 [3, 3], R [T, 3, 3] -> [T + 1, 3, 3]"""
    D = np.linalg.inv(np.diag(np.square(np.array([noise_params[1], noise_params[0], noise_params[0]], dtype=np.float64))))
    B = [np.asarray(F0, dtype=np.float64)]
    for Rt in R:
        B.append(D + Rt - np.square(D) @ np.linalg.inv(B[-1] + D))
    return np.array(B)
