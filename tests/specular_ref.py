"""Yardstick of the physical specular model (include/pm_api.h
pm_add_material_specular; tests/test_specular.py, test_specular_gpu.py): the
Fresnel term, the lobe choice and the directions in float64 from the float32
parameters, and the two Philox draws through the oracle module, as
tests/mesh_light_ref.py takes its light samples.
"""
import numpy as np

import oracle

F32 = np.float32


def u01(word):
    """pmdm_u01: the top 24 bits as a float32 in [0, 1)"""
    return F32(word >> 8) * F32(1.0 / 16777216.0)


def photon_u(pid, n_i, pass_index, spec, seed, mpc=4):
    """The draw of a photon path's specular step: counter (pid mpc + nI, pass, spec, 0), key (seed, 0);
    nI >= 1 is the path's deposit counter at the hit, spec >= 1 its specular count including the hit."""
    assert n_i >= 1 and spec >= 1
    o = oracle.philox(((int(pid) * mpc + int(n_i)) & 0xffffffff, int(pass_index), int(spec), 0), (int(seed), 0))
    return u01(o[0])


def eye_u(q, depth, light_seed):
    """The draw of an eye chain's step: counter (lo32 q, hi32 q, 2, depth), key (light_rng_seed, 0)."""
    assert depth >= 1
    o = oracle.philox((int(q) & 0xffffffff, int(q) >> 32, 2, int(depth)), (int(light_seed), 0))
    return u01(o[0])


def fresnel(cos, index, dtype=np.float64):
    """F of pbrt-v2's FresnelDielectric(1, index) for wo.z = cos (its sign picks the side), float64;
    also eta = ei / et and cost (0 at total internal reflection). dtype = float32 runs the same
    operations in the device's precision: its distance from float64 on a test's own inputs is the
    floor that test's tolerance comes from."""
    cos = np.asarray(cos, dtype)
    index = dtype(F32(index))
    one, zero = dtype(1.0), dtype(0.0)
    entering = cos > 0
    ei = np.where(entering, one, index)
    et = np.where(entering, index, one)
    eta = ei / et
    sint2 = eta * eta * np.maximum(zero, one - cos * cos)
    tir = sint2 >= 1.0
    cost = np.sqrt(np.maximum(zero, one - np.where(tir, one, sint2)))
    ci = np.abs(cos)
    with np.errstate(invalid="ignore", divide="ignore"):
        rpar = (et * ci - ei * cost) / (et * ci + ei * cost)
        rper = (ei * ci - et * cost) / (ei * ci + et * cost)
    F = np.where(tir, one, dtype(0.5) * (rpar * rpar + rper * rper))
    return F, eta, cost


def ulp32(x):
    """the spacing of float32 at x"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(F32)).astype(np.float64)


MARGIN_ULPS = 8   # paths with |u - F| below this many fp32 ulps of F are left out of a choice test


def point_light_choice(paths, index, seed, mpc=4, min_cos=0.05):
    """The lobe each upward path of a point light under a horizontal glass quad takes at its first hit:
    (path ids, directions, F, eta, cost, u, sure) in float64, from the Halton emission samples
    (mesh_light_ref.emission_samples) and the photon draw; sure: |u - F| >= MARGIN_ULPS ulps of F."""
    import mesh_light_ref as M
    smp = M.emission_samples(paths, mpc).astype(np.float64)
    z = 1.0 - 2.0 * smp[:, 0]
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    d = np.stack([r * np.cos(2 * np.pi * smp[:, 1]), r * np.sin(2 * np.pi * smp[:, 1]), z], 1)
    up = np.nonzero(z > min_cos)[0]
    F, eta, cost = fresnel(z[up], index)
    u = np.array([photon_u(pid, 1, 0, 1, seed, mpc) for pid in up], np.float64)
    return up, d[up], F, eta, cost, u, np.abs(u - F) >= MARGIN_ULPS * ulp32(F)


def glass_step(wo, u, kr, kt, index):
    """One step through glass in the local frame, float64. wo: (3,) towards where the ray came from.
    Returns None when both lobes are black, else (reflected?, wi, weight, eta2, F, q)."""
    kr, kt = np.asarray(F32(kr), np.float64), np.asarray(F32(kt), np.float64)
    F, eta, cost = (float(v) for v in fresnel(wo[2], index))
    wr, wt = F * kr, (1.0 - F) * kt
    rb, tb = not wr.any(), not wt.any()
    if rb and tb:
        return None
    q = 1.0 if tb else (0.0 if rb else F)
    both = 0.0 < q < 1.0
    if float(u) < q:
        return True, np.array([-wo[0], -wo[1], wo[2]]), (kr if both else wr), 1.0, F, q
    wi = np.array([eta * -wo[0], eta * -wo[1], -cost if wo[2] > 0 else cost])
    return False, wi, (kt if both else wt), eta * eta, F, q


def mirror_weight_chain(alpha, kr, k):
    """fl(alpha * Kr) applied k times in float32: a photon's flux after k hits of a coloured mirror"""
    a, kr = np.asarray(alpha, F32).copy(), np.asarray(kr, F32)
    for _ in range(k):
        a = (a * kr).astype(F32)
    return a
