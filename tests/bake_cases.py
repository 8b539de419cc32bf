"""Inputs shared by the bake tests (tests/test_bake_model.py on the CPU, tests/test_gpu_bake.py on the GPU): lightmap UV
sets for a 36-triangle mesh -- cornell's triangle count -- that hold every case the coverage definition separates, and
the map sizes they are rasterised at.  Nothing here is random per run."""
import numpy as np

F32 = np.float32
N_TRIS = 36
MAPS = ((1, 1), (7, 5), (64, 64), (65, 63), (130, 3))  # (W, H)


def crafted_uv(n_tris=N_TRIS):
    """One UV set with a triangle larger than the map (its box is clipped), one wholly outside [0, 1], a zero-area
    one, one with a NaN UV, two that overlap (4 and 5: the lower id owns the overlap), and two (6 and 7, counter-
    clockwise and clockwise) that share the edge u == v, which passes exactly through the centres of a square map's
    diagonal texels.  The rest have zero area.  At every map of MAPS above 1 x 1 some texels are covered and the
    neighbourhood of (0.2, 0.7) is not."""
    uv = np.zeros((n_tris, 6), F32)
    uv[0] = [-0.5, -0.5, 0.9, -0.5, -0.5, 0.9]
    uv[1] = [1.5, 1.5, 2.5, 1.5, 1.5, 2.5]
    uv[2] = [0.2, 0.2, 0.4, 0.4, 0.6, 0.6]
    uv[3] = [0.1, 0.6, np.nan, 0.6, 0.1, 0.9]
    uv[4] = [0.55, 0.05, 0.95, 0.05, 0.55, 0.45]
    uv[5] = [0.6, 0.05, 0.95, 0.4, 0.6, 0.4]
    uv[6] = [0.5, 0.5, 1.0, 1.0, 0.5, 1.0]
    uv[7] = [0.5, 0.5, 1.0, 1.0, 1.0, 0.5]
    return uv


def random_uv(n_tris=N_TRIS, seed=11):
    """Random overlapping triangles of both windings in the left half of the map, u in [-0.1, 0.5], v in [-0.1, 1.1]:
    the owner rule among many candidates.  The right half stays uncovered."""
    rng = np.random.default_rng(seed)
    uv = np.zeros((n_tris, 3, 2))
    c = np.stack([rng.uniform(0.0, 0.4, n_tris), rng.uniform(0.0, 1.0, n_tris)], axis=1)
    uv[:] = c[:, None, :] + rng.uniform(-0.1, 0.1, (n_tris, 3, 2)) * np.array([1.0, 2.0])
    uv[..., 0] = np.clip(uv[..., 0], -0.1, 0.5)
    return uv.reshape(n_tris, 6).astype(F32)


def mesh(n_tris=N_TRIS, seed=5):
    """(tri_pos [n][9], tri_normal [n][3]) float32 of a random mesh, for the tests that have no scene; some normals have
    a -0 component, which the definition's "+ 0.0f" turns into +0."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-2, 2, (n_tris, 9)).astype(F32)
    nrm = rng.normal(size=(n_tris, 3)).astype(F32)
    nrm[::3, 1] = F32(-0.0)
    return pos, nrm


def dilate_values(W, H, seed=3):
    return np.random.default_rng(seed).uniform(0, 4, (H, W, 3)).astype(F32)
