"""The torture scenes and rays (tests/torture.py) on the CPU: conditions on the oracle's answers alone,
so that the GPU comparisons of tests/test_gpu_torture.py cannot pass vacuously; the host kd tree and box
against the oracle's on scenes that lie entirely below zero on an axis; and the oracle's traversal against
a float64 brute force over all triangles, which needs no reference source.
"""
import numpy as np
import pytest

import torture

SCENES = [(d, p) for d in ("full", "mini") for p in ("origin", "translated")]
_cases = {}


@pytest.fixture(scope="module")
def case(ca, po, scenes, tmp_path_factory):
    directory = tmp_path_factory.mktemp("torture")

    def get(detail, placement):
        if (detail, placement) not in _cases:
            _cases[detail, placement] = torture.Case(ca, po, scenes, directory, detail, placement, device=False)
        return _cases[detail, placement]

    yield get
    _cases.clear()


@pytest.mark.parametrize("detail,placement", SCENES)
def test_scene_is_what_the_generator_made(case, detail, placement):
    """The product's loader reads back the generator's floats (positions, vertex normals, materials, in
    the soup's order), so both sides see the same scene; the sizes select the intended default builds."""
    c = case(detail, placement)
    for k in torture.LAYOUT:
        a, b = c.pair.tris[k], c.soup[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), k
    n = len(c.soup["pos"])
    assert n >= 65536 if detail == "full" else 1024 <= n < 65536
    P = c.soup["pos"].reshape(-1, 3, 3).astype(np.float64)
    area2 = np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1)
    assert (area2 == 0).sum() >= 129  # the repeated-vertex triangles and the point light
    assert ((area2 > 0) & (area2 < torture.EPS)).sum() >= 100  # tiny triangles below a unit ray's epsilon
    assert (area2 > 50.0).sum() == 2  # the room-spanning pair
    ids, surf = c.pair.oracle.lights()
    assert len(ids) == 130 and (surf == 0).sum() == 1  # panel, emissive sliver, emissive point
    m = c.pair.tris["vnrm"].reshape(-1, 3, 3).sum(axis=1)
    assert np.isfinite(m).all() and (np.abs(m).max(axis=1) > 0.5).all()  # a finite material normal everywhere
    e = c.pair.oracle.kd_export()
    lc = e["leaf_count"][e["is_leaf"] == 1]
    if detail == "full":  # leaves without a cull record (more than 16 references), and beyond 32
        assert (lc > 16).sum() >= 1000 and (lc > 32).sum() >= 16 and e["max_depth"] >= 36


@pytest.mark.parametrize("detail,placement", SCENES)
def test_ray_set_floors(case, detail, placement):
    """What the aimed rays must reach on the oracle alone.  Measured (full origin / full translated / mini
    origin / mini translated): class-a groups that disagree 16.4 / 17.5 / 17.0 / 17.6 % (a uniformly random
    ray set: 0 %); class d with another light 0 occluded up to dist, all at dist + 1 ulp; with the hit
    triangle as the light 67 / 97 / 79 / 108 of 762 rays still occluded at dist + 1 ulp; class b 318 / 310
    / 424 / 300 of 1,024 rays hit the triangle whose plane they lie in."""
    c = case(detail, placement)
    r, want, occ = c.rays, c.want, c.want_occ
    cls = r["cls"]
    assert 16000 <= len(cls) <= 20000
    for k in torture.CLASSES:
        assert (want["hit"][cls == k] == 1).sum() >= 64, k
    assert (want["hit"] == 0).sum() >= 64
    assert 0.25 <= occ.mean() <= 0.75
    # a: groups of five whose members differ in hit or triangle
    m = cls == "a"
    assert (r["group"][m].reshape(-1, 5) == r["group"][m].reshape(-1, 5)[:, :1]).all()
    tri = np.where(want["hit"][m] == 1, want["tri"][m].astype(np.int64), -1).reshape(-1, 5)
    share = (tri != tri[:, :1]).any(axis=1).mean()
    print("class a: %.1f %% of %d groups disagree" % (100 * share, len(tri)))
    assert share >= 0.08
    # d: strict t < tmax at the hit distance
    m = cls == "d"
    k, own, o = r["k"][m], r["own"][m] == 1, occ[m]
    base = r["group"][m]
    assert (want["hit"][base] == 1).all()
    assert np.array_equal(r["limit"][m], torture.ulps(want["dist"][base], k))
    assert m.sum() >= 5 * 1024
    assert (o[~own & (k <= 0)] == 0).all()
    assert (o[~own & (k >= 1)] == 1).all()
    still = int(o[own & (k == 1)].sum())
    print("class d: %d of %d rays with the hit triangle as light occluded at dist + 1 ulp" % (still, (own & (k == 1)).sum()))
    assert still >= 64
    # e: origins exactly on a split plane of the axis the ray runs along
    m = cls == "e"
    e = c.pair.oracle.kd_export()
    on = r["own"][m] == 1
    assert on.sum() >= 100
    run = np.argmax(np.abs(r["d"][m][on]), axis=1)
    planes = [set(e["split"][(e["is_leaf"] == 0) & (e["axis"] == a)].view(np.uint32).tolist()) for a in range(3)]
    coord = r["o"][m][on][np.arange(on.sum()), run].view(np.uint32)
    assert all(int(x) in planes[a] for x, a in zip(coord, run))
    assert (np.abs(r["d"][m]).sum(axis=1) == 1.0).all() and (np.abs(r["d"][m]).max(axis=1) == 1.0).all()
    # f: tiny components on each side of the short division's guard
    m = cls == "f"
    ex = r["own"][m]
    small = np.abs(r["d"][m]).min(axis=1).astype(np.float64)
    assert (small[ex != 0] == 2.0 ** ex[ex != 0]).all()
    assert (ex[ex != 0] < -40).sum() >= 100 and (ex[ex != 0] >= -40).sum() >= 100
    assert ((small > 0) & (small < 2.0 ** -126)).sum() >= 64  # subnormal
    assert (np.signbit(r["d"][m]) & (r["d"][m] == 0)).any(axis=1).sum() >= 64  # -0.0
    # b: the ray's own triangle is hit by some and not by others
    m = cls == "b"
    mine = (want["hit"][m] == 1) & (want["tri"][m] == r["own"][m])
    print("class b: %d of %d hit their own triangle" % (mine.sum(), m.sum()))
    assert 64 <= mine.sum() <= m.sum() - 64
    # g: exact powers of two of class-a rays, outside lc_unit's window (torture.rays asserts the windows)
    m = cls == "g"
    src = r["group"][m]
    assert np.array_equal(r["d"][m].astype(np.float64), r["d"][src].astype(np.float64) * 2.0 ** r["k"][m][:, None])
    assert np.array_equal(r["o"][m], r["o"][src]) and not r["unit"][m].any() and r["unit"][~m].all()
    # h: more than 1 outside the padded box on some axis: the kernels without the leaf cull
    oh = r["o"][cls == "h"]
    assert ((oh > e["box"][3:] + np.float32(1.0)) | (oh < e["box"][:3] - np.float32(1.0))).any(axis=1).all()


@pytest.mark.parametrize("detail,placement", SCENES)
def test_render_inputs(case, ca, detail, placement):
    """The three cameras' oracle renders are finite (a bitwise comparison of NaNs says nothing) and lit.
    Measured means: 0.13 (room), 0.044 (floor), 0.13 (wall) at full detail, 0.15 / 0.042 / 0.13 at mini."""
    c = case(detail, placement)
    for name, (eye, centre, up, yview) in torture.cameras(c.soup).items():
        cam = ca.camera(eye, centre, up, yview, 48, 36)
        img, ctr = c.pair.oracle.render(cam.as_array(), 48, 36, 4, 6, 0xC41A05C0)
        assert np.isfinite(img).all(), name
        assert img.mean() > 0.01, (name, img.mean())
        assert ctr["shadow"] > 48 * 36 * 4  # paths bounce and sample the lights
    eye = torture.cameras(c.soup)
    assert eye["floor"][0][1] == float(c.soup["room"][0][1]) and eye["wall"][0][0] == float(c.soup["room"][0][0])


@pytest.mark.parametrize("detail,placement", SCENES)
def test_host_tree_and_box(case, detail, placement):
    """The host kd build equals the oracle's, and the descriptor's box is the oracle's bit for bit -- on
    the translated scene with the reference's FLT_MIN start of the maximum: geometry entirely below zero
    on y gets box_max y = 1e-4 (src/kdtree.cpp:35)."""
    c = case(detail, placement)
    host, orc = c.pair.kd.export(), c.pair.oracle.kd_export()
    for k in ("is_leaf", "axis", "child", "leaf_first", "leaf_count", "refs"):
        np.testing.assert_array_equal(host[k], orc[k], err_msg=k)
    for k in ("split", "box"):
        np.testing.assert_array_equal(host[k].view(np.uint32), orc[k].view(np.uint32), err_msg=k)
    desc = c.pair.kd.describe()
    box = np.array(list(desc.box_min) + list(desc.box_max), np.float32)
    assert np.array_equal(box.view(np.uint32), orc["box"].view(np.uint32))
    assert desc.n_tris == len(c.soup["pos"]) and desc.max_depth == orc["max_depth"]
    if placement == "translated":
        assert c.soup["pos"].reshape(-1, 3)[:, 1].max() < -500.0
        assert 0.0 < box[4] < 2e-4


@pytest.mark.parametrize("placement", ["origin", "translated"])
def test_oracle_traversal_vs_float64_brute_force(case, placement):
    """1,024 random unit rays from inside the full room: at least 90 % are clear-cut for the float64 brute
    force over all triangles, and on every clear-cut ray the oracle's kd traversal finds the same hit flag
    and triangle, at a distance within leafcull.hpp's bound 10.05 u (S + t) g / cb + 2.1 u t of the float64
    one.  Measured: 983 / 983 clear-cut rays, 0 disagreements, at most 1.6 % / 1.5 % of the bound used."""
    c = case("full", placement)
    rng = np.random.default_rng(11)
    n = 1024
    room = c.soup["room"].astype(np.float64)
    o = (room[0] + 0.05 + rng.random((n, 3)) * (room[1] - room[0] - 0.1)).astype(np.float32)
    d = torture.unit32(rng.normal(size=(n, 3)))
    bf = torture.brute_force(c.soup, o, d)
    got = c.pair.oracle.intersect(o, d)
    clear = bf["clear"]
    print("clear-cut: %d of %d" % (clear.sum(), n))
    assert clear.sum() >= 0.9 * n
    assert np.array_equal(got["hit"][clear], bf["hit"][clear])
    h = clear & (bf["hit"] == 1)
    assert h.sum() >= n // 2
    assert np.array_equal(got["tri"][h], bf["tri"][h])
    err = np.abs(got["dist"][h].astype(np.float64) - bf["t"][h])
    bound = torture.dist_bound(bf)[h]
    print("largest share of the distance bound used: %.3f" % (err / bound).max())
    assert (err <= bound).all()
    # the brute force itself: a winner it calls clear is accepted with room to spare
    assert (bf["t"][h] > torture.TOL).all() and np.isfinite(bound).all()
