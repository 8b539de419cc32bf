"""Adversarial scenes and rays for the trace kernels (a helper module, not a conftest).

build(detail, offset, seed)   a closed 10 x 6 x 10 room full of what the exactness arguments of the trace
                              kernels exist for, as a triangle soup in Model.triangles() layout
write_obj(path, soup)         the soup as OBJ + MTL (%.9g coordinates, explicit vn on every corner, Ke on
                              the lights): the product's loader reads back exactly the soup's floats
rays(soup, oracle, seed)      about 18,000 finite rays aimed at edges, planes, split planes, the tmax edge
                              and the short-division guard, labelled by class
brute_force(soup, o, d)       float64 nearest hit over all triangles and whether the ray is clear-cut

The generator and the brute force are written from their descriptions; nothing here
reads the product's or the oracle's sources at run time.
"""
from __future__ import annotations

import numpy as np

ROOM = np.array([10.0, 6.0, 10.0])
PLACEMENTS = {"origin": (0.0, 0.0, 0.0), "translated": (1021.37, -515.9, 2043.11)}
EPS = 1.19209290e-7  # the reference's rejection of |a| (FLT_EPSILON)
U24 = 2.0 ** -24
LAYOUT = ("pos", "vnrm", "uv", "kd", "ke", "tex")
CLASSES = "abcdefgh"

_WHITE, _RED, _GREEN, _BLUE, _GREY = (0.725, 0.71, 0.68), (0.63, 0.065, 0.05), (0.14, 0.45, 0.091), \
    (0.1, 0.2, 0.7), (0.4, 0.4, 0.4)
_DETAIL = {  # wall quads along the 10-unit and the 6-unit sides, column segments and rings
    "full": (64, 40, 64, 16),
    "mini": (16, 10, 16, 4),
}


# ------------------------------------------------------------------ scene --
class _Soup:
    def __init__(self):
        self.t, self.n, self.kd, self.ke = [], [], [], []

    def add(self, tris, kd, ke=(0.0, 0.0, 0.0), hint=None):
        """tris (n, 3, 3) float64; hint (3,) or (n, 3): the winding is flipped where the face normal points
        against it.  The vertex normals are the unit face normal, or the hint (else +y) where the face has
        no area: every triangle keeps a finite, non-zero material normal."""
        t = np.array(tris, np.float64).reshape(-1, 3, 3)
        n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
        h = None if hint is None else np.broadcast_to(np.asarray(hint, np.float64), n.shape)
        if h is not None:
            flip = np.einsum("ij,ij->i", n, h) < 0
            t[flip] = t[flip][:, [0, 2, 1]]
            n[flip] = -n[flip]
        ln = np.linalg.norm(n, axis=1)
        fallback = np.broadcast_to(np.array([0.0, 1.0, 0.0]), n.shape) if h is None else \
            h / np.maximum(np.linalg.norm(h, axis=1), 1e-30)[:, None]
        flat = ln < 1e-12
        n = np.where(flat[:, None], fallback, n / np.maximum(ln, 1e-300)[:, None])
        self.t.append(t)
        self.n.append(n)
        self.kd.append(np.broadcast_to(np.asarray(kd, np.float64), (len(t), 3)))
        self.ke.append(np.broadcast_to(np.asarray(ke, np.float64), (len(t), 3)))


def _lattice_quads(P):
    """(nu + 1, nv + 1, 3) lattice -> (nu * nv * 2, 3, 3) triangles; shared vertices are the same floats."""
    a, b, c, d = P[:-1, :-1], P[1:, :-1], P[1:, 1:], P[:-1, 1:]
    q = np.stack([a, b, c, d], axis=2).reshape(-1, 4, 3)
    return np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], axis=1).reshape(-1, 3, 3)


def _grid(p0, du, dv, nu, nv):
    i = (np.arange(nu + 1) / nu)[:, None, None]
    j = (np.arange(nv + 1) / nv)[None, :, None]
    return _lattice_quads(np.asarray(p0, np.float64) + i * np.asarray(du, np.float64) + j * np.asarray(dv, np.float64))


def _unit_rows(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def _perp_rows(rng, u):
    v = np.cross(u, _unit_rows(rng, len(u)))
    return v / np.linalg.norm(v, axis=1)[:, None]


def build(detail="full", offset=(0.0, 0.0, 0.0), seed=1):
    """The torture room at `offset`.  Returns Model.triangles()'s dict (pos, vnrm, uv, kd, ke, tex) plus
    "room": the room's two corners as the float32 the walls have."""
    nl, ns, nseg, nring = _DETAIL[detail]
    rng = np.random.default_rng(seed)
    X, Y, Z = ROOM
    s = _Soup()
    # walls: axis-aligned, tessellated, facing in
    s.add(_grid((0, 0, 0), (X, 0, 0), (0, 0, Z), nl, nl), _WHITE, hint=(0, 1, 0))
    s.add(_grid((0, Y, 0), (X, 0, 0), (0, 0, Z), nl, nl), _WHITE, hint=(0, -1, 0))
    s.add(_grid((0, 0, 0), (0, 0, Z), (0, Y, 0), nl, ns), _RED, hint=(1, 0, 0))
    s.add(_grid((X, 0, 0), (0, 0, Z), (0, Y, 0), nl, ns), _GREEN, hint=(-1, 0, 0))
    s.add(_grid((0, 0, 0), (X, 0, 0), (0, Y, 0), nl, ns), _WHITE, hint=(0, 0, 1))
    s.add(_grid((0, 0, Z), (X, 0, 0), (0, Y, 0), nl, ns), _WHITE, hint=(0, 0, -1))
    # 16 columns, each with a cone of nseg triangles about one apex
    ang = 2.0 * np.pi * (np.arange(nseg + 1) % nseg) / nseg  # (the seam: the same floats)
    ys = 5.0 * np.arange(nring + 1) / nring
    for cx in (2.0, 4.0, 6.0, 8.0):
        for cz in (2.0, 4.0, 6.0, 8.0):
            r = 0.3
            ring = np.stack([cx + r * np.cos(ang), np.zeros_like(ang), cz + r * np.sin(ang)], axis=1)
            P = ring[:, None, :] + np.stack([np.zeros_like(ys), ys, np.zeros_like(ys)], axis=1)[None, :, :]
            t = _lattice_quads(P)
            c = t.mean(axis=1)
            s.add(t, _GREY, hint=np.stack([c[:, 0] - cx, np.zeros(len(c)), c[:, 2] - cz], axis=1))
            top = P[:, -1, :]
            apex = np.broadcast_to(np.array([cx, 5.3, cz]), (nseg, 3))
            fan = np.stack([apex, top[:-1], top[1:]], axis=1)
            c = fan.mean(axis=1)
            s.add(fan, _BLUE, hint=np.stack([c[:, 0] - cx, np.full(len(c), 0.5), c[:, 2] - cz], axis=1))
    # 512 slivers, 2 long and 1e-4 .. 1e-2 wide; those centred within 1 of a wall poke through it
    n = 512
    c = rng.random((n, 3)) * ROOM
    u = _unit_rows(rng, n)
    w = 10.0 ** rng.uniform(-4.0, -2.0, n)
    s.add(np.stack([c - u, c + u, c + w[:, None] * _perp_rows(rng, u)], axis=1), _RED)
    # 256 degenerate triangles: a repeated vertex; three points of one line (dyadic, so exactly collinear
    # at the origin and within the coordinates' rounding of it when translated)
    n = 128
    a = 0.5 + rng.random((n, 3)) * (ROOM - 1.0)
    b = a + 0.5 * _unit_rows(rng, n)
    s.add(np.stack([a, a, b], axis=1), _GREEN, hint=_unit_rows(rng, n))
    a = np.round((0.5 + rng.random((n, 3)) * (ROOM - 1.5)) * 256.0) / 256.0
    v = rng.integers(-8, 9, (n, 3)).astype(np.float64)
    v[(v == 0).all(axis=1)] = (1.0, 2.0, 3.0)
    v /= 256.0
    s.add(np.stack([a, a + 3.0 * v, a + 7.0 * v], axis=1), _GREEN, hint=_unit_rows(rng, n))
    # 64 quads given twice in different materials (equal t: the tie rule) and a third time 2e-6 along
    # the normal; the three copies of a quad follow one another
    n = 64
    c = 1.0 + rng.random((n, 3)) * (ROOM - 2.0)
    u = _unit_rows(rng, n)
    v = _perp_rows(rng, u)
    nn = np.cross(u, v)
    h = 0.25
    q = np.stack([c - h * u - h * v, c + h * u - h * v, c + h * u + h * v, c - h * u + h * v], axis=1)
    for k in range(n):
        t = np.stack([q[k, [0, 1, 2]], q[k, [0, 2, 3]]])
        s.add(t, _WHITE, hint=nn[k])
        s.add(t, _BLUE, hint=nn[k])
        s.add(t + 2e-6 * nn[k], _RED, hint=nn[k])
    # 512 tiny triangles, edges 2^-13 .. 2^-10: |e1 x e2| straddles the epsilon of a unit ray
    n = 512
    c = 0.5 + rng.random((n, 3)) * (ROOM - 1.0)
    e1 = _unit_rows(rng, n) * (2.0 ** rng.uniform(-13.0, -10.0, n))[:, None]
    e2 = _unit_rows(rng, n) * (2.0 ** rng.uniform(-13.0, -10.0, n))[:, None]
    s.add(np.stack([c, c + e1, c + e2], axis=1), _GREEN)
    # two room-spanning triangles: large and tiny edges meet in one leaf
    s.add([[(0.5, 0.5, 0.5), (9.5, 0.7, 9.3), (0.6, 5.5, 9.4)], [(9.4, 0.4, 0.6), (0.4, 5.6, 0.7), (9.6, 5.4, 9.5)]],
          _WHITE)
    # lights: an 8 x 8 panel under the ceiling, an emissive sliver, an emissive point (light surface 0)
    s.add(_grid((3.5, 5.9, 3.5), (3.0, 0, 0), (0, 0, 3.0), 8, 8), (0.78, 0.78, 0.78), ke=(17.0, 12.0, 4.0),
          hint=(0, -1, 0))
    s.add([[(1.0, 4.0, 1.0), (3.0, 4.2, 1.5), (1.0, 4.0 - 1e-3, 1.0)]], (0.78, 0.78, 0.78), ke=(9.0, 9.0, 9.0),
          hint=(0, -1, 0))
    s.add([[(8.0, 4.5, 8.0), (8.0, 4.5, 8.0), (8.5, 4.5, 8.5)]], (0.78, 0.78, 0.78), ke=(5.0, 5.0, 5.0),
          hint=(0, -1, 0))

    off = np.asarray(offset, np.float64)
    pos = (np.concatenate(s.t) + off).astype(np.float32).reshape(-1, 9)
    nrm = np.concatenate(s.n).astype(np.float32)
    n = len(pos)
    return {"pos": pos, "vnrm": np.ascontiguousarray(np.tile(nrm, (1, 3))), "uv": np.zeros((n, 6), np.float32),
            "kd": np.concatenate(s.kd).astype(np.float32), "ke": np.concatenate(s.ke).astype(np.float32),
            "tex": np.full(n, -1, np.int32), "room": np.stack([off, off + ROOM]).astype(np.float32)}


def write_obj(path, soup):
    """OBJ + MTL next to it: triangles in soup order, a usemtl wherever (kd, ke) changes."""
    from pathlib import Path
    path = Path(path)
    mat = np.concatenate([soup["kd"], soup["ke"]], axis=1)
    uniq, inv = np.unique(mat, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    mtl = []
    for i, m in enumerate(uniq):
        mtl += ["newmtl m%d" % i, "Ka 0 0 0", "Kd %.9g %.9g %.9g" % tuple(m[:3]), "Ks 0 0 0"]
        if (m[3:] > 0).any():
            mtl.append("Ke %.9g %.9g %.9g" % tuple(m[3:]))
        mtl.append("")
    path.with_suffix(".mtl").write_text("\n".join(mtl))
    face = "f -3//-3 -2//-2 -1//-1"
    v = ["v %.9g %.9g %.9g" % tuple(r) for r in soup["pos"].reshape(-1, 3).tolist()]
    vn = ["vn %.9g %.9g %.9g" % tuple(r) for r in soup["vnrm"].reshape(-1, 3).tolist()]
    out = ["mtllib " + path.with_suffix(".mtl").name]
    last = -1
    for t in range(len(inv)):
        if inv[t] != last:
            last = inv[t]
            out.append("usemtl m%d" % last)
        out += v[3 * t: 3 * t + 3]
        out += vn[3 * t: 3 * t + 3]
        out.append(face)
    path.write_text("\n".join(out) + "\n")
    return path


def pair(ca, po, scenes, directory, detail, placement, *overrides, device=True):
    """The product / oracle Pair of a torture scene, loaded through the OBJ as the product loads any scene."""
    from helpers import Pair
    soup = build(detail, PLACEMENTS[placement])
    obj = write_obj(directory / ("torture_%s_%s.obj" % (detail, placement)), soup)
    p = Pair(ca, po, scenes.config_rtc("cornell_box"), "input", str(obj), *overrides, device=device)
    p.soup = soup
    return p


class Case:
    """A torture scene's Pair, its ray set and the oracle's answers to it (computed once)."""

    def __init__(self, ca, po, scenes, directory, detail, placement, *overrides, device=True):
        self.detail, self.placement = detail, placement
        self.pair = pair(ca, po, scenes, directory, detail, placement, *overrides, device=device)
        self.soup = self.pair.soup
        self.rays = rays(self.soup, self.pair.oracle)
        self.o, self.d, self.limit, self.light = (self.rays[k] for k in ("o", "d", "limit", "light"))
        self.want = self.pair.oracle.intersect(self.o, self.d)
        self.want_occ = self.pair.oracle.intersect_shadow(self.o, self.d, self.limit, self.light)


def cameras(soup):
    """(eye, centre, up, yview): the room view, an eye exactly in the floor's plane looking along it, an
    eye exactly in the x = 0 wall's plane looking in."""
    lo = soup["room"][0].astype(np.float64)

    def at(p):
        return [float(x) for x in np.float32(lo + np.asarray(p))]

    floor = at((1.0, 0.0, 1.0))
    floor[1] = float(soup["room"][0][1])
    wall = at((0.0, 3.0, 5.0))
    wall[0] = float(soup["room"][0][0])
    la_floor = at((9.0, 0.0, 8.0))
    la_floor[1] = floor[1]
    return {"room": (at((5.0, 3.0, 0.4)), at((5.0, 2.6, 9.0)), (0.0, 1.0, 0.0), 1.0),
            "floor": (floor, la_floor, (0.0, 1.0, 0.0), 0.8),
            "wall": (wall, at((9.0, 2.5, 5.5)), (0.0, 1.0, 0.0), 1.2)}


# ------------------------------------------------------------------- rays --
def ulps(x, k):
    """float32 x moved by k ulps (k a scalar or an integer array), through zero like nextafter."""
    x = np.array(x, np.float32)
    k = np.broadcast_to(np.asarray(k, np.int64), x.shape)
    for step in range(1, int(np.abs(k).max(initial=0)) + 1):
        up, dn = k >= step, k <= -step
        x = np.where(up, np.nextafter(x, np.float32(np.inf)), np.where(dn, np.nextafter(x, np.float32(-np.inf)), x))
    return x.astype(np.float32)


def unit32(v):
    """Rows normalised in float64 and rounded: |d|^2 is within 3 * 2^-24 of 1."""
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def rays(soup, oracle, seed=7):
    """The aimed ray set of a torture scene.  Returns a dict of arrays over the rays: o, d, limit, light,
    cls (one letter a .. h), unit (the direction is meant to pass lc_unit), group (a and g: the group of
    five / the class-a ray it copies; d: the class-a ray whose hit distance it brackets; else -1), k (a: the
    ulps its component moved; d: the ulps the limit moved; g: the power of two), own (b: the triangle the ray
    lies in the plane of; d: 1 where the light id is the hit triangle; e: 1 where the origin is exactly on
    a split plane of the axis the ray runs along; f: the exponent of the tiny component, 0 for the
    subnormal and signed-zero rays)."""
    rng = np.random.default_rng(seed)
    P = soup["pos"].reshape(-1, 3, 3).astype(np.float64)
    ntri = len(P)
    room = soup["room"].astype(np.float64)
    e = oracle.kd_export()
    blo, bhi = e["box"][:3].astype(np.float64), e["box"][3:].astype(np.float64)
    diag = float(np.linalg.norm(bhi - blo))
    ids, _ = oracle.lights()
    area2 = np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1)
    solid = np.nonzero(area2 > 1e-9)[0]
    # the coincident quads: triangles whose three vertices equal those of the next-but-one
    twin = np.nonzero((soup["pos"][:-2] == soup["pos"][2:]).all(axis=1))[0]
    parts = []

    def inside(n, margin=0.05):
        return (room[0] + margin + rng.random((n, 3)) * (room[1] - room[0] - 2 * margin)).astype(np.float32)

    def put(cls, o, d, unit, group=None, k=None, own=None, limit=None, light=None):
        n = len(o)
        fill = lambda a, v: np.full(n, v, np.int64) if a is None else np.asarray(a, np.int64)
        parts.append({"cls": np.full(n, cls), "o": np.asarray(o, np.float32), "d": np.asarray(d, np.float32),
                      "unit": np.broadcast_to(np.asarray(unit, bool), (n,)).copy(), "group": fill(group, -1),
                      "k": fill(k, 0), "own": fill(own, -1),
                      "limit": (rng.random(n) * diag).astype(np.float32) if limit is None else np.asarray(limit, np.float32),
                      "light": ids[rng.integers(0, len(ids), n)].astype(np.uint32) if light is None
                      else np.asarray(light, np.uint32)})

    # a. aimed at a vertex or a point of an edge, one direction component moved by -2 .. +2 ulps
    ng = 1024
    tri = rng.choice(solid, ng)
    tri[: ng // 4] = rng.choice(twin, ng // 4)  # (edges of the coincident quads: equal t on both copies)
    c0 = rng.integers(0, 3, ng)
    s = np.where(rng.random(ng) < 1.0 / 3.0, 0.0, rng.random(ng))  # a third at the vertex itself
    target = P[tri, c0] + s[:, None] * (P[tri, (c0 + 1) % 3] - P[tri, c0])
    oa = inside(ng)
    da = unit32(target - oa.astype(np.float64))
    comp = np.argmax(np.abs(da) * rng.random((ng, 3)), axis=1)  # a random non-zero component
    shift = np.tile(np.arange(-2, 3), ng)
    o5, d5 = np.repeat(oa, 5, axis=0), np.repeat(da, 5, axis=0)
    rows = np.arange(5 * ng)
    d5[rows, np.repeat(comp, 5)] = ulps(d5[rows, np.repeat(comp, 5)], shift)
    put("a", o5, d5, True, group=np.repeat(np.arange(ng), 5), k=shift)
    want_a = oracle.intersect(o5, d5)

    # b. origins in a triangle's plane (0, +-1, +-4 ulps off it), directions in the plane towards the
    #    centroid or crossing it there at 1e-7 .. 1e-3 rad
    n = 1024
    tri = rng.choice(solid, n)
    nrm = np.cross(P[tri, 1] - P[tri, 0], P[tri, 2] - P[tri, 0])
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    cen = P[tri].mean(axis=1)
    u = P[tri, 0] - cen
    u /= np.linalg.norm(u, axis=1)[:, None]
    turn = rng.random(n) * 2 * np.pi
    u = np.cos(turn)[:, None] * u + np.sin(turn)[:, None] * np.cross(nrm, u)
    back = 0.05 + 1.5 * rng.random(n) ** 2
    theta = np.where(rng.random(n) < 0.25, 0.0, 10.0 ** rng.uniform(-7.0, -3.0, n)) * rng.choice([-1.0, 1.0], n)
    ob = (cen - back[:, None] * u + (back * np.tan(theta))[:, None] * nrm).astype(np.float32)
    dom = np.argmax(np.abs(nrm), axis=1)
    rows = np.arange(n)
    ob[rows, dom] = ulps(ob[rows, dom], rng.choice([0, 0, 1, -1, 4, -4], n))
    towards = rng.random(n) < 0.5  # from the rounded origin at the centroid, or the planned direction
    db = np.where(towards[:, None], cen - ob.astype(np.float64), np.cos(theta)[:, None] * u - np.sin(theta)[:, None] * nrm)
    put("b", ob, unit32(db), True, own=tri)

    # c. surface starts: a vertex; a point of an axis-aligned triangle with the plane's coordinate exact;
    #    p + 0.001 n in float as the path tracer leaves a hit
    n = 1024
    tri = rng.choice(solid, n)
    flat = np.nonzero(((soup["pos"].reshape(-1, 3, 3)[:, 0] == soup["pos"].reshape(-1, 3, 3)[:, 1]) &
                       (soup["pos"].reshape(-1, 3, 3)[:, 0] == soup["pos"].reshape(-1, 3, 3)[:, 2])).any(axis=1)
                      & (area2 > 1e-9))[0]
    third = n // 3
    tri[third: 2 * third] = rng.choice(flat, third)
    bx = rng.random(n)
    by = rng.random(n) * (1.0 - bx)
    A, B, C = (soup["pos"].reshape(-1, 3, 3)[tri, i] for i in range(3))
    f32 = np.float32
    bz = (f32(1.0) - bx.astype(f32) - by.astype(f32)).astype(f32)
    p = ((A * bz[:, None]).astype(f32) + (B * bx.astype(f32)[:, None]).astype(f32)).astype(f32)
    p = (p + (C * by.astype(f32)[:, None]).astype(f32)).astype(f32)
    oc = p.copy()
    oc[:third] = A[:third]
    same = (A == B) & (A == C)  # (the exact plane coordinate of the axis-aligned third: already A's)
    oc[third: 2 * third] = np.where(same[third: 2 * third], A[third: 2 * third], p[third: 2 * third])
    vn = soup["vnrm"].reshape(-1, 3, 3)[tri]
    mn = (((vn[:, 0] + vn[:, 1]).astype(f32) + vn[:, 2]).astype(f32) / f32(3.0)).astype(f32)
    oc[2 * third:] = (p[2 * third:] + (mn[2 * third:] * f32(0.001)).astype(f32)).astype(f32)
    put("c", oc, unit32(rng.normal(size=(n, 3))), True, own=tri)

    # e. exact axis directions: origins on split planes, in the wall planes, on the padded box's faces
    n = 768
    oe = inside(n)
    ax = rng.integers(0, 3, n)
    rows = np.arange(n)
    inner = np.nonzero(e["is_leaf"] == 0)[0]
    pick = rng.choice(inner, n // 2)
    ax[: n // 2] = e["axis"][pick]
    oe[rows[: n // 2], ax[: n // 2]] = e["split"][pick]
    q = n // 2 + n // 4
    side = rng.integers(0, 2, n)
    oe[rows[n // 2: q], ax[n // 2: q]] = soup["room"][side[n // 2: q], ax[n // 2: q]]
    oe[rows[q:], ax[q:]] = e["box"].reshape(2, 3)[side[q:], ax[q:]]
    along = rng.random(n) < 2.0 / 3.0
    along[q:] = True
    run = np.where(along, ax,  # the axis the ray runs along
                   (ax + 1 + rng.integers(0, 2, n)) % 3)
    de = np.zeros((n, 3), np.float32)
    de[rows, run] = rng.choice([-1.0, 1.0], n)
    on_split = np.zeros(n, np.int64)
    on_split[: n // 2] = along[: n // 2]
    put("e", oe, de, True, own=on_split)

    # f. unit directions with one or two components of 2^-45 .. 2^-38 (the short division's guard is
    #    2^-40), subnormal components and -0.0
    n = 1024
    ex = rng.integers(-45, -37, n)
    ex[768:] = 0
    tiny = np.where(ex != 0, 2.0 ** ex.astype(np.float64), np.where(np.arange(n) < 896, 1e-40, -0.0))
    tiny = tiny * np.where(np.arange(n) < 896, rng.choice([-1.0, 1.0], n), 1.0)
    two = rng.random(n) < 0.3
    phi = rng.random(n) * 2 * np.pi
    rest = np.stack([np.cos(phi), np.sin(phi)], axis=1)
    rest[two] = np.stack([np.sign(np.cos(phi[two])), tiny[two]], axis=1)
    first = rng.integers(0, 3, n)
    df = np.zeros((n, 3))
    rows = np.arange(n)
    df[rows, first] = tiny
    df[rows, (first + 1) % 3] = rest[:, 0]
    df[rows, (first + 2) % 3] = rest[:, 1]
    put("f", inside(n), df.astype(np.float32), True, own=ex)

    # g. class a scaled exactly by 2^k: not unit, so the leaf cull is bypassed
    n = 1024
    src = rng.choice(5 * ng, n, replace=False)
    kk = rng.integers(-20, 21, n)
    kk[kk == 0] = 7
    put("g", o5[src], (d5[src].astype(np.float64) * 2.0 ** kk[:, None]).astype(np.float32), False, group=src, k=kk)

    # h. origins three diagonals outside, aimed into the box
    n = 256
    centre = 0.5 * (blo + bhi)
    oh = (centre + 3.0 * diag * _unit_rows(rng, n)).astype(np.float32)
    put("h", oh, unit32(inside(n).astype(np.float64) - oh.astype(np.float64)), True,
        limit=((3.0 + rng.uniform(-0.7, 0.7, n)) * diag).astype(np.float32))  # (around the distance to the room)

    # d. the class-a rays the oracle hits, limit = its dist moved by -2 .. +2 ulps; the light id is the
    #    hit triangle for half of them and another light for the rest
    hits = np.nonzero(want_a["hit"] == 1)[0]
    base = rng.choice(hits, min(1536, len(hits)), replace=False)
    own = rng.random(len(base)) < 0.5
    other = ids[rng.integers(0, len(ids), len(base))]
    clash = other == want_a["tri"][base]
    other[clash] = np.where(ids[0] == want_a["tri"][base][clash], ids[1], ids[0])
    light = np.where(own, want_a["tri"][base], other)
    shift = np.tile(np.arange(-2, 3), len(base))
    put("d", np.repeat(o5[base], 5, axis=0), np.repeat(d5[base], 5, axis=0), True, group=np.repeat(base, 5), k=shift,
        own=np.repeat(own, 5), limit=ulps(np.repeat(want_a["dist"][base], 5), shift), light=np.repeat(light, 5))

    out = {key: np.ascontiguousarray(np.concatenate([p[key] for p in parts])) for key in parts[0]}
    order = np.argsort(out["cls"], kind="stable")  # class-sorted: a .. h
    out = {key: np.ascontiguousarray(v[order]) for key, v in out.items()}
    # positions of the class-a rays in the sorted set (a sorts first and keeps its order)
    assert (out["cls"][: 5 * ng] == "a").all()
    assert np.isfinite(out["o"]).all() and np.isfinite(out["d"]).all() and np.isfinite(out["limit"]).all()
    dn = (out["d"].astype(np.float64) ** 2).sum(axis=1)
    assert (np.abs(dn[out["unit"]] - 1.0) <= 12.0 * U24).all()  # lc_unit's window: the cull really runs
    assert (np.abs(dn[~out["unit"]] - 1.0) > 12.0 * U24).all()
    return out


# ------------------------------------------------------------ brute force --
TOL = 1e-3


def brute_force(soup, o, d, chunk=32):
    """Nearest accepted triangle of every ray over ALL triangles in float64, by the reference's acceptance
    (|a| >= EPS, u, v, 1 - u - v >= 0, t >= 0), and whether the ray is clear-cut, so that an evaluation in
    float32 along any traversal must find the same triangle.

    A triangle is safely in when |a| > EPS + 1e-8 and u, v, 1 - u - v and t all exceed TOL; safely out when
    |a| < EPS - 1e-8 (degenerate for this ray: left out of the boundary test) or one of u, v, 1 - u - v, t
    is below -TOL; anything else is within TOL of a decision boundary.  A ray is clear-cut when no triangle
    near a boundary has t below the winner's (1 + TOL) -- none at all on a miss -- and the runner-up
    is at least TOL (relative) behind.
    Returns hit, tri, t, clear and, for the distance bound, S, g, cb of the winner."""
    P = soup["pos"].reshape(-1, 3, 3).astype(np.float64)
    A = P[:, 0]
    e1, e2 = P[:, 1] - A, P[:, 2] - A
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    n = len(o)
    res = {"hit": np.zeros(n, np.uint32), "tri": np.zeros(n, np.uint32), "t": np.full(n, np.inf),
           "clear": np.zeros(n, bool)}
    ex1, ey1, ez1 = e1.T[:, None, :]
    ex2, ey2, ez2 = e2.T[:, None, :]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i in range(0, n, chunk):
            dx, dy, dz = (d[i: i + chunk].T)[:, :, None]
            sx, sy, sz = (o[i: i + chunk, None, :] - A[None, :, :]).transpose(2, 0, 1)
            px, py, pz = dy * ez2 - dz * ey2, dz * ex2 - dx * ez2, dx * ey2 - dy * ex2
            a = ex1 * px + ey1 * py + ez1 * pz
            u = (sx * px + sy * py + sz * pz) / a
            qx, qy, qz = sy * ez1 - sz * ey1, sz * ex1 - sx * ez1, sx * ey1 - sy * ex1
            v = (dx * qx + dy * qy + dz * qz) / a
            t = (ex2 * qx + ey2 * qy + ez2 * qz) / a
            w = 1.0 - u - v
            lowest = np.minimum(np.minimum(u, v), np.minimum(w, t))
            big = np.abs(a)
            acc = (big >= EPS) & (lowest >= 0.0)
            safe_in = (big > EPS + 1e-8) & (lowest > TOL)
            safe_out = (big < EPS - 1e-8) | (lowest < -TOL)
            near = ~safe_in & ~safe_out  # (NaN from a == 0 compares false everywhere: big < EPS - 1e-8 holds)
            ta = np.where(acc, t, np.inf)
            two = np.partition(ta, 1, axis=1)[:, :2]
            win = np.argmin(ta, axis=1)
            tw, second = two[:, 0], two[:, 1]
            hit = np.isfinite(tw)
            lim = np.where(hit, tw * (1.0 + TOL), np.inf)
            bad = (near & (t <= lim[:, None])).any(axis=1)
            rows = np.arange(len(win))
            clear = ~bad & (~hit | (safe_in[rows, win] & (second >= tw * (1.0 + TOL))))
            sl = slice(i, i + chunk)
            res["hit"][sl], res["tri"][sl], res["t"][sl], res["clear"][sl] = hit, win, tw, clear
    tri = res["tri"]
    nrm = np.cross(e1[tri], e2[tri])
    ln = np.linalg.norm(nrm, axis=1)
    E = np.abs(e1[tri]).sum(axis=1) + np.abs(e2[tri]).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        res["g"] = E * E / ln
        res["cb"] = np.abs((d * nrm).sum(axis=1)) / (ln * np.linalg.norm(d, axis=1))
    res["S"] = np.abs(o[:, None, :] - P[tri]).max(axis=(1, 2))
    return res


def dist_bound(bf):
    """leafcull.hpp's bound on the float evaluation's distance: 10.05 u (S + t) g / cb + 2.1 u t."""
    return 10.05 * U24 * (bf["S"] + bf["t"]) * bf["g"] / bf["cb"] + 2.1 * U24 * bf["t"]
