"""Reading and comparing the reference-pinned fixtures G1-G4 (a helper module, not a conftest).

tests/golden/ref_scene_<name>.npz   G1: a triangle soup (OracleScene's arrays, floats as uint32 bit patterns), its
                                    textures and leaf size, and what the reference's own KDTree constructor made
                                    of it: the tree in pre-order, the padded root box, the light list
tests/golden/ref_rays_<name>.npz    G2: closest and shadow rays with KDTree::intersectRay / intersectShadowRay's
                                    answers
tests/golden/ref_brdf.npz           G3: Diffuse::sample_wi, uniformFloat, Scene::randomLight on scripted words
tests/golden/ref_paths.npz          G4: RayTracer::sendRay per (pixel, sample): the camera ray, the radiance and
                                    the words consumed

All of them are written by tests/golden/make_ref_golden.py from the reference's compiled objects (oracle/ref).
Nothing here needs the reference or the generator: the inputs are stored with the outputs.

Run as a program (python tests/refpin.py <what>) it compares the oracle that pyoracle loads -- the library in
CHIARO_ORACLE_DIR, which is how the must-fail variants of oracle.c are checked -- with the fixtures and prints
the number of differing cases as one JSON line.
"""
from __future__ import annotations

import io
import json
import sys
import zipfile
from pathlib import Path

import numpy as np

GOLD = Path(__file__).resolve().parent / "golden"
U32, F32 = np.uint32, np.float32
SOUP_FLOATS = ("pos", "vnrm", "uv", "kd", "ke")
TREE_KEYS = ("is_leaf", "axis", "split", "count", "refs")
# G1 scenes (file names); G4 cases -> the scene each renders
SCENES = ("cornell_l1", "cornell_l2", "cornell_l8", "textured", "ident24", "onplane", "negative", "nolight",
          "torture_mini")
PATH_CASES = {"cornell": "cornell_l8", "textured": "textured", "cornell_k1": "cornell_l8", "nolight": "nolight"}
RAY_CLASSES = ("camera", "interior", "zero_component", "on_split", "on_triangle", "outside", "equal_t", "torture")
SHADOW_CLASSES = ("random", "at_t", "below_t", "above_t", "at_t_own_light", "torture")


def f32(b):
    return np.ascontiguousarray(b, U32).view(F32)


def bits(x):
    return np.ascontiguousarray(x, F32).view(U32)


def save_npz(path, arrays: dict):
    """A compressed .npz whose bytes depend on the arrays alone (np.savez stamps the time of day)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), version=(1, 0), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                       compress_type=zipfile.ZIP_DEFLATED, compresslevel=9)


def _as_bits(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a, F32).view(U32) if a.dtype.kind == "f" else np.ascontiguousarray(a, U32)


def same_bits(a, b):
    """Mask of differing float32 bit patterns (each side given as floats or as uint32 patterns); a NaN on both
    sides counts as equal."""
    a, b = _as_bits(a), _as_bits(b)
    return (a != b) & ~(np.isnan(a.view(F32)) & np.isnan(b.view(F32)))


# ---------------------------------------------------------------- scenes --
class GoldenScene:
    def __init__(self, name):
        self.name = name
        z = np.load(GOLD / ("ref_scene_%s.npz" % name))
        self.soup = {k: f32(z[k]) for k in SOUP_FLOATS}
        self.soup["tex"] = z["tex"].astype(np.int32)
        self.leaf_size = int(z["leaf_size"][0])
        self.textures = []
        for i in range(len(z["tex_shapes"])):
            w, h, nc = (int(v) for v in z["tex_shapes"][i])
            self.textures.append((w, h, nc, z["tex%d" % i].astype(np.uint8)))
        self.tree = {k: z[k].astype(U32) for k in TREE_KEYS}
        self.box = z["box"].astype(U32)
        self.light_ids = z["light_ids"].astype(U32)
        self.light_surface = z["light_surface"].astype(U32)
        self.view = f32(z["view"])  # eye3, centre3, up3, yview

    @property
    def ntri(self):
        return len(self.soup["pos"])

    def oracle(self, po, threads=1):
        return po.OracleScene(self.soup, leaf_size=self.leaf_size, textures=self.textures, build_threads=threads)


def preorder(e) -> dict:
    """A child-indexed kd export (OracleScene.kd_export / KDTree.export) in the fixtures' pre-order form: node,
    then the subtree of child, then that of child + 1; leaves carry count and their ids in order."""
    out = {k: [] for k in TREE_KEYS}
    split = bits(e["split"])
    stack = [0]
    while stack:
        i = stack.pop()
        leaf = int(e["is_leaf"][i])
        out["is_leaf"].append(leaf)
        if leaf:
            first, n = int(e["leaf_first"][i]), int(e["leaf_count"][i])
            out["axis"].append(3)
            out["split"].append(0)
            out["count"].append(n)
            out["refs"].extend(e["refs"][first: first + n].tolist())
        else:
            out["axis"].append(int(e["axis"][i]))
            out["split"].append(int(split[i]))
            out["count"].append(0)
            stack += [int(e["child"][i]) + 1, int(e["child"][i])]
    return {k: np.array(v, U32) for k, v in out.items()}


def tree_differences(got: dict, gs: GoldenScene, box) -> list:
    bad = [k for k in TREE_KEYS if not np.array_equal(got[k], gs.tree[k])]
    if not np.array_equal(bits(box), gs.box):
        bad.append("box")
    return bad


# ------------------------------------------------- scenes as the product loads them --
def write_scene(directory, gs: GoldenScene) -> Path:
    """The soup as OBJ + MTL (+ one binary PPM / PGM per texture) that the product's loader reads back float for
    float: %.9g coordinates, explicit vn and vt on every corner (vt's v stored flipped: the loader applies
    assimp's FlipUVs), one usemtl run wherever (kd, ke, tex) changes, in soup order."""
    directory = Path(directory)
    directory.mkdir(parents=True, exist_ok=True)
    s = gs.soup
    mat = np.concatenate([bits(s["kd"]), bits(s["ke"]), s["tex"].astype(U32)[:, None]], axis=1)
    uniq, inv = np.unique(mat, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    mtl = []
    for i, m in enumerate(uniq):
        kd, ke, tex = f32(m[:3]), f32(m[3:6]), int(np.int32(m[6]))
        mtl += ["newmtl m%d" % i, "Ka 0 0 0", "Kd %.9g %.9g %.9g" % tuple(kd.tolist()), "Ks 0 0 0"]
        if (ke > 0).any():
            mtl.append("Ke %.9g %.9g %.9g" % tuple(ke.tolist()))
        if tex >= 0:
            mtl.append("map_Kd %s_tex%d.pnm" % (gs.name, tex))
        mtl.append("")
    obj = directory / (gs.name + ".obj")
    obj.with_suffix(".mtl").write_text("\n".join(mtl))
    for i, (w, h, nc, data) in enumerate(gs.textures):
        assert nc in (1, 3)
        (directory / ("%s_tex%d.pnm" % (gs.name, i))).write_bytes(
            b"P%d\n%d %d\n255\n" % (6 if nc == 3 else 5, w, h) + np.ascontiguousarray(data, np.uint8).tobytes())
    uv = s["uv"].reshape(-1, 2).astype(F32)
    flipped = (F32(1.0) - uv[:, 1]).astype(F32)
    assert np.array_equal(bits((F32(1.0) - flipped).astype(F32)), bits(uv[:, 1])), "uv.v does not survive FlipUVs"
    v = ["v %.9g %.9g %.9g" % tuple(r) for r in s["pos"].reshape(-1, 3).tolist()]
    vn = ["vn %.9g %.9g %.9g" % tuple(r) for r in s["vnrm"].reshape(-1, 3).tolist()]
    vt = ["vt %.9g %.9g" % (a, b) for a, b in zip(uv[:, 0].tolist(), flipped.tolist())]
    out = ["mtllib " + obj.with_suffix(".mtl").name]
    last = -1
    for t in range(len(inv)):
        if inv[t] != last:
            last = inv[t]
            out.append("usemtl m%d" % last)
        out += v[3 * t: 3 * t + 3] + vn[3 * t: 3 * t + 3] + vt[3 * t: 3 * t + 3]
        out.append("f -3/-3/-3 -2/-2/-2 -1/-1/-1")
    obj.write_text("\n".join(out) + "\n")
    return obj


def write_rtc(scenes, directory, gs: GoldenScene, obj, **kv) -> Path:
    """The scene's .rtc from scenes.config_rtc (the Cornell config's tokens with this scene's on top)."""
    e, c, u, yv = gs.view[0:3], gs.view[3:6], gs.view[6:9], gs.view[9]
    fmt = lambda v: " ".join("%.9g" % x for x in v.tolist())
    rtc = scenes.config_rtc("cornell", Path(directory), input=obj, kdtree_leaf_size=gs.leaf_size, VP=fmt(e),
                            LA=fmt(c), UP=fmt(u), yview="%.9g" % yv, **kv)
    out = Path(directory) / (gs.name + ".rtc")
    out.write_text(rtc.read_text())
    return out


class Loaded:
    """The fixture scene as the product loads it from OBJ; its triangles, textures and leaf size are asserted
    to be the fixture's, so triangle ids and every float mean the same on both sides."""

    def __init__(self, ca, scenes, directory, gs: GoldenScene, **kv):
        self.gs = gs
        self.scene = ca.Scene(write_rtc(scenes, directory, gs, write_scene(directory, gs), **kv))
        self.info = self.scene.info
        self.model = ca.Model(self.scene)
        t = self.model.triangles()
        assert self.model.num_triangles == gs.ntri and self.info["leaf_size"] == gs.leaf_size
        for k in SOUP_FLOATS:
            assert np.array_equal(bits(t[k]).reshape(-1), bits(gs.soup[k]).reshape(-1)), (gs.name, k)
        assert np.array_equal(t["tex"], gs.soup["tex"])
        tex = self.model.textures()
        assert [(w, h, nc) for w, h, nc, _ in tex] == [(w, h, nc) for w, h, nc, _ in gs.textures]
        assert all(np.array_equal(a[3], b[3]) for a, b in zip(tex, gs.textures))


# ------------------------------------------------------------------- rays --
def load_rays(name) -> dict:
    z = np.load(GOLD / ("ref_rays_%s.npz" % name))
    r = {k: z[k] for k in z.files}
    for k in ("o", "d", "so", "sd", "slimit"):
        r[k] = f32(r[k])
    return r


def closest_differences(got: dict, r: dict) -> np.ndarray:
    """Per ray: the hit flag differs, or on a golden hit the triangle, either barycentric or the distance."""
    hit = r["hit"] == 1
    bad = got["hit"] != r["hit"]
    bad |= hit & (got["tri"] != r["tri"])
    bad |= hit & same_bits(got["bary"], r["bary"]).reshape(-1, 2).any(axis=1)
    bad |= hit & same_bits(got["dist"], r["dist"])
    return bad


# ------------------------------------------------------------------- brdf --
def load_brdf() -> dict:
    """{"sample_wi": [record, ...], "uniform": [...], "index": [...]}: each record a dict of Python ints (float
    fields as bit patterns) and lists of them, from the per-field uint32 arrays of ref_brdf.npz."""
    z = np.load(GOLD / "ref_brdf.npz")
    out = {}
    for key in z.files:
        table, field = key.split("/")
        out.setdefault(table, {})[field] = z[key].tolist()
    return {t: [dict(zip(f, row)) for row in zip(*f.values())] for t, f in out.items()}


# ------------------------------------------------------------------ paths --
def load_paths() -> dict:
    z = np.load(GOLD / "ref_paths.npz")
    out = {}
    for case in PATH_CASES:
        m = z[case + "/meta"]
        out[case] = {"xres": int(m[0]), "yres": int(m[1]), "spp": int(m[2]), "k": int(m[3]), "seed": int(m[4]),
                     "layers": int(m[5]), "bg": f32(z[case + "/bg"]), "cam": f32(z[case + "/cam"]),
                     "rad": z[case + "/rad"].astype(U32), "dir": z[case + "/dir"].astype(U32),
                     "words": z[case + "/words"].astype(U32)}
    return out


def blend_frames(c: dict) -> list:
    """The frames after layer 1, 2, ... as src/rayTracer.cpp:58-64 makes them of the per-sample radiances: the
    samples summed in order in float32 from zero, times 1 / spp, blended (old * (L - 1) + mean) / L."""
    rad = f32(c["rad"])  # [layer][y][x][sample][3]
    inv = F32(1.0) / F32(c["spp"])
    frames, old = [], np.zeros(rad.shape[1:3] + (3,), F32)
    with np.errstate(all="ignore"):
        for li in range(c["layers"]):
            temp = np.zeros_like(old)
            for s in range(c["spp"]):
                temp = (temp + rad[li, :, :, s]).astype(F32)
            L = F32(li + 1)
            old = (((old * F32(li)).astype(F32) + (temp * inv).astype(F32)).astype(F32) / L).astype(F32)
            frames.append(old.copy())
    return frames


# --------------------------------------------- the oracle against the fixtures --
def oracle_tree_cases(po) -> dict:
    out = {}
    for name in SCENES:
        gs = GoldenScene(name)
        for threads in (1, 4):
            osc = gs.oracle(po, threads)
            e = osc.kd_export()
            ids, surf = osc.lights()
            bad = tree_differences(preorder(e), gs, e["box"])
            if not (np.array_equal(ids, gs.light_ids) and np.array_equal(bits(surf), gs.light_surface)):
                bad.append("lights")
            out["%s/threads%d" % (name, threads)] = bad
    return out


def oracle_ray_cases(po) -> dict:
    """{"closest": differing rays, "shadow": differing rays, "n": rays compared} over every G2 file."""
    res = {"closest": 0, "shadow": 0, "n": 0, "by_scene": {}}
    for name in SCENES:
        gs, r = GoldenScene(name), load_rays(name)
        osc = gs.oracle(po)
        c = int(closest_differences(osc.intersect(r["o"], r["d"]), r).sum())
        s = int((osc.intersect_shadow(r["so"], r["sd"], r["slimit"], r["slight"]) != r["occ"]).sum())
        res["closest"] += c
        res["shadow"] += s
        res["n"] += len(r["o"]) + len(r["so"])
        res["by_scene"][name] = [c, s]
    return res


def oracle_brdf_cases(po) -> dict:
    import devmath_cases as dc
    g = load_brdf()
    res = {"sample_wi": 0, "uniform": 0, "index": 0, "n": 0}
    for c in g["sample_wi"]:
        sx = po.rng_uniform_kat(dc.unmix32(c["words"][0]), 0, -1.0, 1.0)
        sy = po.rng_uniform_kat(dc.unmix32(c["words"][1]), 0, -1.0, 1.0)
        wi, pdf = po.sample_wi(f32(c["n"]), f32([c["sx"]])[0], f32([c["sy"]])[0])
        f = (F32(0.31830988618379067154) * f32(c["color"])).astype(F32)
        bad = [dc.b1(sx[0]), dc.b1(sy[0])] != [c["sx"], c["sy"]] or sx[1] != 1 or sy[1] != 1 or c["consumed"] != 2
        bad = bad or same_bits(np.append(wi, F32(pdf)), c["wi"] + [c["pdf"]]).any() or same_bits(f, c["f"]).any()
        res["sample_wi"] += bool(bad)
    for c in g["uniform"]:
        key = dc.unmix32(c["word"])
        val, ctr = po.rng_uniform_kat(key, 0, f32([c["a"]])[0], f32([c["b"]])[0])
        res["uniform"] += bool(same_bits([dc.b1(val)], [c["out"]]).any() or ctr != c["consumed"])
    for c in g["index"]:
        assert dc.raw_draws(c["key"], 0, len(c["words"])) == c["words"]  # (the stream's definition: ours)
        val, ctr = po.rng_index_kat(c["key"], 0, c["n"])
        res["index"] += (val, ctr) != (c["index"], c["consumed"])
    res["n"] = len(g["sample_wi"]) + len(g["uniform"]) + len(g["index"])
    return res


def oracle_path_cases(po) -> dict:
    res = {"radiance": 0, "words": 0, "n": 0}
    scenes = {}
    for case, c in load_paths().items():
        name = PATH_CASES[case]
        if name not in scenes:
            scenes[name] = GoldenScene(name).oracle(po)
        osc = scenes[name]
        for li in range(c["layers"]):
            for y in range(c["yres"]):
                for x in range(c["xres"]):
                    for s in range(c["spp"]):
                        rad, words = osc.path_words(c["cam"], c["xres"], c["yres"], c["k"], c["bg"], c["seed"],
                                                    li + 1, x, y, s)
                        res["radiance"] += bool(same_bits(rad, c["rad"][li, y, x, s]).any())
                        res["words"] += words != int(c["words"][li, y, x, s])
                        res["n"] += 1
    return res


if __name__ == "__main__":
    sys.path[:0] = [str(Path(__file__).resolve().parents[1] / "oracle"), str(Path(__file__).resolve().parent)]
    import pyoracle
    what = {"rays": oracle_ray_cases, "brdf": oracle_brdf_cases, "paths": oracle_path_cases,
            "tree": oracle_tree_cases}[sys.argv[1]]
    print(json.dumps(what(pyoracle)))
