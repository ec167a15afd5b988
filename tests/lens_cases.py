"""Cases and expected images shared by tests/test_lens_host.py and tests/test_lens_gpu.py.

A *case* is (scene, NTRACER_* switches, variant, lens name): a golden scene of ray_color_cases (or "box<n>" for BoxScene(n))
rendered through one of LENSES.  The expected colour of a pixel is the oracle's colour of its ray: `Lens.directions(camera)`
gives the unnormalised v of every pixel in fp32, and a ray (o, v) is the centre pixel of a 2 x 2 view of a camera at o with
forward row v (ray_color_cases.CentrePixel; test_lens_host.py pins the method through the pinhole lens).  Masked pixels are
(0, 0, 0).  No oracle entry was added.

No case may pass on background: through every lens of ORACLE_LENSES the oracle alone must find MIN_OPAQUE pixels with an
opaque hit (BoxScene: MIN_BOX_HITS cube pixels) and, in the scenes with transparent materials, MIN_TRANSPARENT pixels with a
transparent hit.  The golden cameras stand 2 to 4 scene sizes away -- right for the pinhole of 0.8 rad they were captured
with, while a view 3 rad or a whole sphere wide at 37 x 29 sees the scene in a handful of pixels (8 of 1 073 for the 600-cell,
none for the 10-simplex).  VIEWS therefore names, per scene, one golden camera with its ORIENTATION kept and its origin moved
towards the centre c of the scene's box, o' = c + (o - c) * s, and the image size -- 37 x 29 but for the 10-simplex, which is
thin in ten dimensions and needs the 64 x 48 pixels to show 25 hits.  The floors themselves are as asked; `python
tests/lens_cases.py` prints what the oracle finds.  Everything is computed once per process and never modified afterwards."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (run as a script: the package beside tests/)

import fixtures as fx
import ray_color_cases as rc
import ray_query_cases as rq
import support as sup
from ntracer_amd import tracern

f32 = np.float32
W, H = 37, 29                      # a multiple of neither 8 nor 16
FOV = 0.8                          # of the plain renders the pinhole lens is compared with

STRICT, CLEAN, VAR = rc.STRICT, rc.CLEAN, rc.VAR
PLAIN = {"NTRACER_COMPOSITE_KERNEL": "2"}
SWITCHES = rc.SWITCHES + ("NTRACER_COMPOSITE_KERNEL",)


def _fisheye_circle(w, h):
    """the fisheye of 3.0 rad as a circular image: Lens.fisheye's table with the pixels outside the circle of radius w / 2 -- where
    the angle passes fov / 2 -- masked.  (The constructor itself masks beyond pi, which 3.0 rad across 37 pixels never reaches.)"""
    c = tracern.Lens.fisheye(w, h, 3.0).coeffs
    u, v = np.arange(w)[None, :] - w / 2.0, np.arange(h)[:, None] - h / 2.0
    c[np.hypot(u, v) > w / 2.0] = 0.0
    return tracern.Lens(w, h, c)


LENSES = {
    "pinhole": lambda w, h: tracern.Lens.pinhole(w, h, FOV),
    "fisheye": _fisheye_circle,                                             # fov 3.0, masked corners
    "fisheye_open": lambda w, h: tracern.Lens.fisheye(w, h, 3.0),            # ... as the constructor leaves it: no pixel masked
    "equirect": lambda w, h: tracern.Lens.equirectangular(w, h),
    "cylindrical": lambda w, h: tracern.Lens.cylindrical(w, h, 3.0),
}
ORACLE_LENSES = ("fisheye", "equirect")

SCENES = [
    ("cell600_n4", {}, ""),            # lean: the packet walk, lens_shade<N,false,false>
    ("cell600_n4", {}, "lit"),         # lights, shadows, reflection: lens_shade<N,true,false>
    ("simplex10_n10", {}, ""),         # loose triangles in the leaves (SCAL): lens_shade<N,true,true>
    ("feature5_n5", {}, ""),           # transparent materials, Solids: the ray route, rays_color_t<N,true>
    ("feature11_n11", {}, ""),         # run-time n: rays_color_var_t<true>
    ("box6", {}, ""),                  # rays_box<N>
    ("box25", {}, ""),                 # rays_box_var
]
# scene -> (golden camera, s of o' = c + (o - c) * s, image size)
VIEWS = {
    "cell600_n4": (0, 0.25, (W, H)),
    "simplex10_n10": (3, 0.25, (64, 48)),
    "feature5_n5": (0, 0.125, (W, H)),
    "feature11_n11": (2, 0.03, (W, H)),
    "box6": (0, 1.0, (W, H)),
    "box25": (4, 1.0, (W, H)),
}
# one case each under a switch, and the ray route's kernels that the scenes above do not reach
SWITCHED = [
    ("cell600_n4", STRICT, "lit", "fisheye"),
    ("feature5_n5", CLEAN, "", "equirect"),            # rays_color_t<N,false>
    ("simplex10_n10", VAR, "", "fisheye"),             # rays_color_var
    ("cell600_n4", PLAIN, "", "equirect"),             # the ray route for a scene the packet walk would take: rays_color<N,false,false>
    ("cell600_n4", PLAIN, "lit", "fisheye"),           # rays_color<N,true,false>
    ("simplex10_n10", PLAIN, "", "fisheye"),           # rays_color<N,true,true>
    ("feature11_n11", CLEAN, "", "fisheye"),           # rays_color_var_t<false>
]
ORACLE_CASES = [s + (l,) for s in SCENES for l in ORACLE_LENSES] + SWITCHED

MIN_OPAQUE, MIN_BOX_HITS = 25, 100
MIN_TRANSPARENT = {"feature5_n5": 20, "feature11_n11": 20}


def case_id(case):
    name, env, variant, lens = case
    return name + "".join("," + k[len("NTRACER_"):] for k in sorted(env)) + ("," + variant if variant else "") + "," + lens


def is_box(name):
    return name.startswith("box")


def size(name):
    return VIEWS[name][2]


@functools.lru_cache(maxsize=None)
def lens_at(lens_name, w, h):
    return LENSES[lens_name](w, h)


def lens(case):
    """the case's Lens, of its scene's image size"""
    return lens_at(case[3], *size(case[0]))


def route(case):
    """the kernels a case lands on, by the rules of enqueue_lens (nt_api.cpp): the packet walk's two passes, or the ray-colour
    kernel behind lens_expand"""
    name, env, variant, _ = case
    if is_box(name):
        return ("lens_expand", rc.box_route(int(name[3:])))
    n, flat, params = rc.case_scene((name, env, variant))
    m = np.asarray(flat["materials"])
    opaque = bool((m[:, 6] >= 1).all())
    solids = len(flat["solid_types"]) > 0
    clean = env.get("NTRACER_CLEAN_NORMALS") == "1"
    faithful = not opaque or (solids and not clean)
    var = n > 10 or env.get("NTRACER_FORCE_VAR") == "1"
    if faithful or var or env.get("NTRACER_COMPOSITE_KERNEL", "0") != "0":
        return ("lens_expand", rc.route((name, env, variant)))
    r = rc.route((name, env, variant))                      # rays_color<N,FEAT,SCAL>: the same FEAT / SCAL rules
    feat, scal = r[len("rays_color<N,"):-1].split(",")
    return ("composite_packet<N,32,false,%s,true,true>" % scal, "lens_shade<N,%s,%s>" % (feat, scal))


@functools.lru_cache(maxsize=None)
def camera(name):
    """(origin, axes) of the scene's case camera: VIEWS"""
    k, sc, _ = VIEWS[name]
    if is_box(name):
        n = int(name[3:])
        if n == 6:
            g = fx.load("box_n6_1920x1080")
            return np.asarray(g["origins"][k], f32), np.asarray(g["axes"][k], f32)
        o, q = fx.stress_cameras(n, np.random.default_rng(rc.SEED))[k]
        return np.asarray(o, f32), np.asarray(q, f32)
    g, n, flat = rq.scene(name)
    f = int(g["frames"][k])
    o, q = np.asarray(g["origins"][f], f32), np.asarray(g["axes"][f], f32)
    c = f32(0.5) * (np.asarray(g["aabb_start"], f32) + np.asarray(g["aabb_end"], f32))
    return (c + (o - c) * f32(sc)).astype(f32), q


def camera_of(o, q):
    c = tracern.Camera(len(o))
    c._origin, c._axes = np.array(o, f32), np.array(q, f32)
    return c


def _unit(v):
    return (v / np.sqrt((v * v).sum(axis=1, dtype=f32))[:, None]).astype(f32)


@functools.lru_cache(maxsize=None)
def counts(name, lens_name):
    """(opaque hits, pixels with a transparent hit) the oracle finds through the lens; BoxScene: (cube pixels, 0)"""
    o, q = camera(name)
    ln = lens_at(lens_name, *size(name))
    live = ~ln.masked.reshape(-1)
    v = ln.directions(camera_of(o, q))[live]
    if is_box(name):
        ref = rc.CentrePixel(len(o)).colors(o, v)
        return int((ref[:, 0] != ref[:, 1]).sum()), 0
    g, n, flat = rq.scene(name)
    orc = rq.Oracle(n, flat, False, len(flat["solid_types"]) == 0)
    cnt = len(v)
    none = np.full(cnt, -1, np.int32)
    r = orc.intersects(np.repeat(o[None], cnt, axis=0), _unit(v), np.full(cnt, -rq.FLT_MAX), np.full(cnt, rq.FLT_MAX), none, none)
    return int((r["item"] >= 0).sum()), int((r["n_transparent"] > 0).sum())


def check_floors(case):
    name = case[0]
    c = counts(name, case[3])
    if is_box(name):
        assert c[0] >= MIN_BOX_HITS, (case_id(case), c)
    else:
        assert c[0] >= MIN_OPAQUE and c[1] >= MIN_TRANSPARENT.get(name, 0), (case_id(case), c)
    return c


def oracle_colors(name, env, variant, o, v):
    """the oracle's colour of rays (o, v[i]), the oracle in the GPU's mode (as ray_color_cases has it)"""
    if is_box(name):
        return rc.CentrePixel(len(o)).colors(o, v)
    n, flat, params = rc.case_scene((name, env, variant))
    clean = env.get("NTRACER_CLEAN_NORMALS") == "1"
    prune = env.get("NTRACER_STRICT_REFERENCE") != "1" and len(flat["solid_types"]) == 0
    return rc.CentrePixel(n, flat, params, clean, prune).colors(o, v)


@functools.lru_cache(maxsize=None)
def _expected(name, clean, strict, variant, lens_name, cam):
    env = dict(([("NTRACER_CLEAN_NORMALS", "1")] if clean else []) + ([("NTRACER_STRICT_REFERENCE", "1")] if strict else []))
    o, q = camera(name) if cam is None else (np.frombuffer(cam[0], f32), np.frombuffer(cam[1], f32).reshape(len(cam[0]) // 4, -1))
    ln = lens_at(lens_name, *size(name))
    live = ~ln.masked.reshape(-1)
    v = ln.directions(camera_of(o, q))
    out = np.zeros((len(v), 3), f32)
    out[live] = oracle_colors(name, env, variant, np.asarray(o, f32), v[live])
    out.setflags(write=False)
    return out


def expected(case, cam=None):
    """fp32 [h * w][3]: the oracle's colour of every pixel of the case (unclamped), (0, 0, 0) where the lens is masked; `cam`:
    another camera (origin, axes) than the case's.  NTRACER_FORCE_VAR and NTRACER_COMPOSITE_KERNEL change the kernels, not the
    answers: they share the default's image."""
    name, env, variant, lens_name = case
    key = None if cam is None else (np.asarray(cam[0], f32).tobytes(), np.asarray(cam[1], f32).tobytes())
    return _expected(name, env.get("NTRACER_CLEAN_NORMALS") == "1", env.get("NTRACER_STRICT_REFERENCE") == "1", variant, lens_name, key)


def scene(case, mp):
    """the case's scene on the library, its camera set and the switches in the environment of `mp`"""
    name, env, variant = case[:3]
    sup.set_switches(mp, SWITCHES, env)
    if is_box(name):
        sc = tracern.BoxScene(int(name[3:]))
    else:
        n, flat, params = rc.case_scene((name, env, variant))
        sc = tracern.CompositeScene.from_flat(n, flat)
        sc.set_params_flat(params)
    sc.set_fov(FOV)
    o, q = camera(name)
    sc._set_camera_arrays(o, q)
    return sc


if __name__ == "__main__":
    import time
    for case in ORACLE_CASES:
        t = time.time()
        c = check_floors(case)
        e = expected(case)
        print("%-40s %dx%d %-66s %4d masked, %4d opaque hits, %4d with a transparent hit, %4d colours (%.1f s)"
              % ((case_id(case),) + size(case[0]) + (" + ".join(route(case)), int(lens(case).masked.sum())) + c + (len(np.unique(e, axis=0)), time.time() - t)))
