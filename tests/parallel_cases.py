"""Cases and expected images shared by tests/test_parallel_host.py and tests/test_parallel_gpu.py.

A *case* is (scene, NTRACER_* switches, variant): a scene of lens_cases.SCENES rendered under the parallel projection
(Scene.set_parallel_projection).  The expected colour of a pixel is the oracle's colour of its ray: `parallel_rays` below
restates the header's formula in numpy fp32 -- o' of every pixel and the forward row -- and a ray (o', forward) is the centre
pixel of a 2 x 2 view of a camera at o' with forward row `forward` (ray_color_cases.CentrePixel, which takes one origin a ray:
for pixel (1, 1) of a 2 x 2 view sx = sy = 0, so the oracle's direction is unit(forward), formed in the same order).  No
oracle entry was added.

The camera is the golden camera that lens_cases.VIEWS names for the scene, its origin NOT moved; the image is 37 x 29;
half_width is half the largest extent of the scene's box for the composite scenes and 1.5 for the boxes.  No case may pass on
background: the oracle alone must find MIN_OPAQUE pixels with an opaque hit (BoxScene: MIN_BOX_HITS cube pixels) and, in the
scenes with transparent materials, MIN_TRANSPARENT pixels with a transparent hit.  `python tests/parallel_cases.py` prints
what the oracle finds.  Everything is computed once per process and never modified afterwards."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (run as a script: the package beside tests/)

import fixtures as fx
import lens_cases as lc
import ray_color_cases as rc
import ray_query_cases as rq
from ntracer_amd import tracern

f32 = np.float32
W, H = lc.W, lc.H
FOV = lc.FOV

STRICT, CLEAN, VAR, PLAIN = lc.STRICT, lc.CLEAN, lc.VAR, lc.PLAIN
SWITCHES = lc.SWITCHES

SCENES = list(lc.SCENES)
# one case each under a switch: the ray route's remaining kernels, and a second opinion on the packet scenes from the per-lane
# kernels (NTRACER_FORCE_VAR, NTRACER_COMPOSITE_KERNEL=2: the same image is expected)
SWITCHED = [
    ("cell600_n4", STRICT, "lit"),
    ("feature5_n5", CLEAN, ""),             # rays_color_t<N,false>
    ("simplex10_n10", VAR, ""),             # rays_color_var
    ("cell600_n4", PLAIN, ""),              # rays_color<N,false,false>
    ("cell600_n4", PLAIN, "lit"),           # rays_color<N,true,false>
    ("simplex10_n10", PLAIN, ""),           # rays_color<N,true,true>
    ("feature11_n11", CLEAN, ""),           # rays_color_var_t<false>
]
CASES = SCENES + SWITCHED

MIN_OPAQUE, MIN_BOX_HITS = 25, 100
MIN_TRANSPARENT = {"feature5_n5": 20, "feature11_n11": 20}
BOX_HALF_WIDTH = 1.5


def case_id(case):
    name, env, variant = case
    return name + "".join("," + k[len("NTRACER_"):] for k in sorted(env)) + ("," + variant if variant else "")


is_box = lc.is_box


@functools.lru_cache(maxsize=None)
def camera(name):
    """(origin, axes) of the scene's golden camera (the index lens_cases.VIEWS names), where it stands"""
    k = lc.VIEWS[name][0]
    if is_box(name):
        n = int(name[3:])
        if n == 6:
            g = fx.load("box_n6_1920x1080")
            return np.asarray(g["origins"][k], f32), np.asarray(g["axes"][k], f32)
        o, q = fx.stress_cameras(n, np.random.default_rng(rc.SEED))[k]
        return np.asarray(o, f32), np.asarray(q, f32)
    g, n, flat = rq.scene(name)
    f = int(g["frames"][k])
    return np.asarray(g["origins"][f], f32), np.asarray(g["axes"][f], f32)


@functools.lru_cache(maxsize=None)
def box_of(name):
    g, n, flat = rq.scene(name)
    return np.asarray(g["aabb_start"], f32), np.asarray(g["aabb_end"], f32)


@functools.lru_cache(maxsize=None)
def half_width(name):
    if is_box(name):
        return BOX_HALF_WIDTH
    lo, hi = box_of(name)
    return float(f32(0.5) * (hi - lo).max())


def centre_camera(name):
    """the scene's camera moved to the centre of the scene's box: most rays start inside the box (t_near = 0)"""
    o, q = camera(name)
    lo, hi = box_of(name)
    return (f32(0.5) * (lo + hi)).astype(f32), q


def parallel_rays(o, q, w, h, hw):
    """the header's formula in plain numpy fp32, one rounding an operation: (o' [h * w][n], forward [n])"""
    o, q = np.asarray(o, f32), np.asarray(q, f32)
    half_w, half_h = f32(f32(w) / f32(2)), f32(f32(h) / f32(2))
    k = f32(f32(hw) / half_w)
    out = np.zeros((h * w, len(o)), f32)
    for y in range(h):
        sy = f32(k * f32(f32(y) - half_h))
        for x in range(w):
            sx = f32(k * f32(f32(x) - half_w))
            out[y * w + x] = (o + q[0] * sx).astype(f32) - (q[1] * sy).astype(f32)
    return out, q[2].copy()


def library_rays(o, q, w, h, hw):
    """the same rays from the library: Scene.parallel_rays (test_parallel_host.py pins the two against each other bit for bit)"""
    sc = tracern.BoxScene(len(o))                    # (the rays depend on the camera and the setting alone)
    sc.set_parallel_projection(hw)
    return sc.parallel_rays(w, h, lc.camera_of(o, q))


def _unit(v):
    return (v / np.sqrt((v * v).sum(dtype=f32))).astype(f32)


def inside_box(name, origins):
    lo, hi = box_of(name)
    return int(((origins > lo) & (origins < hi)).all(axis=1).sum())


@functools.lru_cache(maxsize=None)
def _counts(name, centred, hw):
    o, q = centre_camera(name) if centred else camera(name)
    org, fwd = library_rays(o, q, W, H, hw)          # the floors are counted on the rays the library says a render casts
    cnt = len(org)
    v = np.repeat(fwd[None], cnt, axis=0)
    if is_box(name):
        ref = rc.CentrePixel(len(o)).colors(org, v)
        return int((ref[:, 0] != ref[:, 1]).sum()), 0
    g, n, flat = rq.scene(name)
    orc = rq.Oracle(n, flat, False, len(flat["solid_types"]) == 0)
    none = np.full(cnt, -1, np.int32)
    r = orc.intersects(org, np.repeat(_unit(fwd)[None], cnt, axis=0), np.full(cnt, -rq.FLT_MAX), np.full(cnt, rq.FLT_MAX), none, none)
    return int((r["item"] >= 0).sum()), int((r["n_transparent"] > 0).sum())


def counts(name, centred=False, hw=None):
    """(opaque hits, pixels with a transparent hit) the oracle finds at W x H; BoxScene: (cube pixels, 0)"""
    return _counts(name, centred, half_width(name) if hw is None else hw)


def check_floors(case, centred=False):
    name = case[0]
    c = counts(name, centred)
    if is_box(name):
        assert c[0] >= MIN_BOX_HITS, (case_id(case), c)
    else:
        assert c[0] >= MIN_OPAQUE and c[1] >= MIN_TRANSPARENT.get(name, 0), (case_id(case), c)
    return c


@functools.lru_cache(maxsize=None)
def _expected(name, clean, strict, variant, cam, w, h, hw):
    env = dict(([("NTRACER_CLEAN_NORMALS", "1")] if clean else []) + ([("NTRACER_STRICT_REFERENCE", "1")] if strict else []))
    o, q = camera(name) if cam is None else (np.frombuffer(cam[0], f32), np.frombuffer(cam[1], f32).reshape(len(cam[0]) // 4, -1))
    org, fwd = parallel_rays(o, q, w, h, hw)
    v = np.repeat(fwd[None], len(org), axis=0)
    out = rc.CentrePixel(len(o)).colors(org, v) if is_box(name) else lc.oracle_colors(name, env, variant, org, v)
    out.setflags(write=False)
    return out


def expected(case, cam=None, size=(W, H), hw=None):
    """fp32 [h * w][3]: the oracle's colour of every pixel of the case (unclamped); `cam`: another camera (origin, axes) than
    the case's.  NTRACER_FORCE_VAR and NTRACER_COMPOSITE_KERNEL change the kernels, not the answers: they share the default's
    image."""
    name, env, variant = case
    key = None if cam is None else (np.asarray(cam[0], f32).tobytes(), np.asarray(cam[1], f32).tobytes())
    return _expected(name, env.get("NTRACER_CLEAN_NORMALS") == "1", env.get("NTRACER_STRICT_REFERENCE") == "1", variant, key,
                     size[0], size[1], half_width(name) if hw is None else hw)


def route(case):
    """the kernels a case lands on, by the rules of enqueue_parallel (nt_api.cpp): the packet walk's two passes, or the
    ray-colour kernel behind parallel_expand"""
    name, env, variant = case
    if is_box(name):
        return ("parallel_expand", rc.box_route(int(name[3:])))
    r = lc.route(case + ("",))
    if r[0] == "lens_expand":
        return ("parallel_expand", r[1])
    scal = r[0][len("composite_packet<N,32,false,"):].split(",")[0]
    return ("parallel_packet<N,32,%s>" % scal, r[1].replace("lens_shade", "parallel_shade"))


def scene(case, mp, cam=None):
    """the case's scene on the library, its camera and the projection set and the switches in the environment of `mp`"""
    sc = lc.scene(case + ("",), mp)
    o, q = camera(case[0]) if cam is None else cam
    sc._set_camera_arrays(o, q)
    sc.set_parallel_projection(half_width(case[0]))
    return sc


if __name__ == "__main__":
    import time
    for case in CASES:
        t = time.time()
        c = check_floors(case)
        e = expected(case)
        print("%-40s %dx%d half_width %-8.5g %-60s %4d opaque hits, %4d with a transparent hit, %4d colours (%.1f s)"
              % (case_id(case), W, H, half_width(case[0]), " + ".join(route(case)), c[0], c[1], len(np.unique(e, axis=0)), time.time() - t))
    for name in ("box6", "box25"):
        print("%s at half_width 2.5: %d cube pixels" % (name, counts(name, hw=2.5)[0]))
    o, q = centre_camera("cell600_n4")
    print("cell600_n4 from the centre of its box: %d opaque hits, %d of %d origins inside the box"
          % (counts("cell600_n4", True)[0], inside_box("cell600_n4", parallel_rays(o, q, W, H, half_width("cell600_n4"))[0]), W * H))
