"""Ray sets and the oracle's colours shared by tests/test_ray_colors_host.py and tests/test_ray_colors_gpu.py.

The oracle has no entry that takes a ray.  It needs none: a ray (o, v) is exactly the centre pixel of a 2 x 2 view of a camera
with origin o and forward row v -- sx = sy = 0, so the ray source yields v / |v| in its own operation order -- and
`CentrePixel` asks for `colors_at([1], [1], 2, 2)` through such a camera, one oracle call a ray.
tests/test_ray_colors_host.py pins the method itself against colors_at of real cameras, bit for bit.

A *case* is (golden scene, NTRACER_* switches, variant).  The variant changes materials and parameters:
  ""                         as captured
  "mirror"                   every material 30 % reflective
  "lit"                      "mirror" with shadows on, a point light outside the scene's box, one inside it and a global
                             light (the lit variant of tools/composite_soak.py)
  "reflective"               "lit" with max_reflect_depth 6
  "transparent_reflective"   every material 30 % reflective, max_reflect_depth 6: with transparent materials that is more
                             ray_color frames than the fixed-n kernel keeps (NT_TFRAMES), at any n
Rays of a case, from ray_query_cases.batches (whose oracle hit records come with them): (A) the golden cameras' primary rays
thinned to <= 1 500, (B) second legs from the oracle's hit points, <= 1 000, (C) the 500 edge cases -- zero components, origins
on the root's split plane -- and (S) 200 rays of (A) with the direction scaled by seeded factors in [1e-3, 1e3], whose
expected colours are the unscaled rays'.

The kernel instantiation each case reaches (nt_rays.hpp launch_rays_fixed, nt_var.hip nt_launch_rays; `route` below works it
out from the scene by the rules of rays_enqueue in nt_api.cpp, and test_ray_colors_host.py checks that no launch is left out):
  cell600_n4 mirror                       rays_color<N,true,false>     batches alone, reflective
  cell600_n4 mirror STRICT_REFERENCE      rays_color<N,true,false>     ... the reference's exact walk
  cell600_n4 lit                          rays_color<N,true,false>     ... shadow rays
  cell600_n4 reflective                   rays_color<N,true,false>     ... six levels
  simplex7_n7                             rays_color<N,false,false>    batches alone, camera light only (*)
  simplex10_n10                           rays_color<N,true,true>      loose triangles in the leaves
  simplex10_n10 FORCE_VAR                 rays_color_var
  feature5_n5                             rays_color_t<N,true>         transparent materials, Solids
  feature5_n5 CLEAN_NORMALS               rays_color_t<N,false>
  feature5_n5 FORCE_VAR                   rays_color_var_t<true>
  feature5_n5 FORCE_VAR transparent_refl. rays_color_var_t<true>       seven frames
  feature11_n11                           rays_color_var_t<true>
  feature11_n11 CLEAN_NORMALS             rays_color_var_t<false>      (*)
  lit12_n12, feature16_n16                rays_color_var_t<true>
  BoxScene n = 3, 6, 10, 12, 24           rays_box<N>
  BoxScene n = 25, 40                     rays_box_var
(*) two cases more than the feature's list asked for: without them two launches would have no case.

Everything is computed once per process and never modified afterwards."""
import ctypes as C
import ctypes.util
import functools

import numpy as np

import fixtures as fx
import oracle_binding as ob
import ray_query_cases as rq

f32 = np.float32
SEED = 20241018
MAX_A, MAX_B, N_SCALED = 1500, 1000, 200

STRICT = {"NTRACER_STRICT_REFERENCE": "1"}
CLEAN = {"NTRACER_CLEAN_NORMALS": "1"}
VAR = {"NTRACER_FORCE_VAR": "1"}
SWITCHES = ("NTRACER_STRICT_REFERENCE", "NTRACER_CLEAN_NORMALS", "NTRACER_FORCE_VAR")       # what a ray call routes on

CASES = [
    ("cell600_n4", {}, "mirror"),
    ("cell600_n4", STRICT, "mirror"),
    ("cell600_n4", {}, "lit"),
    ("cell600_n4", {}, "reflective"),
    ("feature5_n5", {}, ""),
    ("feature5_n5", CLEAN, ""),
    ("feature5_n5", VAR, ""),
    ("feature5_n5", VAR, "transparent_reflective"),
    ("simplex7_n7", {}, ""),
    ("simplex10_n10", {}, ""),
    ("simplex10_n10", VAR, ""),
    ("feature11_n11", {}, ""),
    ("feature11_n11", CLEAN, ""),
    ("lit12_n12", {}, ""),
    ("feature16_n16", {}, ""),
]
BOX_DIMS = (3, 6, 10, 12, 24, 25, 40)
BOX_CAMERAS, BOX_VIEW = 20, (64, 48)

# floors by the oracle alone, so that no case passes on background: opaque hits among (A), rays with a transparent hit, rays of
# the lit variants whose colour the shadows change, BoxScene rays that hit the cube (red != green).  The fixtures meet every one
# on this set of rays, so none was lowered (python tests/ray_color_cases.py prints the figures: opaque hits 47 .. 671, transparent
# 31 and 44, shadowed 671, cube hits 1352 .. 1452).
MIN_OPAQUE = 25
MIN_TRANSPARENT = {"feature5_n5": 20, "feature11_n11": 20}
MIN_SHADOWED = 10
MIN_BOX_HITS = 100


def case_id(case):
    name, env, variant = case
    return name + "".join("," + k[len("NTRACER_"):] for k in sorted(env)) + ("," + variant if variant else "")


def route(case):
    """the kernel a composite case lands on, by the rules of rays_enqueue (nt_api.cpp) and the two launchers"""
    name, env, variant = case
    n, flat, params = case_scene(case)
    m = np.asarray(flat["materials"])
    opaque, reflective = bool((m[:, 6] >= 1).all()), bool((m[:, 7] > 0).any())
    solids, scalar = len(flat["solid_types"]) > 0, len(flat["solid_types"]) + len(flat["tri_recs"]) > 0
    clean = env.get("NTRACER_CLEAN_NORMALS") == "1"
    var = n > 10 or env.get("NTRACER_FORCE_VAR") == "1"
    if not opaque or (solids and not clean):
        frames = int(params["max_reflect_depth"]) + 1 if reflective else 1
        alias = "false" if clean else "true"
        return "rays_color_var_t<%s>" % alias if var or frames > 6 else "rays_color_t<N,%s>" % alias
    if var:
        return "rays_color_var"
    lights = np.asarray(params["point_light_color"]).size + np.asarray(params["global_light_color"]).size > 0
    feat = lights or reflective or scalar
    return "rays_color<N,%s,%s>" % ("true" if feat else "false", "true" if scalar else "false")


def box_route(n):
    return "rays_box<N>" if n <= 24 else "rays_box_var"


@functools.lru_cache(maxsize=None)
def _case_scene(name, variant):
    g, n, flat = rq.scene(name)
    flat, params = dict(flat), dict(fx.params_of(g))
    if variant:
        m = np.array(flat["materials"], f32).copy()
        m[:, 7] = 0.3
        flat["materials"] = m
    if variant in ("lit", "reflective"):
        lo, hi = np.asarray(g["aabb_start"], f32), np.asarray(g["aabb_end"], f32)
        ctr, ext = 0.5 * (lo + hi), 0.5 * (hi - lo)
        out_pos = ctr + ext * 3.0 * np.resize(np.array([1.0, 0.8, -0.9, 0.4], f32), n)
        in_pos = ctr + ext * 0.15 * np.resize(np.array([-0.5, 0.3, 0.2, -0.4], f32), n)
        gdir = np.resize(np.array([0.2, -0.9, 0.3, 0.1], f32), n)
        params.update(shadows=1, point_light_pos=np.array([out_pos, in_pos], f32),
                      point_light_color=np.array([[40.0 * np.linalg.norm(ext) ** (n - 1)] * 3, [0.5 * np.linalg.norm(ext) ** (n - 1)] * 3], f32),
                      global_light_dir=np.array([gdir / np.linalg.norm(gdir)], f32), global_light_color=np.array([[0.4, 0.4, 0.5]], f32),
                      ambient=np.array([0.02, 0.02, 0.03], f32))
    if variant in ("reflective", "transparent_reflective"):
        params["max_reflect_depth"] = 6
    return n, flat, params


def case_scene(case):
    """(n, flat description, parameters) of a case's scene"""
    return _case_scene(case[0], case[2])


_tanf = None


def fov_inverse(fov, width):
    """flat_origin_ray_source::set_params (tracer.hpp:65-69) as the library and the oracle compute it: tanf in fp32"""
    global _tanf
    if _tanf is None:
        _tanf = C.CDLL(ctypes.util.find_library("m") or "libm.so.6").tanf
        _tanf.restype, _tanf.argtypes = C.c_float, [C.c_float]
    return f32(f32(_tanf(f32(f32(fov) / f32(2)))) / f32(f32(width) / f32(2)))


def camera_rays(axes, xs, ys, width, height, fov=0.8):
    """the camera's own unnormalised rays, v = (forward + right * sx) - up * sy in fp32 (tracer.hpp:71-74)"""
    axes = np.asarray(axes, f32)
    fov_i = fov_inverse(fov, width)
    sx = (fov_i * (np.asarray(xs).astype(f32) - f32(width) / f32(2))).astype(f32)
    sy = (fov_i * (np.asarray(ys).astype(f32) - f32(height) / f32(2))).astype(f32)
    return np.ascontiguousarray(((axes[2][None] + axes[0][None] * sx[:, None]) - axes[1][None] * sy[:, None]).astype(f32))


class CentrePixel(object):
    """the oracle's colour of arbitrary rays: pixel (1, 1) of a 2 x 2 view of a camera at o whose forward row is v"""

    def __init__(self, n, flat=None, params=None, clean_normals=False, prune=False):
        self.n = n
        self.sc = ob.OracleScene(n, np.zeros(n, f32), np.eye(n, dtype=f32), flat=flat, params=params, clean_normals=clean_normals, prune=prune)
        self.o, self.a = self.sc._keep["origin"], self.sc._keep["axes"]        # the arrays the oracle reads
        assert self.o.shape == (n,) and self.a.shape == (n, n)

    def colors(self, origins, directions):
        origins, directions = np.asarray(origins, f32), np.asarray(directions, f32)
        count = len(directions)
        out = np.zeros((count, 3), f32)
        one = np.ones(1, np.int32)
        px, L, s = one.ctypes.data_as(ob.i32p), ob.lib(), C.byref(self.sc.s)
        c = ob.Counters()
        for i in range(count):
            self.o[:] = origins if origins.ndim == 1 else origins[i]
            self.a[2] = directions[i]
            L.nto_colors_at(s, 2, 2, 1, px, px, C.cast(out.ctypes.data + 12 * i, ob.f32p), C.byref(c))
        return out


class Rays(object):
    pass


def _thin(sl, cap):
    count = sl.stop - sl.start
    step = -(-count // cap)
    return np.arange(sl.start, sl.stop, max(step, 1))


@functools.lru_cache(maxsize=None)
def _rays(name, env_key, variant):
    case = (name, dict(env_key), variant)
    env = case[1]
    n, flat, params = case_scene(case)
    b = rq.batches((name, env))
    ia, ib, ic = _thin(b.i_slices["A"], MAX_A), _thin(b.i_slices["B"], MAX_B), _thin(b.i_slices["C"], rq.N_EDGE)
    pick = np.concatenate([ia, ib, ic])
    rng = np.random.default_rng(SEED)
    scaled = ia[np.linspace(0, len(ia) - 1, N_SCALED).astype(int)]
    factors = (10.0 ** rng.uniform(-3.0, 3.0, N_SCALED)).astype(f32)
    r = Rays()
    r.n, r.case = n, case
    r.slices = dict(A=slice(0, len(ia)), B=slice(len(ia), len(ia) + len(ib)), C=slice(len(ia) + len(ib), len(pick)),
                    S=slice(len(pick), len(pick) + N_SCALED))
    r.origins = np.ascontiguousarray(np.concatenate([b.i_origins[pick], b.i_origins[scaled]]))
    r.directions = np.ascontiguousarray(np.concatenate([b.i_directions[pick], (b.i_directions[scaled] * factors[:, None]).astype(f32)]))
    assert np.isfinite(r.directions).all() and (r.directions != 0).any(axis=1).all()
    r.per_frame = b.per_frame
    # the oracle's hit records of the rays (no skip for (A) and (C); the (B) records were taken with the skip and only count)
    r.opaque_hits_a = int((b.i_ref["item"][ia] >= 0).sum())
    r.transparent = int((b.i_ref["n_transparent"][np.concatenate([ia, ic])] > 0).sum())
    clean = env.get("NTRACER_CLEAN_NORMALS") == "1"
    prune = env.get("NTRACER_STRICT_REFERENCE") != "1" and len(flat["solid_types"]) == 0        # (as ray_query_cases.batches)
    orc = CentrePixel(n, flat, params, clean, prune)
    ref = orc.colors(r.origins[:len(pick)], r.directions[:len(pick)])
    r.ref = np.concatenate([ref, ref[np.searchsorted(ia, scaled)]])          # (S): the unscaled rays' colours
    r.shadowed = None
    if variant in ("lit", "reflective"):
        p0 = dict(params)
        p0["shadows"] = 0
        unshadowed = CentrePixel(n, flat, p0, clean, prune).colors(r.origins[r.slices["A"]], r.directions[r.slices["A"]])
        r.shadowed = int((unshadowed != ref[r.slices["A"]]).any(axis=1).sum())
    for v in vars(r).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def rays(case):
    """the rays of a composite case and the oracle's colour of each, the oracle in the GPU's mode"""
    name, env, variant = case
    return _rays(name, tuple(sorted(env.items())), variant)


@functools.lru_cache(maxsize=None)
def box_rays(n):
    """BoxScene(n): the first 20 stress cameras, a 10 x 10 lattice of a 64 x 48 view each, rays as the unnormalised v"""
    rng = np.random.default_rng(SEED + n)
    w, h = BOX_VIEW
    xs, ys = np.meshgrid(3 + 6 * np.arange(10), 2 + 5 * np.arange(10))
    xs, ys = xs.ravel(), ys.ravel()
    os_, ds = [], []
    for o, q in fx.stress_cameras(n, rng)[:BOX_CAMERAS]:
        ds.append(camera_rays(q, xs, ys, w, h))
        os_.append(np.repeat(np.asarray(o, f32)[None], len(xs), axis=0))
    r = Rays()
    r.n = n
    r.per_camera = len(xs)
    r.origins, r.directions = np.ascontiguousarray(np.concatenate(os_)), np.ascontiguousarray(np.concatenate(ds))
    ok = np.isfinite(r.directions).all(axis=1) & (r.directions != 0).any(axis=1)
    assert ok.all()
    r.ref = CentrePixel(n).colors(r.origins, r.directions)
    r.hits = int((r.ref[:, 0] != r.ref[:, 1]).sum())
    for v in vars(r).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def check_floors(case):
    r = rays(case)
    assert r.opaque_hits_a >= MIN_OPAQUE, (case_id(case), r.opaque_hits_a)
    if case[0] in MIN_TRANSPARENT:
        assert r.transparent >= MIN_TRANSPARENT[case[0]], (case_id(case), r.transparent)
    if r.shadowed is not None:
        assert r.shadowed >= MIN_SHADOWED, (case_id(case), r.shadowed)


if __name__ == "__main__":
    import time
    for case in CASES:
        t = time.time()
        r = rays(case)
        print("%-50s %-26s %5d rays, %4d opaque hits in (A), %4d with a transparent hit, shadows change %s  (%.1f s)"
              % (case_id(case), route(case), len(r.ref), r.opaque_hits_a, r.transparent, r.shadowed,
                 time.time() - t))
        check_floors(case)
    for n in BOX_DIMS:
        r = box_rays(n)
        print("BoxScene(%d): %d rays, %d hit the cube" % (n, len(r.ref), r.hits))
        assert r.hits >= MIN_BOX_HITS
