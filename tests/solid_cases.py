"""Torture scenes for the Solid family (hypercube, hypersphere), their ray batches and two references, shared by
tests/test_solids_host.py (on the CPU) and tests/test_solids_gpu.py.

Scenes -- scene(name, n), built here from tables, the tree from the native builder:
  field     40 Solids and no simplex: 20 cubes and 20 spheres on a jittered 5 x 4 x 2 lattice in the first three coordinates.  Four
            orientation kinds cycle: c I, c R (a rotation), an anisotropic diagonal (4 : 1) and a shear (R D R' plus off-diagonal
            terms).  Solid k is a cube for even k, of kind (k // 2) % 4 and of material k % 3.
  nest      a transparent cube around an opaque sphere; a transparent sphere in front of a transparent cube in front of an opaque
            sheared cube; two cubes at the same place with different materials (COINCIDENT: equal distances, the first one tested
            wins, so the float64 comparison takes the two for one).
  mirror    a reflective sphere facing a reflective sheared cube, a point light between them, shadows on, max_reflect_depth 4.
  pierced   simplices in batches with a sphere and a sheared cube poking through them, so that within one leaf the nearest hit
            alternates between a batch lane and a Solid: at n <= 10 the lean N-orthoplex of test_composite_matrix, beyond it (2^n
            facets, their normals of length 0 in fp32) the three planes of high_dimension_cases.wide_comb(n, 4).
Materials: 0 opaque, 1 reflective, 2 transparent; none has a specular term, so no colour goes through powf and the colours of the
oracle and of the kernels can be compared bit for bit.  kinds(name) are the parameter sets a scene is rendered with.

Above the third coordinate everything is kept small -- the cameras' hidden tilt, the Solids' hidden offsets -- and R mixes the
visible and the hidden axes by 0.1 rad a plane: at n = 64 a freely rotated cube of half-edge c reaches c sqrt(n) into the view.

Ray batches -- batches(name, n, variant), laid end to end in one closest-hit and one occlusion batch as ray_query_cases does:
  A0 A1 A2  primary rays of three cameras: outside, inside a sphere, inside a cube
  B         +-e_k from lattice origins against the identity-oriented cubes: every other component of the direction is exactly 0,
            some origins lie exactly on a face plane (dist == 0: no hit), some lines run exactly along a face (p_j == +-1)
  C         rays aimed at each sphere's limb, at (1 +- delta) of its radius, delta of DELTAS
  D         rays aimed at cube edges and vertices, (1 +- delta) of them
  ES        from every hit of A0..A2 towards a random point of the scene's box, with skip_item the Solid that was hit
  ENO, ENI  the same legs without the skip, those that leave the Solid (ENO) and those that head into it (ENI, by the sign of
            ld . n_local in float64: self-intersection at a distance around 0, of either sign in fp32, so oracle only)
            -- as occlusion queries the leg's length is `distance`

References:
  the oracle (oracle/ntracer_oracle.c) through ray_query_cases.Oracle, prune_beyond_hit off, in both normal modes;
  brute_force: float64, numpy, no tree, the reference's rules written out -- see its docstring.

The float64 comparison leaves out the rays nearer than MARGIN to a decision boundary; EXEMPT names the batches that are inside
it by construction, every other batch keeps at least 1 - CAP of its rays (test_solids_host.py asserts it by float64 alone).
TOLERANCE[n] is four times MEASURED[n], the largest relative deviation of the oracle's dist from float64 seen on the CPU.
float64 has no say on occlusion: the reference's _occludes leaves the far child of a branch out whenever the split lies nearer
than `distance` (tracer.hpp:1298), so what blocks a ray depends on the tree; there the oracle alone is the reference.

render_cases, query_cases, hits_cases and projection_cases list what tests/test_solids_gpu.py runs, route() names the kernels a
call lands on, and ROUTES is the table of them that tests/test_solids_host.py holds against the sources."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (run as a script: the package beside tests/)

import fixtures as fx
import oracle_binding as ob
import ray_color_cases as rc
import ray_query_cases as rq
from ntracer_amd import _lib, tracern

f32 = np.float32
FLT_MAX = rq.FLT_MAX
CUBE, SPHERE = tracern.CUBE, tracern.SPHERE

VIEW = (97, 61)                 # of the renders
QUERY_VIEW = (37, 21)           # of the cameras' rays in the query batches
THREADS = 16                    # the oracle's
FOV = 0.8
MARGIN = 1e-4
CAP = 0.05
DELTAS = (1e-7, 1e-6, 1e-5, 1e-3)
SEED = 20261020

SCENES = ("field", "nest", "mirror", "pierced")
FIELD_FIXED = tuple(range(3, 11))
OTHER_FIXED = (3, 4, 7, 10)
VAR_N = (11, 17, 33, 64)
FORCED_VAR = (("field", 3), ("field", 10), ("pierced", 3), ("pierced", 10))
COINCIDENT = (5, 6)             # of nest
BIG = (28, 31)                  # of field: an anisotropic cube and a sheared sphere of the far layer that reach across several cells

# [r g b, specular r g b, opacity, reflectivity, specular intensity, specular exponent]
MATERIALS = np.array([[0.9, 0.35, 0.2, 1, 1, 1, 1.0, 0.0, 0, 8],
                      [0.25, 0.8, 0.4, 1, 1, 1, 1.0, 0.3, 0, 8],
                      [0.3, 0.45, 0.95, 1, 0.9, 0.8, 0.5, 0.0, 0, 8]], f32)

# The deviation of the oracle's dist from float64's over every ray outside the margin of every batch of every scene at that n, all
# material variants, measured on the CPU (x86-64, glibc) by `python tests/solid_cases.py` -- dist_deviation's two figures: the
# largest relative deviation where the hit lies at NEAR = 1e-2 or further, and for the few nearer hits (Solids that touch or
# overlap where a second leg starts; down to 2e-3) the largest absolute deviation in ulps of the origin's largest coordinate, what
# such a distance is made of.  The tolerance is 4 x each: the kernels must equal the oracle bit for bit anyway, so the factor
# covers another platform's libm and sqrt only.
MEASURED = {3: (9.2e-06, 1.1), 4: (1.1e-05, 2.4), 5: (9.5e-05, 5.0), 6: (1.4e-05, 38), 7: (1.7e-05, 2.2), 8: (1.5e-05, 0.24), 9: (1.9e-05, 0.43),
            10: (1.9e-05, 204), 11: (4.7e-04, 6.7), 17: (2.7e-05, 8.0), 33: (2.7e-05, 29), 64: (1.9e-04, 33)}
TOLERANCE = {n: (4.0 * a, 4.0 * b) for n, (a, b) in MEASURED.items()}


def dims(name):
    return (FIELD_FIXED if name == "field" else OTHER_FIXED) + VAR_N


def scene_dims():
    return [(name, n) for name in SCENES for n in dims(name)]


def kinds(name):
    """the parameter sets a scene is rendered with (params, materials)"""
    return {"field": ("unlit", "lit", "reflective", "transparent"), "nest": ("unlit", "transparent"),
            "mirror": ("mirror",), "pierced": ("lit", "transparent")}[name]


def variants(name, n):
    """material variants of the query batches: "default" the three materials, "opaque" every material opaque (nest, and field at
    four dimensions: the plain query kernels)"""
    return ("default", "opaque") if name == "nest" or (name == "field" and n in (3, 10, 11, 64)) else ("default",)


def _freeze(c):
    for v in vars(c).values():
        for a in (v.values() if isinstance(v, dict) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return c


# ------------------------------------------------------------------ orientations and Solids
def _rot(rng, k):
    q, r = np.linalg.qr(rng.standard_normal((k, k)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def rotation(n, rng, angle=0.1):
    """a rotation of the first three axes, one of the others, and `angle` in each plane (k % 3, 3 + k)"""
    r = np.eye(n)
    r[:3, :3] = _rot(rng, 3)
    if n > 4:
        r[3:, 3:] = _rot(rng, n - 3)
    c, s = math.cos(angle), math.sin(angle)
    for k in range(n - 3):
        g = np.eye(n)
        a, b = k % 3, 3 + k
        g[a, a], g[a, b], g[b, a], g[b, b] = c, -s, s, c
        r = r @ g
    return r


KIND_NAMES = ("identity", "rotation", "anisotropic", "shear")


def orientation(n, kind, scale, rng):
    """the four orientation kinds, float64"""
    if kind == 0:
        return scale * np.eye(n)
    if kind == 1:
        return scale * rotation(n, rng)
    if kind == 2:
        return np.diag(2.4 * scale * np.resize([1.0, 0.5, 0.25, 0.7, 0.4], n))
    m = rotation(n, rng) @ np.diag(scale * np.resize([1.0, 0.6, 0.8, 0.7], n)) @ rotation(n, rng)
    off = 0.2 * scale * rng.uniform(-1, 1, (n, n))
    off[3:, :] *= 0.5 / math.sqrt(n)
    off[:, 3:] *= 0.5 / math.sqrt(n)
    np.fill_diagonal(off, 0)
    return m + off


def _centre(n, xyz, hidden=0.0):
    c = np.zeros(n)
    c[:3] = xyz
    c[3:] = hidden * np.where(np.arange(n - 3) % 2 == 0, 1.0, -1.0)
    return c


_MATERIAL = None


def solid_record(n, typ, centre, orient):
    """the record of a Solid whose image of the origin is `centre`: orientation, inverse, position = O^-1 centre, as
    tracern.Solid makes them"""
    global _MATERIAL
    if _MATERIAL is None:
        import ntracer_amd
        _MATERIAL = ntracer_amd.Material((1, 1, 1))
    m = tracern.Matrix(n, np.asarray(orient, f32))
    pos = np.linalg.solve(m._m.astype(np.float64), np.asarray(centre, np.float64))
    s = tracern.Solid(typ, list(pos), m, _MATERIAL)
    return np.concatenate([s.orientation._m.ravel(), s.inv_orientation._m.ravel(), s.position._v]).astype(f32)


def _empty_tables(n):
    rl = n * n + n + 1
    return dict(batch_recs=np.zeros((0, 4, rl), f32), batch_mats=np.zeros((0, 4), np.int32), tri_recs=np.zeros((0, rl), f32),
                tri_mats=np.zeros(0, np.int32))


def _build(n, solids, tables=None, **tree):
    """the flat scene of `solids` [(type, centre, orientation, material)] and of `tables` (batches, or none at all) under the
    native builder's tree"""
    d = dict(_empty_tables(n) if tables is None else tables)
    d["solid_recs"] = np.asarray([solid_record(n, t, c, o) for t, c, o, _ in solids], f32).reshape(-1, 2 * n * n + n)
    d["solid_types"] = np.asarray([t for t, _, _, _ in solids], np.int32)
    d["solid_mats"] = np.asarray([m for _, _, _, m in solids], np.int32)
    items = [(k << 2) | _lib.KIND_BATCH for k in range(len(d["batch_recs"]))] + [(k << 2) | _lib.KIND_SOLID for k in range(len(solids))]
    d.update(root=0, node_axis=np.array([-1], np.int32), node_split=np.zeros(1, f32), node_left=np.array([0], np.int32),
             node_right=np.array([len(items)], np.int32), items=np.asarray(items, np.int32), materials=MATERIALS.copy(),
             aabb_start=np.full(n, -8, f32), aabb_end=np.full(n, 8, f32))
    flat = tracern.CompositeScene.from_flat(n, d).with_rebuilt_tree(**tree)._flat_description()
    flat = {k: (np.array(v) if isinstance(v, (list, tuple, np.ndarray)) else v) for k, v in flat.items()}
    flat["batch_size"] = 4
    return flat


def field_solids(n):
    rng = np.random.default_rng(SEED + n)
    out = []
    for k in range(40):
        kind = (k // 2) % 4
        ix, iy, iz = k % 5, (k // 5) % 4, k // 20
        # (multiples of 1 / 64: with c = 1 / 4 the identity-oriented Solids' local coordinates are exact)
        jit = rng.integers(-8, 9, 3) / 64.0
        xyz = np.array([ix - 2.0, iy - 1.5, 1.25 * iz]) + jit
        scale = 0.25 if kind == 0 else float(rng.uniform(0.22, 0.32))
        if k in BIG:
            scale = 0.6
        out.append((CUBE if k % 2 == 0 else SPHERE, _centre(n, xyz, 0.0 if kind == 0 else 0.01), orientation(n, kind, scale, rng), k % 3))
    return out


def nest_solids(n):
    rng = np.random.default_rng(SEED + 100 + n)
    a, b = (-0.9, -0.2, 0.0), (0.9, -0.2, 0.0)
    return [(CUBE, _centre(n, a, 0.01), orientation(n, 1, 0.5, rng), 2),
            (SPHERE, _centre(n, a, 0.01), orientation(n, 0, 0.25, rng), 0),
            (SPHERE, _centre(n, (b[0], b[1], -0.9), 0.01), orientation(n, 2, 0.3, rng), 2),
            (CUBE, _centre(n, b, 0.01), orientation(n, 1, 0.3, rng), 2),
            (CUBE, _centre(n, (b[0], b[1], 0.9), 0.01), orientation(n, 3, 0.35, rng), 0),
            (CUBE, _centre(n, (0.0, 0.875, 0.25)), orientation(n, 0, 0.25, rng), 0),
            (CUBE, _centre(n, (0.0, 0.875, 0.25)), orientation(n, 0, 0.25, rng), 1)]


def mirror_solids(n):
    rng = np.random.default_rng(SEED + 200 + n)
    return [(SPHERE, _centre(n, (-0.75, 0.0, 0.0), 0.01), orientation(n, 0, 0.4, rng), 1),
            (CUBE, _centre(n, (0.75, 0.0, 0.1), 0.01), orientation(n, 3, 0.4, rng), 1)]


def pierced_solids(n):
    rng = np.random.default_rng(SEED + 300 + n)
    if n <= 10:         # on the facets x + y - z = 1 and -x - y - z = 1 of the octahedron the orthoplex shows in the first three axes
        return [(SPHERE, _centre(n, (0.4, 0.2, -0.4), 0.02), orientation(n, 0, 0.3, rng), 0),
                (CUBE, _centre(n, (-0.4, -0.2, -0.4), 0.02), orientation(n, 3, 0.25, rng), 1)]
    # through the planes z = 1 / 2 and z = 1 / 6 of wide_comb(n, 4)
    return [(SPHERE, _centre(n, (0.3, 0.25, 0.5)), orientation(n, 0, 0.3, rng), 0),
            (CUBE, _centre(n, (-0.25, -0.2, 0.17)), orientation(n, 3, 0.22, rng), 1)]


def _pierced_tables(n):
    if n <= 10:
        import test_composite_matrix as tcm
        flat = tcm.lean_flat(n)
    else:
        import high_dimension_cases as hd
        flat = hd.wide_comb(n, 4)
    return dict(batch_recs=np.asarray(flat["batch_recs"], f32), batch_mats=np.asarray(flat["batch_mats"], np.int32).reshape(-1, 4),
                tri_recs=np.zeros((0, n * n + n + 1), f32), tri_mats=np.zeros(0, np.int32))


@functools.lru_cache(maxsize=None)
def scene(name, n):
    """the flat description of a scene, the three materials as they are"""
    if name == "field":
        # (no cost terms: the builder cuts down to two Solids a leaf, the long anisotropic ones across several cells)
        flat = _build(n, field_solids(n), max_depth=10, split_threshold=2, traversal_cost=0.003, intersection_cost=2.0)
    elif name == "nest":
        flat = _build(n, nest_solids(n))
    elif name == "mirror":
        flat = _build(n, mirror_solids(n))
    elif name == "pierced":
        flat = _build(n, pierced_solids(n), _pierced_tables(n))
    else:
        raise KeyError(name)
    for v in flat.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return flat


def materials(kind):
    m = MATERIALS.copy()
    if kind in ("unlit", "lit", "opaque"):
        m[:, 6], m[:, 7] = 1.0, 0.0
    elif kind == "reflective":
        m[:, 6] = 1.0
        m[::2, 7] = 0.25
    return m


def scene_flat(name, n, kind):
    """the scene with the materials of a kind (or of a query variant)"""
    f = dict(scene(name, n))
    f["materials"] = materials(kind)
    return f


def params(name, n, kind):
    p = dict(fov=FOV, shadows=0, camera_light=1, max_reflect_depth=4, bg_gradient_axis=1, ambient=[.02, .02, .03],
             bg1=[1, 1, 1], bg2=[0, 0, 0], bg3=[0, 1, 1], point_light_pos=np.zeros((0, n), f32),
             point_light_color=np.zeros((0, 3), f32), global_light_dir=np.zeros((0, n), f32), global_light_color=np.zeros((0, 3), f32))
    if kind == "unlit":
        return p
    pl = np.zeros((1, n), f32)
    # a point light's strength is distance^-(n - 1): it stands within a unit or so of what it lights, and never nearer than 0.5
    pl[0, :3] = {"field": (0.5, -0.5, -0.9), "nest": (0.0, 0.1, -0.8), "mirror": (0.0, 0.15, -0.05), "pierced": (0.0, 0.1, -1.2)}[name]
    gl = np.full((1, n), 0.01, f32)
    gl[0, :3] = (0.2, -0.9, 0.3)
    p.update(shadows=1, point_light_pos=pl, point_light_color=np.array([[0.8, 0.7, 0.6]], f32), global_light_dir=gl,
             global_light_color=np.array([[.4, .4, .5]], f32))
    if kind == "reflective":
        p["max_reflect_depth"] = 2
    return p


# ------------------------------------------------------------------ cameras
def _axes(n, yaw, pitch, tilt, seed):
    """an orthonormal frame near the identity: the first three rows turned by yaw and pitch, every hidden component of them
    about `tilt`"""
    rng = np.random.default_rng(seed)
    m = np.eye(n)
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    m[:3, :3] = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    m[:3, 3:] = tilt * rng.uniform(0.5, 1.0, (3, n - 3)) * np.where(rng.random((3, n - 3)) < 0.5, -1.0, 1.0)
    # Gram-Schmidt by rows, the first three first
    q, _ = np.linalg.qr(m.T)
    q = q.T * np.sign(np.diag(q.T @ m.T))[:, None]
    return np.ascontiguousarray(q, f32)


def _hidden(n, size):
    return size * np.where(np.arange(n - 3) % 2 == 0, 1.0, -1.0)


def solid_centre(flat, k):
    n = len(flat["aabb_start"])
    r = np.asarray(flat["solid_recs"], np.float64)[k]
    return r[:n * n].reshape(n, n) @ r[2 * n * n:]


INSIDE_SPHERE = {"field": 11, "nest": 1, "mirror": 0, "pierced": 0}      # the Solid cameras 1 and 2 stand in
INSIDE_CUBE = {"field": 2, "nest": 3, "mirror": 1, "pierced": 1}


def cameras(name, n):
    """(origin, axes) of the three cameras: outside; inside a sphere; inside a cube -- all looking down +z, more or less"""
    flat = scene(name, n)
    tilt = 0.002
    hid = 0.001 if (name == "pierced" and n > 10) else (0.04 if name == "pierced" else 0.003)
    o0 = np.zeros(n)
    o0[:3] = {"field": (0.3, 0.2, -3.25), "nest": (0.1, 0.15, -4.0), "mirror": (0.05, 0.3, -3.5), "pierced": (0.1, 0.15, -3.0)}[name]
    o0[3:] = _hidden(n, hid)
    cams = [(o0.astype(f32), _axes(n, -0.05, 0.03, 0.0 if name == "pierced" else tilt, SEED + 7 * n))]
    for j, k in enumerate((INSIDE_SPHERE[name], INSIDE_CUBE[name])):
        c = solid_centre(flat, k)
        o = c.copy()
        r = np.asarray(flat["solid_recs"], np.float64)[k][:n * n].reshape(n, n)
        o += r @ np.concatenate([[0.2, -0.15, 0.1], np.resize([0.002, -0.002], n - 3)])          # well inside: |u| < 0.3
        # (mirror: towards the other Solid; nest: from the sphere towards the other group)
        yaw = {("mirror", 0): -1.2, ("mirror", 1): 1.2, ("nest", 0): -1.0}.get((name, j), 0.0)
        cams.append((o.astype(f32), _axes(n, yaw, 0.02, 0.0 if name == "pierced" else tilt, SEED + 7 * n + 1 + j)))
    return cams


# ------------------------------------------------------------------ the float64 reference
class Brute(object):
    pass


def _solid_parts(flat):
    n = len(flat["aabb_start"])
    r = np.asarray(flat["solid_recs"], np.float64).reshape(-1, 2 * n * n + n)
    return n, r[:, :n * n].reshape(-1, n, n), r[:, n * n:2 * n * n].reshape(-1, n, n), r[:, 2 * n * n:]


def _cube64(lo, ld):
    """the reference's hypercube rule on local rays: (dist or 0, local normal ray, margin)"""
    count, n = lo.shape
    dist = np.zeros(count)
    margin = np.full(count, np.inf)
    no, nd = np.zeros((count, n)), np.zeros((count, n))
    open_ = np.ones(count, bool)
    cols = np.arange(n)
    with np.errstate(all="ignore"):
        for i in range(n):
            di = ld[:, i]
            s = np.where(di < 0, 1.0, -1.0)
            t = (s - lo[:, i]) / di
            tried = open_ & (di != 0) & (t > 0)
            # an origin within MARGIN of the face's plane and within the face: whether t > 0 is the decision
            grazing = open_ & (di != 0) & (np.abs(s - lo[:, i]) < MARGIN) & (np.abs(np.delete(lo, i, axis=1)) <= 1 + MARGIN).all(axis=1)
            margin = np.where(grazing, np.minimum(margin, np.abs(s - lo[:, i])), margin)
            if not tried.any():
                continue
            idx = np.nonzero(tried)[0]
            p = ld[idx] * t[idx, None] + lo[idx]
            excess = np.abs(p[:, cols != i]) - 1.0                     # > 0: outside the face
            worst = excess.max(axis=1) if n > 1 else np.full(len(idx), -1.0)
            inside = worst <= 0
            # the distance to this axis's decision: the point nearest to leaving the face, or the one furthest outside it
            margin[idx] = np.minimum(margin[idx], np.abs(worst))
            h = idx[inside]
            dist[h] = t[h]
            p[:, i] = s[idx]
            no[h] = p[inside]
            nd[h, i] = s[h]
            open_[h] = False
    return dist, no, nd, margin


def _sphere64(lo, ld):
    with np.errstate(all="ignore"):
        a = (ld * ld).sum(axis=1)
        b = 2 * (ld * lo).sum(axis=1)
        c = (lo * lo).sum(axis=1) - 1
        disc = b * b - 4 * a * c
        t = (-b - np.sqrt(np.where(disc >= 0, disc, 0))) / (2 * a)
        hit = (disc >= 0) & (t > 0)
        margin = np.where(b != 0, np.abs(disc) / (b * b), np.where(disc == 0, 0.0, np.inf))
        # an origin within MARGIN of the surface, heading in: the sign of the near root is the decision
        margin = np.where((b < 0) & (np.abs(c) < MARGIN), np.minimum(margin, np.abs(c)), margin)
    dist = np.where(hit, t, 0.0)
    p = lo + ld * dist[:, None]
    return dist, p, p.copy(), margin


def _simplices64(n, recs, o, d):
    """triangle::intersects in float64 on the fp32 records [count][n n + n + 1]: per ray the nearest (dist, record) and margin"""
    recs = np.asarray(recs, np.float64)
    best = np.full(len(o), np.inf)
    which = np.full(len(o), -1)
    margin = np.full(len(o), np.inf)
    with np.errstate(all="ignore"):
        for k, r in enumerate(recs):
            fn, p1, e = r[1:1 + n], r[1 + n:1 + 2 * n], r[1 + 2 * n:].reshape(n - 1, n)
            denom = d @ fn
            t = -(o @ fn + r[0]) / denom
            ok = (denom != 0) & (t > 0)
            if not ok.any():
                continue
            idx = np.nonzero(ok)[0]
            area = (p1[None] - (o[idx] + t[idx, None] * d[idx])) @ e.T
            worst = np.maximum((-area).max(axis=1), area.sum(axis=1) - 1)          # > 0: outside
            margin[idx] = np.minimum(margin[idx], np.abs(worst))
            h = idx[(worst <= 0) & (t[idx] < best[idx])]
            best[h], which[h] = t[h], k
    return best, which, margin


def brute_force(flat, origins, directions, skip_item=None, opaque_only=True):
    """The nearest opaque hit of every ray, in float64, with no tree: a loop over all primitives with the reference's rules
    (src/tracer.hpp:126-173, 251-276) written out plainly on the fp32 records.
      the local ray of a Solid is (O^-1 o - p, O^-1 d): a point x of its surface is O (u + p);
      cube: the first axis in index order whose entry face (at -sign(d_i)) lies at a distance > 0 and whose point lies within the
            face, |p_j| <= 1 -- no fuzz; only entry faces are looked at, so from inside a cube is not there;
      sphere: the near root of the quadratic, which must be > 0 -- from inside it is negative and the sphere is not there;
      the normal ray is (O (u + p), O n_local), n_local = +-e_i for the cube and u itself for the sphere, not normalised;
      a simplex is hit at t > 0 where every edge coordinate is >= 0 and their sum <= 1.
    Returns item ((index << 2) | kind, -1: none), lane, dist, normal_origin, normal and `margin`, each ray's distance to the nearest
    decision boundary of a primitive it could hit: per cube axis tried, how far the face point is from leaving (or from
    entering) the face, max_j |p_j| - 1; |disc| / b^2 of a sphere; how far an origin that lies on a surface is from it; the edge
    coordinates' distance from 0 and their sum's from 1.  (The plainer min_j ||p_j| - 1| over every j is the same number for an
    axis whose point is within the face and a smaller one -- more rays left out -- for an axis that misses by a wide mark in
    another coordinate.)  Rays whose margin is below MARGIN are the ones fp32 may decide differently."""
    o, d = np.asarray(origins, np.float64), np.asarray(directions, np.float64)
    count = len(o)
    n, orient, inv, pos = _solid_parts(flat)
    mats = np.asarray(flat["materials"])
    skip = np.full(count, -1) if skip_item is None else np.asarray(skip_item)
    b = Brute()
    b.dist = np.full(count, np.inf)
    b.item, b.lane = np.full(count, -1, np.int32), np.full(count, -1, np.int32)
    b.margin = np.full(count, np.inf)
    b.normal_origin, b.normal = np.zeros((count, n)), np.zeros((count, n))
    for k in range(len(orient)):
        if opaque_only and not mats[int(flat["solid_mats"][k])][6] >= 1:
            continue
        item = (k << 2) | _lib.KIND_SOLID
        lo, ld = o @ inv[k].T - pos[k], d @ inv[k].T
        dist, no, nd, margin = (_cube64 if int(flat["solid_types"][k]) == CUBE else _sphere64)(lo, ld)
        live = skip != item
        b.margin = np.where(live, np.minimum(b.margin, margin), b.margin)
        h = np.nonzero(live & (dist > 0) & (dist < b.dist))[0]
        b.dist[h], b.item[h], b.lane[h] = dist[h], item, -1
        b.normal_origin[h] = (no[h] + pos[k]) @ orient[k].T
        b.normal[h] = nd[h] @ orient[k].T
    brec = np.asarray(flat["batch_recs"], np.float64).reshape(-1, n * n + n + 1)
    if len(brec):
        bm = np.asarray(flat["batch_mats"]).reshape(-1)
        lane_opaque = mats[bm][:, 6] >= 1
        # (skip: a batch lane is skipped by (item, lane); the batches here never start a second leg)
        for q in range(len(brec) // 4):
            # A QUIRK OF THE REFERENCE, found by this comparison: triangle_batch::intersects (tracer.hpp:551-599) answers with
            # the nearest lane alone, and the leaf then puts the whole batch on its `checked` list.  Where that lane is
            # transparent, an opaque lane of the same batch behind it is never seen: the batch gives no opaque hit.
            t, which, margin = _simplices64(n, brec[4 * q:4 * q + 4], o, d)
            b.margin = np.minimum(b.margin, margin)
            h = np.nonzero((which >= 0) & (t < b.dist))[0]
            if opaque_only:
                h = h[lane_opaque[4 * q + which[h]]]
            rec = 4 * q + which[h]
            b.dist[h], b.item[h], b.lane[h] = t[h], (q << 2) | _lib.KIND_BATCH, which[h]
            fn = brec[rec][:, 1:1 + n]
            fn = fn / np.linalg.norm(fn, axis=1)[:, None]
            b.normal[h] = np.where(((d[h] * fn).sum(axis=1) > 0)[:, None], -fn, fn)
            b.normal_origin[h] = o[h] + t[h, None] * d[h]
    b.safe = b.margin >= MARGIN
    return _freeze(b)


def canonical(name, item):
    """nest's coincident cubes count as one in the float64 comparison"""
    item = np.array(item)
    if name == "nest":
        item[item == ((COINCIDENT[1] << 2) | _lib.KIND_SOLID)] = (COINCIDENT[0] << 2) | _lib.KIND_SOLID
    return item


# ------------------------------------------------------------------ ray batches
def _unit32(v):
    v = np.asarray(v, f32)
    return (v / np.sqrt((v * v).sum(axis=1, dtype=f32))[:, None]).astype(f32)


def camera_batch(n, cam, w=QUERY_VIEW[0], h=QUERY_VIEW[1]):
    """the camera's own rays through every pixel of a w x h view, as nto_primary_dir gives them"""
    osc = ob.OracleScene(n, cam[0], cam[1], FOV)
    d = np.stack([osc.primary_dir(x, y, w, h) for y in range(h) for x in range(w)]).astype(f32)
    return np.repeat(np.asarray(cam[0], f32)[None], len(d), axis=0), d


def _axis_rays(n, flat):
    """B: +-e_k against every identity-oriented cube.  Local coordinates u = 4 (x - centre), exact in fp32."""
    _, orient, _, _ = _solid_parts(flat)
    os_, ds = [], []
    axes = list(range(n)) if n <= 6 else [0, 1, 2, 3, n // 2, n - 1]
    along = (-2.0, -1.5, 0.0, 0.5, 2.0)                     # of the ray's axis, in front of the entry face (sign +), inside, behind
    # of two other coordinates: inside the face, three times; outside it
    across = ((0.5, -0.25), (-0.75, 0.125), (0.25, 0.625), (1.5, 0.25))
    # inside the margin by construction, so only with the first of the axes: the origin exactly ON the entry face's plane
    # (dist == 0: no hit) and a line exactly along a face (p_j == 1)
    special = ((-1.0, (0.5, -0.25)), (-2.0, (1.0, 0.5)))
    for k in range(len(orient)):
        if int(flat["solid_types"][k]) != CUBE or not np.array_equal(orient[k], orient[k][0, 0] * np.eye(n)):
            continue
        c, s = solid_centre(flat, k), orient[k][0, 0]
        for a in axes:
            others = [j for j in range(n) if j != a]
            for sign in (1.0, -1.0):
                grid = [(u, v, q) for u in along for q, v in enumerate(across)]
                if a == axes[0]:
                    grid += [(u, v, 0) for u, v in special]
                for u, (v0, v1), q in grid:
                    loc = np.zeros(n)
                    loc[a] = u * sign
                    loc[others[(q + a) % len(others)]] = v0
                    loc[others[(q + a + 1) % len(others)]] = v1
                    os_.append(c + s * loc)
                    e = np.zeros(n)
                    e[a] = sign
                    ds.append(e)
    return np.asarray(os_, f32).reshape(-1, n), np.asarray(ds, f32).reshape(-1, n)


def _limb_rays(n, flat, rng):
    """C: from 3 w towards (1 +- delta) T, T a point of the tangent cone's circle of contact, in each sphere's local frame"""
    _, orient, _, pos = _solid_parts(flat)
    os_, ds = [], []
    for k in range(len(orient)):
        if int(flat["solid_types"][k]) != SPHERE:
            continue
        for rep in range(2):
            w = np.zeros(n)
            w[:3] = rng.standard_normal(3)
            w[3:] = 0.01 * rng.standard_normal(n - 3)
            w /= np.linalg.norm(w)
            v = np.zeros(n)
            v[:3] = rng.standard_normal(3)
            v -= (v @ w) * w
            v /= np.linalg.norm(v)
            t = w / 3.0 + math.sqrt(1 - 1 / 9.0) * v
            for delta in DELTAS:
                for sgn in (1.0, -1.0):
                    a, b = orient[k] @ (3.0 * w + pos[k]), orient[k] @ ((1 + sgn * delta) * t + pos[k])
                    os_.append(a)
                    ds.append(b - a)
    return np.asarray(os_, f32).reshape(-1, n), _unit32(np.asarray(ds).reshape(-1, n))


def _edge_rays(n, flat, rng):
    """D: towards (1 +- delta) e for e on an edge of the cube's section in the first three axes, at a vertex of it and at a vertex
    of the whole cube, from a point 3 units out"""
    _, orient, _, pos = _solid_parts(flat)
    os_, ds = [], []
    for k in range(len(orient)):
        if int(flat["solid_types"][k]) != CUBE:
            continue
        targets = []
        sg = lambda m: np.where(rng.random(m) < 0.5, -1.0, 1.0)
        e = np.zeros(n)
        e[:3] = sg(3)
        e[int(rng.integers(0, 3))] = rng.uniform(-0.8, 0.8)
        targets.append(e)
        e = np.zeros(n)
        e[:3] = sg(3)
        targets.append(e)
        targets.append(sg(n))
        for e in targets:
            src = 3.0 * e / np.linalg.norm(e) * math.sqrt(3.0)
            src[:3] += rng.uniform(-0.3, 0.3, 3)
            for delta in DELTAS:
                for sgn in (1.0, -1.0):
                    a, b = orient[k] @ (src + pos[k]), orient[k] @ ((1 + sgn * delta) * e + pos[k])
                    os_.append(a)
                    ds.append(b - a)
    return np.asarray(os_, f32).reshape(-1, n), _unit32(np.asarray(ds).reshape(-1, n))


EXEMPT = ("C", "D", "ENI")      # inside the margin by construction: oracle only there.  ENI: a leg that starts ON a Solid and
                                # heads into it meets that Solid at a distance around 0, of either sign


def heads_inward(flat, items, x, d):
    """in float64, whether a leg from the point x of the surface of Solid `items` (one a ray) along d goes into the Solid:
    ld . n_local < 0 in the Solid's own coordinates, n_local the outward normal of the unit cube's nearest face or of the unit
    sphere"""
    n, orient, inv, pos = _solid_parts(flat)
    out = np.zeros(len(x), bool)
    for i in range(len(x)):
        k = int(items[i]) >> 2
        u, ld = inv[k] @ x[i].astype(np.float64) - pos[k], inv[k] @ d[i].astype(np.float64)
        if int(flat["solid_types"][k]) == CUBE:
            a = int(np.argmax(np.abs(u)))
            out[i] = ld[a] * np.sign(u[a]) < 0
        else:
            out[i] = ld @ u < 0
    return out


class Batches(object):
    pass


def oracle_of(flat, n, clean):
    return rq.Oracle(n, flat, clean, False)                 # (prune_beyond_hit is off for every scene with Solids)


@functools.lru_cache(maxsize=None)
def batches(name, n, variant="default"):
    """the closest-hit batch (i_*) and the occlusion batch (o_*) of a scene with the oracle's answers in both normal modes
    (i_ref[clean], o_ref) and float64's (brute), computed once and frozen"""
    flat = scene_flat(name, n, "opaque" if variant == "opaque" else "transparent")
    rng = np.random.default_rng(SEED + 1000 + n)
    orc = oracle_of(flat, n, False)
    lo, hi = np.asarray(flat["aabb_start"], f32), np.asarray(flat["aabb_end"], f32)
    parts = []
    for j, cam in enumerate(cameras(name, n)):
        parts.append(("A%d" % j,) + camera_batch(n, cam))
    if variant == "default":
        parts.append(("B",) + _axis_rays(n, flat))
        parts.append(("C",) + _limb_rays(n, flat, rng))
        parts.append(("D",) + _edge_rays(n, flat, rng))
    parts = [p for p in parts if len(p[1])]
    oa, da = np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])
    na = sum(len(p[1]) for p in parts if p[0].startswith("A"))
    none = lambda m: np.full(m, -1, np.int32)
    ra = orc.intersects(oa[:na], da[:na], np.full(na, -FLT_MAX), np.full(na, FLT_MAX), none(na), none(na))
    # ---- E: from the hit point of every camera ray that hit a Solid towards a random point of the scene's box
    hit = np.nonzero((ra["item"] >= 0) & ((ra["item"] & 3) == _lib.KIND_SOLID))[0]
    oe = (oa[hit] + ra["dist"][hit, None] * da[hit]).astype(f32)
    to = (lo + (hi - lo) * rng.random((len(hit), n), dtype=f32)).astype(f32) - oe
    length = np.sqrt((to * to).sum(axis=1, dtype=f32)).astype(f32)
    de = (to / length[:, None]).astype(f32)
    # (without the self-skip: the legs that leave the Solid first, ENO, then those that head into it, ENI)
    inward = heads_inward(flat, ra["item"][hit], oe, de)
    order = np.concatenate([np.nonzero(~inward)[0], np.nonzero(inward)[0]])
    n_out = int((~inward).sum())
    on, dn, ln = oe[order], de[order], length[order]
    b = Batches()
    b.name, b.n, b.variant = name, n, variant
    b.slices, at = {}, 0
    for p in parts + [("ES", oe, de), ("ENO", on[:n_out], dn[:n_out]), ("ENI", on[n_out:], dn[n_out:])]:
        b.slices[p[0]] = slice(at, at + len(p[1]))
        at += len(p[1])
    b.i_origins = np.ascontiguousarray(np.concatenate([oa, oe, on]))
    b.i_directions = np.ascontiguousarray(np.concatenate([da, de, dn]))
    count = len(b.i_origins)
    b.i_t_near, b.i_t_far = np.full(count, -FLT_MAX, f32), np.full(count, FLT_MAX, f32)
    b.i_skip_item = np.concatenate([none(len(oa)), ra["item"][hit], none(len(hit))]).astype(np.int32)
    b.i_skip_lane = none(count)
    b.i_ref = {clean: oracle_of(flat, n, clean).intersects(b.i_origins, b.i_directions, b.i_t_near, b.i_t_far, b.i_skip_item, b.i_skip_lane)
               for clean in (False, True)}
    b.o_origins, b.o_directions = b.i_origins, b.i_directions
    b.o_distance = np.concatenate([np.full(len(oa), FLT_MAX, f32), length, ln])
    b.o_ref = orc.occludes(b.o_origins, b.o_directions, b.o_distance, b.i_t_near, b.i_t_far, b.i_skip_item, b.i_skip_lane)
    b.brute = brute_force(flat, b.i_origins, b.i_directions, b.i_skip_item)
    for v in [b.i_ref[False], b.i_ref[True], b.o_ref]:
        for a in v.values():
            a.setflags(write=False)
    return _freeze(b)


def capped(b, key):
    return key not in EXEMPT


NEAR = 1e-2                     # hits nearer than this (self-intersections, Solids that touch) are held to an absolute bound


def dist_deviation(origins, got, want, both):
    """(largest relative deviation of dist over the rays of `both` whose float64 dist is >= NEAR, largest absolute deviation over
    the nearer ones in ulps of the origin's largest coordinate -- the rounding of the origin is what such a distance is made of)"""
    dev = np.abs(np.asarray(got, np.float64) - want)
    far, near = both & (want >= NEAR), both & (want < NEAR)
    ulp = np.spacing(np.abs(np.asarray(origins, f32)).max(axis=1)).astype(np.float64)
    return (float((dev[far] / want[far]).max()) if far.any() else 0.0, float((dev[near] / ulp[near]).max()) if near.any() else 0.0)


def compare_with_float64(b, got, label, tolerance=None):
    """`got` (dist, item as the oracle's records have them) against b.brute on the rays outside the margin: which primitive is
    hit must be equal, dist within TOLERANCE[n] (dist_deviation's two figures).  Returns the two figures."""
    bf = b.brute
    tol = TOLERANCE[b.n] if tolerance is None else tolerance
    safe = bf.safe
    gi, wi = canonical(b.name, got["item"]), canonical(b.name, bf.item)
    bad = np.nonzero(safe & (gi != wi))[0]
    assert len(bad) == 0, "%s: float64 names another primitive on %d rays, first %d: got %d, float64 %d (margin %g)" % (
        label, len(bad), bad[0], gi[bad[0]], wi[bad[0]], bf.margin[bad[0]])
    worst = dist_deviation(b.i_origins, got["dist"], bf.dist, safe & (wi >= 0))
    assert worst[0] <= tol[0] and worst[1] <= tol[1], "%s: dist differs from float64 by %g relative, nearer than %g by %g ulps (allowed %g, %g)" % (
        (label, worst[0], NEAR, worst[1]) + tuple(tol))
    return worst


# ------------------------------------------------------------------ renders
@functools.lru_cache(maxsize=None)
def oracle_scene(name, n, kind, camera, clean):
    cam = cameras(name, n)[camera]
    p = params(name, n, kind)
    return ob.OracleScene(n, cam[0], cam[1], fov=FOV, flat=scene_flat(name, n, kind), params=p, clean_normals=clean)


@functools.lru_cache(maxsize=None)
def frame(name, n, kind, camera, clean):
    """the oracle's RGBF32 frame of the view as (H, W * 3) floats"""
    a = oracle_scene(name, n, kind, camera, clean).render(VIEW[0], VIEW[1], fx.RGBF32, threads=THREADS).view(">f4").astype(f32)
    a.setflags(write=False)
    return a


def lattice(w=VIEW[0], h=VIEW[1]):
    ys, xs = np.mgrid[1:h:4, 0:w:3]
    return xs.ravel(), ys.ravel()


@functools.lru_cache(maxsize=None)
def probes(name, n, kind, camera, clean):
    xs, ys = lattice()
    a = oracle_scene(name, n, kind, camera, clean).colors_at(xs, ys, VIEW[0], VIEW[1])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def ray_colours(name, n, kind, camera, clean):
    """the oracle's colours of the camera's own rays through the lattice (rays as ray_color_cases.camera_rays: unnormalised)"""
    cam = cameras(name, n)[camera]
    xs, ys = lattice()
    d = rc.camera_rays(cam[1], xs, ys, VIEW[0], VIEW[1], FOV)
    o = np.ascontiguousarray(np.repeat(np.asarray(cam[0], f32)[None], len(d), axis=0))
    c = rc.CentrePixel(n, scene_flat(name, n, kind), params(name, n, kind), clean, False).colors(o, d)
    for a in (o, d, c):
        a.setflags(write=False)
    return o, d, c


@functools.lru_cache(maxsize=None)
def hit_records(name, n, kind, camera, clean, w=QUERY_VIEW[0], h=QUERY_VIEW[1]):
    """the oracle's primary-hit records of a view (high_dimension_cases.hit_records) and float64's of the same rays"""
    import high_dimension_cases as hd
    cam = cameras(name, n)[camera]
    flat = scene_flat(name, n, kind)
    rec = hd.hit_records(n, flat, cam[0], cam[1], FOV, w, h, clean, False)
    d = rec["d"].reshape(-1, n)
    bf = brute_force(flat, np.repeat(np.asarray(cam[0], f32)[None], len(d), axis=0), d)
    for a in rec.values():
        a.setflags(write=False)
    return rec, bf


CLEAN = {"NTRACER_CLEAN_NORMALS": "1"}
VAR = {"NTRACER_FORCE_VAR": "1"}
SWITCHES = ("NTRACER_STRICT_REFERENCE", "NTRACER_CLEAN_NORMALS", "NTRACER_FORCE_VAR", "NTRACER_COMPOSITE_KERNEL", "NTRACER_TWO_PASS",
            "NTRACER_NUMERATORS", "NTRACER_TILE_ORDER", "NTRACER_FRAME_MAJOR", "NTRACER_CHUNK_FRAMES")
CALLS = ("render", "colors_at", "ray_colors", "intersect", "occludes", "primary_hits", "lens", "parallel")


def route(name, n, kind, env, call):
    """The kernels a call on a scene of this module lands on -- every one has Solids, and a tree far shallower than the packet
    walk's 32 levels -- by composite_route (nt_api.cpp) and the launchers (launch_composite_fixed, launch_hits_fixed,
    launch_lens_fixed, launch_parallel_fixed, the query and ray launchers, and their run-time-n counterparts in nt_var.hip).
    kind: a parameter set of kinds(name), or a query variant ("default": the three materials).
    This is a restatement, as fixtures.COMPOSITE_ROUTES is: nothing at run time tells which kernel ran, so a change of the C++
    rule has to be followed here by hand -- test_solids_host.py only sees a launch or a call site that appears or disappears."""
    m = materials("transparent" if kind == "default" else kind)
    opaque, reflective = bool((m[:, 6] >= 1).all()), bool((m[:, 7] > 0).any())
    clean = env.get("NTRACER_CLEAN_NORMALS") == "1"
    var = n > 10 or env.get("NTRACER_FORCE_VAR") == "1"
    choice = int(env.get("NTRACER_COMPOSITE_KERNEL", "0"))
    faithful = not opaque or not clean
    alias = "false" if clean else "true"
    frames = params(name, n, kind)["max_reflect_depth"] + 1 if reflective and call not in ("intersect", "occludes", "primary_hits") else 1
    var_t = var or frames > 6
    packet_walk = not faithful and not var and choice == 0

    def rays():
        if faithful:
            return "rays_color_var_t<%s>" % alias if var_t else "rays_color_t<N,%s>" % alias
        return "rays_color_var" if var else "rays_color<N,true,true>"
    if call == "occludes":
        if opaque:
            return ("query_occluded_var",) if var else ("query_occluded<N,true>",)
        return ("query_occluded_var_t",) if var else ("query_occluded_t<N>",)
    if call == "intersect":
        if faithful:
            return ("query_closest_var_t<%s>" % alias,) if var else ("query_closest_t<N,%s>" % alias,)
        return ("query_closest_var",) if var else ("query_closest<N,true>",)
    if call == "primary_hits":
        if faithful:
            return ("hits_closest_var_t<%s>" % alias,) if var else ("hits_closest_t<N,%s>" % alias,)
        if var:
            return ("hits_closest_var",)
        return ("composite_packet<N,32,false,true,true>", "hits_normals<N,true>") if choice == 0 else ("hits_closest<N,true>",)
    if call == "ray_colors":
        return (rays(),)
    if call == "lens":
        return ("composite_packet<N,32,false,true,true,true>", "lens_shade<N,true,true>") if packet_walk else ("lens_expand", rays())
    if call == "parallel":
        return ("parallel_packet<N,32,true>", "parallel_shade<N,true,true>") if packet_walk else ("parallel_expand", rays())
    assert call in ("render", "colors_at"), call
    if faithful:
        return ("composite_kernel_var_t<%s>" % alias,) if var_t else ("composite_kernel_t<N,%s>" % alias,)
    if var:
        return ("composite_kernel_var",)
    if call == "render" and packet_walk and env.get("NTRACER_TWO_PASS", "1") != "0":
        return ("composite_packet<N,32,false,true>", "composite_kernel<N,true,false>")
    return ("composite_kernel<N,true,false>",)


# The functions that hold a call of solid_intersects, solid_intersects_marks (nt_composite.hpp, nt_parallel.hpp), solid_var or
# solid_marks_var (nt_var.hip), and the family of kernels whose leaf loops and normal passes they are.
SITES = {
    "leaf_closest": "fixed", "leaf_occludes": "fixed", "hit_normal": "fixed",
    "test_item": "fixed_t", "test_item_marks": "fixed_t<true>",
    "composite_packet": "packet", "parallel_packet": "parallel",
    "leaf_closest_var": "var", "leaf_occludes_var": "var", "composite_color_var": "var", "hit_normal_var": "var",
    "test_item_var": "var_t", "test_item_marks_var": "var_t<true>",
}


def family(kernel):
    """the family of SITES a kernel instantiation of ROUTES belongs to"""
    stem = kernel.split("<")[0]
    if stem in ("lens_expand", "parallel_expand"):
        return None                                         # (they make rays; the ray kernel behind them walks)
    if stem == "parallel_packet":
        return "parallel"
    if stem == "composite_packet":
        return "packet"
    var = stem.endswith("_var") or stem.endswith("_var_t")
    if stem.endswith("_t"):
        marks = kernel.endswith("true>") or stem in ("query_occluded_t", "query_occluded_var_t")
        base = "var_t" if var else "fixed_t"
        return base + "<true>" if marks and not stem.startswith("query_occluded") else base
    return "var" if var else "fixed"


def render_cases(name, n):
    """(kind, switches, camera) of every frame the GPU test renders of a scene at a dimension: every kind in both normal modes
    from the outside camera; from the two inside cameras the first kind in the default mode and, for field, the opaque `unlit` in
    the clean one (the packet walk at n <= 10); field's clean `lit` under each switch that changes its route; and the scenes of
    FORCED_VAR under NTRACER_FORCE_VAR"""
    out = []
    for kind in kinds(name):
        out += [(kind, {}, 0), (kind, CLEAN, 0)]
    for cam in (1, 2):
        out.append((kinds(name)[-1], {}, cam))
        if name == "field":
            out.append(("unlit", CLEAN, cam))
    if name == "field" and n <= 10:
        for extra in ({"NTRACER_TWO_PASS": "0"}, {"NTRACER_COMPOSITE_KERNEL": "1"}, {"NTRACER_COMPOSITE_KERNEL": "2"}):
            out.append(("lit", dict(CLEAN, **extra), 0))
    if (name, n) in FORCED_VAR:
        for kind in kinds(name):
            out += [(kind, VAR, 0), (kind, dict(CLEAN, **VAR), 0)]
    return out


def query_cases(name, n):
    """(variant, switches) of the query batches the GPU test sends"""
    out = []
    for variant in variants(name, n):
        out += [(variant, {}), (variant, CLEAN)]
        if (name, n) in FORCED_VAR:
            out += [(variant, VAR), (variant, dict(CLEAN, **VAR))]
    return out


def hits_cases(name, n):
    """(kind, switches, camera) of the primary-hit views"""
    kind = "unlit" if name in ("field", "nest") else kinds(name)[0]
    out = [(kind, {}, cam) for cam in (0, 1, 2)] + [(kind, CLEAN, cam) for cam in (0, 1, 2)]
    out += [(kinds(name)[-1], {}, 0), (kinds(name)[-1], CLEAN, 0)]
    if name == "field" and n <= 10:
        out.append((kind, dict(CLEAN, NTRACER_COMPOSITE_KERNEL="2"), 0))
    if (name, n) in FORCED_VAR:
        out += [(kind, VAR, 0), (kind, dict(CLEAN, **VAR), 0), (kinds(name)[-1], VAR, 0)]
    return out


PROJECTION_DIMS = (3, 6, 10, 17)        # field under a fisheye lens and under the parallel projection
PROJECTION_VIEW = (37, 29)
PARALLEL_HALF_WIDTH = 2.2


def projection_cases(n):
    return [("lit", CLEAN), ("lit", {}), ("transparent", CLEAN)] if n <= 10 else [("lit", CLEAN), ("lit", {})]


def reached():
    """{kernel: [(scene, n, kind, switches, call), ...]}: every kernel the calls of tests/test_solids_gpu.py land on"""
    out = {}

    def add(name, n, kind, env, call):
        for k in route(name, n, kind, env, call):
            out.setdefault(k, []).append((name, n, kind, tuple(sorted(env.items())), call))
    for name, n in scene_dims():
        for kind, env, cam in render_cases(name, n):
            for call in ("render", "colors_at", "ray_colors"):
                add(name, n, kind, env, call)
        for variant, env in query_cases(name, n):
            add(name, n, variant, env, "intersect")
            add(name, n, variant, env, "occludes")
        for kind, env, cam in hits_cases(name, n):
            add(name, n, kind, env, "primary_hits")
    for n in PROJECTION_DIMS:
        for kind, env in projection_cases(n):
            add("field", n, kind, env, "lens")
            add("field", n, kind, env, "parallel")
    return out


# The route table: every kernel instantiation whose leaf loops (or normal pass) can reach one of the four functions on a scene with
# Solids, through the calls tests/test_solids_gpu.py makes, with one of the cases that reach it (scene, n, kind, switches, call);
# tests/test_solids_host.py holds it against reached() and against the sources.  (`fixed` kernels with SCAL = false and
# composite_persistent never see a scene with Solids; the kernels of the adaptive, ambient-occlusion, outline, depth-cue and
# clip-plane settings -- OTHER_SUITES -- walk with the same leaf functions and are their own suites' to reach.)
ROUTES = [
    ("composite_kernel_t<N,true>", ("field", 5, "lit", {}, "render")),
    ("composite_kernel_t<N,false>", ("field", 5, "transparent", CLEAN, "render")),
    ("composite_packet<N,32,false,true>", ("field", 5, "lit", CLEAN, "render")),
    ("composite_kernel<N,true,false>", ("field", 5, "lit", dict(CLEAN, NTRACER_COMPOSITE_KERNEL="2"), "render")),
    ("composite_kernel_var_t<true>", ("field", 17, "lit", {}, "render")),
    ("composite_kernel_var_t<false>", ("nest", 64, "transparent", CLEAN, "render")),
    ("composite_kernel_var", ("field", 3, "lit", dict(CLEAN, **VAR), "render")),
    ("rays_color_t<N,true>", ("mirror", 7, "mirror", {}, "ray_colors")),
    ("rays_color_t<N,false>", ("pierced", 4, "transparent", CLEAN, "ray_colors")),
    ("rays_color<N,true,true>", ("field", 8, "unlit", CLEAN, "ray_colors")),
    ("rays_color_var_t<true>", ("pierced", 33, "lit", {}, "ray_colors")),
    ("rays_color_var_t<false>", ("field", 11, "transparent", CLEAN, "ray_colors")),
    ("rays_color_var", ("pierced", 10, "lit", dict(CLEAN, **VAR), "ray_colors")),
    ("query_closest_t<N,true>", ("field", 9, "default", {}, "intersect")),
    ("query_closest_t<N,false>", ("nest", 7, "default", CLEAN, "intersect")),
    ("query_closest<N,true>", ("nest", 4, "opaque", CLEAN, "intersect")),
    ("query_closest_var_t<true>", ("mirror", 11, "default", {}, "intersect")),
    ("query_closest_var_t<false>", ("field", 64, "default", CLEAN, "intersect")),
    ("query_closest_var", ("field", 64, "opaque", CLEAN, "intersect")),
    ("query_occluded_t<N>", ("field", 6, "default", {}, "occludes")),
    ("query_occluded<N,true>", ("nest", 10, "opaque", {}, "occludes")),
    ("query_occluded_var_t", ("field", 33, "default", {}, "occludes")),
    ("query_occluded_var", ("nest", 17, "opaque", {}, "occludes")),
    ("hits_closest_t<N,true>", ("field", 4, "unlit", {}, "primary_hits")),
    ("hits_closest_t<N,false>", ("field", 4, "transparent", CLEAN, "primary_hits")),
    ("composite_packet<N,32,false,true,true>", ("field", 7, "unlit", CLEAN, "primary_hits")),
    ("hits_normals<N,true>", ("field", 7, "unlit", CLEAN, "primary_hits")),
    ("hits_closest<N,true>", ("field", 7, "unlit", dict(CLEAN, NTRACER_COMPOSITE_KERNEL="2"), "primary_hits")),
    ("hits_closest_var_t<true>", ("field", 64, "unlit", {}, "primary_hits")),
    ("hits_closest_var_t<false>", ("field", 17, "transparent", CLEAN, "primary_hits")),
    ("hits_closest_var", ("field", 17, "unlit", CLEAN, "primary_hits")),
    ("composite_packet<N,32,false,true,true,true>", ("field", 6, "lit", CLEAN, "lens")),
    ("lens_shade<N,true,true>", ("field", 6, "lit", CLEAN, "lens")),
    ("lens_expand", ("field", 6, "lit", {}, "lens")),
    ("parallel_packet<N,32,true>", ("field", 6, "lit", CLEAN, "parallel")),
    ("parallel_shade<N,true,true>", ("field", 6, "lit", CLEAN, "parallel")),
    ("parallel_expand", ("field", 17, "lit", {}, "parallel")),
]
OTHER_ROWS = ("composite_kernel<N,true,true>",)        # the statistics launch: a row of fixtures.COMPOSITE_ROUTES
# kernels that walk with the same leaf functions under a setting this module does not turn on
OTHER_SUITES = ("refine_color", "refine_color_t", "refine_color_var", "refine_color_var_t", "ao_kernel", "clip_shade", "cue_shade",
                "cue_factors_fixed", "outline_shade", "outline_mark_fixed")


# ------------------------------------------------------------------ surfaces, for the bounds and the membership tests
def surface_points(flat, k, count, rng):
    """`count` points of Solid k's surface in float64: O (u + p), u on the unit sphere, or on the cube's boundary -- its vertices
    first, where a linear map's extremes are"""
    n, orient, _, pos = _solid_parts(flat)
    if int(flat["solid_types"][k]) == SPHERE:
        u = rng.standard_normal((count, n))
        u /= np.linalg.norm(u, axis=1)[:, None]
        # (the extreme of coordinate k is at u = O_k. / |O_k.|)
        rows = orient[k] / np.linalg.norm(orient[k], axis=1)[:, None]
        u[:2 * n] = np.concatenate([rows, -rows])[:min(2 * n, count)] if count >= 2 * n else u[:2 * n]
    else:
        u = rng.uniform(-1, 1, (count, n))
        half = count // 2
        u[:half] = np.where(rng.random((half, n)) < 0.5, -1.0, 1.0)                   # vertices
        face = rng.integers(0, n, count - half)
        u[np.arange(half, count), face] = np.where(rng.random(count - half) < 0.5, -1.0, 1.0)
        sg = np.sign(orient[k])
        sg[sg == 0] = 1.0
        ext = np.concatenate([sg, -sg])                                              # the vertex that is extreme in coordinate k
        m = min(len(ext), half)
        u[:m] = ext[:m]
    return (u + pos[k]) @ orient[k].T


def leaves(flat):
    """[(lo, hi, items)] of every leaf of the tree, the cells in float64"""
    axis, split, left, right = (np.asarray(flat[k]) for k in ("node_axis", "node_split", "node_left", "node_right"))
    out = []
    stack = [(int(flat["root"]), np.asarray(flat["aabb_start"], np.float64), np.asarray(flat["aabb_end"], np.float64))]
    while stack:
        node, lo, hi = stack.pop()
        if node < 0:
            continue
        if axis[node] < 0:
            out.append((lo, hi, [int(i) for i in np.asarray(flat["items"])[left[node]:left[node] + right[node]]]))
            continue
        a, s = int(axis[node]), float(split[node])
        lhi, rlo = hi.copy(), lo.copy()
        lhi[a], rlo[a] = s, s
        stack.append((int(left[node]), lo, lhi))
        stack.append((int(right[node]), rlo, hi))
    return out


if __name__ == "__main__":
    import sys
    import time
    worst = {}
    for name, n in scene_dims():
        for variant in variants(name, n):
            t = time.time()
            b = batches(name, n, variant)
            w = compare_with_float64(b, b.i_ref[False], "%s n=%d %s" % (name, n, variant), tolerance=(np.inf, np.inf))
            worst[n] = tuple(max(p, q) for p, q in zip(worst.get(n, (0.0, 0.0)), w))
            out = {k: "%d/%d" % (int((~b.brute.safe[s]).sum()), s.stop - s.start) for k, s in b.slices.items()}
            print("%-8s n=%-2d %-8s %5d rays, oracle vs float64 %.3g (near: %.3g ulps), inside the margin %s  (%.1f s)" % (name, n, variant, len(b.i_origins), w[0], w[1], out,
                                                                                                         time.time() - t))
            sys.stdout.flush()
    print("MEASURED = {%s}" % ", ".join("%d: (%.2g, %.3g)" % ((n,) + worst[n]) for n in sorted(worst)))
