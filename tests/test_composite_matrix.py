"""Every CompositeScene kernel route against the oracle at every fixed N = 3..10: the rows of fixtures.COMPOSITE_ROUTES (pinned
to launch_composite_fixed<N> and nt_launch_composite by tests/test_composite_routes.py) on scenes built here.

- lean: the N-orthoplex (its 2^N facets in closed form), batches only, built by build_composite_scene;
- mixed: the same tables with one batch's four triangles loose, plus a cube and a sphere, under a tree from the native builder;
- deep: hand-built combs of a chosen stack_depth (31, 32, 33, 40; 64 at N >= 8; 124 and 125 at N = 10), see comb_flat;
- checked: 31, 32 and 33 primitives at N = 3 and 10 (one, two and three words of the transparency kernels' `checked` lists).

Each row renders a ragged 97 x 61 RGBF32 frame into a padded host buffer seeded with a sentinel.  Its floats must be within
TOL_ORACLE of the oracle's on the same flat scene, parameters, normal mode and camera, and its bytes must equal every other
row's frame of the same scene, parameters, camera and normal mode.  The oracle renders each of those once.  At N = 6 and 9 a
three-frame nt_render_frames_device call (plain, in chunks of two frames, tiles before frames) must equal the single-frame
renders and a camera-table call, and leave every byte outside the pixels alone."""
import ctypes as C
import itertools

import numpy as np
import pytest

import fixtures as fx
import ntracer_amd
import oracle_binding as ob
import support as sup
from ntracer_amd import _lib, tracern
from ntracer_amd.render import CameraTable

pytestmark = pytest.mark.gpu

TOL_ORACLE = 1e-5
W, H = 97, 61
PAD = 36                    # bytes of pitch padding
SENTINEL = 0xA7
THREADS = 16                # the oracle's
FIXED_N = range(3, 11)
MATERIALS = np.array([[0.9, 0.35, 0.2, 1, 1, 1, 1, 0, 0.6, 12],
                      [0.25, 0.8, 0.4, 1, 1, 1, 1, 0, 0.3, 8],
                      [0.3, 0.45, 0.95, 1, 0.9, 0.8, 1, 0, 1.0, 30]], np.float32)


def _fmt(w=W, h=H, chans=fx.RGBF32, pad=PAD):
    bpp = sum(c[0] for c in chans) // 8
    return sup.fmt_of(w, h, chans, w * bpp + pad)


def _render(sc, **kw):
    """one frame into a sentinel-filled host buffer: (pixels as (H, W * 12) bytes, bytes written outside the pixels)"""
    fmt = _fmt()
    buf = bytearray([SENTINEL]) * (fmt.pitch * H)
    assert ntracer_amd.BlockingRenderer().render(buf, fmt, sc, **kw)
    a = np.frombuffer(bytes(buf), np.uint8).reshape(H, fmt.pitch)
    return a[:, :W * 12].copy(), int((a[:, W * 12:] != SENTINEL).sum())


# ------------------------------------------------------------------ scenes

def camera(n):
    """seeded, off-axis: every coordinate of every ray direction non-zero"""
    rng = np.random.default_rng(7100 + n)
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    q = np.ascontiguousarray(q, np.float32)
    o = (-3.2 * q[2] + 0.15 * q[0] - 0.1 * q[1]).astype(np.float32)
    return o, q


def params(n, kind):
    p = dict(fov=0.8, shadows=0, camera_light=1, max_reflect_depth=4, bg_gradient_axis=1, ambient=[.02, .02, .03],
             bg1=[1, 1, 1], bg2=[0, 0, 0], bg3=[0, 1, 1], point_light_pos=np.zeros((0, n), np.float32),
             point_light_color=np.zeros((0, 3), np.float32), global_light_dir=np.zeros((0, n), np.float32),
             global_light_color=np.zeros((0, 3), np.float32))
    if kind != "unlit":
        pl = np.zeros((1, n), np.float32)
        pl[0, :3] = (2.5, 3.0, -4.0)
        gl = np.full((1, n), 0.1, np.float32)
        gl[0, :3] = (0.2, -0.9, 0.3)
        p.update(shadows=1, point_light_pos=pl, point_light_color=np.array([[30.0, 27.0, 24.0]], np.float32),
                 global_light_dir=gl, global_light_color=np.array([[.4, .4, .5]], np.float32))
    if kind == "reflective":
        p["max_reflect_depth"] = 2
    if kind == "transparent_reflective":
        p["max_reflect_depth"] = 6
    return p


def materials(table, kind):
    m = np.array(table, np.float32).copy()
    if kind == "reflective":
        m[:, 7] = 0.3
    if kind in ("transparent", "transparent_reflective"):
        m[0::2, 6] = 0.5                          # some materials
    if kind == "transparent_reflective":
        m[1:, 7] = 0.3
    return m


def orthoplex_facets(n):
    """the simplices on (s_0 e_0, ..., s_{N-1} e_{N-1}) for every sign vector s: (2^N, N points, N)"""
    signs = np.array(list(itertools.product((-1.0, 1.0), repeat=n)), np.float32)
    return signs[:, :, None] * np.eye(n, dtype=np.float32)[None]


def _mats():
    return [ntracer_amd.Material(tuple(r[:3]), 1, 0, float(r[8]), float(r[9]), tuple(r[3:6])) for r in MATERIALS]


def lean_flat(n, facets=None):
    """the N-orthoplex (or `facets`) in batches, facet i of material i mod 3, through build_composite_scene"""
    mats = _mats()
    facets = orthoplex_facets(n) if facets is None else facets
    protos = [tracern.TrianglePrototype([list(p) for p in f], mats[i % 3]) for i, f in enumerate(facets)]
    flat = tracern.build_composite_scene(protos)._flat_description()
    assert len(flat["tri_recs"]) == 0 and len(flat["solid_recs"]) == 0 and len(flat["batch_recs"]) * 4 == len(facets)
    # (materials are interned in the order of first use: renumber them to MATERIALS' order)
    got = np.asarray(flat["materials"], np.float32)
    perm = np.array([int(np.nonzero((MATERIALS == r).all(axis=1))[0][0]) for r in got], np.int32)
    flat["batch_mats"] = perm[np.asarray(flat["batch_mats"], np.int32)]
    flat["materials"] = MATERIALS.copy()
    return flat


def _tables_tree(n, flat, keep_batches, loose, solids):
    """a scene over chosen tables with the native builder's tree: `keep_batches` of flat's batches, the triangles `loose`
    [(batch, lane)] of its batches as loose triangles, `solids` [(type, position, orientation, material index)]"""
    rl = n * n + n + 1
    brec = np.asarray(flat["batch_recs"], np.float32).reshape(-1, 4, rl)
    bmat = np.asarray(flat["batch_mats"], np.int32).reshape(-1, 4)
    d = {k: np.array(v) for k, v in flat.items()}
    d["batch_recs"], d["batch_mats"] = brec[keep_batches], bmat[keep_batches]
    d["tri_recs"] = np.asarray([brec[b, l] for b, l in loose], np.float32).reshape(-1, rl)
    d["tri_mats"] = np.asarray([bmat[b, l] for b, l in loose], np.int32)
    srec, stype, smat = [], [], []
    for typ, pos, orient, mi in solids:
        s = tracern.Solid(typ, pos, tracern.Matrix(n, orient), _mats()[mi])
        srec.append(np.concatenate([s.orientation._m.ravel(), s.inv_orientation._m.ravel(), s.position._v]))
        stype.append(typ)
        smat.append(mi)
    d["solid_recs"] = np.asarray(srec, np.float32).reshape(-1, 2 * n * n + n)
    d["solid_types"] = np.asarray(stype, np.int32)
    d["solid_mats"] = np.asarray(smat, np.int32)
    items = ([(k << 2) | _lib.KIND_BATCH for k in range(len(d["batch_recs"]))] + [(k << 2) | _lib.KIND_TRIANGLE for k in range(len(d["tri_recs"]))]
             + [(k << 2) | _lib.KIND_SOLID for k in range(len(srec))])
    d.update(root=0, node_axis=np.array([-1], np.int32), node_split=np.zeros(1, np.float32), node_left=np.array([0], np.int32),
             node_right=np.array([len(items)], np.int32), items=np.asarray(items, np.int32),
             aabb_start=np.full(n, -4, np.float32), aabb_end=np.full(n, 4, np.float32))
    return tracern.CompositeScene.from_flat(n, d).with_rebuilt_tree()._flat_description()


def mixed_flat(n, lean):
    _, q = camera(n)
    nb = len(lean["batch_recs"])
    rng = np.random.default_rng(7200 + n)
    rot, _ = np.linalg.qr(rng.standard_normal((n, n)))
    solids = [(tracern.CUBE, 0.7 * q[0] + 0.35 * q[1] - 0.55 * q[2], 0.22 * rot, 1),
              (tracern.SPHERE, -0.65 * q[0] - 0.3 * q[1] - 0.5 * q[2], 0.25 * np.eye(n), 2)]
    return _tables_tree(n, lean, list(range(1, nb)), [(0, lane) for lane in range(4)], solids)


def subdivided_octahedron():
    """the octahedron's facets cut in four twice: 128 triangles"""
    tris = [f.astype(np.float64) for f in orthoplex_facets(3)]
    for _ in range(2):
        nxt = []
        for a, b, c in tris:
            ab, bc, ca = (a + b) / 2, (b + c) / 2, (c + a) / 2
            nxt += [np.array(t) for t in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))]
        tris = nxt
    return np.asarray(tris, np.float32)


def checked_flat(n, prims):
    """`prims` primitives: prims - 2 batches and two loose triangles of a chopped orthoplex (N = 3: subdivided)"""
    flat = lean_flat(n, subdivided_octahedron() if n == 3 else None)
    nb = len(flat["batch_recs"])
    assert nb >= prims - 1
    return _tables_tree(n, flat, list(range(prims - 2)), [(prims - 2, 0), (prims - 2, 2)], [])


def comb_flat(n, stack_depth, mirrored=False):
    """A k-d tree of `stack_depth` (nodes on its longest path + 1) that makes a walk push at every level.

    K = stack_depth - 2 splits on axis 2, the axis the camera looks along, cut the slab 0 <= z <= 1 into K + 1 cells.  The
    camera (comb_camera) is at z = -1.  The chain of branches runs down the near (camera) side; every branch's far child is a
    leaf, the cell between its split and its parent's, so a primary ray pushes K entries, the deepest last.  Each cell holds one
    batch of four small simplices flat in the plane through its middle, facing the camera and apart from each other on the
    screen (32 tile positions; a cell 32 further away hides behind).  Each leaf lists exactly the batch in its own cell, so a
    dropped push leaves that batch out of the frame and the frame shows what is behind it.  `mirrored`: z -> 1 - z, the camera
    at z = 2 looking down: the chain runs down right children, near = right."""
    K = stack_depth - 2
    cells = K + 1
    zb = np.linspace(0.0, 1.0, cells + 1).astype(np.float32)
    rl = n * n + n + 1
    recs, mats = [], []
    mats_obj = _mats()
    for c in range(cells):
        zc = float(zb[c] + zb[c + 1]) / 2
        d = zc + 1.0
        tx, ty = (c % 32) % 8, (c % 32) // 8
        batch, bm = [], []
        for qx, qy in ((0, 0), (1, 0), (0, 1), (1, 1)):
            ax0 = -0.4 + 0.1 * tx + 0.05 * qx + 0.003
            ay0 = -0.25 + 0.125 * ty + 0.0625 * qy + 0.003
            leg = 0.044 * d
            v0 = np.zeros(n)
            v0[0], v0[1], v0[2] = ax0 * d, ay0 * d, zc
            v0[3:] = -0.02 * leg
            pts = [v0] + [v0 + leg * np.eye(n)[i] for i in range(n) if i != 2]
            if mirrored:
                for p in pts:
                    p[2] = 1.0 - p[2]
            mi = (c + qx + 2 * qy) % 3
            batch.append(tracern.Triangle.from_points([list(p) for p in pts], mats_obj[mi])._record())
            bm.append(mi)
        recs.append(batch)
        mats.append(bm)
    axis, split, left, right, items = [], [], [], [], []

    def leaf(c):
        axis.append(-1), split.append(0.0), left.append(len(items)), right.append(1)
        items.append((c << 2) | _lib.KIND_BATCH)
        return len(axis) - 1

    def branch(s, near, far):
        axis.append(2), split.append(s)
        if mirrored:
            left.append(far), right.append(near)
        else:
            left.append(near), right.append(far)
        return len(axis) - 1

    # built from the deepest branch up: branch j (1 = root) splits at zb[K + 1 - j]; its far child holds cell K + 1 - j
    node = leaf(0)
    for j in range(K, 0, -1):
        s = float(zb[K + 1 - j])
        node = branch(1.0 - s if mirrored else s, node, leaf(K + 1 - j))
    lo = np.full(n, -1.0, np.float32)
    hi = np.full(n, 1.0, np.float32)
    lo[2], hi[2] = 0.0, 1.0
    lo[3:], hi[3:] = -0.01, 0.2
    return dict(root=node, node_axis=np.asarray(axis, np.int32), node_split=np.asarray(split, np.float32),
                node_left=np.asarray(left, np.int32), node_right=np.asarray(right, np.int32), items=np.asarray(items, np.int32),
                batch_recs=np.asarray(recs, np.float32).reshape(-1, 4, rl), batch_mats=np.asarray(mats, np.int32),
                tri_recs=np.zeros((0, rl), np.float32), tri_mats=np.zeros(0, np.int32),
                solid_recs=np.zeros((0, 2 * n * n + n), np.float32), solid_types=np.zeros(0, np.int32),
                solid_mats=np.zeros(0, np.int32), materials=MATERIALS.copy(), aabb_start=lo, aabb_end=hi)


def comb_camera(n, mirrored=False):
    o = np.zeros(n, np.float32)
    a = np.eye(n, dtype=np.float32)
    o[2] = 2.0 if mirrored else -1.0
    if mirrored:
        a[2, 2] = -1.0
    return o, a


# ------------------------------------------------------------------ checks

_flats = {}
_oracle = {}


def flat_of(n, scene):
    if (n, scene) not in _flats:
        if not any(k[0] == n for k in _flats):
            _flats.clear()
            _oracle.clear()
        if scene == "lean":
            _flats[n, scene] = lean_flat(n)
        elif scene == "mixed":
            _flats[n, scene] = mixed_flat(n, flat_of(n, "lean"))
        else:
            raise KeyError(scene)
    return _flats[n, scene]


def _scene_flat(flat, kind):
    f = {k: np.array(v) for k, v in flat.items()}
    f["materials"] = materials(flat["materials"], kind)
    f["batch_size"] = 4
    return f


def _oracle_scene(n, key, flat, p, cam, clean):
    k = (n, key, clean)
    if k not in _oracle:
        _oracle[k] = ob.OracleScene(n, cam[0], cam[1], fov=p["fov"], flat=flat, params=p, clean_normals=clean)
    return _oracle[k]


def _oracle_frame(n, key, flat, p, cam, clean):
    k = (n, key, clean, "frame")
    if k not in _oracle:
        _oracle[k] = _oracle_scene(n, key, flat, p, cam, clean).render(W, H, fx.RGBF32, threads=THREADS).view(">f4")
    return _oracle[k]


def _lattice():
    ys, xs = np.mgrid[0:H:4, 0:W:3]
    return xs.ravel(), ys.ravel()


SWITCHES = sorted({k for _, ways in fx.COMPOSITE_ROUTES for _, _, env, _ in ways for k in env} |
                  {k for env in fx.COMPOSITE_FRAME_ENVS for k in env})


def _clear_switches(mp):
    sup.set_switches(mp, SWITCHES, {})


def run_way(n, scene_key, flat, kind, env, mode, cam, groups, failures, label):
    """one (scene, parameters, switches, mode) with the switches set before the scene is made"""
    clean = env.get("NTRACER_CLEAN_NORMALS") == "1"
    p = params(n, kind)
    f = _scene_flat(flat, kind)
    with pytest.MonkeyPatch.context() as mp:
        _clear_switches(mp)
        for k, v in env.items():
            mp.setenv(k, v)
        sc = tracern.CompositeScene.from_flat(n, f)
        sc.set_params_flat(p)
        sc._set_camera_arrays(cam[0], cam[1])
        if mode == "colors_at":
            xs, ys = _lattice()
            got = sc.colors_at(xs, ys, W, H)
            ref = _oracle_scene(n, (scene_key, kind), f, p, cam, clean).colors_at(xs, ys, W, H)
            d = float(np.abs(got - ref).max())
            if not d < TOL_ORACLE:
                failures.append("%s: colors_at differs from the oracle by %g" % (label, d))
            return
        img, stray = _render(sc, collect_stats=(mode == "stats"))
        if stray:
            failures.append("%s: %d bytes of pitch padding written" % (label, stray))
        if mode == "stats":
            st = sc.last_stats()
            if scene_key == "lean" and st["rays"] != W * H or st["rays"] < W * H:
                failures.append("%s: %d rays counted" % (label, st["rays"]))
    ref = _oracle_frame(n, (scene_key, kind), f, p, cam, clean)
    d = np.abs(img.view(">f4").reshape(ref.shape) - ref)
    if not d.max() < TOL_ORACLE:
        ys, xs = np.nonzero(d.reshape(H, -1) >= TOL_ORACLE)
        failures.append("%s: %d floats differ from the oracle (max %g), first at x=%d y=%d"
                        % (label, len(ys), float(d.max()), xs[0] // 3, ys[0]))
    groups.setdefault((scene_key, kind, clean), []).append((label, img))


def check_groups(groups, failures):
    for key, frames in groups.items():
        label0, img0 = frames[0]
        for label, img in frames[1:]:
            if not np.array_equal(img, img0):
                failures.append("%s and %s: frames differ in %d bytes" % (label0, label, int((img != img0).sum())))


def _env_label(env):
    return ",".join("%s=%s" % (k[len("NTRACER_"):], v) for k, v in sorted(env.items())) or "default"


@pytest.mark.parametrize("n", FIXED_N)
def test_composite_routes_equal_the_oracle(n):
    """every row of fixtures.COMPOSITE_ROUTES on the lean and mixed scenes"""
    cam = camera(n)
    groups, failures = {}, []
    for scene_key, kind, env, mode in fx.composite_route_ways():
        if scene_key == "deep":
            continue
        label = "n=%d %s/%s %s %s" % (n, scene_key, kind, _env_label(env), mode)
        run_way(n, scene_key, flat_of(n, scene_key), kind, env, mode, cam, groups, failures, label)
    check_groups(groups, failures)
    # the frames are not trivial: most of the lattice's rays hit the polytope, some miss it
    xs, ys = _lattice()
    _, cnt = _oracle_scene(n, ("lean", "unlit"), None, None, cam, False).colors_at(xs, ys, W, H, counters=True)
    assert 0.1 * len(xs) < cnt["hits"] < len(xs), cnt
    assert not failures, "\n".join(failures)


def _deep_depths(n):
    d = list(fx.COMPOSITE_DEEP_DEPTHS)
    if n >= 8:
        d += list(fx.COMPOSITE_DEEP_DEPTHS_WIDE)
    if n == 10:
        d.append(fx.COMPOSITE_MAX_DEPTH_N10)
    return d


@pytest.mark.parametrize("n", FIXED_N)
def test_deep_trees_equal_the_oracle(n):
    """the deep rows of fixtures.COMPOSITE_ROUTES on comb_flat trees of stack_depth 31, 32, 33, 40 (64 at N >= 8, 124 at
    N = 10), both combs; the lean frames through the packet (or, past 32, the persistent), persistent and per-lane kernels
    are compared byte for byte"""
    ways = [(kind, env) for scene_key, kind, env, mode in fx.composite_route_ways() if scene_key == "deep"]
    failures = []
    for sd in _deep_depths(n):
        for mirrored in (False, True):
            flat = comb_flat(n, sd, mirrored)
            cam = comb_camera(n, mirrored)
            groups = {}
            key = "deep%d%s" % (sd, "m" if mirrored else "")
            for kind, env in ways:
                label = "n=%d stack_depth %d%s %s %s" % (n, sd, " mirrored" if mirrored else "", kind, _env_label(env))
                run_way(n, key, flat, kind, env, "render", cam, groups, failures, label)
            check_groups(groups, failures)
            # every primary ray crosses every split inside the box: the walk pushes stack_depth - 2 entries
            _, cnt = _oracle_scene(n, (key, "unlit"), _scene_flat(flat, "unlit"), params(n, "unlit"), cam, False).colors_at(
                [W // 2], [H // 2], W, H, counters=True)
            assert cnt["branches"] == sd - 2, (n, sd, cnt)
    assert not failures, "\n".join(failures)


def test_deepest_tree_that_fits_and_one_deeper_at_n10():
    """N = 10: stack_depth 124 takes exactly 160 KiB of LDS and renders (test_deep_trees_equal_the_oracle); 125 is refused
    before anything is launched, on every route, and leaves the scene unlocked"""
    n = 10
    flat = comb_flat(n, fx.COMPOSITE_MAX_DEPTH_N10 + 1)
    cam = comb_camera(n)
    for kind, env in (("unlit", {}), ("unlit", {"NTRACER_COMPOSITE_KERNEL": "2"}), ("lit", {}), ("transparent", {})):
        with pytest.MonkeyPatch.context() as mp:
            _clear_switches(mp)
            for k, v in env.items():
                mp.setenv(k, v)
            sc = tracern.CompositeScene.from_flat(n, _scene_flat(flat, kind))
            sc.set_params_flat(params(n, kind))
            sc._set_camera_arrays(cam[0], cam[1])
            fmt = _fmt()
            buf = bytearray([SENTINEL]) * (fmt.pitch * H)
            with pytest.raises(RuntimeError, match=r"k-d tree too deep for the LDS traversal stack \(depth 125\)"):
                ntracer_amd.BlockingRenderer().render(buf, fmt, sc)
            assert not sc.locked, (kind, env)
            assert buf == bytearray([SENTINEL]) * (fmt.pitch * H), (kind, env)


@pytest.mark.parametrize("prims", (31, 32, 33))
@pytest.mark.parametrize("n", (3, 10))
def test_transparency_kernels_at_checked_word_boundaries(n, prims):
    """31, 32 and 33 primitives: one, two and three words of the `checked` bitmap, default and clean normal modes"""
    flat = checked_flat(n, prims)
    assert len(flat["batch_recs"]) + len(flat["tri_recs"]) + len(flat["solid_recs"]) == prims
    cam = camera(n)
    groups, failures = {}, []
    for env in ({}, {"NTRACER_CLEAN_NORMALS": "1"}):
        for mode in ("render", "colors_at"):
            label = "n=%d %d primitives transparent %s %s" % (n, prims, _env_label(env), mode)
            run_way(n, "checked%d" % prims, flat, "transparent", env, mode, cam, groups, failures, label)
    assert not failures, "\n".join(failures)


FRAME_PAD = 64
FRAME_TAIL = 256
GUARD = 4096


@pytest.mark.parametrize("kind", ("unlit", "lit"))
@pytest.mark.parametrize("n", (6, 9))
def test_three_frame_launches_equal_single_frames_and_the_camera_table(n, kind):
    """nt_render_frames_device with three cameras: plainly, in chunks of two frames (NTRACER_CHUNK_FRAMES=2) and with the
    packet kernel's tiles before its frames (NTRACER_FRAME_MAJOR=0).  Each frame equals the single-frame render of its camera,
    the whole call equals one through a four-camera table (first = 1, count = 3), and nothing outside the pixels is written."""
    import torch
    flat = _scene_flat(flat_of(n, "lean"), kind)
    p = params(n, kind)
    o0, a0 = camera(n)
    rng = np.random.default_rng(7300 + n)
    cams = [(o0, a0)]
    for k in range(3):
        q, _ = np.linalg.qr((a0 + 0.2 * rng.standard_normal((n, n))).T)
        q = np.ascontiguousarray(q.T, np.float32)
        cams.append(((-3.0 * q[2] + 0.1 * k * q[0]).astype(np.float32), q))
    so = np.ascontiguousarray(np.stack([c[0] for c in cams]), np.float32)
    sa = np.ascontiguousarray(np.stack([c[1] for c in cams]), np.float32)
    fo, fa = np.ascontiguousarray(so[1:]), np.ascontiguousarray(sa[1:])
    fmt = _fmt(pad=FRAME_PAD)
    fst = fmt._as_struct()
    frame_bytes = H * fmt.pitch + FRAME_TAIL
    failures = []
    single = []
    with pytest.MonkeyPatch.context() as mp:
        _clear_switches(mp)
        sc = tracern.CompositeScene.from_flat(n, flat)
        sc.set_params_flat(p)
        for o, a in cams[1:]:
            sc._set_camera_arrays(o, a)
            single.append(_render(sc)[0])
            ref = ob.OracleScene(n, o, a, fov=p["fov"], flat=flat, params=p).render(W, H, fx.RGBF32, threads=THREADS).view(">f4")
            assert np.abs(single[-1].view(">f4").reshape(ref.shape) - ref).max() < TOL_ORACLE
    calls = {}
    for env in fx.COMPOSITE_FRAME_ENVS:
        with pytest.MonkeyPatch.context() as mp:
            _clear_switches(mp)
            for k, v in env.items():
                mp.setenv(k, v)
            sc = tracern.CompositeScene.from_flat(n, flat)
            sc.set_params_flat(p)
            for entry in ("frames", "table"):
                if entry == "table" and env:
                    continue
                buf = torch.full((GUARD + 3 * frame_bytes + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
                dest = buf[GUARD:GUARD + 3 * frame_bytes]
                stream = torch.cuda.current_stream().cuda_stream
                if entry == "frames":
                    _lib.check(_lib.lib().nt_render_frames_device(sc._handle, C.c_void_p(dest.data_ptr()), frame_bytes, 3,
                                                                  fo.ctypes.data_as(_lib.f32p), fa.ctypes.data_as(_lib.f32p),
                                                                  C.byref(fst), None, C.c_void_p(stream)))
                else:
                    table = CameraTable(n, so, sa)
                    assert table.render(sc, dest, fmt, frame_bytes=frame_bytes, first=1, count=3)
                torch.cuda.synchronize()
                got = buf.cpu().numpy()
                label = "n=%d %s %s %s" % (n, kind, _env_label(env), entry)
                calls[label] = got
                frames = got[GUARD:GUARD + 3 * frame_bytes].reshape(3, frame_bytes)
                for f in range(3):
                    pix = frames[f, :H * fmt.pitch].reshape(H, fmt.pitch)
                    if not np.array_equal(pix[:, :W * 12], single[f]):
                        failures.append("%s: frame %d differs from its single-frame render" % (label, f))
                    pix[:, :W * 12] = SENTINEL
                stray = int((got != SENTINEL).sum())
                if stray:
                    failures.append("%s: %d bytes written outside the pixels" % (label, stray))
    labels = list(calls)
    for label in labels[1:]:
        if not np.array_equal(calls[label], calls[labels[0]]):
            failures.append("%s and %s differ" % (labels[0], label))
    assert len(calls) == 4
    assert not failures, "\n".join(failures)
